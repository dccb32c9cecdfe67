"""Memory-footprint audit of the feature kernels (tests/footprint.py): every entry point of sample.hip, intensity.hip,
crop_label.hip, resample.hip, spline.hip, edt.hip, postprocess.hip, head.hip, the second loss family, the fused optimiser
family, ema_step, ssl.hip, wsl.hip, nll.hip and cl.hip runs on operands placed in an arena - exact sizes, 64 KiB guard bands,
outputs and workspaces pre-filled - under two fill bytes and at two placements.  No value is judged here except by
bit-equality between runs of the device itself; what the kernels compute is the business of the families' oracle tests.

AUDITED is the set of symbols the cases below list (and must launch); COVERED_ELSEWHERE names, for every other pointer-taking
prototype of include/fplx.h, the existing test file that already poisons around it (or, for the host-only entry points, calls
it).  tests/test_footprint_cpu.py holds the two tables against the header.

The callables run only shipped kernels on valid arguments.  Operands the header requires to be aligned keep their alignment at
the second placement (P(..., aligned=True)); that the library refuses them misaligned is asserted at the end of this file.
"""
import ctypes
import functools
import zlib

import numpy as np
import pytest
import torch

import footprint as fp
import streamorder

F32, F64, U8, I32, BF = torch.float32, torch.float64, torch.uint8, torch.int32, torch.bfloat16
CAPACITY = 96 << 20

CASES = []


def case(id, symbols, pointwise=False, unguarded=()):
    def deco(run):
        CASES.append(fp.Case(id, ["fplx_" + s for s in symbols], run, pointwise=pointwise, unguarded=unguarded))
        return run
    return deco


def _ops():
    from fplx import ops
    return ops


def _lib():
    from fplx import _lib as L
    return L.lib()


def rng(name):
    return np.random.Generator(np.random.Philox(key=zlib.crc32(name.encode()) + 0xF007))


# the generators are pure functions of their arguments and cached: a case runs four times.  Nothing may write into what they return.
@functools.lru_cache(None)
def normal(name, shape, scale=1.0, shift=0.0):
    import detdata
    return detdata.normal("fp." + name, shape, scale, shift)


@functools.lru_cache(None)
def uniform(name, shape, lo=0.0, hi=1.0):
    import detdata
    return detdata.uniform("fp." + name, shape, lo, hi)


@functools.lru_cache(None)
def labels(name, shape, top):
    """uint8 labels 0..top"""
    return rng(name).integers(0, top + 1, size=tuple(shape)).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------- documented sizes (S)
def _rows(v):
    return _lib().fplx_loss_rows(int(v))


def _vps(a):
    return a["voxels_per_sample"]


DOCUMENTED = {
    ("fplx_normalize_mean_std", "ws"): lambda a: _lib().fplx_normalize_ws_bytes(),
    ("fplx_normalize_positive", "ws"): lambda a: _lib().fplx_normalize_ws_bytes(),
    ("fplx_normalize_range", "ws"): lambda a: _lib().fplx_normalize_ws_bytes(),
    ("fplx_channel_minmax", "ws"): lambda a: 16,
    ("fplx_select_kth", "ws"): lambda a: _lib().fplx_select_ws_bytes(),
    ("fplx_edt_squared", "ws"): lambda a: 2 * a["n"] * a["d"] * a["h"] * a["w"] * 4,                  # FPLX_EDT_WS_BYTES
    ("fplx_cc_label", "ws"): lambda a: 320 * 4,                                                       # FPLX_CC_LABEL_WS_BYTES
    ("fplx_keep_largest_component", "ws"): lambda a: (320 + 2 * a["d"] * a["h"] * a["w"]) * 4,        # FPLX_KLC_WS_BYTES
    ("fplx_head_wgrad", "ws"): lambda a: _lib().fplx_head_wgrad_ws_bytes(a["n"], a["v"], a["c"], a["ncls"]),
    ("fplx_seg_loss_ext_fwd", "part"): lambda a: a["n"] * _rows(_vps(a)) * (10 * a["c"] + 7) * 4,
    ("fplx_seg_loss_ext_sums", "part"): lambda a: a["n"] * _rows(_vps(a)) * (10 * a["c"] + 7) * 4,
    ("fplx_ssl_consistency_fwd", "part"): lambda a: a["n"] * _rows(_vps(a)) * 2 * 4,
    ("fplx_ssl_entropy_fwd", "part"): lambda a: a["n"] * _rows(_vps(a)) * 4,
    ("fplx_ssl_pyramid_fwd", "part"): lambda a: a["n"] * _rows(_vps(a)) * 3 * a["k"] * 4,
    ("fplx_wsl_gatedcrf_fwd", "part"): lambda a: a["n"] * a["d"] * ((a["h"] + 15) // 16) * ((a["w"] + 15) // 16) * 4,
    ("fplx_wsl_tv_fwd", "ws"): lambda a: 12 * a["n"] * a["c"] * a["d"] * a["h"] * a["w"],
    ("fplx_wsl_tv_fwd", "part"): lambda a: a["n"] * a["c"] * _rows(a["d"] * a["h"] * a["w"]) * 4,
    ("fplx_wsl_mumford_shah_fwd", "part"): lambda a: a["n"] * a["d"] * _rows(a["h"] * a["w"]) * a["c"] * (1 + a["ci"]) * 4,
    ("fplx_nll_voxel_ce_fwd", "part"): lambda a: a["k"] * a["n"] * _lib().fplx_nll_ce_rows(_vps(a)) * 4,
    ("fplx_nll_select_mask", "ws"): lambda a: _lib().fplx_nll_mask_ws_bytes(),
    ("fplx_nll_select_fwd", "ws"): lambda a: _lib().fplx_nll_select_ws_bytes(),
    ("fplx_cl_class_stats", "ws"): lambda a: _lib().fplx_cl_stats_ws_bytes(),
}


@functools.lru_cache(None)
def target():
    from fplx import _lib as L, ops
    return fp.Target(ops, streamorder.parse_prototypes(L.HEADER), DOCUMENTED, "cuda")


# ======================================================================================================== pointwise over n
NS = (1, 3, 4, 5, 15, 16, 17, 63, 257, 1021, 4099)
IT_CAP = 1024 * 256 + 257           # intensity.hip: IT_MAX_BLOCKS x IT_THREADS, one element per lane and trip
SP_CAP = 2048 * 256 + 257           # sample.hip sp_grid / crop_label.hip cl_grid: 2048 blocks x 256
CS = (1, 3, 255)


@functools.lru_cache(None)
def _intensity(n):
    x = normal("it.x.%d" % n, (n,), 40.0, 10.0).copy()
    if n > 4:
        x[n // 2] = np.nan
    return x


def _pointwise_intensity(n):
    tag = "n%d" % n
    X, NOISE = (lambda: _intensity(n)), (lambda: normal("it.noise.%d" % n, (n,)))

    @case("clip_affine-" + tag, ["clip_affine"], pointwise=True)
    def _(P):
        xs = P(X())
        return _ops().clip_affine(P(X()), -20.0, 55.0, 3.0, 7.0), _ops().clip_affine(xs, -20.0, 55.0, 3.0, 7.0, out=xs)   # y may alias x

    @case("clip_affine_dev-" + tag, ["clip_affine_dev"], pointwise=True)
    def _(P):
        one = lambda v: P(np.array([v], np.float32))
        return _ops().clip_affine_dev(P(X()), one(-20.0), one(55.0), one(-20.0), one(55.0))

    @case("threshold_replace-" + tag, ["threshold_replace"], pointwise=True)
    def _(P):
        return _ops().threshold_replace(P(X()), -5.0, -7.0, 40.0, 41.0), _ops().threshold_replace(P(X()), None, 0, 40.0, 41.0)

    @case("normalize_range-" + tag, ["normalize_range"])
    def _(P):
        o = _ops()
        return (o.normalize_range(P(X()), P(NOISE()), -20.0, 60.0, want_moments=True), o.normalize_range(P(X()), P(NOISE()), None, 30.0))

    @case("gamma-" + tag, ["gamma"], pointwise=True)
    def _(P):
        xx = uniform("it.g.%d" % n, (n,), 1.0, 9.0)
        return _ops().gamma_correct(P(xx), P(np.array([1.0], np.float32)), P(np.array([9.0], np.float32)), 1.7)

    @case("add_noise_f64-" + tag, ["add_noise_f64"], pointwise=True)
    def _(P):
        return _ops().add_noise_f64(P(X()), P(NOISE().astype(np.float64) * 3.0))

    @case("add_noise_philox-" + tag, ["add_noise_philox"], pointwise=True)
    def _(P):
        o = _ops()
        return o.add_noise_philox(P(X()), 0x1234567890ABCDEF, 7, 0.5, 2.0, want_uniforms=True), o.add_noise_philox(P(X()), 3, 1, 0.0, 1.0)


def _pointwise_sample(n):
    tag = "n%d" % n
    X, NOISE = (lambda: normal("sp.x.%d" % n, (n,), 30.0, 5.0)), (lambda: normal("sp.noise.%d" % n, (n,)))

    @case("normalize_mean_std-given-" + tag, ["normalize_mean_std"], pointwise=True, unguarded=("mean_std",))
    def _(P):
        return _ops().normalize_mean_std(P(X()), (4.5, 31.0), want_moments=True)

    @case("normalize_mean_std-computed-" + tag, ["normalize_mean_std"])
    def _(P):
        return _ops().normalize_mean_std(P(X()), None, want_moments=True), _ops().normalize_mean_std(P(X()))

    @case("normalize_positive-" + tag, ["normalize_positive"])
    def _(P):
        o = _ops()
        xs = P(X())
        return o.normalize_positive(P(X()), P(NOISE()), want_moments=True), o.normalize_positive(xs, P(NOISE()), out=xs)      # y = x

    @case("set_weight-" + tag, ["set_weight"], pointwise=True)
    def _(P):
        pw = (uniform("sp.pw.%d" % n, (n,)) > 0.4).astype(np.float32) * np.float32(1.0)
        return _ops().set_weight_(P(pw), 0.73)

    @case("pixel_weight-" + tag, ["pixel_weight"], pointwise=True)
    def _(P):
        a, b = labels("sp.a.%d" % n, (n,), 1), labels("sp.b.%d" % n, (n,), 1)
        return _ops().pixel_weight(P(a), P(b)), _ops().pixel_weight(P(a), P(b), 0.6)


def _pointwise_labels(n, cs=CS):
    tag = "n%d" % n
    LAB = lambda: labels("lab.%d" % n, (n,), 255)
    lut = ((np.arange(256) * 37 + 11) % 256).astype(np.uint8)

    @case("label_lut-" + tag, ["label_lut"], pointwise=True)
    def _(P):
        o = _ops()
        own = P(LAB())
        return o.label_lut(P(LAB()), P(lut)), o.label_lut(own, P(lut), out=own)                      # separate, then out = in

    for c in cs:
        lc = functools.partial(labels, "lab.%d.%d" % (n, c), (n,), c)      # 0..c: c itself marks the unlabelled voxels of the partial form

        @case("label_to_probability-%s-c%d" % (tag, c), ["label_to_probability"], pointwise=True)
        def _(P, c=c, lc=lc):
            return _ops().label_to_probability(P(np.minimum(lc(), c - 1)), c)

        @case("partial_label_to_probability-%s-c%d" % (tag, c), ["partial_label_to_probability"], pointwise=True)
        def _(P, c=c, lc=lc):
            return _ops().partial_label_to_probability(P(lc()), c)


def _pointwise_learning(n):
    tag = "n%d" % n

    big = n > 100000                 # above the grid cap one tensor per entry point says it all

    @case("ssl_perturb-" + tag, ["ssl_perturb"], pointwise=True)
    def _(P):
        o = _ops()
        x = normal("ssl.x.%d" % n, (n,))
        if big:
            return o.ssl_perturb(P(x), None, seed=11, stream_id=3), o.ssl_perturb(P(x), P(normal("ssl.z1.%d" % n, (1, n))))
        return (o.ssl_perturb(P(x), P(normal("ssl.z.%d" % n, (2, n))), reps=2), o.ssl_perturb(P(x), P(normal("ssl.z1.%d" % n, (1, n)))),
                o.ssl_perturb(P(x), None, reps=2, seed=11, stream_id=3))

    @case("ssl_pseudo_onehot-" + tag, ["ssl_pseudo_onehot"], pointwise=True)
    def _(P):
        o = _ops()
        if big:
            return o.ssl_pseudo_onehot([P(normal("ssl.oh.%d" % n, (1, 2, n)))])
        ls = [normal("ssl.oh.%d.%d" % (n, j), (2, 3, n)) for j in range(3)]
        return o.ssl_pseudo_onehot([P(l) for l in ls]), o.ssl_pseudo_onehot([P(ls[0][:, :2].copy())])

    @case("cl_softmax-" + tag, ["cl_softmax"], pointwise=True)
    def _(P):
        if big:
            return _ops().cl_softmax(P(normal("cl.sm.%d" % n, (2, n), 2.0)))
        return _ops().cl_softmax(P(normal("cl.sm.%d" % n, (3, n), 2.0))), _ops().cl_softmax(P(normal("cl.sm8.%d" % n, (8, n), 2.0)))

    @case("ema_step-" + tag, ["ema_step"], pointwise=True)
    def _(P):
        return _ops().ema_step(P(normal("ema.e.%d" % n, (n,))), P(normal("ema.p.%d" % n, (n,))), 0.99)


OPT_STATES = {"SGD": 1, "Adadelta": 2, "Adagrad": 1, "Adamax": 2, "ASGD": 1, "RMSprop": 2, "Rprop": 2, "Adam": 2}


def _optim_hp(kind):
    import optimoracle as OO
    if kind == "Adam":
        return (1e-3, 0.9, 0.999, 1e-8, 1e-5)
    lr = {"Adadelta": 1.0, "Rprop": 1e-2, "Adagrad": 1e-2, "ASGD": 1e-2}.get(kind, 1e-3)
    return OO.abi_hp(kind, OO.named_hp(kind, lr, 0.0 if kind == "Rprop" else 1e-5, 0.9 if kind in ("SGD", "RMSprop") else 0.0), 2)


def _optim_data(kind, n):
    g = rng("optim.%s.%d" % (kind, n))
    p = g.standard_normal(n).astype(np.float32)
    grad = (g.standard_normal(n) * 1e-2).astype(np.float32)
    s0 = (g.random(n) * 1e-2).astype(np.float32)
    s1 = (g.random(n) * 1e-2 + 1e-6).astype(np.float32)
    return p, grad, s0, (s1 if OPT_STATES[kind] > 1 else None)


def _pointwise_optim(n, kinds=tuple(OPT_STATES)):
    for kind in kinds:
        @case("optim_step-%s-n%d" % (kind, n), ["optim_step"], pointwise=True)
        def _(P, kind=kind):
            p, grad, s0, s1 = _optim_data(kind, n)
            tp, ts0, ts1 = P(p), P(s0), (None if s1 is None else P(s1))
            _ops().optim_step(kind, tp, P(grad), ts0, ts1, _optim_hp(kind), 2, 0.5)
            return tp, ts0, ts1

    @case("optim_step-mixed-alignment-n%d" % n, ["optim_step"], pointwise=True)
    def _(P):
        """the scalar body: the streams do not share p's offset inside a 16-byte line"""
        p, grad, s0, s1 = _optim_data("Adam", n)
        tp, ts0, ts1 = P(p), P(s0, misalign=2), P(s1, misalign=3)
        _ops().optim_step("Adam", tp, P(grad, misalign=1), ts0, ts1, _optim_hp("Adam"), 2, 1.0)
        return tp, ts0, ts1


PACK_CO, PACK_CI = 16, 32                                      # the smallest layer fplx_adam_pack_ok takes


def _optim_pack(kind):
    @case("optim_pack_step-" + kind, ["optim_pack_step"], pointwise=True)
    def _(P):
        """p = 8 loose elements | one [16][32][3][3][3] weight | 5 loose elements.  The flat buffers must be 16-byte aligned (the
        header; the refusal is asserted below) and the packs are what the MFMA kernels load: all keep their alignment"""
        ops = _ops()
        nw = PACK_CO * PACK_CI * 27
        n = 8 + nw + 5
        p, grad, s0, s1 = _optim_data(kind, n)
        A = dict(aligned=True)
        tp, ts0, ts1 = P(p, **A), P(s0, **A), (None if s1 is None else P(s1, **A))
        wf, wb = P.empty((27, PACK_CO, PACK_CI), BF, **A), P.empty((27, PACK_CI, PACK_CO), BF, **A)
        stamp = P.empty(ops.pack_stamp_floats(PACK_CO, PACK_CI), F32, **A)
        ops.optim_pack_step(kind, tp, P(grad, **A), ts0, ts1, _optim_hp(kind), 2, 0.5, [(8, PACK_CO, PACK_CI, wf, wb, stamp)])
        return tp, ts0, ts1, wf, wb, stamp


for _n in NS:
    _pointwise_intensity(_n)
    _pointwise_sample(_n)
    _pointwise_labels(_n)
    _pointwise_learning(_n)
    _pointwise_optim(_n)
_pointwise_intensity(IT_CAP)
_pointwise_sample(SP_CAP)
_pointwise_labels(SP_CAP, cs=(3,))
_pointwise_labels(2048 * 256 * 16 + 257, cs=())                 # label_lut_k<VEC>: 16 bytes per lane
_pointwise_labels(2048 * 256 * 4 + 5, cs=(1,))                  # partial_label_k<4>: four voxels per lane
_pointwise_learning(2048 * 256 + 257)                           # grid1(n, 2048): the one-element bodies
_pointwise_optim(4096 * 256 + 257, kinds=("SGD", "Adam"))       # ew_grid: 4096 blocks, the scalar body (mixed alignment)
for _k in OPT_STATES:
    _optim_pack(_k)


@case("ema_step+ssl_perturb-above-the-vector-cap", ["ema_step", "ssl_perturb"], pointwise=True)
def _(P):
    n = 2048 * 256 * 4 + 5                                      # grid1(n / 4, 2048) is capped: every lane makes a second trip
    o = _ops()
    x = normal("ssl.big.x", (n,))
    return o.ema_step(P(x), P(normal("ssl.big.p", (n,))), 0.5), o.ssl_perturb(P(x), P(normal("ssl.big.z", (1, n))))


@case("cl_softmax-above-the-vector-cap", ["cl_softmax"], pointwise=True)
def _(P):
    return _ops().cl_softmax(P(normal("cl.big", (2, 1024 * 256 * 4 + 4), 2.0)))


@case("optim_step-above-the-vector-cap", ["optim_step"], pointwise=True)
def _(P):
    n = 4096 * 256 * 4 + 7
    tp = P(normal("optim.big.p", (n,)))
    _ops().optim_step("SGD", tp, P(normal("optim.big.g", (n,), 1e-2)), None, None, (1e-3, 0.0, 1e-5), 2, 1.0)
    return tp


# =========================================================================================== reductions with partial rows
VS = (1, 63, 257, 4097)


def _reductions_flat(v):
    tag = "v%d" % v
    x = _intensity(v) if v != 63 else normal("red.x", (v,), 40.0, 10.0)

    @case("channel_minmax-" + tag, ["channel_minmax"])
    def _(P):
        return _ops().channel_minmax(P(x)), _ops().channel_minmax(P(x), -20.0, 55.0)

    @case("select_kth+percentiles-" + tag, ["select_kth"])
    def _(P):
        o = _ops()
        return o.select_kth(P(x), [0, v - 1, 0]), o.select_kth(P(x), [v // 2]), [float(q) for q in o.percentiles(P(x), [0, 37.5, 100])]

    for nl, fuse in ((1, False), (16, False), (16, True), (1, True)):
        @case("overlap_counts-%s-l%d-fuse%d" % (tag, nl, fuse), ["overlap_counts"], unguarded=("labels",))
        def _(P, nl=nl, fuse=fuse):
            return _ops().overlap_counts(P(labels("ov.s.%d" % v, (v,), 17)), P(labels("ov.g.%d" % v, (v,), 17)), list(range(1, nl + 1)),
                                         fuse=fuse, on_device=True)

    @case("label_bbox+nonzero_bbox-" + tag, ["label_bbox", "nonzero_bbox"], unguarded=("mask_labels",))
    def _(P):
        o = _ops()
        lab = labels("bb.l.%d" % v, (1, 1, 1, v), 3)
        xz = normal("bb.x.%d" % v, (1, 1, 1, v)) * (uniform("bb.m.%d" % v, (1, 1, 1, v)) > 0.7)
        return o.label_bbox(P(lab), [1, 3]), o.nonzero_bbox(P(xz.astype(np.float32)))


@case("label_bbox+nonzero_bbox-volumes", ["label_bbox", "nonzero_bbox"], unguarded=("mask_labels",))
def _(P):
    o = _ops()
    out = []
    for shape in ((2, 4, 8, 16), (2, 3, 5, 7), (1, 9, 16, 33)):                 # a multiple of 16 elements (the quad loads) and not
        xz = normal("bb.vol.%s" % (shape,), shape) * (uniform("bb.volm.%s" % (shape,), shape) > 0.8)
        xz[-1, -1, -1, -1] = 2.5                                                 # the last element counts
        out += [o.nonzero_bbox(P(xz.astype(np.float32))), o.label_bbox(P(labels("bb.voll.%s" % (shape,), shape, 4)), [2, 4])]
    return out


def _ssl(n, c, v):
    import ssloracle as SO
    tag = "n%d-c%d-v%d" % (n, c, v)
    for t in (0, 2):
        @case("ssl_consistency-%s-t%d" % (tag, t), ["ssl_consistency_fwd", "ssl_consistency_bwd"])
        def _(P, t=t):
            o = _ops()
            st, te, mc = SO.logits_case("fp.ssl.%s.%d" % (tag, t), n, c, v, t)
            s, tt = P(st), P(te)
            out, mask = o.ssl_consistency_fwd(s, tt, None if mc is None else P(mc), thr=float(SO.uamt_threshold(0.5, c)))
            return out, mask, o.ssl_consistency_bwd(s, tt, mask, out, P(np.array([1.5], np.float32)), t)

    @case("ssl_entropy-" + tag, ["ssl_entropy_fwd", "ssl_entropy_bwd"])
    def _(P):
        o = _ops()
        lg = P(SO.logits_case("fp.ssl.ent." + tag, n, c, v, 0)[0])
        return o.ssl_entropy_fwd(lg), o.ssl_entropy_bwd(lg, P(np.array([0.5], np.float32)))

    for k in (2, 4):
        @case("ssl_pyramid-%s-k%d" % (tag, k), ["ssl_pyramid_fwd", "ssl_pyramid_bwd"])
        def _(P, k=k):
            o = _ops()
            ls = [P(SO.logits_case("fp.ssl.pyr.%s.%d" % (tag, j), n, c, v, 0)[0]) for j in range(k)]
            out = o.ssl_pyramid_fwd(ls)
            return out, o.ssl_pyramid_bwd(ls, out, P(np.array([2.0], np.float32)))


LOSS_EXT = ("focal", "noise_robust", "explog", "gce", "mae", "mse", "slsr")


def _loss_ext(n, c, v):
    import lossoracle_ext as LE
    tag = "n%d-c%d-v%d" % (n, c, v)
    lg = normal("le.lg." + tag, (n, c, v), 1.5)
    cls = rng("le.y." + tag).integers(0, c, (n, v))
    y = np.zeros((n, c, v), np.float32)
    np.put_along_axis(y, cls[:, None], 1.0, 1)
    pw = (uniform("le.pw." + tag, (n, 1, v)) > 0.3).astype(np.float32)
    iw = uniform("le.iw." + tag, (n,), 0.5, 1.5)
    for term in LOSS_EXT + ("all",):
        w7 = LE.weights(**({t: 1.0 for t in LOSS_EXT} if term == "all" else {term: 1.0}))
        terms = (0.4, 0.3, 0.2, 0.1) if term == "all" else (0.0, 0.0, 0.0, 0.0)
        prm = LE.params(use_pw=(term == "all"))
        cfg = (ctypes.c_float * (18 + c))(*LE.cfg_array(terms, w7, prm, c))

        @case("seg_loss_ext-%s-%s" % (term, tag), ["seg_loss_ext_fwd", "seg_loss_ext_sums", "seg_loss_ext_from_sums", "seg_loss_ext_bwd"])
        def _(P, cfg=cfg):
            """part holds doubles in its spare rows (8-byte aligned, the header): it keeps its alignment"""
            o = _ops()
            k, rows = o.loss_ext_k(c), o.loss_rows(v)
            tl, ty, tpw, tiw = P(lg), P(y), P(pw), P(iw)
            part, out, coef = P.empty((n, rows, k), F32, aligned=True), P.empty(o.loss_ext_nout(c), F32), P.empty(o.loss_ext_ncoef(n, c), F32)
            o.seg_loss_ext_fwd(tl, ty, tpw, tiw, cfg, True, part, out, coef)
            part2, sums, totals = P.empty((n, rows, k), F32, aligned=True), P.empty((n, k), F64), P.empty(k, F64)
            o.seg_loss_ext_sums(tl, ty, tpw, cfg, True, part2, sums, totals)
            out2, coef2 = P.empty(o.loss_ext_nout(c), F32), P.empty(o.loss_ext_ncoef(n, c), F32)
            o.seg_loss_ext_from_sums(sums, totals, tiw, n, n, c, v, True, cfg, out2, coef2)
            dl = P.empty((n, c, v), F32)
            o.seg_loss_ext_bwd(tl, ty, tpw, coef, P(np.array([1.25], np.float32)), cfg, True, dl)
            return out, coef, sums, totals, out2, coef2, dl


def _nll(n, c, v):
    import nlloracle as NO
    tag = "n%d-c%d-v%d" % (n, c, v)
    for method, k in (("CoTeaching", 2), ("TriNet", 3)):
        @case("nll-%s-%s" % (method, tag), ["nll_voxel_ce_fwd", "nll_select_mask", "nll_select_fwd", "nll_select_bwd", "select_kth"])
        def _(P, method=method, k=k):
            o = _ops()
            logits, y = NO.logits_case("fp.nll.%s.%s" % (method, tag), k, n, c, v)
            ls, ty = [P(l) for l in logits], P(y)
            loss, part = o.nll_voxel_ce_fwd(ls, ty)
            if method == "CoTeaching":
                masks = [o.nll_select_mask(l, o.NLL_RANK, num_remb=max(1, (3 * n * v) // 4)) for l in loss]
                masks0 = o.nll_select_mask(loss[0], o.NLL_RANK, num_remb=0)
            else:
                masks = [o.nll_select_mask(l, o.NLL_BELOW, q=0.8) for l in loss]
                masks0 = None
            uses = o.NLL_USES[method]
            out = o.nll_select_fwd(loss, masks, uses, part)
            dl = o.nll_select_bwd(ls, ty, masks, uses, out, P(np.array([1.0], np.float32)), 1.0 if k == 2 else 1.0 / 3)
            return loss, masks, masks0, out, dl


def _cl(c, m):
    import cloracle as CO
    tag = "c%d-m%d" % (c, m)

    @case("cl-" + tag, ["cl_softmax", "cl_class_stats", "cl_confident_joint", "cl_select_keys", "cl_noise_mask"], unguarded=("pair_active",))
    def _(P):
        o = _ops()
        s, x = CO.logits_case(1234 + c * 10007 + m, c, m)
        ts = P(s)
        psx = o.cl_softmax(P(x))
        sums, counts, thr = o.cl_class_stats(psx, ts)
        joint = o.cl_confident_joint(psx, ts, thr)
        keys = o.cl_select_keys(psx, ts, 0), o.cl_select_keys(psx, ts, 1, 0)
        cc, pc = P(np.full(c, 0.45, np.float32)), P(np.full((c, c), 0.05, np.float32))
        act = 1 - np.eye(c, dtype=np.uint8)
        res = [o.cl_noise_mask(psx, ts, meth, cc, pc, act) for meth in (o.CL_BY_CLASS, o.CL_BY_NOISE_RATE, o.CL_BOTH)]
        return psx, sums, counts, thr, joint, keys, res


for _v in VS:
    _reductions_flat(_v)
    for _nn in (1, 2):
        for _c in (2, 8):
            _ssl(_nn, _c, _v)
            _loss_ext(_nn, _c, _v)
            _nll(_nn, _c, _v)
    for _c in (2, 8):
        _cl(_c, _v)


# ======================================================================================= neighbourhood and gather kernels
TV_SHAPES = ((1, 1, 1), (1, 3, 5), (3, 17, 33), (5, 29, 29))
MS_SHAPES = ((1, 1), (5, 7), (17, 65))


def _wsl_tv(d, h, w):
    import wsloracle as WO

    @case("wsl_tv-%dx%dx%d" % (d, h, w), ["wsl_tv_fwd", "wsl_tv_bwd"])
    def _(P):
        """ws must be 16-byte aligned (the header): it keeps its alignment"""
        o = _ops()
        n, c = 2, 3
        lg = P(WO.logits_case("fp.tv.%d.%d.%d" % (d, h, w), n, c, d, h, w)[0])
        ws = P.empty(3 * n * c * d * h * w, I32, aligned=True)
        out, count = o.wsl_tv_fwd(lg, True, ws=ws)
        return out, count, o.wsl_tv_bwd(lg, count, P(np.array([1.5], np.float32)))


def _wsl_crf(d, h, w):
    import wsloracle as WO

    @case("wsl_gatedcrf-%dx%dx%d" % (d, h, w), ["wsl_gatedcrf_fwd", "wsl_gatedcrf_bwd"], unguarded=("desc",))
    def _(P):
        o = _ops()
        lg, im = WO.logits_case("fp.crf.%d.%d.%d" % (d, h, w), 2, 3, d, h, w, ci=2)
        tl = P(lg)
        out, kp = o.wsl_gatedcrf_fwd(tl, P(im), WO.DEFAULT_DESC, 3)
        return out, kp, o.wsl_gatedcrf_bwd(tl, kp, P(np.array([0.75], np.float32)))


def _wsl_ms(h, w):
    import wsloracle as WO

    @case("wsl_mumford_shah-%dx%d" % (h, w), ["wsl_mumford_shah_fwd", "wsl_mumford_shah_bwd"])
    def _(P):
        o = _ops()
        res = []
        for penalty in (1, 2):
            lg, im = WO.logits_case("fp.ms.%d.%d" % (h, w), 2, 3, 3, h, w, ci=2)
            tl, ti = P(lg), P(im)
            out, cen = o.wsl_mumford_shah_fwd(tl, ti, penalty, 0.5)
            res += [out, cen, o.wsl_mumford_shah_bwd(tl, ti, cen, P(np.array([1.0], np.float32)), penalty, 0.5)]
        return res


for _s in TV_SHAPES:
    _wsl_tv(*_s)
    _wsl_crf(*_s)
for _s in MS_SHAPES:
    _wsl_ms(*_s)


def _both_dtypes(name, shape):
    return (("f32", normal(name, shape, 10.0)), ("u8", labels(name, shape, 255)))


@case("pad_reflect", ["pad_reflect"], pointwise=True)
def _(P):
    o = _ops()
    res = []
    for dt, x in _both_dtypes("pad", (2, 3, 4, 5)):
        res.append(o.pad_reflect(P(x), (1, 2, 3), (6, 8, 11)))
        res.append(o.pad_reflect(P(x), (4, 5, 7), (12, 15, 20)))               # wider than the volume: reflected more than once
        res.append(o.pad_reflect(P(x[:, :1, :1, :]), (0, 0, 2), (1, 1, 9)))
    return res


@case("crop_flip", ["crop_flip"], pointwise=True)
def _(P):
    o = _ops()
    res = []
    for dt, x in _both_dtypes("crop", (2, 5, 6, 7)):
        for mask in range(8):
            res.append(o.crop_flip(P(x), (2, 2, 3), (3, 4, 4), mask))           # the box ends at the far corner
        res.append(o.crop_flip(P(x), (0, 0, 0), (5, 6, 7), 5))
    return res


@case("paste_roi", ["paste_roi"], pointwise=True)
def _(P):
    o = _ops()
    res = []
    for dt, x in _both_dtypes("paste", (2, 3, 4, 5)):
        res += [o.paste_roi(P(x), (0, 0, 0), (5, 7, 9)), o.paste_roi(P(x), (2, 3, 4), (5, 7, 9)), o.paste_roi(P(x), (0, 0, 0), (3, 4, 5))]
    return res


SHEAR = (np.array([[0.93, 0.11, -0.07], [-0.21, 1.08, 0.13], [0.05, -0.17, 0.89]]), np.array([0.6, 2.3, 1.9]))
RS_SHAPES = ((1, 37, 29), (7, 1, 23), (2, 3, 2))


def _transforms(shape):
    """(matrix, offset, output size): the shear of test_gpu_resample's general-matrix test; the identity one voxel beyond
    the far faces; a quarter turn in the (h, w) plane whose samples fall on the last voxel and one step outside it; 10 degrees"""
    import resample_ref as R
    d, h, w = shape
    quarter = (np.array([[1.0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]]), np.array([0.0, h - 1.0, 0.0]), (d, w + 1, h + 1))
    m10, t10 = R.rotate_affine(shape, np.cos(np.pi / 18), np.sin(np.pi / 18), (-1, -2))
    return [SHEAR + ((d + 2, h + 1, w + 3),), (np.eye(3), np.zeros(3), (d + 1, h + 1, w + 1)), quarter, (m10, t10, shape)]


def _resample(shape):
    tag = "%dx%dx%d" % shape

    @case("resample_affine-" + tag, ["resample_affine"], pointwise=True)
    def _(P):
        o = _ops()
        res = []
        for dt, x in _both_dtypes("rs." + tag, (2,) + shape):
            for m, t, out in _transforms(shape):
                for order in ((0, 1) if dt == "f32" else (0,)):
                    res.append(o.resample_affine(P(x), m, t, out, order))
        return res

    @case("spline-" + tag, ["spline_prefilter", "resample_spline"], pointwise=True)
    def _(P):
        o = _ops()
        x = normal("spl." + tag, (2,) + shape, 10.0)
        res = [o.spline_prefilter(P(x), order) for order in o.SPLINE_ORDERS]
        for order in o.SPLINE_ORDERS:
            res += [o.resample_spline(P(x), m, t, out, order) for m, t, out in _transforms(shape)]
        return res


for _s in RS_SHAPES + ((1, 2, 1), (2, 1, 5), (1, 1, 1)):
    _resample(_s)

EDT_SHAPES = ((1, 1, 1), (31, 32, 33), (33, 1, 31), (2, 129, 128))      # EDT_LINES = 32 lines a block; 128 / 129: the thread-count steps


def _edt(shape, nd):
    tag = "%s-%dd" % ("x".join(str(s) for s in shape), nd)
    shp = shape if nd == 3 else shape[1:]
    nb = 2 if nd == 3 else shape[0]

    @case("edt_squared-" + tag, ["edt_squared", "edt_finish"], unguarded=("phantom",))
    def _(P):
        o = _ops()
        m = (uniform("edt." + tag, (nb,) + shp) > 0.2).astype(np.uint8)
        m[-1] = 1 if m[-1].size < 40 else m[-1]                                  # a small last mask has no background: the phantom
        tm = P(m)
        sq, idx = o.edt_squared(tm, (1.5, 1.0, 0.75)[3 - nd:], return_indices=True, batched=True)
        sq2 = o.edt_squared(tm, None, batched=True)
        return sq, idx, sq2, o.edt_finish(sq), o.edt_finish(sq[:1], sq2[:1])

    @case("edt_pass-" + tag, ["edt_pass"])
    def _(P):
        o = _ops()
        g0 = np.where(uniform("edtp." + tag, (2,) + shape) > 0.2, np.inf, 0.0)
        return [o.edt_pass(P(g0), axis, 0.5 + axis) for axis in range(3)]


for _s in EDT_SHAPES:
    _edt(_s, 3)
    _edt(_s, 2)


@case("surface_edge_points", ["surface_edge_points"], pointwise=True)
def _(P):
    o = _ops()
    return [o.edge_points(P((uniform("edge.%s" % (s,), s) > 0.3).astype(np.uint8))) for s in ((1, 1), (17, 33), (1, 1, 1), (5, 17, 33), (3, 1, 257))]


for _ns in (0, 1, 1023, 1024, 1025):
    for _nq in (1, 257):
        @case("surface_min_dist-ns%d-nq%d" % (_ns, _nq), ["surface_min_dist"], pointwise=True)
        def _(P, ns=_ns, nq=_nq):
            q = rng("smd.q.%d.%d" % (ns, nq)).integers(0, 40, (nq, 3)).astype(np.int32)
            s = rng("smd.s.%d.%d" % (ns, nq)).integers(0, 40, (ns, 3)).astype(np.int32)
            return _ops().surface_min_dist(P(q), P(s), (1.5, 1.0, 0.75))

CC_SHAPES = ((1, 1, 1), (1, 1, 300), (3, 129, 65), (9, 70, 131))


def _cc(shape):
    tag = "x".join(str(s) for s in shape)

    @case("connected_components-" + tag, ["cc_label", "keep_largest_component"])
    def _(P):
        o = _ops()
        seg = (labels("cc." + tag, shape, 2) * (uniform("cc.m." + tag, shape) > 0.35)).astype(np.uint8)
        res = []
        for s in ((seg, seg[0]) if shape[0] > 1 else (seg, seg[0], seg[0, 0][None])):
            t = P(np.ascontiguousarray(s))
            res += [o.connected_components(t), o.connected_components(t, per_class=True), o.keep_largest_component(t, 1),
                    o.keep_largest_component(t, 2)]
        return res


for _s in CC_SHAPES:
    _cc(_s)


def _head(hc):
    import headoracle as HO

    @case("head-" + HO.head_id(hc), ["head_fwd", "head_dgrad", "head_wgrad"])
    def _(P):
        """a / da: rows 16-byte aligned (the header; the refusal is asserted below): the activation buffers keep their alignment"""
        o = _ops()
        n, dhw, c, lda, k, dt = hc
        v = dhw[0] * dhw[1] * dhw[2]
        dtype = {"fp32": F32, "bf16": BF}[dt]
        d = HO.head_data(hc)

        def act(arr):
            buf = torch.full((n * v, lda), 3.0, dtype=dtype)
            buf[:, :c] = torch.from_numpy(arr.reshape(n * v, c)).to(dtype)
            buf = P(buf, aligned=True)
            return buf, buf[:, :c]
        f = lambda key: P(d[key].astype(np.float32))
        w, bias, dl = f("w"), f("bias"), f("dlogits")
        abuf, a = act(d["a"])
        logits = P.empty((n, k, v), F32)
        o.head_fwd(a, w, bias, logits, n, v, c, k)
        res = [logits]
        for acc in (False, True):
            dbuf, da = act(d["da0"])
            o.head_dgrad(dl, w, da, n, v, c, k, acc)
            res.append(dbuf)
        nb = o.head_wgrad_ws_bytes(n, v, c, k)
        assert nb > 0 and nb % 4 == 0
        ws = P.empty(nb // 4, F32)
        dw, db, dw2 = P.empty((k, c), F32), P.empty(k, F32), P.empty((k, c), F32)
        o.head_wgrad(a, dl, dw, db, n, v, c, k, ws)
        o.head_wgrad(a, dl, dw2, None, n, v, c, k, ws)
        return res + [dw, db, dw2]


def _interp(ic):
    import headoracle as HO

    @case("interp-" + HO.interp_id(ic), ["interp_fwd", "interp_bwd"], pointwise=True)
    def _(P):
        o = _ops()
        nc, dims, f = ic
        d = HO.interp_data(ic)
        y = P.empty((nc,) + tuple(f * s for s in dims), F32)
        o.interp_fwd(P(d["x"].astype(np.float32)), y, nc, dims, f)
        dx = P.empty((nc,) + tuple(dims), F32)
        o.interp_bwd(P(d["dy"].astype(np.float32)), dx, nc, dims, f)
        return y, dx


def _head_cases():
    import headoracle as HO
    for hc in HO.HEAD_CASES:
        _head(hc)
    for ic in HO.INTERP_CASES:
        _interp(ic)


_head_cases()

AUDITED = frozenset(s for c in CASES for s in c.symbols)

# ---- every other pointer-taking prototype: (the test file that poisons around it - or, for the host-only entry points, calls
# it -, a string that file contains: the symbol or the fplx.ops wrapper it is reached through)
_CONV, _BN, _GEOM, _K, _D25 = ("tests/test_gpu_conv_exact.py", "tests/test_gpu_bn_exact.py", "tests/test_gpu_geom_exact.py",
                               "tests/test_gpu_kernels.py", "tests/test_gpu_25d.py")
_LOSS, _HOST = "tests/test_gpu_loss_exact.py", "tests/test_host_cpu.py"
COVERED_ELSEWHERE = {
    "fplx_last_error": (_GEOM, "last_error"), "fplx_set_tuning": (_HOST, "fplx_set_tuning"), "fplx_get_tuning": (_HOST, "fplx_get_tuning"),
    "fplx_tuning_key": (_HOST, "fplx_tuning_key"), "fplx_conv3d_plan_query": (_CONV, "fplx_conv3d_plan_query"),
    "fplx_pack_conv_weight": (_CONV, "pack_conv_weight"), "fplx_pack_conv_weights_batched": (_CONV, "pack_conv_weights_batched"),
    "fplx_pack_weights_multi": (_K, "pack_weights_multi"), "fplx_pack_deconv_weight": (_CONV, "pack_deconv_weight"),
    "fplx_pack_conv2d_weight": (_CONV, "pack_conv2d_weight"), "fplx_pack_deconv122_weight": (_K, "fplx_pack_deconv122_weight"),
    "fplx_conv3d_fwd": (_CONV, "fplx_conv3d_fwd"), "fplx_conv3d_wgrad": (_CONV, "fplx_conv3d_wgrad"),
    "fplx_stem_wgrad_bn": (_CONV, "fplx_stem_wgrad_bn"), "fplx_conv3d_fwd_cat2": (_CONV, "fplx_conv3d_fwd_cat2"),
    "fplx_conv3d_dgrad_split2": (_CONV, "conv3d_dgrad_split2"), "fplx_conv3d_wgrad_cat2": (_CONV, "conv3d_wgrad_cat2"),
    "fplx_conv3d_fwd_act": (_CONV, "fplx_conv3d_fwd_act"), "fplx_deconv2_fwd": (_CONV, "deconv2_fwd"),
    "fplx_deconv2_dgrad": (_CONV, "deconv2_dgrad"), "fplx_deconv2_wgrad": (_CONV, "deconv2_wgrad"),
    "fplx_conv2d_fwd": (_CONV, "fplx_conv2d_fwd"), "fplx_conv2d_fwd_cat2": (_CONV, "fplx_conv2d_* forms"),
    "fplx_conv2d_dgrad_split2": (_CONV, "fplx_conv2d_* forms"), "fplx_conv2d_wgrad": (_CONV, "fplx_conv2d_wgrad"),
    "fplx_conv2d_wgrad_cat2": (_D25, "conv3d_wgrad_cat2(g0, g1, dyg, dw9, dims, cin, cout, ws, mid=True)"),
    "fplx_maxpool122_fwd": (_GEOM, "fplx_maxpool122_fwd"), "fplx_maxpool122_bwd": (_GEOM, "fplx_maxpool122_bwd"),
    "fplx_deconv122_fwd": (_D25, "deconv2_fwd(xg, wf, b.cuda(), yg, (n, d, h, w), c, co, sd=1)"),
    "fplx_deconv122_dgrad": (_D25, "deconv2_dgrad(dyg, wb, dxg, (n, d, h, w), c, co, sd=1)"),
    "fplx_deconv122_wgrad": (_D25, "deconv2_wgrad(xg, dyg, dw, db, (n, d, h, w), c, co, ws, sd=1)"),
    "fplx_bn_train_finalize": (_BN, "fplx_bn_train_finalize"), "fplx_channel_stats": (_BN, "fplx_channel_stats"),
    "fplx_bn_eval_prepare": (_BN, "bn_eval_prepare"), "fplx_bn_act_fwd": (_BN, "bn_act_fwd"),
    "fplx_bn_act_bwd_reduce": (_BN, "fplx_bn_act_bwd_reduce"), "fplx_bn_act_bwd_finalize": (_BN, "fplx_bn_act_bwd_finalize"),
    "fplx_bn_act_bwd_apply": (_BN, "fplx_bn_act_bwd_apply"), "fplx_maxpool2_fwd": (_GEOM, "fplx_maxpool2_fwd"),
    "fplx_maxpool2_bwd": (_GEOM, "fplx_maxpool2_bwd"), "fplx_bn_act_pool_fwd": (_BN, "bn_act_pool_fwd"),
    "fplx_pool_bwd_bn_reduce": (_BN, "pool_bwd_bn_reduce"), "fplx_outconv_fwd_bn": (_CONV, "fplx_outconv_fwd_bn"),
    "fplx_outconv_dgrad_bn_reduce": (_CONV, "fplx_outconv_dgrad_bn_reduce"),
    "fplx_outconv_dgrad_bn_apply": (_CONV, "fplx_outconv_dgrad_bn_apply"), "fplx_outconv_wgrad_bn": (_CONV, "fplx_outconv_wgrad_bn"),
    "fplx_upsample2_fwd": (_GEOM, "upsample2_fwd"), "fplx_upsample2_bwd": (_GEOM, "upsample2_bwd"),
    "fplx_seg_loss_fwd": (_LOSS, "fplx_seg_loss_fwd"), "fplx_seg_loss_sums": (_LOSS, "fplx_seg_loss_sums"),
    "fplx_seg_loss_from_sums": (_LOSS, "fplx_seg_loss_from_sums"), "fplx_seg_loss_bwd": (_LOSS, "fplx_seg_loss_bwd"),
    "fplx_adam_step": (_K, "fplx_adam_step"), "fplx_adam_pack_step": (_K, "fplx_adam_pack_step"),
    "fplx_mc_filter": (_LOSS, "mc_filter"), "fplx_hard_label": (_LOSS, "hard_label"),
    "fplx_sw_extract": (_GEOM, "fplx_sw_extract"), "fplx_sw_merge": (_GEOM, "fplx_sw_merge"), "fplx_sw_merge_mc": (_GEOM, "fplx_sw_merge_mc"),
}


# ================================================================================================================ the tests
@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=lambda c: c.id)
def test_footprint(c):
    try:
        fp.audit(c, target(), capacity=CAPACITY)
    except RuntimeError as e:
        if any(k in str(e) for k in ("HIP error", "hipError", "illegal memory access", "unspecified launch failure")):
            pytest.exit("footprint audit: GPU fault in case %s - nothing more is started on this device: %s" % (c.id, e), 3)
        raise


@pytest.mark.gpu
def test_an_odd_number_of_mc_passes_is_refused():
    """the consistency pass takes an even T (the header): T = 3 never reaches a kernel, which is why the audit runs T = 0 and 2"""
    import ssloracle as SO
    o = _ops()
    st, te, mc = (torch.from_numpy(a).cuda() for a in SO.logits_case("fp.ssl.odd", 1, 2, 63, 3))
    out = torch.full((4,), float("nan"), dtype=F64, device="cuda")
    with pytest.raises(ValueError):
        o.ssl_consistency_fwd(st, te, mc, thr=0.5, out=out)
    assert bool(torch.isnan(out).all())


@pytest.mark.gpu
def test_alignment_the_header_requires_is_refused():
    """where include/fplx.h requires an alignment, the misaligned operand is refused before any launch (the outputs keep their
    fill) instead of being audited one element off"""
    import headoracle as HO
    o = _ops()
    arena = fp.Arena("cuda", 0xFF, capacity=8 << 20)
    # the fused update + pack: p, g and the state streams on 16 bytes
    nw = PACK_CO * PACK_CI * 27
    p, grad, s0, s1 = _optim_data("Adam", 8 + nw)
    wf, wb = arena.empty((27, PACK_CO, PACK_CI), BF), arena.empty((27, PACK_CI, PACK_CO), BF)
    for bad in range(4):
        ts = [arena.place(a, misalign=1 if i == bad else 0) for i, a in enumerate((p, grad, s0, s1))]
        with pytest.raises(ValueError):
            o.optim_pack_step("Adam", ts[0], ts[1], ts[2], ts[3], _optim_hp("Adam"), 2, 1.0, [(8, PACK_CO, PACK_CI, wf, wb)])
    # the head: rows of a / da on 16 bytes
    n, dhw, c, lda, k, dt = HO.HEAD_CASES[0]
    a = arena.place(np.zeros((n, lda), np.float32), misalign=1)
    w, bias, logits = arena.place(np.zeros((k, c), np.float32)), arena.place(np.zeros(k, np.float32)), arena.empty((n, k, 1), F32)
    with pytest.raises(ValueError):
        o.head_fwd(a, w, bias, logits, n, 1, c, k)
    with pytest.raises(ValueError):
        o.head_dgrad(logits, w, a, n, 1, c, k)
    # TotalVariation's workspace on 16 bytes
    lg = arena.place(normal("refuse.tv", (1, 2, 2, 3, 4)))
    e = lg.numel()
    out = arena.empty(4, F64)
    with pytest.raises(ValueError):
        o.wsl_tv_fwd(lg, True, ws=arena.empty(3 * e, I32, misalign=1), out=out)
    # the class statistics' workspace on 8 bytes
    from fplx import _lib as L
    nb = L.lib().fplx_cl_stats_ws_bytes()
    psx, s = arena.place(uniform("refuse.cl", (2, 8))), arena.place(np.zeros(8, np.uint8))
    ws = arena.empty(nb // 4 + 1, I32, misalign=1)
    sums, counts, thr = arena.empty(2, F64), arena.empty(4, torch.int64), arena.empty(2, F64)
    with pytest.raises(ValueError):
        o.call("fplx_cl_class_stats", psx.data_ptr(), s.data_ptr(), 2, 8, ws.data_ptr(), nb, sums.data_ptr(), counts.data_ptr(),
               thr.data_ptr(), o.stream())
    assert arena.check() == {}
    for t in (wf, wb, logits, out, sums, counts, thr):
        assert bool(t.view(U8).eq(0xFF).all())
