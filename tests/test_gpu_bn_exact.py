"""The exact oracle A and the rounding oracle B of tests/bnoracle.py applied to the BatchNorm kernel family of
fpl-plus_amd/csrc/elementwise.hip through the C ABI (fplx.ops; ops.call where there is no wrapper).  Every output buffer starts as
NaN, every tensor sits in a poisoned buffer (gap columns where ld > C, the elements behind a partial-row buffer's documented extent)
that must come back unchanged.  Every case prints its worst error / bound ratio; with FPLX_RATIO_LOG=<file> the same lines are
written there (profiles/bn_oracle_ratios.txt is such a run).

What each test reaches (kernel<T, VEC, U>; "g" = the channel-group-stationary forms, "flat" = the flat-index forms):
  test_site_voxel_edges        bf16: fwd_g / apply_g<8, 2> / reduce<8, 2> at C = 8, 32, 512 (butterfly reduction, G = 1, 4, 64);
                               fp32: fwd / apply / reduce <float, 4> flat (C = 512: G = 128, the serial LDS reduction);
                               bn_act_bwd_finalize train = 1 and 0; DROP = true and false
  test_pool_voxel_edges        bn_act_pool_fwd_col_k / pool_bwd_bn_reduce_col_k (C = 8, 32) and, at C = 512 with DEFAULT knobs, the
                               thread-per-pooled-voxel bn_act_pool_fwd_k / pool_bwd_bn_reduce_k; pool_col = 0 forces the latter at
                               C = 8, 32 and must give the same bits; pd = 1 and 2; dskip = None
  test_apply_loops             the unrolled main loops AND ragged tails of fwd_g (4), apply_g<U = 2, 4>, flat fwd / apply <bf16, 8>
                               (ew_group = 0), <bf16, 1> (ld = C + 1) and <float, 4>
  test_reduce_loops            reduce<8, U, DROP = true and false> with several trips per lane: C = 512, V = 500 (VL = 4) and C = 32,
                               V = (U - 1) 32768 + 777
  test_every_instantiation     U = 1, 2, 4 of apply_g and reduce (knobs ew_inflight, ew_inflight_reduce) x ew_group = 0, 1, each with
                               dropout (DROP = true) and with p = 0 (DROP = false); C = 24, 48
                               (flat bf16 <8>, serial reduction G = 3, 6); C = 5 (bf16 <1> and fp32 <1>); C = 12 fp32 (<4>, G = 3)
  test_leading_dimensions      every kernel on the engine's views cats[:, :C] and cats[:, C:] (ld = 2 C); bf16 ld = C + 1 and a view
                               starting one element in (<bf16, 1>); the fused tail refuses those (FPLX_E_BADSHAPE), nothing is launched
  test_modes                   p = 0, 0.3, 0.5 (the mask is the oracle's Philox stream), train = 0, dy aliasing dout through
                               ops.bn_act_bwd, accumulation into non-zero dgamma / dbeta / dslope
  test_train_finalize          bn_train_finalize_k: dyadic rows (A), a negative variance before the clamp, a constant channel,
                               count = 1, with and without running-statistics pointers, two successive calls
  test_eval_prepare_then_forward   bn_eval_prepare_k (A with eps = 0, B with 1e-5), its scale / shift through bn_act_fwd
  test_statistics_path         channel_stats_k<bf16 / float> (C = 96: blockIdx.y = 1; C = 8; ld = 2 C) -> bn_train_finalize at
                               mean / sigma = 0, 8, 64 with a constant channel; channel_stats A at the voxel-count edges"""
import os

import numpy as np
import pytest
import torch

import bnoracle as O

pytestmark = pytest.mark.gpu

V_EDGES = (1, 63, 255, 257, 4095, 4097)
POOL_DIMS = {2: ((1, 2, 2, 2), (1, 2, 4, 8), (1, 4, 8, 8), (1, 2, 6, 22), (1, 16, 16, 16), (1, 2, 18, 114)),
             1: ((1, 1, 2, 2), (1, 1, 8, 8), (1, 3, 6, 14), (1, 5, 2, 26), (1, 3, 22, 62), (1, 5, 10, 82))}
PS_A, PS_B = (0.0, 0.5, 0.75), (0.0, 0.3, 0.5)
SEED, SID = 0x1234567890, 11
POISON = -777.0
LAYOUTS = {"plain": (1, 0, 0, 0), "cat0": (2, 0, 0, 0), "catC": (2, 1, 0, 0), "ld+1": (1, 0, 1, 0), "lead1": (1, 0, 0, 1)}
_LINES = []


@pytest.fixture(scope="module", autouse=True)
def _ratio_log():
    yield
    path = os.environ.get("FPLX_RATIO_LOG")
    if path and _LINES:
        with open(path, "a") as f:
            f.write("\n".join(_LINES) + "\n")


@pytest.fixture
def knobs():
    """set tuning knobs for one test; the previous values come back whatever happens"""
    from fplx import _lib
    prev = {}

    def set_(**kv):
        for key, val in kv.items():
            prev.setdefault(key, _lib.get_tuning(key))
            _lib.set_tuning(key, val)
    try:
        yield set_
    finally:
        for key, val in prev.items():
            _lib.set_tuning(key, val)


def _log(case, res):
    line = "%-84s %s" % (case, "  ".join("%s %.3g" % kv for kv in sorted(res.items())))
    print(line)
    _LINES.append(line)


class Buf(object):
    """a [V, C] tensor as the view buf[:, off : off + C] of a poisoned [V, ld] buffer that starts `lead` elements into its
    allocation; data = None: an output, NaN"""

    def __init__(self, v, c, bf16, layout="plain", data=None):
        mul, offc, extra, lead = LAYOUTS[layout]
        ld = mul * c + extra
        dt = torch.bfloat16 if bf16 else torch.float32
        self.flat = torch.full((lead + v * ld + 8,), POISON, dtype=dt, device="cuda")
        self.view = self.flat[lead: lead + v * ld].view(v, ld)[:, offc * c: offc * c + c]
        if data is None:
            self.view.fill_(float("nan"))
        else:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(data, np.float32)).to(dt))

    def np(self):
        return self.view.float().cpu().numpy().astype(np.float64)

    def gaps_ok(self):
        f = self.flat.clone()
        lead = (self.view.data_ptr() - self.flat.data_ptr()) // self.flat.element_size()
        v, c = self.view.shape
        w = torch.as_strided(f, (v, c), (self.view.stride(0), 1), lead)
        w.fill_(POISON)
        return bool((f == POISON).all())


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _bnbuf(k):
    return torch.stack([_f32(k["mean"]), _f32(k["rstd"]), _f32(k["scale"]), _f32(k["shift"])]), _f32([k["slope"]])


def _dev_site(y, dout, k, coef, p, bf16, layout="plain", train=1, acc0=0.0, fwd=True, bwd=True):
    """a site through the C ABI: bn_act_fwd, bn_act_bwd_reduce -> part (exactly fplx_num_partials x (2 C + 1) floats, poison
    behind), bn_act_bwd_finalize, bn_act_bwd_apply with the coef that was handed in -> the dict bnoracle.check_site takes"""
    from fplx import ops
    v, c = y.shape
    bnbuf, slope = _bnbuf(k)
    yb = Buf(v, c, bf16, layout, y)
    got, bufs = {}, [yb]
    if fwd:
        ob = Buf(v, c, bf16, layout)
        ops.bn_act_fwd(yb.view, ob.view, bnbuf, slope, p, SEED, SID, c)
        got["out"] = ob
        bufs.append(ob)
    if bwd:
        db, dyb = Buf(v, c, bf16, layout, dout), Buf(v, c, bf16, layout)
        rows = ops.num_partials(v)
        assert rows == O.num_partials(v)
        need = rows * (2 * c + 1)
        arena = torch.full((need + 256,), POISON, dtype=torch.float32, device="cuda")
        arena[:need] = float("nan")
        dgamma, dbeta, dslope = (torch.full((n,), acc0, dtype=torch.float32, device="cuda") for n in (c, c, 1))
        cf_out = torch.full((2, c), float("nan"), dtype=torch.float32, device="cuda")
        bn = [ops.ptr(bnbuf[i]) for i in range(4)]
        ops.call("fplx_bn_act_bwd_reduce", ops.ptr(yb.view), ops.ld_of(yb.view), ops.ptr(db.view), ops.ld_of(db.view), bn[0], bn[1], bn[2], bn[3],
                 ops.ptr(slope), float(p), SEED, SID, v, c, ops.dt_of(yb.view), ops.ptr(arena), ops.stream())
        ops.call("fplx_bn_act_bwd_finalize", ops.ptr(arena), rows, c, v, train, ops.ptr(dgamma), ops.ptr(dbeta), ops.ptr(dslope), ops.ptr(cf_out),
                 ops.stream())
        cf_in = _f32(coef)
        ops.call("fplx_bn_act_bwd_apply", ops.ptr(yb.view), ops.ld_of(yb.view), ops.ptr(db.view), ops.ld_of(db.view), ops.ptr(dyb.view),
                 ops.ld_of(dyb.view), bn[0], bn[1], bn[2], bn[3], ops.ptr(slope), ops.ptr(cf_in), float(p), SEED, SID, v, c, ops.dt_of(yb.view),
                 ops.stream())
        torch.cuda.synchronize()
        assert bool((arena[need:] == POISON).all()), "bn_act_bwd_reduce wrote behind fplx_num_partials x (2 C + 1)"
        got.update(part=arena[:need].view(rows, 2 * c + 1).cpu().numpy(), dbeta=dbeta.cpu().numpy(), dgamma=dgamma.cpu().numpy(),
                   dslope=dslope.cpu().numpy()[0], coef=cf_out.cpu().numpy(), dy=dyb)
        bufs += [db, dyb]
    torch.cuda.synchronize()
    for b in bufs:
        assert b.gaps_ok(), "a kernel wrote outside its [V, C] view (layout %s)" % layout
    raw = {n: b.view.clone() for n, b in got.items() if isinstance(b, Buf)}
    return {n: (b.np() if isinstance(b, Buf) else b) for n, b in got.items()}, raw


def _site_data(tag, v, c, bf16, exact, fine=True):
    if exact:
        k, coef = O.exact_consts("g.k%s" % tag, c, fine)
        y, d = O.exact_acts("g.a%s" % tag, v, c, fine)
    else:
        y, d = O.real_acts("g.r%s" % tag, v, c, bf16)
        k, coef = O.real_consts("g.rk%s" % tag, y)
    return y, d, k, coef


def _run_site(tag, v, c, bf16, i=0, layout="plain", aligned=True, train=1, fine=True, autograd=None, note=""):
    """A and B on one site shape -> the raw device tensors of both runs (for torch.equal between knob settings)"""
    raws = []
    vec = O.vec_of(bf16, c, aligned)
    gm = O.reduce_geom(v, c, vec)
    for exact in (True, False):
        p = (PS_A if exact else PS_B)[i % 3]
        y, d, k, coef = _site_data("%s.%d.%d.%d" % (tag, c, v, bf16), v, c, bf16, exact, fine)
        got, raw = _dev_site(y, d, k, coef, p, bf16, layout, train)
        res = O.check_site(got, y, d, k, coef, p, SEED, SID, bf16, gm, exact, train, "%s %s" % (tag, "A" if exact else "B"),
                           use_autograd=(v <= 300) if autograd is None else autograd)
        _log("%s %s%s %s c=%d v=%d p=%g %s train=%d" % ("A" if exact else "B", tag, note, "bf16" if bf16 else "fp32", c, v, p, layout, train), res)
        raws.append(raw)
    return raws


# ---------------------------------------------------------------- voxel-count edges

@pytest.mark.parametrize("v", V_EDGES)
@pytest.mark.parametrize("c", [8, 32, 512])
@pytest.mark.parametrize("bf16", [True, False])
def test_site_voxel_edges(bf16, c, v):
    _run_site("edges", v, c, bf16, V_EDGES.index(v) + c // 8)
    if v <= 257:                                           # train = 0 changes the finalize alone: the small volumes suffice
        _run_site("edges.eval", v, c, bf16, V_EDGES.index(v) + c // 8 + 1, train=0, autograd=False)


def _dev_pool(y, g, dskip, k, dims, c, pd, layout="plain"):
    from fplx import ops
    v, vo = y.shape[0], g.shape[0]
    bnbuf, slope = _bnbuf(k)
    yb, a2, pooled = Buf(v, c, True, layout, y), Buf(v, c, True, layout), Buf(vo, c, True, layout)
    gb, sb, dx = Buf(vo, c, True, layout, g), None if dskip is None else Buf(v, c, True, layout, dskip), Buf(v, c, True, layout)
    ops.bn_act_pool_fwd(yb.view, a2.view, pooled.view, bnbuf, slope, dims, c, pd)
    rows = ops.num_partials(v)
    need = rows * (2 * c + 1)
    arena = torch.full((need + 256,), POISON, dtype=torch.float32, device="cuda")
    arena[:need] = float("nan")
    ops.pool_bwd_bn_reduce(yb.view, gb.view, None if sb is None else sb.view, dx.view, bnbuf, slope, dims, c, arena, pd)
    torch.cuda.synchronize()
    assert bool((arena[need:] == POISON).all()), "pool_bwd_bn_reduce wrote behind fplx_num_partials x (2 C + 1)"
    for b in (yb, a2, pooled, gb, dx) + (() if sb is None else (sb,)):
        assert b.gaps_ok(), "a kernel wrote outside its view (layout %s)" % layout
    raw = dict(a2=a2.view.clone(), pooled=pooled.view.clone(), dx=dx.view.clone())
    return dict(a2=a2.np(), pooled=pooled.np(), dx=dx.np(), part=arena[:need].view(rows, 2 * c + 1).cpu().numpy()), raw


def _pool_data(tag, dims, c, pd, exact):
    n, d, h, w = dims
    v, vo = n * d * h * w, n * (d // pd) * (h // 2) * (w // 2)
    if exact:
        k, _ = O.exact_consts("g.pk%s" % tag, c, fine=False)
        y, _ = O.exact_acts("g.pa%s" % tag, v, c, fine=False)
        dskip, g = O.exact_pool_grads("g.pg%s" % tag, v, vo, c)
    else:
        y, dskip = O.real_acts("g.pr%s" % tag, v, c, True)
        k, _ = O.real_consts("g.prk%s" % tag, y)
        g = O.real_acts("g.prg%s" % tag, vo, c, True)[1]
    return y, g, dskip, k


def _run_pool(tag, dims, c, pd, knobs, layout="plain", no_skip=False):
    from fplx import ops
    assert ops.bn_pool_fused_ok(c, torch.bfloat16)
    for exact in (True, False):
        y, g, dskip, k = _pool_data("%s.%s.%d.%d" % (tag, dims, c, pd), dims, c, pd, exact)
        if no_skip:
            dskip = None
        raws = []
        for col in ((1,) if c // 8 > 32 else (1, 0)):        # C = 512: both settings launch the same kernels
            knobs(pool_col=col)
            gm = O.pool_geom(dims, c, pd, col)
            got, raw = _dev_pool(y, g, dskip, k, dims, c, pd, layout)
            res = O.check_pool(got, y, g, dskip, k, gm, exact, "%s %s" % (tag, "A" if exact else "B"),
                               use_autograd=(col == 1 and y.shape[0] <= 300 and dskip is not None))
            _log("%s %s %s c=%d pd=%d %s pool_col=%d (%s) dskip=%d" % ("A" if exact else "B", tag, dims, c, pd, layout, col,
                                                                      "col" if gm["col"] else "per pooled voxel", dskip is not None), res)
            raws.append(raw)
        for n in raws[0]:                                  # the two forms promise the same a2 / pooled / dx bits
            assert torch.equal(raws[0][n].view(torch.int16), raws[-1][n].view(torch.int16)), n


@pytest.mark.parametrize("i", range(6))
@pytest.mark.parametrize("c", [8, 32, 512])
@pytest.mark.parametrize("pd", [2, 1])
def test_pool_voxel_edges(pd, c, i, knobs):
    """C = 512 takes the thread-per-pooled-voxel kernels with the default knobs as well (C / 8 = 64 > 32)"""
    assert not O.pool_geom(POOL_DIMS[pd][i], 512, pd, 1)["col"]
    _run_pool("pool", POOL_DIMS[pd][i], c, pd, knobs, no_skip=(i == 2))


# ---------------------------------------------------------------- loop structure

def _tile_cmp(got, block, bound=None):
    """got [V, C] against the period-P reference block [P, C] -> number of differing entries (bound None) or the worst ratio"""
    p = block.shape[0]
    worst = 0.0
    for s in range(0, got.shape[0], 64 * p):
        part = got[s: s + 64 * p]
        n = part.shape[0] // p
        pieces = [(part[: n * p].reshape(n, p, -1), block, bound)]
        if part.shape[0] > n * p:
            r = part.shape[0] - n * p
            pieces.append((part[n * p:], block[:r], None if bound is None else bound[:r]))
        for a, b, bd in pieces:
            if a.size == 0:
                continue
            if bound is None:
                worst += float((~(a == b)).sum())
            else:
                err = np.abs(a - b)
                worst = max(worst, float(np.max(np.where(err == 0, 0.0, err / bd))) if np.isfinite(a).all() else np.inf)
    return worst


@pytest.mark.parametrize("name,bf16,c,v,layout,kn,unroll", [
    ("apply_g U=4 + fwd_g", True, 512, 65536 + 37, "plain", dict(ew_inflight=4), 4),
    ("apply_g U=2", True, 512, 32768 + 37, "plain", dict(ew_inflight=2), 2),
    ("flat bf16 <8>", True, 512, 65536 + 37, "plain", dict(ew_group=0), 4),
    ("flat bf16 <1>", True, 512, 8192 + 5, "ld+1", dict(), 4),
    ("flat fp32 <4>", False, 512, 32768 + 37, "plain", dict(), 4)])
def test_apply_loops(name, bf16, c, v, layout, kn, unroll, knobs):
    """bn_act_fwd / bn_act_bwd_apply where the 4096-block cap bites: V C / VEC just above U 2^20 plus an odd remainder, so that
    lanes run the unrolled loop AND a ragged tail (asserted on the mirrored launch).  The data has period 4099 voxels (a prime: no
    lane sees a repeating pattern), p = 0, so one block of the reference serves the whole tensor; A and B."""
    from fplx import ops
    knobs(**kn)
    vec = O.vec_of(bf16, c, layout == "plain")
    group = O.group_form(bf16, c, vec, kn.get("ew_group", 1))
    pl = O.apply_plan(v, c, vec, group, unroll)
    assert pl["grid"] == 4096 and O.plan_enters_main_and_tail(pl), pl
    if unroll == 4:                                        # the forward kernels unroll 4 whatever the knob says
        assert O.plan_enters_main_and_tail(O.apply_plan(v, c, vec, group, 4))
    per = 4099
    for exact in (True, False):
        y, d, k, coef = _site_data("loop.%s" % name, per, c, bf16, exact, fine=False)
        e = O.elem(y, d, k, None, 1.0)
        if exact:
            O.exact_pre(y, d, k, coef, 0.0, bf16)
        bnbuf, slope = _bnbuf(k)
        rep = -(-v // per)
        big = lambda a: np.tile(a, (rep, 1))[:v]
        yb, db, ob, dyb = Buf(v, c, bf16, layout, big(y)), Buf(v, c, bf16, layout, big(d)), Buf(v, c, bf16, layout), Buf(v, c, bf16, layout)
        ops.bn_act_fwd(yb.view, ob.view, bnbuf, slope, 0.0, SEED, SID, c)
        cf = _f32(coef)
        ops.call("fplx_bn_act_bwd_apply", ops.ptr(yb.view), ops.ld_of(yb.view), ops.ptr(db.view), ops.ld_of(db.view), ops.ptr(dyb.view),
                 ops.ld_of(dyb.view), ops.ptr(bnbuf[0]), ops.ptr(bnbuf[1]), ops.ptr(bnbuf[2]), ops.ptr(bnbuf[3]), ops.ptr(slope), ops.ptr(cf),
                 0.0, SEED, SID, v, c, ops.dt_of(yb.view), ops.stream())
        torch.cuda.synchronize()
        assert ob.gaps_ok() and dyb.gaps_ok()
        dy = O.apply_dy(e, k, coef)
        hb = O.HB if bf16 else 0.0
        if exact:
            res = {"out": _tile_cmp(ob.np(), O.store(e["out"], bf16)), "dy": _tile_cmp(dyb.np(), O.store(dy, bf16))}
            assert res == {"out": 0.0, "dy": 0.0}, res
        else:
            b1 = 3 * O.U * np.abs(e["out"])
            mag = np.abs(np.asarray(k["scale"], np.float64)) * (np.abs(e["dz"]) + np.abs(coef[0].astype(np.float64)) + np.abs(e["xh"] * coef[1]))
            b2 = 7 * O.U * mag
            res = {"out": _tile_cmp(ob.np(), e["out"], O.GAMMA_SLACK * (b1 + hb * (np.abs(e["out"]) + b1)) + O.ETA),
                   "dy": _tile_cmp(dyb.np(), dy, O.GAMMA_SLACK * (b2 + hb * (np.abs(dy) + b2)) + O.ETA)}
            assert max(res.values()) <= 1.0, res
        _log("%s loops %s c=%d v=%d %s" % ("A" if exact else "B", name, c, v, layout), res)


@pytest.mark.parametrize("u", [1, 2, 4])
def test_reduce_loops(u, knobs):
    """bn_act_bwd_reduce_k<bf16, 8, U>: `sdz += ...` across trips.  C = 512, V = 500: VL = 4 lanes, 4 trips each.  C = 32,
    V = (U - 1) 32768 + 777 (U = 1: 2 x 32768 + 777): 512 rows of 64 lanes, the lanes below 777 run the unrolled loop, the rest
    only the tail.  Dropout on: the mask index inside the unrolled loop."""
    knobs(ew_inflight_reduce=u, ew_inflight=u)
    for c, v in ((512, 500), (32, max(u - 1, 2) * 32768 + 777)):
        gm = O.reduce_geom(v, c, 8)
        st = gm["rows"] * gm["lanes"]
        plans = [O.loop_plan(v, s, st, u) for s in (0, st - 1)]
        assert gm["iters"] > 1 and any(m > 0 for m, _ in plans) and (u == 1 or any(t > 0 for _, t in plans)), (gm["iters"], plans)
        for i in (1, 0):                                   # DROP = true (A 0.5, B 0.3) and DROP = false (p = 0): separate instantiations
            _run_site("reduce.U%d" % u, v, c, True, i, fine=(c == 512), autograd=False)


# ---------------------------------------------------------------- every instantiation

@pytest.mark.parametrize("bf16,c,v", [(True, 32, 257), (True, 24, 255), (True, 48, 4097), (True, 5, 257), (False, 5, 257), (False, 12, 255),
                                      (True, 512, 63)])
def test_every_instantiation(bf16, c, v, knobs):
    """U = 1, 2, 4 x ew_group = 0, 1: the knobs select among kernels with the same arithmetic per element, so out / dy are the same
    bits under every setting (the partial rows too: the knobs do not change how the voxels are dealt)"""
    for i in (1, 0):                                       # DROP = true (A 0.5, B 0.3), then DROP = false (p = 0) of every <T, VEC, U>
        ref = None
        for grp in (1, 0):
            for u in (1, 2, 4):
                knobs(ew_group=grp, ew_inflight=u, ew_inflight_reduce=u)
                raws = _run_site("inst", v, c, bf16, i, autograd=False, note=" ew_group=%d U=%d" % (grp, u))
                if ref is None:
                    ref = raws
                for a, b in zip(ref, raws):
                    for n in a:
                        assert torch.equal(a[n].view(torch.int16 if bf16 else torch.int32), b[n].view(torch.int16 if bf16 else torch.int32)), (n, grp, u, i)


# ---------------------------------------------------------------- leading dimensions and alignment

@pytest.mark.parametrize("layout", ["cat0", "catC", "ld+1", "lead1"])
@pytest.mark.parametrize("bf16", [True, False])
def test_leading_dimensions(bf16, layout, knobs):
    """the engine's views into concatenation buffers (ld = 2 C, the neighbouring columns belong to another tensor) and the two
    misaligned forms, which the generic kernels serve through VEC = 1 (fp32 as well: ld = C + 1 is not a multiple of 4)"""
    from fplx import ops
    aligned = layout in ("cat0", "catC")
    for c, v in ((32, 257), (8, 4097)):
        _run_site("ld", v, c, bf16, 1, layout, aligned, autograd=False)
        # channel_stats on the same views
        y, _ = O.exact_acts("g.ld.st%d" % c, v, c)
        yb = Buf(v, c, bf16, layout, y)
        rows = ops.num_partials(v)
        arena = torch.full((rows * 2 * c + 64,), POISON, dtype=torch.float32, device="cuda")
        ops.call("fplx_channel_stats", ops.ptr(yb.view), ops.ld_of(yb.view), v, c, ops.dt_of(yb.view), ops.ptr(arena), ops.stream())
        torch.cuda.synchronize()
        assert bool((arena[rows * 2 * c:] == POISON).all())
        O.check_stats(arena[: rows * 2 * c].view(rows, 2, c).cpu().numpy(), y, O.stats_geom(v), True, "channel_stats %s" % layout)
    if bf16 and aligned:
        _run_pool("ld.pool", (1, 2, 6, 22), 32, 2, knobs, layout)
        _run_pool("ld.pool", (1, 3, 6, 14), 512, 1, knobs, layout)
    elif bf16:
        # the fused tail has no scalar form: it must refuse, and nothing is launched (the outputs stay NaN)
        dims, c, pd = (1, 2, 4, 8), 32, 2
        y, g, dskip, k = _pool_data("ld.refuse", dims, c, pd, True)
        bnbuf, slope = _bnbuf(k)
        yb, a2, pooled = Buf(64, c, True, layout, y), Buf(64, c, True, layout), Buf(8, c, True, layout)
        with pytest.raises(ValueError):
            ops.bn_act_pool_fwd(yb.view, a2.view, pooled.view, bnbuf, slope, dims, c, pd)
        part = torch.full((ops.num_partials(64), 2 * c + 1), float("nan"), device="cuda")
        gb, sb, dx = Buf(8, c, True, layout, g), Buf(64, c, True, layout, dskip), Buf(64, c, True, layout)
        with pytest.raises(ValueError):
            ops.pool_bwd_bn_reduce(yb.view, gb.view, sb.view, dx.view, bnbuf, slope, dims, c, part, pd)
        torch.cuda.synchronize()
        assert bool(torch.isnan(a2.view.float()).all()) and bool(torch.isnan(dx.view.float()).all()) and bool(torch.isnan(part).all())
    else:
        with pytest.raises(ValueError):                    # fp32: the fused tail is bf16 only
            y32 = torch.zeros((64, 32), device="cuda")
            bnbuf, slope = torch.ones((4, 32), device="cuda"), torch.full((1,), 0.25, device="cuda")
            ops.bn_act_pool_fwd(y32, torch.empty_like(y32), torch.empty((8, 32), device="cuda"), bnbuf, slope, (1, 2, 4, 8), 32, 2)


# ---------------------------------------------------------------- modes

@pytest.mark.parametrize("p", [0.0, 0.3, 0.5])
def test_modes(p):
    """dropout p through the whole site (check_fwd asserts the mask IS the oracle's Philox stream), train = 0, accumulation into
    non-zero gradients, and ops.bn_act_bwd with dy aliasing dout as it documents"""
    from fplx import ops
    v, c = 1021, 64
    gm = O.reduce_geom(v, c, 8)
    y, d, k, coef = _site_data("modes", v, c, True, False)
    for train in (1, 0):
        got, _ = _dev_site(y, d, k, coef, p, True, train=train, acc0=0.5)
        res = O.check_site(got, y, d, k, coef, p, SEED, SID, True, gm, False, train, "modes", acc0=0.5)
        _log("B modes p=%g train=%d acc0=0.5" % (p, train), res)
    if p != 0.3:
        ye, de, ke, ce = _site_data("modes.e", v, c, True, True)
        got, _ = _dev_site(ye, de, ke, ce, p, True, train=0)
        _log("A modes p=%g train=0" % p, O.check_site(got, ye, de, ke, ce, p, SEED, SID, True, gm, True, 0, "modes A"))
    # the three stages through ops.bn_act_bwd, dy written over dout
    bnbuf, slope = _bnbuf(k)
    yb, db = Buf(v, c, True, "cat0", y), Buf(v, c, True, "catC", d)
    part = torch.full((ops.num_partials(v), 2 * c + 1), float("nan"), device="cuda")
    cf = torch.full((2, c), float("nan"), device="cuda")
    dgamma, dbeta, dslope = torch.zeros(c, device="cuda"), torch.zeros(c, device="cuda"), torch.zeros(1, device="cuda")
    ops.bn_act_bwd(yb.view, db.view, db.view, bnbuf, slope, p, SEED, SID, c, True, dgamma, dbeta, dslope, part, cf)
    torch.cuda.synchronize()
    assert yb.gaps_ok() and db.gaps_ok()
    got = dict(part=part.cpu().numpy(), dbeta=dbeta.cpu().numpy(), dgamma=dgamma.cpu().numpy(), dslope=dslope.cpu().numpy()[0],
               coef=cf.cpu().numpy(), dy=db.np())
    _log("B modes p=%g dy aliases dout" % p, O.check_site(got, y, d, k, None, p, SEED, SID, True, gm, False, 1, "alias"))


# ---------------------------------------------------------------- statistics

def _dev_train_finalize(stats, count, gamma, beta, rm, rv, nbt, mom, eps, calls=1):
    from fplx import ops
    rows, _, c = stats.shape
    st = _f32(stats)
    bnbuf = torch.full((4, c), float("nan"), device="cuda")
    rmd, rvd = (None, None) if rm is None else (_f32(rm), _f32(rv))
    nb = None if nbt is None else torch.tensor([nbt], dtype=torch.int64, device="cuda")
    outs = []
    for _ in range(calls):
        ops.bn_train_finalize(st, rows, c, count, _f32(gamma), _f32(beta), rmd, rvd, nb, bnbuf, mom, eps)
        torch.cuda.synchronize()
        b = bnbuf.cpu().numpy()
        outs.append(dict(mean=b[0], rstd=b[1], scale=b[2], shift=b[3], rm=None if rm is None else rmd.cpu().numpy(),
                         rv=None if rv is None else rvd.cpu().numpy(), nbt=None if nbt is None else int(nb.item())))
    return outs


@pytest.mark.parametrize("c,count,rows", [(8, 64, 5), (96, 4096, 257), (512, 1 << 20, 512), (5, 1, 1)])
def test_train_finalize(c, count, rows):
    """bn_train_finalize_k on dyadic rows (A: momentum 1/4; B: momentum 0.1), two successive calls (the momentum recursion and
    the counter), with and without running-statistics pointers; rows > 256: a thread sums two rows; count = 1: the n - 1 guard"""
    if count == 1:
        stats = np.stack([np.full((1, c), 1.5, np.float32), np.full((1, c), 2.25, np.float32)], 1)
        _, gamma, beta, rm, rv = O.dyadic_rows("g.fin1", c, 64, 1)
    else:
        stats, gamma, beta, rm, rv = O.dyadic_rows("g.fin%d" % c, c, count, rows)
        r = O.train_finalize(stats, count, gamma, beta, rm, rv, 0, 0.25, 1e-5)
        assert r["var_raw"][1] < 0 and r["var"][1] == 0 and r["var"][2] == 0
    for mom, exact in ((0.25, True), (0.1, False)):
        outs = _dev_train_finalize(stats, count, gamma, beta, rm, rv, 41, mom, 1e-5, calls=2)
        res = O.check_train_finalize(outs[0], stats, count, gamma, beta, rm, rv, 41, mom, 1e-5, exact)
        res2 = O.check_train_finalize(outs[1], stats, count, gamma, beta, outs[0]["rm"], outs[0]["rv"], 42, mom, 1e-5, exact)
        _log("%s train_finalize c=%d count=%d rows=%d mom=%g" % ("A" if exact else "B", c, count, rows, mom),
             {n: max(res[n], res2[n]) for n in res})
        outs = _dev_train_finalize(stats, count, gamma, beta, None, None, None, mom, 1e-5)
        O.check_train_finalize(outs[0], stats, count, gamma, beta, None, None, None, mom, 1e-5, exact, "no running statistics")


def test_eval_prepare_then_forward():
    from fplx import ops
    g = O.rng("g.ev")
    for c, exact in ((40, True), (40, False), (200, False)):
        gamma, beta, rm = g.integers(-8, 9, c) / 8.0, g.integers(-8, 9, c) / 8.0, g.integers(-8, 9, c) / 4.0
        rv, eps = (4.0 ** g.integers(-2, 3, c), 0.0) if exact else ((0.1 + g.random(c)).astype(np.float32), 1e-5)
        if exact:                                          # the forward's A needs a power-of-two scale = gamma / sqrt(rv)
            gamma = 2.0 ** g.integers(-1, 2, c) * g.choice([1.0, -1.0], c)
        bnbuf = torch.full((4, c), float("nan"), device="cuda")
        ops.bn_eval_prepare(_f32(gamma), _f32(beta), _f32(rm), _f32(rv), bnbuf, eps)
        torch.cuda.synchronize()
        b = bnbuf.cpu().numpy()
        assert np.isnan(b[:2]).all()                       # rows 0 / 1 (mean, rstd) are not eval_prepare's
        res = O.check_eval_prepare(b[2], b[3], gamma, beta, rm, rv, eps, exact)
        # forward with the prepared constants: the kernel's inputs are whatever the device prepared
        k = dict(mean=np.zeros(c, np.float32), rstd=np.ones(c, np.float32), scale=b[2], shift=b[3], slope=0.25)
        y, _ = O.exact_acts("g.evy%d" % c, 255, c) if exact else O.real_acts("g.evy%d" % c, 255, c, True)
        got, _ = _dev_site(y, None, k, None, 0.0, True, bwd=False)
        res.update(O.check_fwd(got["out"], y, k, 0.0, SEED, SID, True, exact))
        _log("%s eval_prepare c=%d eps=%g -> fwd" % ("A" if exact else "B", c, eps), res)


@pytest.mark.parametrize("ratio", [0.0, 8.0, 64.0])
@pytest.mark.parametrize("c", [96, 8])
@pytest.mark.parametrize("bf16", [True, False])
def test_statistics_path(bf16, c, ratio):
    """fplx_channel_stats -> fplx_bn_train_finalize against the float64 statistics of the data.  The variance is E[y^2] - m^2
    from fp32 rows: its error relative to sigma^2 carries (m^2 + sigma^2) / sigma^2, logged as `amp`; channel 3 is constant.
    Also logged: the device's and torch's fp32 batch_norm (CPU) relative error of rstd against float64, worst non-constant channel."""
    from fplx import ops
    v = 4097
    y, _ = O.real_acts("g.st%g.%d" % (ratio, c), v, c, bf16, ratio)
    y[:, 3] = np.float32(3.0)
    gm = O.stats_geom(v)
    rows = ops.num_partials(v)
    assert rows == gm["rows"]
    yb = Buf(v, c, bf16, "cat0", y)
    arena = torch.full((rows * 2 * c + 64,), POISON, dtype=torch.float32, device="cuda")
    arena[: rows * 2 * c] = float("nan")
    ops.call("fplx_channel_stats", ops.ptr(yb.view), ops.ld_of(yb.view), v, c, ops.dt_of(yb.view), ops.ptr(arena), ops.stream())
    torch.cuda.synchronize()
    assert bool((arena[rows * 2 * c:] == POISON).all()) and yb.gaps_ok()
    part = arena[: rows * 2 * c].view(rows, 2, c).cpu().numpy()
    res = {"stats_" + n: r for n, r in O.check_stats(part, y, gm, False).items()}
    g = O.rng("g.stg")
    gamma, beta = (0.5 + g.random(c)).astype(np.float32), g.standard_normal(c).astype(np.float32)
    got = _dev_train_finalize(part, v, gamma, beta, None, None, None, 0.1, 1e-5)[0]
    m, var, dm, dvar, amp = O.stats_path_bounds(y, gm)
    res.update(O.check_train_finalize(got, part, v, gamma, beta, None, None, None, 0.1, 1e-5, False, data_bounds=(m, var, dm, dvar)))
    live = np.arange(c) != 3
    rs64 = 1.0 / np.sqrt(var + float(np.float32(1e-5)))
    yt = torch.from_numpy(y).t().reshape(1, c, v)
    _, _, inv = torch.native_batch_norm(yt, None, None, None, None, True, 0.1, 1e-5)
    res["amp"] = float(np.median(amp[live]))
    res["rstd_relerr_device"] = float(np.max(np.abs(got["rstd"][live] - rs64[live]) / rs64[live]))
    res["rstd_relerr_torch_cpu_fp32"] = float(np.max(np.abs(inv.numpy().astype(np.float64)[live] - rs64[live]) / rs64[live]))
    res["const_channel_var_device"] = float(1.0 / float(got["rstd"][3]) ** 2 - float(np.float32(1e-5)))
    _log("B statistics path %s c=%d v=%d mean/sigma=%g" % ("bf16" if bf16 else "fp32", c, v, ratio), res)
    if ratio == 0.0:
        for ve in V_EDGES:                                 # channel_stats A at the voxel-count edges
            ye, _ = O.exact_acts("g.ste%d" % ve, ve, c)
            b = Buf(ve, c, bf16, "plain", ye)
            r2 = ops.num_partials(ve)
            pe = torch.full((r2, 2, c), float("nan"), device="cuda")
            ops.call("fplx_channel_stats", ops.ptr(b.view), c, ve, c, ops.dt_of(b.view), ops.ptr(pe), ops.stream())
            torch.cuda.synchronize()
            O.check_stats(pe.cpu().numpy(), ye, O.stats_geom(ve), True, "channel_stats A v=%d" % ve)
