"""The two order-independent oracles of tests/convoracle.py on the convolution entry points of the C ABI.

Oracle A (exact): integer operands, results bit for bit - bf16 outputs equal bf16_rne(float64 reference), fp32 outputs (dw,
db, logits) and the host sums of the statistics rows equal the reference.  Sentinels: NaN in every output and statistics
buffer, 0xFF bytes in every workspace (include/fplx.h asks no caller to zero one), 4096 in the unused columns of channel-slice
operands; the columns beside an output slice must keep their NaN.  Oracle B (rounding): real bf16 operands, every element
within the rounding bound and the mean signed error within 0.1 ulp.  Every tuning knob a test sets is restored by the
`knobs` fixture.  test_forward_cases_reach_every_plan is host code only (no `gpu` mark)."""
import pytest
import torch

import convoracle as O
from util import plan_kernel

gpu = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
SENT = 4096.0
K333 = (3, 3, 3)


@pytest.fixture
def knobs():
    from fplx import _lib
    saved = {}

    def set_(key, value):
        if key not in saved:
            saved[key] = _lib.get_tuning(key)
        _lib.set_tuning(key, value)
    try:
        yield set_
    finally:
        for key, value in saved.items():
            _lib.set_tuning(key, value)


def _ws(nbytes):
    return torch.full((max(int(nbytes), 16),), 0xFF, dtype=torch.uint8, device="cuda")


def _nan(shape, dtype=F32):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _sliced(t2d, lo=8, hi=8):
    """[V, C] -> the channel slice [:, lo:lo + C] of a wider buffer whose other columns hold SENT"""
    v, c = t2d.shape
    buf = torch.full((v, lo + c + hi), SENT, dtype=t2d.dtype, device="cuda")
    buf[:, lo:lo + c] = t2d
    return buf[:, lo:lo + c]


def _out_slice(v, c, dtype, lo=8, hi=8):
    buf = _nan((v, lo + c + hi), dtype)
    return buf, buf[:, lo:lo + c]


def _untouched(buf, lo, c):
    assert bool(torch.isnan(buf[:, :lo].float()).all()) and bool(torch.isnan(buf[:, lo + c:].float()).all()), \
        "a write beside the output slice"


def _pre(x, wt, b, dy, what):
    """the 2^24 precondition from per-output upper bounds of the sums of |terms|: forward max|x| sum|w[co]| + |b[co]|, data
    gradient max|dy| sum|w[:, ci]|, weight gradient max|x| sum_v |dy[co]|, bias gradient sum_v |dy[co]|"""
    O.assert_exact_pre(float(x.abs().max()) * wt.abs().flatten(1).sum(1) + (0 if b is None else b.abs()), what + " y")
    if dy is not None:
        O.assert_exact_pre(float(dy.abs().max()) * wt.abs().transpose(0, 1).flatten(1).sum(1), what + " dx")
        O.assert_exact_pre(float(x.abs().max()) * dy.abs().transpose(0, 1).flatten(1).sum(1), what + " dw / db")


# ------------------------------------------------------------------ fplx_conv3d_fwd / data gradient / fplx_conv3d_wgrad

# (n, Cin, Cout, D, H, W), dtype, knobs.  Families by fplx_conv3d_plan_query: 0 generic, 1 direct, 2 tile, 4 march, 5 brick
# (stem 6 and out_conv 7 below; 3 is reserved: its kernel was removed and no plan returns it); test_forward_cases_reach_every_plan checks that every (family, geometry, split > 1)
# the dispatcher can return is here.
FWD_CASES = [
    ((1, 5, 7, 3, 9, 6), F32, {}),           # the fp32 generic path
    ((2, 12, 7, 1, 17, 33), F32, {}),
    ((1, 5, 7, 3, 9, 6), BF, {}),            # generic bf16: Cin % 16 != 0, Cout % 32 != 0
    ((2, 16, 8, 4, 6, 10), BF, {}),
    ((1, 3, 11, 1, 1, 1), BF, {}),           # a single voxel
    ((3, 32, 96, 7, 40, 60), BF, {}),        # direct, unsplit: n = 3, Cout = 96
    ((1, 16, 32, 8, 64, 256), BF, {}),       # direct, unsplit, Cin = 16
    ((2, 16, 32, 4, 6, 10), BF, {}),         # direct, 27-way tap split
    ((1, 48, 32, 5, 15, 33), BF, {}),        # ... H = 15, W = 33
    ((1, 32, 32, 4, 16, 33), BF, {}),        # ... W = 33 (no march below W = 64)
    ((2, 32, 64, 8, 40, 60), BF, {}),        # tile, unsplit, ragged last tile
    ((1, 32, 64, 1, 17, 31), BF, {}),        # tile, D = 1, H = 17, W = 31
    ((2, 128, 128, 2, 5, 5), BF, {}),        # tile, 27-way split
    ((1, 128, 64, 10, 20, 20), BF, {}),      # tile, 9-way split
    ((1, 32, 64, 4, 17, 130), BF, {"march": 0}),    # tile, 9-way split, on a march32 shape with the march kernels off: H = 17
    ((1, 32, 32, 9, 16, 64), BF, {}),        # march32 v2 / v3 (geometry 2)
    ((2, 32, 64, 12, 32, 96), BF, {}),
    ((3, 32, 96, 6, 17, 65), BF, {}),        # march32 8-wave (geometry 0), ragged, n = 3, Cout = 96
    ((1, 64, 64, 6, 16, 80), BF, {}),        # march64, 16 x 16 footprint
    ((1, 64, 32, 7, 24, 64), BF, {}),        # march64, 8 x 32 footprint
    ((1, 64, 32, 37, 24, 64), BF, {}),       # ... several depth segments
    ((1, 128, 64, 4, 17, 65), BF, {}),       # Cin = 128 (streamed weights), ragged
    ((2, 128, 64, 12, 32, 64), BF, {}),      # brick 4 x 8 x 8, unsplit
    ((2, 128, 128, 10, 40, 40), BF, {}),     # brick 5 x 4 x 8, unsplit
    ((2, 256, 128, 8, 32, 32), BF, {}),      # brick 4 x 8 x 8, Cin split 3 + finish
    ((2, 256, 256, 10, 20, 20), BF, {}),     # brick 5 x 4 x 8, Cin split 2 (level 3)
    ((2, 512, 512, 5, 10, 10), BF, {}),      # brick, Cin split 4 (level 4), D = 5: a depth remainder of 1 per brick
]

# what fplx_mfma_conv3d_plan / fplx_conv3d_plan_query can return (conv_mfma.hip, conv_generic.hip)
ALL_PLANS = {(0, -1, False), (1, -1, False), (1, -1, True), (2, -1, False), (2, -1, True),
             (4, 0, False), (4, 2, False), (4, 16, False), (4, 32, False),
             (5, 0, False), (5, 1, False), (5, 0, True), (5, 1, True), (6, -1, False), (7, -1, False)}


def _ids(cases):
    return ["%s-%s%s" % ("x".join(map(str, s)), "f32" if dt == F32 else "bf16",
                         "".join("-%s=%s" % kv for kv in sorted(kn.items()))) for s, dt, kn in cases]


_REF = {}


def _conv3d_refs(shape, mid):
    """integer operands and float64 references of one layer (the last one is kept: knob sweeps repeat a shape)"""
    key = (shape, mid)
    if key not in _REF:
        _REF.clear()
        n, cin, cout, d, h, w = shape
        v = n * d * h * w
        tag = "ex%s%d" % (shape, mid)
        x = O.int_operand(tag + ".x", (n, cin, d, h, w), O.density_for(v, cin * (9 if mid else 27)))
        wt = O.int_weight(tag + ".w", (cout, cin, 3, 3, 3))
        if mid:                                   # a Conv2d in the middle depth plane
            wt[:, :, 0] = 0
            wt[:, :, 2] = 0
        b = O.int_operand(tag + ".b", (cout,), 0.7, 3) if 9 * v < (1 << 21) else torch.zeros(cout)
        dy = O.int_operand(tag + ".dy", (n, cout, d, h, w), 0.5)
        _pre(x, wt, b, dy, str(shape))
        yr = O.cl(O.conv3d_ref(x, wt, b, 1))
        _REF[key] = (x, wt, b, dy, yr, O.stats_ref(yr), O.cl(O.dgrad_ref(dy, wt, 1)), O.wgrad_ref(x, dy, wt.shape, 1),
                     dy.double().sum((0, 2, 3, 4)))
    return _REF[key]


def _run_conv3d_exact(shape, dtype=BF, mid=False):
    """forward + statistics (dense), forward on channel slices without statistics, data gradient (mirrored pack), weight + bias
    gradient (channel slices) - each against the exact result"""
    from fplx import ops
    n, cin, cout, d, h, w = shape
    dims, v = (n, d, h, w), n * d * h * w
    x, wt, b, dy, yr, (s1, s2), dxr, dwr, dbr = _conv3d_refs(shape, mid)
    dt = ops._DT[dtype]
    rnd = O.bf16_rne if dtype == BF else (lambda t: t)
    xg, dyg = O.cl(x).to(dtype).cuda(), O.cl(dy).to(dtype).cuda()
    if mid:
        wf, wb = ops.pack_conv2d_weight(wt[:, :, 1].contiguous().cuda(), dtype)
    else:
        wf, wb = ops.pack_conv_weight(wt.cuda(), dtype)
    cls = ops.cl_strides
    fws = lambda ci, co: _ws(ops.conv3d_fwd_ws_bytes(dims, ci, co, K333, dt, dt, mid))
    # (a) forward + statistics, dense operands
    rows = ops.conv3d_stats_rows(dims, cin, cout, K333, dt, dt, mid)
    stats, y = _nan((rows, 2, cout)), _nan((v, cout), dtype)
    ops.conv3d_fwd(xg, cls(d, h, w, cin), dt, wf, b.cuda(), y, cls(d, h, w, cout), dt, dims, cin, cout, K333, stats, fws(cin, cout), mid)
    O.assert_exact(y, rnd(yr), "y")
    g1, g2 = O.stats_sum(stats)
    O.assert_exact(g1, s1, "sum y")
    O.assert_exact(g2, s2, "sum y^2")
    # (b) channel slices in and out, no statistics
    xs = _sliced(xg)
    ybuf, ys = _out_slice(v, cout, dtype)
    ops.conv3d_fwd(xs, cls(d, h, w, cin + 16), dt, wf, b.cuda(), ys, cls(d, h, w, cout + 16), dt, dims, cin, cout, K333, None,
                   fws(cin, cout), mid)
    O.assert_exact(ys, rnd(yr), "y (channel slices)")
    _untouched(ybuf, 8, cout)
    # (c) data gradient: the same entry point on the mirrored pack
    dx = _nan((v, cin), dtype)
    ops.conv3d_fwd(dyg, cls(d, h, w, cout), dt, wb, None, dx, cls(d, h, w, cin), dt, dims, cout, cin, K333, None, fws(cout, cin), mid)
    O.assert_exact(dx, rnd(dxr), "dx")
    # (d) weight + bias gradient
    db = _nan((cout,))
    if mid:
        dw = _nan((cout, cin, 3, 3))
        ops.conv2d_wgrad(xg, cls(d, h, w, cin), dt, dyg, cls(d, h, w, cout), dt, dw, db, dims, cin, cout,
                         _ws(ops.conv2d_wgrad_ws_bytes(dims, cin, cout)))
        O.assert_exact(dw, dwr[:, :, 1], "dw (Conv2d)")
    else:
        dw = _nan((cout, cin, 3, 3, 3))
        ops.conv3d_wgrad(xs, cls(d, h, w, cin + 16), dt, _sliced(dyg), cls(d, h, w, cout + 16), dt, dw, db, dims, cin, cout, K333,
                         _ws(ops.conv3d_wgrad_ws_bytes(dims, cin, cout, K333)))
        O.assert_exact(dw, dwr, "dw")
    O.assert_exact(db, dbr, "db")


def test_forward_cases_reach_every_plan(knobs):
    """every (family, geometry, split > 1) the forward dispatcher can return is reached by FWD_CASES (3x3x3 layers) or by the
    stem / out_conv cases: a new family without exact coverage fails here"""
    from fplx import _lib
    got = set()
    for (n, cin, cout, d, h, w), dtype, kn in FWD_CASES:
        default = {key: _lib.get_tuning(key) for key in kn}
        for key, value in kn.items():
            knobs(key, value)
        dt = 1 if dtype == BF else 0
        k, g, ks, _ = plan_kernel(n, d, h, w, cin, cout, x_dt=dt, y_dt=dt, full=True)
        got.add((k, g, ks > 1))
        for key, value in default.items():
            knobs(key, value)
    for n, cin, cout, d, h, w in STEM_CASES:
        k, g, ks, _ = plan_kernel(n, d, h, w, cin, cout, x_dt=0, y_dt=1, full=True)
        got.add((k, g, ks > 1))
    for n, c0, ncls, d, h, w in OUTCONV_CASES:
        k, g, ks, _ = plan_kernel(n, d, h, w, c0, ncls, k=(1, 3, 3), x_dt=1, y_dt=0, full=True)
        got.add((k, g, ks > 1))
    assert got == ALL_PLANS, (sorted(ALL_PLANS - got), sorted(got - ALL_PLANS))
    # and ALL_PLANS names every family the ABI declares (include/fplx.h, enum FPLX_KERNEL_*) but the reserved value 3
    # (FPLX_KERNEL_STREAM: kept in the enum so that nothing is renumbered, returned by no plan)
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fplx.h")).read()
    families = {int(v) for v in re.findall(r"FPLX_KERNEL_\w+\s*=\s*(\d+)", header)}
    assert len(families) >= 8 and families - {3} == {k for k, _, _ in ALL_PLANS}, sorted(families)


@gpu
@pytest.mark.parametrize("shape,dtype,kn", FWD_CASES, ids=_ids(FWD_CASES))
def test_conv3d_exact(shape, dtype, kn, knobs):
    for key, value in kn.items():
        knobs(key, value)
    _run_conv3d_exact(shape, dtype)


@gpu
@pytest.mark.parametrize("shape", [(1, 32, 32, 5, 16, 64), (2, 32, 64, 6, 20, 70), (1, 64, 32, 4, 9, 70), (1, 64, 96, 9, 24, 64),
                                   (1, 128, 64, 5, 16, 64), (1, 64, 128, 3, 8, 9), (2, 64, 64, 2, 5, 6), (1, 16, 32, 3, 15, 33)])
def test_conv2d_forms_exact(shape):
    """fplx_conv2d_fwd (statistics, channel slices) / its data gradient / fplx_conv2d_wgrad + db: the 2.5D levels"""
    _run_conv3d_exact(shape, BF, mid=True)


@gpu
def test_benchmark_level0_forward_exact():
    """a level-0 layer of the benchmark (2 x 32 -> 32 at 80 x 160 x 160, march32 v2): forward + statistics; 4.1 M voxels x K = 864
    keeps sum y^2 < 2^24 only at about 0.06 % nonzero inputs without bias - the reference scatters the nonzeros"""
    from fplx import ops
    n, cin, cout, d, h, w = shape = (2, 32, 32, 80, 160, 160)
    dims, v = (n, d, h, w), n * d * h * w
    x = O.int_operand("bench.x", (n, cin, d, h, w), O.density_for(v, cin * 27))
    wt = O.int_weight("bench.w", (cout, cin, 3, 3, 3))
    _pre(x, wt, None, None, str(shape))
    yr = O.conv3d_sparse_ref(x, wt, None)
    s1, s2 = O.stats_ref(yr)
    assert plan_kernel(n, d, h, w, cin, cout, full=True)[:2] == (4, 2)
    wf, _ = ops.pack_conv_weight(wt.cuda(), BF, False)
    xg = O.cl(x).to(BF).cuda()
    del x
    rows = ops.conv3d_stats_rows(dims, cin, cout, K333, ops.BF16, ops.BF16)
    stats, y = _nan((rows, 2, cout)), _nan((v, cout), BF)
    ops.conv3d_fwd(xg, ops.cl_strides(d, h, w, cin), ops.BF16, wf, None, y, ops.cl_strides(d, h, w, cout), ops.BF16, dims, cin, cout,
                   K333, stats)
    O.assert_exact(y, O.bf16_rne(yr), "y")
    g1, g2 = O.stats_sum(stats)
    O.assert_exact(g1, s1, "sum y")
    O.assert_exact(g2, s2, "sum y^2")


# ------------------------------------------------------------------ two-tensor (concatenation) forms

@gpu
@pytest.mark.parametrize("shape,mid", [((1, 20, 40, 64), False), ((2, 21, 24, 70), False), ((1, 16, 32, 64), False),
                                       ((2, 12, 48, 96), False), ((1, 16, 32, 64), True), ((2, 12, 48, 96), True)])
def test_cat2_forms_exact(shape, mid):
    """fplx_conv3d_fwd_cat2 / _dgrad_split2 / _wgrad_cat2 and their fplx_conv2d_* forms: both halves as channel slices"""
    from fplx import ops
    n, d, h, w = dims = shape
    cin, cout, v = 64, 32, n * d * h * w
    assert ops.conv3d_cat2_ok(dims, cin, cout)
    x, wt, b, dy, yr, (s1, s2), dxr, dwr, _ = _conv3d_refs((n, cin, cout, d, h, w), mid)
    wf, wb = (ops.pack_conv2d_weight(wt[:, :, 1].contiguous().cuda(), BF) if mid else ops.pack_conv_weight(wt.cuda(), BF))
    xg = O.cl(x).to(BF).cuda()
    x0, x1 = _sliced(xg[:, :32].contiguous()), _sliced(xg[:, 32:].contiguous())
    rows = ops.conv3d_stats_rows(dims, cin, cout, K333, ops.BF16, ops.BF16, mid)
    stats = _nan((rows, 2, cout))
    ybuf, ys = _out_slice(v, cout, BF)
    ops.conv3d_fwd_cat2(x0, x1, wf, b.cuda(), ys, dims, cin, cout, stats, mid)
    O.assert_exact(ys, O.bf16_rne(yr), "y")
    _untouched(ybuf, 8, cout)
    g1, g2 = O.stats_sum(stats)
    O.assert_exact(g1, s1, "sum y")
    O.assert_exact(g2, s2, "sum y^2")
    b0, dx0 = _out_slice(v, 32, BF)
    b1, dx1 = _out_slice(v, 32, BF)
    ops.conv3d_dgrad_split2(O.cl(dy).to(BF).cuda(), wb, dx0, dx1, dims, cin, cout, mid)
    O.assert_exact(torch.cat([dx0.float().cpu(), dx1.float().cpu()], 1), O.bf16_rne(dxr), "dx0 | dx1")
    _untouched(b0, 8, 32)
    _untouched(b1, 8, 32)
    dw = _nan((cout, cin, 3, 3) if mid else (cout, cin, 3, 3, 3))
    ops.conv3d_wgrad_cat2(x0, x1, _sliced(O.cl(dy).to(BF).cuda()), dw, dims, cin, cout,
                          _ws(ops.conv3d_wgrad_ws_bytes(dims, cin, cout, K333)), mid)
    O.assert_exact(dw, dwr[:, :, 1] if mid else dwr, "dw")


@gpu
@pytest.mark.parametrize("shape,two", [((1, 32, 32, 9, 16, 64), False), ((2, 128, 64, 12, 32, 64), False),
                                       ((2, 128, 128, 2, 5, 5), False), ((2, 256, 256, 10, 20, 20), False),
                                       ((4, 64, 32, 16, 32, 64), True), ((4, 128, 64, 16, 32, 44), True),
                                       ((3, 128, 64, 12, 40, 40), True)])
def test_conv3d_fwd_act_exact(shape, two):
    """fplx_conv3d_fwd_act (eval-mode BatchNorm folded into the pack by the caller, PReLU slope 1/4 in the write-out): one-tensor
    form on the march / brick / split-K kernels, two-tensor form with a shared skip tensor (n_x0 = 1) and without"""
    from fplx import ops
    n, cin, cout, d, h, w = shape
    dims, v = (n, d, h, w), n * d * h * w
    assert ops.conv3d_fwd_act_ok(dims, cin, cout, False, two)
    tag = "act%s" % (shape,)
    wt = O.int_weight(tag + ".w", (cout, cin, 3, 3, 3))
    b = O.int_operand(tag + ".b", (cout,), 0.7, 3)
    slope = torch.tensor([0.25])
    wp, _ = ops.pack_conv_weight(wt.cuda(), BF, False)
    p = O.density_for(v, cin * 27, pmax=0.3)
    for n0 in ((n, 1) if two else (n,)):
        half = cin // 2
        x0 = O.int_operand(tag + ".x0%d" % n0, (n0, half if two else cin, d, h, w), p)
        x1 = O.int_operand(tag + ".x1", (n, half, d, h, w), p) if two else None
        full = torch.cat([x0.repeat(n // n0, 1, 1, 1, 1), x1], 1) if two else x0
        _pre(full, wt, b, None, tag)
        z = O.cl(O.conv3d_ref(full, wt, b, 1))
        ref = torch.where(z > 0, z, z * 0.25)
        ybuf, ys = _out_slice(v, cout, BF, 0, 8)
        x0g, x1g = O.cl(x0).to(BF).cuda(), None if x1 is None else O.cl(x1).to(BF).cuda()
        ws = _ws(ops.conv3d_fwd_ws_bytes(dims, cin, cout, K333, ops.BF16, ops.BF16))     # (ops.conv3d_fwd_act brings its own)
        bg, sg = b.cuda(), slope.cuda()
        ops.call("fplx_conv3d_fwd_act", ops.ptr(x0g), ops.ptr(x1g), ops.ld_of(x0g), ops.ptr(wp), ops.ptr(bg), ops.ptr(sg),
                 ops.ptr(ys), ops.ld_of(ys), n, d, h, w, cin, cout, 0, 0 if n0 == n else n0, ops.ptr(ws), ws.numel(), ops.stream())
        O.assert_exact(ys, O.bf16_rne(ref), "PReLU(conv) n_x0 = %d" % n0)
        assert bool(torch.isnan(ybuf[:, cout:].float()).all())


# ------------------------------------------------------------------ transposed convolutions

@gpu
@pytest.mark.parametrize("shape,sd,dtype", [((2, 12, 7, 3, 4, 5), 2, F32), ((2, 64, 32, 3, 4, 5), 2, BF), ((1, 128, 64, 2, 5, 9), 2, BF),
                                            ((1, 32, 32, 4, 4, 7), 2, BF), ((1, 96, 32, 2, 3, 67), 2, BF), ((2, 64, 32, 9, 37, 50), 2, BF),
                                            ((1, 128, 64, 8, 65, 63), 2, BF), ((1, 64, 32, 1, 1, 1), 2, BF),
                                            ((2, 16, 24, 5, 8, 12), 1, F32), ((2, 16, 24, 5, 8, 12), 1, BF), ((2, 64, 32, 5, 8, 12), 1, BF),
                                            ((2, 32, 64, 5, 8, 12), 1, BF), ((1, 64, 32, 3, 17, 33), 1, BF)])
def test_deconv_exact(shape, sd, dtype):
    """fplx_deconv2_* (ConvTranspose3d(2, 2)) and fplx_deconv122_* (ConvTranspose2d(2, 2) per depth slice): forward into the
    upper half of a concatenation buffer, data gradient, weight + bias gradient"""
    from fplx import ops
    n, cin, cout, d, h, w = shape
    dims, v = (n, d, h, w), n * d * h * w
    do, vo = sd * d, n * sd * d * 4 * h * w
    tag = "dc%s%d" % (shape, sd)
    x = O.int_operand(tag + ".x", (n, cin, d, h, w), 0.5)
    wt = O.int_weight(tag + ".w", (cin, cout, 2, 2, 2) if sd == 2 else (cin, cout, 2, 2))
    b = O.int_operand(tag + ".b", (cout,), 0.7, 3)
    dy = O.int_operand(tag + ".dy", (n, cout, do, 2 * h, 2 * w), 0.5)
    w5 = wt if sd == 2 else wt.unsqueeze(2)
    stride = (sd, 2, 2)
    xr, wr, br = x.double().requires_grad_(True), w5.double().requires_grad_(True), b.double().requires_grad_(True)
    yr = torch.nn.functional.conv_transpose3d(xr, wr, br, stride=stride)
    yr.backward(dy.double())
    O.assert_exact_pre(float(x.abs().sum(1).max()) * 2 + 3, tag)            # K = Cin terms of |w| <= 2
    O.assert_exact_pre(dy.abs().sum((0, 2, 3, 4)) * float(x.abs().max()), tag + " dw")
    O.assert_exact_pre(float(dy.abs().max()) * wt.abs().flatten(1).sum(1), tag + " dx")       # taps x Cout terms per dx
    dt = ops._DT[dtype]
    rnd = O.bf16_rne if dtype == BF else (lambda t: t)
    wf, wb = ops.pack_deconv_weight(wt.cuda(), dtype)
    cat = _nan((vo, 2 * cout), dtype)
    ops.deconv2_fwd(O.cl(x).to(dtype).cuda(), wf, b.cuda(), cat[:, cout:], dims, cin, cout, sd)
    O.assert_exact(cat[:, cout:], rnd(O.cl(yr.detach())), "y")
    assert bool(torch.isnan(cat[:, :cout].float()).all())
    dx = _nan((v, cin), dtype)
    dyg = O.cl(dy).to(dtype).cuda()
    ops.deconv2_dgrad(dyg, wb, dx, dims, cin, cout, sd)
    O.assert_exact(dx, rnd(O.cl(xr.grad)), "dx")
    dw, db = _nan(tuple(wt.shape)), _nan((cout,))
    ops.deconv2_wgrad(O.cl(x).to(dtype).cuda(), dyg, dw, db, dims, cin, cout, _ws(ops.deconv2_wgrad_ws_bytes(dims, cin, cout, sd)), sd)
    O.assert_exact(dw, wr.grad.view(wt.shape), "dw")
    O.assert_exact(db, br.grad, "db")


# ------------------------------------------------------------------ stem and out_conv

STEM_CASES = [(2, 1, 32, 3, 9, 35), (1, 1, 32, 1, 1, 40), (3, 1, 32, 5, 7, 161), (1, 1, 32, 1, 1, 1), (2, 1, 64, 6, 20, 96),
              (2, 4, 32, 3, 9, 35), (3, 4, 64, 2, 5, 70), (1, 4, 32, 1, 1, 1), (1, 1, 32, 4, 15, 33)]
OUTCONV_CASES = [(2, 32, 2, 3, 9, 35), (1, 32, 3, 2, 16, 64), (1, 64, 2, 2, 8, 40), (1, 16, 4, 3, 15, 33), (1, 32, 1, 1, 1, 1),
                 (2, 32, 4, 1, 17, 31)]


@gpu
@pytest.mark.parametrize("shape", STEM_CASES)
def test_stem_exact(shape):
    """the MFMA stem kernels (fp32 NCDHW network input of 1 | 4 channels -> bf16 NDHWC): forward + statistics, weight gradient"""
    from fplx import ops
    n, cin, cout, d, h, w = shape
    dims, v = (n, d, h, w), n * d * h * w
    assert plan_kernel(n, d, h, w, cin, cout, x_dt=0, y_dt=1) == 6
    tag = "st%s" % (shape,)
    x = O.int_operand(tag + ".x", (n, cin, d, h, w), O.density_for(v, cin * 27))
    wt = O.int_weight(tag + ".w", (cout, cin, 3, 3, 3))
    b = O.int_operand(tag + ".b", (cout,), 0.7, 3)
    dy = O.int_operand(tag + ".dy", (n, cout, d, h, w), 0.5)
    _pre(x, wt, b, dy, tag)
    yr = O.cl(O.conv3d_ref(x, wt, b, 1))
    s1, s2 = O.stats_ref(yr)
    wf, _ = ops.pack_conv_weight(wt.cuda(), BF, False)
    rows = ops.conv3d_stats_rows(dims, cin, cout, K333, ops.F32, ops.BF16)
    stats, y = _nan((rows, 2, cout)), _nan((v, cout), BF)
    ops.conv3d_fwd(x.cuda(), ops.planar_strides(cin, d, h, w), ops.F32, wf, b.cuda(), y, ops.cl_strides(d, h, w, cout), ops.BF16,
                   dims, cin, cout, K333, stats)
    O.assert_exact(y, O.bf16_rne(yr), "y")
    g1, g2 = O.stats_sum(stats)
    O.assert_exact(g1, s1, "sum y")
    O.assert_exact(g2, s2, "sum y^2")
    dw = _nan((cout, cin, 3, 3, 3))
    ops.conv3d_wgrad(x.cuda(), ops.planar_strides(cin, d, h, w), ops.F32, O.cl(dy).to(BF).cuda(), ops.cl_strides(d, h, w, cout),
                     ops.BF16, dw, None, dims, cin, cout, K333, _ws(ops.conv3d_wgrad_ws_bytes(dims, cin, cout, K333)))
    O.assert_exact(dw, O.wgrad_ref(x, dy, wt.shape, 1), "dw")


def _outconv_refs(tag, n, c0, ncls, d, h, w, a=None):
    x = a if a is not None else O.int_operand(tag + ".x", (n, c0, d, h, w), 0.5)
    wt = O.int_weight(tag + ".w", (ncls, c0, 1, 3, 3))
    b = O.int_operand(tag + ".b", (ncls,), 0.7, 3)
    dl = O.int_operand(tag + ".dl", (n, ncls, d, h, w), 0.5)
    xr, wr, br = x.double().requires_grad_(True), wt.double().requires_grad_(True), b.double().requires_grad_(True)
    lr = torch.nn.functional.conv3d(xr, wr, br, padding=(0, 1, 1))
    lr.backward(dl.double())
    return x, wt, b, dl, lr.detach(), xr.grad, wr.grad, br.grad


@gpu
@pytest.mark.parametrize("shape", OUTCONV_CASES)
def test_outconv_exact(shape, knobs):
    """out_conv (bf16 NDHWC features -> fp32 planar logits, kernel (1, 3, 3)): forward, data gradient, weight + bias gradient"""
    from fplx import ops
    n, c0, ncls, d, h, w = shape
    dims, v = (n, d, h, w), n * d * h * w
    assert plan_kernel(n, d, h, w, c0, ncls, k=(1, 3, 3), x_dt=1, y_dt=0) == 7
    x, wt, b, dl, lr, dxr, dwr, dbr = _outconv_refs("oc%s" % (shape,), n, c0, ncls, d, h, w)
    _pre(x, wt, b, dl, "out_conv")
    wf, _ = ops.pack_conv_weight(wt.cuda(), F32, False)
    _, wb = ops.pack_conv_weight(wt.cuda(), BF, True)
    xg = O.cl(x).to(BF).cuda()
    lg = _nan((n, ncls, d, h, w))
    ops.conv3d_fwd(xg, ops.cl_strides(d, h, w, c0), ops.BF16, wf, b.cuda(), lg, ops.planar_strides(ncls, d, h, w), ops.F32, dims, c0,
                   ncls, (1, 3, 3), None)
    O.assert_exact(lg, lr, "logits")
    dx = _nan((v, c0), BF)
    ops.conv3d_fwd(dl.cuda(), ops.planar_strides(ncls, d, h, w), ops.F32, wb, None, dx, ops.cl_strides(d, h, w, c0), ops.BF16, dims,
                   ncls, c0, (1, 3, 3), None)
    O.assert_exact(dx, O.bf16_rne(O.cl(dxr)), "dx")
    dw, db = _nan((ncls, c0, 1, 3, 3)), _nan((ncls,))
    ops.conv3d_wgrad(xg, ops.cl_strides(d, h, w, c0), ops.BF16, dl.cuda(), ops.planar_strides(ncls, d, h, w), ops.F32, dw, db, dims,
                     c0, ncls, (1, 3, 3), _ws(ops.conv3d_wgrad_ws_bytes(dims, c0, ncls, (1, 3, 3))))
    O.assert_exact(dw, dwr, "dw")
    O.assert_exact(db, dbr, "db")


@gpu
@pytest.mark.parametrize("rows", [1, 0])
@pytest.mark.parametrize("shape", [(2, 3, 9, 35, 2), (1, 2, 16, 64, 2), (1, 4, 24, 40, 3), (1, 1, 1, 1, 2), (2, 1, 32, 32, 2),
                                   (1, 3, 5, 31, 1)])
def test_outconv_fused_bn_exact(shape, rows, knobs):
    """fplx_outconv_fwd_bn (a = PReLU(scale y + shift) and the logits in one pass) and fplx_outconv_wgrad_bn (dw, db from y),
    row-segment and tile forms: power-of-two scales, integer shifts and slope 1/4 keep a dyadic (multiples of 1/8) and the
    logits / gradients exact - the precondition in units of 1/8"""
    from fplx import ops
    n, d, h, w, ncls = shape
    c0, dims, v = 32, (n, d, h, w), n * d * h * w
    knobs("outconv_fwd_rows", rows)
    knobs("outconv_dgrad_rows", rows)
    tag = "ocbn%s" % (shape,)
    y = O.int_operand(tag + ".y", (v, c0), 0.6, 2)
    scale = 2.0 ** torch.randint(-1, 2, (c0,), generator=O._gen(tag + ".s")).float()
    shift = torch.randint(-1, 2, (c0,), generator=O._gen(tag + ".t")).float()
    z = y * scale + shift
    a2 = torch.where(z > 0, z, z * 0.25)
    a = O.uncl(a2, n, d, h, w)
    x, wt, b, dl, lr, _, dwr, dbr = _outconv_refs(tag, n, c0, ncls, d, h, w, a)
    _pre(8 * a, wt, 8 * b, dl, tag + " (units of 1/8)")
    bnbuf = torch.stack([torch.zeros(c0), torch.ones(c0), scale, shift]).cuda()
    slope = torch.tensor([0.25]).cuda()
    wf, _ = ops.pack_conv_weight(wt.cuda(), F32, False)
    yg = y.to(BF).cuda()
    ag, lg = _nan((v, c0), BF), _nan((n, ncls, d, h, w))
    ops.outconv_fwd_bn(yg, bnbuf, slope, ag, wf, b.cuda(), lg, dims, c0, ncls)
    O.assert_exact(ag, O.bf16_rne(a2), "a")
    O.assert_exact(lg, lr, "logits")
    nws = ops.outconv_wgrad_bn_ws_bytes(dims, c0, ncls)
    if nws:
        dw, db = _nan((ncls, c0, 1, 3, 3)), _nan((ncls,))
        ops.outconv_wgrad_bn(yg, bnbuf, slope, dl.cuda(), dw, db, dims, c0, ncls, _ws(nws))
        O.assert_exact(dw, dwr, "dw")
        O.assert_exact(db, dbr, "db")
    else:
        assert rows == 0 or ncls > 3


def _bn_consts(tag, c):
    """BatchNorm constants that keep the fused backward exact: integer mean, power-of-two rstd and scale, integer shift, and
    coefficients coef = [k0, k1] on a grid of 1/4 (what fplx_bn_act_bwd_finalize would write, chosen directly)"""
    g = O._gen(tag + ".bn")
    mean = torch.randint(-1, 2, (c,), generator=g).float()
    rstd = 2.0 ** torch.randint(-1, 2, (c,), generator=g).float()
    scale = 2.0 ** torch.randint(-1, 2, (c,), generator=g).float()
    shift = torch.randint(-1, 2, (c,), generator=g).float()
    coef = torch.stack([torch.randint(-4, 5, (c,), generator=g).float() / 4, torch.randint(-1, 2, (c,), generator=g).float() / 4])
    return mean, rstd, scale, shift, coef


def _bn_bwd_ref(y, da, mean, rstd, scale, shift, coef, slope=0.25):
    """float64 on [V, C]: dz = d(PReLU) da, x-hat, the reduction's three sums and the apply pass's dy (before its bf16 rounding)"""
    y, da = y.double(), da.double()
    z = y * scale.double() + shift.double()
    dz = torch.where(z > 0, da, da * slope)
    xh = (y - mean.double()) * rstd.double()
    dy = scale.double() * (dz - coef[0].double() - xh * coef[1].double())
    sums = (dz.sum(0), (dz * xh).sum(0), torch.where(z > 0, torch.zeros_like(z), da * z).sum().view(1))
    mags = (dz.abs().sum(0), (dz * xh).abs().sum(0), (da * z).abs().sum().view(1))
    return dy, sums, mags


@gpu
@pytest.mark.parametrize("rows", [1, 0])
@pytest.mark.parametrize("shape", [(2, 3, 9, 35, 2), (1, 2, 16, 64, 2), (1, 4, 24, 40, 3), (1, 1, 1, 1, 2), (2, 1, 32, 32, 2),
                                   (1, 3, 5, 31, 1), (2, 2, 17, 33, 4)])
def test_outconv_dgrad_bn_exact(shape, rows, knobs):
    """fplx_outconv_dgrad_bn_reduce / _apply (out_conv's data gradient recomputed inside the last site's BatchNorm + PReLU
    backward, never stored), row-segment and tile forms: the reduction's partial rows (NaN-filled) summed on the host give
    sum dz, sum dz x-hat and the slope sum exactly; the apply pass writes bf16_rne(scale (dz - k0 - x-hat k1)) into a channel
    slice.  dz is a multiple of 1/4, x-hat and z of 1/2, dy of 1/16: the precondition in those units"""
    from fplx import ops
    n, d, h, w, ncls = shape
    c0, dims, v = 32, (n, d, h, w), n * d * h * w
    knobs("outconv_dgrad_rows", rows)
    knobs("outconv_fwd_rows", rows)
    tag = "ocdg%s" % (shape,)
    y = O.int_operand(tag + ".y", (v, c0), 0.6, 2)
    mean, rstd, scale, shift, coef = _bn_consts(tag, c0)
    _, wt, _, dl, _, dar, _, _ = _outconv_refs(tag, n, c0, ncls, d, h, w, O.uncl(y, n, d, h, w))
    da = O.cl(dar)                                # out_conv's data gradient: integers, exact in bf16
    dyr, sums, mags = _bn_bwd_ref(y, da, mean, rstd, scale, shift, coef)
    O.assert_exact_pre(float(dl.abs().max()) * wt.abs().transpose(0, 1).flatten(1).sum(1), tag + " d(a)")
    for m, unit, what in zip(mags, (4, 8, 2), ("sum dz", "sum dz x-hat", "slope sum")):
        O.assert_exact_pre(unit * m, "%s %s (units of 1/%d)" % (tag, what, unit))       # dz: quarters, x-hat: halves, z: halves
    O.assert_exact_pre(16 * (2 * dyr.abs()), tag + " dy (units of 1/16)")
    bn = [t.cuda() for t in (mean, rstd, scale, shift)]
    slope = torch.tensor([0.25]).cuda()
    _, wb = ops.pack_conv_weight(wt.cuda(), BF, True)
    yg, dlg = y.to(BF).cuda(), dl.cuda()
    nrows = ops.outconv_bn_rows(dims, c0, ncls)
    part = _nan((nrows, 2 * c0 + 1))
    ops.call("fplx_outconv_dgrad_bn_reduce", ops.ptr(dlg), ops.ptr(wb), ops.ptr(yg), c0, *[ops.ptr(t) for t in bn], ops.ptr(slope),
             ops.ptr(part), n, d, h, w, c0, ncls, ops.stream())
    tot = part.double().cpu().sum(0)
    O.assert_exact(tot[:c0], sums[0], "sum dz")
    O.assert_exact(tot[c0:2 * c0], sums[1], "sum dz x-hat")
    O.assert_exact(tot[2 * c0:], sums[2], "slope sum")
    dbuf, dys = _out_slice(v, c0, BF)
    coefg = coef.cuda()
    ops.call("fplx_outconv_dgrad_bn_apply", ops.ptr(dlg), ops.ptr(wb), ops.ptr(yg), c0, *[ops.ptr(t) for t in bn], ops.ptr(slope),
             ops.ptr(coefg), ops.ptr(dys), ops.ld_of(dys), n, d, h, w, c0, ncls, ops.stream())
    O.assert_exact(dys, O.bf16_rne(dyr), "dy")
    _untouched(dbuf, 8, c0)


@gpu
@pytest.mark.parametrize("shape", [(2, 1, 32, 3, 9, 35), (1, 1, 32, 5, 16, 64), (1, 4, 32, 2, 16, 64), (3, 1, 32, 5, 7, 161),
                                   (1, 1, 32, 1, 1, 1), (2, 1, 64, 6, 20, 96), (2, 4, 32, 3, 10, 48), (1, 4, 64, 4, 15, 33)])
def test_stem_wgrad_bn_exact(shape):
    """fplx_stem_wgrad_bn (the stem's weight gradient forming dy = bf16(scale (dz - k0 - x-hat k1)) from y and d(a) itself):
    dw against the float64 weight gradient of that dy, bit for bit; dy is a multiple of 1/32 - the precondition in those units"""
    from fplx import ops
    n, cin, cout, d, h, w = shape
    dims, v = (n, d, h, w), n * d * h * w
    assert ops.stem_wgrad_bn_ok(dims, cin, cout)
    tag = "swbn%s" % (shape,)
    x = O.int_operand(tag + ".x", (n, cin, d, h, w), 0.5)
    y = O.int_operand(tag + ".y", (v, cout), 0.6, 2)
    da = O.int_operand(tag + ".da", (v, cout), 0.6)
    mean, rstd, scale, shift, coef = _bn_consts(tag, cout)
    dyr, _, _ = _bn_bwd_ref(y, da, mean, rstd, scale, shift, coef)
    dyq = O.bf16_rne(dyr)                         # the kernel rounds dy to bf16 where the two-pass path stores it
    O.assert_exact_pre(32 * float(x.abs().max()) * dyq.abs().sum(0), tag + " dw (units of 1/32)")
    dwr = O.wgrad_ref(x, O.uncl(dyq, n, d, h, w), (cout, cin, 3, 3, 3), 1)
    bnbuf = torch.stack([mean, rstd, scale, shift]).cuda()
    dw = _nan((cout, cin, 3, 3, 3))
    ops.stem_wgrad_bn(x.cuda(), y.to(BF).cuda(), da.to(BF).cuda(), bnbuf, torch.tensor([0.25]).cuda(), coef.cuda(), dw, dims, cin,
                      cout, _ws(ops.conv3d_wgrad_ws_bytes(dims, cin, cout, K333)))
    O.assert_exact(dw, dwr, "dw")


# ------------------------------------------------------------------ knob invariance

# knob, values, shape, kind - "fwd": run _run_conv3d_exact, and the plan must change for one of the values; "hidden": the same
# run for a knob fplx_conv3d_plan_query cannot see (block order, tile width); "wg": the same run, the knob picks the
# weight-gradient kernel; "pack": the weight packs against host-built packs, then the same run; "mid": the Conv2d forms;
# "wg-stream": as "wg" with the rolling-window kernel off (knob wg_roll = 0), so that the footprint march these knobs configure
# (conv_wgrad_stream) takes the layer; "deconv" / "stem" / "outconv": those tests' bodies
KNOB_SWEEP = [
    ("xcd", (0,), (1, 32, 32, 9, 16, 64), "hidden"),
    ("pack_tiled", (0,), (1, 64, 32, 7, 24, 64), "pack"),
    ("pack_multi", (0,), (1, 64, 32, 7, 24, 64), "pack"),
    ("brick", (0, 3), (2, 128, 64, 12, 32, 64), "fwd"),
    ("brick_fill", (1, 4096), (2, 256, 128, 8, 32, 32), "fwd"),
    ("brick_geo", (0, 1), (2, 128, 128, 10, 40, 40), "fwd"),
    ("brick_ksplit", (2, 4), (2, 128, 128, 10, 40, 40), "fwd"),
    ("march", (0,), (1, 64, 32, 7, 24, 64), "fwd"),
    ("march64_fw", (16, 32), (1, 64, 32, 7, 24, 64), "fwd"),
    ("march_ds", (2, 3), (1, 32, 32, 12, 16, 64), "fwd"),
    ("march128", (0,), (1, 128, 64, 4, 17, 65), "fwd"),
    ("march32_v2", (0, 1), (1, 32, 32, 9, 16, 64), "fwd"),
    ("tile_nt", (64,), (2, 128, 128, 2, 5, 5), "hidden"),
    ("tile_ks", (1, 3, 9), (2, 128, 128, 2, 5, 5), "fwd"),
    ("rows_small_div", (64,), (2, 16, 8, 4, 6, 10), "wg"),
    ("wg_vox", (0, 2), (1, 64, 64, 9, 33, 17), "wg"),
    ("wg_vox_lw", (0, 2), (3, 32, 96, 3, 7, 9), "wg"),
    ("wg_vox_maxv", (0, 100000), (1, 64, 64, 9, 33, 17), "wg"),
    ("wg_vox_cus", (32, 256), (1, 64, 64, 9, 33, 17), "wg"),
    ("wg_roll", (0,), (2, 32, 64, 7, 20, 70), "wg"),
    ("wg_roll_geo", (1, 2, 3), (2, 32, 64, 7, 20, 70), "wg"),
    ("wg_roll_m16", (0,), (1, 32, 32, 9, 16, 64), "wg"),
    ("wg_roll_mb", (0, 2), (2, 32, 64, 7, 20, 70), "wg"),
    ("wg_roll_cus", (16, 1024), (2, 32, 64, 7, 20, 70), "wg"),
    ("wg_roll_ovh", (0, 64), (2, 32, 64, 7, 20, 70), "wg"),
    ("wg_roll_minvox", (1 << 30,), (2, 32, 64, 7, 20, 70), "wg"),
    ("wg_cit", (1,), (1, 64, 64, 20, 40, 40), "wg-stream"),
    ("wg_cot", (1,), (1, 64, 64, 20, 40, 40), "wg-stream"),
    ("wg_cot_minvox", (1 << 30,), (1, 64, 64, 20, 40, 40), "wg-stream"),
    ("wg_tw", (16, 32), (1, 64, 64, 20, 40, 40), "wg-stream"),
    ("wg_ds", (2,), (1, 64, 64, 20, 40, 40), "wg-stream"),
    ("wg_reduce_rows", (0, 64), (2, 512, 512, 5, 10, 10), "wg"),
    ("mid_tile", (0,), (1, 64, 128, 3, 8, 9), "mid"),
    ("march64_lw", (0,), (1, 128, 64, 5, 16, 64), "mid"),
    ("wg_roll2d", (0,), (1, 32, 32, 5, 16, 64), "mid"),
    ("wg_roll2d_ovh", (0, 64), (1, 32, 32, 5, 16, 64), "mid"),
    ("deconv_rows", (0,), (2, 64, 32, 9, 37, 50), "deconv"),
    ("deconv_dgrad_rows", (0,), (2, 64, 32, 9, 37, 50), "deconv"),
    ("edge_blocks", (1, 4096), (3, 1, 32, 5, 7, 161), "stem"),
    ("stem_rows", (0, 2), (2, 4, 32, 3, 9, 35), "stem"),
    ("outconv_t", (0,), (2, 32, 2, 3, 9, 35), "outconv"),
    ("outconv_dgrad_mfma", (0,), (2, 32, 2, 3, 9, 35), "outconv"),
]


@gpu
@pytest.mark.parametrize("key,values,shape,kind", KNOB_SWEEP, ids=[k[0] for k in KNOB_SWEEP])
def test_no_knob_changes_a_result(key, values, shape, kind, knobs):
    """common.h, FPLX_KNOB_LIST: "no knob changes a result, only which kernel / geometry computes it" - with exact data, at zero
    tolerance, for every value listed; a forward knob must change fplx_conv3d_plan_query's answer (family, geometry, split or
    statistics rows, re-queried under the knob) for one of its values on the shape it runs on"""
    n, cin, cout, d, h, w = shape
    if kind == "wg-stream":
        knobs("wg_roll", 0)
    plans = {plan_kernel(n, d, h, w, cin, cout, full=True)}
    for value in values:
        knobs(key, value)
        plans.add(plan_kernel(n, d, h, w, cin, cout, full=True))
        if kind == "pack":
            _check_packs(cout, cin)
        if kind in ("fwd", "hidden", "wg", "wg-stream", "pack"):
            _run_conv3d_exact(shape)
        elif kind == "mid":
            _run_conv3d_exact(shape, BF, mid=True)
        elif kind == "deconv":
            test_deconv_exact(shape, 2, BF)
        elif kind == "stem":
            test_stem_exact(shape)
        else:
            test_outconv_exact(shape, knobs)
    if kind == "fwd":
        assert len(plans) > 1, (key, plans)


def _check_packs(cout, cin):
    """fplx_pack_conv_weight and fplx_pack_conv_weights_batched against the layouts of include/fplx.h built on the host:
    wf[tap][co][ci] = w[co][ci][tap], wb[tap][ci][co] = w[co][ci][26 - tap] (integer weights: exact in bf16)"""
    from fplx import ops
    wt = O.int_weight("pk%d.%d" % (cout, cin), (cout, cin, 3, 3, 3))
    wf_ref = wt.permute(2, 3, 4, 0, 1).reshape(27, cout, cin)
    wb_ref = wt.flip(2, 3, 4).permute(2, 3, 4, 1, 0).reshape(27, cin, cout)
    for wf, wb in [ops.pack_conv_weight(wt.cuda(), BF)] + ops.pack_conv_weights_batched([wt.cuda()], BF, [True]):
        O.assert_exact(wf, wf_ref, "wf")
        O.assert_exact(wb, wb_ref, "wb")


# ------------------------------------------------------------------ oracle B: rounding bound and bias, real-valued operands

B_CASES = [((1, 5, 7, 3, 9, 6), {}), ((3, 32, 96, 7, 40, 60), {}), ((2, 16, 32, 4, 6, 10), {}), ((2, 32, 64, 8, 40, 60), {}),
           ((2, 128, 128, 2, 5, 5), {}), ((1, 32, 32, 9, 16, 64), {}),
           ((3, 32, 96, 6, 17, 65), {}), ((1, 64, 64, 6, 16, 80), {}), ((1, 64, 32, 7, 24, 64), {}), ((2, 128, 64, 12, 32, 64), {}),
           ((2, 256, 256, 10, 20, 20), {})]


@gpu
@pytest.mark.parametrize("shape,kn", B_CASES, ids=_ids([(s, BF, k) for s, k in B_CASES]))
def test_conv3d_rounding_bound(shape, kn, knobs):
    """oracle B per family: y and dx (bf16) within 2^-8 (|ref| + gamma S) + gamma S element by element and a mean signed error
    within 0.1 ulp; dw (fp32) within gamma S and 1e-4 of its largest entry"""
    from fplx import ops
    for key, value in kn.items():
        knobs(key, value)
    n, cin, cout, d, h, w = shape
    dims, v = (n, d, h, w), n * d * h * w
    tag = "rb%s" % (shape,)
    x = O.real_operand(tag + ".x", (n, cin, d, h, w))
    wt = O.real_operand(tag + ".w", (cout, cin, 3, 3, 3), (2.0 / (27 * cin)) ** 0.5)
    b = O.real_operand(tag + ".b", (cout,), 0.1)
    dy = O.real_operand(tag + ".dy", (n, cout, d, h, w))
    wf, wb = ops.pack_conv_weight(wt.cuda(), BF)
    cls, dt = ops.cl_strides, ops.BF16
    y = _nan((v, cout), BF)
    ops.conv3d_fwd(O.cl(x).to(BF).cuda(), cls(d, h, w, cin), dt, wf, b.cuda(), y, cls(d, h, w, cout), dt, dims, cin, cout, K333, None,
                   _ws(ops.conv3d_fwd_ws_bytes(dims, cin, cout, K333, dt, dt)))
    ry, by = O.check_rounding(y, O.cl(O.conv3d_ref(x, wt, b, 1)), O.cl(O.conv3d_abs(x, wt, b, 1)), cin * 27 + 1, "y")
    dx = _nan((v, cin), BF)
    dyg = O.cl(dy).to(BF).cuda()
    ops.conv3d_fwd(dyg, cls(d, h, w, cout), dt, wb, None, dx, cls(d, h, w, cin), dt, dims, cout, cin, K333, None,
                   _ws(ops.conv3d_fwd_ws_bytes(dims, cout, cin, K333, dt, dt)))
    rx, bx = O.check_rounding(dx, O.cl(O.dgrad_ref(dy, wt, 1)), O.cl(O.dgrad_ref(dy.abs(), wt.abs(), 1)), cout * 27, "dx")
    dw = _nan((cout, cin, 3, 3, 3))
    ops.conv3d_wgrad(O.cl(x).to(BF).cuda(), cls(d, h, w, cin), dt, dyg, cls(d, h, w, cout), dt, dw, None, dims, cin, cout, K333,
                     _ws(ops.conv3d_wgrad_ws_bytes(dims, cin, cout, K333)))
    dwr = O.wgrad_ref(x, dy, wt.shape, 1)
    rw, _ = O.check_rounding(dw, dwr, O.wgrad_ref(x.abs(), dy.abs(), wt.shape, 1), v, "dw", bf16_out=False)
    assert float((dw.cpu().double() - dwr).abs().max()) <= 1e-4 * float(dwr.abs().max())
    print("\nrounding %s %s: y %.3f of the bound, bias %+.4f ulp | dx %.3f, bias %+.4f | dw %.3f" % (
        shape, plan_kernel(n, d, h, w, cin, cout, full=True)[:3], ry, by, rx, bx, rw))


def _report(what, *pairs):
    print("\nrounding %s: %s" % (what, " | ".join("%s %.3f of the bound, bias %+.4f ulp" % p for p in pairs)))


@gpu
@pytest.mark.parametrize("shape", [(2, 1, 32, 3, 9, 35), (2, 4, 64, 3, 10, 48), (1, 1, 32, 5, 16, 64)])
def test_stem_rounding_bound(shape):
    """oracle B on the stem kernels: y (bf16) element by element and its bias, dw (fp32); the kernel rounds its fp32 input to bf16,
    so x is bf16-valued and the reference is formed from it"""
    from fplx import ops
    n, cin, cout, d, h, w = shape
    dims, v = (n, d, h, w), n * d * h * w
    tag = "rbs%s" % (shape,)
    x = O.real_operand(tag + ".x", (n, cin, d, h, w))
    wt = O.real_operand(tag + ".w", (cout, cin, 3, 3, 3), (2.0 / (27 * cin)) ** 0.5)
    b = O.real_operand(tag + ".b", (cout,), 0.1)
    dy = O.real_operand(tag + ".dy", (n, cout, d, h, w))
    wf, _ = ops.pack_conv_weight(wt.cuda(), BF, False)
    y = _nan((v, cout), BF)
    ops.conv3d_fwd(x.cuda(), ops.planar_strides(cin, d, h, w), ops.F32, wf, b.cuda(), y, ops.cl_strides(d, h, w, cout), ops.BF16,
                   dims, cin, cout, K333, None)
    ry = O.check_rounding(y, O.cl(O.conv3d_ref(x, wt, b, 1)), O.cl(O.conv3d_abs(x, wt, b, 1)), cin * 27 + 1, "y")
    dw = _nan((cout, cin, 3, 3, 3))
    ops.conv3d_wgrad(x.cuda(), ops.planar_strides(cin, d, h, w), ops.F32, O.cl(dy).to(BF).cuda(), ops.cl_strides(d, h, w, cout),
                     ops.BF16, dw, None, dims, cin, cout, K333, _ws(ops.conv3d_wgrad_ws_bytes(dims, cin, cout, K333)))
    dwr = O.wgrad_ref(x, dy, wt.shape, 1)
    rw = O.check_rounding(dw, dwr, O.wgrad_ref(x.abs(), dy.abs(), wt.shape, 1), v, "dw", bf16_out=False)
    assert float((dw.cpu().double() - dwr).abs().max()) <= 1e-4 * float(dwr.abs().max())
    _report("stem %s" % (shape,), ("y",) + ry, ("dw",) + rw)


@gpu
@pytest.mark.parametrize("shape", [(2, 32, 2, 3, 9, 35), (1, 64, 3, 2, 16, 64), (1, 16, 4, 3, 15, 33), (1, 32, 2, 4, 24, 40)])
def test_outconv_rounding_bound(shape, knobs):
    """oracle B on out_conv: logits (fp32, within gamma S), dx (bf16, bound and bias), dw (fp32); bf16-valued weights and dlogits
    (the MFMA forms take bf16 operands)"""
    from fplx import ops
    n, c0, ncls, d, h, w = shape
    dims, v = (n, d, h, w), n * d * h * w
    tag = "rbo%s" % (shape,)
    x = O.real_operand(tag + ".x", (n, c0, d, h, w))
    wt = O.real_operand(tag + ".w", (ncls, c0, 1, 3, 3), (2.0 / (9 * c0)) ** 0.5)
    b = O.real_operand(tag + ".b", (ncls,), 0.1)
    dl = O.real_operand(tag + ".dl", (n, ncls, d, h, w))
    conv = lambda a, k, c: torch.nn.functional.conv3d(a.double(), k.double(), None if c is None else c.double(), padding=(0, 1, 1))
    tconv = lambda a, k: torch.nn.functional.conv_transpose3d(a.double(), k.double(), padding=(0, 1, 1))
    wf, _ = ops.pack_conv_weight(wt.cuda(), F32, False)
    _, wb = ops.pack_conv_weight(wt.cuda(), BF, True)
    xg = O.cl(x).to(BF).cuda()
    lg = _nan((n, ncls, d, h, w))
    ops.conv3d_fwd(xg, ops.cl_strides(d, h, w, c0), ops.BF16, wf, b.cuda(), lg, ops.planar_strides(ncls, d, h, w), ops.F32, dims, c0,
                   ncls, (1, 3, 3), None)
    rl = O.check_rounding(lg, conv(x, wt, b), conv(x.abs(), wt.abs(), b.abs()), c0 * 9 + 1, "logits", bf16_out=False)
    dx = _nan((v, c0), BF)
    ops.conv3d_fwd(dl.cuda(), ops.planar_strides(ncls, d, h, w), ops.F32, wb, None, dx, ops.cl_strides(d, h, w, c0), ops.BF16, dims,
                   ncls, c0, (1, 3, 3), None)
    rx = O.check_rounding(dx, O.cl(tconv(dl, wt)), O.cl(tconv(dl.abs(), wt.abs())), ncls * 9, "dx")
    dw = _nan((ncls, c0, 1, 3, 3))
    ops.conv3d_wgrad(xg, ops.cl_strides(d, h, w, c0), ops.BF16, dl.cuda(), ops.planar_strides(ncls, d, h, w), ops.F32, dw, None, dims,
                     c0, ncls, (1, 3, 3), _ws(ops.conv3d_wgrad_ws_bytes(dims, c0, ncls, (1, 3, 3))))
    gw = lambda a, g: torch.nn.grad.conv3d_weight(a.double(), wt.shape, g.double(), padding=(0, 1, 1))
    rw = O.check_rounding(dw, gw(x, dl), gw(x.abs(), dl.abs()), v, "dw", bf16_out=False)
    _report("out_conv %s" % (shape,), ("logits",) + rl, ("dx",) + rx, ("dw",) + rw)


@gpu
@pytest.mark.parametrize("shape,sd", [((2, 64, 32, 9, 37, 50), 2), ((1, 128, 64, 2, 5, 9), 2), ((2, 32, 32, 4, 4, 7), 2),
                                      ((2, 64, 32, 5, 8, 12), 1), ((2, 32, 64, 5, 8, 12), 1)])
def test_deconv_rounding_bound(shape, sd):
    """oracle B on the transposed convolutions (fplx_deconv2_* / fplx_deconv122_*): y and dx (bf16) element by element and their
    bias, dw (fp32)"""
    from fplx import ops
    n, cin, cout, d, h, w = shape
    dims, v = (n, d, h, w), n * d * h * w
    tag = "rbd%s%d" % (shape, sd)
    taps = 4 * sd
    x = O.real_operand(tag + ".x", (n, cin, d, h, w))
    wt = O.real_operand(tag + ".w", (cin, cout, 2, 2, 2) if sd == 2 else (cin, cout, 2, 2), (1.0 / cin) ** 0.5)
    b = O.real_operand(tag + ".b", (cout,), 0.1)
    dy = O.real_operand(tag + ".dy", (n, cout, sd * d, 2 * h, 2 * w))
    w5, stride = (wt if sd == 2 else wt.unsqueeze(2)), (sd, 2, 2)
    F_ = torch.nn.functional
    yref = O.cl(F_.conv_transpose3d(x.double(), w5.double(), b.double(), stride=stride))
    yS = O.cl(F_.conv_transpose3d(x.double().abs(), w5.double().abs(), b.double().abs(), stride=stride))
    dxref = O.cl(F_.conv3d(dy.double(), w5.double(), stride=stride))
    dxS = O.cl(F_.conv3d(dy.double().abs(), w5.double().abs(), stride=stride))
    # dw[ci][co][tap] = sum_v x[ci][v] dy[co][child(v, tap)]: the weight gradient of conv3d(dy) with x as its output gradient
    gw = lambda a, g: torch.nn.grad.conv3d_weight(g.double(), w5.shape, a.double(), stride=stride).view(wt.shape)
    wf, wb = ops.pack_deconv_weight(wt.cuda(), BF)
    xg = O.cl(x).to(BF).cuda()
    y = _nan((n * sd * d * 4 * h * w, cout), BF)
    ops.deconv2_fwd(xg, wf, b.cuda(), y, dims, cin, cout, sd)
    ry = O.check_rounding(y, yref, yS, cin + 1, "y")
    dyg = O.cl(dy).to(BF).cuda()
    dx = _nan((v, cin), BF)
    ops.deconv2_dgrad(dyg, wb, dx, dims, cin, cout, sd)
    rx = O.check_rounding(dx, dxref, dxS, taps * cout, "dx")
    dw = _nan(tuple(wt.shape))
    ops.deconv2_wgrad(xg, dyg, dw, None, dims, cin, cout, _ws(ops.deconv2_wgrad_ws_bytes(dims, cin, cout, sd)), sd)
    rw = O.check_rounding(dw, gw(x, dy), gw(x.abs(), dy.abs()), v, "dw", bf16_out=False)
    _report("deconv sd=%d %s" % (sd, shape), ("y",) + ry, ("dx",) + rx, ("dw",) + rw)


@gpu
@pytest.mark.parametrize("shape,form", [((1, 64, 32, 4, 9, 70), "mid"), ((1, 32, 32, 5, 16, 64), "mid"), ((1, 64, 128, 3, 8, 9), "mid"),
                                        ((1, 64, 32, 16, 32, 64), "cat2"), ((2, 64, 32, 12, 48, 96), "cat2")])
def test_conv2d_and_cat2_rounding_bound(shape, form):
    """oracle B on the 2.5D forms (fplx_conv2d_fwd and its data gradient: a Conv2d pack in the middle depth plane) and on the
    two-tensor forms (fplx_conv3d_fwd_cat2 / _dgrad_split2): y and dx element by element and their bias"""
    from fplx import ops
    n, cin, cout, d, h, w = shape
    dims, v = (n, d, h, w), n * d * h * w
    mid = form == "mid"
    tag = "rb2%s%s" % (shape, form)
    taps = 9 if mid else 27
    x = O.real_operand(tag + ".x", (n, cin, d, h, w))
    wt = O.real_operand(tag + ".w", (cout, cin, 3, 3, 3), (2.0 / (taps * cin)) ** 0.5)
    if mid:
        wt[:, :, 0] = 0
        wt[:, :, 2] = 0
    b = O.real_operand(tag + ".b", (cout,), 0.1)
    dy = O.real_operand(tag + ".dy", (n, cout, d, h, w))
    wf, wb = ops.pack_conv2d_weight(wt[:, :, 1].contiguous().cuda(), BF) if mid else ops.pack_conv_weight(wt.cuda(), BF)
    xg, dyg = O.cl(x).to(BF).cuda(), O.cl(dy).to(BF).cuda()
    y, dx = _nan((v, cout), BF), _nan((v, cin), BF)
    cls, dt = ops.cl_strides, ops.BF16
    if mid:
        ops.conv3d_fwd(xg, cls(d, h, w, cin), dt, wf, b.cuda(), y, cls(d, h, w, cout), dt, dims, cin, cout, K333, None, mid=True)
        ops.conv3d_fwd(dyg, cls(d, h, w, cout), dt, wb, None, dx, cls(d, h, w, cin), dt, dims, cout, cin, K333, None, mid=True)
    else:
        assert ops.conv3d_cat2_ok(dims, cin, cout)
        ops.conv3d_fwd_cat2(xg[:, :32].contiguous(), xg[:, 32:].contiguous(), wf, b.cuda(), y, dims, cin, cout, None)
        dx0, dx1 = _nan((v, 32), BF), _nan((v, 32), BF)
        ops.conv3d_dgrad_split2(dyg, wb, dx0, dx1, dims, cin, cout)
        dx = torch.cat([dx0, dx1], 1)
    ry = O.check_rounding(y, O.cl(O.conv3d_ref(x, wt, b, 1)), O.cl(O.conv3d_abs(x, wt, b, 1)), cin * taps + 1, "y")
    rx = O.check_rounding(dx, O.cl(O.dgrad_ref(dy, wt, 1)), O.cl(O.dgrad_ref(dy.abs(), wt.abs(), 1)), cout * taps, "dx")
    _report("%s %s" % (form, shape), ("y",) + ry, ("dx",) + rx)
