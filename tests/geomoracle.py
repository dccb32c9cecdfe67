"""Oracles for the three kernel families that are pure index arithmetic plus a handful of floating-point operations per output:
plain max-pooling (maxpool2_fwd_k / maxpool2_bwd_k, csrc/elementwise.hip), linear x2 upsampling (csrc/upsample.hip) and the
sliding-window extract / merge of the Inferer (csrc/infer.hip).  tests/test_geom_oracle_cpu.py proves the references on the CPU
(and shows that the upsampling bound rejects wrong kernels); tests/test_gpu_geom_exact.py holds the kernels to them.

1. Max-pooling - bit for bit.  Reference: float64 F.max_pool3d(x, (pd, 2, 2)) and its autograd, dx = grad + dskip rounded once to
   the activation type.  x holds half-integers in [-4, 4] (exact in bf16, many ties: the first maximum of a window wins, in the
   order depth, row, column), dy and dskip integers of magnitude <= 8: the one addition of the backward is an integer of
   magnitude <= 16, exact in fp32 and in bf16, so there is no rounding at all and nothing to tolerate.  +-inf and +-0 are
   covered (the comparison is on the bit patterns, so +0 and -0 differ).  NOT covered: NaN inputs (neither the project nor the
   reference defines them for training: a > b is false for both orders) and the 64-bit index branch of the kernels
   (total >= 2^31 work items: tens of GB).

2. Upsampling - an exact family and a derived bound.
   Exact: when every interpolated axis has length 1 all weights are exactly 1: y is x replicated, dx the sum of the 8 (sd = 2) or
   4 (sd = 1) upstream values, exact on small integers.
   Bound, forward.  Reference: float64 F.interpolate(scale_factor = 2, align_corners = True), trilinear (sd = 2) or bilinear per
   depth slice (sd = 1); T(s) below is its continuous interpolant, s* = o (in - 1) / (out - 1) the exact source coordinate.
   src_of forms scale = fl((in - 1) / (out - 1)) and s = fl(scale o): two roundings, |s - s*| <= (2 u + u^2) s* <= e_a :=
   (2 u + u^2) (in_a - 1) with u = 2^-24.  i0 = (int) s and l1 = s - i0 (exact: both are multiples of ulp(s) and the difference
   is smaller than s; when the compiler contracts scale o - i0 into one fma the product is not rounded first and the result is
   closer still; a clamp of l1 to [0, 1] moves it towards s*), so the kernel evaluates the axis at s_eff = i0 + l1 with
   |s_eff - s*| <= e_a.  Whether s fell on the other side of an integer than s* does not matter: T is continuous there, and on
   either side of the knot the kernel's (i0, i1, l0, l1) describe the same piecewise-linear function.  Moving one axis at a time
   from s* to s_eff changes T by at most e_a times the largest |x[.., i + 1, ..] - x[.., i, ..]| over the segments of axis a and
   the neighbours of the other axes that s* or s_eff can touch (the cell of s*, widened by one index wherever s* lies within e
   of a knot): the coordinate term  C = sum_a e_a G_a.  What is left is the arithmetic at s_eff: l0 = fl(1 - l1), one product and
   one addition per axis and term, k = 3 roundings per interpolated axis (fewer when contracted), so
   |y - T(s_eff)| <= gamma(k) S_eff with S_eff the same interpolation of |x| at s_eff, and S_eff <= S + C because
   | |x_i+1| - |x_i| | <= |x_i+1 - x_i|:
        |y - ref| <= B := gamma(k) (S + C) + C                    (fp32; gamma's unit 2^-23 is twice the round-to-nearest unit)
        |y - ref| <= 2^-8 (|ref| + B) + B                          (bf16: half an ulp of the stored value on top)
   An axis with out == in (depth under sd = 1) or in == 1 has the exact weights 1 and 0: e_a = 0 and it adds nothing to k.
   torch's float32 CPU kernel forms the same two-rounding coordinate and sums eight products of three weights: 3 + 3 + 7 = 13
   roundings of 2^-24 against the 9 x 2^-23 allowed, so it must lie inside the same bound - the CPU file asserts it and records
   how much of the bound it uses.
   Bound, backward.  dx[i] = sum_o w_d w_h w_w dy[o] over the outputs whose weight on i is not zero; the exact weight of output o
   on input i is the hat function max(0, 1 - |s*_o - i|), Lipschitz 1 and continuous across knots, so the kernel's weight obeys
   0 <= w <= w* + e_a 1[|s*_o - i| < 1 + e_a] on every axis.  With S+ the transposed interpolation of |dy| under the widened
   weights w* + e 1 and S the one under w*, the coordinate term is C = S+ - S (exactly the sum over o of |dy| (prod(w* + e 1) -
   prod w*)) and the arithmetic - three weight roundings, three products, and at most n additions for the n = K_d K_h K_w
   candidate terms - gives
        |dx - ref| <= B := gamma(6 + n) S+ + C,                    bf16 as above.
   The transpose check of the GPU file has no coordinate term at all: it extracts the device's own axis weights with one-hot
   forwards and requires dx to lie within gamma(3 + n) of their Kronecker transpose, so an output that the backward's candidate
   window drops is seen whatever the coordinate rounding did.

3. Sliding window - bit for bit.  A numpy restatement of the Inferer's loops as fplx/infer.py and csrc/infer.hip document them:
   per axis the starts min(k stride, size - window) for k stride < size with duplicates kept; tiles enumerated with w outermost,
   then h, then d; output[sl] += patch and counter[sl] += 1 in float32, then output / counter (a single tile is the prediction
   itself, no division); flips (0, 2, 1, 3) = none, H, W, H + W combined as ((o1 + o2) + o3 + o4) / 4.  numpy performs the same
   float32 additions in the same order and the divisions are correctly rounded on both sides, so the results are equal bit
   for bit on any data; on small integers a mismatch can only be an index or coverage error.
"""
import functools
import warnings

import numpy as np
import torch
import torch.nn.functional as F

import detdata
from convoracle import bf16_rne, gamma, rounding_bias, BIAS_LIMIT
from headoracle import ints

def _t(a):
    """a read-only array as a tensor (never written to: the shared data stay as they were generated)"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return torch.from_numpy(a)

# ================================================================ 1. max-pooling

EW_THREADS, EW_GRID_CAP = 256, 4096          # csrc/elementwise.hip: EW_THREADS, ew_grid
VEC = {"fp32": 4, "bf16": 8}                 # csrc/common.h: Vec<T>::N (16-byte accesses)
PAD = 8                                      # ld = C + PAD for a column slice of a wider buffer
POOL_TENSORS = ("x", "y", "dy", "dskip", "dx")


def _pool_cases():
    cases = []
    for pd in (2, 1):
        for dt in ("fp32", "bf16"):
            for c in (5, 8):
                cases.append(dict(pd=pd, dt=dt, n=1, dhw=(pd, 2, 2), c=c, kind="ties"))
                cases.append(dict(pd=pd, dt=dt, n=2, dhw=(4, 6, 8), c=c, kind="ties"))
            for wide in POOL_TENSORS:
                cases.append(dict(pd=pd, dt=dt, n=2, dhw=(4, 6, 8), c=8, kind="ties", wide=(wide,)))
            cases.append(dict(pd=pd, dt=dt, n=2, dhw=(4, 6, 8), c=5, kind="ties", wide=POOL_TENSORS))
            cases.append(dict(pd=pd, dt=dt, n=2, dhw=(4, 6, 8), c=8, kind="ties", misaligned=True))
            cases.append(dict(pd=pd, dt=dt, n=2, dhw=(4, 6, 8), c=8, kind="ties", noskip=True))
            cases.append(dict(pd=pd, dt=dt, n=2, dhw=(4, 6, 8), c=5, kind="ties", noskip=True))
            cases.append(dict(pd=pd, dt=dt, n=1, dhw=(2, 4, 6), c=8, kind="equal"))
            cases.append(dict(pd=pd, dt=dt, n=1, dhw=(2, 4, 6), c=5, kind="equal"))
            cases.append(dict(pd=pd, dt=dt, n=1, dhw=(2, 4, 8), c=8, kind="special"))
            cases.append(dict(pd=pd, dt=dt, n=1, dhw=(2, 4, 8), c=5, kind="special"))
    return cases


POOL_CASES = _pool_cases()
# the grid-stride loop runs a second time when the work items (pooled voxels x channel groups) exceed 4096 x 256
POOL_GRID_CASES = [
    dict(pd=2, dt="fp32", n=1, dhw=(2, 1184, 1184), c=3, kind="ties"),          # VEC = 1: 592 * 592 * 3 = 1 051 392 items
    dict(pd=1, dt="bf16", n=1, dhw=(1, 1184, 1184), c=3, kind="ties", noskip=True),
    dict(pd=1, dt="fp32", n=1, dhw=(4, 1026, 1024), c=4, kind="ties"),          # VEC = 4: 4 * 513 * 512 = 1 050 624 items
]


def pool_items(case):
    """work items of the kernels for this case (pooled voxels x channel groups)"""
    d, h, w = case["dhw"]
    v = VEC[case["dt"]]
    vec = case["c"] % v == 0 and not case.get("misaligned") and (not case.get("wide") or (case["c"] + PAD) % v == 0)
    return case["n"] * (d // case["pd"]) * (h // 2) * (w // 2) * (case["c"] // v if vec else case["c"])


def pool_id(case):
    d, h, w = case["dhw"]
    s = "pd%d_%s_n%d_%dx%dx%d_c%d_%s" % (case["pd"], case["dt"], case["n"], d, h, w, case["c"], case["kind"])
    if case.get("wide"):
        s += "_wide-" + ("all" if len(case["wide"]) > 1 else case["wide"][0])
    if case.get("misaligned"):
        s += "_misaligned"
    if case.get("noskip"):
        s += "_noskip"
    return s


@functools.lru_cache(maxsize=2)
def _pool_data(pd, n, dhw, c, kind):
    d, h, w = dhw
    tag = "pool.%d.%d.%dx%dx%d.%d.%s" % (pd, n, d, h, w, c, kind)
    x = ints(tag + ".x", (n, c, d, h, w), -8, 8) / 2.0
    if kind == "equal":
        x[:] = 1.5                                   # every window a tie of all 8 (4): position 0 takes the gradient
        x[:, :, :, : h // 2] = -2.0
    elif kind == "special":
        # per window column pair (w // 2 = 0..3) along W: -inf among finite values, a window of -inf only, +inf twice (the first
        # wins), and +0 beside -0 in both orders above negative values
        x[..., 0] = -np.inf
        x[..., 2:4] = -np.inf
        x[..., 4] = np.inf
        x[:, :, :, 1::2, 5] = np.inf
        x[..., 6:8] = np.where(x[..., 6:8] > 0, -x[..., 6:8], x[..., 6:8]) - 1.0
        x[:, :, :, 0, 6], x[:, :, :, 0, 7] = 0.0, -0.0
        x[:, :, :, 2, 6], x[:, :, :, 2, 7] = -0.0, 0.0
        x[:, :, :, 3, 6] = 0.0
    dy = ints(tag + ".dy", (n, c, d // pd, h // 2, w // 2), -8, 8)
    dskip = ints(tag + ".ds", (n, c, d, h, w), -8, 8)
    xt = torch.from_numpy(x).requires_grad_(True)
    y = F.max_pool3d(xt, (pd, 2, 2))
    y.backward(torch.from_numpy(dy))
    out = dict(x=x, dy=dy, dskip=dskip, y=y.detach().numpy(), grad=xt.grad.numpy())
    for a in out.values():
        a.setflags(write=False)
    return out


def pool_data(case):
    """float64 arrays (read-only, shared between the cases on the same numbers): x, dy, dskip, y, grad [N, C, ...]"""
    return _pool_data(case["pd"], case["n"], tuple(case["dhw"]), case["c"], case["kind"])


def pool_dx(case, data):
    return data["grad"] if case.get("noskip") else data["grad"] + data["dskip"]


def pool_ref_numpy(x, dy, pd):
    """the same pooling written out: the first maximum in window order (depth, row, column) wins -> y, grad (float64)"""
    n, c, d, h, w = x.shape
    win = [x[:, :, a::pd, b::2, e::2] for a in range(pd) for b in range(2) for e in range(2)]
    best, arg = win[0].copy(), np.zeros(win[0].shape, np.int64)
    for t in range(1, len(win)):
        take = win[t] > best
        best = np.where(take, win[t], best)
        arg = np.where(take, t, arg)
    grad = np.zeros_like(x)
    for t, (a, b, e) in enumerate((a, b, e) for a in range(pd) for b in range(2) for e in range(2)):
        grad[:, :, a::pd, b::2, e::2] = np.where(arg == t, dy, 0.0)
    return best, grad


def bits(t):
    """the bit patterns of a float32 / bfloat16 / float64 tensor as integers (so that +0 and -0, and NaNs, compare as written)"""
    t = t.detach().cpu().contiguous()
    return t.view({torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float64: torch.int64}[t.dtype])


def assert_bits(got, want64, what):
    """got (fp32 | bf16 tensor) equals the float64 array want64, converted exactly to got's type, bit for bit"""
    want = torch.from_numpy(np.ascontiguousarray(want64))
    w = want.to(got.dtype)
    assert torch.equal(w.double(), want) or bool(torch.isnan(want).any()), "%s: the reference is not exact in %s" % (what, got.dtype)
    g, w = bits(got), bits(w)
    assert g.shape == w.shape, (what, tuple(g.shape), tuple(w.shape))
    bad = g != w
    nbad = int(bad.sum())
    if nbad:
        idx = int(bad.flatten().nonzero()[0, 0])
        raise AssertionError("%s: %d of %d elements differ in their bits (first at flat index %d: got %r, want %r)" % (
            what, nbad, g.numel(), idx, float(got.detach().cpu().flatten()[idx]), float(want.flatten()[idx])))


def to_cl(a):
    """[N, C, D, H, W] array -> [V, C] channels-last array"""
    return np.ascontiguousarray(np.moveaxis(a, 1, -1)).reshape(-1, a.shape[1])


def from_cl(a2, n, dhw):
    return np.moveaxis(a2.reshape((n,) + tuple(dhw) + (-1,)), -1, 1)


# ================================================================ 2. upsampling

UP_THREADS, UP_GRID_CAP = 256, 16384         # csrc/upsample.hip: UP_THREADS, up_grid
U32 = 2.0 ** -24
E_COORD = 2.0 * U32 + U32 * U32              # |s - s*| <= E_COORD s* after the two roundings of src_of

# (n, (D, H, W), C, ld) x sd x dtype; which = "both" | "fwd" | "bwd"
_UP_SHAPES = [(1, (1, 1, 1), 1, 1), (2, (3, 5, 4), 6, 6), (1, (2, 7, 13), 5, 8), (1, (1, 2, 97), 3, 3), (1, (1, 33, 2), 3, 3)]
UP_CASES = [dict(n=n, dhw=dhw, c=c, ld=ld, sd=sd, dt=dt, which="both")
            for (n, dhw, c, ld) in _UP_SHAPES for sd in (2, 1) for dt in ("fp32", "bf16")]
UP_CASES += [
    dict(n=1, dhw=(4, 128, 257), c=4, ld=4, sd=2, dt="fp32", which="fwd"),      # 8 * 131 584 * 4 = 4 210 688 outputs > 16384 * 256
    dict(n=1, dhw=(2, 724, 725), c=4, ld=4, sd=1, dt="fp32", which="bwd"),      # 2 * 524 900 * 4 = 4 199 200 inputs  > 16384 * 256
]
# every interpolated axis of length 1: all weights are 1
UP_EXACT_CASES = [dict(n=2, dhw=dhw, c=5, ld=8, sd=sd, dt=dt) for sd, dhw in ((2, (1, 1, 1)), (1, (3, 1, 1))) for dt in ("fp32", "bf16")]
# backward shapes of the transpose check (axis lengths 2, 3, 13, 97 on every axis the backward walks)
UP_TRANSPOSE_CASES = [(2, (2, 3, 13), 2), (1, (3, 13, 2), 2), (1, (13, 2, 3), 2), (1, (2, 97, 3), 2), (2, (1, 2, 97), 1), (1, (2, 3, 97), 2)]
UP_TRANSPOSE_LENGTHS = (2, 3, 13, 97)
FWD_MUTANTS = ("align_corners_false", "l0_l1_swapped", "i1_not_clamped")
BWD_MUTANTS = ("align_corners_false", "skips_last_output", "window_too_narrow")
SEPARATION = 10.0


def up_id(case):
    d, h, w = case["dhw"]
    s = "sd%d_%s_n%d_%dx%dx%d_c%d_ld%d" % (case["sd"], case["dt"], case["n"], d, h, w, case["c"], case["ld"])
    return s + ("" if case.get("which", "both") == "both" else "_" + case["which"])


def up_out_dims(case):
    d, h, w = case["dhw"]
    return (d * case["sd"], 2 * h, 2 * w)


def up_items(case, which):
    """work items of the forward (outputs) / backward (inputs) kernel"""
    dims = up_out_dims(case) if which == "fwd" else case["dhw"]
    return case["n"] * dims[0] * dims[1] * dims[2] * case["c"]


def _act_valued(a, dt):
    return bf16_rne(a).numpy() if dt == "bf16" else a.astype(np.float64)


@functools.lru_cache(maxsize=2)
def _up_data(key, n, dhw, c, sd, dt, which):
    out = {}
    if which in ("both", "fwd"):
        out["x"] = _act_valued(detdata.normal("up.%s.x" % key, (n, c) + dhw), dt)
    if which in ("both", "bwd"):
        out["dy"] = _act_valued(detdata.normal("up.%s.dy" % key, (n, c, dhw[0] * sd, 2 * dhw[1], 2 * dhw[2])), dt)
    for a in out.values():
        a.setflags(write=False)
    return out


def up_data(case):
    """float64 arrays x [N, C, D, H, W] and / or dy [N, C, Do, Ho, Wo] (bf16-valued for a bf16 case), read-only"""
    return _up_data(up_id(case), case["n"], tuple(case["dhw"]), case["c"], case["sd"], case["dt"], case.get("which", "both"))


def _interp(x, sd, align=True):
    n, c, d, h, w = x.shape
    if sd == 2:
        return F.interpolate(x, scale_factor=2, mode="trilinear", align_corners=align)
    y = F.interpolate(x.transpose(1, 2).reshape(n * d, c, h, w), scale_factor=2, mode="bilinear", align_corners=align)
    return y.reshape(n, d, c, 2 * h, 2 * w).transpose(1, 2)


def up_torch(x, dy, sd, dtype=torch.float64, align=True):
    """F.interpolate and its autograd in `dtype` on the CPU -> (y | None, dx | None) as float64 arrays"""
    y = dx = None
    if x is not None:
        with torch.no_grad():
            y = _interp(_t(x).to(dtype), sd, align).double().numpy()
    if dy is not None:
        n, c, do, ho, wo = dy.shape
        xin = torch.zeros((n, c, do // sd, ho // 2, wo // 2), dtype=dtype, requires_grad=True)
        _interp(xin, sd, align).backward(_t(dy).to(dtype))
        dx = xin.grad.double().numpy()
    return y, dx


def _axes(dhw, sd):
    return [(2, dhw[0], dhw[0] * sd), (3, dhw[1], 2 * dhw[1]), (4, dhw[2], 2 * dhw[2])]


def _interpolated(n_in, n_out):
    return n_in > 1 and n_out != n_in


def axis_table(n_in, n_out):
    """the exact source coordinates of one axis, align_corners = True -> i0, i1, l0, l1, s (float64 / int arrays over o)"""
    o = np.arange(n_out)
    if n_out == n_in:
        return o, o, np.ones(n_out), np.zeros(n_out), o.astype(np.float64)
    s = (o * (n_in - 1)) / float(n_out - 1) if n_out > 1 else np.zeros(n_out)
    i0 = np.minimum(np.floor(s).astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = s - i0
    return i0, i1, 1.0 - l1, l1, s


def _bcast(v, axis, ndim=5):
    shape = [1] * ndim
    shape[axis] = -1
    return np.asarray(v).reshape(shape)


def up_forward_own(x, sd, swap=False):
    """the interpolation written out from axis_table, one axis at a time (swap: the mutant with l0 and l1 exchanged)"""
    y = x
    for axis, n_in, n_out in _axes(x.shape[2:], sd):
        i0, i1, l0, l1, _ = axis_table(n_in, n_out)
        if swap and _interpolated(n_in, n_out):
            l0, l1 = l1, l0
        y = _bcast(l0, axis) * np.take(y, i0, axis) + _bcast(l1, axis) * np.take(y, i1, axis)
    return y


def up_forward_unclamped(x, sd):
    """mutant: i1 = i0 + 1 without the clamp at the upper border, on the channels-last voxel list followed by a NaN guard row -
    it reads the next row (weight exactly 0: invisible on finite data) and, for the last voxel, the guard"""
    n, c, d, h, w = x.shape
    flat = np.concatenate([to_cl(x), np.full((1, c), np.nan)], 0)
    vmax = flat.shape[0] - 1
    tabs = [axis_table(n_in, n_out) for _, n_in, n_out in _axes((d, h, w), sd)]
    do, ho, wo = (len(t[0]) for t in tabs)
    strides = (h * w, w, 1)
    corners = []                                                     # per axis: [(offset over o, weight over o)] x 2
    for (i0, i1, l0, l1, _), st, (_, n_in, n_out) in zip(tabs, strides, _axes((d, h, w), sd)):
        j1 = i0 + 1 if n_out != n_in else i1
        corners.append(((i0 * st, l0), (j1 * st, l1)))
    y = np.zeros((n, do, ho, wo, c))
    base = (np.arange(n) * d * h * w).reshape(n, 1, 1, 1)
    for od, wd_ in corners[0]:
        for oh, wh_ in corners[1]:
            for ow, ww_ in corners[2]:
                idx = base + od.reshape(1, -1, 1, 1) + oh.reshape(1, 1, -1, 1) + ow.reshape(1, 1, 1, -1)
                wt = wd_.reshape(1, -1, 1, 1) * wh_.reshape(1, 1, -1, 1) * ww_.reshape(1, 1, 1, -1)
                with np.errstate(invalid="ignore"):
                    y += wt[..., None] * flat[np.minimum(idx, vmax)]
    return np.moveaxis(y, -1, 1)


def _reach(n_in, n_out):
    """index range [lo, hi] of the inputs of one axis that output o can touch at s* or at any s_eff within e of it, and e"""
    i0, i1, _, _, s = axis_table(n_in, n_out)
    if not _interpolated(n_in, n_out):
        return i0, i1, 0.0
    e = E_COORD * (n_in - 1)
    j = i0
    f = s - j
    lo = np.where((f <= e) & (j > 0), j - 1, j)
    hi = np.minimum(j + 1 + (1.0 - f <= e), n_in - 1)
    return lo, hi, e


def _range_max(a, axis, lo, hi):
    out = np.take(a, lo, axis)
    for t in range(1, int((hi - lo).max()) + 1):
        out = np.maximum(out, np.take(a, np.minimum(lo + t, hi), axis))
    return out


def up_k_fwd(dhw, sd):
    return 3 * sum(_interpolated(a, b) for _, a, b in _axes(dhw, sd))


def up_fwd_bound(x, ref, sd, bf16):
    """per-element bound on |y - ref| (module docstring, section 2) -> float64 array like ref"""
    axes = _axes(x.shape[2:], sd)
    reach = [_reach(a, b) for _, a, b in axes]
    S = up_forward_own(np.abs(x), sd)
    C = np.zeros_like(S)
    for (axis, n_in, n_out), (_, _, e) in zip(axes, reach):
        if e == 0.0:
            continue
        g = np.abs(np.diff(x, axis=axis))
        for (axis_b, _, _), (lo, hi, _) in zip(axes, reach):
            g = _range_max(g, axis_b, lo, hi - 1) if axis_b == axis else _range_max(g, axis_b, lo, hi)
        C += e * g
    b32 = gamma(up_k_fwd(x.shape[2:], sd)) * (S + C) + C if up_k_fwd(x.shape[2:], sd) else C
    return 2.0 ** -8 * (np.abs(ref) + b32) + b32 if bf16 else b32


def _bwd_table(n_in, n_out):
    """candidate outputs of every input of one axis -> idx [in, K], exact hat weights wt [in, K], mask [in, K] of the
    candidates (|s* - i| < 1 + e), e"""
    _, _, _, _, s = axis_table(n_in, n_out)
    if n_out == n_in:
        return np.arange(n_in)[:, None], np.ones((n_in, 1)), np.ones((n_in, 1), bool), 0.0
    e = E_COORD * (n_in - 1) if n_in > 1 else 0.0
    dist = np.abs(s[None, :] - np.arange(n_in)[:, None])              # [in, out] (small: axis lengths only)
    cand = dist < 1.0 + e
    first = cand.argmax(1)
    K = int(cand.sum(1).max())
    idx = np.minimum(first[:, None] + np.arange(K)[None, :], n_out - 1)
    mask = (first[:, None] + np.arange(K)[None, :] < n_out) & np.take_along_axis(cand, idx, 1)
    wt = np.where(mask, np.maximum(0.0, 1.0 - np.take_along_axis(dist, idx, 1)), 0.0)
    return idx, wt, mask, e


def _apply_T(a, axis, idx, wt):
    out = 0.0
    for k in range(idx.shape[1]):
        if np.any(wt[:, k] != 0.0):
            out = out + _bcast(wt[:, k], axis) * np.take(a, idx[:, k], axis)
    return out


def up_backward_own(dy, sd, mutant=None, widen=False):
    """the transposed interpolation written out from the hat weights (mutant: 'skips_last_output' - no input hears the last
    output of an interpolated axis; 'window_too_narrow' - every input loses the last output of its support; widen: the
    weights w* + e 1 of the bound)"""
    dx = dy
    n, c, do, ho, wo = dy.shape
    for axis, n_in, n_out in _axes((do // sd, ho // 2, wo // 2), sd):
        idx, wt, mask, e = _bwd_table(n_in, n_out)
        if widen:
            wt = wt + e * mask
        if n_out != n_in and mutant == "skips_last_output":
            wt = np.where(idx == n_out - 1, 0.0, wt)
        if n_out != n_in and mutant == "window_too_narrow":
            last = (wt.shape[1] - 1) - (wt[:, ::-1] > 0).argmax(1)
            wt = wt.copy()
            wt[np.arange(n_in), last] = 0.0
        dx = _apply_T(dx, axis, idx, wt)
    return dx


def up_n_bwd(dhw, sd):
    """candidate terms of one input: the product over the axes of the largest candidate count"""
    n = 1
    for _, a, b in _axes(dhw, sd):
        n *= _bwd_table(a, b)[0].shape[1]
    return n


def up_bwd_bound(dy, ref, sd, bf16):
    """per-element bound on |dx - ref| (module docstring, section 2)"""
    n, c, do, ho, wo = dy.shape
    dhw = (do // sd, ho // 2, wo // 2)
    a = np.abs(dy)
    S = up_backward_own(a, sd)
    Sp = up_backward_own(a, sd, widen=True)
    b32 = gamma(6 + up_n_bwd(dhw, sd)) * Sp + (Sp - S)
    return 2.0 ** -8 * (np.abs(ref) + b32) + b32 if bf16 else b32


def up_mutant_fwd(name, x, sd):
    if name == "align_corners_false":
        return up_torch(x, None, sd, align=False)[0]
    if name == "l0_l1_swapped":
        return up_forward_own(x, sd, swap=True)
    return up_forward_unclamped(x, sd)


def up_mutant_bwd(name, dy, sd):
    if name == "align_corners_false":
        return up_torch(None, dy, sd, align=False)[1]
    return up_backward_own(dy, sd, mutant=name)


def ratio(got, ref, bound):
    """max over the elements of |got - ref| / bound, 0 where both vanish, inf for a NaN or an error against a zero bound"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max())


def check_bf16_bias(got, ref, what):
    b = rounding_bias(torch.from_numpy(np.asarray(got, np.float64)), torch.from_numpy(np.asarray(ref, np.float64)))
    assert abs(b) <= BIAS_LIMIT, "%s: rounding bias %.3f ulp (round-to-nearest-even gives ~0, truncation ~ -0.5)" % (what, b)
    return b


def up_exact_data(case):
    """float64 small integers: x [N, C, D, H, W] in -8..8, dy [N, C, Do, Ho, Wo] in -4..4 (a sum of 8 stays below 2^6: exact in bf16)"""
    tag = "upx." + up_id(case)
    dhw = case["dhw"]
    return dict(x=ints(tag + ".x", (case["n"], case["c"]) + dhw, -8, 8),
                dy=ints(tag + ".dy", (case["n"], case["c"]) + up_out_dims(case), -4, 4))


def up_exact_ref(case, d):
    sd = case["sd"]
    y = d["x"].repeat(sd, 2).repeat(2, 3).repeat(2, 4)
    n, c, do, ho, wo = d["dy"].shape
    dx = d["dy"].reshape(n, c, do // sd, sd, 1, 2, 1, 2).sum((3, 5, 7))
    return y, dx


def kron_transpose(dy, sd, weights):
    """dx and the same sum on magnitudes under the per-axis weight matrices weights[length] [2 length, length] (float64)"""
    n, c, do, ho, wo = dy.shape
    mats = []
    for _, n_in, n_out in _axes((do // sd, ho // 2, wo // 2), sd):
        mats.append(np.eye(n_in) if n_out == n_in else (np.ones((2, 1)) if n_in == 1 else weights[n_in]))
    dx = np.einsum("ncxyz,xd,yh,zw->ncdhw", dy, *mats, optimize=True)
    S = np.einsum("ncxyz,xd,yh,zw->ncdhw", np.abs(dy), *[np.abs(m) for m in mats], optimize=True)
    nterm = 1
    for m in mats:
        nterm *= int((m != 0).sum(0).max())
    return dx, S, nterm


# ================================================================ 3. sliding window

SW_THREADS, SW_GRID_CAP, SW_MAX = 256, 8192, 64      # csrc/infer.hip
FLIPS_TTA = (0, 2, 1, 3)                             # none, H, W, H + W (bit 0: W flipped, bit 1: H flipped)

# name -> image (d, h, w), window, stride
SW_PLANS = {
    "no_overlap": ((8, 12, 16), (4, 6, 8), (4, 6, 8)),
    "dup_last": ((6, 32, 12), (6, 16, 8), (6, 8, 4)),                  # h: 0, 8, 16, 16
    "dup_repeated": ((4, 6, 20), (2, 6, 16), (2, 6, 4)),               # w: 0, 4, 4, 4, 4
    "window_is_size_2axes": ((5, 7, 12), (5, 7, 8), (5, 7, 3)),        # w: 0, 3, 4, 4
    "window_1": ((3, 5, 8), (1, 5, 4), (1, 5, 4)),                     # d: window 1
    "ragged_all": ((7, 9, 11), (4, 4, 4), (3, 2, 3)),
    "tiles_64": ((2, 3, 64), (2, 3, 1), (2, 3, 1)),                    # 64 tiles on w: the limit
    "single_tile": ((3, 5, 8), (3, 5, 8), (3, 5, 8)),                  # W % 4 == 0: the whole-image path with aligned pointers
    "single_tile_w7": ((3, 5, 7), (3, 5, 7), (3, 5, 7)),
}
SW_CASES = [(name, tta) for name in SW_PLANS for tta in (0, 1)]
# element counts above 8192 * 256 = 2 097 152
SW_BIG_EXTRACT = dict(n=2, c=3, dhw=(8, 64, 64), window=(8, 32, 32), stride=(8, 16, 16), tta=1)        # 4 * 16 * 6 * 8192 = 3 145 728
SW_BIG_MERGE = dict(n=2, c=2, dhw=(16, 192, 192), window=(16, 96, 128), stride=(16, 96, 64), tta=0)     # 4 * 589 824 = 2 359 296
SW_BIG_WHOLE = dict(n=1, c=2, dhw=(16, 512, 516), window=(16, 512, 516), stride=(16, 512, 516), tta=1)  # 8 454 144 / 4 > 2 097 152


def sw_id(case):
    return "%s_tta%d" % case


def axis_starts(size, window, stride):
    return [min(k, size - window) for k in range(0, size, stride)]


def sw_starts(dhw, window, stride):
    """as Inferer._plan: the window is capped by the image, the stride by the window; a window that covers the image is one tile"""
    window = [min(a, b) for a, b in zip(window, dhw)]
    stride = [min(a, b) for a, b in zip(stride, window)]
    if all(a >= b for a, b in zip(window, dhw)):
        return window, [[0], [0], [0]]
    return window, [axis_starts(s, a, b) for s, a, b in zip(dhw, window, stride)]


def sw_flips(tta):
    return FLIPS_TTA if tta else (0,)


def _flip(a, f):
    if f & 2:
        a = a[..., ::-1, :]
    if f & 1:
        a = a[..., ::-1]
    return a


def sw_tiles(starts):
    return [(a, b, c) for c in starts[2] for b in starts[1] for a in starts[0]]


def sw_extract_ref(image, starts, window, flips):
    """-> [flips][tiles][n][c][wd][wh][ww] float32"""
    n, c = image.shape[:2]
    tiles = sw_tiles(starts)
    out = np.empty((len(flips), len(tiles), n, c) + tuple(window), np.float32)
    for fi, f in enumerate(flips):
        img = _flip(image, f)
        for ti, (a, b, e) in enumerate(tiles):
            out[fi, ti] = img[:, :, a:a + window[0], b:b + window[1], e:e + window[2]]
    return out


def sw_merge_ref(patches, dhw, starts, window, flips):
    """patches [flips][tiles][n][k][wd][wh][ww] float32 -> [n][k][d][h][w] float32, the reference's additions in its order"""
    patches = np.asarray(patches, np.float32)
    n, k = patches.shape[2:4]
    tiles = sw_tiles(starts)
    res = []
    for fi, f in enumerate(flips):
        if len(tiles) == 1:
            o = patches[fi, 0]
        else:
            output = np.zeros((n, k) + tuple(dhw), np.float32)
            counter = np.zeros((n, k) + tuple(dhw), np.float32)
            for ti, (a, b, e) in enumerate(tiles):
                sl = (slice(None), slice(None), slice(a, a + window[0]), slice(b, b + window[1]), slice(e, e + window[2]))
                output[sl] += patches[fi, ti]
                counter[sl] += np.float32(1.0)
            o = output / counter
        res.append(_flip(o, f))
    if len(flips) == 1:
        return np.ascontiguousarray(res[0])
    return ((res[0] + res[1]) + res[2] + res[3]) / np.float32(4.0)


def sw_mc_layout(per_pass, chunk):
    """per_pass [passes][nb][...] -> the prediction buffer [chunks][passes][patches of the chunk][...] flattened to [passes nb][...]"""
    passes, nb = per_pass.shape[:2]
    parts = []
    for b0 in range(0, nb, chunk):
        for q in range(passes):
            parts.append(per_pass[q, b0:b0 + chunk])
    return np.ascontiguousarray(np.concatenate(parts, 0))


def sw_image(tag, n, c, dhw, kind):
    shape = (n, c) + tuple(dhw)
    if kind == "int":
        return ints("sw.%s.int" % tag, shape, -8, 8).astype(np.float32)
    return detdata.normal("sw.%s.real" % tag, shape)


def toy_patches(patches, classes):
    """the toy network x -> 2 x + 1 on the one image channel, repeated to `classes` channels, in float32"""
    o = np.float32(2.0) * patches + np.float32(1.0)
    return np.repeat(o, classes, axis=3)


def toy_inferer_ref(image, cfg):
    """what Inferer(cfg).run(toy, image) must return, from the loops above"""
    dhw = image.shape[2:]
    if cfg.get("sliding_window_enable", False):
        window, starts = sw_starts(dhw, cfg["sliding_window_size"], cfg["sliding_window_stride"])
    else:
        window, starts = list(dhw), [[0], [0], [0]]
    flips = sw_flips(cfg.get("tta_mode", 0))
    p = toy_patches(sw_extract_ref(image, starts, window, flips), cfg["class_num"])
    return sw_merge_ref(p, dhw, starts, window, flips)


class Toy(torch.nn.Module):
    """x -> 2 x + 1 repeated to `classes` channels: exact on small integers, one output tensor"""

    def __init__(self, classes):
        super().__init__()
        self.classes = classes
        self.calls = []

    def forward(self, x, domain_label=None):
        self.calls.append(int(x.shape[0]))
        return (2.0 * x + 1.0).repeat(1, self.classes, 1, 1, 1)


INFERER_CASES = {
    # name -> (n, (d, h, w), cfg, train mode)
    "overlap_tta1": (2, (6, 32, 12), dict(sliding_window_enable=True, sliding_window_size=[6, 16, 8], sliding_window_stride=[6, 8, 4],
                                           tta_mode=1, class_num=3), False),
    "ragged_chunks": (2, (6, 32, 12), dict(sliding_window_enable=True, sliding_window_size=[6, 16, 8], sliding_window_stride=[6, 8, 4],
                                            tta_mode=1, class_num=2, infer_batch_voxels=6 * 16 * 8 * 10), False),
    "train_mode": (2, (7, 9, 11), dict(sliding_window_enable=True, sliding_window_size=[4, 4, 4], sliding_window_stride=[3, 2, 3],
                                        tta_mode=0, class_num=2), True),
    "no_window_tta1": (2, (3, 5, 8), dict(sliding_window_enable=False, tta_mode=1, class_num=2), False),
}
