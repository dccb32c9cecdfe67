"""The plain max-pooling kernels, the x2 upsampling kernels and the sliding-window extract / merge kernels against the oracles of
tests/geomoracle.py: bit for bit where the arithmetic is exact (pooling, the length-1 upsampling family, the sliding window), a
derived rounding bound otherwise (upsampling on real data; every case prints its largest error / bound, and with
FPLX_RATIO_LOG=<file> the same lines are written there).  Every output lives in a buffer poisoned with NaN - the columns beyond C
of a wide buffer, one guard row (or 64 guard floats) before and after it - and must leave the poison alone.

What each test reaches:
  test_maxpool_*                 maxpool2_fwd_k / maxpool2_bwd_k <float, 4 | 1> and <bf16_t, 8 | 1>, pd = 2 and 1: ld == C, ld = C + 8
                                 for each tensor in turn (a column slice at offset 8), a pointer one element off 16 bytes (VEC = 1
                                 on the numbers of the vector run), dskip == nullptr, ties, +-inf, +-0, the grid-stride loop
  test_upsample_*                upsample2_fwd_k / upsample2_bwd_k <float | bf16_t>, sd = 2 and 1: ld > C on both sides, axes of
                                 length 1, a 97 -> 194 axis, the grid-stride loop, the backward's candidate window against the
                                 device's own forward weights
  test_sw_*, test_inferer_*      sw_extract_k (n = 2, c = 3), sw_merge_k, sw_merge_whole_k: duplicated starts, 64 tiles, flips,
                                 Monte-Carlo passes with a ragged last chunk, the grid-stride loops, Inferer.run / run_mc
NOT reached: NaN inputs (undefined on both sides) and the 64-bit index branch of the pooling kernels (2^31 work items)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import geomoracle as O

pytestmark = pytest.mark.gpu

_DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
NAN = float("nan")
_LINES = []


@pytest.fixture(scope="module", autouse=True)
def _ratio_log():
    yield
    path = os.environ.get("FPLX_RATIO_LOG")
    if path and _LINES:
        with open(path, "a") as f:
            f.write("\n".join(_LINES) + "\n")


def _log(case, res):
    line = "%-44s %s" % (case, "  ".join("%s %.3g" % kv for kv in sorted(res.items())))
    print(line)
    _LINES.append(line)


class Buf(object):
    """a [rows, c] view at column `off` of rows 1 .. rows of a NaN-filled [rows + 2, ld] device buffer (one guard row before and
    one after), optionally starting one element off a 16-byte boundary"""

    def __init__(self, rows, c, dtype, ld=None, off=0, misaligned=False, data=None):
        ld = c if ld is None else ld
        assert off + c <= ld
        self.flat = torch.full(((rows + 2) * ld + 16,), NAN, dtype=dtype, device="cuda")
        assert self.flat.data_ptr() % 16 == 0
        s = 1 if misaligned else 0
        self.whole = self.flat[s:s + (rows + 2) * ld].view(rows + 2, ld)
        self.view = self.whole[1:rows + 1, off:off + c]
        self.rows, self.c, self.off = rows, c, off
        if data is not None:
            self.view.copy_(torch.from_numpy(np.array(data)).to(dtype))          # a copy: the shared data are read-only

    def assert_guards(self, what):
        keep = torch.ones(self.whole.shape, dtype=torch.bool, device="cuda")
        keep[1:self.rows + 1, self.off:self.off + self.c] = False
        assert bool(torch.isnan(self.whole[keep]).all()), "%s: written outside the result" % what
        n = self.whole.numel()
        assert bool(torch.isnan(self.flat[:1]).all()) and bool(torch.isnan(self.flat[n + 1:]).all()), what
        assert not bool(torch.isnan(self.view).any()), "%s: not every element of the result was written" % what

    def host(self):
        return self.view.detach().cpu().contiguous()


# ================================================================ max-pooling

def _run_pool(case, d, misaligned):
    """-> (y, dx) host tensors [V, C] of the activation type, guards checked"""
    from fplx import ops
    n, (dd, h, w), c, pd, dtype = case["n"], case["dhw"], case["c"], case["pd"], _DT[case["dt"]]
    wide = case.get("wide", ())
    v, vo = n * dd * h * w, n * (dd // pd) * (h // 2) * (w // 2)

    def buf(name, rows, data=None):
        return Buf(rows, c, dtype, c + O.PAD if name in wide else c, O.PAD if name in wide else 0, misaligned, data)

    x = buf("x", v, O.to_cl(d["x"]))
    y = buf("y", vo)
    dy = buf("dy", vo, O.to_cl(d["dy"]))
    dskip = None if case.get("noskip") else buf("dskip", v, O.to_cl(d["dskip"]))
    dx = buf("dx", v)
    el = x.view.element_size()
    if c % O.VEC[case["dt"]] == 0:       # the vector kernel unless a pointer is off: make sure the buffers are what the case says
        for b in (x, y, dy, dskip, dx):
            assert b is None or b.view.data_ptr() % 16 == (el if misaligned else 0)
    dims = (n, dd, h, w)
    ops.maxpool2_fwd(x.view, y.view, dims, c, pd)
    ops.maxpool2_bwd(x.view, dy.view, None if dskip is None else dskip.view, dx.view, dims, c, pd)
    torch.cuda.synchronize()
    y.assert_guards("y")
    dx.assert_guards("dx")
    return y.host(), dx.host()


def _check_pool(case):
    d = O.pool_data(case)
    y, dx = _run_pool(case, d, bool(case.get("misaligned")))
    O.assert_bits(y, O.to_cl(d["y"]), "y")
    O.assert_bits(dx, O.to_cl(O.pool_dx(case, d)), "dx")
    return d, y, dx


@pytest.mark.parametrize("case", O.POOL_CASES, ids=O.pool_id)
def test_maxpool_equals_float64_bit_for_bit(case):
    d, y, dx = _check_pool(case)
    if case.get("misaligned"):           # the scalar fallback on the numbers of the vector run: the same bits
        y2, dx2 = _run_pool(case, d, False)
        assert torch.equal(O.bits(y), O.bits(y2)) and torch.equal(O.bits(dx), O.bits(dx2))


@pytest.mark.parametrize("case", O.POOL_GRID_CASES, ids=O.pool_id)
def test_maxpool_grid_stride_loop(case):
    assert O.pool_items(case) > O.EW_GRID_CAP * O.EW_THREADS
    _check_pool(case)


def test_maxpool_refusals():
    """FPLX_E_BADSHAPE (-1) before any launch: odd H or W, D % pd != 0, a leading dimension smaller than C - both entry points"""
    from fplx import _lib
    lib = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    n, d, h, w, c = 1, 4, 6, 8, 8
    x = torch.zeros((n * d * h * w, c), device="cuda")
    y = torch.full((n * d * h * w, c), 7.0, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for pd, fwd, bwd in ((2, lib.fplx_maxpool2_fwd, lib.fplx_maxpool2_bwd), (1, lib.fplx_maxpool122_fwd, lib.fplx_maxpool122_bwd)):
        shapes = [(d, 5, w), (d, h, 7), (d, 1, w), (d, h, 0)] + ([(3, h, w), (1, h, w)] if pd == 2 else [(0, h, w)])
        for (d_, h_, w_) in shapes:
            assert fwd(p(x), c, p(y), c, n, d_, h_, w_, c, 0, st) == -1, (pd, d_, h_, w_)
            assert bwd(p(x), c, p(x), c, p(x), c, p(y), c, n, d_, h_, w_, c, 0, st) == -1, (pd, d_, h_, w_)
        for lds in ((c - 1, c), (c, c - 1)):
            assert fwd(p(x), lds[0], p(y), lds[1], n, d, h, w, c, 0, st) == -1
        for k in range(4):
            lds = [c - 1 if j == k else c for j in range(4)]
            assert bwd(p(x), lds[0], p(x), lds[1], p(x), lds[2], p(y), lds[3], n, d, h, w, c, 0, st) == -1, (pd, k)
            assert "leading dimension" in _lib.last_error()
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    # without dskip its leading dimension means nothing
    assert lib.fplx_maxpool2_bwd(p(x), c, p(x), c, None, 0, p(y), c, n, d, h, w, c, 0, st) == 0
    torch.cuda.synchronize()
    assert bool((y == 0.0).all())


# ================================================================ upsampling

def _run_up(case, x=None, dy=None):
    """-> (y, dx) float64 arrays [N, C, ...] (None where the side was not asked for), guards checked"""
    from fplx import ops
    n, dhw, c, ld, sd, dtype = case["n"], case["dhw"], case["c"], case["ld"], case["sd"], _DT[case["dt"]]
    odims = O.up_out_dims(case)
    v, vo = n * dhw[0] * dhw[1] * dhw[2], n * odims[0] * odims[1] * odims[2]
    dims = (n,) + tuple(dhw)
    y = dx = None
    if x is not None:
        xb, yb = Buf(v, c, dtype, ld, data=O.to_cl(x)), Buf(vo, c, dtype, ld)
        ops.upsample2_fwd(xb.view, yb.view, dims, c, sd)
        torch.cuda.synchronize()
        yb.assert_guards("y")
        y = O.from_cl(yb.host().double().numpy(), n, odims)
    if dy is not None:
        db, xb = Buf(vo, c, dtype, ld, data=O.to_cl(dy)), Buf(v, c, dtype, ld)
        ops.upsample2_bwd(db.view, xb.view, dims, c, sd)
        torch.cuda.synchronize()
        xb.assert_guards("dx")
        dx = O.from_cl(xb.host().double().numpy(), n, dhw)
    return y, dx


@pytest.mark.parametrize("case", O.UP_CASES, ids=O.up_id)
def test_upsample_within_the_derived_bound(case):
    sd, bf16 = case["sd"], case["dt"] == "bf16"
    d = O.up_data(case)
    x, dy = d.get("x"), d.get("dy")
    if case["which"] != "both":
        assert O.up_items(case, case["which"]) > O.UP_GRID_CAP * O.UP_THREADS
    y64, dx64 = O.up_torch(x, dy, sd)
    y, dx = _run_up(case, x, dy)
    res = {}
    for side, got, ref, bound in (("fwd", y, y64, None if x is None else O.up_fwd_bound(x, y64, sd, bf16)),
                                  ("bwd", dx, dx64, None if dy is None else O.up_bwd_bound(dy, dx64, sd, bf16))):
        if got is None:
            continue
        res[side] = O.ratio(got, ref, bound)
        if bf16 and got.size >= 1000:
            res[side + ".bias"] = O.check_bf16_bias(got, ref, side)
    _log(O.up_id(case), res)
    assert all(res[s] <= 1.0 for s in ("fwd", "bwd") if s in res), res


@pytest.mark.parametrize("case", O.UP_EXACT_CASES, ids=O.up_id)
def test_upsample_length_one_axes_are_exact(case):
    d = O.up_exact_data(case)
    y64, dx64 = O.up_exact_ref(case, d)
    y, dx = _run_up(case, d["x"], d["dy"])
    assert np.array_equal(y, y64) and np.array_equal(dx, dx64)


def _device_axis_weights():
    """the device's own weights of output o on input i, A[L][o, i], read from forwards on one-hot inputs along W (D = H = 1,
    C = L, channel i one at position i: the other two axes have the exact weights 1 and 0)"""
    from fplx import ops
    weights = {}
    for L in O.UP_TRANSPOSE_LENGTHS:
        xb = Buf(L, L, torch.float32, data=np.eye(L))
        yb = Buf(8 * L, L, torch.float32)
        ops.upsample2_fwd(xb.view, yb.view, (1, 1, 1, L), L, 2)
        torch.cuda.synchronize()
        yb.assert_guards("one-hot y")
        a = yb.host().double().numpy().reshape(2, 2, 2 * L, L)
        assert all(np.array_equal(a[i, j], a[0, 0]) for i in range(2) for j in range(2))
        a = a[0, 0]
        i0, i1, l0, l1, _ = O.axis_table(L, 2 * L)
        exact = np.zeros((2 * L, L))
        np.add.at(exact, (np.arange(2 * L), i0), l0)
        np.add.at(exact, (np.arange(2 * L), i1), l1)
        # each weight is the hat function at s_eff: within the coordinate error of the exact one, plus the rounding of 1 - l1
        assert (a >= 0).all() and np.abs(a - exact).max() <= O.E_COORD * (L - 1) + 2.0 ** -24
        assert np.abs(a.sum(1) - 1.0).max() <= 2.0 ** -23
        weights[L] = a
    return weights


def test_upsample_backward_is_the_transpose_of_the_device_forward():
    """no tolerance on the decisions: whatever i0 the forward took for an output, the backward must hand that output's gradient
    to the same inputs with the same weights - a candidate window that drops an output fails here"""
    from fplx import ops
    weights = _device_axis_weights()
    res = {}
    for n, dhw, sd in O.UP_TRANSPOSE_CASES:
        c = 3
        case = dict(n=n, dhw=dhw, c=c, ld=c, sd=sd, dt="fp32")
        dy = O.ints("upt.%dx%dx%d.%d" % (dhw + (sd,)), (n, c) + O.up_out_dims(case), -4, 4)
        want, S, nterm = O.kron_transpose(dy, sd, weights)
        _, dx = _run_up(case, None, dy)
        key = "%dx%dx%d.sd%d" % (dhw + (sd,))
        res[key] = O.ratio(dx, want, O.gamma(3 + nterm) * S)
    _log("transpose", res)
    assert max(res.values()) <= 1.0, res


# ================================================================ sliding window

GUARD = 64


class Flat(object):
    """a contiguous float32 array of `shape` between two guards of 64 NaN floats, optionally one element off 16 bytes"""

    def __init__(self, shape, misaligned=False, data=None):
        self.n = int(np.prod(shape))
        self.flat = torch.full((self.n + 2 * GUARD + 4,), NAN, dtype=torch.float32, device="cuda")
        s = GUARD + (1 if misaligned else 0)
        self.start = s
        self.view = self.flat[s:s + self.n].view(tuple(shape))
        assert self.view.data_ptr() % 16 == (4 if misaligned else 0)
        if data is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(data, np.float32)))

    def assert_guards(self, what):
        assert bool(torch.isnan(self.flat[:self.start]).all()) and bool(torch.isnan(self.flat[self.start + self.n:]).all()), \
            "%s: written outside the result" % what
        assert not bool(torch.isnan(self.view).any()), "%s: not every element of the result was written" % what

    def host(self):
        return self.view.detach().cpu().numpy()


def _cargs(n, c, dhw, window, starts, flips):
    arr = [(ctypes.c_int * len(s))(*s) for s in starts]
    fl = (ctypes.c_int * len(flips))(*flips)
    return (n, c, dhw[0], dhw[1], dhw[2], arr[0], len(starts[0]), arr[1], len(starts[1]), arr[2], len(starts[2]),
            window[0], window[1], window[2], fl, len(flips))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _extract(image, starts, window, flips, misaligned=False):
    from fplx._lib import call
    n, c = image.shape[:2]
    tiles = len(O.sw_tiles(starts))
    img = Flat(image.shape, misaligned, image)
    out = Flat((len(flips), tiles, n, c) + tuple(window), misaligned)
    call("fplx_sw_extract", img.view.data_ptr(), *_cargs(n, c, image.shape[2:], window, starts, flips), out.view.data_ptr(), _stream())
    torch.cuda.synchronize()
    out.assert_guards("patches")
    return out.host()


def _merge(buffer, passes, chunk, n, k, dhw, starts, window, flips, misaligned=(False, False), plain=False):
    """buffer: the prediction buffer in the layout of fplx_sw_merge_mc -> [passes, n, k, d, h, w]"""
    from fplx._lib import call
    src = Flat(buffer.shape, misaligned[0], buffer)
    out = Flat((passes, n, k) + tuple(dhw), misaligned[1])
    args = _cargs(n, k, dhw, window, starts, flips)
    if plain:
        call("fplx_sw_merge", src.view.data_ptr(), *args, out.view.data_ptr(), _stream())
    else:
        call("fplx_sw_merge_mc", src.view.data_ptr(), passes, chunk, *args, out.view.data_ptr(), _stream())
    torch.cuda.synchronize()
    out.assert_guards("merged")
    return out.host()


def _same_bits(a, b):
    return a.dtype == np.float32 and b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def _plan(name, tta):
    dhw, window, stride = O.SW_PLANS[name]
    window, starts = O.sw_starts(dhw, window, stride)
    return dhw, window, starts, O.sw_flips(tta)


@pytest.mark.parametrize("case", O.SW_CASES, ids=O.sw_id)
def test_sw_extract_equals_the_slices(case):
    dhw, window, starts, flips = _plan(*case)
    img = O.sw_image(case[0], 2, 3, dhw, "real")
    assert _same_bits(_extract(img, starts, window, flips), O.sw_extract_ref(img, starts, window, flips))


@pytest.mark.parametrize("kind", ["int", "real"])
@pytest.mark.parametrize("case", O.SW_CASES, ids=O.sw_id)
def test_sw_merge_equals_the_loops(case, kind):
    dhw, window, starts, flips = _plan(*case)
    n, k = 2, 2
    tiles = len(O.sw_tiles(starts))
    p = O.sw_image("%s.p%d" % case, len(flips) * tiles * n, k, window, kind).reshape((len(flips), tiles, n, k) + tuple(window))
    want = O.sw_merge_ref(p, dhw, starts, window, flips)
    nb = len(flips) * tiles * n
    buf = p.reshape((nb, k) + tuple(window))
    assert _same_bits(_merge(buf, 1, nb, n, k, dhw, starts, window, flips, plain=True)[0], want)
    assert _same_bits(_merge(buf, 1, nb, n, k, dhw, starts, window, flips, misaligned=(True, False))[0], want)


@pytest.mark.parametrize("case", O.SW_CASES, ids=O.sw_id)
def test_sw_round_trip_returns_the_image(case):
    dhw, window, starts, flips = _plan(*case)
    img = O.sw_image(case[0], 2, 3, dhw, "int")
    p = _extract(img, starts, window, flips)
    nb = p.shape[0] * p.shape[1] * 2
    back = _merge(p.reshape((nb, 3) + tuple(window)), 1, nb, 2, 3, dhw, starts, window, flips)[0]
    assert _same_bits(back, img)


@pytest.mark.parametrize("tta", [0, 1])
@pytest.mark.parametrize("kind", ["int", "real"])
def test_sw_whole_image_path_equals_the_generic_path(tta, kind):
    """one tile, W % 4 == 0: aligned pointers take sw_merge_whole_k, a pointer 4 bytes off takes sw_merge_k - the same bits"""
    dhw, window, starts, flips = _plan("single_tile", tta)
    n, k = 2, 3
    assert dhw[2] % 4 == 0 and len(O.sw_tiles(starts)) == 1
    p = O.sw_image("whole.%d" % tta, len(flips) * n, k, dhw, kind)
    want = O.sw_merge_ref(p.reshape((len(flips), 1, n, k) + tuple(dhw)), dhw, starts, window, flips)
    nb = len(flips) * n
    got = [_merge(p, 1, nb, n, k, dhw, starts, window, flips, misaligned=m, plain=plain)[0]
           for m in ((False, False), (True, False), (False, True)) for plain in (False, True)]
    assert all(_same_bits(g, want) for g in got)


@pytest.mark.parametrize("chunk", [10, 7, 96, 1000])
def test_sw_merge_mc_with_a_ragged_last_chunk(chunk):
    dhw, window, starts, flips = _plan("dup_last", 1)
    n, k, passes = 2, 3, 3
    tiles = len(O.sw_tiles(starts))
    nb = len(flips) * tiles * n
    assert nb == 96
    per = O.sw_image("mc", passes * nb, k, window, "real").reshape((passes, nb, k) + tuple(window))
    want = np.stack([O.sw_merge_ref(per[q].reshape((len(flips), tiles, n, k) + tuple(window)), dhw, starts, window, flips)
                     for q in range(passes)])
    got = _merge(O.sw_mc_layout(per, chunk), passes, chunk, n, k, dhw, starts, window, flips)
    assert _same_bits(got, want)
    for q in range(passes):              # and fplx_sw_merge on each pass alone
        assert _same_bits(_merge(per[q], 1, nb, n, k, dhw, starts, window, flips, plain=True)[0], want[q])


def test_sw_single_tile_mc_on_the_whole_image_path():
    dhw, window, starts, flips = _plan("single_tile", 1)
    n, k, passes, chunk = 2, 2, 3, 6
    nb = len(flips) * n
    per = O.sw_image("mcwhole", passes * nb, k, dhw, "real").reshape((passes, nb, k) + tuple(dhw))
    want = np.stack([O.sw_merge_ref(per[q].reshape((len(flips), 1, n, k) + tuple(dhw)), dhw, starts, window, flips) for q in range(passes)])
    lay = O.sw_mc_layout(per, chunk)
    assert _same_bits(_merge(lay, passes, chunk, n, k, dhw, starts, window, flips), want)
    assert _same_bits(_merge(lay, passes, chunk, n, k, dhw, starts, window, flips, misaligned=(True, False)), want)


def test_sw_refusals():
    """FPLX_E_BADSHAPE (-1) before any launch: 65 tiles on an axis, starts that decrease, a gap, tiles short of the end, a window
    larger than the image - from all three entry points; 64 tiles are accepted (test_sw_merge_equals_the_loops[tiles_64])"""
    from fplx import _lib
    lib = _lib.lib()
    st = _stream()
    n, c = 1, 2
    src = torch.zeros(1 << 16, device="cuda")
    out = torch.full((1 << 16,), 7.0, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def rc_all(dhw, window, starts):
        a = _cargs(n, c, dhw, window, starts, (0,))
        return (lib.fplx_sw_extract(p(src), *a, p(out), st), lib.fplx_sw_merge(p(src), *a, p(out), st),
                lib.fplx_sw_merge_mc(p(src), 2, 3, *a, p(out), st))

    assert rc_all((2, 3, 65), (2, 3, 1), [[0], [0], list(range(65))]) == (-1, -1, -1)
    assert "tiles per axis" in _lib.last_error()
    assert rc_all((2, 32, 4), (2, 16, 4), [[0], [0, 16, 8, 16], [0]]) == (-1, -1, -1)          # not monotone
    assert rc_all((2, 40, 4), (2, 16, 4), [[0], [0, 24], [0]]) == (-1, -1, -1)                 # a gap: 16 .. 23 uncovered
    assert "gap" in _lib.last_error()
    assert rc_all((2, 32, 4), (2, 16, 4), [[0], [0, 8], [0]]) == (-1, -1, -1)                  # ends at 24 of 32
    assert "reach the end" in _lib.last_error()
    assert rc_all((2, 32, 4), (2, 16, 4), [[0], [8, 16], [0]]) == (-1, -1, -1)                 # does not start at 0
    assert rc_all((2, 8, 4), (2, 16, 4), [[0], [0], [0]]) == (-1, -1, -1)                      # window larger than the image
    assert "window" in _lib.last_error()
    assert rc_all((2, 32, 4), (2, 16, 4), [[0], [0, 8, 16, 17], [0]]) == (-1, -1, -1)          # beyond the image
    a = _cargs(n, c, (2, 32, 4), (2, 16, 4), [[0], [0, 16], [0]], (0,))
    assert lib.fplx_sw_merge_mc(p(src), 0, 3, *a, p(out), st) == -1                             # no passes
    assert lib.fplx_sw_merge_mc(p(src), 2, 0, *a, p(out), st) == -1                             # no chunk
    assert lib.fplx_sw_extract(None, *a, p(out), st) == -5 and lib.fplx_sw_merge(p(src), *a, None, st) == -5
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def test_sw_grid_stride_loops():
    cap = O.SW_GRID_CAP * O.SW_THREADS
    b = O.SW_BIG_EXTRACT
    window, starts = O.sw_starts(b["dhw"], b["window"], b["stride"])
    flips = O.sw_flips(b["tta"])
    img = O.sw_image("big.extract", b["n"], b["c"], b["dhw"], "real")
    got = _extract(img, starts, window, flips)
    assert got.size > cap and _same_bits(got, O.sw_extract_ref(img, starts, window, flips))
    for b, name in ((O.SW_BIG_MERGE, "big.merge"), (O.SW_BIG_WHOLE, "big.whole")):
        window, starts = O.sw_starts(b["dhw"], b["window"], b["stride"])
        flips = O.sw_flips(b["tta"])
        tiles = len(O.sw_tiles(starts))
        n, k = b["n"], b["c"]
        nb = len(flips) * tiles * n
        p = O.sw_image(name, nb, k, window, "int" if name == "big.whole" else "real")
        want = O.sw_merge_ref(p.reshape((len(flips), tiles, n, k) + tuple(window)), b["dhw"], starts, window, flips)
        assert want.size // (4 if tiles == 1 else 1) > cap
        assert _same_bits(_merge(p, 1, nb, n, k, b["dhw"], starts, window, flips, plain=name == "big.merge")[0], want)


@pytest.mark.parametrize("name", sorted(O.INFERER_CASES))
def test_inferer_run_and_run_mc_equal_the_loops(name):
    import fplx
    n, dhw, cfg, train = O.INFERER_CASES[name]
    img = O.sw_image("inferer." + name, n, 1, dhw, "int")
    want = O.toy_inferer_ref(img, cfg)
    dom = torch.zeros(n, dtype=torch.long)
    toy = O.Toy(cfg["class_num"]).cuda().train(train)
    got = fplx.Inferer(cfg).run(toy, torch.from_numpy(img).cuda(), dom)
    assert got.is_cuda and _same_bits(got.cpu().numpy(), want)
    calls = list(toy.calls)
    if name == "ragged_chunks":          # 96 patches in chunks of 10: nine full ones and a ragged one
        assert calls == [10] * 9 + [6]
    if train:                            # train-mode BatchNorm keeps the reference's batches: one tile per forward
        window, starts = O.sw_starts(dhw, cfg["sliding_window_size"], cfg["sliding_window_stride"])
        assert calls == [n] * len(O.sw_tiles(starts))
    passes = 3
    cfg_mc = dict(cfg)
    if "infer_batch_voxels" in cfg:
        cfg_mc["infer_batch_voxels"] = cfg["infer_batch_voxels"] * passes
    del toy.calls[:]
    mc = fplx.Inferer(cfg_mc).run_mc(toy, torch.from_numpy(img).cuda(), dom, passes).cpu().numpy()
    assert mc.shape == (passes,) + want.shape and all(_same_bits(np.ascontiguousarray(m), want) for m in mc)
    if name == "ragged_chunks":
        assert toy.calls == [30] * 9 + [18]
