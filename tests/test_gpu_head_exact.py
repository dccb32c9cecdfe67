"""Exact oracles for fplx_head_* and fplx_interp_* (csrc/head.hip): on the integer data of tests/headoracle.py the GPU result
must equal the float64 CPU result bit for bit, whatever the order of the additions.  Refusals return the documented error codes
before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import headoracle as O

pytestmark = pytest.mark.gpu

_DT = {"fp32": torch.float32, "bf16": torch.bfloat16}


def _act(arr, lda, dtype, fill=3.0):
    """[N, V, C] float64 -> the [N * V, :C] view of a [N * V, lda] device buffer (the rest of a concat buffer holds `fill`)"""
    n, v, c = arr.shape
    buf = torch.full((n * v, lda), fill, dtype=dtype, device="cuda")
    buf[:, :c] = torch.from_numpy(arr.reshape(n * v, c)).to(dtype)
    return buf, buf[:, :c]


@pytest.mark.parametrize("case", O.HEAD_CASES, ids=O.head_id)
def test_head_kernels_equal_float64(case):
    from fplx import ops
    n, dhw, c, lda, k, dt = case
    v = dhw[0] * dhw[1] * dhw[2]
    dtype = _DT[dt]
    d = O.head_data(case)
    ref = O.head_ref(d)
    w = torch.from_numpy(d["w"]).float().cuda()
    bias = torch.from_numpy(d["bias"]).float().cuda()
    dl = torch.from_numpy(d["dlogits"]).float().cuda()
    # forward
    buf, a = _act(d["a"], lda, dtype)
    logits = torch.full((n, k, v), float("nan"), device="cuda")
    ops.head_fwd(a, w, bias, logits, n, v, c, k)
    assert torch.equal(logits.double().cpu(), ref["logits"])
    # data gradient, plain and accumulated in place; the columns beyond C (the other half of a concat buffer) stay untouched
    for acc, want in ((False, ref["da"]), (True, ref["da_acc"])):
        dbuf, da = _act(d["da0"], lda, dtype, fill=5.0)
        ops.head_dgrad(dl, w, da, n, v, c, k, acc)
        assert torch.equal(da.double().cpu().view(n, v, c), want), acc
        assert lda == c or bool((dbuf[:, c:] == 5.0).all())
    # weight and bias gradient through the two-stage reduction
    ws = torch.empty(max(ops.head_wgrad_ws_bytes(n, v, c, k), 16), dtype=torch.uint8, device="cuda")
    dw = torch.full((k, c), float("nan"), device="cuda")
    db = torch.full((k,), float("nan"), device="cuda")
    ops.head_wgrad(a, dl, dw, db, n, v, c, k, ws)
    assert torch.equal(dw.double().cpu(), ref["dw"])
    assert torch.equal(db.double().cpu(), ref["db"])
    dw2 = torch.empty_like(dw)
    ops.head_wgrad(a, dl, dw2, None, n, v, c, k, ws)             # the bias gradient is optional
    assert torch.equal(dw2, dw)


@pytest.mark.parametrize("case", O.INTERP_CASES, ids=O.interp_id)
def test_interpolation_equals_float64_interpolate_and_its_autograd(case):
    from fplx import ops
    nc, dims, f = case
    d = O.interp_data(case)
    ref = O.interp_ref(case, d)
    x = torch.from_numpy(d["x"]).float().cuda()
    y = torch.full((nc,) + tuple(f * s for s in dims), float("nan"), device="cuda")
    ops.interp_fwd(x, y, nc, dims, f)
    assert torch.equal(y.double().cpu(), ref["y"])
    dy = torch.from_numpy(d["dy"]).float().cuda()
    dx = torch.full_like(x, float("nan"))
    ops.interp_bwd(dy, dx, nc, dims, f)
    assert torch.equal(dx.double().cpu(), ref["dx"])


def test_bad_arguments_are_refused_with_the_documented_codes():
    """FPLX_E_BADSHAPE -1, FPLX_E_BADDTYPE -2, FPLX_E_WORKSPACE -3, FPLX_E_NULL -5 - checked on the host, nothing is launched
    (the output buffers keep their fill)"""
    from fplx import _lib
    lib = _lib.lib()
    n, v, c, k = 1, 10, 16, 2
    a = torch.zeros((n * v, c), device="cuda")
    w = torch.zeros((k, c), device="cuda")
    lg = torch.full((n, k, v), 7.0, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.fplx_head_fwd(p(a), 12, 0, p(w), None, p(lg), n, v, 12, k, st) == -1          # C not a multiple of 8
    assert lib.fplx_head_fwd(p(a), c, 0, p(w), None, p(lg), n, v, c, 9, st) == -1            # 9 classes
    assert lib.fplx_head_fwd(p(a), c, 0, p(w), None, p(lg), n, v, 520, k, st) == -1          # C > 512
    assert lib.fplx_head_fwd(p(a), 8, 0, p(w), None, p(lg), n, v, c, k, st) == -1            # lda < C
    assert lib.fplx_head_fwd(p(a), c, 7, p(w), None, p(lg), n, v, c, k, st) == -2            # dtype
    assert lib.fplx_head_fwd(None, c, 0, p(w), None, p(lg), n, v, c, k, st) == -5
    assert lib.fplx_head_fwd(p(a), c, 0, None, None, p(lg), n, v, c, k, st) == -5
    assert lib.fplx_head_dgrad(p(lg), p(w), None, c, 0, n, v, c, k, 0, st) == -5
    assert lib.fplx_head_dgrad(p(lg), p(w), p(a), c, 0, n, v, c, 0, 0, st) == -1             # no classes
    need = lib.fplx_head_wgrad_ws_bytes(n, v, c, k)
    assert need > 0 and lib.fplx_head_wgrad_ws_bytes(n, v, 12, k) == 0 and lib.fplx_head_wgrad_ws_bytes(n, v, c, 9) == 0
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    dw = torch.full((k, c), 7.0, device="cuda")
    assert lib.fplx_head_wgrad(p(a), c, 0, p(lg), p(dw), None, n, v, c, k, p(ws), need - 1, st) == -3
    assert lib.fplx_head_wgrad(p(a), c, 0, p(lg), p(dw), None, n, v, c, k, None, need, st) == -5
    x = torch.zeros((2, 2, 2, 2), device="cuda")
    y = torch.full((2, 6, 6, 6), 7.0, device="cuda")
    assert lib.fplx_interp_fwd(p(x), p(y), 2, 2, 2, 2, 3, st) == -1                          # factor 3
    assert lib.fplx_interp_bwd(p(y), p(x), 2, 2, 2, 2, 16, st) == -1
    assert lib.fplx_interp_fwd(None, p(y), 2, 2, 2, 2, 2, st) == -5
    assert lib.fplx_interp_bwd(p(y), None, 2, 2, 2, 2, 2, st) == -5
    assert lib.fplx_interp_fwd(p(x), p(y), 0, 2, 2, 2, 2, st) == -1
    torch.cuda.synchronize()
    assert bool((lg == 7.0).all()) and bool((dw == 7.0).all()) and bool((y == 7.0).all())
    assert "factor" in _lib.last_error() or "shape" in _lib.last_error()
