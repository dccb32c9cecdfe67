"""Exact oracles for the 1x1x1 head and the deep-supervision interpolation kernels (csrc/head.hip), in the style of
tests/convoracle.py: small-integer data on which every partial sum of every kernel fits the 24-bit significand of fp32 (and
every bf16 result stays an integer of at most 256), so the result does not depend on the order of the additions and must equal
the float64 result bit for bit.  tests/test_nets3d_cpu.py proves the premise on the CPU (float32 torch == float64 torch on
exactly these data); tests/test_gpu_head_exact.py holds the kernels to it.

Bit budgets.  Head forward: C <= 128 products of magnitude <= 16 plus the bias: < 2^12.  Data gradient: <= 8 classes x 4 x 2 = 64,
plus <= 8 when accumulating: an integer <= 72, exact in bf16.  Weight gradient: <= 1024 voxels x 2 x 4 < 2^14.
Interpolation by f: the three axis weights are multiples of 1 / (2 f), so a product has 3 log2(2 f) fractional bits (12 for
f = 8); forward values are convex combinations of integers <= 8 (4 more bits); a backward sum is bounded by the sum of the
weights, f^3 = 512 (9 integer bits) times the largest upstream value - 1 for f = 8 (21 bits), 4 for f <= 4 (9 + 6 + 2 + 1 bits).
"""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

# (N, (D, H, W), C, lda, classes, dtype)
HEAD_CASES = [
    (1, (1, 1, 1), 8, 8, 2, "fp32"),
    (2, (3, 5, 7), 16, 32, 3, "bf16"),
    (1, (2, 4, 33), 32, 32, 2, "bf16"),
    (2, (4, 8, 16), 128, 128, 5, "bf16"),
    (1, (1, 1, 257), 64, 64, 8, "fp32"),
]
# (NC, coarse (d, h, w), factor)
INTERP_CASES = [(nc, dims, f) for dims, f in (((1, 1, 1), 8), ((2, 3, 5), 2), ((1, 2, 3), 4), ((3, 1, 2), 8)) for nc in (2, 6)]


def ints(name, shape, lo, hi):
    rng = np.random.Generator(np.random.Philox(key=zlib.crc32(name.encode()) + 0x5EED))
    return rng.integers(lo, hi + 1, size=tuple(shape)).astype(np.float64)


def head_id(case):
    n, dhw, c, lda, k, dt = case
    return "n%d_%dx%dx%d_c%d_ld%d_k%d_%s" % ((n,) + tuple(dhw) + (c, lda, k, dt))


def head_data(case):
    """float64 arrays: a [N, V, C], w [K, C], bias [K], dlogits [N, K, V], da0 [N, V, C] (what da holds before accumulate = 1)"""
    n, dhw, c, lda, k, dt = case
    v = dhw[0] * dhw[1] * dhw[2]
    tag = "head." + head_id(case)
    return dict(a=ints(tag + ".a", (n, v, c), -4, 4), w=ints(tag + ".w", (k, c), -4, 4), bias=ints(tag + ".b", (k,), -4, 4),
                dlogits=ints(tag + ".dl", (n, k, v), -2, 2), da0=ints(tag + ".da0", (n, v, c), -8, 8))


def head_ref(d, dtype=torch.float64):
    """-> logits [N, K, V], da [N, V, C], da accumulated onto da0, dw [K, C], db [K], computed in `dtype` on the CPU"""
    t = {k: torch.from_numpy(v).to(dtype) for k, v in d.items()}
    logits = torch.einsum("kc,nvc->nkv", t["w"], t["a"]) + t["bias"].view(1, -1, 1)
    da = torch.einsum("kc,nkv->nvc", t["w"], t["dlogits"])
    dw = torch.einsum("nkv,nvc->kc", t["dlogits"], t["a"])
    return dict(logits=logits, da=da, da_acc=t["da0"] + da, dw=dw, db=t["dlogits"].sum((0, 2)))


def interp_id(case):
    nc, dims, f = case
    return "nc%d_%dx%dx%d_f%d" % ((nc,) + tuple(dims) + (f,))


def interp_data(case):
    """float64 arrays: x [NC, d, h, w], dy [NC, f d, f h, f w]"""
    nc, dims, f = case
    tag = "interp." + interp_id(case)
    fine = tuple(f * s for s in dims)
    g = 1 if f == 8 else 4
    return dict(x=ints(tag + ".x", (nc,) + tuple(dims), -8, 8), dy=ints(tag + ".dy", (nc,) + fine, -g, g))


def interp_ref(case, d, dtype=torch.float64):
    """F.interpolate(x, size, mode='trilinear') (align_corners = False) and its autograd transpose, in `dtype` on the CPU"""
    nc, dims, f = case
    x = torch.from_numpy(d["x"]).to(dtype)[None].requires_grad_(True)
    y = F.interpolate(x, [f * s for s in dims], mode="trilinear")
    y.backward(torch.from_numpy(d["dy"]).to(dtype)[None])
    return dict(y=y.detach()[0], dx=x.grad[0])
