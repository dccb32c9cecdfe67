"""Order-independent oracles for the convolution kernels ("two oracles").

A - exact oracle.  Integer operands (x, dy in {-1, 0, 1} at a chosen density, w in {-2..2}, integer bias): every product is
    exact in bf16 x bf16 -> fp32 and every partial sum is an integer.  While the sum of the magnitudes of an output's terms stays
    below 2^24, every partial sum is exact in fp32 in ANY order (MFMA grouping, split-K, tree reductions), so the result is
    fully determined: bf16 outputs equal bf16_rne(ref) bit for bit, fp32 outputs (dw, db, logits, statistics) equal ref.  The
    precondition is asserted, never assumed (assert_exact_pre, stats_ref).
B - rounding oracle.  Random bf16-valued operands; each element against the float64 reference of the same operands:
    |y - ref| <= 2^-8 (|ref| + gamma S) + gamma S with S the same convolution on |x|, |w|, |b| and gamma = K u / (1 - K u),
    K terms, u = 2^-23 (twice the fp32 round-to-nearest unit: whether the MFMA's internal adds round or truncate is not
    assumed).  Sound for any summation order.  Plus the rounding bias: the mean of sign(ref) (y - ref) / ulp_bf16(ref) over all
    elements, about 0 for round-to-nearest-even and about -0.5 for truncation.

Pure torch / numpy on the CPU; tests/test_conv_oracles_cpu.py checks the oracles themselves, tests/test_gpu_conv_exact.py
applies them to the kernels."""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

EXACT_LIMIT = float(1 << 24)
U_ACC = 2.0 ** -23          # per-addition relative error allowed to an fp32 accumulation (twice the RNE unit)
BIAS_LIMIT = 0.1            # |mean signed error| in bf16 ulps


# ---------------------------------------------------------------- bf16 rounding without torch's conversion

def _np64(t):
    return t.detach().double().cpu().numpy() if torch.is_tensor(t) else np.asarray(t, np.float64)


def bf16_rne(t):
    """round to the nearest bf16 value, ties to even (normal range) -> float64 tensor.  Written with frexp and numpy's
    half-to-even round, independently of torch's conversion, so that the two can be compared."""
    m, e = np.frexp(_np64(t))                # a = m 2^e, 0.5 <= |m| < 1: 8 significant bits = m * 256 in [128, 256)
    return torch.from_numpy(np.ldexp(np.round(m * 256.0), e - 8))


def bf16_trunc(t):
    """round toward zero to bf16 (the defect the rounding oracle must see) -> float64 tensor"""
    m, e = np.frexp(_np64(t))
    return torch.from_numpy(np.ldexp(np.trunc(m * 256.0), e - 8))


def ulp_bf16(t):
    """spacing of the bf16 numbers in the binade of |t| (the smallest normal's for 0) -> float64 tensor"""
    a = np.abs(_np64(t))
    _, e = np.frexp(np.where(a == 0, 2.0 ** -126, a))
    return torch.from_numpy(np.ldexp(1.0, e - 8))


# ---------------------------------------------------------------- operands

def _gen(key):
    return torch.Generator().manual_seed(zlib.crc32(key.encode()))


def int_operand(key, shape, density, vmax=1):
    """reproducible integer tensor (float32): nonzero with probability `density`, then uniform in {-vmax..vmax} \\ {0}"""
    g = _gen(key)
    nz = torch.rand(shape, generator=g) < density
    mag = torch.randint(1, vmax + 1, shape, generator=g)
    sgn = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (mag * sgn * nz).float()


def int_weight(key, shape):
    """w in {-2..2}, E[w^2] = 2"""
    return int_operand(key, shape, 0.8, 2)


def density_for(voxels, k_terms, budget=float(1 << 22), e_w2=2.0, pmax=0.5):
    """density of a {-1, 0, 1} input that keeps a channel's expected sum of y^2 (voxels K p E[w^2]) near `budget` (a quarter
    of 2^24); the precondition itself is checked on the actual data"""
    return float(min(pmax, budget / (voxels * k_terms * e_w2)))


def real_operand(key, shape, std=1.0):
    """bf16-valued float32 tensor ~ N(0, std^2)"""
    return (torch.randn(shape, generator=_gen(key)) * std).bfloat16().float()


# ---------------------------------------------------------------- references (float64) and the precondition

def conv3d_ref(x, w, b, padding):
    return F.conv3d(x.double(), w.double(), None if b is None else b.double(), padding=padding)


def conv3d_abs(x, w, b, padding):
    """S: the same convolution on |x|, |w|, |b| = per output the sum of the magnitudes of its terms"""
    return conv3d_ref(x.abs(), w.abs(), None if b is None else b.abs(), padding)


def dgrad_ref(dy, w, padding):
    """data gradient of conv3d(x, w, padding), stride 1"""
    return F.conv_transpose3d(dy.double(), w.double(), padding=padding)


def wgrad_ref(x, dy, wshape, padding):
    return torch.nn.grad.conv3d_weight(x.double(), wshape, dy.double(), padding=padding)


def conv3d_sparse_ref(x, w, b):
    """3x3x3 'same' convolution of a SPARSE integer x by scattering its nonzeros -> [V, Cout] channels-last, float32 - exact
    under the precondition (every partial sum an integer below 2^24), at a fraction of a dense reference's memory"""
    n, _, d, h, wd = x.shape
    cout = w.shape[0]
    y = torch.zeros((n, d, h, wd, cout), dtype=torch.float32)
    if b is not None:
        y += b.float()
    nz = x.nonzero()
    val = x[tuple(nz.t())].float()
    for kd in range(3):
        for kh in range(3):
            for kw in range(3):
                od, oh, ow = nz[:, 2] + 1 - kd, nz[:, 3] + 1 - kh, nz[:, 4] + 1 - kw
                ok = (od >= 0) & (od < d) & (oh >= 0) & (oh < h) & (ow >= 0) & (ow < wd)
                contrib = val[ok, None] * w[:, nz[ok, 1], kd, kh, kw].t().float()
                y.index_put_((nz[ok, 0], od[ok], oh[ok], ow[ok]), contrib, accumulate=True)
    return y.view(-1, cout)


def assert_exact_pre(S, what):
    """precondition of oracle A: every output's sum of term magnitudes (or an upper bound of it) below 2^24"""
    m = float(torch.as_tensor(S).max())
    assert m < EXACT_LIMIT, "%s: sum of |terms| reaches %g >= 2^24 - the exact oracle does not apply" % (what, m)


def stats_ref(y2d):
    """per-channel (sum y, sum y^2) of a [V, C] tensor in float64, with the precondition asserted: sum |y|, sum y^2 < 2^24"""
    y = y2d.double()
    s1, s2, sa = y.sum(0), (y * y).sum(0), y.abs().sum(0)
    assert float(s2.max()) < EXACT_LIMIT and float(sa.max()) < EXACT_LIMIT, \
        "statistics: sum y^2 = %g, sum |y| = %g >= 2^24 - lower the density" % (float(s2.max()), float(sa.max()))
    return s1, s2


def stats_sum(stats):
    """a kernel's [rows][2][C] fp32 partial rows summed in float64 on the host -> (sum, sum of squares)"""
    s = stats.detach().double().cpu().sum(0)
    return s[0], s[1]


def exact_mismatches(got, want):
    """number of elements that differ (NaN counts as a difference)"""
    return int((~(got.detach().double().cpu() == want.detach().double().cpu())).sum())


def assert_exact(got, want, what):
    g, w = got.detach().double().cpu(), want.detach().double().cpu()
    assert g.shape == w.shape, (what, tuple(g.shape), tuple(w.shape))
    bad = ~(g == w)
    nbad = int(bad.sum())
    if nbad:
        idx = int(bad.flatten().nonzero()[0, 0])
        raise AssertionError("%s: %d of %d elements differ from the exact result (first at flat index %d: got %r, want %r)" % (
            what, nbad, g.numel(), idx, float(g.flatten()[idx]), float(w.flatten()[idx])))


# ---------------------------------------------------------------- oracle B

def gamma(k_terms):
    ku = k_terms * U_ACC
    assert ku < 0.5
    return ku / (1.0 - ku)


def rounding_bound(ref, S, k_terms, bf16_out=True):
    """per-element bound on |y - ref| for a result accumulated in fp32 from K exact products in any order, then rounded to
    bf16 (bf16_out) or stored as fp32"""
    g = gamma(k_terms)
    ref, S = ref.double(), S.double()
    if bf16_out:
        return 2.0 ** -8 * (ref.abs() + g * S) + g * S
    return g * S + 2.0 ** -24 * (ref.abs() + g * S)


def bound_ratio(got, ref, S, k_terms, bf16_out=True):
    """max over the elements of |y - ref| / bound (NaN -> inf): <= 1 passes"""
    err = (got.detach().double().cpu() - ref.double()).abs()
    r = err / rounding_bound(ref, S, k_terms, bf16_out).clamp_min(1e-300)
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return float(r.max())


def rounding_bias(got, ref):
    """mean over the nonzero reference elements of sign(ref) (y - ref) / ulp_bf16(ref)"""
    y, r = got.detach().double().cpu().flatten(), ref.double().flatten()
    nz = r != 0
    y, r = y[nz], r[nz]
    return float((torch.sign(r) * (y - r) / ulp_bf16(r)).mean())


def check_rounding(got, ref, S, k_terms, what, bf16_out=True):
    """oracle B on one output tensor; returns (max err / bound, bias)"""
    ratio = bound_ratio(got, ref, S, k_terms, bf16_out)
    assert ratio <= 1.0, "%s: the error reaches %.3g of the rounding bound" % (what, ratio)
    bias = rounding_bias(got, ref) if bf16_out else 0.0
    assert abs(bias) <= BIAS_LIMIT, "%s: rounding bias %.3f ulp (round-to-nearest-even gives ~0, truncation ~ -0.5)" % (what, bias)
    return ratio, bias


# ---------------------------------------------------------------- layouts

def cl(t):
    """NCDHW -> [V, C] channels-last, contiguous (for n = 1 a reshape alone would be a column-major view)"""
    return t.permute(0, 2, 3, 4, 1).contiguous().view(-1, t.shape[1])


def uncl(t2, n, d, h, w):
    return t2.reshape(n, d, h, w, -1).permute(0, 4, 1, 2, 3)
