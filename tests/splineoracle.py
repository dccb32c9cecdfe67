"""numpy restatement of scipy.ndimage's cubic-spline resampling (order 3, mode='constant', cval=0) - the rules csrc/spline.hip
implements - and the float64 rounding bound the tests hold the kernels to.

The restatement
  prefilter    fp32 samples -> fp64 coefficients; along D, then H, then W, per line of length n > 1, z = sqrt(3) - 2:
                 c *= (1 - z)(1 - 1/z)
                 c[0] = (c[0] + z^(n-1) c[n-1] + sum_{i=1..n-2} z^i (c[i] + z^(n-1) c[n-1-i])) / (1 - z^(2n-2))
                 c[i] += z c[i-1] upwards;  c[n-1] = (z c[n-2] + c[n-1]) z / (z z - 1);  c[i] = z (c[i+1] - c[i]) downwards
               z^i by repeated multiplication, z^(n-1) by math.pow; a line of length 1 is left alone
  coordinates  tests/resample_ref.py's: c_i = ((o_0 M[i][0] + o_1 M[i][1]) + o_2 M[i][2]) + t_i; outside (c_i < 0, c_i > n_i - 1
               or NaN) -> 0.  The last output coordinate of a zoom can exceed n - 1 by an ulp, and scipy writes 0 there
  taps         floor(c) - 1 + k, k = 0..3, reflected about the first and last sample: period 2n - 2, i -> |i| mod period,
               then period - i where i >= n; an axis of extent 1 reads index 0
  weights      y = c - floor(c), zc = 1 - y: w1 = (y y (y-2) 3 + 4) / 6, w2 = (zc zc (zc-2) 3 + 4) / 6, w0 = zc zc zc / 6,
               w3 = 1 - w0 - w1 - w2
  sum          fp64, acc += ((coef * w_d) * w_h) * w_w, k_d outermost, k_w innermost; one cast to fp32

scipy's own float64 bits are not reproduced (none of 36 variants of the line filter was; nearly every fp64 element differs in
its last bits), so nothing is compared bit for bit in fp64.  What is asserted instead is derived here.

The bound.  u = 2^-53, a = |z| = 0.268, r = 1 / (1 - a) = 1.366, X = max|x|.
 One axis of the prefilter, on lines with max-norm A.  The exact filter is linear with max-norm gain at most sqrt(3)
 (G below); the causal half alone has gain 6 r = 8.2 (P = 8.2 A bounds every causal value), the anticausal half maps a
 perturbation eps of the causal values to at most a r eps = 0.366 eps (the start value's coefficients sum to
 (a^2 + a) / (1 - a^2) = a r, the recursion's tail to a (1 + a + ...) = a r).
   gain:       one product with a constant that carries 3 roundings itself: 4 u * 6 A = 24 u A per sample, 24 r = 33 u A on the
               causal values.
   start-up:   term i is z^i (s_i + z^(n-1) s_j): 3 operations, z^i carries i roundings, z^(n-1) two: at most (i + 6) u on a
               term of size a^i 6 A (1 + a); summed over i, 7.6 (a r^2 + 6 a r) u A = 21 u A.  Each addition rounds by at most
               u P, and never by more than the term it adds (the old sum is itself representable): sum_i min(u P, 6.01 A a^i)
               <= 28 u P + 8.2 u A = 238 u A, 28 being the index where a^i falls below u - independent of n.  The division by
               1 - z^(2n-2): 3 u P = 25 u A.  Together at most 300 u A on c[0], decaying with a^i along the line.
   causal:     c[i] + z c[i-1]: the product, the sum, z's own rounding: (1 + 2 a) u P per step, times r through the
               recursion: 17 u A.  The causal values are off by at most 300 + 33 + 17 = 350 u A.
   anticausal: the start value, 6 operations on at most a r P = 3 A: 18 u A, decaying.  A step z (c[i+1] - c[i]): u (3 A + P)
               a = 3 u A for the difference, 2 u * 3 A for the product and z: 9 u A per step, times r: 12.3 u A.
   output:     0.366 * 350 + 18 + 12.3 = 158 u A with the figures as rounded up above (152 from the unrounded ones, which
               tests/test_spline_cpu.py recomputes).  K = 256, the next power of two, is the constant used: the output of one
               axis is off by at most G e_in + K u A, e_in the error its input carried.
 Three axes, A = X, G X, G^2 X:  e = K u X (G^2 + G^2 + G^2) = 9 K u X                                   (prefilter_bound)
 Interpolation.  |coef| <= G^3 X = 5.2 X.  The weights are non-negative and sum to 1: the coefficient errors pass at most once.
   Per axis the computed weights are off by at most 8 u (w0 + w1 + w2) + 4 u <= 12 u in sum, 36 u over three axes; the three
   products per term add 3 u, the 64 additions 64 u, all on at most G^3 X: 103 u G^3 X, 104 used.  The coordinates are scipy's
   own fp64 numbers, operation for operation (the order-0 and order-1 tests hold that to 0 differing elements), so they add
   nothing.
 scipy's float64 result went through the same operations and is off from the exact value by as much, so two results differ by
 at most twice the sum:      B = 2 (9 K + 104 G^3) u X = 5689 u X = 2^-40.5 X                               (interp_bound)
 The condition B <= 2^-40 X holds, and the restatement's own distance from scipy (with scipy 1.15.3: 2^-48.9 X over the
 zooms, 2^-47.1 X for spline_filter, 3 of 3 734 480 float32 outputs not identical; tests/test_spline_cpu.py prints them) leaves
 the derivation its room.  A wrong weight or tap is off by 2^-10 X or more.
The fp32 cast adds half an fp32 ulp: |float64(got) - ref64| <= 2^-24 |ref64| + B.
"""
import math

import numpy as np

Z = math.sqrt(3.0) - 2.0
GAIN = (1.0 - Z) * (1.0 - 1.0 / Z)
U = 2.0 ** -53
K_AXIS = 256.0
G_AXIS = math.sqrt(3.0)
CAP = 2.0 ** -40                       # the condition on every bound, in units of max|x|
MAX_DIFFERING_SHARE = 1e-4             # of the pooled elements not identical to scipy's fp32 result


def prefilter_bound(xmax):
    """|coef - scipy's spline_filter(output=float64)| elementwise"""
    return 2.0 * 9.0 * K_AXIS * U * float(xmax)


def interp_bound(xmax):
    """B of the criterion |float64(got) - ref64| <= 2^-24 |ref64| + B"""
    return 2.0 * (9.0 * K_AXIS + 104.0 * G_AXIS ** 3) * U * float(xmax)


def _filter_axis(c, axis):
    """the line filter along `axis` of a float64 array, in place, all lines at once"""
    n = c.shape[axis]
    if n == 1:
        return
    c = np.moveaxis(c, axis, 0)                      # a view: c[i] is the i-th sample of every line
    c *= GAIN
    zn1 = math.pow(Z, n - 1)
    acc = c[0] + zn1 * c[n - 1]
    zi = Z
    for i in range(1, n - 1):
        acc = acc + zi * (c[i] + zn1 * c[n - 1 - i])
        zi = zi * Z
    c[0] = acc / (1.0 - zn1 * zn1)
    for i in range(1, n):
        c[i] = c[i] + Z * c[i - 1]
    c[n - 1] = (Z * c[n - 2] + c[n - 1]) * Z / (Z * Z - 1.0)
    for i in range(n - 2, -1, -1):
        c[i] = Z * (c[i + 1] - c[i])


def prefilter(x):
    """[C,D,H,W] float32 -> float64 coefficients"""
    x = np.asarray(x)
    assert x.ndim == 4 and x.dtype == np.float32
    c = x.astype(np.float64)
    for axis in (1, 2, 3):
        _filter_axis(c, axis)
    return c


def coordinates(shape, matrix, offset, out_size):
    """-> ([c_d, c_h, c_w] fp64 arrays of out_size, inside mask): resample_ref's sum and outside rule"""
    m = np.asarray(matrix, np.float64).reshape(3, 3)
    t = np.asarray(offset, np.float64).reshape(3)
    o = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in out_size], indexing="ij")
    c = []
    for i in range(3):
        s = o[0] * m[i, 0]
        s = s + o[1] * m[i, 1]
        s = s + o[2] * m[i, 2]
        c.append(s + t[i])
    inside = np.ones(tuple(out_size), bool)
    with np.errstate(invalid="ignore"):
        for i in range(3):
            inside &= (c[i] >= 0) & (c[i] <= shape[i] - 1)
    return c, inside


def reflect(i, n):
    """tap indices (integer array) reflected about samples 0 and n - 1"""
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    period = 2 * n - 2
    i = np.abs(i) % period
    return np.where(i >= n, period - i, i)


def weights(c):
    """-> (floor(c) as int64, [w0, w1, w2, w3])"""
    f = np.floor(c)
    y = c - f
    zc = 1.0 - y
    w1 = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0
    w2 = (zc * zc * (zc - 2.0) * 3.0 + 4.0) / 6.0
    w0 = zc * zc * zc / 6.0
    w3 = 1.0 - w0 - w1 - w2
    return f.astype(np.int64), [w0, w1, w2, w3]


def interpolate(coef, matrix, offset, out_size, dtype=np.float32):
    """float64 coefficients [C,D,H,W] -> [C,*out_size]; dtype float64 keeps the sum uncast"""
    n = coef.shape[1:]
    c, inside = coordinates(n, matrix, offset, out_size)
    c = [np.where(inside, ci, 0.0) for ci in c]
    fw = [weights(ci) for ci in c]
    idx = [[reflect(f - 1 + k, s) for k in range(4)] for (f, _), s in zip(fw, n)]
    w = [wk for _, wk in fw]
    acc = np.zeros((coef.shape[0],) + tuple(out_size), np.float64)
    for kd in range(4):
        for kh in range(4):
            for kw in range(4):
                v = coef[:, idx[0][kd], idx[1][kh], idx[2][kw]]
                acc = acc + ((v * w[0][kd][None]) * w[1][kh][None]) * w[2][kw][None]
    return np.where(inside[None], acc, 0.0).astype(dtype)


def resample(x, matrix, offset, out_size, dtype=np.float32):
    return interpolate(prefilter(x), matrix, offset, out_size, dtype)


def outside(shape, matrix, offset, out_size):
    return ~coordinates(shape, matrix, offset, out_size)[1]


class Pool(object):
    """criterion 3: the count of elements not identical to scipy's fp32 result, pooled over a test function"""

    def __init__(self, what):
        self.what, self.differing, self.total = what, 0, 0

    def add(self, got, ref32):
        self.differing += int((got != ref32).sum())
        self.total += int(got.size)

    def check(self, min_total=100000):
        print("%s: %d of %d elements not identical to scipy's float32 (share %.2e)" % (
            self.what, self.differing, self.total, self.differing / max(self.total, 1)))
        assert self.total >= min_total, (self.what, self.total)
        assert self.differing <= MAX_DIFFERING_SHARE * self.total, (self.what, self.differing, self.total)


def check(got, ref32, ref64, xmax, what, pool=None, outside_mask=None):
    """criteria 1 and 2 for one float32 result; its elements join `pool` for criterion 3"""
    assert got.dtype == np.float32 and got.shape == ref32.shape == ref64.shape, what
    if outside_mask is not None:
        assert not got[np.broadcast_to(outside_mask[None], got.shape)].any(), (what, "outside is exactly 0")
    b = interp_bound(xmax)
    assert b <= CAP * xmax
    err = np.abs(got.astype(np.float64) - ref64)
    tol = 2.0 ** -24 * np.abs(ref64) + b
    differing = int((got != ref32).sum())
    print("%s: %d of %d not identical to scipy's float32; max |got - ref64| - 2^-24 |ref64| = %.3g (B = %.3g)" % (
        what, differing, got.size, float((err - 2.0 ** -24 * np.abs(ref64)).max()) if got.size else 0.0, b))
    assert bool((err <= tol).all()), (what, float((err - tol).max()))
    if pool is not None:
        pool.add(got, ref32)
