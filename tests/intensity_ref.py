"""numpy restatements behind the intensity transforms (fplx.transform, csrc/intensity.hip), written out so that the CPU
tests can hold them against numpy itself and the GPU tests can hold the kernels against them.

  percentile   numpy.percentile(x, q) (method 'linear') on a float32 array of n values with q a Python number.  NumPy 2 does
               the INDEX arithmetic in float32 too: quantile = float32(q) / float32(100), v = float32(n - 1) * quantile, each
               rounded to float32 (not (n - 1) q / 100 in double: the two differ in the last bits of g for most q, and in lo
               itself once n is large),
               lo = floor(v), g = v - lo, a = s[lo], b = s[lo + 1] of the sorted values; v >= n - 1 reads the last element
               twice.  d = b - a; a + d g if g < 0.5, else b - d (1 - g) - every step float32, the result a numpy.float32.
               A NaN anywhere sorts last and makes the result NaN.
  gamma_f64    GammaCorrection's formula evaluated in float64 from the float32 inputs (voxels, min, max, float32(gamma)):
               the yardstick both numpy's float32 pass and the kernel are measured against, in units of one float32 ulp at
               max(|vmin|, |vmax|)
  philox_noise the device generator of GaussianNoise's `gaussiannoise_device_rng` extension: element i takes words
               2 (i & 1), 2 (i & 1) + 1 of Philox4x32-10(counter = (i >> 1, 0, stream, 0), key = seed), u = (word + 1) / 2^32,
               z = sqrt(-2 ln u1) cos(2 pi u2) in float64, y = float32((double(x) + mean) + std z)
"""
import math

import numpy as np

import detdata
from oracle import np_ref

SHAPE = (8, 28, 36)            # the fixture volume is [2, *SHAPE]


def inputs():
    """-> image [2,D,H,W] float32 (channel 0: log-normal, skewed, a quarter of it negative; channel 1: a cubed uniform with a
    negative floor and many repeated values), image1 (the second image of NormalizeWithMeanStd_dual), label uint8 [1,D,H,W]"""
    c0 = np.exp(detdata.normal("it.image0", SHAPE) * 0.9) * 60.0 - 30.0
    c1 = np.round(detdata.uniform("it.image1", SHAPE) ** 3 * 500.0) * 0.5 - 20.0
    img = np.stack([c0, c1]).astype(np.float32)
    img1 = (detdata.normal("it.second", (2,) + SHAPE) * 55.0 + 40.0).astype(np.float32)
    zz, yy, xx = np.meshgrid(*[np.arange(s) for s in SHAPE], indexing="ij")
    lab = (((zz - 4) ** 2 * 5 + (yy - 13) ** 2 + (xx - 19) ** 2 * 0.7) < 70).astype(np.uint8)[None]
    return img, img1, lab


def percentile_index(n, q):
    """-> (lo, hi, g): numpy's float32 index arithmetic (see the module docstring)"""
    f = np.float32
    qq = f(q) / f(100)
    v = f(n - 1) * qq
    if v >= f(n - 1):
        return n - 1, n - 1, v + f(1)
    lo = int(np.floor(v))
    return lo, lo + 1, v - f(lo)


def lerp(a, b, g):
    a, b, g = np.float32(a), np.float32(b), np.float32(g)
    with np.errstate(invalid="ignore", over="ignore"):
        d = b - a
        return a + d * g if g < 0.5 else b - d * (np.float32(1) - g)


def percentile(x, q):
    flat = np.asarray(x, np.float32).reshape(-1)
    n = flat.size
    lo, hi, g = percentile_index(n, q)
    part = np.partition(flat, sorted({lo, hi, n - 1}))
    if np.isnan(part[n - 1]):
        return np.float32(np.nan)
    return lerp(part[lo], part[hi], g)


def clip_affine(x, v0, v1):
    """the float32 pass of NormalizeWithMinMax / NormalizeWithPercentiles with numpy.float32 v0, v1"""
    y = np.array(x, np.float32)
    v0, v1 = np.float32(v0), np.float32(v1)
    y[y < v0] = v0
    y[y > v1] = v1
    with np.errstate(invalid="ignore", divide="ignore"):
        return (y - v0) / (v1 - v0)


def ulp_unit(vmin, vmax):
    return float(np.spacing(np.float32(max(abs(float(vmin)), abs(float(vmax))))))


def gamma_f64(x, gamma):
    """x: one float32 channel; gamma: the drawn Python float (enters numpy's pass as float32) -> float64 array"""
    x = np.asarray(x, np.float32)
    vmin, vmax = np.float64(x.min()), np.float64(x.max())
    g = np.float64(np.float32(gamma))
    with np.errstate(invalid="ignore", divide="ignore"):
        n = (x.astype(np.float64) - vmin) / (vmax - vmin)
        return np.power(n, g) * (vmax - vmin) + vmin


def gamma_error_units(y, x, gamma):
    """max |y - gamma_f64| in units of one float32 ulp at max(|vmin|, |vmax|)"""
    u = ulp_unit(x.min(), x.max())
    return float(np.abs(np.asarray(y, np.float64) - gamma_f64(x, gamma)).max() / u)


def philox_uniforms(n, seed, stream):
    """-> (words uint32 [n, 2], uniforms float64 [n, 2] in (0, 1])"""
    n2 = (n + 1) // 2
    idx = np.arange(n2, dtype=np.uint32)
    z = np.zeros(n2, np.uint32)
    r = np_ref.philox4x32_10(idx, z, np.full(n2, stream & 0xFFFFFFFF, np.uint32), z, seed & 0xFFFFFFFF,
                             (seed >> 32) & 0xFFFFFFFF)
    words = np.stack(r, axis=1).reshape(-1, 2)[:n]
    return words, (words.astype(np.float64) + 1.0) * (1.0 / 4294967296.0)


def philox_noise(x, seed, stream, mean, std):
    x = np.asarray(x, np.float32)
    _, u = philox_uniforms(x.size, seed, stream)
    z = np.sqrt(-2.0 * np.log(u[:, 0])) * np.cos(6.283185307179586 * u[:, 1])
    y = (x.reshape(-1).astype(np.float64) + float(mean)) + float(std) * z
    return y.astype(np.float32).reshape(x.shape), z
