"""numpy restatement of scipy.ndimage's resampling for spline orders 0 and 1 under mode='constant', cval=0: the rules
csrc/resample.hip implements, written out so that the CPU tests can hold them against scipy itself (0 differing elements)
and the host logic of fplx.transform can be tested without a device.

  coordinates  fp64, c_i = ((o_0 M[i][0] + o_1 M[i][1]) + o_2 M[i][2]) + t_i - products added in the order j = 0, 1, 2, the
               offset LAST; numpy never fuses a multiply with an add
  outside      any c_i < 0 or c_i > n_i - 1 -> 0 (order 0 as well)
  order 0      x[floor(c_i + 0.5)]
  order 1      f = floor(c), y = c - f, weights (1 - y, 1 - (1 - y)) - scipy forms the last weight as 1 minus the others,
               which is not y to the last bit; fp64 sum of ((x * w_d) * w_h) * w_w over the 8 neighbours - the VALUE is
               multiplied by one axis weight after the other, as scipy's loop does - k_d outermost, k_w innermost; an index
               one past the end has weight 0 and is clamped; one cast to the output type.
               Either shortcut (weights (1 - y, y), or x times the product of the weights) moves the fp64 sum by an ulp
               and with it an fp32 result now and then: 1 element of 3000 at zoom x0.5, 1 of 108 on a 2x2x2 volume,
               203 over 2376 random cases - against 0 over 4700 with the rule above.
"""

import numpy as np

import detdata


def resample_affine(x, matrix, offset, out_size, order):
    """x [C,D,H,W] (float32, or uint8 with order 0) -> [C,*out_size]"""
    x = np.asarray(x)
    assert x.ndim == 4 and order in (0, 1)
    m = np.asarray(matrix, np.float64).reshape(3, 3)
    t = np.asarray(offset, np.float64).reshape(3)
    n = x.shape[1:]
    o = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in out_size], indexing="ij")
    c = []
    for i in range(3):
        s = o[0] * m[i, 0]
        s = s + o[1] * m[i, 1]
        s = s + o[2] * m[i, 2]
        c.append(s + t[i])
    inside = np.ones(tuple(out_size), bool)
    for i in range(3):
        inside &= (c[i] >= 0) & (c[i] <= n[i] - 1)
    c = [np.where(inside, ci, 0.0) for ci in c]
    if order == 0:
        idx = [np.floor(ci + 0.5).astype(np.int64) for ci in c]
        y = x[:, idx[0], idx[1], idx[2]]
        return np.where(inside[None], y, 0).astype(x.dtype)
    f = [np.floor(ci) for ci in c]
    frac = [ci - fi for ci, fi in zip(c, f)]
    w = [(1.0 - yi, 1.0 - (1.0 - yi)) for yi in frac]
    i0 = [fi.astype(np.int64) for fi in f]
    i1 = [np.minimum(i + 1, s - 1) for i, s in zip(i0, n)]
    ii = list(zip(i0, i1))
    acc = np.zeros((x.shape[0],) + tuple(out_size), np.float64)
    for kd in range(2):
        for kh in range(2):
            for kw in range(2):
                v = x[:, ii[0][kd], ii[1][kh], ii[2][kw]].astype(np.float64)
                acc = acc + ((v * w[0][kd][None]) * w[1][kh][None]) * w[2][kw][None]
    return np.where(inside[None], acc, 0.0).astype(x.dtype)


def zoom_size(shape, zoom):
    """scipy.ndimage.zoom's output extents: int(round(n * zoom)) with Python's round"""
    return [int(round(n * z)) for n, z in zip(shape, zoom)]


def zoom_affine(shape, out_size):
    """diagonal matrix and zero offset of a zoom: step (n - 1) / (out - 1) per axis, 1.0 where out == 1"""
    step = [(float(n) - 1) / (float(o) - 1) if o > 1 else 1.0 for n, o in zip(shape, out_size)]
    return np.diag(step), np.zeros(3)


def rotate_affine(shape, cos, sin, axes):
    """scipy.ndimage.rotate(reshape=False) in the plane `axes` (two of -1, -2, -3, any order: scipy sorts them): matrix
    [[cos, sin], [-sin, cos]] on the sorted axes, offset (n - 1) / 2 - R (n - 1) / 2"""
    a, b = sorted(ax % 3 for ax in axes)
    m = np.eye(3)
    m[a, a], m[a, b], m[b, a], m[b, b] = cos, sin, -sin, cos
    r = np.array([[cos, sin], [-sin, cos]], np.float64)
    centre = (np.array([shape[a], shape[b]], np.float64) - 1) / 2
    off = centre - np.dot(r, centre)
    t = np.zeros(3)
    t[a], t[b] = off[0], off[1]
    return m, t


def prediction(name, shape):
    """the [1,2,D,H,W] fp32 predictions of tests/golden/resample_inverse.npz, regenerated from their names: channel 0 generic
    values, channel 1 a blocky 0 / 1 map"""
    g = detdata.normal(name, tuple(shape)).astype(np.float32)
    b = (detdata.uniform(name + ".b", tuple((n + 3) // 4 for n in shape)) > 0.5).astype(np.float32)
    b = b.repeat(4, 0).repeat(4, 1).repeat(4, 2)[:shape[0], :shape[1], :shape[2]]
    return np.stack([g, b])[None]
