"""What csrc/edt.hip computes, restated in numpy, and what its results are held to.

separable_sq   the float64 squared distance by three one-dimensional minima, g[j] = min_i (g[i] + ((j - i) s)^2) along axis
               0, then 1, then 2 from g0 = 0 on background / +inf on foreground: product, square, sum, each rounded once -
               the kernel's operations in the kernel's order, so the kernel's squared map must equal it in every element.
               A mask without background is seeded by one phantom background element at index (-1, 0, ...), scipy's rule.
brute_sq       the minimum over ALL background elements of scipy's expression ((d0 s0)^2 + (d1 s1)^2) + (d2 s2)^2
               (distance_transform_edt: dt = ft - indices; dt *= sampling; dt *= dt; add.reduce over axis 0), all pairs.
brute_sq_int   the same for unit sampling in int64: no rounding at all.
check_indices  an index map names, for every element, a background element (or the phantom (-1, 0, ...) of a mask without
               background) at which scipy's expression reproduces the returned squared distance bit for bit.
ulp_distance   |a - b| in units in the last place of b (float64).
"""
import numpy as np


def sampling_of(sampling, ndim):
    if sampling is None:
        return [1.0] * ndim
    s = [float(v) for v in np.atleast_1d(sampling)]
    return s * ndim if len(s) == 1 else s


def separable_sq(mask, sampling=None):
    mask = np.asarray(mask) != 0
    s = sampling_of(sampling, mask.ndim)
    g = np.where(mask, np.inf, 0.0)
    phantom = bool(mask.all())
    for ax in range(mask.ndim):
        n = mask.shape[ax]
        gm = np.moveaxis(g, ax, 0)
        if ax == 0 and phantom:                                     # one background element at (-1, 0, ...)
            seed = np.full((1,) + gm.shape[1:], np.inf)
            seed[(0,) + (0,) * (mask.ndim - 1)] = 0.0
            gm = np.concatenate([seed, gm], axis=0)
        pos = np.arange(gm.shape[0], dtype=np.float64)
        out = np.empty((n,) + gm.shape[1:])
        for j in range(n):
            jj = j + (gm.shape[0] - n)
            t = (jj - pos) * s[ax]
            t = t * t
            out[j] = (gm + t.reshape((-1,) + (1,) * (gm.ndim - 1))).min(axis=0)
        g = np.moveaxis(out, 0, ax)
    return np.ascontiguousarray(g)


def _background(mask):
    mask = np.asarray(mask) != 0
    if mask.all():
        return np.array([[-1] + [0] * (mask.ndim - 1)], np.int64)
    return np.argwhere(~mask).astype(np.int64)


def _chunk(nbg):
    """elements per slab of the all-pairs searches: about 2^21 pairs at a time"""
    return max(1, (1 << 21) // max(1, nbg))


def expression(delta, s):
    """scipy's squared distance of coordinate differences delta [..., ndim] (float64): ((d0 s0)^2 + (d1 s1)^2) + (d2 s2)^2"""
    acc = None
    for a in range(delta.shape[-1]):
        t = delta[..., a] * s[a]
        t = t * t
        acc = t if acc is None else acc + t
    return acc


def brute_sq(mask, sampling=None):
    mask = np.asarray(mask)
    s = sampling_of(sampling, mask.ndim)
    bg = _background(mask).astype(np.float64)
    at = np.argwhere(np.ones(mask.shape, bool)).astype(np.float64)
    out = np.empty(len(at))
    chunk = _chunk(len(bg))
    for a in range(0, len(at), chunk):
        out[a:a + chunk] = expression(at[a:a + chunk, None, :] - bg[None, :, :], s).min(axis=1)
    return out.reshape(mask.shape)


def brute_sq_int(mask):
    mask = np.asarray(mask)
    bg = _background(mask)
    at = np.argwhere(np.ones(mask.shape, bool)).astype(np.int64)
    out = np.empty(len(at), np.int64)
    chunk = _chunk(len(bg))
    for a in range(0, len(at), chunk):
        d = at[a:a + chunk, None, :] - bg[None, :, :]
        out[a:a + chunk] = (d * d).sum(axis=2).min(axis=1)
    return out.reshape(mask.shape)


def check_indices(mask, sampling, sq, idx):
    """asserts the feature transform idx [ndim, ...] against the mask and the squared distances sq"""
    mask = np.asarray(mask) != 0
    s = sampling_of(sampling, mask.ndim)
    idx = np.asarray(idx)
    assert idx.dtype == np.int32 and idx.shape == (mask.ndim,) + mask.shape, (idx.dtype, idx.shape)
    if mask.all():
        want = np.array([-1] + [0] * (mask.ndim - 1)).reshape((-1,) + (1,) * mask.ndim)
        assert (idx == want).all(), "a mask without background names the phantom element"
    else:
        for a in range(mask.ndim):
            assert idx[a].min() >= 0 and idx[a].max() < mask.shape[a], a
        assert not mask[tuple(idx[a] for a in range(mask.ndim))].any(), "an index names a foreground element"
    grid = np.indices(mask.shape).astype(np.float64)
    delta = np.moveaxis(idx.astype(np.float64) - grid, 0, -1)        # scipy: dt = ft - indices
    assert np.array_equal(expression(delta, s), sq), "scipy's expression at the index is not the returned distance"


def ulp_distance(a, b):
    """|a - b| / ulp(b), elementwise; 0 where both are equal (so inf == inf counts as 0)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b) / np.spacing(np.abs(b))
    return np.where(a == b, 0.0, d)
