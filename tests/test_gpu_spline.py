"""-m gpu tests of cubic-spline resampling (csrc/spline.hip through fplx.ops.spline_prefilter / resample_spline, and fplx.resample)
against scipy.ndimage itself.

Criterion (tests/splineoracle.py derives the bound): where the coordinates are outside the result is exactly 0; every element
satisfies |float64(got) - ref64| <= 2^-24 |ref64| + B with B <= 2^-40 max|x|; the elements not identical to scipy's float32
result are counted and printed, and pooled over a test function they are at most 1e-4 of at least 1e5 elements.  The
prefilter alone is held to scipy.ndimage.spline_filter(output=float64, mode='mirror') within prefilter_bound."""
import numpy as np
import pytest
import torch

import detdata
import resample_ref as R
import splineoracle as S
from test_resample_cpu import GENERIC_ANGLES, PLANES, SPECIAL_ANGLES, assert_close_to_scipy, scipy_rotation

pytestmark = pytest.mark.gpu

SEG = 32            # SP_SEG of csrc/spline.hip: the columns the W pass stages through LDS per step
LINES = 64          # SP_LINES: the lines of a W-pass block

# the shapes and zooms of tests/test_gpu_resample.py, and one volume with several blocks per pass
SHAPES = [((12, 40, 50), 1), ((9, 33, 31), 3), ((1, 37, 29), 1), ((7, 1, 23), 3), ((11, 19, 1), 1), ((5, 5, 5), 3),
          ((16, 32, 48), 1), ((3, 64, 17), 3), ((13, 27, 45), 1), ((2, 3, 2), 1), ((40, 64, 64), 1)]
ZOOMS = [(4.0 / 3, 1.2, 0.96), (0.83, 1.21, 0.9), (2.0, 2.0, 2.0), (0.5, 0.5, 0.5), (1.0, 0.7, 1.6), (1.37, 1.41, 1.96)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _volume(shape, channels, name):
    return (detdata.normal(name, (channels,) + tuple(shape)) * 100.0).astype(np.float32)


def _scipy_zoom(x, zoom, dtype):
    from scipy import ndimage
    return ndimage.zoom(x, [1.0] + list(zoom), order=3, output=dtype)


def _scipy_filter(x):
    from scipy import ndimage
    return np.stack([ndimage.spline_filter(c.astype(np.float64), 3, output=np.float64, mode="mirror") for c in x])


def _check_prefilter(x, what):
    from fplx import ops
    coef = ops.spline_prefilter(_dev(x))
    assert coef.dtype == torch.float64 and coef.is_cuda and tuple(coef.shape) == x.shape
    got, ref = coef.cpu().numpy(), _scipy_filter(x)
    xmax = float(np.abs(x).max())
    b = S.prefilter_bound(xmax)
    assert b <= S.CAP * xmax
    err = float(np.abs(got - ref).max())
    print("%s: prefilter max |got - scipy| = %.3g (bound %.3g, %.1f ulp of max|x|)" % (what, err, b, err / (S.U * 2 * xmax)))
    assert err <= b, (what, err, b)
    return got


@pytest.mark.parametrize("shape", [(1, 37, 29), (7, 1, 23), (11, 19, 1), (2, 3, 2), (5, 5, 5)])
@pytest.mark.parametrize("channels", [1, 3])
def test_prefilter_line_lengths(shape, channels):
    """extents 1, 2, 3 and 5 along each axis: length 2 empties the start-up sum, length 1 skips the axis"""
    _check_prefilter(_volume(shape, channels, "sp.gpu.len"), ("lengths", shape, channels))


@pytest.mark.parametrize("w", [SEG - 1, SEG, SEG + 1, 2 * SEG + 7])
def test_prefilter_w_segments(w):
    """W shorter than the W pass's LDS segment, equal to it, one more, and two segments and a remainder"""
    _check_prefilter(_volume((3, 4, w), 1, "sp.gpu.seg"), ("segments", w))


@pytest.mark.parametrize("shape,channels", [((3, 5, 40), 1), ((5, 13, 40), 1), ((5, 13, 40), 3), ((9, 15, 33), 3)])
def test_prefilter_line_counts_and_channels(shape, channels):
    """D x H line counts of 15, 65, 195 and 405: less than one W-pass tile of lines, a tile and one line, tiles and a remainder"""
    assert (channels * shape[0] * shape[1]) % LINES != 0
    x = _volume(shape, channels, "sp.gpu.lines")
    whole = _check_prefilter(x, ("lines", shape, channels))
    from fplx import ops
    for c in range(channels):                 # one launch with C channels equals C launches with one
        assert np.array_equal(whole[c:c + 1], ops.spline_prefilter(_dev(x[c:c + 1])).cpu().numpy()), c


def _resample(x, m, t, out):
    from fplx import ops
    y = ops.resample_spline(_dev(x), m, t, out, 3)
    assert y.dtype == torch.float32 and y.is_cuda and tuple(y.shape) == (x.shape[0],) + tuple(out)
    return y.cpu().numpy()


def test_zoom_equals_scipy():
    pool = S.Pool("zoom, order 3")
    for shape, channels in SHAPES:
        x = _volume(shape, channels, "sp.gpu.zoom")
        xmax = float(np.abs(x).max())
        for zoom in ZOOMS:
            out = R.zoom_size(shape, zoom)
            if min(out) < 1:
                continue                              # scipy refuses an empty output
            m, t = R.zoom_affine(shape, out)
            S.check(_resample(x, m, t, out), _scipy_zoom(x, zoom, np.float32), _scipy_zoom(x, zoom, np.float64), xmax,
                    ("zoom", shape, channels, zoom), pool, S.outside(shape, m, t, out))
    pool.check()


def test_rotate_equals_scipy():
    """the matrix and the offset are scipy's own (cosdg / sindg, its matrix-vector product)"""
    from scipy import ndimage
    pool = S.Pool("rotate, order 3")
    for shape, channels in (((12, 40, 50), 1), ((9, 33, 31), 3)):
        x = _volume(shape, channels, "sp.gpu.rot")
        xmax = float(np.abs(x).max())
        for angle in GENERIC_ANGLES + SPECIAL_ANGLES:
            for axes in PLANES:
                m, t = scipy_rotation(shape, angle, axes)
                ref32 = ndimage.rotate(x, angle, axes, reshape=False, order=3)
                ref64 = ndimage.rotate(x, angle, axes, reshape=False, order=3, output=np.float64)
                S.check(_resample(x, m, t, shape), ref32, ref64, xmax, ("rotate", shape, angle, axes), pool,
                        S.outside(shape, m, t, shape))
    pool.check()


def test_general_matrix_equals_restatement_and_nan_reads_nothing():
    """shear + anisotropic scale + offset: no scipy wrapper builds it; the restatement (held to scipy on the CPU) does"""
    shape, out = (9, 21, 26), (11, 19, 30)
    x = _volume(shape, 2, "sp.gpu.affine")
    m = np.array([[0.93, 0.11, -0.07], [-0.21, 1.08, 0.13], [0.05, -0.17, 0.89]])
    t = np.array([0.6, 2.3, 1.9])
    ref64 = S.resample(x, m, t, out, np.float64)
    S.check(_resample(x, m, t, out), ref64.astype(np.float32), ref64, float(np.abs(x).max()), "general matrix", None,
            S.outside(shape, m, t, out))
    bad = m.copy()
    bad[1, 1] = np.nan
    assert not _resample(x, bad, t, out).any()


def test_impulses_at_corners_edge_and_interior():
    """a unit impulse at every corner, on an edge and in the interior of 4x5x6 under zoom 1.5: a wrong reflection shows here"""
    shape, zoom = (4, 5, 6), (1.5, 1.5, 1.5)
    out = R.zoom_size(shape, zoom)
    m, t = R.zoom_affine(shape, out)
    places = [(d, h, w) for d in (0, 3) for h in (0, 4) for w in (0, 5)] + [(0, 2, 0), (3, 4, 3), (2, 2, 3), (1, 3, 2)]
    for p in places:
        x = np.zeros((1,) + shape, np.float32)
        x[(0,) + p] = 1.0
        got = _resample(x, m, t, out)
        S.check(got, _scipy_zoom(x, zoom, np.float32), _scipy_zoom(x, zoom, np.float64), 1.0, ("impulse", p), None,
                S.outside(shape, m, t, out))
        assert got.any()


def test_same_call_twice_gives_the_same_bits():
    from fplx import ops
    shape = (7, 45, 2 * SEG + 7)
    x = _dev(_volume(shape, 3, "sp.gpu.det"))
    m, t = scipy_rotation(shape, 17.3, (-1, -2))
    c1, c2 = ops.spline_prefilter(x), ops.spline_prefilter(x)
    assert torch.equal(c1, c2)
    y1, y2 = ops.resample_spline(x, m, t, shape), ops.resample_spline(x, m, t, shape)
    assert torch.equal(y1, y2)


# ---- fplx.resample

def test_resample_orders_0_and_1_are_resample_affine():
    from fplx import ops, resample
    from fplx.transform import _rotate_affine
    shape, zoom = (9, 33, 31), (1.37, 0.7, 1.21)
    x = _dev(_volume(shape, 2, "sp.gpu.api"))
    lab = _dev((detdata.uniform("sp.gpu.api.lab", (2,) + shape) * 4).astype(np.uint8))
    out = R.zoom_size(shape, zoom)
    mz, tz = R.zoom_affine(shape, out)
    mr, tr = _rotate_affine(shape, 17.3, (-1, -3))
    ma, ta = [[0.93, 0.11, -0.07], [-0.21, 1.08, 0.13], [0.05, -0.17, 0.89]], [0.6, 2.3, 1.9]
    for v, order in ((x, 0), (x, 1), (lab, 0)):
        assert torch.equal(resample.zoom(v, zoom, order), ops.resample_affine(v, mz, tz, out, order))
        assert torch.equal(resample.rotate(v, 17.3, (-1, -3), order), ops.resample_affine(v, mr, tr, shape, order))
        assert torch.equal(resample.affine(v, ma, ta, (8, 30, 35), order), ops.resample_affine(v, ma, ta, (8, 30, 35), order))


def test_resample_order_3_meets_the_criterion():
    from scipy import ndimage
    from fplx import resample
    pool = S.Pool("fplx.resample, order 3")
    shape = (16, 40, 50)
    x = _volume(shape, 2, "sp.gpu.api3")
    xmax = float(np.abs(x).max())
    for zoom in ZOOMS[:3]:
        out = R.zoom_size(shape, zoom)
        m, t = R.zoom_affine(shape, out)
        got = resample.zoom(_dev(x), zoom)                                     # order 3 is the default, as in scipy
        S.check(got.cpu().numpy(), _scipy_zoom(x, zoom, np.float32), _scipy_zoom(x, zoom, np.float64), xmax, ("api zoom", zoom),
                pool, S.outside(shape, m, t, out))
    got = resample.zoom(_dev(x), 1.5).cpu().numpy()
    m, t = R.zoom_affine(shape, got.shape[1:])
    S.check(got, _scipy_zoom(x, [1.5] * 3, np.float32), _scipy_zoom(x, [1.5] * 3, np.float64), xmax, "api scalar zoom", pool,
            S.outside(shape, m, t, got.shape[1:]))
    # at the right angles the host's cos / sin are scipy's cosdg / sindg to the bit, so scipy itself is the reference
    for angle, axes in ((90.0, (-1, -2)), (180.0, (-1, -3)), (270.0, (-2, -3))):
        got = resample.rotate(_dev(x), angle, axes).cpu().numpy()
        m, t = scipy_rotation(shape, angle, axes)
        S.check(got, ndimage.rotate(x, angle, axes, reshape=False, order=3),
                ndimage.rotate(x, angle, axes, reshape=False, order=3, output=np.float64), xmax, ("api rotate", angle), pool,
                S.outside(shape, m, t, shape))
    m = [[0.93, 0.11, -0.07], [-0.21, 1.08, 0.13], [0.05, -0.17, 0.89]]
    ref64 = S.resample(x, m, [0.6, 2.3, 1.9], (11, 19, 30), np.float64)
    S.check(resample.affine(_dev(x), m, [0.6, 2.3, 1.9], (11, 19, 30), 3).cpu().numpy(), ref64.astype(np.float32), ref64, xmax,
            "api affine", None, S.outside(shape, m, [0.6, 2.3, 1.9], (11, 19, 30)))
    pool.check()


def test_resample_refusals():
    from fplx import ops, resample
    x = torch.zeros((1, 4, 5, 6), device="cuda:0")
    eye = np.eye(3)
    for order in (2, 4, 5):
        for call in (lambda: resample.zoom(x, 1.5, order), lambda: resample.rotate(x, 10.0, (-1, -2), order),
                     lambda: resample.affine(x, eye, (0, 0, 0), (4, 5, 6), order),
                     lambda: resample.resample_to_spacing(x, (1, 1, 1), (2, 2, 2), order)):
            with pytest.raises(ValueError, match=r"built: 0, 1, 3"):
                call()
        with pytest.raises(ValueError, match=r"built: 3"):
            ops.resample_spline(x, eye, (0, 0, 0), (4, 5, 6), order)
        with pytest.raises(ValueError, match=r"built: 3"):
            ops.spline_prefilter(x, order)
    for order in (0, 1, 3):
        with pytest.raises(RuntimeError, match="must live on the GPU"):                    # no CPU fallback
            resample.zoom(torch.zeros((1, 4, 5, 6)), 1.5, order)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ops.spline_prefilter(torch.zeros((1, 4, 5, 6)))
    lab = torch.zeros((1, 4, 5, 6), dtype=torch.uint8, device="cuda:0")
    with pytest.raises(ValueError, match="uint8"):
        resample.zoom(lab, 1.5, 3)
    with pytest.raises(ValueError, match="uint8"):
        resample.zoom(lab, 1.5, 1)
    assert resample.zoom(lab, 1.5, 0).dtype == torch.uint8
    with pytest.raises(ValueError, match="float32"):
        ops.resample_spline(lab, eye, (0, 0, 0), (4, 5, 6))
    with pytest.raises(ValueError):
        ops.resample_spline(x.double(), eye, (0, 0, 0), (4, 5, 6))
    with pytest.raises(ValueError):
        resample.zoom(x, 0.1, 3)                                 # an empty output: int(round(4 * 0.1)) == 0
    with pytest.raises(ValueError):
        resample.affine(x, eye, (0, 0, 0), (4, 0, 6), 3)
    with pytest.raises(ValueError):
        resample.zoom(x[0], 1.5, 3)                              # a [D,H,W] tensor


def test_resample_to_spacing_keeps_the_reference_axis_assignment():
    """spacing (0.5, 0.8, 1.5) to (1, 1, 1): zoom (x, y, z) = (0.5, 0.8, 1.5), applied as [1.5, 0.5, 0.8] on [D,H,W]"""
    from scipy import ndimage
    from fplx import resample
    shape = (10, 40, 45)
    x = _volume(shape, 1, "sp.gpu.spacing")
    zoom = [1.5 / 1, 0.5 / 1, 0.8 / 1]
    for order in (0, 1, 3):
        got, spacing = resample.resample_to_spacing(_dev(x), (0.5, 0.8, 1.5), (1, 1, 1), order)
        assert spacing == (1.0, 1.0, 1.0)
        assert tuple(got.shape) == (1, 15, 20, 36)
        ref32 = ndimage.zoom(x[0], zoom, order=order)[None]
        if order == 3:
            m, t = R.zoom_affine(shape, got.shape[1:])
            S.check(got.cpu().numpy(), ref32, ndimage.zoom(x[0], zoom, order=3, output=np.float64)[None], float(np.abs(x).max()),
                    "resample_to_spacing", None, S.outside(shape, m, t, got.shape[1:]))
        elif order == 1:
            assert_close_to_scipy(got.cpu().numpy(), ref32, "resample_to_spacing, order 1")
        else:
            assert np.array_equal(got.cpu().numpy(), ref32)
