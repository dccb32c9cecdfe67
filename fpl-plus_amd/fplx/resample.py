"""Resampling of [C,D,H,W] device volumes with scipy.ndimage's semantics (mode='constant', cval=0) at spline orders 0, 1 and 3:
what the reference's dataset preparation calls on the host - ndimage.zoom(img_sub, zoom) in data/preprocess_vs.py (order 3,
scipy's default) and resample_sitk_image_to_given_spacing(image, spacing, order) in PyMIC/pymic/util/image_process.py:210-228.

Orders 0 and 1 are ops.resample_affine, unchanged (csrc/resample.hip: scipy's bits).  Order 3 is ops.resample_spline
(csrc/spline.hip): the B-spline prefilter and the 64-tap interpolation, within a derived float64 rounding bound of scipy
(tests/splineoracle.py).  Orders 2, 4 and 5 are not built.  uint8 volumes (labels) take order 0 only."""
import numbers

import torch

from . import ops
from .transform import _rotate_affine

ORDERS = (0, 1) + tuple(ops.SPLINE_ORDERS)


def _check(x, order, who):
    if not torch.is_tensor(x) or x.dim() != 4:
        raise ValueError("fplx.resample.{0:} takes a [C,D,H,W] device tensor".format(who))
    if isinstance(order, bool) or not isinstance(order, numbers.Real) or int(order) != order or int(order) not in ORDERS:
        raise ValueError("fplx.resample.{0:}: spline order {1:} is not built (built: {2:})".format(
            who, order, ", ".join(str(o) for o in ORDERS)))
    ops.require_gpu(x)
    if x.dtype == torch.uint8 and int(order) != 0:
        raise ValueError("fplx.resample.{0:}: uint8 volumes take order 0 only".format(who))
    return int(order)


def affine(x, matrix, offset, out_size, order=3):
    """scipy.ndimage.affine_transform(x[c], matrix, offset, output_shape=out_size, order=order) for every channel:
    y[c][o] = interp(x[c], matrix o + offset), 0 outside the volume"""
    order = _check(x, order, "affine")
    x = x.contiguous()
    if order in ops.SPLINE_ORDERS:
        return ops.resample_spline(x, matrix, offset, out_size, order)
    return ops.resample_affine(x, matrix, offset, out_size, order)


def zoom_size(shape, zoom):
    """scipy.ndimage.zoom's output extents: int(round(n * zoom)) with Python's round"""
    return [int(round(shape[i] * zoom[i])) for i in range(3)]


def zoom(x, zoom, order=3):
    """scipy.ndimage.zoom(x, [1] + zoom, order=order): zoom is a number or one factor per axis (D, H, W).  The coordinate step
    is (n - 1) / (out - 1), not 1 / zoom, and 1.0 where out == 1, as in fplx.transform._zoom"""
    order = _check(x, order, "zoom")
    zoom = [float(zoom)] * 3 if isinstance(zoom, numbers.Real) else [float(z) for z in zoom]      # numpy scalars are Real
    if len(zoom) != 3:
        raise ValueError("fplx.resample.zoom takes one factor, or one per axis (D, H, W)")
    shape = x.shape[1:]
    out = zoom_size(shape, zoom)
    step = [(shape[i] - 1.0) / (out[i] - 1.0) if out[i] > 1 else 1.0 for i in range(3)]
    m = [[step[i] if i == j else 0.0 for j in range(3)] for i in range(3)]
    return affine(x, m, (0.0, 0.0, 0.0), out, order)


def rotate(x, angle, axes, order=3):
    """scipy.ndimage.rotate(x, angle, axes, reshape=False, order=order): angle in degrees, axes two of -1, -2, -3 (W, H, D)"""
    order = _check(x, order, "rotate")
    m, t = _rotate_affine(x.shape[1:], angle, axes)
    return affine(x, m, t, x.shape[1:], order)


def spacing_zoom(spacing, new_spacing):
    """the zoom factors (D, H, W) of image_process.py:221-222, kept literally: zoom = spacing / new_spacing per (x, y, z), then
    [zoom[2], zoom[0], zoom[1]] on the [D,H,W] array - z's factor on D, but x's on H and y's on W, although H is the y axis
    of the array and W its x axis."""
    if len(spacing) != 3 or len(new_spacing) != 3:
        raise ValueError("fplx.resample: spacings are (x, y, z) triples")
    z = [float(spacing[i]) / float(new_spacing[i]) for i in range(3)]
    return [z[2], z[0], z[1]]


def resample_to_spacing(x, spacing, new_spacing, order=3):
    """resample_sitk_image_to_given_spacing (image_process.py:210-228): x [C,D,H,W], spacing and new_spacing (x, y, z) as
    SimpleITK gives them -> (volume, new_spacing as a tuple).

    The reference's axis assignment is kept literally (spacing_zoom): x's factor lands on H and y's on W.  With equal in-plane
    spacing, as in every shipped volume, that is the same as the right assignment; with unequal spacing it reproduces the
    reference, not the geometry."""
    return zoom(x, spacing_zoom(spacing, new_spacing), order), tuple(float(v) for v in new_spacing)
