"""The distance maps of the reference's PyMIC/pymic/util/image_process.py on the GPU: get_euclidean_distance (lines
165-192) and the scipy.ndimage.distance_transform_edt it calls, on the exact kernels of csrc/edt.hip (fplx.ops.edt_squared /
edt_finish).  The file's other functions are mirrored elsewhere: bounding box, crop, ROI paste, crop-and-pad and label
conversion in fplx.transform and fplx.ops, the largest component in fplx.postprocess, resampling in fplx.resample.

numpy in gives numpy out (float64 distances, int32 indices); a device tensor in gives device tensors out, without a host
copy of the volume.  There is no CPU path: a numpy input is copied to the current GPU and back.
"""
import numpy as np
import torch

from . import ops


def _to_device_mask(a, as_mask):
    """-> (uint8 device tensor of as_mask(a), input was numpy); the comparison runs where the data is"""
    if isinstance(a, torch.Tensor):
        ops.require_gpu(a)
        return as_mask(a).to(torch.uint8).contiguous(), False
    m = np.ascontiguousarray(np.asarray(as_mask(np.asarray(a)), np.uint8))
    if not torch.cuda.is_available():
        raise RuntimeError("fplx: the distance transform runs on the GPU (HIP path only, no CPU fallback)")
    return torch.from_numpy(m).cuda(), True


def distance_transform_edt(input, sampling=None, return_distances=True, return_indices=False):
    """scipy.ndimage.distance_transform_edt of a 2D or 3D array (any dtype, nonzero = foreground): the exact Euclidean
    distance of every element to the nearest zero element under `sampling` (a scalar or one value per axis), and / or the
    int32 indices [ndim, ...] of such an element.  Without scipy's `distances=` / `indices=` output arguments.  The squared
    distances equal scipy's bit for bit and the root is taken once; among several zero elements at the same distance the
    indices may name another one than scipy's.  An input without a zero gets scipy's result: the distance to index
    (-1, 0, 0) (2D: (-1, 0))."""
    nd = input.dim() if isinstance(input, torch.Tensor) else np.ndim(input)
    if nd not in (2, 3):
        raise ValueError("fplx: distance_transform_edt takes a 2D or 3D input, got {0:}D".format(nd))
    s = ops.edt_sampling(sampling, nd)
    if not (return_distances or return_indices):
        raise RuntimeError("at least one of return_distances/return_indices must be True")       # scipy's error
    mask, host = _to_device_mask(input, lambda a: a != 0)
    r = ops.edt_squared(mask, s, return_indices)
    sq, idx = r if return_indices else (r, None)
    out = []
    if return_distances:
        out.append(ops.edt_finish(sq))
    if return_indices:
        out.append(idx)
    if host:
        out = [t.cpu().numpy() for t in out]
    return out[0] if len(out) == 1 else tuple(out)


def get_euclidean_distance(image, dim=3, spacing=[1.0, 1.0, 1.0]):
    """The reference's signed distance map of a 3D binary image (util/image_process.py:165-192):
    edt(image <= 0.5) - edt(image > 0.5) in float64 - positive inside the object, negative outside.  One batched kernel
    call transforms the two masks, a second one takes the roots and the difference.

    :param image: the 3D array (numpy, or a device tensor).
    :param dim: 3; dim = 2 and every other value raise the reference's ValueErrors.
    :param spacing: accepted and IGNORED, exactly as in the reference, whose two calls pass no sampling: the distances are in
        voxels.  For physical distances use distance_transform_edt(sampling=spacing) on the two masks."""
    input_dim = image.dim() if isinstance(image, torch.Tensor) else np.ndim(image)
    if input_dim != 3:
        raise ValueError("Not implemented for {0:}D image".format(input_dim))
    if dim == 2:
        raise ValueError("Not implemented for {0:}D image".format(input_dim))
    elif dim != 3:
        raise ValueError("Not implemented for {0:}D distance".format(dim))
    both = torch.stack if isinstance(image, torch.Tensor) else np.stack
    masks, host = _to_device_mask(image, lambda a: both([a > 0.5, a <= 0.5]))       # the reference's two comparisons (a NaN: neither)
    sq = ops.edt_squared(masks, None, False, batched=True)
    out = ops.edt_finish(sq[0], sq[1])
    return out.cpu().numpy() if host else out
