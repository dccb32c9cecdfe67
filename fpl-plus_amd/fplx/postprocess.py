"""Prediction post-processing - the reference's PyMIC/pymic/util/post_process.py:1-49 and
util/image_process.get_largest_k_components (139-163), with the connected-component labelling on the device
(csrc/postprocess.hip) instead of scipy.ndimage.label.

Calling contract of the reference: a post-processor takes one predicted volume [D, H, W] (or [H, W]) and returns the
processed volume; numpy in, numpy out, so a plugin's own post-processor (SegmentationAgent.set_postprocessor) keeps
working.  A device tensor in gives a device tensor out.

Deliberate differences ("Prediction post-processing"):
 - mode 2 keeps the largest component of every foreground class; the reference builds that result and then returns its
   input unchanged;
 - every component of the maximal size is kept (the reference's tie path fails or compares the wrong axis);
 - get_largest_k_components takes k = 1 only.
"""
import numpy as np
import torch

from . import ops


def _to_device_uint8(seg):
    """-> (uint8 device tensor, how to give the result back)"""
    if isinstance(seg, torch.Tensor):
        if not seg.is_cuda:
            raise ValueError("fplx: post-processing takes a numpy array or a device tensor, got a host tensor")
        if seg.dtype != torch.uint8:
            raise ValueError("fplx: post-processing takes uint8 device volumes, got {0:}".format(seg.dtype))
        return seg, None
    arr = np.asarray(seg)
    if arr.dtype != np.bool_ and not np.issubdtype(arr.dtype, np.integer):
        raise ValueError("fplx: post-processing takes an integer label volume, got dtype {0:}".format(arr.dtype))
    if arr.ndim not in (2, 3):
        raise ValueError("the dimension number should be 2 or 3")                  # image_process.py:153
    if arr.size and (int(arr.min()) < 0 or int(arr.max()) > 255):
        raise ValueError("fplx: post-processing takes labels in [0, 255]")
    t = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.uint8)).cuda()
    return t, arr.dtype


def _back(t, dtype):
    return t if dtype is None else t.cpu().numpy().astype(dtype, copy=False)


def _check_dims(t):
    if t.dim() not in (2, 3):
        raise ValueError("the dimension number should be 2 or 3")
    if t.numel() == 0:
        raise ValueError("fplx: post-processing of an empty volume")


def get_largest_k_components(image, k=1):
    """image_process.py:139-163 for k = 1: the mask (0 / 1 in the input's dtype) of the largest 6-connected (2D: 4-connected)
    component(s) of the nonzero voxels; an image without foreground comes back unchanged."""
    if k != 1:
        raise ValueError("fplx: get_largest_k_components supports k = 1 only (got k = {0!r})".format(k))
    t, dtype = _to_device_uint8(image)
    _check_dims(t)
    out = ops.keep_largest_component(t, 1)
    if dtype is None:
        return (out != 0).to(image.dtype)
    out = out.cpu().numpy()
    if not out.any():                                              # image.sum() == 0: the input itself (line 149)
        return image
    return (out != 0).astype(dtype)


class PostProcess(object):
    """post_process.py:8-16: the abstract post-processor (identity)"""

    def __init__(self, params):
        self.params = params

    def __call__(self, seg):
        return seg


class PostKeepLargestComponent(PostProcess):
    """post_process.py:18-45.  params key `keeplargestcomponent_mode` (the config parser lower-cases keys):
    1 keeps the largest component of the union of the foreground classes, 2 the largest component of each foreground
    class.  The kept voxels keep their class values; everything else becomes 0."""

    def __init__(self, params):
        super(PostKeepLargestComponent, self).__init__(params)
        self.mode = params.get("KeepLargestComponent_mode".lower(), 1)
        if self.mode not in (1, 2):
            raise ValueError("fplx: KeepLargestComponent_mode must be 1 or 2, got {0!r}".format(self.mode))

    def __call__(self, seg):
        t, dtype = _to_device_uint8(seg)
        _check_dims(t)
        return _back(ops.keep_largest_component(t, self.mode), dtype)


PostProcessDict = {
    'KeepLargestComponent': PostKeepLargestComponent}
