"""Generates tests/golden/postprocess.npz by RUNNING the reference's post-processing
(the reference's PyMIC/pymic/util/post_process.py: PostKeepLargestComponent, mode 1; util/image_process.py:139-163:
get_largest_k_components, applied per foreground class for mode 2 - the reference's own mode 2 returns its input, see
DESIGN.md), imported with the stub modules of _ref_import.py and scipy.  Build-container only; the GPU box reads the
fixture.

Inputs: detdata-seeded blob masks (a smoothed random map cut into 1-3 classes, plus islands) at odd shapes, 2D and 3D, and
the shipped label volume nifti/vs_gk_98_t2_lab.nii.gz with islands added.  Every input is checked to have a unique
largest component (per class for mode 2), so that the reference ran on its defined path."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "fpl-plus_amd"))
import _ref_import  # noqa: E402
import detdata  # noqa: E402

_ref_import.install()
import scipy.ndimage as ndi  # noqa: E402
from pymic.util.post_process import PostKeepLargestComponent  # noqa: E402
from pymic.util.image_process import get_largest_k_components  # noqa: E402

# (name, shape, classes)
CASES = [("blob_a", (17, 41, 67), 1), ("blob_b", (23, 37, 91), 2), ("blob_c", (9, 65, 130), 3),
         ("blob_2d", (77, 131), 2), ("blob_d", (5, 3, 301), 1), ("blob_e", (40, 33, 19), 3)]


def _smooth(a, passes=3):
    """box filter of width 5 along every axis, `passes` times (a plain-numpy low-pass: no scipy in the input path)"""
    for _ in range(passes):
        for ax in range(a.ndim):
            p = np.pad(a, [(2, 2) if k == ax else (0, 0) for k in range(a.ndim)], mode="edge")
            n = a.shape[ax]
            a = sum(np.take(p, np.arange(j, j + n), axis=ax) for j in range(5)) / 5.0
    return a


def blob_mask(name, shape, classes):
    """a smooth random map cut at thresholds into classes 0..classes (class k where the map lies in the k-th band above
    0.35 standard deviations), plus single-voxel and 2x2(x2) islands of random classes"""
    f = _smooth(detdata.normal(name + ".field", shape).astype(np.float64))
    f = f / f.std()
    cuts = np.linspace(0.35, 2.0, classes + 1)[:-1]
    seg = np.zeros(shape, np.uint8)
    for k, c in enumerate(cuts):
        seg[f > c] = k + 1
    u = detdata.uniform(name + ".islands", (40, 1 + len(shape)))
    for row in u:
        at = [int(row[1 + a] * (shape[a] - 1)) for a in range(len(shape))]
        size = 1 if row[0] < 0.5 else 2
        sl = tuple(slice(p, min(p + size, shape[a])) for a, p in enumerate(at))
        seg[sl] = 1 + int(row[0] * 97) % classes
    return seg


def vs_with_islands():
    from fplx.nifti import load_nifty_volume_as_4d_array
    lab = load_nifty_volume_as_4d_array(os.path.join(HERE, "nifti", "vs_gk_98_t2_lab.nii.gz"))["data_array"][0]
    seg = np.asarray(lab > 0, np.uint8)
    u = detdata.uniform("vs.islands", (25, 3))
    for i, row in enumerate(u):
        z, y, x = [int(row[a] * (seg.shape[a] - 3)) for a in range(3)]
        seg[z:z + 1 + i % 3, y:y + 2, x:x + 1 + i % 2] = 1
    return seg


def _unique_largest(mask):
    st = ndi.generate_binary_structure(mask.ndim, 1)
    lab, n = ndi.label(mask, st)
    if n == 0:
        return True
    sizes = np.bincount(lab.ravel())[1:]
    return int((sizes == sizes.max()).sum()) == 1


def main():
    keep1 = PostKeepLargestComponent({"keeplargestcomponent_mode": 1})
    out = {}
    inputs = [(n, blob_mask(n, s, c)) for n, s, c in CASES] + [("vs_islands", vs_with_islands())]
    for name, seg in inputs:
        assert _unique_largest(seg > 0), name
        classes = [int(c) for c in np.unique(seg) if c]
        for c in classes:
            assert _unique_largest(seg == c), (name, c)
        m1 = np.asarray(keep1(seg.copy()), np.uint8)
        m2 = np.zeros_like(seg)
        for c in range(1, int(seg.max()) + 1):                     # the documented intent of mode 2 (post_process.py:41-44)
            m2 = m2 + np.asarray(get_largest_k_components(np.asarray(seg == c, np.uint8)), np.uint8) * c
        assert m1.any() and not np.array_equal(m1, seg), name    # the islands were really removed
        out[name + ".seg"] = seg
        out[name + ".mode1"] = m1
        out[name + ".mode2"] = m2.astype(np.uint8)
        print(name, seg.shape, classes, int((seg > 0).sum()), int((m1 > 0).sum()), int((m2 > 0).sum()))
    out["names"] = np.array([n for n, _ in inputs])
    np.savez_compressed(os.path.join(HERE, "postprocess.npz"), **out)


if __name__ == "__main__":
    main()
