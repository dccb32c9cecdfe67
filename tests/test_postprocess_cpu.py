"""CPU tests of prediction post-processing (fplx/postprocess.py, fplx_cc_label / fplx_keep_largest_component): a scipy
restatement of KeepLargestComponent that reproduces the reference's fixture, the config surface, and argument rejection
before any device work.  The restatement is shared with tests/test_gpu_postprocess.py."""
import ctypes
import os

import numpy as np
import pytest

import scipy.ndimage as scipy_ndimage  # noqa: E402


# ---- restatement (scipy): canonical labels and the kept components
def canonical_labels(seg, per_class=False):
    """scipy.ndimage.label under the 6-face (2D: 4-neighbour) structure, relabelled to the C-order linear index of each
    component's first voxel; -1 for background.  per_class: every class labelled on its own."""
    seg = np.asarray(seg)
    st = scipy_ndimage.generate_binary_structure(seg.ndim, 1)
    out = np.full(seg.shape, -1, np.int64)
    classes = [c for c in np.unique(seg) if c] if per_class else [None]
    flat_out = out.ravel()
    for c in classes:
        lab, n = scipy_ndimage.label(seg == c if per_class else seg != 0, st)
        flat = lab.ravel()
        ids, first = np.unique(flat, return_index=True)
        table = np.zeros(n + 1, np.int64)
        table[ids] = first
        sel = flat > 0
        flat_out[sel] = table[flat[sel]]
    return out


def keep_largest_ref(seg, mode):
    """the documented intent of PostKeepLargestComponent: mode 1 keeps the largest component(s) of the foreground, mode 2
    those of every foreground class; every component of the maximal size is kept; kept voxels keep their values"""
    seg = np.asarray(seg)
    lab = canonical_labels(seg, per_class=(mode == 2))
    out = np.zeros_like(seg)
    fg = lab >= 0
    if not fg.any():
        return out
    sizes = np.bincount(lab[fg], minlength=seg.size)
    cls = seg if mode == 2 else (seg != 0).astype(seg.dtype)
    for c in np.unique(cls[fg]):
        roots = np.unique(lab[fg & (cls == c)])
        best = sizes[roots].max()
        keep = roots[sizes[roots] == best]
        m = np.isin(lab, keep)
        out[m] = seg[m]
    return out


def test_restatement_reproduces_the_reference_fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "postprocess.npz"))
    names = [str(n) for n in z["names"]]
    assert len(names) >= 6 and "vs_islands" in names
    assert any(z[n + ".seg"].ndim == 2 for n in names)
    for n in names:
        seg = z[n + ".seg"]
        for mode in (1, 2):
            want = z["%s.mode%d" % (n, mode)]
            assert np.array_equal(keep_largest_ref(seg, mode), want), (n, mode)


def test_restatement_labels_and_ties():
    seg = np.zeros((3, 4, 5), np.uint8)
    seg[0, 0, 0:2] = 1           # size 2
    seg[2, 3, 3:5] = 2           # size 2: tie with the first in mode 1
    seg[1, 1, 1] = 2             # single voxel touching nothing (6-connectivity)
    seg[0, 0, 2] = 2             # joins the first run in mode 1 only
    lab1 = canonical_labels(seg)
    assert lab1[0, 0, 2] == 0 and lab1[2, 3, 4] == 2 * 20 + 3 * 5 + 3 and lab1[1, 1, 1] == 20 + 5 + 1
    lab2 = canonical_labels(seg, per_class=True)
    assert lab2[0, 0, 2] == 2 and lab2[0, 0, 1] == 0
    k1 = keep_largest_ref(seg, 1)
    assert k1[0, 0, :3].tolist() == [1, 1, 2] and k1[2, 3].sum() == 0 and k1[1, 1, 1] == 0
    k2 = keep_largest_ref(seg, 2)                     # class 2: the run of two at the far corner; class 1: its run
    assert k2[2, 3, 3:5].tolist() == [2, 2] and k2[0, 0, 2] == 0 and k2[0, 0, :2].tolist() == [1, 1]
    seg[2, 3, 3:5] = 1
    seg[0, 0, 2] = 0
    assert np.array_equal(keep_largest_ref(seg, 1) != 0, (seg == 1))   # tie of two runs of two: both kept


def test_post_process_parses_from_a_config_with_the_line_enabled(golden_dir, tmp_path):
    import fplx
    from fplx.config import parse_config
    src = open(os.path.join(golden_dir, "sample_vs.cfg")).read()
    cfg = tmp_path / "pp.cfg"
    cfg.write_text(src.replace("[testing]\n", "[testing]\npost_process = KeepLargestComponent\n"
                               "KeepLargestComponent_mode = 2\n"))
    t = parse_config(str(cfg))["testing"]
    assert t["post_process"] == "KeepLargestComponent" and t["keeplargestcomponent_mode"] == 2
    p = fplx.PostProcessDict[t["post_process"]](t)
    assert isinstance(p, fplx.PostKeepLargestComponent) and isinstance(p, fplx.PostProcess) and p.mode == 2
    assert fplx.PostKeepLargestComponent({}).mode == 1
    assert fplx.postprocess.PostProcessDict is fplx.PostProcessDict and list(fplx.PostProcessDict) == ["KeepLargestComponent"]
    seg = np.ones((2, 3), np.uint8)
    assert fplx.PostProcess({})(seg) is seg
    with pytest.raises(KeyError):
        fplx.PostProcessDict["KeepLargestComponents"]


def test_bad_arguments_are_rejected_before_any_device_work():
    import torch
    import fplx
    from fplx import postprocess as pp
    img = np.zeros((4, 5, 6), np.uint8)
    img[1, 1, 1] = 1
    with pytest.raises(ValueError):
        pp.get_largest_k_components(img, k=2)
    with pytest.raises(ValueError):
        pp.get_largest_k_components(img, k=0)
    keep = fplx.PostKeepLargestComponent({"keeplargestcomponent_mode": 1})
    for bad in (np.zeros((4,), np.uint8), np.zeros((2, 3, 4, 5), np.uint8), np.zeros((3, 4), np.float32),
                np.full((3, 4), 256, np.int32), np.full((3, 4), -1, np.int16), torch.zeros((3, 4), dtype=torch.uint8)):
        with pytest.raises(ValueError):
            keep(bad)
    with pytest.raises(ValueError):
        fplx.PostKeepLargestComponent({"keeplargestcomponent_mode": 3})
    with pytest.raises(ValueError):
        fplx.ops.keep_largest_component(torch.zeros((3, 4), dtype=torch.uint8), mode=0)


def test_abi_rejects_bad_shapes_and_workspaces_before_any_launch():
    from fplx import _lib
    lib = _lib.lib()
    seg = (ctypes.c_uint8 * 64)()
    lab = (ctypes.c_int * 64)()
    ws = (ctypes.c_int * 448)()
    head = 320 * 4
    assert lib.fplx_cc_label(None, 4, 4, 4, 0, lab, ws, head, None) == -5
    assert lib.fplx_cc_label(seg, 4, 4, 4, 0, None, ws, head, None) == -5
    assert lib.fplx_cc_label(seg, 4, 4, 4, 0, lab, None, head, None) == -5 and "workspace" in _lib.last_error()
    assert lib.fplx_cc_label(seg, 4, 4, 4, 0, lab, ws, head - 4, None) == -3
    for d, h, w in ((0, 4, 4), (4, -1, 4), (4, 4, 0), (1 << 11, 1 << 10, 1 << 10)):
        assert lib.fplx_cc_label(seg, d, h, w, 0, lab, ws, head, None) == -1
        assert lib.fplx_keep_largest_component(seg, d, h, w, 1, seg, ws, 1 << 40, None) == -1
    need = (320 + 2 * 64) * 4
    assert lib.fplx_keep_largest_component(seg, 4, 4, 4, 0, seg, ws, need - 1, None) == -3
    assert "keep_largest_component" in _lib.last_error()
    assert lib.fplx_keep_largest_component(seg, 4, 4, 4, 0, None, ws, need, None) == -5
    with pytest.raises(ValueError):
        _lib.check(lib.fplx_keep_largest_component(seg, 0, 4, 4, 0, seg, ws, need, None))
