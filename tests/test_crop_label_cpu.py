"""CPU tests of the crop, bounding-box and label feature (csrc/crop_label.hip; fplx.transform.CenterCrop,
CropWithBoundingBox, RandomResizedCrop, LabelConvert, LabelConvertNonzero, PartialLabelToProbability, ReduceLabelDim,
GrayscaleToRGB and RandomCrop's inverse):
 - tests/crop_label_ref.py, the numpy restatement, against what the reference's classes left in tests/golden/crop_label.npz:
   arrays (shape, dtype, NaN positions, every other element bit for bit), `<Name>_Param` strings, the position of Python's
   generator after the draws, inverse results;
 - the host classes with fplx.ops replaced by the restatement's kernels: the same fixture, the same criterion - this checks
   the draw order, the json, the truncation and the refusals without a GPU;
 - the registry holds exactly the reference's 23 names;
 - the ABI's argument checks, which run before any launch."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import crop_label_ref as CL
import resample_ref as R


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "crop_label.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def inp():
    return CL.inputs()


def test_fixture_holds_the_named_inputs_and_cases(fx, inp):
    for k, v in inp.items():
        CL.assert_same(v, fx[k], k)
    assert json.loads(str(fx["cases_json"])) == json.loads(json.dumps(CL.CASES))
    a = inp["image_a"]
    assert np.isnan(a[-1, -1, -1, -1]) and np.signbit(a[0, 0, 0, 3]) and a[0, 0, 0, 3] == 0
    assert CL.nonzero_bbox(a)[1:] == ([0, 2, 5, 4], [2, 9, 20, 23])
    assert CL.nonzero_bbox(inp["image_b"]) == (1, [0, 0, 0, 0], [1, 1, 1, 1])
    assert CL.nonzero_bbox(inp["image_c"]) == (1, [1, 8, 19, 22], [2, 9, 20, 23])
    assert sorted(np.unique(inp["label"]).tolist()) == [0, 1, 2, 3, 4]
    # the cases the feature was specified with
    assert json.loads(str(fx["cwb_size_CropWithBoundingBox_Param"]))[2][3] == 30 and fx["cwb_size_image"].shape[3] == 23
    assert fx["cwb_far_image"].shape == (2, 2, 5, 3)                      # truncated on every axis
    assert CL.lut_table([1, 2, 4, 4], [3, 1, 200, 100])[4] == 44


@pytest.mark.parametrize("case", sorted(CL.CASES))
def test_restatement_equals_reference(case, fx, inp):
    CL.check_case(fx, case, CL.TRANSFORMS, inp)


# ---- the host classes on the restatement's kernels

@pytest.fixture
def host_transforms(monkeypatch):
    """fplx.transform with every kernel it reaches replaced by the numpy restatement and the device checks by type checks"""
    from fplx import transform as T
    tn = torch.from_numpy

    def crop_flip(x, crop_min, out_size, flip_mask=0, out=None):
        assert flip_mask == 0 and x.dim() == 4
        y = tn(CL.crop(x.numpy(), [int(v) for v in crop_min], [int(v) for v in out_size]))
        if out is None:
            return y
        out.copy_(y)
        return out

    def label_bbox(label, mask_labels):
        idx = np.nonzero(np.isin(label.numpy(), list(mask_labels)))
        if idx[0].size == 0:
            return 0, [CL.INT_MAX] * 4, [0] * 4
        return int(idx[0].size), [int(i.min()) for i in idx], [int(i.max()) + 1 for i in idx]

    def partial(label, class_num):
        prob, weight, top = CL.partial_label(label.numpy(), class_num)
        return tn(prob), tn(weight), top

    fakes = {
        "crop_flip": crop_flip, "label_bbox": label_bbox, "partial_label_to_probability": partial,
        "nonzero_bbox": lambda x: CL.nonzero_bbox(x.numpy()),
        "label_lut": lambda label, lut, out=None: tn(CL.label_lut(label.numpy(), lut)),
        "paste_roi": lambda sub, lower, out_size: tn(CL.paste_roi(sub.numpy(), [int(v) for v in lower], out_size)),
        "label_to_probability": lambda label, class_num: tn(CL.partial_label(label.numpy(), class_num)[0]),
        "resample_affine": lambda x, m, t, out_size, order: tn(R.resample_affine(x.numpy(), m, t, [int(v) for v in out_size], order)),
    }
    for name, fn in fakes.items():
        monkeypatch.setattr(T.ops, name, fn)

    def check_volume(t, name):
        if not (torch.is_tensor(t) and t.dim() == 4):
            raise ValueError("fplx.transform: sample['{0:}'] must be a [C,D,H,W] device tensor".format(name))
        return t.contiguous()

    def check_tensor(t, name):
        if not torch.is_tensor(t):
            raise ValueError("fplx.transform: sample['{0:}'] must be a device tensor".format(name))
        return t.contiguous()

    monkeypatch.setattr(T, "_check_volume", check_volume)
    monkeypatch.setattr(T, "_check_tensor", check_tensor)
    return T


def _t(a):
    return torch.from_numpy(np.array(a))


@pytest.mark.parametrize("case", sorted(CL.CASES))
def test_host_classes_equal_reference(case, fx, inp, host_transforms):
    s = CL.check_case(fx, case, host_transforms.TransformDict, inp, to_sample=_t, to_numpy=lambda t: t.numpy())
    if case == "pl2p":
        assert s["pixel_weight"].shape == s["label"].shape               # the sample's own pixel weight was replaced
        assert not np.array_equal(s["pixel_weight"].numpy(), inp["pixel_weight"])


def test_registry_holds_the_reference_names(fx):
    from fplx import transform as T
    names = json.loads(str(fx["names_json"]))
    assert len(names) == 23 and set(CL.NEW_NAMES) <= set(names)
    assert sorted(T.TransformDict) == names
    for name in names:
        assert T.TransformDict[name].__name__ == name
    # the family tree of the reference's crop.py: the inverse is CenterCrop's
    for name in ("CropWithBoundingBox", "RandomCrop", "RandomResizedCrop"):
        assert issubclass(T.TransformDict[name], T.CenterCrop)
    assert T.RandomCrop.inverse_transform_for_prediction is T.CenterCrop.inverse_transform_for_prediction
    assert T.CropWithBoundingBox.inverse_transform_for_prediction is T.CenterCrop.inverse_transform_for_prediction
    p = dict(task="segmentation", randomcrop_output_size=[4, 8, 9], centercrop_output_size=[4, 8, 9],
             cropwithboundingbox_start=None, cropwithboundingbox_output_size=None, randomresizedcrop_output_size=[8, 8],
             randomresizedcrop_scale=[0.5, 1.0], randomresizedcrop_ratio=[0.9, 1.1])
    assert [T.TransformDict[n](p).inverse for n in ("CenterCrop", "CropWithBoundingBox", "RandomCrop", "RandomResizedCrop")] == \
        [True, True, True, False]
    for n in ("LabelConvertNonzero", "PartialLabelToProbability", "ReduceLabelDim", "GrayscaleToRGB"):
        assert T.TransformDict[n](dict(p, partiallabeltoprobability_class_num=2)).inverse is False
    built = T.build_transforms(list(CL.NEW_NAMES), dict(p, labelconvert_source_list=[1], labelconvert_target_list=[2],
                                                       partiallabeltoprobability_class_num=2))
    assert [type(t).__name__ for t in built] == list(CL.NEW_NAMES)


def test_refusals_and_asserts(inp, host_transforms):
    T = host_transforms
    seg = {"task": "segmentation"}
    vol = lambda: {"image": _t(inp["image_a"]), "label": _t(inp["label"])}
    # CenterCrop: an output size beyond the volume (the reference slices from a negative start)
    with pytest.raises(ValueError, match="exceeds the volume"):
        T.CenterCrop(dict(seg, centercrop_output_size=[None, 8, 24]))(vol())
    with pytest.raises(ValueError, match="exceeds the volume"):
        CL.CenterCrop(dict(centercrop_output_size=[10, 8, 9]))({"image": inp["image_a"]})
    with pytest.raises(ValueError, match=r"must be a \[C,D,H,W\] device tensor"):
        T.CenterCrop(dict(seg, centercrop_output_size=[8, 9]))({"image": _t(inp["plane"])})
    # CropWithBoundingBox: a start without a size, at construction; an all-zero image
    with pytest.raises(ValueError, match="output_size"):
        T.CropWithBoundingBox(dict(seg, cropwithboundingbox_start=[0, 0, 0], cropwithboundingbox_output_size=None))
    cwb = T.CropWithBoundingBox(dict(seg, cropwithboundingbox_start=None, cropwithboundingbox_output_size=None))
    with pytest.raises(ValueError, match="all-zero"):
        cwb({"image": torch.zeros((2, 4, 5, 6))})
    with pytest.raises(ValueError, match="all-zero"):                     # -0.0 is zero
        cwb({"image": -torch.zeros((1, 4, 5, 6))})
    # a start beyond the volume leaves nothing to gather
    with pytest.raises(ValueError):
        T.CropWithBoundingBox(dict(seg, cropwithboundingbox_start=[9, 0, 0], cropwithboundingbox_output_size=[2, 2, 2]))(vol())
    # RandomResizedCrop: 2-D samples only, as the reference asserts; no inverse
    rrc = T.RandomResizedCrop(dict(seg, **CL.CASES["rrc_seed1"]["params"]))
    with pytest.raises(AssertionError):
        rrc(vol())
    with pytest.raises(AssertionError):
        T.RandomResizedCrop(dict(seg, randomresizedcrop_output_size=8, randomresizedcrop_scale=[0.5, 1], randomresizedcrop_ratio=[1, 1]))
    with pytest.raises(ValueError, match="not implemented"):
        rrc.inverse_transform_for_prediction({})
    # label conversion: labels outside uint8, lists of different length
    for src, tgt in (([1, 256], [1, 2]), ([1, 2], [1, 256]), ([-1], [1]), ([1], [-1]), ([1.5], [1])):
        with pytest.raises(ValueError, match="0..255"):
            T.LabelConvert(dict(seg, labelconvert_source_list=src, labelconvert_target_list=tgt))
    with pytest.raises(AssertionError):
        T.LabelConvert(dict(seg, labelconvert_source_list=[1, 2], labelconvert_target_list=[1]))
    with pytest.raises(ValueError, match="uint8"):
        T.LabelConvertNonzero(seg)({"label": torch.zeros((1, 2, 2, 2), dtype=torch.int32)})
    # PartialLabelToProbability: a label beyond class_num is the reference's AssertionError
    with pytest.raises(AssertionError):
        T.PartialLabelToProbability(dict(seg, partiallabeltoprobability_class_num=3))(vol())
    # GrayscaleToRGB: one or three channels
    with pytest.raises(AssertionError):
        T.GrayscaleToRGB(seg)(vol())
    with pytest.raises(ValueError, match=r"\[C,H,W\] or \[C,D,H,W\]"):
        T.GrayscaleToRGB(seg)({"image": torch.zeros((1, 4))})
    three = _t(inp["plane"])
    assert T.GrayscaleToRGB(seg)({"image": three})["image"] is three      # left as it is
    # another task: only the image is cropped
    s = T.CenterCrop({"task": "classification", "centercrop_output_size": [5, 8, 9]})(vol())
    assert tuple(s["image"].shape) == (2, 5, 8, 9) and tuple(s["label"].shape) == (1, 9, 20, 23)


def test_label_table_is_the_reference_arithmetic():
    from fplx import ops
    for src, tgt in (([1, 2, 4, 4], [3, 1, 200, 100]), ([0, 1, 2, 4], [0, 1, 2, 3]), ([7, 7, 7], [255, 255, 3]), ([], [])):
        assert ops.label_lut_table(src, tgt) == CL.lut_table(src, tgt)
        # convert_label itself, on all 256 values: products and sums in uint8
        lab = np.arange(256, dtype=np.uint8)
        want = np.zeros_like(lab)
        for s, t in zip(src, tgt):
            want = want + np.asarray(lab == s, np.uint8) * np.uint8(t)
        assert np.array_equal(np.asarray(CL.lut_table(src, tgt), np.uint8), want)
    assert ops.label_lut_table([4, 4], [200, 100])[4] == 44


def test_abi_rejects_bad_arguments_before_any_launch():
    from fplx import _lib
    lib = _lib.lib()
    f4, u1, i9 = (ctypes.c_float * 64)(), (ctypes.c_uint8 * 256)(), (ctypes.c_int * 9)()
    f = lib.fplx_nonzero_bbox
    assert f(None, 1, 4, 4, 4, i9, None) == -5 and f(f4, 1, 4, 4, 4, None, None) == -5 and "nonzero_bbox" in _lib.last_error()
    for shape in ((0, 4, 4, 4), (1, 4, -1, 4), (1, 4, 4, 0), (2, 1 << 10, 1 << 10, 1 << 10), (1 << 30, 1 << 30, 1 << 30, 1 << 30)):
        assert f(f4, *shape, i9, None) == -1, shape
    f = lib.fplx_label_lut
    assert f(None, u1, 16, u1, None) == -5 and f(u1, None, 16, u1, None) == -5 and f(u1, u1, 16, None, None) == -5
    assert f(u1, u1, 0, u1, None) == -1 and f(u1, u1, -3, u1, None) == -1 and "label_lut" in _lib.last_error()
    f = lib.fplx_partial_label_to_probability
    assert f(None, f4, f4, 2, 8, i9, None) == -5 and f(u1, None, f4, 2, 8, i9, None) == -5
    assert f(u1, f4, None, 2, 8, i9, None) == -5 and f(u1, f4, f4, 2, 8, None, None) == -5
    for class_num, voxels in ((0, 8), (256, 8), (-1, 8), (2, 0)):
        assert f(u1, f4, f4, class_num, voxels, i9, None) == -1, (class_num, voxels)
    f = lib.fplx_paste_roi
    ok = (4, 1, 2, 2, 2, 4, 4, 4, 1, 1, 1)
    assert f(None, f4, *ok, None) == -5 and f(f4, None, *ok, None) == -5
    for bad in ((4, 0, 2, 2, 2, 4, 4, 4, 1, 1, 1), (4, 1, 0, 2, 2, 4, 4, 4, 1, 1, 1), (4, 1, 2, 2, 2, 4, 4, 4, -1, 1, 1),
                (4, 1, 2, 2, 2, 4, 4, 4, 3, 1, 1), (4, 1, 2, 2, 5, 4, 4, 4, 0, 0, 0), (4, 1, 2, 2, 2, 4, 4, 4, 1, 1, 1 << 31 - 1),
                (4, 1, 2, 2, 2, 4, 4, 4, 1, (1 << 31) - 1, 1)):
        assert f(f4, f4, *bad, None) == -1, bad
    assert "paste_roi" in _lib.last_error()
    for elem_bytes in (0, 2, 8):
        assert f(f4, f4, elem_bytes, *ok[1:], None) == -2
    import fplx
    for call in (lambda: fplx.ops.nonzero_bbox(torch.zeros((1, 2, 2, 2))), lambda: fplx.ops.label_lut(torch.zeros(4, dtype=torch.uint8), [0] * 256),
                 lambda: fplx.ops.partial_label_to_probability(torch.zeros(4, dtype=torch.uint8), 2),
                 lambda: fplx.ops.paste_roi(torch.zeros((1, 2, 2, 2)), (0, 0, 0), (4, 4, 4))):
        with pytest.raises(RuntimeError, match="must live on the GPU"):       # no CPU fallback
            call()
