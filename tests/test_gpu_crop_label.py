"""-m gpu tests of the crop, bounding-box and label kernels (csrc/crop_label.hip through fplx.ops) and of CenterCrop,
CropWithBoundingBox, RandomResizedCrop, LabelConvert, LabelConvertNonzero, PartialLabelToProbability, ReduceLabelDim,
GrayscaleToRGB and RandomCrop's inverse (fplx.transform) against the numpy restatement tests/crop_label_ref.py and the
reference-generated fixture tests/golden/crop_label.npz.

Criterion: equality.  Every result is an integer, a copy or a scipy-exact interpolation: arrays have the fixture's shape
and dtype, NaNs in the same places and every other element bit for bit; `<Name>_Param` strings are the reference's."""
import json
import os
import random

import numpy as np
import pytest
import torch

import crop_label_ref as CL
import detdata

pytestmark = pytest.mark.gpu

BIG = (1, 33, 65, 67)                                    # 143715 voxels: many blocks, a ragged tail of 3


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _np(t):
    return t.cpu().numpy()


def _unaligned(a):
    """the same values at an address that is no multiple of 16 bytes (the kernels' element-by-element forms)"""
    src = _dev(a)
    flat = torch.empty(a.size + 1, dtype=src.dtype, device="cuda:0")
    view = flat[1:].view(a.shape)
    view.copy_(src)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    return view


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "crop_label.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def inp():
    return CL.inputs()


# ---- every fixture case through the real classes on device tensors

@pytest.mark.parametrize("case", sorted(CL.CASES))
def test_transforms_equal_reference(case, fx, inp):
    from fplx import transform as T
    s = CL.check_case(fx, case, T.TransformDict, inp, to_sample=_dev, to_numpy=_np)
    for k in CL.SAMPLE_KEYS:
        assert k not in s or s[k].is_cuda


def test_registry_and_config_built_lists(fx):
    from fplx import transform as T
    assert sorted(T.TransformDict) == json.loads(str(fx["names_json"]))
    p = dict(task="segmentation", centercrop_output_size=[4, 8, 9], cropwithboundingbox_start=None,
             cropwithboundingbox_output_size=None, randomresizedcrop_output_size=[8, 8], randomresizedcrop_scale=[0.5, 1.0],
             randomresizedcrop_ratio=[0.9, 1.1], labelconvert_source_list=[4], labelconvert_target_list=[3],
             partiallabeltoprobability_class_num=4)
    assert [type(t).__name__ for t in T.build_transforms(list(CL.NEW_NAMES), p)] == list(CL.NEW_NAMES)


# ---- the kernels against the restatement

def _bbox_volume(hits, shape=BIG):
    x = np.zeros(int(np.prod(shape)), np.float32)
    for k, i in enumerate(hits):
        x[i] = (-1.0) ** k * (k + 1.5)
    return x.reshape(shape)


def test_nonzero_bbox_on_fixture_images_and_edge_volumes(inp):
    from fplx import ops
    from fplx import transform as T
    for name in ("image_a", "image_b", "image_c"):
        want = CL.nonzero_bbox(inp[name])
        assert ops.nonzero_bbox(_dev(inp[name])) == want, name
        assert ops.nonzero_bbox(_unaligned(inp[name])) == want, name
    assert ops.nonzero_bbox(_dev(inp["image_a"]))[1:] == ([0, 2, 5, 4], [2, 9, 20, 23])      # the NaN counts, the -0.0 does not
    # nothing set: count 0, and the class refuses
    zero = torch.zeros((2, 5, 6, 7), device="cuda:0")
    assert ops.nonzero_bbox(zero) == (0, [CL.INT_MAX] * 4, [0] * 4) == CL.nonzero_bbox(_np(zero))
    cwb = T.CropWithBoundingBox(dict(task="segmentation", cropwithboundingbox_start=None, cropwithboundingbox_output_size=None))
    for z in (zero, -zero):
        with pytest.raises(ValueError, match="all-zero"):
            cwb({"image": z})
    for v, want in ((0.0, 0), (-0.0, 0), (2.0, 1), (float("nan"), 1), (1e-45, 1)):          # 1e-45: a denormal is not zero
        one = np.full((1, 1, 1, 1), v, np.float32)
        got = ops.nonzero_bbox(_dev(one))
        assert got == CL.nonzero_bbox(one) and got[0] == want, v


def test_nonzero_bbox_over_many_blocks_with_a_ragged_tail():
    from fplx import ops
    n = int(np.prod(BIG))
    assert n % 4 == 3 and n > 100 * 1024
    cases = [[0], [n - 1], [n - 4], [n - 3], [0, n - 1], [1023, 1024], [255, 256, 257], [1024 * 70 - 1, 1024 * 70],
             [3, 4, 67, 67 * 65 - 1, 67 * 65, 4 * 2048 * 256 % n, n - 2], list(range(0, n, 9973))]
    for hits in cases:
        x = _bbox_volume(hits)
        want = CL.nonzero_bbox(x)
        assert want[0] == len(set(hits))
        assert ops.nonzero_bbox(_dev(x)) == want, hits
        assert ops.nonzero_bbox(_unaligned(x)) == want, hits
    dense = detdata.normal("cl.bbox.dense", (3, 7, 11, 13))
    dense[:, :2] = 0
    dense[:, :, :, 11:] = 0
    assert ops.nonzero_bbox(_dev(dense)) == CL.nonzero_bbox(dense) == (3 * 5 * 11 * 11, [0, 2, 0, 0], [3, 7, 11, 11])


SIZES = (1, 255, 256, 257, 33 * 65 * 67, 33 * 65 * 68)


def _labels(n, top):
    """0 .. top in a fixed shuffle; for n >= top + 1 every value occurs"""
    lab = (np.arange(n, dtype=np.int64) * 7919 % (top + 1)).astype(np.uint8)
    return lab


@pytest.mark.parametrize("n", SIZES)
def test_label_lut(n):
    from fplx import ops
    lab = _labels(n, 255)
    if n >= 256:
        assert np.unique(lab).size == 256
    lut = [int(v) for v in (np.arange(256) * 37 + 11) % 256]
    assert sorted(lut) == list(range(256))
    want = CL.label_lut(lab, lut)
    assert np.array_equal(_np(ops.label_lut(_dev(lab), lut)), want)
    assert np.array_equal(_np(ops.label_lut(_unaligned(lab), lut)), want)
    inplace = _dev(lab)
    assert ops.label_lut(inplace, lut, out=inplace) is inplace and np.array_equal(_np(inplace), want)
    # the two tables the classes use
    dup = ops.label_lut_table([1, 2, 4, 4], [3, 1, 200, 100])
    assert dup == CL.lut_table([1, 2, 4, 4], [3, 1, 200, 100]) and dup[4] == 44
    for table in (dup, [0] + [1] * 255):
        assert np.array_equal(_np(ops.label_lut(_dev(lab), table)), CL.label_lut(lab, table))


@pytest.mark.parametrize("n", SIZES)
def test_partial_label_to_probability(n):
    from fplx import ops
    lab = _labels(n, 3)
    lab[-1] = 4                                          # the largest label is the very last voxel
    for arr in (lab, np.where(lab == 4, 200, lab).astype(np.uint8)):
        want = CL.partial_label(arr, 4)
        for dev in (_dev(arr), _unaligned(arr)):
            prob, weight, top = ops.partial_label_to_probability(dev, 4)
            assert prob.dtype == weight.dtype == torch.float32 and tuple(prob.shape) == (4, n) and tuple(weight.shape) == (n,)
            assert np.array_equal(_np(prob), want[0]) and np.array_equal(_np(weight), want[1]) and top == want[2]
    assert want[2] == 200 and CL.partial_label(lab, 4)[2] == 4 and CL.partial_label(lab, 4)[1][-1] == 0
    z = np.zeros(n, np.uint8)
    prob, weight, top = ops.partial_label_to_probability(_dev(z), 1)
    assert top == 0 and float(prob.min()) == 1.0 and float(weight.min()) == 1.0


def test_partial_label_class_asserts_like_the_reference(inp):
    from fplx import transform as T
    s = {"image": _dev(inp["image_a"]), "label": _dev(inp["label"])}
    with pytest.raises(AssertionError):
        T.PartialLabelToProbability(dict(task="segmentation", partiallabeltoprobability_class_num=3))(s)


@pytest.mark.parametrize("dtype", (np.float32, np.uint8))
def test_paste_roi(dtype):
    from fplx import ops
    out = (7, 11, 13)
    boxes = [((0, 2, 3), (3, 4, 5)), ((4, 2, 3), (3, 4, 5)), ((1, 0, 3), (3, 4, 5)), ((1, 7, 3), (3, 4, 5)), ((1, 2, 0), (3, 4, 5)),
             ((1, 2, 8), (3, 4, 5)), ((0, 0, 0), out), ((6, 10, 12), (1, 1, 1)), ((2, 3, 4), (1, 5, 1))]
    for lo, size in boxes:
        sub = (np.abs(detdata.normal("cl.paste%s%s" % (lo, size), (3,) + tuple(size))) * 50 % 256).astype(dtype)
        if dtype == np.float32:
            sub.flat[0] = np.nan
            sub.flat[-1] = -0.0
        want = np.zeros((3,) + out, dtype)
        want[:, lo[0]:lo[0] + size[0], lo[1]:lo[1] + size[1], lo[2]:lo[2] + size[2]] = sub
        CL.assert_same(CL.paste_roi(sub, lo, out), want, (lo, size))
        got = ops.paste_roi(_dev(sub), lo, out)
        CL.assert_same(_np(got), want, (lo, size))
    big = (np.abs(detdata.normal("cl.paste.big", (2, 30, 60, 61))) * 50 % 256).astype(dtype)           # more than one block
    CL.assert_same(_np(ops.paste_roi(_dev(big), (3, 5, 6), BIG[1:])), CL.paste_roi(big, (3, 5, 6), BIG[1:]), "big")
    with pytest.raises(ValueError, match="outside the output"):
        ops.paste_roi(_dev(big), (4, 5, 6), BIG[1:])


def test_refusals_on_device_tensors(inp):
    from fplx import transform as T
    seg = {"task": "segmentation"}
    vol = lambda: {"image": _dev(inp["image_a"]), "label": _dev(inp["label"])}
    with pytest.raises(ValueError, match="exceeds the volume"):
        T.CenterCrop(dict(seg, centercrop_output_size=[None, 8, 24]))(vol())
    with pytest.raises(ValueError, match="output_size"):
        T.CropWithBoundingBox(dict(seg, cropwithboundingbox_start=[0, 0, 0], cropwithboundingbox_output_size=None))
    with pytest.raises(ValueError):                      # a start beyond the volume leaves nothing to gather
        T.CropWithBoundingBox(dict(seg, cropwithboundingbox_start=[9, 0, 0], cropwithboundingbox_output_size=[2, 2, 2]))(vol())
    with pytest.raises(AssertionError):                  # RandomResizedCrop takes 2-D samples only
        T.RandomResizedCrop(dict(seg, **CL.CASES["rrc_seed1"]["params"]))(vol())
    with pytest.raises(ValueError, match="0..255"):
        T.LabelConvert(dict(seg, labelconvert_source_list=[1, 256], labelconvert_target_list=[1, 2]))
    with pytest.raises(AssertionError):
        T.GrayscaleToRGB(seg)(vol())
    with pytest.raises(ValueError, match="device tensor"):
        T.LabelConvertNonzero(seg)({"label": torch.zeros((1, 2, 2, 2), dtype=torch.uint8)})
    with pytest.raises(ValueError, match="device tensor"):
        T.CenterCrop(dict(seg, centercrop_output_size=[1, 1, 1]))({"image": torch.zeros((1, 2, 2, 2))})


# ---- end to end: a test_transform list with a crop in it, through SegmentationAgent.infer()

class _FixedInferer(object):
    """stands in for the sliding-window inferer: two-class logits that are a pure function of the input's shape"""

    def run(self, model, image, domain_label=None):
        shp = (image.shape[0], 2) + tuple(image.shape[2:])
        return torch.from_numpy(detdata.normal("cl.e2e%s" % (shp,), shp)).to(image.device)


def _agent(tmp_path, tag, volume, dataset):
    import fplx
    from fplx import nifti
    root = tmp_path / tag
    (root / "img").mkdir(parents=True)
    nifti.write_nifti(str(root / "img" / "c0.nii.gz"), volume, (0.5, 0.6, 1.2), (3.0, -4.0, 5.0))
    (root / "test.csv").write_text("image\nimg/c0.nii.gz\n")
    net_cfg = dict(net_type="UNet2D5_dsbn", in_chns=1, feature_chns=[8, 16, 32, 32, 32], dropout=[0.0, 0.0, 0.2, 0.2, 0.2],
                   conv_dims=[3, 3, 3, 3, 3], class_num=2, bilinear=False, num_domains=2, precision="fp32")
    config = {
        "dataset": dict({"root_dir": str(root), "test_csv": str(root / "test.csv"), "tensor_type": "float",
                         "normalizewithmeanstd_channels": [0], "normalizewithmeanstd_mean": [0.0],
                         "normalizewithmeanstd_std": [40.0]}, **dataset),
        "network": net_cfg,
        "training": {"ckpt_save_dir": "model/vs_t1s_g", "random_seed": 1},
        "testing": {"gpus": [0], "domian_label": 1, "evaluation_mode": True, "output_dir": str(root / "out")},
    }
    torch.manual_seed(0)
    agent = fplx.SegmentationAgent(config, "test")
    agent.create_dataset()
    agent.create_network()
    agent.set_inferer(_FixedInferer())
    return agent, root


def _written(root):
    from fplx import nifti
    return nifti.load_nifty_volume_as_4d_array(str(root / "out" / "vs_t1s_g_test" / "c0.nii.gz"))["data_array"][0]


def _expected_mask(shape, box_lo, box_size, net_shape, net_lo):
    """argmax of the fixed logits on the network's input extent, the block [net_lo, net_lo + box_size) of it pasted at
    box_lo into zeros of the input's shape"""
    shp = (1, 2) + tuple(net_shape)
    logits = detdata.normal("cl.e2e%s" % (shp,), shp)[0]
    sl = tuple(slice(a, a + s) for a, s in zip(net_lo, box_size))
    want = np.zeros(shape, np.uint8)
    want[tuple(slice(a, a + s) for a, s in zip(box_lo, box_size))] = np.argmax(logits[(slice(None),) + sl], axis=0)
    return want


def test_agent_infers_through_a_bounding_box_crop(tmp_path, inp):
    shape = CL.VOL
    volume = np.zeros(shape, np.float64)
    volume[2:7, 5:16, 4:19] = inp["image_a"][0, 2:7, 5:16, 4:19]                       # zero outside the inner block
    agent, root = _agent(tmp_path, "cwb", volume, {
        "test_transform": ["NormalizeWithMeanStd", "CropWithBoundingBox", "Pad"], "cropwithboundingbox_start": None,
        "cropwithboundingbox_output_size": None, "pad_output_size": [16, 32, 48]})
    out = agent.infer()
    mask = out["img/c0.nii.gz"].cpu().numpy()
    # Pad centres the 5 x 11 x 15 crop in 16 x 32 x 48: lower margins int(11 / 2), int(21 / 2), int(33 / 2)
    want = _expected_mask(shape, (2, 5, 4), (5, 11, 15), (16, 32, 48), (5, 10, 16))
    assert mask.shape == shape and mask.dtype == np.uint8
    assert np.array_equal(mask, want) and 0 < want.sum() < want[2:7, 5:16, 4:19].size
    outside = np.ones(shape, bool)
    outside[2:7, 5:16, 4:19] = False
    assert not mask[outside].any()
    assert np.array_equal(_written(root), want)


def test_agent_infers_through_random_crop(tmp_path, inp):
    """RandomCrop in a test_transform list: its inverse (CenterCrop's, as in the reference) pastes the prediction back"""
    shape, size = CL.VOL, (8, 16, 16)
    agent, root = _agent(tmp_path, "rc", inp["volume1"][0].astype(np.float64), {
        "test_transform": ["NormalizeWithMeanStd", "RandomCrop"], "randomcrop_output_size": list(size)})
    random.seed(11)
    lo = [random.randint(0, n - s) for n, s in zip(shape, size)]
    random.seed(11)
    mask = agent.infer()["img/c0.nii.gz"].cpu().numpy()
    want = _expected_mask(shape, lo, size, size, (0, 0, 0))
    assert mask.shape == shape and np.array_equal(mask, want) and want.any()
    assert np.array_equal(_written(root), want)
