"""-m gpu tests of the resampling kernel (csrc/resample.hip through fplx.ops.resample_affine) and of RandomRotate / Rescale /
RandomRescale (fplx.transform) against scipy.ndimage itself and against the reference-generated fixtures
tests/golden/resample*.npz.

Criteria.  Labels (uint8, order 0) and fp32 volumes at order 0: bit-exact, 0 differing elements - a condition.  fp32 at
order 1: bit-exact is the design target (the kernel restates scipy's fp64 arithmetic operation for operation, see
tests/resample_ref.py); asserted is that every element lies within 1 fp32 ulp of scipy's and that at most 1e-4 of the elements
are not identical, and every comparison prints its count."""
import json
import os
import random

import numpy as np
import pytest
import torch

import detdata
import resample_ref as R
from test_resample_cpu import (GENERIC_ANGLES, PLANES, SPECIAL_ANGLES, assert_close_to_scipy, scipy_rotate, scipy_rotation,
                               scipy_zoom, volumes)

pytestmark = pytest.mark.gpu

# extents of 1 along every axis, odd sizes, C = 1 and 3
SHAPES = [((12, 40, 50), 1), ((9, 33, 31), 3), ((1, 37, 29), 1), ((7, 1, 23), 3), ((11, 19, 1), 1), ((5, 5, 5), 3),
          ((16, 32, 48), 1), ((3, 64, 17), 3), ((13, 27, 45), 1), ((2, 3, 2), 1)]
ZOOMS = [(4.0 / 3, 1.2, 0.96), (0.83, 1.21, 0.9), (2.0, 2.0, 2.0), (0.5, 0.5, 0.5), (1.0, 0.7, 1.6), (1.37, 1.41, 1.96)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _resample(x, m, t, out, order):
    from fplx import ops
    y = ops.resample_affine(_dev(x), m, t, out, order)
    assert y.dtype == _dev(x).dtype and tuple(y.shape) == (x.shape[0],) + tuple(out) and y.is_cuda
    return y.cpu().numpy()


def _compare(x_img, x_lab, m, t, out, refs, what):
    """refs: scipy's (label order 0, image order 0, image order 1)"""
    got = _resample(x_lab, m, t, out, 0)
    assert got.dtype == np.uint8 and int((got != refs[0]).sum()) == 0, (what, "label")
    got = _resample(x_img, m, t, out, 0)
    assert int((got != refs[1]).sum()) == 0, (what, "image order 0")
    assert_close_to_scipy(_resample(x_img, m, t, out, 1), refs[2], (what, "image order 1"))


@pytest.mark.parametrize("shape,channels", SHAPES)
def test_kernel_equals_scipy_zoom(shape, channels):
    img, lab = volumes(shape, channels, "rs.gpu.zoom")
    for zoom in ZOOMS:
        out = R.zoom_size(shape, zoom)
        if min(out) < 1:
            continue                                  # scipy refuses an empty output
        m, t = R.zoom_affine(shape, out)
        refs = [scipy_zoom(lab, zoom, 0), scipy_zoom(img, zoom, 0), scipy_zoom(img, zoom, 1)]
        _compare(img, lab, m, t, out, refs, ("zoom", shape, channels, zoom))


@pytest.mark.parametrize("shape,channels", SHAPES)
def test_kernel_equals_scipy_rotate(shape, channels):
    """the matrix and the offset are scipy's own (cosdg / sindg, its matrix-vector product): the kernel is judged on the
    numbers scipy used; the product's trig is judged against the fixtures below"""
    img, lab = volumes(shape, channels, "rs.gpu.rot")
    for angle in GENERIC_ANGLES + SPECIAL_ANGLES:
        for axes in PLANES:
            m, t = scipy_rotation(shape, angle, axes)
            refs = [scipy_rotate(lab, angle, axes, 0), scipy_rotate(img, angle, axes, 0), scipy_rotate(img, angle, axes, 1)]
            _compare(img, lab, m, t, shape, refs, ("rotate", shape, channels, angle, axes))


def test_kernel_equals_restatement_on_a_general_matrix():
    """shear + anisotropic scale + offset: no scipy wrapper builds it, the restatement (held to scipy on the CPU) does"""
    shape = (9, 21, 26)
    img, lab = volumes(shape, 2, "rs.gpu.affine")
    m = np.array([[0.93, 0.11, -0.07], [-0.21, 1.08, 0.13], [0.05, -0.17, 0.89]])
    t = np.array([0.6, 2.3, 1.9])
    out = (11, 19, 30)
    assert int((_resample(lab, m, t, out, 0) != R.resample_affine(lab, m, t, out, 0)).sum()) == 0
    assert int((_resample(img, m, t, out, 0) != R.resample_affine(img, m, t, out, 0)).sum()) == 0
    assert_close_to_scipy(_resample(img, m, t, out, 1), R.resample_affine(img, m, t, out, 1), "general matrix")
    # a non-finite matrix reads nothing: every voxel counts as outside
    bad = m.copy()
    bad[1, 1] = np.nan
    assert not _resample(img, bad, t, out, 1).any() and not _resample(lab, bad, t, out, 0).any()


# ---- the transforms against the reference's fixtures

def _fx(golden_dir, name="resample.npz"):
    return np.load(os.path.join(golden_dir, name), allow_pickle=False)


def _sample(g):
    return {k: _dev(g[k]) for k in ("image", "label", "pixel_weight")}


def _params(g, variant=None):
    p = json.loads(str(g["params_json"]))
    if variant:
        p.update(json.loads(str(g["variants_json"]))[variant])
    return p


def _seed(seed):
    random.seed(seed)
    np.random.seed(seed)


def _check(g, key, s, param_keys):
    for k in param_keys:
        assert json.loads(s[k]) == json.loads(str(g[key + k])), (key, k)
    assert random.random() == float(g[key + "next_random"]) and np.random.uniform() == float(g[key + "next_np_random"]), key
    assert s["image"].dtype == torch.float32 and s["label"].dtype == torch.uint8 and s["pixel_weight"].dtype == torch.float32
    for k in ("image", "label", "pixel_weight"):
        assert s[k].is_cuda and tuple(s[k].shape) == g[key + k].shape, (key, k)
    assert int((s["label"].cpu().numpy() != g[key + "label"]).sum()) == 0, key
    for k in ("image", "pixel_weight"):
        assert_close_to_scipy(s[k].cpu().numpy(), g[key + k], (key, k))


def test_each_transform_matches_reference_fixture(golden_dir):
    from fplx import transform as T
    g = _fx(golden_dir)
    seeds = [int(v) for v in g["seeds"]]
    assert len(seeds) >= 5
    for seed in seeds:
        _seed(seed)
        s = T.TransformDict["RandomRotate"](_params(g))(_sample(g))
        _check(g, "seed%d_rotate_" % seed, s, ["RandomRotate_Param"])
        _seed(seed)
        s = T.TransformDict["RandomRescale"](_params(g))(_sample(g))
        _check(g, "seed%d_randomrescale_" % seed, s, ["RandomRescale_origin_shape"])
    _seed(seeds[0])
    _check(g, "rotate_d_", T.RandomRotate(_params(g, "rotate_d"))(_sample(g)), ["RandomRotate_Param"])
    _seed(seeds[0])
    _check(g, "randomrescale_scalar_", T.RandomRescale(_params(g, "randomrescale_scalar"))(_sample(g)),
           ["RandomRescale_origin_shape"])
    for key, variant in (("rescale_list_", None), ("rescale_none_", "rescale_none"), ("rescale_int_", "rescale_int")):
        _seed(seeds[0])
        _check(g, key, T.TransformDict["Rescale"](_params(g, variant))(_sample(g)), ["Rescale_origin_shape"])


def test_chain_matches_reference_fixture(golden_dir):
    from fplx import transform as T
    g, gc = _fx(golden_dir), _fx(golden_dir, "resample_chain.npz")
    names = ["RandomRotate", "RandomRescale", "Pad", "RandomCrop"]
    for seed in [int(v) for v in g["seeds"]]:
        _seed(seed)
        s = T.apply_transforms(T.build_transforms(names, _params(g)), _sample(g))
        _check(gc, "seed%d_chain_" % seed, s,
               ["RandomRotate_Param", "RandomRescale_origin_shape", "Pad_Param", "RandomCrop_Param"])


def test_inverses_match_reference_fixture(golden_dir):
    from fplx import transform as T
    g, gi = _fx(golden_dir), _fx(golden_dir, "resample_inverse.npz")
    for seed in [int(v) for v in g["seeds"]]:
        k = "seed%d_" % seed
        s = {"RandomRotate_Param": str(g[k + "rotate_RandomRotate_Param"]), "predict": _dev(gi["predict"])}
        s = T.RandomRotate(_params(g)).inverse_transform_for_prediction(s)
        assert s["predict"].is_cuda and s["predict"].dtype == torch.float32
        assert_close_to_scipy(s["predict"].cpu().numpy(), gi[k + "rotate_inverse"], k + "rotate_inverse")
        pred = R.prediction("rs.predict.%d" % seed, g[k + "randomrescale_image"].shape[1:])
        s = {"RandomRescale_origin_shape": [str(g[k + "randomrescale_RandomRescale_origin_shape"])], "predict": _dev(pred)}
        s = T.RandomRescale(_params(g)).inverse_transform_for_prediction(s)
        assert_close_to_scipy(s["predict"].cpu().numpy(), gi[k + "randomrescale_inverse"], k + "randomrescale_inverse")
    pred = R.prediction("rs.predict.rescale", g["rescale_list_image"].shape[1:])
    s = {"Rescale_origin_shape": str(g["rescale_list_Rescale_origin_shape"]), "predict": _dev(pred)}
    s = T.Rescale(_params(g)).inverse_transform_for_prediction(s)
    assert_close_to_scipy(s["predict"].cpu().numpy(), gi["rescale_inverse"], "rescale_inverse")


class _FixedInferer(object):
    """stands in for the sliding-window inferer: two-class logits, a pure function of the input's shape"""

    def run(self, model, image, domain_label=None):
        shp = (image.shape[0], 2) + tuple(image.shape[2:])
        return torch.from_numpy(detdata.normal("rs.e2e%s" % (shp,), shp)).to(image.device)


def test_agent_undoes_rescale_on_the_prediction(tmp_path):
    """SegmentationAgent's inverse walk with a test_transform that contains Rescale: the masks have the volumes' own shapes
    and equal the argmax of scipy's zoom of the same logits"""
    import fplx
    from fplx import nifti
    rs = np.random.RandomState(5)
    root = tmp_path / "data"
    (root / "img").mkdir(parents=True)
    shapes = [(11, 30, 37), (9, 33, 40)]
    for i, shp in enumerate(shapes):
        nifti.write_nifti(str(root / "img" / ("c%d.nii.gz" % i)), rs.randn(*shp) * 40 + 150, (0.5, 0.6, 1.2), (3.0, -4.0, 5.0))
    (tmp_path / "test.csv").write_text("image\nimg/c0.nii.gz\nimg/c1.nii.gz\n")
    size = [16, 32, 48]
    config = {
        "dataset": {"root_dir": str(root), "test_csv": str(tmp_path / "test.csv"), "tensor_type": "float",
                    "test_transform": ["NormalizeWithMeanStd", "Rescale"], "normalizewithmeanstd_channels": [0],
                    "rescale_output_size": list(size), "rescale_inverse": True},
        "network": dict(net_type="UNet2D5_dsbn", in_chns=1, feature_chns=[8, 16, 32, 32, 32],
                        dropout=[0.0, 0.0, 0.2, 0.2, 0.2], conv_dims=[3, 3, 3, 3, 3], class_num=2, bilinear=False,
                        num_domains=2, precision="fp32"),
        "training": {"ckpt_save_dir": "model/vs_t1s_g", "random_seed": 1},
        "testing": {"gpus": [0], "domian_label": 1, "evaluation_mode": True},
    }
    torch.manual_seed(0)
    agent = fplx.SegmentationAgent(config, "test")
    agent.create_dataset()
    agent.create_network()
    agent.set_inferer(_FixedInferer())
    assert any(isinstance(t, fplx.transform.Rescale) for t in agent.transform_list)
    out = agent.infer()
    from scipy import ndimage
    for i, shp in enumerate(shapes):
        mask = out["img/c%d.nii.gz" % i].cpu().numpy()
        logits = detdata.normal("rs.e2e%s" % ((1, 2) + tuple(size),), (1, 2) + tuple(size))
        back = ndimage.zoom(logits, [1.0, 1.0] + [float(a) / b for a, b in zip(shp, size)], order=1)
        assert back.shape[2:] == shp
        assert mask.reshape(shp).shape == shp and np.array_equal(mask.reshape(shp), back[0].argmax(0).astype(np.uint8))


# ---- independence of the launch shape

def test_inference_size_and_channel_independence():
    shape = (48, 160, 272)
    img, lab = volumes(shape, 1, "rs.gpu.big")
    m, t = scipy_rotation(shape, 17.0, (-1, -2))
    refs = [scipy_rotate(lab, 17.0, (-1, -2), 0), scipy_rotate(img, 17.0, (-1, -2), 0), scipy_rotate(img, 17.0, (-1, -2), 1)]
    _compare(img, lab, m, t, shape, refs, "rotate 17 at 1x48x160x272")
    zoom = (1.2, 1.2, 1.2)
    out = R.zoom_size(shape, zoom)
    mz, tz = R.zoom_affine(shape, out)
    _compare(img, lab, mz, tz, out, [scipy_zoom(lab, zoom, 0), scipy_zoom(img, zoom, 0), scipy_zoom(img, zoom, 1)],
             "zoom 1.2 at 1x48x160x272")
    # one launch with C = 4 equals four launches with C = 1
    shape = (10, 37, 41)
    img, lab = volumes(shape, 4, "rs.gpu.c4")
    m, t = scipy_rotation(shape, -23.7, (-2, -3))
    for x, order in ((img, 1), (img, 0), (lab, 0)):
        whole = _resample(x, m, t, shape, order)
        for c in range(4):
            assert np.array_equal(whole[c:c + 1], _resample(x[c:c + 1], m, t, shape, order)), (order, c)


def test_refusals():
    from fplx import ops
    from fplx import transform as T
    p = {"task": "segmentation", "randomrotate_angle_range_d": [-10, 10], "randomrotate_angle_range_h": None,
         "randomrotate_angle_range_w": None, "rescale_output_size": [8, 8, 8], "randomrescale_lower_bound": 0.9,
         "randomrescale_upper_bound": 1.1}
    for name in ("RandomRotate", "Rescale", "RandomRescale"):
        t = T.TransformDict[name](dict(p))
        with pytest.raises(ValueError, match=r"must be a \[C,D,H,W\] device tensor"):
            t({"image": torch.zeros((1, 8, 8), device="cuda:0")})                       # a [C,H,W] sample
        with pytest.raises(ValueError, match=r"must be a \[C,D,H,W\] device tensor"):
            t({"image": torch.zeros((1, 4, 8, 8))})                                     # a host tensor
    eye = np.eye(3)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ops.resample_affine(torch.zeros((1, 4, 4, 4)), eye, (0, 0, 0), (4, 4, 4), 1)
    lab = torch.zeros((1, 4, 4, 4), dtype=torch.uint8, device="cuda:0")
    with pytest.raises(ValueError, match="uint8"):
        ops.resample_affine(lab, eye, (0, 0, 0), (4, 4, 4), 1)
    with pytest.raises(ValueError):
        ops.resample_affine(lab.to(torch.int32), eye, (0, 0, 0), (4, 4, 4), 0)
    with pytest.raises(ValueError):
        ops.resample_affine(lab, eye, (0, 0, 0), (4, 4, 4), 2)
    with pytest.raises(ValueError):
        ops.resample_affine(lab, eye, (0, 0, 0), (4, 0, 4), 0)
    with pytest.raises(ValueError, match="float32"):
        T.Rescale(dict(p))({"image": lab})
