"""CPU tests of the resampling feature (csrc/resample.hip, fplx.transform.RandomRotate / Rescale / RandomRescale):
 - tests/resample_ref.py, the numpy restatement of the kernel's rules, against scipy.ndimage.zoom / rotate themselves:
   0 differing elements, labels and fp32 images, both orders (a condition, not a tolerance);
 - the host logic of the three transforms with ops.resample_affine replaced by the restatement: parameter strings, shapes,
   draw order and - the restatement being exact - the data of the reference's fixture tests/golden/resample.npz;
 - the ABI's argument checks, which run before any launch."""
import ctypes
import json
import os
import random

import numpy as np
import pytest
import torch

import detdata
import resample_ref as R

SHAPE = (12, 40, 50)
ZOOMS = [(4.0 / 3, 1.2, 0.96), (0.83, 1.21, 0.9), (2.0, 2.0, 2.0), (0.5, 0.5, 0.5), (1.0, 0.7, 1.6)]
GENERIC_ANGLES = [17.3, -8.1, 29.9]
SPECIAL_ANGLES = [0.0, 45.0, -45.0, 90.0, 135.0, 180.0, 270.0]
PLANES = [(-1, -2), (-1, -3), (-2, -3)]


def volumes(shape=SHAPE, channels=1, name="rs.cpu"):
    img = (detdata.normal(name + ".image", (channels,) + tuple(shape)) * 37.0 + 210.0).astype(np.float32)
    zz, yy, xx = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    c = [(n - 1) / 2.0 for n in shape]
    ell = sum(((g - ci) / max(0.35 * n, 0.6)) ** 2 for g, ci, n in zip((zz, yy, xx), c, shape)) < 1.0
    lab = np.stack([(ell * (1 + k)).astype(np.uint8) for k in range(channels)])
    return img, lab


def scipy_rotate(x, angle, axes, order):
    from scipy import ndimage
    return ndimage.rotate(x, angle, axes, reshape=False, order=order)


def scipy_zoom(x, zoom, order):
    from scipy import ndimage
    return ndimage.zoom(x, [1.0] + list(zoom), order=order)


def scipy_rotation(shape, angle, axes):
    """matrix and offset as scipy.ndimage.rotate builds them: cosdg / sindg and its own matrix-vector product"""
    from scipy import special
    return R.rotate_affine(shape, special.cosdg(angle), special.sindg(angle), axes)


@pytest.mark.parametrize("zoom", ZOOMS)
def test_restatement_equals_scipy_zoom(zoom):
    img, lab = volumes()
    out = R.zoom_size(SHAPE, zoom)
    m, t = R.zoom_affine(SHAPE, out)
    for x, order in ((lab, 0), (img, 0), (img, 1)):
        ref = scipy_zoom(x, zoom, order)
        got = R.resample_affine(x, m, t, out, order)
        assert got.shape == ref.shape and got.dtype == ref.dtype
        assert int((got != ref).sum()) == 0, (zoom, order, x.dtype)


@pytest.mark.parametrize("axes", PLANES)
@pytest.mark.parametrize("angle", GENERIC_ANGLES + SPECIAL_ANGLES)
def test_restatement_equals_scipy_rotate(angle, axes):
    img, lab = volumes()
    m, t = scipy_rotation(SHAPE, angle, axes)
    for x, order in ((lab, 0), (img, 0), (img, 1)):
        ref = scipy_rotate(x, angle, axes, order)
        got = R.resample_affine(x, m, t, SHAPE, order)
        assert got.dtype == ref.dtype
        assert int((got != ref).sum()) == 0, (angle, axes, order, x.dtype)


def test_restatement_outside_rule_and_ties():
    from scipy import ndimage
    a = np.arange(1, 6, dtype=np.float32)
    x = a.reshape(1, 1, 1, 5)
    for c in (-0.49, -1e-9, 0.0, 0.5, 1.5, 3.999, 4.0, 4.0 + 1e-9):
        for order in (0, 1):
            ref = ndimage.map_coordinates(a, [[c]], order=order, mode="constant", cval=0.0)[0]
            got = R.resample_affine(x, np.eye(3), (0.0, 0.0, c), (1, 1, 1), order)[0, 0, 0, 0]
            assert got == ref, (c, order)
    assert R.resample_affine(x, np.eye(3), (0.0, 0.0, -0.49), (1, 1, 1), 0)[0, 0, 0, 0] == 0      # not a[0]
    assert R.resample_affine(x, np.eye(3), (0.0, 0.0, 0.5), (1, 1, 1), 0)[0, 0, 0, 0] == 2        # ties round up


# ---- host logic of the transforms on the restatement

def _fx(golden_dir, name="resample.npz"):
    return np.load(os.path.join(golden_dir, name), allow_pickle=False)


@pytest.fixture
def host_transforms(monkeypatch):
    """fplx.transform with the kernel replaced by the numpy restatement and the device check by a rank check"""
    from fplx import transform as T

    def resample(x, matrix, offset, out_size, order):
        return torch.from_numpy(R.resample_affine(x.numpy(), matrix, offset, [int(v) for v in out_size], order))

    def check(t, name):
        if not (torch.is_tensor(t) and t.dim() == 4):
            raise ValueError("fplx.transform: sample['{0:}'] must be a [C,D,H,W] device tensor".format(name))
        return t.contiguous()

    monkeypatch.setattr(T.ops, "resample_affine", resample)
    monkeypatch.setattr(T, "_check_volume", check)
    return T


def _sample(g):
    return {k: torch.from_numpy(g[k].copy()) for k in ("image", "label", "pixel_weight")}


def _params(g, variant=None):
    p = json.loads(str(g["params_json"]))
    if variant:
        p.update(json.loads(str(g["variants_json"]))[variant])
    return p


def _seed(seed):
    random.seed(seed)
    np.random.seed(seed)


def _check_against_fixture(g, key, s, param_keys):
    for k in param_keys:
        assert json.loads(s[k]) == json.loads(str(g[key + k])), (key, k)
    # the draws left both generators where the reference left them
    assert random.random() == float(g[key + "next_random"]), key
    assert np.random.uniform() == float(g[key + "next_np_random"]), key
    for k in ("image", "label", "pixel_weight"):
        got = s[k].numpy()
        assert got.shape == g[key + k].shape and got.dtype == g[key + k].dtype, (key, k)
    # labels: a condition.  Images: the host's cos / sin may differ from scipy's cosdg / sindg in the last bit
    # (DESIGN, "where bit parity is not promised"); with the exact restatement nothing else can differ
    assert np.array_equal(s["label"].numpy(), g[key + "label"]), key
    for k in ("image", "pixel_weight"):
        assert_close_to_scipy(s[k].numpy(), g[key + k], (key, k))


def ulp_distance(a, b):
    """distance in units of the last place between two float32 arrays (finite values)"""
    def ordered(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(ordered(a) - ordered(b))


def assert_close_to_scipy(got, ref, what):
    """the fp32 criterion of the feature: every element within 1 fp32 ulp of scipy's, at most 1e-4 of them not identical"""
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.float32, what
    d = ulp_distance(got, ref)
    differing = int((d != 0).sum())
    print("%s: %d of %d elements differ from scipy, max %d ulp" % (what, differing, d.size, int(d.max()) if d.size else 0))
    assert int(d.max()) <= 1, what
    assert differing <= 1e-4 * d.size, (what, differing, d.size)


def test_transforms_reproduce_reference_parameters_shapes_and_draw_order(golden_dir, host_transforms):
    T = host_transforms
    g = _fx(golden_dir)
    seeds = [int(v) for v in g["seeds"]]
    assert len(seeds) >= 5
    for seed in seeds:
        _seed(seed)
        s = T.RandomRotate(_params(g))(_sample(g))
        _check_against_fixture(g, "seed%d_rotate_" % seed, s, ["RandomRotate_Param"])
        assert s["RandomRotate_Param"] == str(g["seed%d_rotate_RandomRotate_Param" % seed])        # the very string
        _seed(seed)
        s = T.RandomRescale(_params(g))(_sample(g))
        _check_against_fixture(g, "seed%d_randomrescale_" % seed, s, ["RandomRescale_origin_shape"])
    _seed(seeds[0])
    s = T.RandomRotate(_params(g, "rotate_d"))(_sample(g))
    _check_against_fixture(g, "rotate_d_", s, ["RandomRotate_Param"])
    assert len(json.loads(s["RandomRotate_Param"])) == 1
    _seed(seeds[0])
    s = T.RandomRescale(_params(g, "randomrescale_scalar"))(_sample(g))
    _check_against_fixture(g, "randomrescale_scalar_", s, ["RandomRescale_origin_shape"])
    for key, variant in (("rescale_list_", None), ("rescale_none_", "rescale_none"), ("rescale_int_", "rescale_int")):
        _seed(seeds[0])
        s = T.Rescale(_params(g, variant))(_sample(g))
        _check_against_fixture(g, key, s, ["Rescale_origin_shape"])


def test_inverses_reproduce_reference(golden_dir, host_transforms):
    T = host_transforms
    g, gi = _fx(golden_dir), _fx(golden_dir, "resample_inverse.npz")
    shape = g["image"].shape[1:]
    assert np.array_equal(gi["predict"], R.prediction("rs.predict", shape))
    for seed in [int(v) for v in g["seeds"]]:
        k = "seed%d_" % seed
        s = {"RandomRotate_Param": str(g[k + "rotate_RandomRotate_Param"]), "predict": torch.from_numpy(gi["predict"].copy())}
        s = T.RandomRotate(_params(g)).inverse_transform_for_prediction(s)
        assert_close_to_scipy(s["predict"].numpy(), gi[k + "rotate_inverse"], k + "rotate_inverse")
        pred = R.prediction("rs.predict.%d" % seed, g[k + "randomrescale_image"].shape[1:])
        s = {"RandomRescale_origin_shape": [str(g[k + "randomrescale_RandomRescale_origin_shape"])],    # as a batch collates it
             "predict": torch.from_numpy(pred)}
        s = T.RandomRescale(_params(g)).inverse_transform_for_prediction(s)
        assert_close_to_scipy(s["predict"].numpy(), gi[k + "randomrescale_inverse"], k + "randomrescale_inverse")
    pred = R.prediction("rs.predict.rescale", g["rescale_list_image"].shape[1:])
    s = {"Rescale_origin_shape": str(g["rescale_list_Rescale_origin_shape"]), "predict": torch.from_numpy(pred)}
    s = T.Rescale(_params(g)).inverse_transform_for_prediction(s)
    assert_close_to_scipy(s["predict"].numpy(), gi["rescale_inverse"], "rescale_inverse")


def test_registry_asserts_and_refusals(host_transforms):
    T = host_transforms
    for name in ("RandomRotate", "Rescale", "RandomRescale"):
        assert name in T.TransformDict
    p = {"task": "segmentation", "randomrotate_angle_range_d": None, "randomrotate_angle_range_h": None,
         "randomrotate_angle_range_w": None, "rescale_output_size": [8, 8, 8], "randomrescale_lower_bound": 1,
         "randomrescale_upper_bound": 2}
    vol = {"image": torch.zeros((1, 4, 5, 6))}
    with pytest.raises(AssertionError):
        T.RandomRotate(p)(dict(vol))                       # no range set
    with pytest.raises(AssertionError):
        T.RandomRescale(p)                                 # integer bounds, as in the reference
    with pytest.raises(AssertionError):
        T.Rescale(dict(p, rescale_output_size="8"))
    p["randomrotate_angle_range_d"] = [-10, 10]
    for t in (T.RandomRotate(p), T.Rescale(p), T.RandomRescale(dict(p, randomrescale_lower_bound=0.9,
                                                                      randomrescale_upper_bound=1.1))):
        with pytest.raises(ValueError, match=r"must be a \[C,D,H,W\] device tensor"):
            t({"image": torch.zeros((1, 5, 6))})
    # a sample without label / pixel_weight, and image1 left alone
    s = T.Rescale(p)({"image": torch.ones((2, 4, 5, 6)), "image1": torch.ones((2, 4, 5, 6))})
    assert tuple(s["image"].shape) == (2, 8, 8, 8) and tuple(s["image1"].shape) == (2, 4, 5, 6)
    assert json.loads(s["Rescale_origin_shape"]) == [2, 4, 5, 6]
    with pytest.raises(ValueError, match="float32"):
        T.Rescale(p)({"image": torch.ones((1, 4, 5, 6), dtype=torch.uint8)})


def test_host_trig_is_exact_at_right_angles_and_its_offset_is_scipys():
    from scipy import special
    from fplx import transform as T
    for a in (0, 90, 180, 270, 360, -90, -180, -270, 450):
        c, s = T._cos_sin_deg(a)
        assert (c, s) == (float(special.cosdg(a)), float(special.sindg(a))), a
        assert abs(c) in (0.0, 1.0) and abs(s) in (0.0, 1.0)
    rng = np.random.RandomState(7)
    # given scipy's own cos / sin, the offset is scipy's to the bit (its BLAS product rounds once per row)
    for a in rng.uniform(-180, 180, 200):
        c, s = float(special.cosdg(a)), float(special.sindg(a))
        for axes in PLANES:
            m_ref, t_ref = R.rotate_affine(SHAPE, c, s, axes)
            saved = T._cos_sin_deg
            T._cos_sin_deg = lambda _a: (c, s)
            try:
                m, t = T._rotate_affine(SHAPE, a, axes)
            finally:
                T._cos_sin_deg = saved
            assert np.array_equal(np.array(m), m_ref) and np.array_equal(np.array(t), t_ref), (a, axes)


def test_abi_rejects_bad_arguments_before_any_launch():
    from fplx import _lib
    lib = _lib.lib()
    x = (ctypes.c_float * 64)()
    y = (ctypes.c_float * 64)()
    m = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    t = (ctypes.c_double * 3)()
    f = lib.fplx_resample_affine
    assert f(None, y, 4, 1, 1, 4, 4, 4, 4, 4, 4, m, t, None) == -5
    assert f(x, None, 4, 1, 1, 4, 4, 4, 4, 4, 4, m, t, None) == -5
    assert f(x, y, 4, 1, 1, 4, 4, 4, 4, 4, 4, None, t, None) == -5
    assert f(x, y, 4, 1, 1, 4, 4, 4, 4, 4, 4, m, None, None) == -5 and "resample_affine" in _lib.last_error()
    for c, d, h, w in ((0, 4, 4, 4), (1, 0, 4, 4), (1, 4, -1, 4), (1, 4, 4, 0), (2, 1 << 10, 1 << 10, 1 << 10),
                       (1 << 30, 1 << 30, 1 << 30, 1 << 30)):
        assert f(x, y, 4, 1, c, d, h, w, 4, 4, 4, m, t, None) == -1, (c, d, h, w)
    for od, oh, ow in ((0, 4, 4), (4, -1, 4), (4, 4, 0), (1 << 11, 1 << 10, 1 << 10), (1 << 30, 1 << 30, 1 << 30)):
        assert f(x, y, 4, 0, 1, 4, 4, 4, od, oh, ow, m, t, None) == -1, (od, oh, ow)
    for order in (-1, 2, 3):
        assert f(x, y, 4, order, 1, 4, 4, 4, 4, 4, 4, m, t, None) == -1
    for elem_bytes in (0, 2, 8):
        assert f(x, y, elem_bytes, 0, 1, 4, 4, 4, 4, 4, 4, m, t, None) == -2
    assert f(x, y, 1, 1, 1, 4, 4, 4, 4, 4, 4, m, t, None) == -2 and "uint8" in _lib.last_error()
    with pytest.raises(ValueError):
        _lib.check(f(x, y, 1, 1, 1, 4, 4, 4, 4, 4, 4, m, t, None))
    import fplx
    with pytest.raises(RuntimeError, match="must live on the GPU"):         # no CPU fallback
        fplx.ops.resample_affine(torch.zeros((1, 4, 4, 4)), np.eye(3), (0, 0, 0), (4, 4, 4), 1)
