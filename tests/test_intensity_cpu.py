"""CPU tests of the intensity transforms' host side: the percentile interpolation restated in tests/intensity_ref.py (and
its twin in fplx.ops, which the product uses on the device's order statistics) against numpy.percentile itself, the
restatements against the reference-generated fixtures tests/golden/intensity*.npz, and the registry."""
import json
import os

import numpy as np
import pytest

import detdata
import intensity_ref as IR

SEVEN = {
    "NormalizeWithMinMax": ["normalizewithminmax_channels", "normalizewithminmax_threshold_lower",
                            "normalizewithminmax_threshold_upper"],
    "NormalizeWithPercentiles": ["normalizewithpercentiles_channels", "normalizewithpercentiles_percentile_lower",
                                 "normalizewithpercentiles_percentile_upper"],
    "ChannelWiseThreshold": ["channelwisethreshold_channels", "channelwisethreshold_threshold_lower",
                             "channelwisethreshold_threshold_upper", "channelwisethreshold_replace_lower",
                             "channelwisethreshold_replace_upper"],
    "ChannelWiseThresholdWithNormalize": ["channelwisethresholdwithnormalize_channels",
                                          "channelwisethresholdwithnormalize_threshold_lower",
                                          "channelwisethresholdwithnormalize_threshold_upper",
                                          "channelwisethresholdwithnormalize_mean_std_mode"],
    "GammaCorrection": ["gammacorrection_channels", "gammacorrection_gamma_min", "gammacorrection_gamma_max"],
    "GaussianNoise": ["gaussiannoise_channels", "gaussiannoise_mean", "gaussiannoise_std"],
    "NormalizeWithMeanStd_dual": ["normalizewithmeanstd_channels"],
}


def _fx(golden_dir, name="intensity.npz"):
    return np.load(os.path.join(golden_dir, name), allow_pickle=False)


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _volumes():
    img = IR.inputs()[0]
    yield "normal 12x40x50", detdata.normal("it.cpu.a", (12, 40, 50), 30.0, 5.0)
    yield "fixture channel 0", img[0]
    yield "fixture channel 1 (ties)", img[1]
    yield "70 % zeros", np.where(detdata.uniform("it.cpu.z", (9, 31, 17)) < 0.7, 0.0, detdata.normal("it.cpu.zz", (9, 31, 17))).astype(np.float32)
    for n in (1, 2, 3, 255, 256, 257):
        yield "n = %d" % n, detdata.normal("it.cpu.n%d" % n, (n,), 3.0)


def test_lerp_restatement_equals_numpy_percentile():
    """0 differing bit patterns over some thousand q per volume, q = 0 and q = 100 among them; the result is a numpy.float32"""
    from fplx import ops
    total = 0
    for what, x in _volumes():
        qs = np.concatenate([np.linspace(0.0, 100.0, 1003), detdata.uniform("it.cpu.q." + what, (1000,), 0.0, 100.0).astype(np.float64),
                             [0.0, 100.0, 50.0, 1.0, 99.0, 0.5, 99.9]])
        # one call per q with a Python float, as the reference calls it: an ARRAY of q would promote the result to float64
        want = [np.percentile(x, float(q)) for q in qs]
        assert all(type(w) is np.float32 for w in want)
        flat = np.sort(x.reshape(-1))
        n = flat.size
        bad = 0
        for q, w in zip(qs, want):
            got = IR.percentile(x, float(q))
            assert type(got) is np.float32
            lo, g = ops.percentile_index(n, float(q))
            assert (lo, g) == IR.percentile_index(n, float(q))[::2]
            twin = ops.percentile_lerp(flat[lo], flat[min(lo + 1, n - 1)], g)
            bad += int(_bits(got) != _bits(w)) + int(_bits(twin) != _bits(w))
        total += len(qs)
        assert bad == 0, (what, bad, len(qs))
    assert total > 10000


def test_percentile_scalar_call_is_float32():
    x = IR.inputs()[0][0]
    for q in (0, 1.0, 37.5, 99.0, 100):
        w = np.percentile(x, q)
        assert isinstance(w, np.float32) and _bits(IR.percentile(x, q)) == _bits(w)


def test_restatement_reproduces_the_fixture(golden_dir):
    g = _fx(golden_dir)
    cases = json.loads(str(g["cases_json"]))
    img = g["image"]
    assert np.array_equal(img, IR.inputs()[0]) and np.array_equal(g["image1"], IR.inputs()[1])
    assert (img < 0).mean() > 0.05 and (img[1] == img[1].min()).sum() > 1          # partly negative, with ties
    for key in ("percentiles_1_99", "percentiles_wide", "percentiles_0_100"):
        p = cases[key][1]
        chns = p["normalizewithpercentiles_channels"]
        want = img.copy()
        for c in (chns if chns is not None else range(img.shape[0])):
            v0 = IR.percentile(img[c], p["normalizewithpercentiles_percentile_lower"])
            v1 = IR.percentile(img[c], p["normalizewithpercentiles_percentile_upper"])
            want[c] = IR.clip_affine(img[c], v0, v1)
        assert np.array_equal(_bits(want), _bits(g[key + "_image"])), key
    want = np.stack([IR.clip_affine(img[c], img[c].min(), img[c].max()) for c in range(img.shape[0])])
    assert np.array_equal(_bits(want), _bits(g["minmax_none_image"]))


def test_gamma_yardstick_reproduces_the_fixture(golden_dir):
    g, gm = _fx(golden_dir), _fx(golden_dir, "intensity_gamma.npz")
    cases = json.loads(str(g["cases_json"]))
    img = g["image"]
    seen = 0
    for key, case in [("seed%d_gamma_" % s, "gamma") for s in g["seeds"]] + [("gamma_always_", "gamma_always"),
                                                                            ("gamma_never_", "gamma_never")]:
        chns = cases[case][1]["gammacorrection_channels"]
        if not bool(gm[key + "fired"]):
            assert np.array_equal(_bits(gm[key + "image"]), _bits(img)) and float(gm[key + "e_ref"]) == 0.0
            continue
        seen += 1
        e = 0.0
        for j, (c, gamma) in enumerate(zip(chns, gm[key + "gammas"])):
            # the float64 power may differ in its last place between two C libraries: 4 float64 ulp, 1e-9 float32 ulp
            np.testing.assert_allclose(IR.gamma_f64(img[c], float(gamma)), gm[key + "f64"][j], rtol=1e-15 * 4, atol=0)
            u = IR.ulp_unit(img[c].min(), img[c].max())
            e = max(e, float(np.abs(gm[key + "image"][c].astype(np.float64) - gm[key + "f64"][j]).max() / u))
        assert abs(e - float(gm[key + "e_ref"])) < 1e-9
        assert 0.5 < e < 4.0          # numpy's float32 pass: three roundings and a power that is not correctly rounded
    assert seen >= 3 and float(gm["e_ref_max"]) < 4.0


def test_philox_noise_restatement():
    from oracle import np_ref
    words, u = IR.philox_uniforms(1001, 0x0123456789ABCDEF, 7)
    assert words.shape == (1001, 2) and words.dtype == np.uint32
    r = np_ref.philox4x32_10(np.array([0, 1, 500], np.uint32), 0, 7, 0, 0x89ABCDEF, 0x01234567)
    assert [int(words[0, 0]), int(words[0, 1]), int(words[1, 0]), int(words[1, 1])] == [int(r[k][0]) for k in range(4)]
    assert int(words[2, 0]) == int(r[0][1]) and int(words[1000, 1]) == int(r[1][2])
    assert u.min() > 0.0 and u.max() <= 1.0
    x = detdata.normal("it.cpu.noise", (50, 40), 10.0)
    y, z = IR.philox_noise(x, 99, 1, 2.0, 3.0)
    assert y.dtype == np.float32 and np.isfinite(z).all() and abs(z.mean()) < 0.1 and abs(z.std() - 1.0) < 0.05
    assert np.array_equal(y, ((x.astype(np.float64).reshape(-1) + 2.0) + 3.0 * z).astype(np.float32).reshape(x.shape))
    assert not np.array_equal(y, IR.philox_noise(x, 99, 2, 2.0, 3.0)[0])
    assert not np.array_equal(y, IR.philox_noise(x, 98, 1, 2.0, 3.0)[0])


def test_the_seven_names_are_registered_with_the_reference_keys(golden_dir):
    from fplx import transform as T
    cases = json.loads(str(_fx(golden_dir)["cases_json"]))
    for name, keys in SEVEN.items():
        assert name in T.TransformDict, name
        params = {"task": "segmentation"}
        params.update({k: None for k in keys})
        t = T.TransformDict[name](params)
        assert t.inverse is False and t.task == "segmentation"
        for k in keys:                                       # every required key is required, as in the reference
            with pytest.raises(KeyError):
                T.TransformDict[name]({kk: v for kk, v in params.items() if kk != k})
    assert T.GammaCorrection(dict(cases["gamma"][1], task="segmentation")).prob == 0.5
    assert T.GaussianNoise(dict(cases["noise"][1], task="segmentation")).prob == 0.5
    assert T.GaussianNoise(dict(cases["noise"][1], task="segmentation")).device_rng is False
    for key, (name, p) in cases.items():
        if key == "chain":
            ts = T.build_transforms(name, dict(p, task="segmentation"))
            assert [type(t).__name__ for t in ts] == name
        else:
            assert type(T.TransformDict[name](dict(p, task="segmentation"))).__name__ == name
    # the earlier registry is unchanged
    for name in ("NormalizeWithMeanStd", "Pad", "RandomCrop", "RandomFlip", "LabelToProbability", "RandomRotate", "Rescale",
                 "RandomRescale"):
        assert name in T.TransformDict
