"""-m gpu tests of the intensity kernels (csrc/intensity.hip through fplx.ops) and of NormalizeWithMinMax,
NormalizeWithPercentiles, ChannelWiseThreshold, ChannelWiseThresholdWithNormalize, GammaCorrection, GaussianNoise and
NormalizeWithMeanStd_dual (fplx.transform) against numpy and against the reference-generated fixtures
tests/golden/intensity*.npz.

Criteria.  Selection, min / max, classes 1-3, the min-max mode of class 4, host-noise GaussianNoise and the given-moments
form of NormalizeWithMeanStd_dual: 0 differing elements.  Moments computed on the device (mean-std mode, the dual class):
NORM_RTOL / NORM_ATOL of test_gpu_transform.py on the normalised voxels, the replaced voxels exact.  GammaCorrection: within
e_ref + 0.5 float32 ulp (at max(|vmin|, |vmax|)) of the float64 evaluation, e_ref being the reference's own distance stored in
the fixture.  Device-generated noise: uniforms exact, every element within 1 float32 ulp of the float64 restatement and at
most 1e-4 of them not identical (the order-1 bar of test_gpu_resample.py).  Every tolerance comparison prints its figures."""
import json
import os
import random

import numpy as np
import pytest
import torch

import detdata
import intensity_ref as IR
from test_gpu_transform import NORM_ATOL, NORM_RTOL

pytestmark = pytest.mark.gpu

FULL = (48, 160, 272)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _fx(golden_dir, name="intensity.npz"):
    return np.load(os.path.join(golden_dir, name), allow_pickle=False)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b):
    return int((_bits(a) != _bits(b)).sum())


def _seed(seed):
    random.seed(seed)
    np.random.seed(seed)


def _cases(golden_dir):
    return json.loads(str(_fx(golden_dir)["cases_json"]))


def _make(case):
    from fplx import transform as T
    name, p = case
    return T.TransformDict[name](dict(json.loads(json.dumps(p)), task="segmentation"))


def _sample(g):
    return {"image": _dev(g["image"]), "image1": _dev(g["image1"]), "label": _dev(g["label"])}


def _run(t, g):
    """-> (image as numpy, sample); the other keys must come back untouched and the image must be the SAME tensor (in place)"""
    s = _sample(g)
    before = dict(s)
    out = t(s)
    assert out is s and set(out.keys()) == set(before.keys())
    assert out["image"] is before["image"] and out["label"] is before["label"]
    assert np.array_equal(out["label"].cpu().numpy(), g["label"])
    if not type(t).__name__.endswith("_dual"):
        assert out["image1"] is before["image1"] and np.array_equal(out["image1"].cpu().numpy(), g["image1"])
    return out["image"].cpu().numpy(), out


# ---------------------------------------------------------------- selection

def _select(x, ranks):
    from fplx import ops
    got = ops.select_kth(_dev(np.asarray(x, np.float32).reshape(-1)), ranks)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(ranks), 2) and got.is_cuda
    return got.cpu().numpy()


def _check_select(x, ranks, what):
    s = np.sort(np.asarray(x, np.float32).reshape(-1))
    n = s.size
    for lo in range(0, len(ranks), 4):
        rk = list(ranks[lo:lo + 4])
        want = np.array([[s[k], s[min(k + 1, n - 1)]] for k in rk], np.float32)
        got = _select(x, rk)
        # equal as VALUES: -0.0 and +0.0 tie in numpy's sort, NaNs sort last
        assert np.array_equal(got, want, equal_nan=True), (what, rk, got, want)


def _ranks(n, name):
    r = {0, n - 1, n // 2, max(n - 2, 0), min(1, n - 1), n // 100, (n * 99) // 100}
    r |= set(int(v) for v in (detdata.uniform("it.rank." + name, (9,)) * n).astype(np.int64).clip(0, n - 1))
    return sorted(r)


def test_select_random_normals_and_small_sizes():
    for n in (1, 2, 3, 63, 64, 65, 255, 256, 257, 1000, 100003):
        x = detdata.normal("it.sel.%d" % n, (n,), 100.0, -7.0)
        _check_select(x, _ranks(n, "n%d" % n) if n > 300 else list(range(n)), ("normal", n))


def test_select_heavy_ties():
    shape = (20, 64, 72)
    zeros = np.where(detdata.uniform("it.sel.zmask", shape) < 0.7, 0.0, detdata.normal("it.sel.zval", shape, 50.0)).astype(np.float32)
    _check_select(zeros, _ranks(zeros.size, "zeros"), "70 % zeros")
    u8 = np.floor(detdata.uniform("it.sel.u8", shape) ** 2 * 256.0).astype(np.float32)
    _check_select(u8, _ranks(u8.size, "u8"), "uint8-valued")
    const = np.full(5000, -3.25, np.float32)
    _check_select(const, [0, 1, 2499, 4998, 4999], "constant")


def test_select_special_values():
    tiny = np.float32(1e-45)
    x = np.array([0.0, -0.0, np.inf, -np.inf, tiny, -tiny, 3 * tiny, 1.17549435e-38, -1.17549435e-38, 1.0, -1.0, 0.0, -0.0,
                  3.4028235e38, -3.4028235e38, np.inf, -np.inf, 2.5, -0.0, 0.0], np.float32)
    x = np.concatenate([x, detdata.normal("it.sel.special", (500,), 1e-39)]).astype(np.float32)      # denormals
    _check_select(x, list(range(x.size)), "special values")
    got = _select(x, [4, 5])                                  # signed zeros come back as zeros of either sign
    s = np.sort(x)
    assert np.array_equal(got, np.array([[s[4], s[5]], [s[5], s[6]]]))
    y = x.copy()
    y[7] = np.nan
    y[300] = -np.nan
    _check_select(y, list(range(y.size - 4, y.size)) + [0, 1, 2], "NaNs sort last")


def test_select_full_volume_and_rank_grouping():
    x = detdata.normal("it.sel.full", FULL, 300.0, 100.0)
    n = x.size
    rk = [0, n - 1, percentile_rank(n, 1.0), percentile_rank(n, 99.0)]
    _check_select(x, rk + [n // 2, n // 3, 12345, n - 2], "48x160x272")
    # four ranks in one call against four calls, bit for bit; and the same call twice
    four = _select(x, rk)
    assert np.array_equal(_bits(four), _bits(_select(x, rk)))
    for j, k in enumerate(rk):
        assert np.array_equal(_bits(four[j]), _bits(_select(x, [k])[0]))
    assert np.array_equal(_bits(_select(x, [7, 7, 7, 8])[0]), _bits(_select(x, [7])[0]))


def percentile_rank(n, q):
    return IR.percentile_index(n, q)[0]


def test_select_refuses_bad_ranks():
    from fplx import _lib, ops
    x = _dev(detdata.normal("it.sel.bad", (100,)))
    for rk in ([100], [-1], [0, 1, 2, 3, 4], [], [5, 100]):
        with pytest.raises(ValueError):
            ops.select_kth(x, rk)
    assert "rank 100 outside [0, 100)" in _lib.last_error()
    assert np.array_equal(ops.select_kth(x, [99]).cpu().numpy()[0], [x.max().item()] * 2)       # nothing was left behind


def test_channel_minmax_and_its_nan_policy():
    from fplx import ops
    for n in (1, 2, 257, 70001):
        x = detdata.normal("it.mm.%d" % n, (n,), 40.0, 3.0)
        got = ops.channel_minmax(_dev(x)).cpu().numpy()
        assert np.array_equal(_bits(got), _bits([x.min(), x.max(), x.min(), x.max()])), n
        c = x.copy()
        c[c < np.float32(-10.5)] = np.float32(-10.5)
        c[c > np.float32(20.25)] = np.float32(20.25)
        got = ops.channel_minmax(_dev(x), -10.5, 20.25).cpu().numpy()
        assert np.array_equal(_bits(got), _bits([x.min(), x.max(), c.min(), c.max()])), n
        lo_only = np.where(x < np.float32(1.5), np.float32(1.5), x)
        got = ops.channel_minmax(_dev(x), 1.5, None).cpu().numpy()
        assert np.array_equal(_bits(got), _bits([x.min(), x.max(), lo_only.min(), lo_only.max()])), n
    # numpy's min / max propagate NaN; a clip written as comparisons lets it through, so all four are NaN
    x = detdata.normal("it.mm.nan", (5000,))
    x[1234] = np.nan
    assert np.isnan(ops.channel_minmax(_dev(x), -1.0, 1.0).cpu().numpy()).all() and np.isnan(x.min()) and np.isnan(x.max())
    x = np.array([-np.inf, 0.0, -0.0, np.inf], np.float32)
    assert np.array_equal(ops.channel_minmax(_dev(x)).cpu().numpy(), [-np.inf, np.inf, -np.inf, np.inf])


# ---------------------------------------------------------------- the bit-identical classes against the fixture

@pytest.mark.parametrize("key", ["minmax_none", "minmax_given", "minmax_mixed", "percentiles_1_99", "percentiles_wide",
                                 "percentiles_0_100", "cwt_both", "cwt_partial"])
def test_classes_1_to_3_bit_identical(golden_dir, key):
    g = _fx(golden_dir)
    got, _ = _run(_make(_cases(golden_dir)[key]), g)
    bad = _same_bits(got, g[key + "_image"])
    print(key, "differing elements:", bad, "of", got.size)
    assert bad == 0 and not np.array_equal(got, g["image"])


@pytest.mark.parametrize("key", ["cwtn_minmax_both", "cwtn_minmax_partial"])
def test_threshold_with_normalize_min_max_mode_bit_identical(golden_dir, key):
    g, w = _fx(golden_dir), _fx(golden_dir, "intensity_cwtn.npz")
    got, _ = _run(_make(_cases(golden_dir)[key]), g)
    bad = _same_bits(got, w[key + "_image"])
    print(key, "differing elements:", bad, "of", got.size)
    assert bad == 0


def _inside(x, v0, v1):
    m = np.ones(x.shape, bool)
    if v0 is not None:
        m &= x > np.float32(v0)
    if v1 is not None:
        m &= x < np.float32(v1)
    return m


def _check_mean_std(got, want, img, p, what):
    lower = p["channelwisethresholdwithnormalize_threshold_lower"]
    upper = p["channelwisethresholdwithnormalize_threshold_upper"]
    chns = p["channelwisethresholdwithnormalize_channels"]
    for c in (chns if chns is not None else range(img.shape[0])):
        m = _inside(img[c], lower[c], upper[c])
        assert m.any() and (~m).any()
        assert _same_bits(got[c][~m], want[c][~m]) == 0, (what, c, "replaced voxels")
        err = np.abs(got[c][m].astype(np.float64) - want[c][m])
        print(what, "channel", c, "max abs error of the normalised voxels %.3g" % err.max(), "differing",
              _same_bits(got[c][m], want[c][m]), "of", int(m.sum()))
        np.testing.assert_allclose(got[c][m], want[c][m], rtol=NORM_RTOL, atol=NORM_ATOL)


def test_threshold_with_normalize_mean_std_mode(golden_dir):
    g, w = _fx(golden_dir), _fx(golden_dir, "intensity_cwtn.npz")
    cases = _cases(golden_dir)
    runs = [("seed%d_cwtn_meanstd_" % s, int(s), "cwtn_meanstd") for s in g["seeds"][:3]]
    runs.append(("cwtn_meanstd_partial_", int(g["seeds"][0]), "cwtn_meanstd_partial"))
    for key, seed, case in runs:
        _seed(seed)
        got, _ = _run(_make(cases[case]), g)
        _check_mean_std(got, w[key + "image"], g["image"], cases[case][1], key)
        assert random.random() == float(w[key + "next_random"]) and np.random.uniform() == float(w[key + "next_np_random"])


def test_normalize_mean_std_dual(golden_dir):
    g, w, nz = _fx(golden_dir), _fx(golden_dir, "intensity_cwtn.npz"), _fx(golden_dir, "intensity_noise.npz")
    cases = _cases(golden_dir)
    t = _make(cases["dual_plain"])
    assert t.mean is None
    got, s = _run(t, g)
    assert t.mean == [None, None] and t.std == [None, None]              # filled on first use, as in the reference
    for name, arr in (("image", got), ("image1", s["image1"].cpu().numpy())):
        np.testing.assert_allclose(arr, w["dual_plain_" + name], rtol=NORM_RTOL, atol=NORM_ATOL)
    got, s = _run(_make(cases["dual_given"]), g)
    assert _same_bits(got, w["dual_given_image"]) == 0 and _same_bits(s["image1"].cpu().numpy(), w["dual_given_image1"]) == 0
    _seed(int(g["seeds"][0]))
    got, s = _run(_make(cases["dual_np"]), g)
    for name, arr, src in (("image", got, g["image"]), ("image1", s["image1"].cpu().numpy(), g["image1"])):
        bg = src <= 0
        assert bg.any() and _same_bits(arr[bg], nz["dual_np_" + name][bg]) == 0
        np.testing.assert_allclose(arr[~bg], nz["dual_np_" + name][~bg], rtol=NORM_RTOL, atol=NORM_ATOL)
    assert np.random.uniform() == float(nz["dual_np_next_np_random"])
    with pytest.raises(KeyError):
        _make(cases["dual_plain"])({"image": _dev(g["image"])})


def test_gaussian_noise_host_draw_bit_identical(golden_dir):
    g, w = _fx(golden_dir), _fx(golden_dir, "intensity_noise.npz")
    cases = _cases(golden_dir)
    runs = [("seed%d_noise_" % s, int(s), "noise") for s in g["seeds"]]
    runs += [("noise_always_", int(g["seeds"][0]), "noise_always"), ("noise_never_", int(g["seeds"][0]), "noise_never")]
    fired = 0
    for key, seed, case in runs:
        _seed(seed)
        got, _ = _run(_make(cases[case]), g)
        if bool(w[key + "fired"]):
            fired += 1
            bad = _same_bits(got, w[key + "image"])
            print(key, "differing elements:", bad)
            assert bad == 0
        else:
            assert _same_bits(got, g["image"]) == 0, key             # the gate did not fire: untouched
        assert random.random() == float(w[key + "next_random"]) and np.random.uniform() == float(w[key + "next_np_random"])
    assert 0 < fired < len(runs)


# ---------------------------------------------------------------- gamma

def test_gamma_correction_within_the_reference_error(golden_dir):
    """Observed figures are printed per case (and recorded in DESIGN.md 1f)."""
    g, w = _fx(golden_dir), _fx(golden_dir, "intensity_gamma.npz")
    cases = _cases(golden_dir)
    img = g["image"]
    runs = [("seed%d_gamma_" % s, int(s), "gamma") for s in g["seeds"]]
    runs += [("gamma_always_", int(g["seeds"][0]), "gamma_always"), ("gamma_never_", int(g["seeds"][0]), "gamma_never")]
    fired = 0
    for key, seed, case in runs:
        _seed(seed)
        t = _make(cases[case])
        got, _ = _run(t, g)
        assert random.random() == float(w[key + "next_random"]) and np.random.uniform() == float(w[key + "next_np_random"])
        if not bool(w[key + "fired"]):
            assert _same_bits(got, img) == 0, key
            continue
        fired += 1
        chns = cases[case][1]["gammacorrection_channels"]
        assert t.last_gammas == [float(v) for v in w[key + "gammas"]]        # the drawn gammas, exactly
        e_ref = float(w[key + "e_ref"])
        worst = 0.0
        for j, c in enumerate(chns):
            u = IR.ulp_unit(img[c].min(), img[c].max())
            worst = max(worst, float(np.abs(got[c].astype(np.float64) - w[key + "f64"][j]).max() / u))
        differ = sum(_same_bits(got[c], w[key + "image"][c]) for c in chns) / float(sum(got[c].size for c in chns))
        print(key, "gammas", t.last_gammas, "max distance from the float64 evaluation: %.4f u (reference %.4f u);"
              " share of elements not identical to the reference: %.4f" % (worst, e_ref, differ))
        assert worst <= e_ref + 0.5
        for c in range(img.shape[0]):
            if c not in chns:
                assert _same_bits(got[c], img[c]) == 0
    assert 0 < fired < len(runs)


# ---------------------------------------------------------------- device-generated noise

def _ulp_distance(a, b):
    def key(v):
        i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def test_device_noise_against_the_restatement():
    from fplx import ops
    n = 200001
    x = detdata.normal("it.noise.x", (n,), 30.0, 10.0)
    seed, sid, mean, std = 0xC0FFEE1234567890, 3, 1.5, 6.25
    y, u = ops.add_noise_philox(_dev(x), seed, sid, mean, std, want_uniforms=True)
    y, u = y.cpu().numpy(), u.cpu().numpy()
    words, want_u = IR.philox_uniforms(n, seed, sid)
    assert np.array_equal(u, want_u)                                        # uniforms exact
    assert np.array_equal((u * 4294967296.0 - 1.0).astype(np.uint32), words)  # and with them the Philox words
    want, _ = IR.philox_noise(x, seed, sid, mean, std)
    d = _ulp_distance(y, want)
    print("device noise: max ulp distance", int(d.max()), "not identical", int((d > 0).sum()), "of", n)
    assert d.max() <= 1 and (d > 0).sum() <= 1e-4 * n
    # the same seed gives the same bits; another seed or stream does not; in place is the same
    again = ops.add_noise_philox(_dev(x), seed, sid, mean, std).cpu().numpy()
    assert _same_bits(again, y) == 0
    assert _same_bits(ops.add_noise_philox(_dev(x), seed + 1, sid, mean, std).cpu().numpy(), y) > n // 2
    assert _same_bits(ops.add_noise_philox(_dev(x), seed, sid + 1, mean, std).cpu().numpy(), y) > n // 2
    assert _same_bits(ops.add_noise_philox(_dev(x), seed ^ (1 << 40), sid, mean, std).cpu().numpy(), y) > n // 2
    xd = _dev(x)
    ops.add_noise_philox(xd, seed, sid, mean, std, out=xd)
    assert _same_bits(xd.cpu().numpy(), y) == 0


def test_device_noise_moments():
    from fplx import ops
    n = 3600000
    z = ops.add_noise_philox(torch.zeros(n, dtype=torch.float32, device="cuda:0"), 20240229, 0, 0.0, 1.0).cpu().numpy()
    z = z.astype(np.float64)
    m, s = z.mean(), z.std()
    print("device noise over %d draws: mean %.6f (standard error %.6f), std %.6f (standard error %.6f)" % (
        n, m, 1 / np.sqrt(n), s, 1 / np.sqrt(2 * n)))
    assert abs(m) < 5.0 / np.sqrt(n) and abs(s - 1.0) < 5.0 / np.sqrt(2.0 * n)
    assert np.isfinite(z).all() and z.max() > 4.0 and z.min() < -4.0


def test_gaussian_noise_device_rng_extension(golden_dir):
    g = _fx(golden_dir)
    p = dict(_cases(golden_dir)["noise_always"][1], gaussiannoise_device_rng=True)
    outs = []
    for _ in range(2):
        _seed(11)
        t = _make(["GaussianNoise", p])
        got, _ = _run(t, g)
        outs.append(got)
        _seed(11)
        np.random.uniform()
        assert t.last_seed == random.getrandbits(64)                       # Python's seed fixes the run
        for c in (0, 1):
            assert _same_bits(got[c], IR.philox_noise(g["image"][c], t.last_seed, c, p["gaussiannoise_mean"],
                                                       p["gaussiannoise_std"])[0]) <= 1e-4 * got[c].size
    assert _same_bits(outs[0], outs[1]) == 0
    _seed(12)
    other, _ = _run(_make(["GaussianNoise", p]), g)
    assert _same_bits(other, outs[0]) > other.size // 2
    # a gate that does not fire draws no seed and leaves the tensor alone
    _seed(11)
    t = _make(["GaussianNoise", dict(p, gaussiannoise_probability=0.0)])
    got, _ = _run(t, g)
    assert t.last_seed is None and _same_bits(got, g["image"]) == 0


# ---------------------------------------------------------------- full size, chain, degenerate inputs

def test_percentiles_full_size_against_numpy():
    from fplx import transform as T
    x = (np.exp(detdata.normal("it.full", (1,) + FULL) * 0.8) * 90.0 - 40.0).astype(np.float32)
    p = {"task": "segmentation", "normalizewithpercentiles_channels": None, "normalizewithpercentiles_percentile_lower": 1.0,
         "normalizewithpercentiles_percentile_upper": 99.0}
    got = T.NormalizeWithPercentiles(p)({"image": _dev(x)})["image"].cpu().numpy()
    v0, v1 = np.percentile(x[0], 1.0), np.percentile(x[0], 99.0)
    assert isinstance(v0, np.float32)
    want = x.copy()
    c = want[0]
    c[c < v0] = v0
    c[c > v1] = v1
    want[0] = (c - v0) / (v1 - v0)
    bad = _same_bits(got, want)
    print("full size percentiles: v0 %r v1 %r, differing elements %d of %d" % (v0, v1, bad, got.size))
    assert bad == 0 and got.min() == 0.0 and got.max() == 1.0


def test_chain_against_the_fixture(golden_dir):
    """[NormalizeWithPercentiles, GammaCorrection, GaussianNoise, Pad, RandomCrop].  Percentiles are bit-identical, so the
    gamma stage sees the reference's input; its output is within (e_ref + 0.5) u of the reference's (both lie that close
    to the float64 evaluation on the same side of the bound the gamma test holds); adding the same float64 noise and
    rounding each sum once moves the two results apart by at most one more ulp of the result; Pad and RandomCrop copy."""
    from fplx import transform as T
    g, w = _fx(golden_dir), _fx(golden_dir, "intensity_chain.npz")
    names, p = _cases(golden_dir)["chain"]
    for seed in (int(s) for s in g["seeds"]):
        k = "seed%d_chain_" % seed
        _seed(seed)
        ts = T.build_transforms(names, dict(p, task="segmentation"))
        s = T.apply_transforms(ts, {"image": _dev(g["image"]), "label": _dev(g["label"])})
        assert json.loads(s["Pad_Param"]) == json.loads(str(w[k + "Pad_Param"]))
        assert json.loads(s["RandomCrop_Param"]) == json.loads(str(w[k + "RandomCrop_Param"]))
        assert random.random() == float(w[k + "next_random"]) and np.random.uniform() == float(w[k + "next_np_random"])
        assert np.array_equal(s["label"].cpu().numpy(), w[k + "label"])
        got, want = s["image"].cpu().numpy(), w[k + "image"]
        assert got.shape == want.shape and got.dtype == np.float32
        if bool(w[k + "gamma_fired"]):
            assert ts[1].last_gammas == [float(v) for v in w[k + "gammas"]]
        bound = (float(w[k + "e_ref"]) + 0.5) * float(w[k + "gamma_unit"]) * bool(w[k + "gamma_fired"]) + np.spacing(np.abs(want))
        err = np.abs(got.astype(np.float64) - want)
        print(k, "gamma fired", bool(w[k + "gamma_fired"]), "differing", _same_bits(got, want), "of", got.size,
              "max error / bound %.3f" % float((err / bound).max()))
        assert (err <= bound).all()
        if not bool(w[k + "gamma_fired"]):
            assert _same_bits(got, want) == 0


def test_degenerate_inputs(golden_dir):
    from fplx import ops, transform as T
    cases = _cases(golden_dir)
    const = np.full((2, 4, 6, 8), 3.5, np.float32)
    lab = np.zeros((1, 4, 6, 8), np.uint8)
    # a constant channel: 0 / 0, as in the reference
    s = _make(cases["minmax_none"])({"image": _dev(const), "label": _dev(lab)})
    assert np.isnan(s["image"].cpu().numpy()).all()
    s = _make(cases["gamma_always"])({"image": _dev(const), "label": _dev(lab)})
    out = s["image"].cpu().numpy()
    assert np.isnan(out[1]).all() and np.array_equal(out[0], const[0])
    # an empty mask in mean-std mode: NaN moments, every voxel replaced by the host draw
    p = dict(cases["cwtn_meanstd"][1])
    p["channelwisethresholdwithnormalize_threshold_lower"] = [1e6, 1e6]
    p["channelwisethresholdwithnormalize_threshold_upper"] = [2e6, 2e6]
    _seed(4)
    s = _make(["ChannelWiseThresholdWithNormalize", p])({"image": _dev(const), "label": _dev(lab)})
    _seed(4)
    want = np.stack([np.random.normal(0, 1, size=const.shape[1:]).astype(np.float32) for _ in range(2)])
    assert _same_bits(s["image"].cpu().numpy(), want) == 0
    y, ms = ops.normalize_range(_dev(const[0]), _dev(want[0]), 1e6, 2e6, want_moments=True)
    assert np.isnan(ms.cpu().numpy()).all() and _same_bits(y.cpu().numpy(), want[0]) == 0
    # NaN voxels pass through the clips; the percentiles of a volume with a NaN are NaN, as numpy's
    x = detdata.normal("it.deg.nan", (1, 4, 6, 8), 10.0)
    x[0, 1, 2, 3] = np.nan
    got = _make(cases["cwt_both"])({"image": _dev(np.concatenate([x, x])), "label": _dev(lab)})["image"].cpu().numpy()
    assert np.isnan(got[:, 1, 2, 3]).all() and np.isnan(got).sum() == 2
    assert all(np.isnan(v) for v in ops.percentiles(_dev(x.reshape(-1)), [1.0, 99.0])) and np.isnan(np.percentile(x, 1.0))
    # [C,H,W] is refused, as everywhere else
    for key in ("minmax_none", "percentiles_1_99", "cwt_both", "cwtn_minmax_both", "gamma_always", "noise_always", "dual_plain"):
        with pytest.raises(ValueError):
            _make(cases[key])({"image": _dev(const[:, 0]), "image1": _dev(const[:, 0]), "label": _dev(lab[:, 0])})
