"""Generates tests/golden/intensity.npz, intensity_cwtn.npz, intensity_gamma.npz, intensity_noise.npz and
intensity_chain.npz (each below 1 MiB) by RUNNING the reference's intensity transforms (PyMIC/pymic/transform/
{normalize,threshold,intensity}.py of the reference tree, imported with the stub modules of _ref_import.py) on the
deterministic volume of tests/intensity_ref.py:inputs().  Both generators (`random`, `numpy.random`) are seeded per case; the
host mirror (fplx/transform.py) draws from the same generators in the same order, and the next draw of both is stored so
that a test can see that they were left in the same state.

Stored besides the results: every case's class name and parameter dict (cases_json), whether a probability gate fired, the
gammas GammaCorrection drew (re-drawn here in the reference's order: numpy.random.uniform() for the gate, then one
random.random() per channel), the float64 evaluation of the gamma formula from the float32 inputs and the reference's own
maximum distance from it in units of one float32 ulp at max(|vmin|, |vmax|) (e_ref: numpy's float32 power is not correctly
rounded, so this is measured where the fixture is made, not assumed).
Build-container only; the GPU box reads the .npz."""
import json
import os
import random
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _ref_import  # noqa: E402

_ref_import.install()
warnings.filterwarnings("ignore", category=DeprecationWarning)
import intensity_ref as IR  # noqa: E402
from pymic.transform.trans_dict import TransformDict  # noqa: E402

SEEDS = [1, 2, 3, 5, 8]
T = "segmentation"

# ---- cases without a random draw: name -> (class, parameters)
PLAIN = {
    "minmax_none": ("NormalizeWithMinMax", {"normalizewithminmax_channels": None, "normalizewithminmax_threshold_lower": None,
                                            "normalizewithminmax_threshold_upper": None}),
    "minmax_given": ("NormalizeWithMinMax", {"normalizewithminmax_channels": [0, 1],
                                             "normalizewithminmax_threshold_lower": [-10.0, 0.1],
                                             "normalizewithminmax_threshold_upper": [250.0, 120.7]}),
    "minmax_mixed": ("NormalizeWithMinMax", {"normalizewithminmax_channels": [1, 0],
                                             "normalizewithminmax_threshold_lower": [None, -5.3],
                                             "normalizewithminmax_threshold_upper": [100.25, None]}),
    "percentiles_1_99": ("NormalizeWithPercentiles", {"normalizewithpercentiles_channels": None,
                                                      "normalizewithpercentiles_percentile_lower": 1.0,
                                                      "normalizewithpercentiles_percentile_upper": 99.0}),
    "percentiles_wide": ("NormalizeWithPercentiles", {"normalizewithpercentiles_channels": [0],
                                                      "normalizewithpercentiles_percentile_lower": 0.5,
                                                      "normalizewithpercentiles_percentile_upper": 99.9}),
    "percentiles_0_100": ("NormalizeWithPercentiles", {"normalizewithpercentiles_channels": [1],
                                                       "normalizewithpercentiles_percentile_lower": 0,
                                                       "normalizewithpercentiles_percentile_upper": 100}),
    "cwt_both": ("ChannelWiseThreshold", {"channelwisethreshold_channels": None,
                                          "channelwisethreshold_threshold_lower": [0.0, 10.3],
                                          "channelwisethreshold_threshold_upper": [200.0, 150.0],
                                          "channelwisethreshold_replace_lower": [None, -1.7],
                                          "channelwisethreshold_replace_upper": [255.0, None]}),
    "cwt_partial": ("ChannelWiseThreshold", {"channelwisethreshold_channels": [1, 0],
                                             "channelwisethreshold_threshold_lower": [None, 5.1],
                                             "channelwisethreshold_threshold_upper": [100.0, None],
                                             "channelwisethreshold_replace_lower": None,
                                             "channelwisethreshold_replace_upper": None}),
}
CWTN = {
    "cwtn_minmax_both": ("ChannelWiseThresholdWithNormalize", {
        "channelwisethresholdwithnormalize_channels": None,
        "channelwisethresholdwithnormalize_threshold_lower": [0.3, 10.0],
        "channelwisethresholdwithnormalize_threshold_upper": [200.0, 150.2],
        "channelwisethresholdwithnormalize_mean_std_mode": False}),
    # thresholds are indexed by the channel number: channel 0 -> (None, 220.4), channel 1 -> (5.0, None)
    "cwtn_minmax_partial": ("ChannelWiseThresholdWithNormalize", {
        "channelwisethresholdwithnormalize_channels": [1, 0],
        "channelwisethresholdwithnormalize_threshold_lower": [None, 5.0],
        "channelwisethresholdwithnormalize_threshold_upper": [220.4, None],
        "channelwisethresholdwithnormalize_mean_std_mode": False}),
    "dual_plain": ("NormalizeWithMeanStd_dual", {"normalizewithmeanstd_channels": None}),
    "dual_given": ("NormalizeWithMeanStd_dual", {"normalizewithmeanstd_channels": [1, 0], "normalizewithmeanstd_mean": [10.5, 20.0],
                                                 "normalizewithmeanstd_std": [50.0, 61.3]}),
}
# ---- seeded cases
CWTN_MEANSTD = ("ChannelWiseThresholdWithNormalize", {
    "channelwisethresholdwithnormalize_channels": None,
    "channelwisethresholdwithnormalize_threshold_lower": [0.3, 10.0],
    "channelwisethresholdwithnormalize_threshold_upper": [200.0, 150.2],
    "channelwisethresholdwithnormalize_mean_std_mode": True})
CWTN_MEANSTD_PARTIAL = ("ChannelWiseThresholdWithNormalize", {
    "channelwisethresholdwithnormalize_channels": [1, 0],
    "channelwisethresholdwithnormalize_threshold_lower": [None, 5.0],
    "channelwisethresholdwithnormalize_threshold_upper": [220.4, None],
    "channelwisethresholdwithnormalize_mean_std_mode": True})
DUAL_NP = ("NormalizeWithMeanStd_dual", {"normalizewithmeanstd_channels": None, "normalizewithmeanstd_ignore_non_positive": True})
GAMMA = {"gammacorrection_channels": [0, 1], "gammacorrection_gamma_min": 0.7, "gammacorrection_gamma_max": 1.5}
NOISE = {"gaussiannoise_channels": [1], "gaussiannoise_mean": 2.0, "gaussiannoise_std": 7.5}
CHAIN = {
    "normalizewithpercentiles_channels": None, "normalizewithpercentiles_percentile_lower": 1.0,
    "normalizewithpercentiles_percentile_upper": 99.0,
    "gammacorrection_channels": [0, 1], "gammacorrection_gamma_min": 0.7, "gammacorrection_gamma_max": 1.5,
    "gaussiannoise_channels": [0, 1], "gaussiannoise_mean": 0.0, "gaussiannoise_std": 0.05,
    "pad_output_size": [10, 32, 40], "pad_ceil_mode": False,
    "randomcrop_output_size": [6, 24, 24], "randomcrop_foreground_focus": False, "randomcrop_mask_label": None,
}
CHAIN_NAMES = ["NormalizeWithPercentiles", "GammaCorrection", "GaussianNoise", "Pad", "RandomCrop"]


def seed_all(seed):
    random.seed(seed)
    np.random.seed(seed)


def make(name, extra):
    p = {"task": T}
    p.update(json.loads(json.dumps(extra)))
    return TransformDict[name](p)


def fresh():
    img, img1, lab = IR.inputs()
    return {"image": img.copy(), "image1": img1.copy(), "label": lab.copy()}


def tail(out, key):
    out[key + "next_random"] = np.array(random.random())
    out[key + "next_np_random"] = np.array(np.random.uniform())


def gamma_draws(seed, p):
    """the reference's draws, in its order"""
    seed_all(seed)
    if np.random.uniform() > p.get("gammacorrection_probability", 0.5):
        return False, []
    return True, [random.random() * (p["gammacorrection_gamma_max"] - p["gammacorrection_gamma_min"]) +
                  p["gammacorrection_gamma_min"] for _ in p["gammacorrection_channels"]]


def gamma_case(out, key, seed, p):
    img = IR.inputs()[0]
    fired, gammas = gamma_draws(seed, p)
    seed_all(seed)
    with np.errstate(invalid="ignore"):
        s = make("GammaCorrection", p)(fresh())
    assert s["image"].dtype == np.float32
    out[key + "image"] = s["image"]
    out[key + "fired"] = np.array(fired)
    out[key + "gammas"] = np.array(gammas, np.float64)
    tail(out, key)
    assert fired == (not np.array_equal(s["image"], img))
    e_ref = 0.0
    if fired:
        f64 = np.stack([IR.gamma_f64(img[c], g) for c, g in zip(p["gammacorrection_channels"], gammas)])
        out[key + "f64"] = f64
        for c, g in zip(p["gammacorrection_channels"], gammas):
            e_ref = max(e_ref, IR.gamma_error_units(s["image"][c], img[c], g))
        assert e_ref < 8.0, e_ref                           # the re-drawn gammas are the ones the reference used
    out[key + "e_ref"] = np.array(e_ref)
    return fired, gammas, e_ref


def main():
    img, img1, lab = IR.inputs()
    cases = {}
    plain = {"image": img, "image1": img1, "label": lab}
    cwtn, gam, noi, chain = {}, {}, {}, {}
    for group, out in ((PLAIN, plain), (CWTN, cwtn)):
        for key, (name, p) in group.items():
            cases[key] = [name, p]
            with np.errstate(invalid="ignore", divide="ignore"):
                s = make(name, p)(fresh())
            assert s["image"].dtype == np.float32 and np.array_equal(s["label"], lab)
            out[key + "_image"] = s["image"]
            if name.endswith("_dual"):
                out[key + "_image1"] = s["image1"]
            else:
                assert np.array_equal(s["image1"], img1)
    # ---- seeded: mean-std mode of ChannelWiseThresholdWithNormalize (host normal draw for every channel)
    cases["cwtn_meanstd"], cases["cwtn_meanstd_partial"], cases["dual_np"] = CWTN_MEANSTD, CWTN_MEANSTD_PARTIAL, DUAL_NP
    for seed in SEEDS[:3]:
        seed_all(seed)
        k = "seed%d_cwtn_meanstd_" % seed
        cwtn[k + "image"] = make(*CWTN_MEANSTD)(fresh())["image"]
        tail(cwtn, k)
    seed_all(SEEDS[0])
    cwtn["cwtn_meanstd_partial_image"] = make(*CWTN_MEANSTD_PARTIAL)(fresh())["image"]
    tail(cwtn, "cwtn_meanstd_partial_")
    seed_all(SEEDS[0])
    s = make(*DUAL_NP)(fresh())
    noi["dual_np_image"], noi["dual_np_image1"] = s["image"], s["image1"]
    tail(noi, "dual_np_")
    # ---- gamma: the default gate on every seed, and gates that always / never fire
    cases["gamma"] = ["GammaCorrection", GAMMA]
    cases["gamma_always"] = ["GammaCorrection", dict(GAMMA, gammacorrection_probability=1.0, gammacorrection_channels=[1])]
    cases["gamma_never"] = ["GammaCorrection", dict(GAMMA, gammacorrection_probability=0.0)]
    report = []
    for seed in SEEDS:
        report.append(("gamma", seed) + gamma_case(gam, "seed%d_gamma_" % seed, seed, cases["gamma"][1]))
    report.append(("gamma_always", SEEDS[0]) + gamma_case(gam, "gamma_always_", SEEDS[0], cases["gamma_always"][1]))
    report.append(("gamma_never", SEEDS[0]) + gamma_case(gam, "gamma_never_", SEEDS[0], cases["gamma_never"][1]))
    gam["e_ref_max"] = np.array(max(r[4] for r in report))
    # ---- noise (host float64 draw)
    cases["noise"] = ["GaussianNoise", NOISE]
    cases["noise_always"] = ["GaussianNoise", dict(NOISE, gaussiannoise_probability=1.0, gaussiannoise_channels=[0, 1])]
    cases["noise_never"] = ["GaussianNoise", dict(NOISE, gaussiannoise_probability=0.0)]
    for key, seed, name in [("seed%d_noise_" % s_, s_, "noise") for s_ in SEEDS] + [("noise_always_", SEEDS[0], "noise_always"),
                                                                                  ("noise_never_", SEEDS[0], "noise_never")]:
        seed_all(seed)
        s = make("GaussianNoise", cases[name][1])(fresh())
        assert s["image"].dtype == np.float32
        fired = not np.array_equal(s["image"], img)
        noi[key + "fired"] = np.array(fired)
        if fired:
            noi[key + "image"] = s["image"]
        tail(noi, key)
        report.append((name, seed, fired))
    # ---- chain, stage by stage for the gamma stage's own e_ref
    cases["chain"] = [CHAIN_NAMES, CHAIN]
    for seed in SEEDS:
        k = "seed%d_chain_" % seed
        seed_all(seed)
        s = {"image": img.copy(), "label": lab.copy()}
        ts = [make(n, CHAIN) for n in CHAIN_NAMES]
        s = ts[0](s)
        before = s["image"].copy()
        state = (random.getstate(), np.random.get_state())
        fired = not (np.random.uniform() > 0.5)
        gammas = [random.random() * (1.5 - 0.7) + 0.7 for _ in (0, 1)] if fired else []
        random.setstate(state[0])
        np.random.set_state(state[1])
        s = ts[1](s)
        assert fired == (not np.array_equal(before, s["image"]))
        e_ref = max([IR.gamma_error_units(s["image"][c], before[c], g) for c, g in zip((0, 1), gammas)] + [0.0])
        assert e_ref < 8.0
        for t in ts[2:]:
            s = t(s)
        chain[k + "image"], chain[k + "label"] = s["image"], s["label"]
        chain[k + "Pad_Param"], chain[k + "RandomCrop_Param"] = np.array(s["Pad_Param"]), np.array(s["RandomCrop_Param"])
        chain[k + "gamma_fired"], chain[k + "gammas"], chain[k + "e_ref"] = np.array(fired), np.array(gammas), np.array(e_ref)
        chain[k + "gamma_unit"] = np.array(max(IR.ulp_unit(before[c].min(), before[c].max()) for c in (0, 1)))
        tail(chain, k)
        report.append(("chain", seed, fired, gammas, e_ref))
    plain["cases_json"] = np.array(json.dumps(cases))
    plain["seeds"] = np.array(SEEDS)
    for name, arrays in (("intensity.npz", plain), ("intensity_cwtn.npz", cwtn), ("intensity_gamma.npz", gam),
                         ("intensity_noise.npz", noi), ("intensity_chain.npz", chain)):
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **arrays)
        print("%s: %d arrays, %d bytes" % (path, len(arrays), os.path.getsize(path)))
        assert os.path.getsize(path) < (1 << 20)
    for r in report:
        print(r)
    print("e_ref_max", float(gam["e_ref_max"]))


if __name__ == "__main__":
    main()
