"""Generates tests/golden/resample.npz, resample_chain.npz and resample_inverse.npz (each below 1 MiB) by RUNNING the
reference's geometric transforms (/root/reference/PyMIC/pymic/transform/{rotate,rescale}.py on top of scipy.ndimage.rotate / zoom, imported with the stub
modules of _ref_import.py) on deterministic inputs.  Both generators are seeded per case: RandomRotate draws its angles
from numpy's global generator, RandomRescale its ratios from Python's `random`, and the host mirror (fplx/transform.py)
draws from the same generators in the same order.  Stored per seed: every transform alone, one chain
[RandomRotate, RandomRescale, Pad, RandomCrop], the parameter strings, the next draw of both generators (the draw order
leaves them in the same state) and, in resample_inverse.npz, the three inverse_transform_for_prediction results on
predictions that prediction() regenerates from their names.
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
import _ref_import  # noqa: E402

_ref_import.install()
warnings.filterwarnings("ignore", category=DeprecationWarning)
import detdata  # noqa: E402
from resample_ref import prediction  # noqa: E402
from pymic.transform.rotate import RandomRotate  # noqa: E402
from pymic.transform.rescale import Rescale, RandomRescale  # noqa: E402
from pymic.transform.pad import Pad  # noqa: E402
from pymic.transform.crop import RandomCrop  # noqa: E402

SHAPE = (10, 32, 40)           # every stored fp32 result is incompressible: sized so that each .npz stays below 1 MiB
SEEDS = [1, 2, 3, 5, 8]
PARAMS = {
    "task": "segmentation",
    "randomrotate_angle_range_d": [-30, 30], "randomrotate_angle_range_h": [-10, 10],
    "randomrotate_angle_range_w": [-10, 10],
    "randomrescale_lower_bound": [0.8, 0.85, 0.85], "randomrescale_upper_bound": [1.25, 1.2, 1.2],
    "rescale_output_size": [13, 37, 36],
    "pad_output_size": [12, 40, 48], "pad_ceil_mode": False,
    "randomcrop_output_size": [8, 24, 24], "randomcrop_foreground_focus": True, "randomcrop_foreground_ratio": 0.5,
    "randomcrop_mask_label": [1],
}
# variants: a single rotation plane; scalar rescale bounds; Rescale with a leading None and with an int
ROTATE_D_ONLY = {"randomrotate_angle_range_d": [-30, 30], "randomrotate_angle_range_h": None,
                 "randomrotate_angle_range_w": None}
RANDOMRESCALE_SCALAR = {"randomrescale_lower_bound": 0.8, "randomrescale_upper_bound": 1.3}
RESCALE_NONE = {"rescale_output_size": [None, 27, 48]}
RESCALE_INT = {"rescale_output_size": 13}


def params(extra=None):
    p = json.loads(json.dumps(PARAMS))
    p.update(extra or {})
    return p


def inputs():
    img = (detdata.normal("rs.image", (1,) + SHAPE) * 37.0 + 210.0).astype(np.float32)
    zz, yy, xx = np.meshgrid(np.arange(SHAPE[0]), np.arange(SHAPE[1]), np.arange(SHAPE[2]), indexing="ij")
    lab = (((zz - 5) ** 2 * 6 + (yy - 17) ** 2 + (xx - 22) ** 2 * 0.6) < 100).astype(np.uint8)[None]
    pw = (blocks("rs.pw") > 0.3).astype(np.float32)[None] * 0.73
    return img, lab, pw


def blocks(name):
    """a piecewise-constant uniform field (2 x 4 x 4 blocks): thresholded, its resampled versions compress"""
    b = detdata.uniform(name, (SHAPE[0] // 2, SHAPE[1] // 4, SHAPE[2] // 4))
    return b.repeat(2, 0).repeat(4, 1).repeat(4, 2)


def seed_all(seed):
    random.seed(seed)
    np.random.seed(seed)


def run(out, key, transforms, sample, param_keys):
    for t in transforms:
        sample = t(sample)
    for k in ("image", "label", "pixel_weight"):
        out[key + k] = sample[k]
    for k in param_keys:
        out[key + k] = np.array(sample[k])
    out[key + "next_random"] = np.array(random.random())
    out[key + "next_np_random"] = np.array(np.random.uniform())
    return sample


def main():
    img, lab, pw = inputs()
    pred = prediction("rs.predict", SHAPE)
    inv = {"predict": pred}
    chain = {}
    out = {"image": img, "label": lab, "pixel_weight": pw, "params_json": np.array(json.dumps(PARAMS)),
           "variants_json": np.array(json.dumps({"rotate_d": ROTATE_D_ONLY, "randomrescale_scalar": RANDOMRESCALE_SCALAR,
                                                  "rescale_none": RESCALE_NONE, "rescale_int": RESCALE_INT})),
           "seeds": np.array(SEEDS)}
    fresh = lambda: {"image": img.copy(), "label": lab.copy(), "pixel_weight": pw.copy()}
    for seed in SEEDS:
        k = "seed%d_" % seed
        seed_all(seed)
        s = run(out, k + "rotate_", [RandomRotate(params())], fresh(), ["RandomRotate_Param"])
        s["predict"] = pred.copy()
        inv[k + "rotate_inverse"] = RandomRotate(params()).inverse_transform_for_prediction(s)["predict"]
        seed_all(seed)
        s = run(out, k + "randomrescale_", [RandomRescale(params())], fresh(), ["RandomRescale_origin_shape"])
        # the prediction of a rescaled sample has the rescaled extents: zoom the stored one forward first
        # the prediction of a rescaled sample has the rescaled extents; tests regenerate it with prediction()
        s["predict"] = prediction("rs.predict.%d" % seed, s["image"].shape[1:])
        inv[k + "randomrescale_inverse"] = RandomRescale(params()).inverse_transform_for_prediction(s)["predict"]
        seed_all(seed)
        run(chain, k + "chain_", [RandomRotate(params()), RandomRescale(params()), Pad(params()), RandomCrop(params())], fresh(),
            ["RandomRotate_Param", "RandomRescale_origin_shape", "Pad_Param", "RandomCrop_Param"])
    seed = SEEDS[0]
    seed_all(seed)
    run(out, "rotate_d_", [RandomRotate(params(ROTATE_D_ONLY))], fresh(), ["RandomRotate_Param"])
    seed_all(seed)
    run(out, "randomrescale_scalar_", [RandomRescale(params(RANDOMRESCALE_SCALAR))], fresh(), ["RandomRescale_origin_shape"])
    for name, extra in (("rescale_list_", None), ("rescale_none_", RESCALE_NONE), ("rescale_int_", RESCALE_INT)):
        seed_all(seed)
        s = run(out, name, [Rescale(params(extra))], fresh(), ["Rescale_origin_shape"])
        if name == "rescale_list_":
            s["predict"] = prediction("rs.predict.rescale", s["image"].shape[1:])
            inv["rescale_inverse"] = Rescale(params()).inverse_transform_for_prediction(s)["predict"]
    for name, arrays in (("resample.npz", out), ("resample_chain.npz", chain), ("resample_inverse.npz", inv)):
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **arrays)
        print("%s: %d arrays, %d bytes" % (path, len(arrays), os.path.getsize(path)))
        assert os.path.getsize(path) < (1 << 20)
    for seed in SEEDS:
        print(seed, out["seed%d_rotate_RandomRotate_Param" % seed], out["seed%d_randomrescale_image" % seed].shape)


if __name__ == "__main__":
    main()
