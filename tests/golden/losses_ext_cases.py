"""Inputs and case list of tests/golden/losses_ext.npz, shared by its generator (make_golden_losses_ext.py) and its tests.

The inputs are regenerated from detdata wherever they are needed; the archive holds what the reference made of them (value and
dlogits per case and shape) and the softmax outputs the `loss_softmax = False` cases take as predictions."""
import numpy as np

import detdata

SHAPES = {
    "a": (2, 2, 5, 30, 31),      # V = 4650: two partial rows, V no multiple of 256 or 4
    "b": (1, 3, 3, 7, 13),       # V = 273
    "c": (2, 8, 2, 16, 16),      # the largest C
    "d": (3, 4, 1, 1, 257),      # one voxel past a block
}

PARAMS = {
    "focaldiceloss_beta": 2.0,
    "noiserobustdiceloss_gamma": 1.5,
    "explogloss_w_dice": 0.8,
    "explogloss_gamma": 0.3,
    "loss_gce_q": 0.7,
    "slsrloss_epsilon": 0.25,
}

MIX = {"loss_type": ["DiceLoss", "NoiseRobustDiceLoss", "GeneralizedCELoss"], "loss_weight": [0.5, 0.3, 0.2]}

# tag -> (loss_type, loss_softmax, with pixel_weight)
CASES = {
    "focal": ("FocalDiceLoss", True, False),
    "nr": ("NoiseRobustDiceLoss", True, False),
    "explog": ("ExpLogLoss", True, False),
    "gce": ("GeneralizedCELoss", True, False),
    "mae": ("MAELoss", True, False),
    "mse": ("MSELoss", True, False),
    "slsr": ("SLSRLoss", True, False),
    "slsr_mask": ("SLSRLoss", True, True),
    "nr_nosm": ("NoiseRobustDiceLoss", False, False),
    "gce_nosm": ("GeneralizedCELoss", False, False),
    "mix": (MIX["loss_type"], True, False),
    "mix_pw": (MIX["loss_type"], True, True),
}


def inputs(skey):
    """-> logits, one-hot label [N, C, D, H, W], pixel_weight [N, 1, D, H, W] (a 0 / 1 mask times a per-image weight)"""
    shape = SHAPES[skey]
    n, c = shape[0], shape[1]
    logits = detdata.normal("loss_ext.logits." + skey, shape, scale=2.0)
    idx = (detdata.uniform("loss_ext.label." + skey, (n,) + shape[2:]) * c).astype(np.int64).clip(0, c - 1)
    label = np.ascontiguousarray(np.moveaxis(np.eye(c, dtype=np.float32)[idx], -1, 1))
    mask = (detdata.uniform("loss_ext.pw." + skey, (n, 1) + shape[2:]) > 0.3).astype(np.float32)
    iw = np.linspace(0.37, 0.93, n).astype(np.float32)
    return logits, label, mask * iw[:, None, None, None, None]


def config(tag):
    """the `params` dictionary of a case, keys lower-cased as the config parser delivers them"""
    name, softmax, _ = CASES[tag]
    cfg = dict(PARAMS)
    cfg["loss_type"] = name
    cfg["loss_softmax"] = softmax
    if isinstance(name, list):
        cfg["loss_weight"] = list(MIX["loss_weight"])
    return cfg


def load(golden_dir):
    """both archives as one dictionary"""
    import os
    out = {}
    for fname in ("losses_ext.npz", "losses_ext_a.npz"):
        with np.load(os.path.join(golden_dir, fname)) as z:
            out.update({k: z[k] for k in z.files})
    return out
