"""Configs, input shapes, labels and deterministic weights of the UNet2D5 / UNet3D parity fixtures - shared by the fixture
generator (make_golden_nets3d.py, imports the reference) and the tests (no reference).  No weights are stored: every tensor
is drawn by its state_dict key (detdata), given the key list and shapes of ref_state_keys_nets3d.json."""
import json
import os

import numpy as np

import detdata

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS_JSON = os.path.join(HERE, "ref_state_keys_nets3d.json")

_FT5 = [8, 16, 32, 64, 128]
# all with dropout 0: the reference draws its masks from torch's global generator, which nothing else can replay
NETS = {
    "u25": dict(net_type="UNet2D5", in_chns=1, feature_chns=_FT5, dropout=[0, 0, 0, 0, 0], conv_dims=[2, 2, 3, 3, 3],
                class_num=2, bilinear=False),
    "u25bl3": dict(net_type="UNet2D5", in_chns=4, feature_chns=_FT5, dropout=[0, 0, 0, 0, 0], conv_dims=[3, 3, 3, 3, 3],
                   class_num=3, bilinear=True),
    "u3d": dict(net_type="UNet3D", in_chns=1, feature_chns=_FT5, dropout=[0, 0, 0, 0, 0], class_num=2, trilinear=False,
                deep_supervise=False),
    "u3dtri_ds": dict(net_type="UNet3D", in_chns=1, feature_chns=_FT5, dropout=[0, 0, 0, 0, 0], class_num=2, trilinear=True,
                      deep_supervise=True),
    "u3d4_ds": dict(net_type="UNet3D", in_chns=1, feature_chns=[8, 16, 32, 64], dropout=[0, 0, 0, 0], class_num=3,
                    trilinear=False, deep_supervise=True),
}
SHAPES = {"u25": (2, 1, 16, 32, 32), "u25bl3": (2, 4, 16, 32, 32), "u3d": (2, 1, 16, 32, 32), "u3dtri_ds": (2, 1, 16, 32, 32),
          "u3d4_ds": (2, 1, 16, 16, 16)}
NAMES = list(NETS)
MAX_LOGIT_FLOATS = 140000      # per fixture file: logits are stored as a strided sample (odd stride: every w, h, d phase is hit)
MAX_GRAD_FLOATS = 8000         # per gradient tensor


def input_for(name):
    return detdata.normal("x.nets3d." + name, SHAPES[name])


def label_for(name):
    n, _, D, H, W = SHAPES[name]
    cls = NETS[name]["class_num"]
    lab = detdata.ball_label((D, H, W), radius=min(D, H, W) / 4.0, n=n, class_num=2, offsets=[(0, 1, -2), (1, -3, 2)][:n])
    if cls == 3:                # split the ball into two classes by x
        out = np.zeros((n, 3, D, H, W), np.float32)
        half = np.zeros((D, H, W), bool)
        half[:, :, W // 2:] = True
        out[:, 0], out[:, 1], out[:, 2] = lab[:, 0], lab[:, 1] * half, lab[:, 1] * (~half)
        lab = out
    return lab


def n_outputs(name):
    return 4 if NETS[name].get("deep_supervise", False) else 1


def logit_stride(name):
    """smallest odd stride that keeps the file's logit samples (eval and train, every output) under MAX_LOGIT_FLOATS"""
    n, _, D, H, W = SHAPES[name]
    total = 2 * n_outputs(name) * n * NETS[name]["class_num"] * D * H * W
    s = 1
    while total // s > MAX_LOGIT_FLOATS:
        s += 2
    return s


def grad_stride(size):
    return max(1, -(-size // MAX_GRAD_FLOATS))


def key_shapes(name):
    with open(KEYS_JSON) as f:
        return [(k, tuple(s)) for k, s in json.load(f)[name]]


def weights_for(name, keys=None):
    """{state_dict key: np.ndarray}: convolutions He-scaled, BatchNorm affine near (1, 0), running statistics away from (0, 1)
    with positive variances, PReLU slopes in (0.1, 0.4)"""
    keys = key_shapes(name) if keys is None else keys
    have = set(k for k, _ in keys)
    sd = {}
    for k, shp in keys:
        tag = "w.%s.%s" % (name, k)
        stem, leaf = k.rsplit(".", 1)
        is_bn = (stem + ".running_mean") in have
        if leaf == "num_batches_tracked":
            sd[k] = np.zeros((), np.int64)
        elif leaf == "running_mean":
            sd[k] = detdata.normal(tag, shp, 0.2)
        elif leaf == "running_var":
            sd[k] = detdata.uniform(tag, shp, 0.5, 1.5)
        elif is_bn:
            sd[k] = detdata.normal(tag, shp, 0.2, 1.0 if leaf == "weight" else 0.0)
        elif leaf == "weight" and len(shp) == 1:                     # PReLU
            sd[k] = detdata.uniform(tag, shp, 0.1, 0.4)
        elif leaf == "weight":
            transposed = ".up." in ("." + k) and not NETS[name].get("bilinear", False) and not NETS[name].get("trilinear", False) \
                and ".conv." not in k
            fan_in = shp[0] if transposed else shp[1] * int(np.prod(shp[2:]))
            sd[k] = detdata.normal(tag, shp, ((1.0 if transposed else 2.0) / fan_in) ** 0.5)
        else:
            sd[k] = detdata.normal(tag, shp, 0.1)
    return sd
