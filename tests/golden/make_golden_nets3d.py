"""Fixture generator for UNet2D5 / UNet3D / DeepSuperviseLoss (build container only: imports the reference).

Runs the REFERENCE classes on the CPU in fp32
  * pymic/net/net3d/unet2d5.py:144-211   UNet2D5
  * pymic/net/net3d/unet3d.py:81-160     UNet3D (with and without deep supervision)
  * pymic/loss/seg/deep_sup.py:7-41      DeepSuperviseLoss over pymic/loss/seg/dice.py DiceLoss
on the configs of nets3d_cfg.py and writes, per config, nets3d_<name>.npz:
  logitsub<s>_eval.<i> / logitsub<s>_train.<i>   every output's logits, flattened, every s-th element (nets3d_cfg.logit_stride)
  loss                                           DiceLoss, or DeepSuperviseLoss(DiceLoss) for a list of outputs
  stat.<key>                                     running statistics of three BatchNorm layers after ONE train-mode forward
  gradnorm_keys / gradnorm_vals                  every parameter that received a gradient, and its norm
  gradsub<s>.<key>                               gradients of selected parameters, every s-th element (nets3d_cfg.grad_stride)
and ref_state_keys_nets3d.json: the state_dict keys and shapes of the five networks, in the reference's order (no values).
"""
import copy
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_import  # noqa: E402

_ref_import.install()
torch.set_num_threads(8)

from pymic.net.net3d.unet2d5 import UNet2D5  # noqa: E402
from pymic.net.net3d.unet3d import UNet3D  # noqa: E402
from pymic.loss.seg.dice import DiceLoss  # noqa: E402
from pymic.loss.seg.deep_sup import DeepSuperviseLoss  # noqa: E402

import nets3d_cfg as C  # noqa: E402

CLASSES = {"UNet2D5": UNet2D5, "UNet3D": UNet3D}


def build(name, keys=None):
    params = copy.deepcopy(C.NETS[name])
    torch.manual_seed(1)
    net = CLASSES[params["net_type"]](params).float()
    if keys is None:
        keys = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    net.load_state_dict({k: torch.from_numpy(v) for k, v in C.weights_for(name, keys).items()}, strict=True)
    return net, keys


def grad_keys(keys):
    """a spread of parameters: every head, the stem, the deepest block, the first and last up-sampling members, the last
    decoder block, three BatchNorm layers and (UNet2D5) PReLU slopes"""
    names = [k for k, _ in keys if k.rsplit(".", 1)[1] in ("weight", "bias")]
    bn = [k.rsplit(".", 1)[0] for k, _ in keys if k.endswith("running_mean")]
    ups = sorted(set(k.split(".")[0] for k in names if k.startswith("up")))
    enc = [k.rsplit(".", 2)[0] for k in names if k.endswith("conv_conv.0.weight") and not k.startswith("up")]
    want = [k for k in names if k.startswith("out_conv")]
    want += [enc[0] + ".0.weight", enc[0] + ".0.bias", enc[1] + ".4.weight", enc[-1] + ".4.weight"]
    for u in (ups[0], ups[-1]):
        want += [k for k in names if k.startswith(u + ".") and ".conv.conv_conv." not in k]
    want += [ups[-1] + ".conv.conv_conv.0.weight", ups[-1] + ".conv.conv_conv.4.weight"]
    for b in (bn[0], bn[len(bn) // 2], bn[-1]):
        want += [b + ".weight", b + ".bias"]
    want += [k for k in (enc[0] + ".2.weight", enc[0] + ".6.weight", ups[1] + ".conv.conv_conv.2.weight") if k in names]
    return [k for k in dict.fromkeys(want) if k in names], (bn[0], bn[len(bn) // 2], bn[-1])


def as_list(out):
    return list(out) if isinstance(out, (list, tuple)) else [out]


def gen(name, all_keys):
    net, keys = build(name)
    all_keys[name] = [[k, list(s)] for k, s in keys]
    x = torch.from_numpy(C.input_for(name))
    y = torch.from_numpy(C.label_for(name))
    s = C.logit_stride(name)
    out = {"logit_stride": np.int64(s)}
    net.eval()
    with torch.no_grad():
        for i, o in enumerate(as_list(net(x))):
            out["logitsub%d_eval.%d" % (s, i)] = o.numpy().reshape(-1)[::s].copy()
    net, _ = build(name, keys)                       # fresh: the running statistics update once
    net.train()
    pred = net(x)
    for i, o in enumerate(as_list(pred)):
        out["logitsub%d_train.%d" % (s, i)] = o.detach().numpy().reshape(-1)[::s].copy()
    base = DiceLoss()
    d = {"prediction": pred, "ground_truth": y}
    if isinstance(pred, (list, tuple)):
        # the agent's construction (agent_seg.py:126-129): the weights it passes are not the key the class reads
        ds = DeepSuperviseLoss({"deep_supervise_weight": [1.0, 0.5, 0.25, 0.125], "base_loss": base})
        loss = ds(d)
        assert ds.deep_sup_weight == [1.0] * len(pred)
    else:
        loss = base(d)
    out["loss"] = np.float32(loss.item())
    loss.backward()
    gk, bns = grad_keys(keys)
    sd = net.state_dict()
    for b in bns:
        for t in ("running_mean", "running_var", "num_batches_tracked"):
            out["stat.%s.%s" % (b, t)] = sd["%s.%s" % (b, t)].numpy().copy()
    named = dict(net.named_parameters())
    norms = {k: float(p.grad.norm()) for k, p in named.items() if p.grad is not None}
    out["gradnorm_keys"] = np.array(sorted(norms))
    out["gradnorm_vals"] = np.array([norms[k] for k in sorted(norms)], np.float64)
    for k in gk:
        g = named[k].grad.numpy().reshape(-1)
        st = C.grad_stride(g.size)
        out["gradsub%d.%s" % (st, k)] = g[::st].copy()
    path = os.path.join(HERE, "nets3d_%s.npz" % name)
    np.savez_compressed(path, **out)
    print("nets3d", name, "ok: %d outputs, logit stride %d, loss %.6f, %d bytes" % (len(as_list(pred)), s, loss.item(),
                                                                                     os.path.getsize(path)))


if __name__ == "__main__":
    all_keys = {}
    for name in C.NAMES:
        gen(name, all_keys)
    with open(C.KEYS_JSON, "w") as f:
        json.dump(all_keys, f, indent=0, sort_keys=True)
        f.write("\n")
