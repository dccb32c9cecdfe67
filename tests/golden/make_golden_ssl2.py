#!/usr/bin/env python3
"""Generate tests/golden/ssl2_steps.npz by RUNNING THE REFERENCE's URPC and CPS training loops on the CPU (float32), as
make_golden_nll.py does for the noisy-label loops.  Build container only:

    python tests/golden/make_golden_ssl2.py

What is executed from the reference: pymic/net_run_ssl/ssl_urpc.py SSLURPC.training and ssl_cps.py SSLCPS.training as
published, one iteration each, on an `object.__new__` stub of the agent whose `net` returns its own parameters as the logits of
the joint batch (so the recorded `.grad` IS d loss / d logits - the gradient that enters the network's last layer), whose
loaders are one-element lists and whose `optimizer.step()` records the gradients.  The supervised loss is the reference's
DiceLoss, through its DeepSuperviseLoss for URPC's four outputs.
Recorded per case: the logits of every output / network, the label, glob_it, the returned scalars and the logit gradients.
Inputs: tests/pyramidoracle.py logits_case with the keys below.  Every CPS case is asserted to have no voxel whose argmax of
the fp32 softmax differs from the argmax of the logits (the one deliberate difference of fplx_ssl_pseudo_onehot)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))                        # tests/: pyramidoracle
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))       # the repository root: oracle/
import _ref_import  # noqa: E402

_ref_import.install()
torch.set_num_threads(8)

from pymic.net_run_ssl.ssl_urpc import SSLURPC  # noqa: E402
from pymic.net_run_ssl.ssl_cps import SSLCPS  # noqa: E402
from pymic.loss.seg.dice import DiceLoss  # noqa: E402
from pymic.loss.seg.deep_sup import DeepSuperviseLoss  # noqa: E402
from pymic.util.ramps import get_rampup_ratio  # noqa: E402

import detdata  # noqa: E402
import pyramidoracle as PO  # noqa: E402

# (n0 labelled rows, n1 unlabelled rows, C, D, H, W)
SHAPES = {"a": (1, 2, 3, 2, 5, 7), "b": (1, 1, 2, 3, 4, 8)}
ITER_MAX, REG_W = 10, 0.1
GLOB_ITS = {"mid": 5, "end": 10}
METHODS = {"URPC": (SSLURPC, 4), "CPS": (SSLCPS, 2)}


def label_for(tag, n0, c, spatial):
    idx = (detdata.uniform("golden.ssl2.label." + tag, (n0,) + spatial, 0.0, 1.0) * c).astype(np.int64).clip(0, c - 1)
    return np.ascontiguousarray(np.moveaxis(np.eye(c, dtype=np.float32)[idx], -1, 1))


def run(method, logits, y, n0, glob_it):
    cls, k = METHODS[method]
    params = [torch.nn.Parameter(torch.from_numpy(l).clone()) for l in logits]
    rec = {}

    class Net(object):
        def train(self):
            pass

        def __call__(self, x):
            return list(params) if method == "URPC" else tuple(params)

    class Opt(object):
        def zero_grad(self):
            for p in params:
                p.grad = None

        def step(self):
            rec["grads"] = [p.grad.numpy().copy() for p in params]

    n = logits[0].shape[0]
    spatial = tuple(logits[0].shape[2:])
    lab = {'image': torch.zeros((n0, 1) + spatial), 'label_prob': torch.from_numpy(y).clone()}
    unlab = {'image': torch.zeros((n - n0, 1) + spatial)}
    agent = object.__new__(cls)
    agent.config = {'network': {'class_num': y.shape[1]}, 'training': {'iter_valid': 1, 'iter_max': ITER_MAX},
                    'semi_supervised_learning': {'regularize_w': REG_W, 'rampup_start': 0, 'rampup_end': ITER_MAX}}
    agent.net, agent.optimizer, agent.scheduler = Net(), Opt(), None
    agent.glob_it, agent.device, agent.tensor_type = glob_it, torch.device("cpu"), 'float'
    agent.train_loader, agent.train_loader_unlab = [lab], [unlab]
    agent.trainIter, agent.trainIter_unlab = iter(agent.train_loader), iter(agent.train_loader_unlab)
    base = DiceLoss({'loss_softmax': True})
    agent.loss_calculator = DeepSuperviseLoss({'deep_supervise_weight': None, 'base_loss': base}) if method == "URPC" else base
    scalars = agent.training()
    return scalars, rec["grads"]


def main():
    out = {}
    for method, (_, k) in METHODS.items():
        for sname, (n0, n1, c, d, h, w) in SHAPES.items():
            for gname, glob_it in GLOB_ITS.items():
                tag = "%s.%s.%s" % (method, sname, gname)
                v = d * h * w
                logits = PO.logits_case("golden.ssl2." + tag, k, n0 + n1, c, v).reshape(k, n0 + n1, c, d, h, w)
                y = label_for(tag, n0, c, (d, h, w))
                scalars, grads = run(method, list(logits), y, n0, glob_it)
                regular_w = REG_W * get_rampup_ratio(glob_it, 0, ITER_MAX, "sigmoid")
                assert scalars['regular_w'] == regular_w, (scalars['regular_w'], regular_w)
                if method == "CPS":
                    soft = torch.softmax(torch.from_numpy(logits[:, n0:]), dim=2).numpy()
                    assert np.array_equal(soft.argmax(2), logits[:, n0:].argmax(2)), tag
                    names = ("loss", "loss_sup1", "loss_sup2", "loss_pse_sup1", "loss_pse_sup2", "avg_dice")
                else:
                    names = ("loss", "loss_sup", "loss_reg", "avg_dice")
                out[tag + ".label"] = y
                out[tag + ".n0"] = np.int64(n0)
                out[tag + ".glob_it"] = np.int64(glob_it)
                out[tag + ".regular_w"] = np.float64(regular_w)
                for j in range(k):
                    out[tag + ".logits%d" % (j + 1)] = logits[j]
                    out[tag + ".dlogits%d" % (j + 1)] = grads[j]
                    assert np.isfinite(grads[j]).all() and np.abs(grads[j]).max() > 0, tag
                for name in names:
                    out[tag + "." + name] = np.float64(scalars[name])
                out[tag + ".class_dice"] = np.asarray(scalars["class_dice"], np.float64)
                print("  %-14s " % tag + "  ".join("%s %.8g" % (nm, scalars[nm]) for nm in names))
    out["iter_max"] = np.int64(ITER_MAX)
    out["regularize_w"] = np.float64(REG_W)
    path = os.path.join(HERE, "ssl2_steps.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < (1 << 20), path
    print("ssl2_steps.npz ok: %d arrays, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
