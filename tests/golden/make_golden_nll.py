#!/usr/bin/env python3
"""Generate tests/golden/nll_steps.npz by RUNNING THE REFERENCE's noisy-label training loops on the CPU (float32), as
make_golden_wsl.py does for the weakly-supervised losses.  Build container only:

    python tests/golden/make_golden_nll.py

What is executed from the reference: pymic/net_run_nll/nll_co_teaching.py NLLCoTeaching.training and nll_trinet.py
NLLTriNet.training as published, one iteration each, on an `object.__new__` stub of the agent whose `net` returns its own
parameters as the logits (so the recorded `.grad` IS d loss / d logits) and whose `optimizer.step()` records them.
Recorded per case: the logits, the label, glob_it, iter_max, the ratio, the returned scalars and the logit gradients.
Inputs: tests/nlloracle.py logits_case with the keys below.  Each CoTeaching case is asserted to have
s[num_remb - 1] < s[num_remb] for both networks (only then is the reference's unstable argsort determined), and every case
to have no voxel within rounding reach of its threshold."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))                        # tests/: nlloracle
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))       # the repository root: oracle/
import _ref_import  # noqa: E402

_ref_import.install()
torch.set_num_threads(8)

from pymic.net_run_nll.nll_co_teaching import NLLCoTeaching  # noqa: E402
from pymic.net_run_nll.nll_trinet import NLLTriNet  # noqa: E402
from pymic.util.ramps import get_rampup_ratio  # noqa: E402

import nlloracle as NO  # noqa: E402

SHAPES = {"a": (2, 3, 2, 5, 7), "b": (1, 2, 3, 4, 8)}
RATIO, ITER_MAX = 0.6, 10
GLOB_ITS = {"mid": 5, "start": 0}
METHODS = {"CoTeaching": (NLLCoTeaching, 2, 'co_teaching_select_ratio', "sigmoid"),
           "TriNet": (NLLTriNet, 3, 'trinet_select_ratio', "linear")}


def run(method, logits, y, glob_it):
    cls, k, key, _ = METHODS[method]
    params = [torch.nn.Parameter(torch.from_numpy(l).clone()) for l in logits]
    rec = {}

    class Net(object):
        def train(self):
            pass

        def __call__(self, x):
            return tuple(params)

    class Opt(object):
        def zero_grad(self):
            for p in params:
                p.grad = None

        def step(self):
            rec["grads"] = [p.grad.numpy().copy() for p in params]

    batch = {'image': torch.zeros((y.shape[0], 1) + tuple(y.shape[2:])), 'label_prob': torch.from_numpy(y).clone()}
    agent = object.__new__(cls)
    agent.config = {'network': {'class_num': y.shape[1]}, 'training': {'iter_valid': 1, 'iter_max': ITER_MAX},
                    'noisy_label_learning': {key: RATIO, 'rampup_start': 0, 'rampup_end': ITER_MAX}}
    agent.net, agent.optimizer, agent.scheduler = Net(), Opt(), None
    agent.glob_it, agent.device, agent.tensor_type = glob_it, torch.device("cpu"), 'float'
    agent.train_loader = [batch]
    agent.trainIter = iter(agent.train_loader)
    scalars = agent.training()
    return scalars, rec["grads"]


def main():
    out = {}
    for method, (_, k, _, ramp_mode) in METHODS.items():
        for sname, shape in SHAPES.items():
            for gname, glob_it in GLOB_ITS.items():
                tag = "%s.%s.%s" % (method, sname, gname)
                logits, y = NO.logits_case("golden.nll." + tag, k, *shape)
                scalars, grads = run(method, logits, y, glob_it)
                remb = 1 - (1 - RATIO) * get_rampup_ratio(glob_it, 0, ITER_MAX, ramp_mode)
                assert scalars['select_ratio'] == remb, (scalars['select_ratio'], remb)
                r = NO.node(logits, y, method, remb)
                assert r.undecided == 0, (tag, r.undecided)
                if method == "CoTeaching":
                    nr = NO.num_remb_of(remb, r.refs[0].L.size)
                    y3 = y.reshape(shape[0], shape[1], -1)
                    for l in logits:                       # on the fp32 losses, as the reference sorts them
                        s = np.sort(NO.ce_fp32(l.reshape(y3.shape), y3)[0])
                        assert nr == s.size or s[nr - 1] < s[nr], tag
                out[tag + ".label"] = y
                out[tag + ".glob_it"] = np.int64(glob_it)
                out[tag + ".ratio"] = np.float64(remb)
                for j in range(k):
                    out[tag + ".logits%d" % (j + 1)] = logits[j]
                    out[tag + ".dlogits%d" % (j + 1)] = grads[j]
                    assert np.isfinite(grads[j]).all(), tag
                for name in ("loss", "loss1", "loss2", "loss_no_select1", "loss_no_select2", "avg_dice"):
                    out[tag + "." + name] = np.float64(scalars[name])
                out[tag + ".class_dice"] = np.asarray(scalars["class_dice"], np.float64)
                print("  %-24s loss %.8g  loss1 %.8g  loss2 %.8g  ratio %.6f" % (tag, scalars["loss"], scalars["loss1"],
                                                                                  scalars["loss2"], remb))
    out["iter_max"] = np.int64(ITER_MAX)
    out["select_ratio"] = np.float64(RATIO)
    path = os.path.join(HERE, "nll_steps.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < (1 << 20), path
    print("nll_steps.npz ok: %d arrays, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
