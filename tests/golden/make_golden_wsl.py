#!/usr/bin/env python3
"""Generate tests/golden/wsl_losses.npz by RUNNING THE REFERENCE's weakly-supervised loss classes on the CPU (float32, value and
dlogits by autograd), as make_golden_losses_ext.py does for the segmentation losses.  Build container only:

    python tests/golden/make_golden_wsl.py

What is executed from the reference (reference paths): pymic/loss/seg/gatedcrf.py GatedCRFLoss as published, called as
net_run_wsl/wsl_gatedcrf.py:80-93 calls it (softmax, transpose + reshape to slices, {'rgb': inputs}); pymic/loss/seg/
mumford_shah.py MumfordShahLoss with its missing `softmax` attribute set on the instance, both penalties;
pymic/loss/seg/ssl.py:57-86 TotalVariationLoss.forward called on a plain object carrying `softmax` (the class cannot be
constructed under a current torch).  Inputs: tests/wsloracle.py logits_case with the keys below."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))                        # tests/: wsloracle
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))       # the repository root: oracle/
import _ref_import  # noqa: E402

_ref_import.install()
torch.set_num_threads(8)

from pymic.loss.seg.gatedcrf import GatedCRFLoss  # noqa: E402
from pymic.loss.seg.mumford_shah import MumfordShahLoss  # noqa: E402
from pymic.loss.seg.ssl import TotalVariationLoss  # noqa: E402

import wsloracle as WO  # noqa: E402

# name -> (n, c, d, h, w, ci)
SHAPES = {"crf5": (1, 3, 3, 9, 11, 1), "crf2": (2, 2, 2, 7, 6, 2), "ms": (2, 3, 2, 7, 9, 2), "tv": (2, 3, 4, 5, 7, 1)}
CRF = {"crf5": 5, "crf2": 2}
MS = {"l1": ("l1", 1.0), "l2": ("l2", 0.25)}


def main():
    out = {}
    for name, (n, c, d, h, w, ci) in SHAPES.items():
        lg, im = WO.logits_case("golden.wsl." + name, n, c, d, h, w, ci)
        out[name + ".logits"], out[name + ".image"] = lg, im

        def run(fn):
            x = torch.from_numpy(lg).clone().requires_grad_(True)
            val = fn(x, torch.from_numpy(im).clone())
            val.backward()
            assert np.isfinite(val.item()) and np.isfinite(x.grad.numpy()).all(), name
            return np.float32(val.item()), x.grad.numpy().copy()

        if name in CRF:
            kernels = [{'weight': 1.0, 'xy': 5, 'rgb': 0.1}, {'weight': 1.0, 'xy': 3}]

            def crf(x, image):
                soft = torch.softmax(x, dim=1)
                inputs = torch.reshape(torch.transpose(image, 1, 2), [n * d, ci, h, w])
                soft = torch.reshape(torch.transpose(soft, 1, 2), [n * d, c, h, w])
                return GatedCRFLoss()(soft, kernels, CRF[name], {'rgb': inputs}, h, w)["loss"]

            out[name + ".loss"], out[name + ".dlogits"] = run(crf)
        elif name == "ms":
            for tag, (penalty, lam) in MS.items():
                mod = MumfordShahLoss({'MumfordShahLoss_penalty': penalty, 'MumfordShahLoss_lambda': lam})
                mod.softmax = True
                out["ms.%s.loss" % tag], out["ms.%s.dlogits" % tag] = run(lambda x, image: mod({"prediction": x, "image": image}))
        else:
            holder = types.SimpleNamespace(softmax=True)
            out["tv.loss"], out["tv.dlogits"] = run(lambda x, image: TotalVariationLoss.forward(holder, {"prediction": x}))
    path = os.path.join(HERE, "wsl_losses.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < (1 << 20), path
    print("wsl_losses.npz ok: %d arrays, %d bytes" % (len(out), os.path.getsize(path)))
    for k in sorted(out):
        if k.endswith(".loss"):
            print("  %s = %.8g" % (k, out[k]))


if __name__ == "__main__":
    main()
