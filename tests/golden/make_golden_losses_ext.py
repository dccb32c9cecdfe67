#!/usr/bin/env python3
"""Generate tests/golden/losses_ext.npz by RUNNING THE REFERENCE's own loss classes on the CPU (float32, value and dlogits by
autograd), as make_golden.py:gen_losses does for the first three losses.  Build container only:

    python tests/golden/make_golden_losses_ext.py

What is executed from the reference (reference paths): pymic/loss/seg/dice.py:130-199 FocalDiceLoss / NoiseRobustDiceLoss,
exp_log.py ExpLogLoss, ce.py:46-93 GeneralizedCELoss (without class or pixel weights - with either it cannot run),
mse.py MSELoss / MAELoss, slsr.py SLSRLoss, combined.py CombinedLoss, loss_dict_seg.py SegLossDict (its key list).
Shapes, parameters and cases: losses_ext_cases.py.  Float gradients do not compress: every case on every shape is 1.4 MB, so
the largest shape ("a") goes to a second archive, losses_ext_a.npz, and each file stays below 1 MiB."""
import contextlib
import io
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

from pymic.loss.seg.combined import CombinedLoss  # noqa: E402
from pymic.loss.loss_dict_seg import SegLossDict  # noqa: E402

import losses_ext_cases as LC  # noqa: E402


def main():
    out = {"names_json": np.frombuffer(json.dumps(sorted(SegLossDict.keys())).encode(), np.uint8)}
    for skey in LC.SHAPES:
        logits, label, pw = LC.inputs(skey)
        probs = torch.softmax(torch.from_numpy(logits), 1).numpy().copy()
        out[skey + ".probs"] = probs
        for tag, (name, softmax, with_pw) in LC.CASES.items():
            cfg = LC.config(tag)
            mod = CombinedLoss(cfg, SegLossDict) if isinstance(name, list) else SegLossDict[name](cfg)
            x = torch.from_numpy(logits if softmax else probs).clone().requires_grad_(True)
            d = {"prediction": x, "ground_truth": torch.from_numpy(label)}
            if with_pw:
                d["pixel_weight"] = torch.from_numpy(pw)
            with contextlib.redirect_stdout(io.StringIO()):
                val = mod(d)
            val.backward()
            g = x.grad.numpy().copy()
            assert np.isfinite(val.item()) and np.isfinite(g).all(), (skey, tag)
            out["%s.%s.loss" % (skey, tag)] = np.float32(val.item())
            out["%s.%s.dlogits" % (skey, tag)] = g
    for fname, keep in (("losses_ext.npz", lambda k: not k.startswith("a.")), ("losses_ext_a.npz", lambda k: k.startswith("a."))):
        path = os.path.join(HERE, fname)
        sub = {k: v for k, v in out.items() if keep(k)}
        np.savez_compressed(path, **sub)
        assert os.path.getsize(path) < (1 << 20), path
        print("%s ok: %d arrays, %d bytes" % (fname, len(sub), os.path.getsize(path)))


if __name__ == "__main__":
    main()
