"""Generates tests/golden/crop_label.npz by RUNNING the reference's crop, bounding-box and label transforms
(PyMIC/pymic/transform/{crop,label_convert,intensity}.py: CenterCrop, CropWithBoundingBox, RandomCrop,
RandomResizedCrop, LabelConvert, LabelConvertNonzero, PartialLabelToProbability, ReduceLabelDim, GrayscaleToRGB, imported
with the stub modules of _ref_import.py) on deterministic inputs.  Stored: the inputs, every output, the `<Name>_Param`
strings, the results of the inverse transforms on deterministic predictions, where the draws left Python's `random`,
and the names of the reference's TransformDict.  Build-container only; the GPU box reads the .npz.

Keys: `<case>_<sample key>` for the forward results, `<case>_param` for the parameter string, `<case>_predict` /
`<case>_inverse` (`..._predict1` / `..._inverse1` for the second entry of a list prediction), `cases_json` for the
parameters of every case (tests/crop_label_ref.py CASES is the same table)."""
import io
import json
import os
import random
import sys
from contextlib import redirect_stdout

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _ref_import  # noqa: E402

_ref_import.install()
import crop_label_ref as CL  # noqa: E402  (inputs and the case table only)
from pymic.transform import trans_dict  # noqa: E402

T = trans_dict.TransformDict


def run(names, params, sample, seed=None):
    if seed is not None:
        random.seed(seed)
        np.random.seed(seed)
    ts = [T[n](dict(params, task="segmentation")) for n in names]
    with redirect_stdout(io.StringIO()):                 # CropWithBoundingBox prints its box
        for t in ts:
            sample = t(sample)
    return ts, sample


def store(out, case, sample, keys):
    for k in keys:
        if k in sample:
            out["%s_%s" % (case, k)] = np.array(sample[k])


def main():
    inp = CL.inputs()
    out = dict(inp)
    out["cases_json"] = np.array(json.dumps(CL.CASES))
    out["names_json"] = np.array(json.dumps(sorted(T.keys())))
    for case, c in CL.CASES.items():
        sample = {k: inp[v].copy() for k, v in c["sample"].items()}
        ts, s = run(c["names"], c["params"], sample, c.get("seed"))
        store(out, case, s, ("image", "label", "pixel_weight", "image1", "label_prob"))
        for t in ts:
            key = type(t).__name__ + "_Param"
            if key in s:
                out["%s_%s" % (case, key)] = np.array(s[key])
        if "seed" in c:
            out[case + "_next_random"] = np.array(random.random())
        inv = c.get("inverse")
        if inv:
            t = [t for t in ts if type(t).__name__ == inv["of"]][0]
            shape = s["image"].shape[1:]
            preds = [CL.prediction("%s.predict%d" % (case, i), (1, inv["channels"]) + tuple(shape)) for i in range(inv["count"])]
            param_key = inv["of"] + "_Param"
            q = {param_key: [s[param_key]] if inv.get("collated") else s[param_key],
                 "predict": [p.copy() for p in preds] if inv["count"] > 1 else preds[0].copy()}
            q = t.inverse_transform_for_prediction(q)
            got = q["predict"] if inv["count"] > 1 else [q["predict"]]
            assert isinstance(q["predict"], list) == (inv["count"] > 1)
            for i, (p, g) in enumerate(zip(preds, got)):
                sfx = "" if i == 0 else str(i)
                out["%s_predict%s" % (case, sfx)] = p
                out["%s_inverse%s" % (case, sfx)] = g
    path = os.path.join(HERE, "crop_label.npz")
    np.savez_compressed(path, **out)
    print("%d arrays, %d bytes" % (len(out), os.path.getsize(path)))
    for case in CL.CASES:
        for k in sorted(out):
            if k.startswith(case + "_") and k.endswith("_Param"):
                print(case, out[k])


if __name__ == "__main__":
    main()
