"""Secondary measurement (not a bench.py line): the exact Euclidean distance transform (csrc/edt.hip) against
scipy.ndimage.distance_transform_edt on the same machine's CPU, on
  (a) the shipped label volume tests/golden/nifti/vs_gk_98_t2_lab.nii.gz and its complement - the two masks of
      get_euclidean_distance;
  (b) a 40x256x256 mask with 0.2 % background;
  (c) a 48x160x272 mask with a single background voxel in a corner: the worst case of the windowed search, every line of
      every pass is searched over its whole length.

Per mask, in alternating rounds in one process (every round times every item once, so drift hits all of them alike), HIP
events around `iters` back-to-back calls and a synchronise:
  pass_d / pass_h / pass_w   fplx_edt_pass alone on the float64 map the passes before it left.  The pass works in place and a
                             second run on its own result would search shorter windows, so every timed call first restores
                             the input with a device copy; the copy is timed alone as `stream` and subtracted.  (Inside
                             fplx_edt_squared the D pass reads the uint8 mask, 1 B per voxel instead of 8.)
  squared                    fplx_edt_squared: the three passes from the uint8 mask
  whole                      fplx.distance_transform_edt on a device tensor: the mask comparison, the no-background
                             reduction, the three passes, the root and the allocations of the public path
  whole_idx                  the same with return_indices=True
  stream                     a device copy of the float64 map (8 B read + 8 B written per voxel): the streaming bound of a pass
and by wall clock, scipy's call (median of `--scipy-runs`).  share_of_stream = stream / pass: 1.0 would be a pass at the
copy's rate.
usage: python tools/edt_bench.py [--iters N] [--rounds N] [--scipy-runs N] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "fpl-plus_amd"))
sys.path.insert(0, os.path.join(HERE, "..", "tests", "golden"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import detdata  # noqa: E402
import fplx  # noqa: E402,F401
from fplx import image_process, ops  # noqa: E402
from fplx.nifti import load_nifty_volume_as_4d_array  # noqa: E402


def cases():
    lab = load_nifty_volume_as_4d_array(os.path.join(HERE, "..", "tests", "golden", "nifti", "vs_gk_98_t2_lab.nii.gz"))
    lab = np.asarray(lab["data_array"][0] > 0, np.uint8)
    sparse = np.asarray(detdata.uniform("bench.edt.sparse", (40, 256, 256)) >= 0.002, np.uint8)
    corner = np.ones((48, 160, 272), np.uint8)
    corner[0, 0, 0] = 0
    return [("label_fg", lab), ("label_bg", 1 - lab), ("sparse_40x256x256", sparse), ("corner_48x160x272", corner)]


def event_ms(once, iters):
    once()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        once()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scipy-runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("edt_bench: no GPU - nothing is measured without one")
    from scipy import ndimage
    rows = []
    for name, mask in cases():
        m = torch.from_numpy(mask).cuda()
        g0 = torch.where(m != 0, float("inf"), 0.0).to(torch.float64)[None].contiguous()
        g1 = ops.edt_pass(g0.clone(), 0)
        g2 = ops.edt_pass(g1.clone(), 1)
        work = torch.empty_like(g0)

        def one_pass(src, axis):
            work.copy_(src)
            ops.edt_pass(work, axis)

        items = {
            "stream": lambda: work.copy_(g0),
            "pass_d": lambda: one_pass(g0, 0),
            "pass_h": lambda: one_pass(g1, 1),
            "pass_w": lambda: one_pass(g2, 2),
            "squared": lambda: ops.edt_squared(m),
            "whole": lambda: image_process.distance_transform_edt(m),
            "whole_idx": lambda: image_process.distance_transform_edt(m, return_indices=True),
        }
        for fn in items.values():                      # warm up every item before the first timed round
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in items}
        for _ in range(a.rounds):
            for k, fn in items.items():
                ms[k].append(event_ms(fn, a.iters))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        vox = float(mask.size)
        r = dict(case=name, shape=list(mask.shape), background=int((mask == 0).sum()), iters=a.iters, rounds=a.rounds)
        r["stream_ms"] = round(med["stream"], 4)
        r["stream_gbytes_per_s"] = round(16.0 * vox / med["stream"] * 1e-6, 1)
        for k in ("pass_d", "pass_h", "pass_w"):
            net = med[k] - med["stream"]                # the pass without its fresh copy
            r[k + "_ms"] = round(net, 4)
            r[k + "_share_of_stream"] = round(med["stream"] / net, 4) if net > 0 else None
        for k in ("squared", "whole", "whole_idx"):
            r[k + "_ms"] = round(med[k], 4)
            r[k + "_ms_min_max"] = [round(min(ms[k]), 4), round(max(ms[k]), 4)]
        t = []
        for _ in range(a.scipy_runs):
            t0 = time.perf_counter()
            want = ndimage.distance_transform_edt(mask)
            t.append((time.perf_counter() - t0) * 1e3)
        r["scipy_ms"] = round(float(np.median(t)), 1)
        r["scipy_over_whole"] = round(r["scipy_ms"] / med["whole"], 1)
        got = image_process.distance_transform_edt(m).cpu().numpy()
        r["not_identical_to_scipy"] = int((got != want).sum())
        r["outputs"] = int(got.size)
        rows.append(r)
        print(json.dumps(r), flush=True)
    res = dict(tool="tools/edt_bench.py --iters %d --rounds %d" % (a.iters, a.rounds), device=torch.cuda.get_device_name(0),
               host_cpus=len(os.sched_getaffinity(0)),
               note="*_ms: median over the rounds of HIP-event time per call; pass_*: one pass on a fresh copy minus the copy "
                    "(stream); scipy_ms: median wall clock of scipy.ndimage.distance_transform_edt on this machine's CPU",
               rows=rows)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
