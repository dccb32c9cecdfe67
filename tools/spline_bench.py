"""Secondary measurement (not a bench.py line): cubic-spline resampling (csrc/spline.hip) on the two volumes the dataset
preparation and the inference path meet - a 1x40x256x256 target crop, zoomed in plane by (1, 1.2, 1.2) as preprocess_vs.py
zooms in plane only, and 1x48x160x272 zoomed by 1.2 along every axis, as tools/resample_bench.py does at order 1.

Per volume, in alternating rounds in one process (every round times every item once, so drift hits all of them alike):
  prefilter   fplx_spline_prefilter alone, HIP events around `iters` back-to-back calls into a preallocated output
  interp      fplx_resample_spline alone on the stored coefficients
  zoom3       fplx.resample.zoom(order=3): both kernels and the allocations of the public path
  zoom1       fplx.resample.zoom(order=1): the order-1 kernel on the same volume and output size
  stream      a device copy of the fp64 coefficient volume (8 B read + 8 B written per voxel): the streaming rate of this
              machine at this size, against which the prefilter's rate is stated
and once, by wall clock on the machine's CPU: scipy.ndimage.zoom(order=3), the reference's cost per volume.

Bytes.  The prefilter's three passes need about 52 B per voxel if every line stayed on chip between a pass's sweeps (4 read
+ 8 written, then 8 + 8 twice, and one more 8 for a start-up sum); the kernels as written request 132 B per voxel (each pass
sweeps its lines three times: start-up sum over the line and its mirror image, causal, anticausal), the re-reads being served
by L2 and the Infinity Cache at these sizes.  Reported: ideal_share = (52 B * voxels / stream rate) / prefilter time, and the
requested rate 132 B * voxels / prefilter time.
usage: python tools/spline_bench.py [--iters N] [--rounds N] [--out FILE.json] [--no-scipy]"""
import argparse
import ctypes
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
from fplx import ops, resample  # noqa: E402
from fplx._lib import call  # noqa: E402

CASES = [("target_crop_40x256x256", (40, 256, 256), (1.0, 1.2, 1.2)), ("inference_48x160x272", (48, 160, 272), (1.2, 1.2, 1.2))]
IDEAL_BYTES, REQUESTED_BYTES = 52, 132


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
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-scipy", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spline_bench: no GPU - nothing is measured without one")
    rows = []
    for name, shape, zoom in CASES:
        img = (detdata.normal("bench.sp." + name, (1,) + shape) * 37.0 + 210.0).astype(np.float32)
        x = torch.from_numpy(img).cuda()
        out = resample.zoom_size(shape, zoom)
        m = [float(n - 1) / (o - 1) if i == j else 0.0 for i, (n, o) in enumerate(zip(shape, out)) for j in range(3)]
        mm, tt = (ctypes.c_double * 9)(*m), (ctypes.c_double * 3)(0.0, 0.0, 0.0)
        coef = torch.empty(x.shape, dtype=torch.float64, device=x.device)
        coef2 = torch.empty_like(coef)
        y = torch.empty((1,) + tuple(out), dtype=torch.float32, device=x.device)
        st = ops.stream()
        c, d, h, w = x.shape
        items = {
            "prefilter": lambda: call("fplx_spline_prefilter", x.data_ptr(), coef.data_ptr(), c, d, h, w, 3, st),
            "interp": lambda: call("fplx_resample_spline", coef.data_ptr(), y.data_ptr(), c, d, h, w, out[0], out[1], out[2], mm,
                                   tt, 3, st),
            "zoom3": lambda: resample.zoom(x, zoom, 3),
            "zoom1": lambda: resample.zoom(x, zoom, 1),
            "stream": lambda: coef2.copy_(coef),
        }
        for fn in items.values():                      # warm up every item before the first timed round
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in items}
        for _ in range(a.rounds):
            for k, fn in items.items():
                ms[k].append(event_ms(fn, a.iters))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        vox = float(np.prod(shape))
        stream_gbs = 16.0 * vox / med["stream"] * 1e-6
        r = dict(case=name, in_shape=[1] + list(shape), out_shape=[1] + list(out), iters=a.iters, rounds=a.rounds)
        for k in items:
            r[k + "_ms"] = round(med[k], 4)
            r[k + "_ms_min_max"] = [round(min(ms[k]), 4), round(max(ms[k]), 4)]
        r["stream_gbytes_per_s"] = round(stream_gbs, 1)
        r["prefilter_requested_gbytes_per_s"] = round(REQUESTED_BYTES * vox / med["prefilter"] * 1e-6, 1)
        r["prefilter_ideal_share_of_stream"] = round((IDEAL_BYTES * vox / (stream_gbs * 1e6)) / med["prefilter"], 4)
        r["zoom3_over_zoom1"] = round(med["zoom3"] / med["zoom1"], 1)
        if not a.no_scipy:
            from scipy import ndimage
            t0 = time.perf_counter()
            want = ndimage.zoom(img, [1.0] + list(zoom), order=3)
            r["scipy_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            r["scipy_over_zoom3"] = round(r["scipy_ms"] / med["zoom3"], 1)
            got = resample.zoom(x, zoom, 3).cpu().numpy()
            r["not_identical_to_scipy_float32"] = int((got != want).sum())
            r["outputs"] = int(got.size)
        rows.append(r)
        print(json.dumps(r), flush=True)
    res = dict(tool="tools/spline_bench.py --iters %d --rounds %d" % (a.iters, a.rounds), device=torch.cuda.get_device_name(0),
               host_cpus=len(os.sched_getaffinity(0)),
               note="*_ms: median over the rounds of HIP-event time per call (min and max of the rounds beside it); scipy_ms: one "
                    "wall-clock call on the GPU machine's CPU; stream: device copy of the fp64 coefficient volume, 16 B per voxel",
               rows=rows)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
