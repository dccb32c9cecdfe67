"""Secondary measurement (not a bench.py line): the affine resampling kernel behind RandomRotate / Rescale / RandomRescale
on one 1x48x160x272 volume (the VS inference size).  For a generic 17 degree rotation in the H-W plane and a x1.2 zoom it
times
  device   fplx_resample_affine, order 0 on uint8 and order 1 on fp32 (order 0 on fp32 as well), HIP events around `iters`
           back-to-back calls into a preallocated output after warm-up;
  copy     ops.crop_flip (fplx_crop_flip) writing a volume of the same output size and element type: the project's plain
           copy rate for these element sizes - the resampler moves the same bytes with a gather on the read side;
  scipy    scipy.ndimage.rotate / zoom on the same arrays on this machine's CPU: the reference's cost per volume.
Bytes are counted as one read of the input volume plus one write of the output (the gather's reuse is served by the caches).
usage: python tools/resample_bench.py [--iters N] [--reps N] [--out FILE.json]"""
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
from fplx import ops, transform  # noqa: E402
from fplx._lib import call  # noqa: E402

SHAPE = (48, 160, 272)
ANGLE, ZOOM = 17.0, 1.2


def event_ms(once, iters):
    for _ in range(5):
        once()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        once()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def wall_ms(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def resample_ms(x, m, t, out, order, iters):
    c, d, h, w = x.shape
    y = torch.empty((c,) + tuple(out), dtype=x.dtype, device=x.device)
    mm = (ctypes.c_double * 9)(*[float(v) for row in m for v in row])
    tt = (ctypes.c_double * 3)(*[float(v) for v in t])
    st = ops.stream()
    ms = event_ms(lambda: call("fplx_resample_affine", x.data_ptr(), y.data_ptr(), x.element_size(), order, c, d, h, w,
                               out[0], out[1], out[2], mm, tt, st), iters)
    return ms, y


def copy_ms(dtype, out, iters):
    """crop_flip of a volume with the resampler's output size (crop at 0, no flip)"""
    src = torch.zeros((1,) + tuple(out), dtype=dtype, device="cuda:0")
    y = torch.empty_like(src)
    st = ops.stream()
    return event_ms(lambda: call("fplx_crop_flip", src.data_ptr(), y.data_ptr(), src.element_size(), 1, out[0], out[1], out[2],
                                 0, 0, 0, out[0], out[1], out[2], 0, st), iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from scipy import ndimage
    img = (detdata.normal("bench.rs.image", (1,) + SHAPE) * 37.0 + 210.0).astype(np.float32)
    zz, yy, xx = np.meshgrid(*[np.arange(n) for n in SHAPE], indexing="ij")
    lab = ((((zz - 24) / 15.0) ** 2 + ((yy - 80) / 50.0) ** 2 + ((xx - 136) / 90.0) ** 2) < 1).astype(np.uint8)[None]
    zoom_out = [int(round(n * ZOOM)) for n in SHAPE]
    step = [(n - 1.0) / (o - 1.0) for n, o in zip(SHAPE, zoom_out)]
    cases = {
        "rotate_17deg": (transform._rotate_affine(SHAPE, ANGLE, (-1, -2)) + (list(SHAPE),),
                         lambda x, order: ndimage.rotate(x, ANGLE, (-1, -2), reshape=False, order=order)),
        "zoom_x1.2": (([[step[i] if i == j else 0.0 for j in range(3)] for i in range(3)], [0.0] * 3, zoom_out),
                      lambda x, order: ndimage.zoom(x, [1.0] + [ZOOM] * 3, order=order)),
    }
    rows = []
    for name, ((m, t, out), ref) in cases.items():
        for what, x, order in (("uint8_order0", lab, 0), ("fp32_order0", img, 0), ("fp32_order1", img, 1)):
            xt = torch.from_numpy(x).cuda()
            ms, y = resample_ms(xt, m, t, out, order, a.iters)
            cms = copy_ms(xt.dtype, out, a.iters)
            want = ref(x, order)
            got = y.cpu().numpy()
            nbytes = (x.size + got.size) * x.itemsize
            r = dict(case=name, volume=what, in_shape=list(x.shape), out_shape=list(got.shape),
                     device_ms=round(ms, 4), crop_flip_ms=round(cms, 4), vs_copy=round(ms / cms, 2),
                     scipy_ms=round(wall_ms(lambda: ref(x, order), a.reps), 2),
                     gbytes_per_s=round(nbytes / ms * 1e-6, 1), differing_from_scipy=int((got != want).sum()))
            r["scipy_over_device"] = round(r["scipy_ms"] / ms, 1)
            rows.append(r)
            print(json.dumps(r), flush=True)
    res = dict(tool="tools/resample_bench.py --iters %d --reps %d" % (a.iters, a.reps), device=torch.cuda.get_device_name(0),
               host_cpus=len(os.sched_getaffinity(0)),
               note="device_ms / crop_flip_ms by HIP events over back-to-back calls after warm-up; scipy_ms by wall clock on the "
                    "GPU machine's CPU (median); gbytes_per_s = (input + output bytes) / device_ms", rows=rows)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
