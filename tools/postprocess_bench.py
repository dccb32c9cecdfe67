"""Secondary measurement (not a bench.py line): KeepLargestComponent post-processing of one predicted volume.
For 48x160x272 (the VS inference size) and 128x256x256, on a realistic mask (the thresholded smooth random map of a
two-class prediction plus islands) and on site-percolation noise at p = 0.31 (huge fractal components: the merge's worst
case), it times
  device   fplx_keep_largest_component (mode 1 and 2) on a device volume, HIP events around `iters` back-to-back calls
           into preallocated buffers, the error word checked afterwards;
  numpy    fplx.PostKeepLargestComponent on a numpy volume (host -> device -> host, the agent's save_outputs contract);
  scipy    the reference's pass restated (image_process.get_largest_k_components: ndimage.label with the 6-neighbour
           structure, ndimage.sum, keep the largest; then seg * mask) on this machine's CPU.
usage: python tools/postprocess_bench.py [--iters N] [--out FILE.json]"""
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
import fplx  # noqa: E402
from fplx import ops  # noqa: E402
from fplx._lib import call  # noqa: E402


def realistic(name, shape):
    f = detdata.normal(name, shape).astype(np.float64)
    for _ in range(3):
        for ax in range(3):
            f = (np.roll(f, -2, ax) + np.roll(f, -1, ax) + f + np.roll(f, 1, ax) + np.roll(f, 2, ax)) / 5.0
    s = (f > 0.25 * f.std()).astype(np.uint8)
    for row in detdata.uniform(name + ".islands", (30, 3)):
        z, y, x = [int(row[a] * (shape[a] - 2)) for a in range(3)]
        s[z:z + 2, y:y + 2, x:x + 1] = 1
    return s


def percolation(name, shape, p=0.31):
    return (detdata.uniform(name, shape) < p).astype(np.uint8)


def scipy_keep_largest(seg):
    import scipy.ndimage as ndi
    mask = np.asarray(seg > 0, np.uint8)
    lab, n = ndi.label(mask, ndi.generate_binary_structure(3, 1))
    sizes = ndi.sum(mask, lab, range(1, n + 1))
    return seg * np.asarray(lab == int(np.argmax(sizes)) + 1, np.uint8)


def device_ms(seg_t, mode, iters):
    n = seg_t.numel()
    d, h, w = seg_t.shape
    out = torch.empty_like(seg_t)
    ws = torch.empty(320 + 2 * n, dtype=torch.int32, device=seg_t.device)
    st = ops.stream()

    def once():
        call("fplx_keep_largest_component", seg_t.data_ptr(), d, h, w, 1 if mode == 2 else 0, out.data_ptr(),
             ws.data_ptr(), ws.numel() * 4, st)

    for _ in range(3):
        once()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        once()
    e1.record()
    torch.cuda.synchronize()
    if int(ws[0].item()):
        raise RuntimeError("error word set")
    return e0.elapsed_time(e1) / iters, out


def wall_ms(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for shape in ((48, 160, 272), (128, 256, 256)):
        for kind, gen in (("realistic", realistic), ("percolation_p0.31", percolation)):
            seg = gen("bench.pp.%s.%s" % (kind, shape), shape)
            t = torch.from_numpy(seg).cuda()
            r = dict(shape=list(shape), input=kind, foreground=float((seg > 0).mean()))
            for mode in (1, 2):
                ms, out = device_ms(t, mode, a.iters)
                r["device_ms_mode%d" % mode] = round(ms, 4)
            post = fplx.PostKeepLargestComponent({"keeplargestcomponent_mode": 1})
            r["numpy_ms"] = round(wall_ms(lambda: post(seg), a.reps), 3)
            try:
                want = scipy_keep_largest(seg)
                r["scipy_ms"] = round(wall_ms(lambda: scipy_keep_largest(seg), a.reps), 2)
                r["matches_scipy"] = bool(np.array_equal(post(seg), want))
            except ImportError:
                r["scipy_ms"] = None
            rows.append(r)
            print(json.dumps(r), flush=True)
    res = dict(tool="tools/postprocess_bench.py", device=torch.cuda.get_device_name(0), iters=a.iters,
               host_cpus=len(os.sched_getaffinity(0)), rows=rows)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
