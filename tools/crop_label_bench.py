"""Secondary measurement (not a bench.py line): the crop, bounding-box and label kernels (csrc/crop_label.hip) and
CropWithBoundingBox end to end on one 1x48x160x272 volume (the VS inference size).  Every row is timed in alternating rounds
with its two yardsticks in the same process:
  device   HIP events around `iters` back-to-back calls into preallocated buffers after warm-up (median over the rounds);
  copy     fplx_crop_flip writing a same-sized copy of the same element type, timed in the same round: the project's
           plain-copy yardstick.  `bytes_per_voxel` is what the kernel must move (read + written), `rate_vs_copy` the
           kernel's bytes per second over the copy's;
  numpy    the numpy restatement (tests/crop_label_ref.py) of the same pass on this machine's CPU (wall clock, median).
The end-to-end row is the class on a device sample (image + label): bounding box, one device->host copy of 9 ints, two
gathers - by wall clock around a device synchronise, against the restatement's class on the host arrays.
Outputs are compared in the same run (every row must say equal).
usage: python tools/crop_label_bench.py [--iters N] [--rounds N] [--reps N] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
for p in ("..", os.path.join("..", "fpl-plus_amd"), os.path.join("..", "tests", "golden"), os.path.join("..", "tests")):
    sys.path.insert(0, os.path.join(HERE, p))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import crop_label_ref as CL  # noqa: E402
import detdata  # noqa: E402
import fplx  # noqa: E402,F401
from fplx import ops, transform  # noqa: E402
from fplx._lib import call  # noqa: E402

SHAPE = (48, 160, 272)
BOX_LO, BOX_SIZE = (6, 20, 30), (36, 120, 212)           # the non-zero block of the image: what CropWithBoundingBox finds
CLASSES = 4


def event_ms(once, iters):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    d, h, w = SHAPE
    n = d * h * w
    image = np.zeros((1,) + SHAPE, np.float32)
    sl = tuple(slice(lo, lo + s) for lo, s in zip(BOX_LO, BOX_SIZE))
    image[(0,) + sl] = detdata.normal("bench.cl.image", BOX_SIZE) * 37.0 + 210.0
    label = np.minimum(detdata.uniform("bench.cl.label", (1,) + SHAPE) * 5.0, 4.0).astype(np.uint8)
    sub = np.ascontiguousarray(image[(slice(None),) + sl])
    lut = CL.lut_table([0, 1, 2, 4], [0, 1, 2, 3])
    dev = lambda x: torch.from_numpy(x).cuda()
    xd, ld, sd = dev(image), dev(label), dev(sub)
    lutd = torch.tensor(lut, dtype=torch.uint8, device="cuda:0")
    y4, y1 = torch.empty_like(xd), torch.empty_like(ld)
    box = torch.empty(9, dtype=torch.int32, device="cuda:0")
    prob = torch.empty((CLASSES,) + SHAPE, dtype=torch.float32, device="cuda:0")
    weight = torch.empty(SHAPE, dtype=torch.float32, device="cuda:0")
    top = torch.empty(1, dtype=torch.int32, device="cuda:0")
    st = ops.stream()
    P = lambda t: t.data_ptr()

    def copy(src, dst, elem):
        return lambda: call("fplx_crop_flip", P(src), P(dst), elem, 1, d, h, w, 0, 0, 0, d, h, w, 0, st)

    copy4, copy1 = copy(xd, y4, 4), copy(ld, y1, 1)
    kernels = [
        # name, launch, yardstick, bytes the yardstick moves per voxel, bytes the kernel moves per voxel, numpy pass, check
        ("nonzero_bbox (reads only)", lambda: call("fplx_nonzero_bbox", P(xd), 1, d, h, w, P(box), st), copy4, 8, 4,
         lambda: CL.nonzero_bbox(image),
         lambda want: (lambda o: (o[0], o[1:5], o[5:9]))(box.tolist()) == want),
        ("label_lut (uint8 -> uint8)", lambda: call("fplx_label_lut", P(ld), P(y1), n, P(lutd), st), copy1, 2, 2,
         lambda: CL.label_lut(label, lut), lambda want: np.array_equal(y1.cpu().numpy(), want)),
        ("partial_label_to_probability (%d classes)" % CLASSES,
         lambda: call("fplx_partial_label_to_probability", P(ld), P(prob), P(weight), CLASSES, n, P(top), st), copy4, 8,
         1 + 4 * (CLASSES + 1), lambda: CL.partial_label(label[0], CLASSES),
         lambda want: np.array_equal(prob.cpu().numpy(), want[0]) and np.array_equal(weight.cpu().numpy(), want[1]) and
         int(top.item()) == want[2]),
        ("paste_roi fp32 (%dx%dx%d into the volume)" % BOX_SIZE,
         lambda: call("fplx_paste_roi", P(sd), P(y4), 4, 1, *BOX_SIZE, d, h, w, *BOX_LO, st), copy4, 8,
         4 + 4.0 * sub.size / n, lambda: CL.paste_roi(sub, BOX_LO, SHAPE),
         lambda want: np.array_equal(y4.cpu().numpy(), want)),
    ]
    rows = []
    for name, once, yard, yard_bytes, bytes_per_voxel, ref, check in kernels:
        for _ in range(10):
            once()
            yard()
        torch.cuda.synchronize()
        k_ms, c_ms = [], []
        for _ in range(a.rounds):                        # alternating rounds: kernel, yardstick, kernel, ...
            k_ms.append(event_ms(once, a.iters))
            c_ms.append(event_ms(yard, a.iters))
        once()
        torch.cuda.synchronize()
        want = ref()
        km, cm = float(np.median(k_ms)), float(np.median(c_ms))
        r = dict(name=name, device_ms=round(km, 4), device_ms_min_max=[round(min(k_ms), 4), round(max(k_ms), 4)],
                 copy_ms=round(cm, 4), copy_ms_min_max=[round(min(c_ms), 4), round(max(c_ms), 4)],
                 bytes_per_voxel=round(bytes_per_voxel, 2), gbytes_per_s=round(bytes_per_voxel * n / km / 1e6, 1),
                 copy_gbytes_per_s=round(yard_bytes * n / cm / 1e6, 1),
                 rate_vs_copy=round((bytes_per_voxel / km) / (yard_bytes / cm), 2), equal_to_numpy=bool(check(want)),
                 numpy_ms=round(wall_ms(ref, a.reps), 2))
        r["numpy_over_device"] = round(r["numpy_ms"] / km, 1)
        rows.append(r)
        print(json.dumps(r), flush=True)

    # CropWithBoundingBox end to end
    params = {"task": "segmentation", "cropwithboundingbox_start": None, "cropwithboundingbox_output_size": None}
    cwb, cwb_np = transform.CropWithBoundingBox(params), CL.CropWithBoundingBox(params)

    def device_pass():
        s = cwb({"image": xd, "label": ld})
        torch.cuda.synchronize()
        return s

    def host_pass():
        return cwb_np({"image": image, "label": label})

    def copy_pass():
        copy4()
        copy1()
        torch.cuda.synchronize()

    e_ms, c_ms = [], []
    for _ in range(a.rounds):
        e_ms.append(wall_ms(device_pass, max(a.reps * 4, 20)))
        c_ms.append(wall_ms(copy_pass, max(a.reps * 4, 20)))
    s, sn = device_pass(), host_pass()
    r = dict(name="CropWithBoundingBox end to end (image + label, wall clock incl. the device->host copy of the box)",
             wall_ms=round(float(np.median(e_ms)), 4), wall_ms_min_max=[round(min(e_ms), 4), round(max(e_ms), 4)],
             copy_both_volumes_wall_ms=round(float(np.median(c_ms)), 4),
             equal_to_numpy=bool(np.array_equal(s["image"].cpu().numpy(), sn["image"]) and
                                 np.array_equal(s["label"].cpu().numpy(), sn["label"]) and
                                 s["CropWithBoundingBox_Param"] == sn["CropWithBoundingBox_Param"]),
             numpy_ms=round(wall_ms(host_pass, a.reps), 2), box=json.loads(s["CropWithBoundingBox_Param"]))
    r["numpy_over_device"] = round(r["numpy_ms"] / r["wall_ms"], 1)
    rows.append(r)
    print(json.dumps(r), flush=True)
    res = dict(tool="tools/crop_label_bench.py --iters %d --rounds %d --reps %d" % (a.iters, a.rounds, a.reps),
               device=torch.cuda.get_device_name(0), host_cpus=len(os.sched_getaffinity(0)), voxels=n,
               note="device_ms / copy_ms: HIP events over back-to-back calls, median of alternating rounds (min and max beside "
                    "it); numpy_ms: wall clock of the numpy restatement on the host CPU (median); rate_vs_copy: bytes per "
                    "second of the kernel over bytes per second of fplx_crop_flip on a same-sized copy of the same element type",
               rows=rows)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    if not all(r["equal_to_numpy"] for r in rows):
        raise SystemExit("a device result differs from the numpy restatement")


if __name__ == "__main__":
    main()
