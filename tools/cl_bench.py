"""Secondary measurement (not a bench.py line): confident learning (fplx.confident, csrc/cl.hip on fplx_select_kth) pass by pass
and as a whole get_confident_map, against the numpy restatement (tests/cloracle.py) on the CPU of the same machine, at the
benchmark's logit shape C = 2, M = 2 x 80 x 160 x 160 voxels and at C = 4 of the same M.
Both sides run in ONE process in alternating rounds: the kernels between HIP events over `iters` back-to-back calls into
warmed-up buffers, numpy once per round under time.perf_counter; the median over the rounds with minimum and maximum beside it.
`ratio` is the numpy median over the kernels' median (above 1: the kernels are faster).  Each streaming pass also reports the
bytes it has to move as a fraction of the streaming rate the project quotes (6.05 TB/s).  No figure is a pass
condition.
usage: python tools/cl_bench.py [--iters N] [--rounds N] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
for p in ("..", os.path.join("..", "fpl-plus_amd"), os.path.join("..", "tests")):
    sys.path.insert(0, os.path.join(HERE, p))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import fplx  # noqa: F401,E402
from fplx import confident, ops  # noqa: E402
import cloracle as O  # noqa: E402

M = 2 * 80 * 160 * 160
STREAM_TBS = 6.05


def event_us(once, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        once()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters


def cpu_us(once):
    t0 = time.perf_counter()
    once()
    return 1e6 * (time.perf_counter() - t0)


def np_softmax(x):
    e = np.exp(x - x.max(0, keepdims=True))
    return e / e.sum(0, keepdims=True)


def np_stats(s, psx):
    c = psx.shape[0]
    cnt = np.array([(s == k).sum() for k in range(c)], np.int64)
    return cnt, np.array([psx[k][s == k].astype(np.float64).sum() for k in range(c)]) / cnt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/cl_bench.py measures on the GPU; none is visible")
    rows = []
    for c in (2, 4):
        s, x = O.logits_case(20 + c, c, M)
        ds, dx = torch.from_numpy(s).cuda(), torch.from_numpy(x).cuda()
        psx_d = ops.cl_softmax(dx)
        psx = psx_d.cpu().numpy()
        an = confident.analyse(ds, psx_d, "both", planar=True)
        thr_d, thr = an.thr_dev, an.thr
        keys_d = torch.empty(M, dtype=torch.float32, device="cuda")
        out_d = torch.empty_like(dx)
        mem = s == 0
        variants = [
            ("cl_softmax", 2 * c * M * 4, lambda: ops.cl_softmax(dx, out=out_d), lambda: np_softmax(x)),
            ("cl_class_stats", c * M * 4 + M, lambda: ops.cl_class_stats(psx_d, ds), lambda: np_stats(s, psx)),
            ("cl_confident_joint", c * M * 4 + M, lambda: ops.cl_confident_joint(psx_d, ds, thr_d),
             lambda: O.confident_joint(s, psx, thr)),
            ("cl_select_keys (margin) + select_kth vs numpy partition", None,
             lambda: ops.select_kth(ops.cl_select_keys(psx_d, ds, 0, 1, out=keys_d), [int(an.P[1][0]) - 1]),
             lambda: np.partition(-(psx[1] - psx[0])[mem], int(an.P[1][0]) - 1)),
            ("cl_select_keys (margin) alone", 13 * M, lambda: ops.cl_select_keys(psx_d, ds, 0, 1, out=keys_d),
             lambda: np.where(mem, -(psx[1] - psx[0]), np.float32(np.nan))),
            ("cl_noise_mask (both)", c * M * 4 + 2 * M,
             lambda: ops.cl_noise_mask(psx_d, ds, ops.CL_BOTH, an.class_cut, an.pair_cut, an.pair_active), None),
            ("get_confident_map('both') from logits, whole", None,
             lambda: confident.get_confident_map(ds, dx, "both", planar=True), lambda: O.run(s, np_softmax(x))),
        ]
        for name, nbytes, fused, ref in variants:
            for _ in range(2):
                fused()
            torch.cuda.synchronize()
            f_us, r_us = [], []
            for _ in range(a.rounds):                            # alternating rounds: kernels, numpy, kernels, ...
                f_us.append(event_us(fused, a.iters))
                if ref is not None:
                    r_us.append(cpu_us(ref))
            fm = float(np.median(f_us))
            r = dict(name=name, classes=c, fused_us=round(fm, 2), fused_us_min_max=[round(min(f_us), 2), round(max(f_us), 2)])
            if ref is not None:
                rm = float(np.median(r_us))
                r.update(numpy_us=round(rm, 1), numpy_us_min_max=[round(min(r_us), 1), round(max(r_us), 1)], ratio=round(rm / fm, 1),
                         beats_numpy=bool(fm < rm))
            if nbytes is not None:
                r.update(bytes=nbytes, tb_per_s=round(nbytes / fm * 1e-6, 3), of_stream_rate=round(nbytes / fm * 1e-6 / STREAM_TBS, 3))
            rows.append(r)
            print(json.dumps(r), flush=True)
    res = dict(tool="tools/cl_bench.py --iters %d --rounds %d" % (a.iters, a.rounds), device=torch.cuda.get_device_name(0),
               voxels=M, stream_rate_tb_per_s=STREAM_TBS,
               note="us per call: HIP events over back-to-back calls (kernels), perf_counter (numpy, same machine's CPU), median of "
                    "alternating rounds; whole = softmax + stats + joint + one host read + the selections + mask",
               rows=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
