"""Secondary measurement (not a bench.py line): each regulariser of csrc/wsl.hip, forward + backward, against the torch
composition that restates the reference (tests/wsloracle.py: crf_statements = gatedcrf.py with F.unfold, tv_statements =
loss/seg/ssl.py:72-86 with max_pool3d, ms_statements = mumford_shah.py's channel loop) on the GPU with autograd, at the
benchmark's logit shape 2 x 2 x 80 x 160 x 160.  The CRF's torch composition unfolds every tensor to 121 copies of itself at
radius 5: it is tried at 160 slices first and at half as many after every out-of-memory error; the fused kernel is timed at
the slice count the composition reached, which the row reports.  Both sides run in ONE process in alternating rounds: HIP
events around `iters` back-to-back calls into warmed-up buffers, the median over the rounds with minimum and maximum beside
it; `ratio` is the torch median over the fused median (above 1: the kernel is faster).
usage: python tools/wsl_bench.py [--iters N] [--rounds N] [--out FILE.json]"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in ("..", os.path.join("..", "fpl-plus_amd"), os.path.join("..", "tests", "golden"), os.path.join("..", "tests")):
    sys.path.insert(0, os.path.join(HERE, p))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import fplx  # noqa: E402,F401
from fplx import ops  # noqa: E402
import wsloracle as WO  # noqa: E402

SHAPE = (2, 2, 80, 160, 160)
RADIUS = 5


def event_us(once, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        once()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/wsl_bench.py measures on the GPU; none is visible")
    g = torch.Generator().manual_seed(7)
    logits = (torch.randn(SHAPE, generator=g) * 1.58).cuda()
    image = torch.rand((SHAPE[0], 1) + SHAPE[2:], generator=g).cuda()
    one = torch.ones(1, dtype=torch.float32, device="cuda")
    dst = torch.empty_like(logits)

    def fused_tv():
        _, count = ops.wsl_tv_fwd(logits, True)
        ops.wsl_tv_bwd(logits, count, one, True, dst)

    def torch_tv():
        s = logits.detach().requires_grad_(True)
        WO.tv_statements(s, True)[0].backward()
        return s.grad

    def fused_ms():
        _, cen = ops.wsl_mumford_shah_fwd(logits, image, 1, 1.0, True)
        ops.wsl_mumford_shah_bwd(logits, image, cen, one, 1, 1.0, True, dst)

    def torch_ms():
        s = logits.detach().requires_grad_(True)
        WO.ms_statements(s, image, 1, 1.0, True)[0].backward()
        return s.grad

    # the CRF: the largest slice count the unfolded composition fits
    slices, crf_l, crf_i = 2 * SHAPE[2], None, None
    while slices >= 2:
        crf_l, crf_i = logits[:, :, :slices // 2].contiguous(), image[:, :, :slices // 2].contiguous()
        try:
            s = crf_l.detach().requires_grad_(True)
            WO.crf_statements(s, crf_i, WO.DEFAULT_DESC, RADIUS, True)[0].backward()
            del s
            torch.cuda.synchronize()
            break
        except torch.cuda.OutOfMemoryError:
            torch.cuda.empty_cache()
            slices //= 2
    crf_dst = torch.empty_like(crf_l)

    def fused_crf():
        _, kp = ops.wsl_gatedcrf_fwd(crf_l, crf_i, WO.DEFAULT_DESC, RADIUS, True)
        ops.wsl_gatedcrf_bwd(crf_l, kp, one, True, crf_dst)

    def torch_crf():
        s = crf_l.detach().requires_grad_(True)
        WO.crf_statements(s, crf_i, WO.DEFAULT_DESC, RADIUS, True)[0].backward()
        return s.grad

    variants = [("TotalVariationLoss fwd + bwd", fused_tv, torch_tv, list(SHAPE)),
                ("MumfordShahLoss (l1, lambda 1) fwd + bwd", fused_ms, torch_ms, list(SHAPE)),
                ("GatedCRFLoss (radius 5, the agent's two kernels) fwd + bwd, %d of 160 slices" % slices, fused_crf, torch_crf,
                 list(crf_l.shape))]
    rows = []
    for name, fused, ref, shape in variants:
        for _ in range(2):
            fused()
            ref()
        torch.cuda.synchronize()
        f_us, r_us = [], []
        for _ in range(a.rounds):                            # alternating rounds: kernel, torch, kernel, ...
            f_us.append(event_us(fused, a.iters))
            r_us.append(event_us(ref, a.iters))
        fm, rm = float(np.median(f_us)), float(np.median(r_us))
        r = dict(name=name, shape=shape, fused_us=round(fm, 2), fused_us_min_max=[round(min(f_us), 2), round(max(f_us), 2)],
                 torch_us=round(rm, 2), torch_us_min_max=[round(min(r_us), 2), round(max(r_us), 2)], ratio=round(rm / fm, 2),
                 beats_torch=bool(fm < rm))
        rows.append(r)
        print(json.dumps(r), flush=True)
    res = dict(tool="tools/wsl_bench.py --iters %d --rounds %d" % (a.iters, a.rounds), device=torch.cuda.get_device_name(0),
               shape=list(SHAPE), crf_slices=slices,
               note="us per fwd + bwd pair: HIP events over back-to-back calls, median of alternating rounds", rows=rows)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
