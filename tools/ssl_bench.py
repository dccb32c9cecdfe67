"""Secondary measurement (not a bench.py line): each kernel of csrc/ssl.hip against the torch composition it replaces - the
reference's own statements (ssl_mt.py:79,90-100,112-113, ssl_uamt.py:77-100, loss/seg/ssl.py:36-43) on the GPU, autograd for
the backward - at the benchmark's logit shape 2 x 2 x 80 x 160 x 160 and, for the EMA, over the benchmark network's parameters.
Both sides run in ONE process in alternating rounds: HIP events around `iters` back-to-back calls into warmed-up buffers, the
median over the rounds with minimum and maximum beside it.  `bytes` is what the algorithm has to move (inputs read once per
pass, outputs written once), `hbm_fraction` the resulting rate over 6.05 TB/s, the rate the project's BatchNorm passes reach
(DESIGN section 5); `ratio` is the torch median over the fused median of the same rounds (above 1: the kernel is faster).
usage: python tools/ssl_bench.py [--iters N] [--rounds N] [--out FILE.json]"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in ("..", os.path.join("..", "fpl-plus_amd"), os.path.join("..", "tests", "golden")):
    sys.path.insert(0, os.path.join(HERE, p))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import fplx  # noqa: E402
from fplx import ops  # noqa: E402

SHAPE = (2, 2, 80, 160, 160)
NET = dict(in_chns=1, feature_chns=[32, 64, 128, 256, 512], dropout=[0.0, 0.0, 0.3, 0.4, 0.5], conv_dims=[3, 3, 3, 3, 3],
           class_num=2, bilinear=False, precision="bf16")          # bench.py's network, as the plain UNet2D5
BN_PASS_RATE = 6.05e12                                             # bytes / s, DESIGN section 5
T_MC = 8


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
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/ssl_bench.py measures on the GPU; none is visible")
    n, c = SHAPE[0], SHAPE[1]
    v = int(np.prod(SHAPE[2:]))
    ncv = n * c * v
    g = torch.Generator().manual_seed(7)
    base = torch.randn(SHAPE, generator=g) * 1.5
    student = (base + 0.5 * torch.randn(SHAPE, generator=g)).cuda()
    teacher = (base + 0.5 * torch.randn(SHAPE, generator=g)).cuda()
    mc = (base[None] + 0.5 * torch.randn((T_MC,) + SHAPE, generator=g)).cuda()
    x1 = torch.randn((n, 1) + SHAPE[2:], generator=g).cuda()
    thr = (0.75 + 0.25 * 0.3) * float(np.log(c))
    one = torch.ones(1, dtype=torch.float32, device="cuda")
    part2, part1 = ops.ssl_part(student, 2), ops.ssl_part(student, 1)
    out = torch.empty(4, dtype=torch.float64, device="cuda")
    mask = torch.empty((n,) + SHAPE[2:], dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(student)
    ybuf = torch.empty((1,) + tuple(x1.shape), dtype=torch.float32, device="cuda")

    def fused_perturb():
        ops.ssl_perturb(x1, None, 1, 0.1, 0.2, 11, 3, ybuf)

    def torch_perturb():
        return x1 + torch.clamp(torch.randn_like(x1) * 0.1, -0.2, 0.2)

    def fused_mt():
        ops.ssl_consistency_fwd(student, teacher, None, 0.0, True, part2, out)
        ops.ssl_consistency_bwd(student, teacher, None, out, one, 0, True, dst)

    def torch_mt():
        s = student.detach().requires_grad_(True)
        p1_soft = torch.softmax(s, dim=1)
        with torch.no_grad():
            p1_ema_soft = torch.softmax(teacher, dim=1)
        torch.nn.MSELoss()(p1_soft, p1_ema_soft).backward()
        return s.grad

    def fused_uamt():
        ops.ssl_consistency_fwd(student, teacher, mc, thr, True, part2, out, mask)
        ops.ssl_consistency_bwd(student, teacher, mask, out, one, T_MC, True, dst)

    def torch_uamt():
        s = student.detach().requires_grad_(True)
        p1_soft = torch.softmax(s, dim=1)
        with torch.no_grad():
            p1_ema_soft = torch.softmax(teacher, dim=1)
        square_error = torch.square(p1_soft - p1_ema_soft)
        preds = torch.softmax(mc, dim=2)
        preds = torch.mean(preds, dim=0)
        uncertainty = -1.0 * torch.sum(preds * torch.log(preds + 1e-6), dim=1, keepdim=True)
        m = (uncertainty < thr).float()
        (torch.sum(m * square_error) / (2 * torch.sum(m) + 1e-16)).backward()
        return s.grad

    def fused_ent():
        ops.ssl_entropy_fwd(student, True, part1, out)
        ops.ssl_entropy_bwd(student, one, True, dst)

    def torch_ent():
        s = student.detach().requires_grad_(True)
        predict = torch.nn.Softmax(dim=1)(s)
        predict = predict * 0.999 + 5e-4
        entropy = torch.sum(-predict * torch.log(predict), dim=1) / np.log(c)
        torch.mean(entropy).backward()
        return s.grad

    net, net_ema = fplx.UNet2D5(dict(NET)).cuda(), fplx.UNet2D5(dict(NET)).cuda()
    net._ensure_flat()
    net_ema._ensure_flat()
    nparam = net.flat_params.numel()
    plist, elist = [p.data for p in net.parameters()], [p.data for p in net_ema.parameters()]
    alpha = 0.99

    def fused_ema():
        ops.ema_step(net_ema.flat_params, net.flat_params, alpha)

    def torch_ema():
        for ema_param, param in zip(elist, plist):
            ema_param.mul_(alpha).add_(param, alpha=1 - alpha)

    f4 = 4.0
    variants = [
        ("ssl_perturb (Philox) vs x + clamp(randn_like * 0.1)", fused_perturb, torch_perturb, f4 * 2 * x1.numel()),
        ("consistency fwd + bwd, MeanTeacher", fused_mt, torch_mt, f4 * (2 + 3) * ncv),
        ("consistency fwd + bwd, UAMT T = %d" % T_MC, fused_uamt, torch_uamt, f4 * (2 + T_MC + 3) * ncv + 2.0 * n * v),
        ("EntropyLoss fwd + bwd", fused_ent, torch_ent, f4 * (1 + 2) * ncv),
        ("ema_step over %d parameters (%d tensors)" % (nparam, len(plist)), fused_ema, torch_ema, f4 * 3 * nparam),
    ]
    rows = []
    for name, fused, ref, nbytes in variants:
        for _ in range(3):
            fused()
            ref()
        torch.cuda.synchronize()
        f_us, r_us = [], []
        for _ in range(a.rounds):                            # alternating rounds: kernel, torch, kernel, ...
            f_us.append(event_us(fused, a.iters))
            r_us.append(event_us(ref, a.iters))
        fm, rm = float(np.median(f_us)), float(np.median(r_us))
        r = dict(name=name, fused_us=round(fm, 2), fused_us_min_max=[round(min(f_us), 2), round(max(f_us), 2)],
                 torch_us=round(rm, 2), torch_us_min_max=[round(min(r_us), 2), round(max(r_us), 2)], ratio=round(rm / fm, 2),
                 bytes=int(nbytes), tbytes_per_s=round(nbytes / fm / 1e6, 3), hbm_fraction=round(nbytes / (fm * 1e-6) / BN_PASS_RATE, 3),
                 beats_torch=bool(fm < rm))
        rows.append(r)
        print(json.dumps(r), flush=True)
    res = dict(tool="tools/ssl_bench.py --iters %d --rounds %d" % (a.iters, a.rounds), device=torch.cuda.get_device_name(0),
               shape=list(SHAPE), ema_parameters=nparam,
               note="us per call (a fwd + bwd pair where the row says so): HIP events over back-to-back calls, median of alternating "
                    "rounds; bytes: algorithmic; hbm_fraction: bytes / fused time over 6.05 TB/s (DESIGN section 5)",
               rows=rows)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
