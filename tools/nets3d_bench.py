"""Secondary measurement (not a bench.py line): one train step (forward, Dice or deep-supervised Dice, backward, fused Adam) of
  1. UNet3D, 32-base, bf16, deep supervision off
  2. the same with deep supervision on (three 1x1x1 heads + trilinear interpolation, four loss passes)
  3. UNet2D5_dsbn with num_domains = 1 on the autograd route - the existing network as the yardstick
at 2 x 1 x 32 x 64 x 128, HIP events around `steps` back-to-back steps after `warmup` steps; and the head / interpolation
kernels of csrc/head.hip alone at 2 x 80 x 160 x 160 voxels, C = 32, 2 classes, as bytes moved over time (the bytes the
algorithm needs, computed from the shapes below: activations once, logits once; interpolation: coarse once, fine once).
usage: python tools/nets3d_bench.py [--steps N] [--warmup N] [--out FILE.json]"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in ("..", os.path.join("..", "fpl-plus_amd"), os.path.join("..", "tests", "golden")):
    sys.path.insert(0, os.path.join(HERE, p))
import torch  # noqa: E402

import fplx  # noqa: E402
from fplx import ops  # noqa: E402

SHAPE = (2, 1, 32, 64, 128)
FT = [32, 64, 128, 256, 512]
KSHAPE = (2, 80, 160, 160)          # N, D, H, W of the kernel-alone measurements
KC, KCLS = 32, 2


def event_ms(once, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        once()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def train_step_ms(net, lossf, x, y, steps, warmup, **call):
    net.cuda().train()
    opt = fplx.FusedAdam(net, 1e-3, weight_decay=1e-5)

    def once():
        opt.zero_grad()
        lossf({"prediction": net(x, **call), "ground_truth": y}).backward()
        opt.step()
    for _ in range(warmup):
        once()
    torch.cuda.synchronize()
    return event_ms(once, steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/nets3d_bench.py needs the GPU: there is nothing to measure without one")
    g = torch.Generator().manual_seed(3)
    torch.cuda.manual_seed(3)
    x = torch.randn(SHAPE, generator=g).cuda()
    lab = torch.zeros((SHAPE[0], 2) + SHAPE[2:])
    lab[:, 0] = 1.0
    lab[:, 0, 8:24, 16:48, 32:96] = 0.0
    lab[:, 1, 8:24, 16:48, 32:96] = 1.0
    lab = lab.cuda()
    rows = []
    u3 = dict(in_chns=1, feature_chns=FT, dropout=[0, 0, 0.3, 0.4, 0.5], class_num=2, trilinear=False, precision="bf16")
    for name, ds in (("UNet3D bf16, deep supervision off", False), ("UNet3D bf16, deep supervision on", True)):
        torch.manual_seed(1)
        net = fplx.UNet3D(dict(u3, deep_supervise=ds))
        lossf = fplx.DeepSuperviseLoss({"base_loss": fplx.DiceLoss()}) if ds else fplx.DiceLoss()
        rows.append(dict(case=name, train_step_ms=round(train_step_ms(net, lossf, x, lab, a.steps, a.warmup), 4)))
        print(json.dumps(rows[-1]), flush=True)
        del net
    torch.manual_seed(1)
    dsbn = fplx.UNet2D5_dsbn(dict(in_chns=1, feature_chns=FT, dropout=[0, 0, 0.3, 0.4, 0.5], conv_dims=[3] * 5, class_num=2,
                                  bilinear=False, num_domains=1, precision="bf16"))
    rows.append(dict(case="UNet2D5_dsbn bf16, num_domains = 1, autograd route (yardstick)",
                     train_step_ms=round(train_step_ms(dsbn, fplx.DiceLoss(), x, lab, a.steps, a.warmup,
                                                       domain_label=torch.zeros(SHAPE[0], dtype=torch.long)), 4)))
    print(json.dumps(rows[-1]), flush=True)
    del dsbn
    # ---- the kernels alone
    n, d, h, w = KSHAPE
    v = d * h * w
    for dt, esz in ((torch.bfloat16, 2), (torch.float32, 4)):
        act = torch.randn((n * v, KC), device="cuda").to(dt)
        wt = torch.randn((KCLS, KC), generator=g).cuda()
        bias = torch.randn((KCLS,), generator=g).cuda()
        lg = torch.empty((n, KCLS, v), device="cuda")
        da = torch.empty_like(act)
        dw, db = torch.empty_like(wt), torch.empty_like(bias)
        ws = torch.empty(ops.head_wgrad_ws_bytes(n, v, KC, KCLS), dtype=torch.uint8, device="cuda")
        a_bytes, l_bytes = n * v * KC * esz, n * v * KCLS * 4
        for kname, once, nbytes in (
                ("head_fwd", lambda: ops.head_fwd(act, wt, bias, lg, n, v, KC, KCLS), a_bytes + l_bytes),
                ("head_dgrad", lambda: ops.head_dgrad(lg, wt, da, n, v, KC, KCLS, False), a_bytes + l_bytes),
                ("head_dgrad accumulate", lambda: ops.head_dgrad(lg, wt, da, n, v, KC, KCLS, True), 2 * a_bytes + l_bytes),
                ("head_wgrad", lambda: ops.head_wgrad(act, lg, dw, db, n, v, KC, KCLS, ws), a_bytes + l_bytes)):
            for _ in range(a.warmup):
                once()
            ms = event_ms(once, a.steps)
            rows.append(dict(kernel="%s %s" % (kname, str(dt).split(".")[1]), ms=round(ms, 4), bytes=nbytes,
                             gbytes_per_s=round(nbytes / ms / 1e6, 1)))
            print(json.dumps(rows[-1]), flush=True)
        del act, da
    for f in (2, 4, 8):
        cd, ch, cw = d // f, h // f, w // f
        coarse = torch.randn((n * KCLS, cd, ch, cw), device="cuda")
        fine = torch.empty((n * KCLS, cd * f, ch * f, cw * f), device="cuda")
        dco = torch.empty_like(coarse)
        nbytes = 4 * (coarse.numel() + fine.numel())
        for kname, once in (("interp_fwd", lambda: ops.interp_fwd(coarse, fine, n * KCLS, (cd, ch, cw), f)),
                            ("interp_bwd", lambda: ops.interp_bwd(fine, dco, n * KCLS, (cd, ch, cw), f))):
            for _ in range(a.warmup):
                once()
            ms = event_ms(once, a.steps)
            rows.append(dict(kernel="%s f=%d" % (kname, f), ms=round(ms, 4), bytes=nbytes, gbytes_per_s=round(nbytes / ms / 1e6, 1)))
            print(json.dumps(rows[-1]), flush=True)
    res = dict(tool="tools/nets3d_bench.py --steps %d --warmup %d" % (a.steps, a.warmup), device=torch.cuda.get_device_name(0),
               shape=list(SHAPE), kernel_shape=list(KSHAPE) + [KC, KCLS],
               note="train_step_ms: HIP events over back-to-back train steps (autograd route, FusedAdam); kernels: HIP events over "
                    "back-to-back launches, bytes = what the algorithm needs (computed from the shapes)", rows=rows)
    if a.out:
        with open(a.out, "w") as f_:
            json.dump(res, f_, indent=1)


if __name__ == "__main__":
    main()
