"""Secondary measurement (not a bench.py line): the second loss family's pass (csrc/loss_ext.hip) against the existing one
(fplx_seg_loss_fwd / _bwd with Dice) at the benchmark's loss shape, 2 x 2 x 80 x 160 x 160 fp32 logits.
Every variant is timed in alternating rounds with the existing pass in the same process: HIP events around `iters`
back-to-back forward + backward pairs into preallocated buffers after warm-up; the median over the rounds is reported with
the minimum and maximum beside it, and `ratio` is the variant's median over the existing pass's median of the SAME rounds.
Bytes are equal for every row (logits and label read twice, dlogits written once), so a ratio above 1 is arithmetic:
`transcendentals` lists what each variant adds per voxel and class.
usage: python tools/loss_ext_bench.py [--iters N] [--rounds N] [--out FILE.json]"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in ("..", os.path.join("..", "fpl-plus_amd"), os.path.join("..", "tests", "golden")):
    sys.path.insert(0, os.path.join(HERE, p))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import fplx  # noqa: E402,F401
from fplx import ops  # noqa: E402

SHAPE = (2, 2, 80, 160, 160)
PRM = (2.0, 1.5, 0.8, 0.3, 0.7, 0.25, False, None)           # the fixture's parameters (ops.LOSS_EXT_PARAMS order)


def event_ms(once, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        once()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def ext_weights(**kw):
    return tuple(float(kw.get(k, 0.0)) for k in ops.LOSS_EXT_TERMS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, c = SHAPE[0], SHAPE[1]
    v = int(np.prod(SHAPE[2:]))
    g = torch.Generator().manual_seed(7)
    logits = (torch.randn(SHAPE, generator=g) * 2.0).cuda()
    label = torch.nn.functional.one_hot(torch.randint(0, c, (n,) + SHAPE[2:], generator=g), c).permute(0, 4, 1, 2, 3).float().contiguous().cuda()
    dl = torch.empty_like(logits)
    one = torch.ones(1, dtype=torch.float32, device="cuda")
    part0 = torch.empty((n, ops.loss_rows(v), ops.loss_k(c)), dtype=torch.float32, device="cuda")
    out0 = torch.empty(4 + c, dtype=torch.float32, device="cuda")
    coef0 = torch.empty(n * c * 2 + 2, dtype=torch.float32, device="cuda")
    part1 = torch.empty((n, ops.loss_rows(v), ops.loss_ext_k(c)), dtype=torch.float32, device="cuda")
    out1 = torch.empty(ops.loss_ext_nout(c), dtype=torch.float32, device="cuda")
    coef1 = torch.empty(ops.loss_ext_ncoef(n, c), dtype=torch.float32, device="cuda")
    dice = (1.0, 0.0, 0.0, 0.0)

    def old():
        ops.seg_loss_fwd(logits, label, None, None, dice, True, part0, out0, coef0)
        ops.seg_loss_bwd(logits, label, None, coef0, one, dice, True, dl)

    def ext(terms, w7):
        cfg = ops.loss_ext_cfg(terms, (w7, PRM), c)

        def once():
            ops.seg_loss_ext_fwd(logits, label, None, None, cfg, True, part1, out1, coef1)
            ops.seg_loss_ext_bwd(logits, label, None, coef1, one, cfg, True, dl)
        return once

    none = (0.0, 0.0, 0.0, 0.0)
    allw = ext_weights(focal=1, noise_robust=1, explog=1, gce=1, mae=1, mse=1, slsr=1)
    variants = [
        # name, call, what it adds per voxel and class to the existing pass (forward; backward)
        ("ext: Dice only", ext(dice, ext_weights()), "none; none"),
        ("ext: MSE", ext(none, ext_weights(mse=1)), "none; none"),
        ("ext: NoiseRobustDice", ext(none, ext_weights(noise_robust=1)), "1 powf; 1 powf"),
        ("ext: ExpLog", ext(none, ext_weights(explog=1)), "1 logf + 1 powf; 1 logf + 1 powf"),
        ("ext: GeneralizedCE", ext(none, ext_weights(gce=1)), "1 powf; 1 powf"),
        ("ext: FocalDice", ext(none, ext_weights(focal=1)), "none (powf in the one-thread finalize); none"),
        ("ext: all eleven terms", ext((0.5, 0.25, 0.0, 0.125), allw), "3 powf + 2 logf; 3 powf + 3 logf + 1 log2f"),
    ]
    rows = []
    bytes_moved = 4.0 * (2 * 2 * logits.numel() + logits.numel())
    for name, once, adds in variants:
        for _ in range(5):
            once()
            old()
        torch.cuda.synchronize()
        k_ms, o_ms = [], []
        for _ in range(a.rounds):                            # alternating rounds: variant, existing pass, variant, ...
            k_ms.append(event_ms(once, a.iters))
            o_ms.append(event_ms(old, a.iters))
        km, om = float(np.median(k_ms)), float(np.median(o_ms))
        once()
        torch.cuda.synchronize()
        r = dict(name=name, fwd_bwd_ms=round(km, 4), fwd_bwd_ms_min_max=[round(min(k_ms), 4), round(max(k_ms), 4)],
                 existing_dice_ms=round(om, 4), existing_dice_ms_min_max=[round(min(o_ms), 4), round(max(o_ms), 4)],
                 ratio=round(km / om, 3), gbytes_per_s=round(bytes_moved / km / 1e6, 1), transcendentals=adds,
                 loss=float(out1[0].item()), finite=bool(torch.isfinite(dl).all().item()))
        rows.append(r)
        print(json.dumps(r), flush=True)
    res = dict(tool="tools/loss_ext_bench.py --iters %d --rounds %d" % (a.iters, a.rounds), device=torch.cuda.get_device_name(0),
               shape=list(SHAPE),
               note="fwd_bwd_ms: HIP events over back-to-back forward + backward pairs, median of alternating rounds (min and max "
                    "beside it); existing_dice_ms: fplx_seg_loss_fwd + _bwd (Dice) in the same rounds; ratio = the two medians",
               rows=rows)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    if not all(r["finite"] for r in rows):
        raise SystemExit("a variant produced a non-finite gradient")


if __name__ == "__main__":
    main()
