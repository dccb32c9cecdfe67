"""Secondary measurement (not a bench.py line): the noisy-label node of fplx.nll (csrc/nll.hip on fplx_select_kth), forward +
backward, against the torch composition it replaces - the reference's own statements (nll_co_teaching.py:91-118,
nll_trinet.py:66-120) on the GPU with autograd - at the benchmark's logit shape 2 x 2 x 80 x 160 x 160, both modes, and
select_mask alone (selection + mask) against torch.argsort / torch.quantile.
Both sides run in ONE process in alternating rounds: HIP events around `iters` back-to-back calls into warmed-up buffers, the
median over the rounds with minimum and maximum beside it; `ratio` is the torch median over the fused median of the same rounds
(above 1: the kernels are faster).  No ratio is a pass condition.
usage: python tools/nll_bench.py [--iters N] [--rounds N] [--out FILE.json]"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in ("..", os.path.join("..", "fpl-plus_amd")):
    sys.path.insert(0, os.path.join(HERE, p))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import fplx  # noqa: E402
from fplx import ops  # noqa: E402

SHAPE = (2, 2, 80, 160, 160)
RATIO = 0.8


def event_us(once, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        once()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters


def reshape_tensor_to_2D(x):
    """loss/seg/util.py: [N, C, D, H, W] -> [N D H W, C]"""
    c = x.shape[1]
    return x.reshape(x.shape[0], c, -1).permute(0, 2, 1).reshape(-1, c)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/nll_bench.py measures on the GPU; none is visible")
    n, c = SHAPE[0], SHAPE[1]
    nv = n * int(np.prod(SHAPE[2:]))
    g = torch.Generator().manual_seed(7)
    base = torch.randn(SHAPE, generator=g) * 1.5
    logits = [(base + 0.7 * torch.randn(SHAPE, generator=g)).cuda() for _ in range(3)]
    cls = base.argmax(1, keepdim=True)
    flip = torch.rand(cls.shape, generator=g) < 0.25
    cls = torch.where(flip, torch.randint(0, c, cls.shape, generator=g), cls)
    labels = torch.zeros(SHAPE).scatter_(1, cls, 1.0).cuda()
    y_2d = reshape_tensor_to_2D(labels)

    def voxel_loss(o):
        prob_2d = reshape_tensor_to_2D(torch.nn.Softmax(dim=1)(o)) * 0.999 + 5e-4
        return torch.sum(-y_2d * torch.log(prob_2d), dim=1)

    def fused_node(mode, k):
        def run():
            ls = [t.detach().requires_grad_(True) for t in logits[:k]]
            fplx.selective_ce_loss(ls, labels, mode, RATIO).backward()
            return ls[0].grad
        return run

    def torch_co():
        o1, o2 = [t.detach().requires_grad_(True) for t in logits[:2]]
        loss1, loss2 = voxel_loss(o1), voxel_loss(o2)
        ind_1_sorted, ind_2_sorted = torch.argsort(loss1), torch.argsort(loss2)
        num_remb = int(RATIO * len(loss1))
        (loss1[ind_2_sorted[:num_remb]].mean() + loss2[ind_1_sorted[:num_remb]].mean()).backward()
        return o1.grad

    def torch_tri():
        os_ = [t.detach().requires_grad_(True) for t in logits]
        ls, ms = [], []
        for o in os_:
            loss = voxel_loss(o)
            ls.append(loss)
            ms.append(loss < torch.quantile(loss, RATIO))
        m12, m13, m23 = (ms[0] * ms[1]).detach(), (ms[0] * ms[2]).detach(), (ms[1] * ms[2]).detach()
        ((torch.sum(ls[0] * m23) / m23.sum() + torch.sum(ls[1] * m13) / m13.sum() + torch.sum(ls[2] * m12) / m12.sum()) / 3).backward()
        return os_[0].grad

    with torch.no_grad():
        loss0 = voxel_loss(logits[0]).contiguous()
    mask = torch.empty(nv, dtype=torch.uint8, device="cuda")
    num_remb = int(RATIO * nv)

    variants = [
        ("CoTeaching node fwd + bwd (2 networks)", fused_node("CoTeaching", 2), torch_co),
        ("TriNet node fwd + bwd (3 networks)", fused_node("TriNet", 3), torch_tri),
        ("select_mask RANK (select_kth + count, scan, write) vs argsort[:k]",
         lambda: ops.nll_select_mask(loss0, ops.NLL_RANK, num_remb=num_remb, mask=mask), lambda: torch.argsort(loss0)[:num_remb]),
        ("select_mask BELOW (select_kth + compare) vs loss < quantile",
         lambda: ops.nll_select_mask(loss0, ops.NLL_BELOW, q=RATIO, mask=mask), lambda: loss0 < torch.quantile(loss0, RATIO)),
    ]
    rows = []
    for name, fused, ref in variants:
        for _ in range(3):
            fused()
            ref()
        torch.cuda.synchronize()
        f_us, r_us = [], []
        for _ in range(a.rounds):                            # alternating rounds: kernels, torch, kernels, ...
            f_us.append(event_us(fused, a.iters))
            r_us.append(event_us(ref, a.iters))
        fm, rm = float(np.median(f_us)), float(np.median(r_us))
        r = dict(name=name, fused_us=round(fm, 2), fused_us_min_max=[round(min(f_us), 2), round(max(f_us), 2)],
                 torch_us=round(rm, 2), torch_us_min_max=[round(min(r_us), 2), round(max(r_us), 2)], ratio=round(rm / fm, 2),
                 beats_torch=bool(fm < rm))
        rows.append(r)
        print(json.dumps(r), flush=True)
    res = dict(tool="tools/nll_bench.py --iters %d --rounds %d" % (a.iters, a.rounds), device=torch.cuda.get_device_name(0),
               shape=list(SHAPE), voxels=nv, ratio=RATIO,
               note="us per call (a fwd + bwd pair for the nodes): HIP events over back-to-back calls, median of alternating rounds",
               rows=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
