"""Secondary measurement (not a bench.py line), as tools/ssl_bench.py: URPC's pyramid consistency (fplx_ssl_pyramid_fwd / _bwd,
K = 4 output scales) and CPS's pseudo labels (fplx_ssl_pseudo_onehot, two networks) against the torch compositions they replace
- the reference's own statements (ssl_urpc.py:76-91, ssl_cps.py:94,103-106) on the GPU, autograd for the backward - at the
logit shape of tools/ssl_bench.py.  Both sides run in ONE process in alternating rounds: HIP events around `iters` back-to-back
calls into warmed-up buffers, the median over the rounds with minimum and maximum beside it.  `bytes` is what the algorithm has
to move: the forward reads K C M floats, the backward reads them again and writes as many, the one-hot pass reads and writes
K C M; `hbm_fraction` is the resulting rate over 6.05 TB/s; `ratio` is the torch median over the fused
median of the same rounds (above 1: the kernel is faster).  The backward alone has no torch counterpart that runs by itself: its
row compares the fused kernel with the difference of torch's forward + backward and forward medians.
usage: python tools/ssl2_bench.py [--iters N] [--rounds N] [--out FILE.json]"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from ssl_bench import SHAPE, BN_PASS_RATE, event_us  # noqa: E402  (also puts the package and tests/golden on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from fplx import ops  # noqa: E402

K_URPC, K_CPS = 4, 2


def torch_urpc(outputs_list):
    """ssl_urpc.py:76-91 over tensors that hold the unlabelled rows only"""
    kl_distance = torch.nn.KLDivLoss(reduction='none')
    outputs_soft_list = [torch.softmax(item, dim=1) for item in outputs_list]
    p1_avg = torch.mean(torch.stack(outputs_soft_list), dim=0) * 0.99 + 0.005
    loss_reg = 0.0
    for soft_i in outputs_soft_list:
        p1_i = soft_i * 0.99 + 0.005
        var = torch.sum(kl_distance(torch.log(p1_i), p1_avg), dim=1, keepdim=True)
        exp_var = torch.exp(-var)
        square_e = torch.square(p1_avg - p1_i)
        loss_reg = loss_reg + torch.mean(square_e * exp_var) / (torch.mean(exp_var) + 1e-8) + torch.mean(var)
    return loss_reg / len(outputs_list)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/ssl2_bench.py measures on the GPU; none is visible")
    if a.rounds < 5:
        raise SystemExit("tools/ssl2_bench.py: at least 5 rounds")
    n, c = SHAPE[0], SHAPE[1]
    v = int(np.prod(SHAPE[2:]))
    ncv = n * c * v
    g = torch.Generator().manual_seed(7)
    base = torch.randn(SHAPE, generator=g) * 1.5
    logits = [(base + 0.5 * torch.randn(SHAPE, generator=g)).cuda() for _ in range(K_URPC)]
    one = torch.ones(1, dtype=torch.float32, device="cuda")
    part = ops.ssl_part(logits[0], 3 * K_URPC)
    out = torch.empty(4 * K_URPC + 2, dtype=torch.float64, device="cuda")
    grads = [torch.empty_like(t) for t in logits]
    onehot = [torch.empty_like(t) for t in logits[:K_CPS]]

    def fused_fwd():
        ops.ssl_pyramid_fwd(logits, part, out)

    def torch_fwd():
        with torch.no_grad():
            return torch_urpc(logits)

    def fused_bwd():
        ops.ssl_pyramid_bwd(logits, out, one, grads)

    def fused_pair():
        fused_fwd()
        fused_bwd()

    def torch_pair():
        ls = [t.detach().requires_grad_(True) for t in logits]
        torch_urpc(ls).backward()
        return [t.grad for t in ls]

    def fused_onehot():
        ops.ssl_pseudo_onehot(logits[:K_CPS], onehot)

    def torch_onehot():
        res = []
        for t in logits[:K_CPS]:
            idx = torch.argmax(torch.softmax(t, dim=1), dim=1, keepdim=True)
            res.append(torch.zeros_like(t).scatter_(1, idx, 1.0))         # get_soft_label's one-hot
        return res

    # same numbers first: the fused pair against torch's on these very inputs
    fused_pair()
    ref = torch_pair()
    agree = dict(loss_abs_diff=abs(float(out[4 * K_URPC]) - float(torch_fwd())),
                 grad_max_abs_diff=max(float((a_ - b_).abs().max()) for a_, b_ in zip(grads, ref)),
                 grad_max_abs=max(float(b_.abs().max()) for b_ in ref))
    fused_onehot()
    agree["onehot_equal"] = all(bool(torch.equal(a_, b_)) for a_, b_ in zip(onehot, torch_onehot()))
    del ref
    f4 = 4.0
    variants = [
        ("pyramid consistency fwd, K = %d" % K_URPC, fused_fwd, torch_fwd, f4 * K_URPC * ncv),
        ("pyramid consistency fwd + bwd, K = %d" % K_URPC, fused_pair, torch_pair, f4 * 3 * K_URPC * ncv),
        ("pyramid consistency bwd alone, K = %d (torch: pair - fwd)" % K_URPC, fused_bwd, None, f4 * 2 * K_URPC * ncv),
        ("pseudo one-hot, %d networks" % K_CPS, fused_onehot, torch_onehot, f4 * 2 * K_CPS * ncv),
    ]
    rows, torch_meds = [], []
    for name, fused, ref_fn, nbytes in variants:
        for _ in range(3):
            fused()
            if ref_fn is not None:
                ref_fn()
        torch.cuda.synchronize()
        f_us, r_us = [], []
        for _ in range(a.rounds):                            # alternating rounds: kernel, torch, kernel, ...
            f_us.append(event_us(fused, a.iters))
            if ref_fn is not None:
                r_us.append(event_us(ref_fn, a.iters))
        fm = float(np.median(f_us))
        if ref_fn is None:                                   # the backward alone: torch's pair minus torch's forward
            rm = torch_meds[1] - torch_meds[0]
        else:
            rm = float(np.median(r_us))
        torch_meds.append(rm)
        r = dict(name=name, fused_us=round(fm, 2), fused_us_min_max=[round(min(f_us), 2), round(max(f_us), 2)],
                 torch_us=round(rm, 2), torch_us_min_max=[round(min(r_us), 2), round(max(r_us), 2)] if r_us else None,
                 ratio=round(rm / fm, 2), bytes=int(nbytes), tbytes_per_s=round(nbytes / fm / 1e6, 3),
                 hbm_fraction=round(nbytes / (fm * 1e-6) / BN_PASS_RATE, 3), beats_torch=bool(fm < rm))
        rows.append(r)
        print(json.dumps(r), flush=True)
    res = dict(tool="tools/ssl2_bench.py --iters %d --rounds %d" % (a.iters, a.rounds), device=torch.cuda.get_device_name(0),
               shape=list(SHAPE), scales=K_URPC, agreement=agree,
               note="us per call: HIP events over back-to-back calls, median of alternating rounds; bytes: algorithmic (fwd K C M "
                    "floats read; bwd that read again and as many written); hbm_fraction: bytes / fused time over 6.05 TB/s "
                    "(DESIGN section 5)",
               rows=rows)
    print(json.dumps(dict(agreement=agree)), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
