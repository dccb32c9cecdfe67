"""Secondary measurement (not a bench.py line): the fused optimiser launch of every kind (fplx_optim_pack_step, csrc/conv_generic.hip)
against Adam's existing one (fplx_adam_pack_step) on the shared segment of the benchmark network (bf16, pack plan on): the update
of all shared parameters plus the bf16 packs and stamps of the 3x3x3 layers in ONE launch.
Every kind is timed in alternating rounds with Adam's launch in the same process: HIP events around `iters` back-to-back
launches after warm-up; the median over the rounds is reported with the minimum and maximum beside it, `ratio` is the kind's
median over Adam's median of the SAME rounds, and `adam_spread` is Adam's own (max - min) / median over those rounds - a ratio
inside 1 +- that spread says nothing.  Algorithmic bytes per element: 4 (p read) + 4 (g read) + 4 (p written) + 8 per state
stream (read + written): SGD without momentum 12, SGD / Adagrad / ASGD / RMSprop without momentum 20, the others and Adam 28;
the packs add 2 x 2 bytes per 3x3x3 weight to every row alike and are counted in `gbytes_per_s`.
usage: python tools/optim_bench.py [--iters N] [--rounds N] [--out FILE.json]"""
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

NET = dict(in_chns=1, feature_chns=[32, 64, 128, 256, 512], dropout=[0.0, 0.0, 0.3, 0.4, 0.5], conv_dims=[3, 3, 3, 3, 3],
           class_num=2, bilinear=False, num_domains=2, precision="bf16", net_type="UNet2D5_dsbn")
# name, hyper-parameters in fplx_optim_step's order (torch's defaults behind lr 1e-3, weight decay 1e-5), state streams
KINDS = [("SGD", (1e-3, 0.0, 1e-5), 0), ("SGD", (1e-3, 0.9, 1e-5), 1), ("Adadelta", (1.0, 0.9, 1e-6, 1e-5), 2),
         ("Adagrad", (1e-2, 0.0, 1e-10, 1e-5), 1), ("Adamax", (2e-3, 0.9, 0.999, 1e-8, 1e-5), 2),
         ("ASGD", (1e-2, 1.0, 1e-4, 1e-5), 1), ("RMSprop", (1e-2, 0.99, 1e-8, 0.0, 1e-5), 1),
         ("RMSprop", (1e-2, 0.99, 1e-8, 0.9, 1e-5), 2), ("Rprop", (1e-2, 0.5, 1.2, 1e-6, 50.0), 2)]


def event_ms(once, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        once()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(3)
    net = fplx.UNet2D5_dsbn(dict(NET)).cuda()
    net._ensure_flat()
    (start, end), _ = net.segments()
    plan = net.engine.adam_pack_plan()
    assert plan and start == 0
    n = end - start
    packed = sum(l[1] * l[2] * 27 for l in plan)
    p0 = net.flat_params.detach()[start:end].clone()
    p = p0.clone()
    g = (torch.randn(n, generator=torch.Generator().manual_seed(7)) * 1e-3).cuda()
    s0, s1 = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")

    def adam():
        ops.adam_pack_step(p, g, s0, s1, 1e-3, 2, 1e-5, 1.0, (0.9, 0.999), 1e-8, plan)

    def kind_call(kind, hp, ns):
        def once():
            ops.optim_pack_step(kind, p, g, s0 if ns > 0 else None, s1 if ns > 1 else None, hp, 2, 1.0, plan)
        return once

    def reset():
        p.copy_(p0)
        s0.fill_(1e-6)
        s1.fill_(1e-6)

    rows = []
    for kind, hp, ns in KINDS:
        once = kind_call(kind, hp, ns)
        reset()
        for _ in range(5):
            once()
            adam()
        torch.cuda.synchronize()
        k_ms, a_ms = [], []
        for _ in range(a.rounds):                            # alternating rounds: the kind, Adam, the kind, ...
            reset()
            k_ms.append(event_ms(once, a.iters))
            reset()
            a_ms.append(event_ms(adam, a.iters))
        km, am = float(np.median(k_ms)), float(np.median(a_ms))
        bpe = 12 + 8 * ns
        r = dict(kind=kind, hp=list(hp), state_streams=ns, bytes_per_element=bpe, us=round(km * 1e3, 2),
                 us_min_max=[round(min(k_ms) * 1e3, 2), round(max(k_ms) * 1e3, 2)], adam_us=round(am * 1e3, 2),
                 adam_us_min_max=[round(min(a_ms) * 1e3, 2), round(max(a_ms) * 1e3, 2)], ratio=round(km / am, 3),
                 adam_spread=round((max(a_ms) - min(a_ms)) / am, 3),
                 gbytes_per_s=round((bpe * n + 4.0 * packed) / km / 1e6, 1),
                 adam_gbytes_per_s=round((28.0 * n + 4.0 * packed) / am / 1e6, 1), finite=bool(torch.isfinite(p).all().item()))
        rows.append(r)
        print(json.dumps(r), flush=True)
    res = dict(tool="tools/optim_bench.py --iters %d --rounds %d" % (a.iters, a.rounds), device=torch.cuda.get_device_name(0),
               elements=n, packed_elements=packed, layers=len(plan),
               note="us: HIP events over back-to-back fused launches, median of alternating rounds (min and max beside it); "
                    "adam_us: fplx_adam_pack_step in the same rounds; ratio = the two medians; adam_spread = Adam's (max - min) / "
                    "median over those rounds", rows=rows)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    if not all(r["finite"] for r in rows):
        raise SystemExit("a kind produced a non-finite parameter")


if __name__ == "__main__":
    main()
