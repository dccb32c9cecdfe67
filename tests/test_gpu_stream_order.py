"""Stream-order audit of the two-stream backward and the gradient exchange (tests/streamorder.py; DESIGN.md, "Stream-order
audit").

(a) the real schedule, two consecutive iterations per route, recorded launch by launch and checked for pairs of launches on
    different streams that share bytes and that no chain of events orders: none may exist; the branches of Engine.backward
    the traces went through are asserted from the traces themselves;
(b) on the recorded traces, on the host: every wait is deleted in turn - the out_conv pair, every convolution site's
    weight-gradient edge and (on the routes without a hook, where nothing else covers it) the final join must each be
    needed; the waits that are not are printed;
(c) engine.backward on one saved forward with the side stream off, on, on with a delay in front of every side-stream launch
    and on with a delay in front of every main-stream launch: the same bits, and the same BatchNorm running statistics and
    parameters after a TrainStep.step.  The delay is twice the measured backward, so the undelayed stream runs as far ahead as
    its waits allow.
"""
import functools
import math
import time

import pytest
import torch

import streamorder as S
from make_golden_cfg import NETS, SHAPES

pytestmark = pytest.mark.gpu

_N32 = dict(in_chns=1, feature_chns=[32, 32, 64, 64, 64], dropout=[0, 0, 0, 0, 0], conv_dims=[3] * 5, class_num=2,
            bilinear=False, num_domains=2, net_type="UNet2D5_dsbn")
_S25 = dict(in_chns=1, feature_chns=[32, 64, 64, 64, 64], dropout=[0.0, 0.0, 0.3, 0.4, 0.5], conv_dims=[2, 2, 3, 3, 3],
            class_num=2, bilinear=False, num_domains=2, net_type="UNet2D5_dsbn")
# name -> (parameters, precision, input shape, Engine attributes)
CONFIGS = {
    "tiny.fp32": (NETS["tiny"], "fp32", SHAPES["tiny"], {}),
    "tiny.bf16": (NETS["tiny"], "bf16", SHAPES["tiny"], {}),
    "tiny25.fp32": (NETS["tiny25"], "fp32", SHAPES["tiny25"], {}),
    "tiny25.bf16": (NETS["tiny25"], "bf16", SHAPES["tiny25"], {}),
    "tinybl.bf16": (NETS["tinybl"], "bf16", SHAPES["tinybl"], {}),
    "tinybl25.fp32": (NETS["tinybl25"], "fp32", SHAPES["tinybl25"], {}),
    "c4.fp32": (NETS["c4"], "fp32", SHAPES["c4"], {}),
    "c4.bf16": (NETS["c4"], "bf16", SHAPES["c4"], {}),
    # 32 channels at level 0, bf16: the fused out_conv (oc_fused, oc_wg), the two-tensor concat, the fused stem site
    "n32.bf16": (_N32, "bf16", (1, 1, 16, 64, 64), {}),
    "n32.stem_side": (_N32, "bf16", (1, 1, 16, 64, 64), {"stem_wgrad_on_main": False}),
    "n32.oc_act": (_N32, "bf16", (1, 1, 16, 64, 64), {"use_outconv_wgrad_bn": False}),      # oc_fused without oc_wg
    "n32.oc_plain": (_N32, "bf16", (1, 1, 16, 64, 64), {"use_outconv_fusion": False}),
    # the shipped dimensionality pattern with active dropout: the two-tensor concat at a 2-D level
    "s25.bf16": (_S25, "bf16", (1, 1, 8, 64, 64), {}),
}
BUCKET = 1 << 12
# name -> (route, configuration, options)
AUDITS = {}
for _c in CONFIGS:
    AUDITS["engine." + _c] = ("engine", _c, {})
AUDITS.update({
    "engine.hook.tiny.bf16": ("engine", "tiny.bf16", {"hook": True}),
    "step.tiny.bf16": ("step", "tiny.bf16", {}),
    "step.n32.bf16": ("step", "n32.bf16", {}),
    "step.s25.bf16": ("step", "s25.bf16", {}),
    "step_all.tiny25.bf16": ("step_all", "tiny25.bf16", {}),
    "step_all.n32.bf16": ("step_all", "n32.bf16", {}),
    "autograd.s25.bf16": ("autograd", "s25.bf16", {}),
    "step.reducer.tiny.fp32": ("step", "tiny.fp32", {"reducer": True}),
    "step.reducer.n32.bf16": ("step", "n32.bf16", {"reducer": True}),
    "step_all.reducer.overlap.n32.bf16": ("step_all", "n32.bf16", {"reducer": True, "overlap": True}),
    "step_all.reducer.overlap.s25.bf16": ("step_all", "s25.bf16", {"reducer": True, "overlap": True}),
    "step_all.reducer.serial.n32.bf16": ("step_all", "n32.bf16", {"reducer": True, "overlap": False}),
    "step.one_stream.n32.bf16": ("step", "n32.bf16", {"side": False}),
    "step_all.reducer.one_stream.tiny.bf16": ("step_all", "tiny.bf16", {"reducer": True, "overlap": True, "side": False}),
})
SIDE_REQUIRED = {"fplx_conv3d_wgrad", "fplx_conv2d_wgrad", "fplx_conv3d_wgrad_cat2", "fplx_deconv2_wgrad", "fplx_stem_wgrad_bn",
                 "fplx_outconv_wgrad_bn"}
# what else the traces must have gone through: the 2-D two-tensor site on the side stream; on the main stream the stem's
# weight gradient in its three forms (wgrad_here), both split data gradients, the fused and the plain pool tail, the
# bilinear and the transposed up-sampling, the fused out_conv passes and the stored-gradient form
SIDE_ALSO = {"fplx_conv2d_wgrad_cat2"}
MAIN_REQUIRED = {"fplx_stem_wgrad_bn", "fplx_conv3d_wgrad", "fplx_conv2d_wgrad", "fplx_conv3d_dgrad_split2", "fplx_conv2d_dgrad_split2",
                 "fplx_pool_bwd_bn_reduce", "fplx_maxpool2_bwd", "fplx_upsample2_bwd", "fplx_deconv2_dgrad",
                 "fplx_outconv_dgrad_bn_reduce", "fplx_outconv_dgrad_bn_apply", "fplx_bn_act_bwd_apply", "fplx_optim_step",
                 "fplx_optim_pack_step"}
# the waits in front of these side-stream launches are the convolution sites' (and out_conv's) weight-gradient edges
SITE_WGRADS = {"fplx_conv3d_wgrad", "fplx_conv2d_wgrad", "fplx_conv3d_wgrad_cat2", "fplx_conv2d_wgrad_cat2", "fplx_stem_wgrad_bn",
               "fplx_outconv_wgrad_bn"}


def _build(cfg, seed=3):
    import fplx
    p, prec, shape, attrs = CONFIGS[cfg]
    torch.manual_seed(seed)
    net = fplx.UNet2D5_dsbn(dict(p, precision=prec)).cuda()
    for k, v in attrs.items():
        assert hasattr(net.engine, k), k
        setattr(net.engine, k, v)
    net.train()
    net._ensure_flat()
    net.dropout_seed, net._fwd_counter = 9, 0
    g = torch.Generator().manual_seed(11)
    n, _, d, h, w = shape
    ncls = p["class_num"]
    batches = []
    for dmn in range(2):
        x = torch.randn(*shape, generator=g)
        idx = torch.zeros((n, d, h, w), dtype=torch.long)
        idx[:, d // 4:d // 2 + 1, h // 4:h // 2, w // 3:2 * w // 3] = 1 + dmn % (ncls - 1)
        lab = torch.nn.functional.one_hot(idx, ncls).permute(0, 4, 1, 2, 3).float().contiguous()
        x[:, 0] += 2.0 * lab[:, 1]
        batches.append({"image": x.cuda(), "label_prob": lab.cuda()})
    return net, batches


def _record(route, cfg, opt):
    """two iterations of one route under the tracer -> (trace, main stream, end of each iteration in the trace, tracer)"""
    import fplx
    net, bs = _build(cfg)
    eng = net.engine
    eng.use_side_stream = opt.get("side", True)
    ts = None
    if route in ("step", "step_all"):
        ts = fplx.TrainStep(net, (1.0, 0.0, 0.0, 0.0), True, lr=1e-3, weight_decay=1e-5, bucket_elems=BUCKET)
        if opt.get("reducer"):
            ts.reducer = S.standin_reducer(ts.reducer.buckets, ts.reducer.domain_ranges)
            ts.overlap_all = bool(opt.get("overlap", True))
            assert len(ts.reducer.buckets) >= 4
    dl = gflat = probe = None
    if route == "engine":
        logits, _ = eng.forward(bs[0]["image"], 0, True, net.dropout_active(), net.dropout_seed, 0, keep=False)
        dl = torch.randn(logits.shape, generator=torch.Generator().manual_seed(5)).cuda()
        gflat = torch.empty_like(net.flat_params)
        probe = torch.zeros(1, device="cuda")
    torch.cuda.synchronize()
    main = int(torch.cuda.current_stream().cuda_stream)
    ends = []
    launched = []
    with S.Tracer() as tr:
        for it in range(2):
            if route == "engine":
                logits, sv = eng.forward(bs[it]["image"], it, True, net.dropout_active(), net.dropout_seed, it, keep=True)
                hook = None
                if opt.get("hook"):           # a plain callable: Engine.backward joins the side stream in front of every call
                    hook = lambda end: probe.add_(gflat[:end].abs().max())
                eng.backward(sv, dl.clone(), gflat, hook)
                probe.add_(gflat.sum())       # the consumer of the result
                del sv, logits
            elif route == "step":
                ts.step(bs[it]["image"], bs[it]["label_prob"], it)
            elif route == "step_all":
                ts.step_all(bs)
            else:
                for q in net.parameters():
                    q.grad = None
                out = net(bs[it]["image"], domain_label=it * torch.ones(bs[it]["image"].shape[0], dtype=torch.long))
                fplx.DiceLoss()({"prediction": out, "ground_truth": bs[it]["label_prob"]}).backward()
                torch.cat([q.grad.reshape(-1) for q in net.parameters() if q.grad is not None])
                del out
            if ts is not None and opt.get("reducer"):
                launched.append(list(ts.reducer.launched))
            ends.append(len(tr.trace))
    torch.cuda.synchronize()
    return tr.trace, main, ends, tr, launched


@functools.lru_cache(maxsize=None)
def audit(name):
    route, cfg, opt = AUDITS[name]
    t0 = time.time()
    trace, main, ends, tr, launched = _record(route, cfg, opt)
    conflicts = S.check(trace)
    names = {}
    for r in trace:
        if r[0] == "launch":
            names.setdefault(r[1], set()).add(r[2])
    side = [s for s in names if s not in (main, S.COMM)]
    print("%s: %d records, %d launches (%d on the side stream, %d collectives), %d waits, %d pointers resolved to their "
          "allocator block, %d conflicts, %.2f s" % (
              name, len(trace), sum(1 for r in trace if r[0] == "launch"),
              sum(1 for r in trace if r[0] == "launch" and r[1] in side), sum(1 for r in trace if r[0] == "launch" and r[1] == S.COMM),
              len(S.waits(trace)), tr.block_resolved, len(conflicts), time.time() - t0))
    for c in conflicts[:24]:
        print("    %s: %s @%d on %s  <->  %s @%d on %s" % (c.kind, c.first_name, c.first_pos, _sname(c.first_stream, main),
                                                           c.second_name, c.second_pos, _sname(c.second_stream, main)))
    return dict(trace=trace, main=main, ends=ends, conflicts=conflicts, names=names, side=side, launched=launched)


def _sname(s, main):
    return "main" if s == main else ("comm" if s == S.COMM else "side")


# --------------------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("name", list(AUDITS))
def test_schedule_has_no_unordered_conflict(name):
    a = audit(name)
    route, cfg, opt = AUDITS[name]
    assert a["names"].get(a["main"]), "nothing was recorded on the main stream"
    if opt.get("side", True):
        assert len(a["side"]) == 1, a["side"]
        assert a["names"][a["side"][0]] & S_WGRAD_ANY, "no weight gradient was seen on the side stream"
    else:
        # one stream: nothing can conflict - a tracer that mis-read the stream argument would show here
        assert a["side"] == [], a["side"]
    if opt.get("reducer"):
        assert S.COMM in a["names"] and all(len(l) >= 5 for l in a["launched"]), a["launched"]
        folds = a["names"].get(a["side"][0], set()) if a["side"] else set()
        if route == "step_all" and opt.get("overlap") and opt.get("side", True):
            assert "aten::add_" in folds, "the reducer's fold was not launched from the side stream"
    assert a["conflicts"] == [], "%d conflicts, first: %s" % (len(a["conflicts"]), a["conflicts"][:4])


S_WGRAD_ANY = SITE_WGRADS | {"fplx_deconv2_wgrad"}


def test_every_branch_of_backward_was_traced():
    side, main_names = set(), set()
    for name in AUDITS:
        a = audit(name)
        for s in a["side"]:
            side |= a["names"][s]
        main_names |= a["names"][a["main"]]
    assert SIDE_REQUIRED <= side, sorted(SIDE_REQUIRED - side)
    assert SIDE_ALSO <= side, sorted(SIDE_ALSO - side)
    assert MAIN_REQUIRED <= main_names, sorted(MAIN_REQUIRED - main_names)
    # per configuration, from its own trace: what the configuration is there for
    def side_of(n):
        a = audit(n)
        return set().union(*[a["names"][s] for s in a["side"]]) if a["side"] else set()
    def main_of(n):
        a = audit(n)
        return a["names"][a["main"]]
    assert "fplx_outconv_wgrad_bn" in side_of("engine.n32.bf16") and "fplx_stem_wgrad_bn" in main_of("engine.n32.bf16")
    assert "fplx_stem_wgrad_bn" in side_of("engine.n32.stem_side")
    assert "fplx_outconv_dgrad_bn_apply" in main_of("engine.n32.oc_act") and "fplx_outconv_wgrad_bn" not in side_of("engine.n32.oc_act")
    assert "fplx_outconv_dgrad_bn_apply" not in main_of("engine.n32.oc_plain")
    assert "fplx_conv2d_wgrad_cat2" in side_of("engine.s25.bf16") and "fplx_conv2d_dgrad_split2" in main_of("engine.s25.bf16")
    assert "fplx_upsample2_bwd" in main_of("engine.tinybl.bf16") and "fplx_upsample2_bwd" in main_of("engine.tinybl25.fp32")
    assert "fplx_maxpool2_bwd" in main_of("engine.tiny.fp32") and "fplx_pool_bwd_bn_reduce" in main_of("engine.tiny.bf16")
    assert "fplx_conv2d_wgrad" in side_of("engine.tiny25.fp32") and "fplx_conv2d_wgrad" in main_of("engine.tiny25.fp32")


def test_schedule3d_runs_on_one_stream():
    """fplx.nets3d.Schedule3D: one stream by design - one stream seen, nothing to conflict"""
    import fplx
    import kinkoracle as K
    case = K.n3d_case("u25")
    p = dict(case.params, precision="fp32")
    net = fplx.SegNetDict[p["net_type"]](p)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in case.weights.items()}, strict=True)
    net.cuda().train()
    net._ensure_flat()
    x = case.x.cuda()
    gflat = torch.empty_like(net.flat_params)
    torch.cuda.synchronize()
    with S.Tracer() as tr:
        for it in range(2):
            outs, sv = net.engine.forward(x, True, list(net.dropout_active()), net.dropout_seed, it, True)
            net.engine.backward(sv, [torch.ones_like(o) for o in outs], gflat)
            gflat.sum()
    torch.cuda.synchronize()
    assert sum(1 for r in tr.trace if r[0] == "launch" and r[2].startswith("fplx_")) > 40
    assert len(S.streams_of(tr.trace)) == 1 and S.check(tr.trace) == []


# --------------------------------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("name", [n for n in AUDITS if AUDITS[n][2].get("side", True)])
def test_every_required_edge_is_needed(name):
    a = audit(name)
    trace, main, side = a["trace"], a["main"], a["side"][0]
    assert a["conflicts"] == []
    required, redundant, n_site = [], [], 0
    joins = [p for p in S.waits(trace) if trace[p][1] == main and S.describe_wait(trace, p)[2] == side]
    final = {max(p for p in joins if p < end) for end in a["ends"]}          # the last join of each iteration
    assert len(final) == 2
    # With a reducer every bucket is launched from the side stream, the communication stream waits for that, and finish()
    # makes the main stream wait for the communication stream: the side stream's work is ordered in front of the optimiser
    # through that chain as well.  With a plain callable the last ready() has joined already.  The final join is then
    # covered twice and is required only on the routes without a hook.
    final_needed = not AUDITS[name][2].get("reducer") and not AUDITS[name][2].get("hook")
    removed = S.check_each_wait_removed(trace)
    for pos in S.waits(trace):
        s, nxt, src, prev = S.describe_wait(trace, pos)
        broken = removed[pos]
        # on_side(): record, wait, launch - the launch is the very next record (ready()'s own edge is followed by the fold or
        # by the collective's records instead)
        after = trace[pos + 1] if pos + 1 < len(trace) else ("",)
        site_edge = s == side and src == main and after[0] == "launch" and after[1] == side and after[2] in SITE_WGRADS
        if site_edge:
            n_site += 1
        if site_edge or (pos in final and final_needed):
            required.append((pos, nxt, prev, len(broken)))
        if not broken:
            redundant.append("@%d %s waits for %s: behind %s, in front of %s" % (pos, _sname(s, main), _sname(src, main) if src is not None
                                                                                 else "?", prev, nxt))
    print("%s: %d waits, %d required (%d site edges, %d final joins), %d whose removal shows no conflict" % (
        name, len(S.waits(trace)), len(required), n_site, len(final) if final_needed else 0, len(redundant)))
    for r in redundant:
        print("    redundant: " + r)
    assert n_site >= 2 * 18                    # out_conv + 18 convolution sites less the stem's when it runs on the main stream
    bad = [r for r in required if r[3] == 0]
    assert not bad, "required edges whose removal produces no conflict (position, next launch, launch behind the record, conflicts): %s" % bad


# --------------------------------------------------------------------------------------------------------------------- (c)
def _cycles_per_ms():
    """torch.cuda._sleep cycles per millisecond, as the slope between two spin lengths (the launch overhead drops out); the
    FASTEST of three measurements each, so that the figure can only be too high - the delays' computed sum too low"""
    def ms(c):
        best = None
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch.cuda._sleep(int(c))
            e1.record()
            e1.synchronize()
            t = e0.elapsed_time(e1)
            best = t if best is None or t < best else best
        return best
    c = 1 << 16
    while ms(c) < 2.0:
        c *= 2
        assert c < 1 << 34
    t1, t4 = ms(c), ms(4 * c)
    return 3 * c / (t4 - t1)


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_four_timings_give_the_same_bits(cfg):
    import fplx
    t_start = time.time()
    net, bs = _build(cfg)
    eng = net.engine
    x, lab = bs[0]["image"], bs[0]["label_prob"]
    logits, sv = eng.forward(x, 0, True, net.dropout_active(), net.dropout_seed, 0, keep=True)
    dl = torch.randn(logits.shape, generator=torch.Generator().manual_seed(5)).cuda()
    main = int(torch.cuda.current_stream().cuda_stream)

    def backward(side_on, delay=None):
        eng.use_side_stream = side_on
        gflat = torch.empty_like(net.flat_params)
        d = dl.clone()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with S.Tracer(torch_ops=False, events=False, collective=False, delay=delay) as tr:
            tr.delay_on = True
            e0.record()
            eng.backward(sv, d, gflat)
            e1.record()
        torch.cuda.synchronize()
        return gflat, e0.elapsed_time(e1), tr

    backward(True)                                                 # workspaces, the side stream, the allocator's pools
    times = sorted(backward(True)[1] for _ in range(3))
    bwd_ms = times[1]
    cyc = _cycles_per_ms()
    delay = int(math.ceil(2.0 * bwd_ms * cyc))
    off, _, tr_off = backward(False)
    on, _, tr_on = backward(True)
    side_d, side_ms, tr_s = backward(True, ("side", delay, main))
    main_d, main_ms, tr_m = backward(True, ("main", delay, main))
    n_side = sum(1 for r in tr_on.trace if r[0] == "launch" and r[1] != main)
    n_main = sum(1 for r in tr_on.trace if r[0] == "launch" and r[1] == main)
    print("%s: backward %.3f ms (three runs: %s), %.0f sleep cycles per ms, delay %d cycles = %.3f ms; %d side-stream launches "
          "delayed: %.1f ms, %d main-stream launches delayed: %.1f ms" % (
              cfg, bwd_ms, ", ".join("%.3f" % t for t in times), cyc, delay, delay / cyc, tr_s.delays, side_ms, tr_m.delays, main_ms))
    assert {r[1] for r in tr_off.trace if r[0] == "launch"} == {main}
    assert n_side >= 15 and (tr_s.delays, tr_m.delays) == (n_side, n_main)
    assert side_ms >= tr_s.delays * delay / cyc and main_ms >= tr_m.delays * delay / cyc       # the delays really executed
    assert torch.equal(on, off), "side stream on / off differ in %d elements" % int((on != off).sum())
    assert torch.equal(side_d, off), "delayed side stream: %d elements differ" % int((side_d != off).sum())
    assert torch.equal(main_d, off), "delayed main stream: %d elements differ" % int((main_d != off).sum())
    del sv

    # ---- one TrainStep.step per timing on a fresh network: gradients, parameters, BatchNorm running statistics
    results = []
    for side_on, which in ((False, None), (True, None), (True, "side"), (True, "main")):
        net2, _ = _build(cfg)
        net2.engine.use_side_stream = side_on
        ts = fplx.TrainStep(net2, (1.0, 0.0, 0.0, 0.0), True, lr=1e-3, weight_decay=1e-5)
        with S.Tracer(torch_ops=False, events=False, collective=False, delay=None if which is None else (which, delay, main)) as tr:
            real = net2.engine.backward

            def bwd(*a, **k):
                tr.delay_on = True                             # the delays belong to backward: the forward has one stream
                try:
                    return real(*a, **k)
                finally:
                    tr.delay_on = False
            net2.engine.backward = bwd
            out = ts.step(x, lab, 0)
        torch.cuda.synchronize()
        assert which is None or tr.delays > 0
        sd = net2.state_dict()
        stats = [sd[k] for k in sorted(sd) if "running_" in k or "num_batches" in k]
        assert len(stats) >= 3 * 18
        results.append([out, ts.gflat, net2.flat_params.detach()] + stats)
    for other, what in zip(results[1:], ("side stream on", "delayed side stream", "delayed main stream")):
        same = [torch.equal(a, b) for a, b in zip(results[0], other)]
        assert all(same), "%s: %d of %d tensors differ from the one-stream step" % (what, same.count(False), len(same))
    print("%s: test run time %.2f s" % (cfg, time.time() - t_start))
