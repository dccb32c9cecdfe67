"""-m gpu: the seven optimiser kinds of fplx_optim_step / fplx_optim_pack_step and the classes on top of them (fplx/optim.py)
against tests/optimoracle.py: the float64 bound on random data (Rprop: bitwise), torch bit for bit on the exact data, zero
gradients, the pack-fused launch against update + pack, TrainStep and SegmentationAgent with a foreign-to-Adam optimiser,
checkpoints both ways, the ABI's refusals, and the eighth kind, Adam, bit for bit against the record of the kernels it had before
it joined the family (its bound: tests/test_gpu_loss_exact.py)."""
import os

import numpy as np
import pytest
import torch

import optimoracle as O

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 4, 5, 1023, 10007)
_LINES = []


def _log(case, res):
    line = "%-78s %s" % (case, "  ".join("%s %.3g" % kv for kv in sorted(res.items())))
    print(line)
    _LINES.append(line)


def _place(a, mode):
    """a on the device at a 16-byte-aligned base ('a') or one float behind one ('o')"""
    buf = torch.zeros(a.size + 8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    off = 1 if mode == "o" else 0
    v = buf[off:off + a.size]
    v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return v


def _run_kernel(kind, case, modes="aaaa"):
    """the case's steps through ops.optim_step; modes: alignment of p, g, s0, s1 -> [(p, s0, s1) after each step] (numpy)"""
    from fplx import ops
    ns = O.n_state(kind, O.abi_hp(kind, case["h"]))
    p = _place(case["p"], modes[0])
    st = [_place(case["state"][i], modes[2 + i]) if i < ns else None for i in range(2)]
    out = []
    for step, gr in zip(case["steps"], case["grads"]):
        ops.optim_step(kind, p, _place(gr, modes[1]), st[0], st[1], O.abi_hp(kind, case["h"], step), step, case["gscale"])
        torch.cuda.synchronize()
        out.append(tuple([p.cpu().numpy()] + [None if s is None else s.cpu().numpy() for s in st]))
    return out


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", O.KINDS)
def test_kernel_against_the_bound(kind, n):
    """every output within optim_ref's bound computed from the device's own state before the step (Rprop: bitwise), on the
    data of the CPU test: aligned base, base offset by one float (scalar head + vector body + tail), and p and g on different
    alignments (the all-scalar kernel)"""
    for wd, mom in O.variants(kind):
        for late in (False, True):
            for gscale in (1.0, 0.125):
                case = O.random_case(kind, n, wd, mom, late, gscale)
                for modes in ("aaaa", "oooo") + (("oaoo",) if gscale == 1.0 else ()):
                    worst = O.check_steps(kind, case, _run_kernel(kind, case, modes))
                    _log("%s n=%d wd=%g mom=%g late=%d gs=%g %s" % (kind, n, wd, mom, late, gscale, modes), worst)
                    assert worst and all(x <= 1.0 for x in worst.values()), worst


@pytest.mark.parametrize("kind,momentum", sorted(O.EXACT_STEPS))
def test_exact_data_equals_torch_bit_for_bit(kind, momentum):
    """n = 10007, the exact data: parameters and state equal torch.optim.<kind> (fp32, CPU) and the op-by-op fp32 evaluation bit
    for bit over EXACT_STEPS' step counts.  Adadelta's p and acc_delta - what lies downstream of std = sqrt(square_avg + eps) -
    are compared with torch only where torch's own CPU sqrt is correctly rounded on THIS host (optimoracle.torch_sqrt_misrounded:
    the set depends on the host's CPU: 0, 78, 1554 or 1566 of 10007 elements on the hosts and paths measured), with optim_f32 everywhere."""
    case = O.exact_case(kind, 10007, momentum)
    ns = O.n_state(kind, O.abi_hp(kind, case["h"]))
    ref = O.run_torch(kind, case)
    bad = O.torch_sqrt_misrounded(kind, case)
    for modes in ("aaaa", "oooo"):
        got = _run_kernel(kind, case, modes)
        cur = (case["p"], case["state"][0], case["state"][1])
        for step, gr, a, b in zip(case["steps"], case["grads"], got, ref):
            cur = O.optim_f32(kind, cur[0], gr, cur[1], cur[2], O.abi_hp(kind, case["h"], step), step)
            for i in range(1 + ns):
                keep = ~bad if (kind, i) in (("Adadelta", 0), ("Adadelta", 2)) else np.ones(bad.size, bool)
                assert np.array_equal(a[i], cur[i]), (kind, momentum, step, i, modes)
                assert np.array_equal(a[i][keep], b[i][keep]), (kind, momentum, step, i, modes)


@pytest.mark.parametrize("kind", O.KINDS)
def test_zero_gradient(kind):
    """wd = 0 and g = 0: p unchanged bit for bit, the state what torch holds after the same steps (zero where torch keeps
    zero; Adamax's exp_inf = eps, ASGD's ax = p, Rprop's step_size = lr).  ASGD has a decay of its own, p *= 1 - lambd eta: it
    runs with lambd = 0 for the unchanged-p check and with torch's default against torch's p."""
    for mom in sorted({m for _, m in O.variants(kind)}):
        for lambd in ((0.0, 1e-4) if kind == "ASGD" else (None,)):
            case = O.random_case(kind, 1023, 0.0, mom, False)
            if lambd is not None:
                case["h"] = O.named_hp(kind, case["h"]["lr"], 0.0, mom, lambd=lambd)
            case["grads"] = [np.zeros(1023, np.float32) for _ in case["grads"][:2]]
            case["steps"] = case["steps"][:2]
            ns = O.n_state(kind, O.abi_hp(kind, case["h"]))
            ref = O.run_torch(kind, case)
            for modes in ("aaaa", "oooo"):
                got = _run_kernel(kind, case, modes)
                for a, b in zip(got, ref):
                    assert np.array_equal(a[0], b[0])
                    assert lambd or np.array_equal(a[0], case["p"])
                    for i in range(1, 1 + ns):
                        assert np.array_equal(a[i], b[i]), (kind, mom, i)
                if kind in ("SGD", "Adadelta", "Adagrad", "RMSprop"):
                    assert all(not got[-1][i].any() for i in range(1, 1 + ns))
                if kind == "Rprop":
                    assert np.array_equal(got[-1][2], np.full(1023, case["h"]["lr"], np.float32)) and not got[-1][1].any()


PACK_SHAPES = [(32, 32), (16, 64), (64, 96)]
PACK_GAPS = [8, 1028, 36, 4097]


@pytest.mark.parametrize("kind,momentum", [(k, 0.9) for k in O.KINDS] + [("SGD", 0.0), ("RMSprop", 0.0)])
def test_pack_kernel_equals_update_then_pack(kind, momentum):
    """fplx_optim_pack_step against fplx_optim_step followed by fplx_pack_conv_weights_batched in the layout of
    test_fused_adam_pack_step_kernel: parameters, both states, both packs and the stamps bit for bit over three steps; a layer
    fplx_adam_pack_ok refuses raises"""
    from fplx import ops
    g = torch.Generator().manual_seed(21)
    offs, pos = [], 0
    for (co, ci), gp in zip(PACK_SHAPES, PACK_GAPS):
        pos += (gp + 3) // 4 * 4
        offs.append(pos)
        pos += co * ci * 27
    n = pos + PACK_GAPS[-1]
    p0 = torch.randn(n, generator=g) * 0.1
    h = O.named_hp(kind, 1e-2, 1e-5, momentum, **({"t0": 1.0} if kind == "ASGD" else {}))
    ns = O.n_state(kind, O.abi_hp(kind, h))
    res = {}
    for fused in (True, False):
        p = p0.clone().cuda()
        st = [torch.zeros(n, device="cuda") if i < ns else None for i in range(2)]
        packs = [(torch.empty((27, co, ci), dtype=torch.bfloat16, device="cuda"),
                  None if k == 1 else torch.empty((27, ci, co), dtype=torch.bfloat16, device="cuda"))
                 for k, (co, ci) in enumerate(PACK_SHAPES)]
        stamps = [torch.zeros(ops.pack_stamp_floats(co, ci), device="cuda") for co, ci in PACK_SHAPES]
        gg = torch.Generator().manual_seed(5)
        for step in range(1, 4):
            grad = (torch.randn(n, generator=gg) * 0.01).cuda()
            hp = O.abi_hp(kind, h, step)
            if fused:
                ops.optim_pack_step(kind, p, grad, st[0], st[1], hp, step, 0.5,
                                    [(o, co, ci, wf, wb, s) for o, (co, ci), (wf, wb), s in zip(offs, PACK_SHAPES, packs, stamps)])
            else:
                ops.optim_step(kind, p, grad, st[0], st[1], hp, step, 0.5)
                ws = [p[o:o + co * ci * 27].view(co, ci, 3, 3, 3) for o, (co, ci) in zip(offs, PACK_SHAPES)]
                ops.pack_conv_weights_batched(ws, torch.bfloat16, [True, False, True], packs, stamps, False)
        torch.cuda.synchronize()
        res[fused] = (p, st, packs, stamps)
    assert torch.equal(res[True][0], res[False][0])
    assert float((res[True][0].cpu() - p0).abs().max()) > 1e-4
    for a, b in zip(res[True][1], res[False][1]):
        assert (a is None and b is None) or torch.equal(a, b)
    for (wf_a, wb_a), (wf_b, wb_b) in zip(res[True][2], res[False][2]):
        assert torch.equal(wf_a, wf_b) and (wb_a is None or torch.equal(wb_a, wb_b))
    for a, b in zip(res[True][3], res[False][3]):
        assert torch.equal(a, b) and float(a.abs().sum()) > 0
    with pytest.raises(ValueError):          # a layer the tiled pack does not take
        ops.optim_pack_step(kind, res[True][0], res[True][0], res[True][1][0], res[True][1][1], O.abi_hp(kind, h, 1), 1, 1.0,
                            [(0, 8, 32, res[True][2][0][0], None)])


def _make_opt(fplx, kind, net, **kw):
    return getattr(fplx, "Fused" + kind)(net, **kw)


@pytest.mark.parametrize("kind,kw", [("SGD", dict(lr=1e-3, momentum=0.9, weight_decay=1e-5)),
                                     ("RMSprop", dict(lr=1e-4, weight_decay=1e-5))])
def test_train_step_with_the_fused_pack_launch(kind, kw):
    """TrainStep(optimizer=Fused...) on the network of test_train_step_with_the_fused_adam_pack_launch, four steps alternating
    domains, the optimiser launch writing the 3x3x3 packs and not: flat_params bit-identical; with it no forward after the first
    repacks a 3x3x3 layer; a single-domain step leaves the other domain's BN segment and its state alone"""
    import fplx
    from fplx import ops
    p = dict(in_chns=1, feature_chns=[32, 64, 64, 128, 128], dropout=[0, 0, 0.3, 0, 0], conv_dims=[3] * 5, class_num=2,
             bilinear=False, num_domains=2, net_type="UNet2D5_dsbn", precision="bf16")
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 1, 16, 32, 64, generator=g).cuda()
    lab = torch.zeros(2, 2, 16, 32, 64)
    lab[:, 0] = 1.0
    lab[:, 0, 4:10, 8:20, 16:40] = 0.0
    lab[:, 1, 4:10, 8:20, 16:40] = 1.0
    lab = lab.cuda()
    res = []
    for fuse in (True, False):
        torch.manual_seed(3)
        net = fplx.UNet2D5_dsbn(dict(p)).cuda()
        net.engine.use_adam_pack = fuse
        opt = _make_opt(fplx, kind, net, **kw)
        ts = fplx.TrainStep(net, (1.0, 0.0, 0.0, 0.0), True, optimizer=opt)
        start = net.flat_params.detach().clone()
        doms = net.segments()[1]
        packed = []
        inner = ops.pack_conv_weights_batched

        def counting(ws, act_dtype, want_wb, into=None, stamps=None, verify=False, _inner=inner, _packed=packed):
            _packed.append((len(ws), bool(verify)))
            return _inner(ws, act_dtype, want_wb, into, stamps, verify)
        ops.pack_conv_weights_batched = counting
        try:
            for it in range(4):
                other = doms[1 - it % 2]
                before = [net.flat_params[other[0]:other[1]].clone()] + [getattr(opt, s)[other[0]:other[1]].clone()
                                                                        for s in opt._active_state()]
                ts.step(x, lab, it % 2)
                after = [net.flat_params[other[0]:other[1]]] + [getattr(opt, s)[other[0]:other[1]] for s in opt._active_state()]
                assert all(torch.equal(a, b) for a, b in zip(before, after))
        finally:
            ops.pack_conv_weights_batched = inner
        torch.cuda.synchronize()
        assert opt.seg_steps == [4, 2, 2]
        assert float((net.flat_params.detach() - start).abs().max()) > 0
        res.append((net.flat_params.detach().clone(), list(packed)))
    assert torch.equal(res[0][0], res[1][0])
    n3 = res[1][1][0][0]
    assert res[1][1] == [(n3, False)] * 4
    assert res[0][1] == [(n3, False)] + [(n3 - 1, True), (1, False)] * 3, res[0][1]


NET = dict(in_chns=1, feature_chns=[4, 4, 8, 8, 8], dropout=[0, 0, 0, 0, 0], conv_dims=[3, 3, 3, 3, 3], class_num=2,
           bilinear=False, num_domains=2, net_type="UNet2D5_dsbn")


def test_agent_trains_with_sgd_from_the_sample_cfg(golden_dir, tmp_path):
    """[training] of the shipped sample cfg with optimizer = SGD: the agent gets the engine step, MultiStepLR drives the fused
    optimiser's param_groups, and a short training_all round on the tiny network lowers the loss"""
    import fplx
    tr = dict(fplx.parse_config(os.path.join(golden_dir, "sample_vs.cfg"))["training"])
    assert tr["optimizer"] == "Adam" and tr["momentum"] == 0.9
    tr.update(optimizer="SGD", learning_rate=0.01, lr_scheduler="MultiStepLR", lr_milestones=[4], lr_gamma=0.5, iter_valid=1,
              ckpt_save_dir=str(tmp_path / "model" / "sgd"))
    cfg = {"dataset": {"tensor_type": "float"}, "network": dict(NET), "training": tr, "testing": {"gpus": [0]}}
    g = np.load(os.path.join(golden_dir, "ref_ckpt.npz"))
    torch.manual_seed(5)
    agent = fplx.SegmentationAgent(cfg, "train")
    agent.create_network()
    agent.create_optimizer()
    agent.create_loss_calculator()
    assert type(agent.optimizer) is fplx.FusedSGD and agent.optimizer.param_groups[0]["momentum"] == 0.9
    assert agent._engine_step() is not None
    b = [{"image": torch.from_numpy(g["x%d" % d]), "label_prob": torch.from_numpy(g["lab%d" % d])} for d in (0, 1)]
    agent.set_loaders([b[0]], [b[1]])
    losses = [agent.training_all()["loss"] for _ in range(8)]
    assert agent.optimizer.seg_steps == [8, 8, 8]
    assert agent.optimizer.param_groups[0]["lr"] == pytest.approx(0.005)
    assert float(agent.optimizer.momentum_buffer.abs().max()) > 0
    assert losses[-1] < losses[0], losses


def _flat_grad(net, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(net.flat_params.numel(), generator=g) * 0.01).cuda()


@pytest.mark.parametrize("kind", O.KINDS)
def test_checkpoint_round_trip_and_torch_interop(kind):
    """two steps (the second on domain 0 only), state_dict, a fresh instance: its third step is bitwise the uninterrupted
    run's.  The same dict in torch.optim.<kind> on the CPU over parameters copied from the device: its third step lies inside
    optim_ref's bound of that step (Rprop: equals it).  An Adam state is refused by name."""
    import fplx
    from fplx.checkpoint import reference_model_state_dict, reference_param_names
    h = O.named_hp(kind, 1e-2, 1e-5, 0.9)
    torch.manual_seed(7)
    net = fplx.UNet2D5_dsbn(dict(NET)).cuda()
    net._ensure_flat()
    opt = _make_opt(fplx, kind, net, **h)
    opt.step_flat(_flat_grad(net, 1), [0, 1])
    opt.step_flat(_flat_grad(net, 2), [0])
    assert opt.seg_steps == [2, 2, 1]
    sd = opt.state_dict()
    p2 = net.flat_params.detach().clone()
    st2 = [getattr(opt, s).clone() for s in opt._active_state()]
    net_b = fplx.UNet2D5_dsbn(dict(NET)).cuda()
    net_b._ensure_flat()
    with torch.no_grad():
        net_b.flat_params.copy_(p2)
    opt_b = _make_opt(fplx, kind, net_b, **O.named_hp(kind, 0.5, 0.0, 0.0))      # every hyper-parameter comes from the dict
    opt_b.load_state_dict(sd)
    assert opt_b.seg_steps == ([1, 1, 1] if kind == "SGD" else [2, 2, 1])
    g3 = _flat_grad(net, 3)
    opt.step_flat(g3, [0, 1])
    opt_b.step_flat(g3, [0, 1])
    torch.cuda.synchronize()
    for k in net._order:                     # parameter by parameter: the alignment gaps between them carry no state
        o, n, _ = net._layout[k]
        assert torch.equal(net.flat_params[o:o + n], net_b.flat_params[o:o + n]), k
        for s in opt._active_state():
            assert torch.equal(getattr(opt, s)[o:o + n], getattr(opt_b, s)[o:o + n]), (k, s)
    assert not torch.equal(net.flat_params, p2)
    # torch on the CPU from the same dict
    names = reference_param_names(2)
    msd = reference_model_state_dict(net)
    prm = []
    for k in names:
        if k in net._layout:
            o, n, shp = net._layout[k]
            prm.append(torch.nn.Parameter(p2[o:o + n].view(shp).cpu().clone()))
        else:
            prm.append(torch.nn.Parameter(msd[k].clone().float()))
    ref = getattr(torch.optim, kind)(prm, foreach=False, **h)
    ref.load_state_dict(sd)
    for k, q in zip(names, prm):
        if k in net._layout:
            o, n, shp = net._layout[k]
            q.grad = g3[o:o + n].view(shp).cpu().clone()
    ref.step()
    worst = {}
    got, g3c, p2c, st2c = net.flat_params.detach().cpu().numpy(), g3.cpu().numpy(), p2.cpu().numpy(), [s.cpu().numpy() for s in st2]
    for si, (a, b) in enumerate(opt.seg_ranges):
        step = [3, 3, 2][si]
        hp = O.abi_hp(kind, h, step)
        for k, q in zip(names, prm):
            if k not in net._layout or not (a <= net._layout[k][0] < b):
                continue
            o, n, _ = net._layout[k]
            sl = slice(o, o + n)
            s01 = [s[sl] for s in st2c] + [None, None]
            tq = q.detach().numpy().reshape(-1)
            if kind == "Rprop":
                r = O.optim_f32(kind, p2c[sl], g3c[sl], s01[0], s01[1], hp, step)
                assert np.array_equal(tq, r[0]) and np.array_equal(got[sl], r[0]), k
                continue
            r = O.optim_ref(kind, p2c[sl], g3c[sl], s01[0], s01[1], hp, step)
            worst["torch"] = max(worst.get("torch", 0.0), O.ratio(tq, r[0], r[3]))
            worst["fused"] = max(worst.get("fused", 0.0), O.ratio(got[sl], r[0], r[3]))
    _log("checkpoint %s third step" % kind, worst)
    assert all(x <= 1.0 for x in worst.values()), worst
    if kind == "SGD":
        adam = fplx.FusedAdam(net, 1e-3)
        adam.step_flat(g3, [0, 1])
        with pytest.raises(ValueError, match="Adam.*FusedSGD"):
            opt.load_state_dict(adam.state_dict())


def _adam_recorder():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("record_adam_digest", os.path.join(root, "tools", "record_adam_digest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("abi", [False, True])
def test_adam_bits_equal_the_recorded_parent(abi):
    """Adam is kind FPLX_OPT_ADAM of fplx_optim_step / fplx_optim_pack_step; before that it had kernels of its own.  The cases of
    tools/record_adam_digest.py (adam_step at an aligned base and one float behind one - vector body / scalar head and tail now,
    one scalar loop then -, adam_pack_step with stamps), through fplx.ops and through the two C entry points themselves: every
    output after every step has the sha256 recorded from the commit before the change (tests/golden/adam_parent_digest.json)."""
    import json
    from fplx import ops
    R = _adam_recorder()
    with open(R.FIXTURE) as f:
        want = json.load(f)
    for behind in (0, 1):
        inputs, out = R.step_case(ops, O.rng, behind, abi)
        assert inputs == want["adam_step"]["inputs"], "the inputs drifted, not the kernel"
        assert out == want["adam_step"]["outputs"], (behind, [a == b for a, b in zip(out, want["adam_step"]["outputs"])])
    inputs, out = R.pack_case(ops, O.rng, abi)
    assert inputs == want["adam_pack_step"]["inputs"], "the inputs drifted, not the kernel"
    assert out == want["adam_pack_step"]["outputs"], [a == b for a, b in zip(out, want["adam_pack_step"]["outputs"])]


def test_abi_refusals():
    from fplx import ops
    p, g, a, b = [torch.zeros(64, device="cuda") for _ in range(4)]
    hp = (1e-3, 0.9, 0.0)
    ops.optim_step("SGD", p, g, a, None, hp, 1)
    for kind in (-1, len(ops.OPTIM_KINDS)):
        with pytest.raises(ValueError, match="kind"):
            ops.optim_step(kind, p, g, a, b, hp, 1)
    adam = (1e-3, 0.9, 0.999, 1e-8, 0.0)
    with pytest.raises(ValueError, match="state"):
        ops.optim_step("Adam", p, g, a, None, adam, 1)
    with pytest.raises(ValueError, match="hyper-parameters"):
        ops.optim_step("Adam", p, g, a, b, adam[:4], 1)
    with pytest.raises(ValueError, match="step"):
        ops.optim_step("Adam", p, g, a, b, adam, 0)
    with pytest.raises(ValueError, match="step"):
        ops.optim_step("SGD", p, g, a, None, hp, 0)
    with pytest.raises(ValueError, match="state"):
        ops.optim_step("SGD", p, g, None, None, hp, 1)                 # momentum 0.9 needs the buffer
    with pytest.raises(ValueError, match="state"):
        ops.optim_step("Adamax", p, g, a, None, (1e-3, 0.9, 0.999, 1e-8, 0.0), 1)
    with pytest.raises(ValueError, match="hyper-parameters"):
        ops.optim_step("SGD", p, g, a, None, hp + (0.0,), 1)
    with pytest.raises(ValueError):
        ops.optim_step("SGD", p[:0], g[:0], None, None, (1e-3, 0.0, 0.0), 1)
    ops.optim_step("SGD", p, g, None, None, (1e-3, 0.0, 0.0), 1)       # momentum 0: no state at all
    torch.cuda.synchronize()
    assert not p.any()
