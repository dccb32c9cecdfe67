"""-m gpu tests of the semi-supervised kernels (csrc/ssl.hip through fplx.ops / fplx.ssl) against tests/ssloracle.py - the exact
part bit for bit, the rounding part inside the derived bounds, every kernel twice for the same bits - then one MeanTeacher
iteration end to end against the CPU restatement of the network, and one train_valid round of each of the three agents."""
import os

import numpy as np
import pytest
import torch

import nets3d_cfg as C
import ssloracle as SO

pytestmark = pytest.mark.gpu

NS, CS, VS, TS = (1, 3), (2, 3, 8), (1, 5, 63, 9240), (0, 2, 8, 16)
GRAD_TOL, LOGIT_TOL = 1e-3, 1e-3          # tests/test_gpu_nets3d.py: the floor every config sits at, max-normalised


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def _fwd_twice(s, q, mc, thr, softmax):
    from fplx import ops
    a, ma = ops.ssl_consistency_fwd(s, q, mc, thr, softmax)
    b, mb = ops.ssl_consistency_fwd(s, q, mc, thr, softmax)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64)) and (ma is None or torch.equal(ma, mb))
    return host(a), (None if ma is None else host(ma))


# ---------------------------------------------------------------- exact part

@pytest.mark.parametrize("v", VS)
@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("n", NS)
def test_exact_sums_counts_and_masks(n, c, v):
    for t in TS:
        s, q, mc, thr = SO.exact_case("gpu.exact.%d.%d.%d.%d" % (n, c, v, t), n, c, v, t)
        SO.exact_pre(s, q)
        out_ref, keep, _, _ = SO.consistency_fwd(s, q, mc, thr, False)
        r = SO.consistency_ref(s, q, mc, thr, False)
        assert not r.undecided.any()
        out, mask = _fwd_twice(dev(s), dev(q), dev(mc), thr, False)
        assert out[0] == out_ref[0] and out[1] == out_ref[1] and out[3] == 0.0, (t, out, out_ref)
        assert out[2] == out_ref[2], (t, out[2], out_ref[2])          # the same double expression of exact sums
        if t:
            assert mask.shape == (n, v) and np.array_equal(mask.astype(bool), keep)
        else:
            assert mask is None


def test_the_mask_is_strictly_below_the_threshold():
    """voxels no pass gives any probability: m = 0, unc = 0 exactly - not kept at thr = 0 (`<`, ssl_uamt.py:99)"""
    n, c, v, t = 1, 3, 63, 2
    s, q, mc, _ = SO.exact_case("gpu.strict", n, c, v, t)
    mc[:, :, :, ::3] = 0.0
    r = SO.consistency_ref(s, q, mc, 0.0, False)
    assert not r.undecided[:, ::3].any() and not r.keep[:, ::3].any() and r.keep.any()
    out, mask = _fwd_twice(dev(s), dev(q), dev(mc), 0.0, False)
    SO.check_consistency_fwd(r, out, mask, "strict")
    assert not mask[:, ::3].any()


@pytest.mark.parametrize("n", [1, 3, 1001, 4096, 4099])
def test_ema_exact_and_inside_the_bound(n):
    from fplx import ops
    e, p = SO.ema_exact_case("gpu.ema.%d" % n, n)
    for off in (0, 1):                                   # 16-byte aligned (quads + tail) and not (scalar form)
        buf = torch.zeros(n + 5, dtype=torch.float32, device="cuda")
        de = buf[off:off + n]
        de.copy_(dev(e))
        ops.ema_step(de, dev(p), 0.75)
        assert np.array_equal(host(de).astype(np.float64), SO.ema(e, p, 0.75))
        assert float(buf[:off].abs().sum()) == 0.0 and float(buf[off + n:].abs().sum()) == 0.0      # nothing outside the segment
    g = SO.LO.rng("gpu.ema.real.%d" % n)
    e, p = g.standard_normal(n).astype(np.float32), g.standard_normal(n).astype(np.float32)
    ref, bound = SO.ema_ref(e, p, 0.99)
    got = [host(ops.ema_step(dev(e), dev(p), 0.99)) for _ in range(2)]
    assert np.array_equal(got[0], got[1])
    assert SO.ratio(got[0], ref, bound) <= 1.0


# ---------------------------------------------------------------- ssl_perturb

@pytest.mark.parametrize("shape,reps", [((1, 1, 3, 5, 7), 1), ((2, 1, 4, 4, 4), 2), ((1, 1, 3, 5, 7), 2), ((3,), 1), ((2, 2, 8, 16, 16), 2)])
def test_perturb_with_injected_noise_is_torch_bit_for_bit(shape, reps):
    from fplx import ops
    gen = torch.Generator().manual_seed(7)
    x1 = torch.randn(shape, generator=gen)
    z = torch.randn((reps,) + tuple(shape), generator=gen)
    want = x1 + torch.clamp(z * 0.1, -0.2, 0.2)                       # ssl_mt.py:79 / ssl_uamt.py:83-85 on the CPU
    got = [ops.ssl_perturb(x1.cuda(), z.cuda(), reps, 0.1, 0.2).cpu() for _ in range(2)]
    assert got[0].shape == want.shape and torch.equal(got[0], got[1])
    assert torch.equal(got[0].view(torch.int32), want.view(torch.int32))
    assert float((z.abs() * 0.1 > 0.2).float().mean()) > 0 or z.numel() < 100     # the clamp is active somewhere


def test_perturb_philox_stream():
    from fplx import ops
    n = 1 << 20
    x = torch.zeros(n, device="cuda")
    a = ops.ssl_perturb(x, None, 2, 0.1, 0.2, seed=1234, stream_id=5)
    b = ops.ssl_perturb(x, None, 2, 0.1, 0.2, seed=1234, stream_id=5)
    assert torch.equal(a, b)                                          # reproducible for a seed
    assert not torch.equal(a[0], a[1])                                # different across r
    assert not torch.equal(a, ops.ssl_perturb(x, None, 2, 0.1, 0.2, seed=1234, stream_id=6))
    assert not torch.equal(a, ops.ssl_perturb(x, None, 2, 0.1, 0.2, seed=1235, stream_id=5))
    clip = float(np.float32(0.2))
    assert float(a.abs().max()) <= clip and float((a.abs() == clip).float().mean()) > 0.01
    xr = torch.randn(4097, device="cuda")
    y = ops.ssl_perturb(xr, None, 1, 0.1, 0.2, seed=3, stream_id=0)[0]
    assert float((y - xr).abs().max()) <= clip + 2.0 ** -21           # within [-clip, clip] of x (one rounding of the sum, |x| < 8)
    m2, m4 = SO.clamped_normal_moments(float(np.float32(0.1)), clip)
    w = host(a[0]).astype(np.float64)
    mean, var = w.mean(), (w * w).mean()
    print("philox clamped normal: mean %.3e (se %.3e), E w^2 %.6e (want %.6e, se %.3e)" % (
        mean, np.sqrt(m2 / n), var, m2, np.sqrt((m4 - m2 * m2) / n)))
    assert abs(mean) <= 5 * np.sqrt(m2 / n)
    assert abs(var - m2) <= 5 * np.sqrt((m4 - m2 * m2) / n)


# ---------------------------------------------------------------- rounding part

@pytest.mark.parametrize("v", VS)
@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("n", NS)
def test_consistency_inside_the_bounds(n, c, v):
    import fplx
    from fplx import ops
    worst = {}
    for t in TS:
        s, q, mc = SO.logits_case("gpu.%d.%d.%d.%d" % (n, c, v, t), n, c, v, t)
        ds, dq, dmc = dev(s), dev(q), dev(mc)
        for ramp in ((0.0, 0.3) if t else (0.0,)):
            thr = SO.uamt_threshold(ramp, c) if t else 0.0
            gs = 0.7
            r = SO.consistency_ref(s, q, mc, thr, True, gs)
            SO.check_case_is_a_real_test(r, n, v)
            out, mask = _fwd_twice(ds, dq, dmc, thr, True)
            res = SO.check_consistency_fwd(r, out, mask, "n%d c%d v%d t%d ramp %g" % (n, c, v, t, ramp))
            dgs = torch.tensor([gs], dtype=torch.float32, device="cuda")
            dout = dev(out)
            dmask = dev(mask)
            d1 = ops.ssl_consistency_bwd(ds, dq, dmask, dout, dgs, t, True)
            d2 = ops.ssl_consistency_bwd(ds, dq, dmask, dout, dgs, t, True)
            assert torch.equal(d1, d2)
            dl, bound = SO.consistency_grad_ref(s, q, mask, gs, t, True)
            res["dstudent"] = SO.ratio(host(d1), dl, bound)
            assert res["dstudent"] <= 1.0, (t, ramp, res)
            for k, x in res.items():
                worst[k] = max(worst.get(k, 0.0), x)
            # the autograd node gives the same numbers
            sg = ds.clone().requires_grad_(True)
            loss = fplx.consistency_loss(sg, dq, dmc, thr if t else None)
            assert float(loss.detach()) == float(np.float32(out[2]))
            (loss * gs).backward()
            assert torch.equal(sg.grad, d1)
    print("n%d c%d v%d: worst error / bound %s" % (n, c, v, worst))


def test_consistency_without_softmax_gradient():
    from fplx import ops
    n, c, v, t = 3, 3, 63, 2
    s, q, mc, thr = SO.exact_case("gpu.nosm", n, c, v, t)
    out, mask = _fwd_twice(dev(s), dev(q), dev(mc), thr, False)
    gs = torch.tensor([1.5], dtype=torch.float32, device="cuda")
    d = host(ops.ssl_consistency_bwd(dev(s), dev(q), dev(mask), dev(out), gs, t, False))
    dl, bound = SO.consistency_grad_ref(s, q, mask, 1.5, t, False)
    assert SO.ratio(d, dl, bound) <= 1.0 and np.abs(d).max() > 0


@pytest.mark.parametrize("v", VS)
@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("n", NS)
def test_entropy_pair_inside_the_bounds(n, c, v):
    import fplx
    from fplx import ops
    s, _, _ = SO.logits_case("gpu.ent.%d.%d.%d" % (n, c, v), n, c, v, 0)
    probs = SO.LO.soft_labels("gpu.entp.%d.%d.%d" % (n, c, v), n, c, v)
    for x, softmax in ((s, True), (probs, False)):
        gs = 0.7
        r = SO.entropy_ref(x, softmax, gs)
        dx = dev(x)
        a, b = ops.ssl_entropy_fwd(dx, softmax), ops.ssl_entropy_fwd(dx, softmax)
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))
        out = host(a)
        assert out[1] == n * v and out[3] == 0.0
        ratios = (SO.ratio(out[0], r.out[0], r.out0_bound), SO.ratio(out[2], r.out[2], r.loss_bound))
        dgs = torch.tensor([gs], dtype=torch.float32, device="cuda")
        d1, d2 = ops.ssl_entropy_bwd(dx, dgs, softmax), ops.ssl_entropy_bwd(dx, dgs, softmax)
        assert torch.equal(d1, d2)
        ratios += (SO.ratio(host(d1), r.dl, r.dl_bound),)
        print("entropy n%d c%d v%d softmax %d: error / bound (sum, loss, gradient) %s" % (n, c, v, softmax, ratios))
        assert max(ratios) <= 1.0, ratios
        lg = dx.clone().requires_grad_(True)
        loss = fplx.EntropyLoss()({"prediction": [lg], "softmax": softmax})
        assert float(loss.detach()) == float(np.float32(out[2]))
        (loss * gs).backward()
        assert torch.equal(lg.grad, d1)


# ---------------------------------------------------------------- one MeanTeacher iteration end to end

NAME = "u3d4_ds"
ITER_MAX = 10
REG_W_CFG = 5.0 / float(np.exp(-5.0))          # regular_w = 5 at glob_it = 0: the regulariser's gradient is well above the tolerance


def _plain_params():
    return dict(C.NETS[NAME], deep_supervise=False, precision="fp32")


def _weights(teacher=False):
    import detdata
    w = {k: v for k, v in C.weights_for(NAME).items() if not k.startswith(("out_conv1", "out_conv2", "out_conv3"))}
    if teacher:                     # another point of the same family: every float tensor nudged, variances kept positive
        for k, v in w.items():
            if v.dtype == np.float32 and not k.endswith("running_var"):
                w[k] = (v + 0.02 * detdata.normal("ema." + k, v.shape)).astype(np.float32)
    return w


def _nets():
    import fplx
    nets = []
    for teacher in (False, True):
        net = fplx.UNet3D(_plain_params())
        net.load_state_dict({k: torch.from_numpy(v) for k, v in _weights(teacher).items()}, strict=True)
        nets.append(net.cuda().train())
    return nets


def _mt_data():
    x, y = torch.from_numpy(C.input_for(NAME)), torch.from_numpy(C.label_for(NAME))
    z = torch.randn((1,) + tuple(x[1:].shape), generator=torch.Generator().manual_seed(21))
    return x[:1], y[:1], x[1:], z


def test_mean_teacher_iteration_matches_the_cpu_restatement(tmp_path):
    import fplx
    from fplx import ops
    import nets3d_ref as R3
    from oracle import torch_ref as R
    x0, y0, x1, z = _mt_data()
    regular_w = REG_W_CFG * fplx.get_rampup_ratio(0, 0, ITER_MAX, "sigmoid")
    # ---- the reference's statements on the CPU (ssl_mt.py:76-101), fp32
    p = _plain_params()
    sd, prm = R.split_state(_weights(False))
    sde, _ = R.split_state(_weights(True), requires_grad=False)
    inputs_ema = x1 + torch.clamp(z[0] * 0.1, -0.2, 0.2)
    outputs = R3.forward(sd, p, torch.cat([x0, x1], dim=0), True)
    loss_sup = R.dice_loss(outputs[:1], y0)
    p1_soft = torch.softmax(outputs, dim=1)[1:]
    with torch.no_grad():
        outputs_ema = R3.forward(sde, p, inputs_ema, True)
        p1_ema_soft = torch.softmax(outputs_ema, dim=1)
    loss_reg = torch.nn.MSELoss()(p1_soft, p1_ema_soft)
    g_sup = torch.autograd.grad(loss_sup, list(prm.values()), retain_graph=True, allow_unused=True)
    (loss_sup + regular_w * loss_reg).backward()
    # ---- the same iteration on the GPU
    net, net_ema = _nets()
    opt = fplx.get_optimizer("SGD", net, {"learning_rate": 0.05, "momentum": 0.0, "weight_decay": 0.0})
    out = net(torch.cat([x0, x1], dim=0).cuda())
    l_sup = fplx.DiceLoss()({"prediction": out[:1], "ground_truth": y0.cuda()})
    ema_in = ops.ssl_perturb(x1.cuda(), z.cuda(), 1, 0.1, 0.2)[0]
    assert torch.equal(ema_in.cpu(), inputs_ema)
    with torch.no_grad():
        out_ema = net_ema(ema_in)
    l_reg = fplx.consistency_loss(out[1:], out_ema)
    loss = l_sup + regular_w * l_reg
    loss.backward()
    assert float((out.detach().cpu() - outputs.detach()).abs().max()) < LOGIT_TOL
    assert float((out_ema.cpu() - outputs_ema).abs().max()) < LOGIT_TOL
    assert abs(float(l_sup) - float(loss_sup)) < 1e-5 and abs(float(l_reg) - float(loss_reg)) < 1e-5 * max(1.0, float(loss_reg) * 100)
    named = dict(net.named_parameters())
    moved = 0
    for (k, t), gs_only in zip(prm.items(), g_sup):
        if t.grad is None:
            continue
        ref, got = t.grad.numpy(), host(named[k].grad)
        parts = k.rsplit(".", 2)
        if k.endswith("bias") and ".conv_conv." in k and parts[1] in ("0", "4"):      # in front of train-mode BatchNorm: exactly 0
            assert np.abs(got).max() == 0.0 and np.abs(ref).max() < 1e-5, k
            continue
        tol = max(GRAD_TOL * np.abs(ref).max(), 2e-7)
        np.testing.assert_allclose(got, ref, atol=tol, rtol=0, err_msg=k)
        if gs_only is not None and float((t.grad - gs_only).abs().max()) > 10 * tol:
            moved += 1
    assert moved >= 10, "the regulariser's share of the gradient is below the tolerance: the comparison would not see it"
    # ---- optimiser step, then the EMA: the teacher is the EMA of the two parameter sets
    ema_before = host(net_ema.flat_params).copy() if net_ema.flat_params is not None else None
    assert ema_before is not None
    before = host(net.flat_params).copy()
    opt.step()
    alpha = min(1 - 1 / (ITER_MAX + 1), 0.99)
    fplx.ema_update(net_ema, net, alpha)
    after = host(net.flat_params)
    assert np.abs(after - before).max() > 0
    ref, bound = SO.ema_ref(ema_before, after, alpha)
    assert SO.ratio(host(net_ema.flat_params), ref, bound) <= 1.0
    sd_ema = net_ema.state_dict()
    assert torch.equal(sd_ema["out_conv.weight"].reshape(-1), net_ema.flat_params[net_ema._layout["out_conv.weight"][0]:][:sd_ema["out_conv.weight"].numel()])
    # ---- the agent runs this very iteration: same student and teacher, bit for bit
    agent = _agent(tmp_path, "MeanTeacher", iter_valid=1, regularize_w=REG_W_CFG, learning_rate=0.05)
    net2, ema2 = _nets()
    agent.net, agent.net_ema = net2, ema2
    agent.create_optimizer()
    agent.create_loss_calculator(1.0)
    agent.set_loaders([{"image": x0, "label_prob": y0}])
    agent.set_unlabeled_loader([{"image": x1}])
    agent.noise_source = lambda reps, shape: z.cuda()
    agent.glob_it = 0
    res = agent.training()
    assert torch.equal(net2.flat_params, net.flat_params) and torch.equal(ema2.flat_params, net_ema.flat_params)
    assert abs(res["loss"] - float(loss)) < 1e-6 and abs(res["loss_reg"] - float(l_reg)) < 1e-7 and res["regular_w"] == regular_w


# ---------------------------------------------------------------- the three agents

def _agent(tmp_path, method, iter_valid=2, regularize_w=0.1, learning_rate=1e-2, **ssl_over):
    import fplx
    net = dict(_plain_params(), net_type="UNet3D")
    cfg = {"dataset": {"tensor_type": "float", "root_dir": str(tmp_path)},
           "network": net,
           "training": {"gpus": [0], "loss_type": "DiceLoss", "optimizer": "SGD", "learning_rate": learning_rate, "weight_decay": 0.0,
                        "momentum": 0.0, "lr_scheduler": None, "iter_start": 0, "iter_max": ITER_MAX, "iter_valid": iter_valid,
                        "iter_save": iter_valid, "dual": False, "ckpt_save_dir": str(tmp_path / "model" / method)},
           "testing": {"gpus": [0], "domian_label": 0},
           "semi_supervised_learning": dict({"ssl_method": method, "regularize_w": regularize_w}, **ssl_over)}
    torch.manual_seed(5)
    return fplx.ssl.ssl_agent_class(method)(cfg, "train")


@pytest.mark.parametrize("method", ["EntropyMinimization", "MeanTeacher", "UAMT"])
def test_agents_run_one_round_and_write_a_checkpoint(tmp_path, method):
    import fplx
    x0, y0, x1, _ = _mt_data()
    agent = _agent(tmp_path, method, uamt_mcdroput_n=4)
    agent.config["training"]["iter_max"] = 2
    assert agent.config["network"]["num_domains"] == 1
    agent.create_network()
    assert type(agent.net) is fplx.UNet3D
    if method == "EntropyMinimization":
        assert agent.net_ema is None
    else:
        assert type(agent.net_ema) is fplx.UNet3D and agent.net_ema.training and agent.net_ema.dropout_seed == agent.net.dropout_seed + 1
    agent.set_loaders([{"image": x0, "label_prob": y0}])
    agent.set_unlabeled_loader([{"image": x1}])
    agent.valid_loader_1 = [{"image": x0, "label_prob": y0}]
    agent.net._ensure_flat()
    student0 = agent.net.flat_params.clone()
    if agent.net_ema is not None:
        agent.net_ema._ensure_flat()
        teacher0 = agent.net_ema.flat_params.clone()
    hist = agent.train_valid()
    assert len(hist) == 1
    glob_it, _, tr, va = hist[0]
    assert glob_it == 2
    assert sorted(tr) == ["avg_dice", "class_dice", "loss", "loss_reg", "loss_sup", "regular_w"]
    for k in ("loss", "loss_sup", "loss_reg", "regular_w", "avg_dice"):
        assert np.isfinite(tr[k]), (k, tr[k])
    assert tr["class_dice"].shape == (3,) and np.isfinite(va["loss"])
    assert tr["regular_w"] == 0.1 * fplx.get_rampup_ratio(0, 0, 2, "sigmoid")
    assert tr["loss_reg"] > 0 or (method == "UAMT" and tr["loss_reg"] == 0)      # UAMT: no voxel may be certain enough yet
    assert abs(tr["loss"] - (tr["loss_sup"] + tr["regular_w"] * tr["loss_reg"])) < 1e-5
    assert not torch.equal(student0, agent.net.flat_params)
    if agent.net_ema is not None:
        assert not torch.equal(teacher0, agent.net_ema.flat_params) and agent.net_ema.training
    # the checkpoint holds the student only and loads into the supervised agent
    ck = tmp_path / "model" / method
    files = sorted(os.listdir(str(ck)))
    assert any(f.endswith("_latest.txt") for f in files) and any(f.endswith("_2.pt") for f in files)
    pt = torch.load(str(ck / [f for f in files if f.endswith("_2.pt")][0]), map_location="cpu", weights_only=False)
    assert list(pt["model_state_dict"]) == list(agent.net.state_dict()) and not any("ema" in k for k in pt)
    agent.config["testing"]["ckpt_mode"] = 0
    sup = fplx.SegmentationAgent(agent.config, "test")
    sup.create_network()
    sup.set_loaders(test_loader=[{"image": x0, "names": ["case0.nii.gz"]}])
    pred = sup.infer()
    for k, v in agent.net.state_dict().items():
        assert torch.equal(sup.net.state_dict()[k].cpu(), v.cpu()), k
    assert pred["case0.nii.gz"].shape == tuple(x0.shape[2:])


# ---------------------------------------------------------------- python -m fplx.ssl_main train config.cfg

SSL_CFG = """
[dataset]
tensor_type = float
task_type = seg
root_dir  = {root}
train_csv = {root}/train.csv
valid_csv = {root}/valid.csv
test_csv  = {root}/test.csv
train_csv_unlab = {root}/unlab.csv
train_batch_size = 1
train_batch_size_unlab = 2
modal_num = 1

train_transform = [NormalizeWithMeanStd, Pad, RandomCrop, RandomFlip, LabelToProbability]
train_transform_unlab = [NormalizeWithMeanStd, Pad, RandomCrop, RandomFlip]
valid_transform = [NormalizeWithMeanStd, Pad, LabelToProbability]
test_transform  = [NormalizeWithMeanStd, Pad]
NormalizeWithMeanStd_channels = [0]
NormalizeWithMeanStd_mean = None
NormalizeWithMeanStd_std  = None
NormalizeWithMeanStd_inverse = False
Pad_output_size = [16, 32, 48]
Pad_ceil_mode   = False
Pad_inverse     = True
RandomCrop_output_size = [16, 32, 32]
RandomCrop_foreground_focus = False
RandomCrop_foreground_ratio = None
Randomcrop_mask_label       = None
RandomCrop_inverse     = False
RandomFlip_flip_depth  = False
RandomFlip_flip_height = True
RandomFlip_flip_width  = True
RandomFlip_inverse     = False
LabelToProbability_class_num = 2
LabelToProbability_inverse   = False

[network]
net_type = {net_type}
class_num     = 2
in_chns       = 1
{net_keys}

[training]
gpus       = [0]
loss_type     = DiceLoss
optimizer     = Adam
learning_rate = 1e-2
momentum      = 0.9
weight_decay  = 1e-5
lr_scheduler  = MultiStepLR
lr_gamma      = 0.5
lr_milestones = [10000, 20000]
ckpt_save_dir    = {root}/model/ssl
iter_start = 0
iter_max   = 4
iter_valid = 2
iter_save  = 2

[semi_supervised_learning]
ssl_method = {method}
regularize_w = 0.1
ema_decay = 0.99
rampup_start = 0
rampup_end = 4
uamt_mcdroput_n = 2

[testing]
gpus       = [0]
ckpt_mode         = 1
output_dir        = {root}/result
evaluation_mode   = True
sliding_window_enable = True
sliding_window_size   = [16, 32, 32]
sliding_window_stride = [16, 32, 32]
"""

NET_KEYS = {
    "UNet3D": "feature_chns  = [8, 16, 32, 64]\ndropout       = [0.0, 0.0, 0.3, 0.4]\ntrilinear     = False\ndeep_supervise = False",
    "UNet2D5": "feature_chns  = [8, 16, 32, 32, 32]\nconv_dims     = [2, 2, 3, 3, 3]\ndropout       = [0.0, 0.0, 0.3, 0.4, 0.5]\n"
               "bilinear      = False",
}


@pytest.mark.parametrize("method,net_type", [("EntropyMinimization", "UNet2D5"), ("MeanTeacher", "UNet3D"), ("UAMT", "UNet2D5")])
def test_ssl_main_trains_and_tests_from_a_cfg(tmp_path, method, net_type):
    """the reference's key surface (train_csv / valid_csv / train_csv_unlab, [semi_supervised_learning]) over synthetic .nii.gz
    cases: two validation rounds with checkpoints, then the student's best checkpoint predicts the test cases"""
    from fplx import ssl_main, nifti
    root = tmp_path
    rs = np.random.RandomState(9)
    (root / "img").mkdir()
    (root / "lab").mkdir()
    names = []
    for i in range(6):
        shp = (16, 30 + 2 * (i % 2), 44)
        lab = np.zeros(shp, np.uint8)
        lab[4:12, 8 + i:20 + i, 10:30] = 1
        img = rs.randn(*shp) * 15 + 90 + 70.0 * lab
        nifti.write_nifti(str(root / "img" / ("c%d.nii.gz" % i)), img.astype(np.float32), (0.5, 0.5, 1.5))
        nifti.write_nifti(str(root / "lab" / ("c%d.nii.gz" % i)), lab, (0.5, 0.5, 1.5))
        names.append("c%d.nii.gz" % i)
    (root / "train.csv").write_text("image,label\n" + "\n".join("img/%s,lab/%s" % (n, n) for n in names[:2]) + "\n")
    (root / "valid.csv").write_text("image,label\n" + "img/%s,lab/%s" % (names[2], names[2]) + "\n")
    (root / "unlab.csv").write_text("image\n" + "\n".join("img/" + n for n in names[2:5]) + "\n")
    (root / "test.csv").write_text("image\n" + "img/" + names[5] + "\n")
    cfg = root / "ssl.cfg"
    cfg.write_text(SSL_CFG.format(root=str(root), method=method, net_type=net_type, net_keys=NET_KEYS[net_type]))
    import random
    random.seed(3)
    ssl_main.main(["fplx.ssl_main", "train", str(cfg)])
    files = sorted(os.listdir(str(root / "model" / "ssl")))
    assert "ssl_latest.txt" in files and "ssl_best.txt" in files and "log_train.txt" in files
    assert "ssl_4.pt" in files
    m = nifti.load_nifty_volume_as_4d_array(str(root / "result" / "ssl_test" / names[5]))
    ref = nifti.load_nifty_volume_as_4d_array(str(root / "img" / names[5]))
    assert m["data_array"].dtype == np.uint8 and m["data_array"].shape == ref["data_array"].shape
