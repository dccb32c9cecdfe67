"""-m gpu tests of the weakly-supervised kernels (csrc/wsl.hip through fplx.ops / fplx.wsl) against tests/wsloracle.py - the exact
families bit for bit, the rounding families inside the derived bounds, every kernel twice for the same bits - then one
WSLGatedCRF and one WSLTotalVariation iteration end to end against the CPU restatement of the network, one USTM iteration,
one train_valid round of each of the five agents, and wsl_main from a written .cfg."""
import os

import numpy as np
import pytest
import torch

import nets3d_cfg as C
import ssloracle as SO
import wsloracle as WO

pytestmark = pytest.mark.gpu

GRAD_TOL, LOGIT_TOL = 1e-3, 1e-3          # tests/test_gpu_nets3d.py: the floor every config sits at, max-normalised
GS = 0.7


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def _gs():
    return torch.tensor([GS], dtype=torch.float32, device="cuda")


def _same_bits(a, b):
    return torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b)


# ---------------------------------------------------------------- TotalVariation

# (1,1,1): no neighbour at all; (5,29,29): 4205 voxels - the 4096-voxel partial rows and the 256-lane blocks are crossed in every axis
TV_SHAPES = [(1, 1, 1), (1, 3, 5), (2, 3, 5), (4, 5, 7), (3, 17, 33), (5, 29, 29)]
TV_NC = [(1, 2), (2, 2), (1, 3), (2, 3), (1, 8), (2, 8)]


def _tv_twice(x, softmax):
    from fplx import ops
    (o1, c1), (o2, c2) = ops.wsl_tv_fwd(x, softmax), ops.wsl_tv_fwd(x, softmax)
    assert _same_bits(o1, o2) and torch.equal(c1, c2)
    return host(o1), c1


@pytest.mark.parametrize("d,h,w", TV_SHAPES)
def test_tv_exact_counts(d, h, w):
    from fplx import ops
    for n, c in TV_NC:
        x = WO.tv_exact_case("gpu.tv.exact.%d.%d.%d.%d.%d" % (n, c, d, h, w), n, c, d, h, w)
        r = WO.tv_ref(x, False, GS)
        assert not r.undecided.any() and r.count_free.all()
        out, count = _tv_twice(dev(x), False)
        assert np.array_equal(host(count), r.count), (n, c)
        assert out[1] == 0.0 and out[3] == n * c * d * h * w
        assert SO.ratio(out[0], r.out[0], r.out0_bound) <= 1.0 and SO.ratio(out[2], r.out[2], r.loss_bound) <= 1.0
        dl, bound = WO.tv_grad_ref(x, r.count, GS, False)
        got = ops.wsl_tv_bwd(dev(x), count, _gs(), False)
        assert SO.ratio(host(got), dl, bound) <= 1.0
        if d * h * w == 1:
            assert out[0] == 0.0 and not host(count).any() and not host(got).any()


@pytest.mark.parametrize("d,h,w", TV_SHAPES)
def test_tv_inside_the_bounds(d, h, w):
    import fplx
    from fplx import ops
    worst = {}
    for n, c in TV_NC:
        x, _ = WO.logits_case("gpu.tv.%d.%d.%d.%d.%d" % (n, c, d, h, w), n, c, d, h, w)
        r = WO.tv_ref(x, True, GS)
        WO.check_tv_case(r)
        dx = dev(x)
        out, count = _tv_twice(dx, True)
        cnt = host(count)
        assert np.array_equal(cnt[r.count_free], r.count[r.count_free]) and cnt.sum() == 0
        res = {"out0": SO.ratio(out[0], r.out[0], r.out0_bound), "loss": SO.ratio(out[2], r.out[2], r.loss_bound)}
        d1, d2 = ops.wsl_tv_bwd(dx, count, _gs(), True), ops.wsl_tv_bwd(dx, count, _gs(), True)
        assert torch.equal(d1, d2)
        dl, bound = WO.tv_grad_ref(x, cnt, GS, True)
        res["dlogits"] = SO.ratio(host(d1), dl, bound)
        print("tv n%d c%d %dx%dx%d: error / bound %s" % (n, c, d, h, w, res))
        assert max(res.values()) <= 1.0, res
        for k, v in res.items():
            worst[k] = max(worst.get(k, 0.0), v)
        lg = dx.clone().requires_grad_(True)                   # the autograd node gives the same numbers
        loss = fplx.TotalVariationLoss()({"prediction": [lg], "softmax": True})
        assert float(loss.detach()) == float(np.float32(out[2]))
        (loss * GS).backward()
        assert torch.equal(lg.grad, d1)
    assert worst["out0"] > 0 or d * h * w < 64


# ---------------------------------------------------------------- Mumford-Shah

@pytest.mark.parametrize("n,d", [(1, 1), (2, 3)])
@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (17, 65)])
def test_mumford_shah_inside_the_bounds(h, w, n, d):
    import fplx
    from fplx import ops
    k = 0
    for ci in (1, 2):
        for penalty in (1, 2):
            for lam in (0.0, 1.0, 0.25):
                c = (2, 3, 8)[k % 3]
                k += 1
                x, im = WO.logits_case("gpu.ms.%d.%d.%d.%d.%d.%d" % (n, d, h, w, ci, k), n, c, d, h, w, ci)
                r = WO.ms_ref(x, im, penalty, lam, True, GS)
                dx, dim = dev(x), dev(im)
                (o1, cen1), (o2, cen2) = ops.wsl_mumford_shah_fwd(dx, dim, penalty, lam, True), ops.wsl_mumford_shah_fwd(dx, dim, penalty, lam, True)
                assert _same_bits(o1, o2) and torch.equal(cen1, cen2)
                out = host(o1)
                assert out[3] == n * c * d * h * w and tuple(cen1.shape) == (n, d, ci, c)
                res = {"out0": SO.ratio(out[0], r.out[0], r.out0_bound), "out1": SO.ratio(out[1], r.out[1], r.out1_bound),
                       "loss": SO.ratio(out[2], r.out[2], r.loss_bound), "cen": SO.ratio(host(cen1), r.cen, r.cen_bound)}
                d1 = ops.wsl_mumford_shah_bwd(dx, dim, cen1, _gs(), penalty, lam, True)
                d2 = ops.wsl_mumford_shah_bwd(dx, dim, cen1, _gs(), penalty, lam, True)
                assert torch.equal(d1, d2)
                res["dlogits"] = SO.ratio(host(d1), r.dl, r.dl_bound)
                print("ms n%d d%d %dx%d c%d ci%d l%d lambda %g: error / bound %s" % (n, d, h, w, c, ci, penalty, lam, res))
                assert max(res.values()) <= 1.0, res
                if h * w == 1:
                    assert out[1] == 0.0 and abs(out[0]) <= r.out0_bound            # one pixel: I = cen up to rounding, no difference
                lg = dx.clone().requires_grad_(True)
                mod = fplx.MumfordShahLoss({"MumfordShahLoss_penalty": "l%d" % penalty, "MumfordShahLoss_lambda": lam})
                loss = mod({"prediction": lg, "image": dim})
                assert float(loss.detach()) == float(np.float32(out[2]))
                (loss * GS).backward()
                assert torch.equal(lg.grad, d1)


def test_mumford_shah_exact_gradient_term_and_4d_input():
    """softmax = 0, p multiples of 2^-6, l1: every |difference| and every partial sum of them is exact in fp32"""
    import fplx
    from fplx import ops
    n, c, d, h, w, ci = 2, 3, 3, 17, 65, 2
    p, im = WO.dyadic_case("gpu.ms.exact", n, c, d, h, w, ci)
    out_ref, cen_ref, _ = WO.ms_fwd(p, im, 1, 1.0, False)
    assert out_ref[1] * 64 < SO.EXACT_LIMIT
    o, cen = ops.wsl_mumford_shah_fwd(dev(p), dev(im), 1, 1.0, False)
    assert host(o)[1] == out_ref[1]
    r = WO.ms_ref(p, im, 1, 1.0, False, GS)
    got = ops.wsl_mumford_shah_bwd(dev(p), dev(im), cen, _gs(), 1, 1.0, False)
    assert SO.ratio(host(o)[0], r.out[0], r.out0_bound) <= 1.0 and SO.ratio(host(got), r.dl, r.dl_bound) <= 1.0
    # [N, C, H, W]: every sample is one slice - the same numbers as [N, C, 1, H, W]
    x, im = WO.logits_case("gpu.ms.4d", 2, 3, 1, 9, 11, 1)
    a = fplx.MumfordShahLoss()({"prediction": dev(x[:, :, 0]), "image": dev(im[:, :, 0])})
    b = fplx.MumfordShahLoss()({"prediction": dev(x), "image": dev(im)})
    assert torch.equal(a, b)


# ---------------------------------------------------------------- GatedCRF

RGB_ONLY = ((0.8, 0.0, 0.15),)
XY_ONLY = ((1.25, 4.0, 0.0),)
CRF_COMBOS = [(2, 1, WO.DEFAULT_DESC), (3, 2, RGB_ONLY), (8, 1, XY_ONLY), (8, 2, WO.DEFAULT_DESC), (2, 2, XY_ONLY), (3, 1, RGB_ONLY)]


def _crf_twice(x, im, desc, r, softmax):
    from fplx import ops
    (o1, k1), (o2, k2) = ops.wsl_gatedcrf_fwd(x, im, desc, r, softmax), ops.wsl_gatedcrf_fwd(x, im, desc, r, softmax)
    assert _same_bits(o1, o2) and torch.equal(k1, k2)
    return host(o1), k1


# 3x4: every window at r = 5 is mostly padding; 33x47: two tiles of 16 and one pixel more in H, three tiles less one pixel in W
@pytest.mark.parametrize("h,w", [(1, 1), (3, 4), (11, 9), (33, 47)])
@pytest.mark.parametrize("radius", [1, 2, 5])
def test_gatedcrf_inside_the_bounds(radius, h, w):
    import fplx
    from fplx import ops
    n, d = 2, 3
    first = (radius + h) % 2 * 3
    for c, ci, desc in CRF_COMBOS[first:first + 3]:
        x, im = WO.logits_case("gpu.crf.%d.%d.%d.%d.%d" % (radius, h, w, c, ci), n, c, d, h, w, ci)
        r = WO.crf_ref(x, im, desc, radius, True, GS)
        dx, dim = dev(x), dev(im)
        out, kp = _crf_twice(dx, dim, desc, radius, True)
        assert out[1] == 0.0 and out[3] == n * d * h * w
        res = {"out0": SO.ratio(out[0], r.out[0], r.out0_bound), "loss": SO.ratio(out[2], r.out[2], r.loss_bound),
               "kp": SO.ratio(host(kp), r.kp, r.kp_bound)}
        d1, d2 = ops.wsl_gatedcrf_bwd(dx, kp, _gs(), True), ops.wsl_gatedcrf_bwd(dx, kp, _gs(), True)
        assert torch.equal(d1, d2)
        res["dlogits"] = SO.ratio(host(d1), r.dl, r.dl_bound)
        print("crf r%d %dx%d c%d ci%d nk%d: error / bound %s" % (radius, h, w, c, ci, len(desc), res))
        assert max(res.values()) <= 1.0, res
        assert out[0] > 0                                      # padding positions count: even one pixel has a loss
        if any(row[2] > 0 for row in desc):                    # the loss class: same numbers through the reference's signature
            lg = dx.clone().requires_grad_(True)
            kd = [dict({"weight": wt}, **dict(([("xy", sxy)] if sxy else []) + ([("rgb", srgb)] if srgb else []))) for wt, sxy, srgb in desc]
            loss = fplx.GatedCRFLoss()(lg, kd, float(radius), {"rgb": dim}, h, w, softmax=True)["loss"]
            assert float(loss.detach()) == float(np.float32(out[2]))
            (loss * GS).backward()
            assert torch.equal(lg.grad, d1)


def test_gatedcrf_one_hot_is_a_plain_sum_of_pair_weights():
    """softmax = 0 and one-hot p: 1 - p(i) . p(j) is exactly 0 or 1, so out0 is the sum of the weights of the pairs that disagree"""
    from fplx import ops
    n, c, d, h, w, ci, radius = 2, 3, 3, 11, 9, 1, 2
    p, im = WO.one_hot_case("gpu.crf.onehot", n, c, d, h, w, ci)
    r = WO.crf_ref(p, im, WO.DEFAULT_DESC, radius, False, GS)
    out, kp = _crf_twice(dev(p), dev(im), WO.DEFAULT_DESC, radius, False)
    assert SO.ratio(out[0], r.out[0], r.out0_bound) <= 1.0 and SO.ratio(host(kp), r.kp, r.kp_bound) <= 1.0
    got = ops.wsl_gatedcrf_bwd(dev(p), kp, _gs(), False)
    assert SO.ratio(host(got), r.dl, r.dl_bound) <= 1.0
    # [N, C, H, W] probabilities through the reference's signature: the slices of the 5-D call
    import fplx
    p4 = np.ascontiguousarray(p.transpose(0, 2, 1, 3, 4)).reshape(n * d, c, h, w)
    i4 = np.ascontiguousarray(im.transpose(0, 2, 1, 3, 4)).reshape(n * d, ci, h, w)
    kd = [{'weight': 1.0, 'xy': 5, 'rgb': 0.1}, {'weight': 1.0, 'xy': 3}]
    loss = fplx.GatedCRFLoss()(dev(p4), kd, radius, {"rgb": dev(i4)}, h, w)["loss"]
    assert float(loss) == float(np.float32(out[2]))


# ---------------------------------------------------------------- one iteration end to end

NAME = "u3d4_ds"
ITER_MAX = 10
RAMP0 = float(np.exp(-5.0))


def _plain_params():
    return dict(C.NETS[NAME], deep_supervise=False, precision="fp32")


def _weights(teacher=False):
    import detdata
    w = {k: v for k, v in C.weights_for(NAME).items() if not k.startswith(("out_conv1", "out_conv2", "out_conv3"))}
    if teacher:
        for k, v in w.items():
            if v.dtype == np.float32 and not k.endswith("running_var"):
                w[k] = (v + 0.02 * detdata.normal("ema." + k, v.shape)).astype(np.float32)
    return w


def _net(teacher=False):
    import fplx
    net = fplx.UNet3D(_plain_params())
    net.load_state_dict({k: torch.from_numpy(v) for k, v in _weights(teacher).items()}, strict=True)
    return net.cuda().train()


def _data():
    return torch.from_numpy(C.input_for(NAME)), torch.from_numpy(C.label_for(NAME))


def _agent(tmp_path, method, iter_valid=2, regularize_w=0.1, learning_rate=1e-2, **wsl_over):
    import fplx
    net = dict(_plain_params(), net_type="UNet3D")
    cfg = {"dataset": {"tensor_type": "float", "root_dir": str(tmp_path)},
           "network": net,
           "training": {"gpus": [0], "loss_type": "DiceLoss", "optimizer": "SGD", "learning_rate": learning_rate, "weight_decay": 0.0,
                        "momentum": 0.0, "lr_scheduler": None, "iter_start": 0, "iter_max": ITER_MAX, "iter_valid": iter_valid,
                        "iter_save": iter_valid, "dual": False, "ckpt_save_dir": str(tmp_path / "model" / method)},
           "testing": {"gpus": [0], "domian_label": 0},
           "weakly_supervised_learning": dict({"wsl_method": method, "regularize_w": regularize_w}, **wsl_over)}
    torch.manual_seed(5)
    return fplx.wsl.wsl_agent_class(method)(cfg, "train")


# regular_w at glob_it = 0 (the ramp is exp(-5) there): the regulariser's share of the gradient must be well above the tolerance
@pytest.mark.parametrize("method,regular_w", [("GatedCRF", 0.5), ("TotalVariation", 200.0)])
def test_iteration_matches_the_cpu_restatement(tmp_path, method, regular_w):
    import fplx
    import nets3d_ref as R3
    from oracle import torch_ref as R
    x, y = _data()
    cfg_w = regular_w / RAMP0
    regular_w = cfg_w * fplx.get_rampup_ratio(0, 0, ITER_MAX, "sigmoid")          # as the agent forms it
    kernels = [{'weight': 1.0, 'xy': 5, 'rgb': 0.1}, {'weight': 1.0, 'xy': 3}]
    # ---- the reference's statements on the CPU (wsl_gatedcrf.py:76-97 / wsl_tv.py:60-66), fp32
    p = _plain_params()
    sd, prm = R.split_state(_weights(False))
    outputs = R3.forward(sd, p, x, True)
    loss_sup = R.dice_loss(outputs, y)
    if method == "GatedCRF":
        loss_reg = WO.crf_statements(outputs, x, WO.DEFAULT_DESC, 5, True)[0]
    else:
        loss_reg = WO.tv_statements(outputs, True)[0]
    g_sup = torch.autograd.grad(loss_sup, list(prm.values()), retain_graph=True, allow_unused=True)
    (loss_sup + regular_w * loss_reg).backward()
    # ---- the same iteration on the GPU
    net = _net()
    opt = fplx.get_optimizer("SGD", net, {"learning_rate": 0.05, "momentum": 0.0, "weight_decay": 0.0})
    out = net(x.cuda())
    l_sup = fplx.DiceLoss()({"prediction": out, "ground_truth": y.cuda()})
    if method == "GatedCRF":
        l_reg = fplx.GatedCRFLoss()(out, kernels, 5, {"rgb": x.cuda()}, x.shape[-2], x.shape[-1], softmax=True)["loss"]
    else:
        l_reg = fplx.TotalVariationLoss()({"prediction": out, "softmax": True})
    loss = l_sup + regular_w * l_reg
    loss.backward()
    assert float((out.detach().cpu() - outputs.detach()).abs().max()) < LOGIT_TOL
    loss_sup, loss_reg, l_sup, l_reg = loss_sup.detach(), loss_reg.detach(), l_sup.detach(), l_reg.detach()
    print("%s: loss_reg cpu %.8g gpu %.8g" % (method, float(loss_reg), float(l_reg)))
    assert abs(float(l_sup) - float(loss_sup)) < 1e-5 and abs(float(l_reg) - float(loss_reg)) < 1e-4 * max(1.0, abs(float(loss_reg)))
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
    opt.step()
    # ---- the agent runs this very iteration: the same parameters bit for bit
    agent = _agent(tmp_path, method, iter_valid=1, regularize_w=cfg_w, learning_rate=0.05)
    net2 = _net()
    agent.net = net2
    agent.create_optimizer()
    agent.create_loss_calculator(1.0)
    agent.set_loaders([{"image": x, "label_prob": y}])
    agent.glob_it = 0
    res = agent.training()
    assert torch.equal(net2.flat_params, net.flat_params)
    loss = loss.detach()
    assert abs(res["loss"] - float(loss)) < 1e-6 * max(1.0, abs(float(loss))) and abs(res["loss_reg"] - float(l_reg)) < 1e-6 * max(1.0, float(l_reg))
    assert res["regular_w"] == regular_w


def test_ustm_iteration_matches_the_cpu_restatement(tmp_path):
    """injected noise, rot_times = 1 on an H != W crop: loss_reg against wsl_ustm.py:81-117 restated on the CPU from the GPU's own
    logits (the networks are compared elsewhere), inside the consistency oracle's bound; the teacher is the EMA afterwards"""
    import fplx
    x, y = _data()
    x, y = x[:1, :, :, :, :8].contiguous(), y[:1, :, :, :, :8].contiguous()       # 16 x 16 x 8
    T = 4
    gen = torch.Generator().manual_seed(33)
    rot_shape = (1, 1, 16, 8, 16)
    shapes = [(1,) + tuple(x.shape), (1,) + rot_shape] + [(2,) + rot_shape] * (T // 2)
    noises = [torch.randn(s, generator=gen) for s in shapes]
    agent = _agent(tmp_path, "USTM", iter_valid=1, regularize_w=1.0, learning_rate=0.05, ustm_mcdroput_n=T)
    agent.net, agent.net_ema = _net(), _net(True)
    agent.create_optimizer()
    agent.create_loss_calculator(1.0)
    agent.set_loaders([{"image": x, "label_prob": y}])
    calls = []

    def noise_source(reps, shape):
        z = noises[len(calls)]
        assert tuple(z.shape) == (reps,) + tuple(shape), (len(calls), z.shape, reps, shape)
        calls.append(shape)
        return z.cuda()

    agent.noise_source, agent.rot_source, agent.glob_it = noise_source, (lambda: 1), 0
    # the same forward passes outside the agent: same inputs, same networks, same dropout streams (all rates are 0)
    clamp = lambda z: torch.clamp(z * 0.1, -0.2, 0.2)
    stu, tea = _net(), _net(True)
    xr = torch.rot90(x, 1, [-2, -1]).contiguous()
    with torch.no_grad():
        s_log = stu((x + clamp(noises[0][0])).cuda())
        t_log = tea((xr + clamp(noises[1][0])).cuda())
        mc = []
        for i in range(T // 2):
            pair = torch.cat([xr + clamp(noises[2 + i][0]), xr + clamp(noises[2 + i][1])], 0)
            mc.append(tea(pair.cuda()).reshape((2,) + tuple(t_log.shape)))
    s_rot = host(torch.rot90(s_log, 1, [-2, -1])).reshape(1, 3, -1)
    t_np, mc_np = host(t_log).reshape(1, 3, -1), host(torch.cat(mc, 0)).reshape(T, 1, 3, -1)
    thr = SO.uamt_threshold(RAMP0, 3)
    r = SO.consistency_ref(s_rot, t_np, mc_np, thr, True)
    res = agent.training()
    assert len(calls) == 2 + T // 2
    print("ustm: loss_reg %.8g oracle %.8g bound %.3g undecided %d" % (res["loss_reg"], r.out[2], r.loss_bound, int(r.undecided.sum())))
    assert abs(res["loss_reg"] - r.out[2]) <= r.loss_bound + 2.0 ** -24 * abs(r.out[2])          # the scalar is read as fp32
    alpha = min(1 - 1 / (ITER_MAX + 1), 0.99)
    tea._ensure_flat()
    ref, bound = SO.ema_ref(host(tea.flat_params), host(agent.net.flat_params), alpha)
    assert SO.ratio(host(agent.net_ema.flat_params), ref, bound) <= 1.0
    stu._ensure_flat()
    assert not torch.equal(agent.net.flat_params, stu.flat_params)              # the student did take its step


# ---------------------------------------------------------------- the five agents

@pytest.mark.parametrize("method", ["EntropyMinimization", "TotalVariation", "MumfordShah", "GatedCRF", "USTM"])
def test_agents_run_one_round_and_write_a_checkpoint(tmp_path, method):
    import fplx
    x, y = _data()
    agent = _agent(tmp_path, method, ustm_mcdroput_n=2)
    agent.config["training"]["iter_max"] = 2
    agent.create_network()
    assert type(agent.net) is fplx.UNet3D
    if method == "USTM":
        assert type(agent.net_ema) is fplx.UNet3D and agent.net_ema.dropout_seed == agent.net.dropout_seed + 1
    else:
        assert agent.net_ema is None
    agent.set_loaders([{"image": x, "label_prob": y}])
    agent.valid_loader_1 = [{"image": x, "label_prob": y}]
    agent.net._ensure_flat()
    student0 = agent.net.flat_params.clone()
    hist = agent.train_valid()
    assert len(hist) == 1
    glob_it, _, tr, va = hist[0]
    assert glob_it == 2
    assert sorted(tr) == ["avg_dice", "class_dice", "loss", "loss_reg", "loss_sup", "regular_w"]
    for k in ("loss", "loss_sup", "loss_reg", "regular_w", "avg_dice"):
        assert np.isfinite(tr[k]), (k, tr[k])
    assert tr["class_dice"].shape == (3,) and np.isfinite(va["loss"])
    assert tr["regular_w"] == 0.1 * fplx.get_rampup_ratio(0, 0, 2, "sigmoid")
    assert tr["loss_reg"] > 0 or (method == "USTM" and tr["loss_reg"] == 0)
    assert abs(tr["loss"] - (tr["loss_sup"] + tr["regular_w"] * tr["loss_reg"])) < 1e-5 * max(1.0, abs(tr["loss"]))
    assert not torch.equal(student0, agent.net.flat_params)
    ck = tmp_path / "model" / method
    files = sorted(os.listdir(str(ck)))
    assert any(f.endswith("_latest.txt") for f in files) and any(f.endswith("_2.pt") for f in files)
    pt = torch.load(str(ck / [f for f in files if f.endswith("_2.pt")][0]), map_location="cpu", weights_only=False)
    assert list(pt["model_state_dict"]) == list(agent.net.state_dict()) and not any("ema" in k for k in pt)


# ---------------------------------------------------------------- python -m fplx.wsl_main train config.cfg

WSL_CFG = """
[dataset]
tensor_type = float
task_type = seg
root_dir  = {root}
train_csv = {root}/train.csv
valid_csv = {root}/valid.csv
test_csv  = {root}/test.csv
train_batch_size = 2
modal_num = 1

train_transform = [NormalizeWithMeanStd, Pad, RandomCrop, RandomFlip, {label_transform}]
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
PartialLabelToProbability_class_num = 2
PartialLabelToProbability_inverse   = False

[network]
net_type = {net_type}
class_num     = 2
in_chns       = 1
{net_keys}

[training]
gpus       = [0]
loss_type     = {loss_type}
optimizer     = Adam
learning_rate = 1e-2
momentum      = 0.9
weight_decay  = 1e-5
lr_scheduler  = MultiStepLR
lr_gamma      = 0.5
lr_milestones = [10000, 20000]
ckpt_save_dir    = {root}/model/wsl
iter_start = 0
iter_max   = 4
iter_valid = 2
iter_save  = 2

[weakly_supervised_learning]
wsl_method = {method}
regularize_w = 0.1
ema_decay = 0.99
rampup_start = 0
rampup_end = 4
ustm_mcdroput_n = 2
GatedCRFLoss_Radius = 3

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


@pytest.mark.parametrize("method,net_type,scribble", [("GatedCRF", "UNet2D5", True), ("TotalVariation", "UNet3D", True),
                                                      ("MumfordShah", "UNet2D5", False), ("USTM", "UNet3D", False),
                                                      ("EntropyMinimization", "UNet3D", False)])
def test_wsl_main_trains_and_tests_from_a_cfg(tmp_path, method, net_type, scribble):
    """the reference's key surface (train_csv / valid_csv, [weakly_supervised_learning]) over synthetic .nii.gz cases; with
    `scribble` the training labels are scribbles (label 2 = not annotated) through PartialLabelToProbability"""
    from fplx import wsl_main, nifti
    root = tmp_path
    rs = np.random.RandomState(9)
    for sub in ("img", "lab", "scr"):
        (root / sub).mkdir()
    names = []
    for i in range(5):
        shp = (16, 30 + 2 * (i % 2), 44)
        lab = np.zeros(shp, np.uint8)
        lab[4:12, 8 + i:20 + i, 10:30] = 1
        scr = np.full(shp, 2, np.uint8)                       # two strokes per case: one inside the object, one in the background
        scr[6:10, 12 + i:16 + i, 18:22] = 1
        scr[2:14, 2:5, 2:40] = 0
        img = rs.randn(*shp) * 15 + 90 + 70.0 * lab
        for sub, vol in (("img", img.astype(np.float32)), ("lab", lab), ("scr", scr)):
            nifti.write_nifti(str(root / sub / ("c%d.nii.gz" % i)), vol, (0.5, 0.5, 1.5))
        names.append("c%d.nii.gz" % i)
    tl = "scr" if scribble else "lab"
    (root / "train.csv").write_text("image,label\n" + "\n".join("img/%s,%s/%s" % (n, tl, n) for n in names[:3]) + "\n")
    (root / "valid.csv").write_text("image,label\n" + "img/%s,lab/%s" % (names[3], names[3]) + "\n")
    (root / "test.csv").write_text("image\n" + "img/" + names[4] + "\n")
    cfg = root / "wsl.cfg"
    cfg.write_text(WSL_CFG.format(root=str(root), method=method, net_type=net_type, net_keys=NET_KEYS[net_type],
                                  label_transform="PartialLabelToProbability" if scribble else "LabelToProbability",
                                  loss_type="CrossEntropyLoss" if scribble else "DiceLoss"))
    wsl_main.main(["fplx.wsl_main", "train", str(cfg)])
    files = sorted(os.listdir(str(root / "model" / "wsl")))
    assert "wsl_latest.txt" in files and "wsl_best.txt" in files and "log_train.txt" in files
    assert "wsl_4.pt" in files
    m = nifti.load_nifty_volume_as_4d_array(str(root / "result" / "wsl_test" / names[4]))
    ref = nifti.load_nifty_volume_as_4d_array(str(root / "img" / names[4]))
    assert m["data_array"].dtype == np.uint8 and m["data_array"].shape == ref["data_array"].shape
