"""-m gpu tests of URPC's pyramid consistency and CPS's pseudo labels (csrc/ssl.hip through fplx.ops / fplx.ssl) against
tests/pyramidoracle.py - the exact part bit for bit, the rounding part inside the derived bounds, every kernel twice for the
same bits - then one URPC and one CPS iteration end to end against the CPU restatement of the networks, one train_valid round
of both agents with a checkpoint that loads back, and `python -m fplx.ssl_main` for both methods."""
import os

import numpy as np
import pytest
import torch

import nets3d_cfg as C
import pyramidoracle as PO

pytestmark = pytest.mark.gpu

NS, CS, KS, VS = (1, 3), (2, 3, 8), (2, 3, 4), (1, 5, 63, 9240)
GRAD_TOL, LOGIT_TOL = 1e-3, 1e-3          # tests/test_gpu_ssl.py, tests/test_gpu_nets3d.py: the floor every config sits at, max-normalised
GS = 0.7                                  # a gscale other than 1


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _fwd_twice(ls):
    from fplx import ops
    a, b = ops.ssl_pyramid_fwd(ls), ops.ssl_pyramid_fwd(ls)
    assert torch.equal(_bits(a), _bits(b))
    return a


# ---------------------------------------------------------------- exact part

@pytest.mark.parametrize("v", VS)
@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("n", NS)
def test_identical_scales_give_zero_bit_for_bit(n, c, v):
    """K in {2, 4} copies of one dyadic tensor: m = p_k exactly, so A_k = 0, V_k = 0, B_k = M and loss_reg = 0"""
    z = dev(PO.exact_case("gpu.exact.%d.%d.%d" % (n, c, v), n, c, v))
    M = float(n * v)
    for k in (2, 4):
        out = host(_fwd_twice([z.clone() for _ in range(k)]))
        want = np.array([0.0, M, 0.0, 0.0] * k + [0.0, 0.0])
        assert out.tobytes() == want.tobytes(), (k, out)


# ---------------------------------------------------------------- rounding part: value and gradient inside the derived bounds

BOUND_CASES = [(k, n, c, v) for v in VS[:3] for k in KS for c in CS for n in NS] + \
              [(k, 1, c, 9240) for k in KS for c in CS] + [(2, 3, 2, 9240), (3, 3, 3, 9240), (4, 3, 8, 9240)]


@pytest.mark.parametrize("k,n,c,v", BOUND_CASES)
def test_pyramid_pair_inside_the_bounds(k, n, c, v):
    from fplx import ops
    z = PO.logits_case("gpu.%d.%d.%d.%d" % (k, n, c, v), k, n, c, v)
    r = PO.pyramid_ref(z, GS)
    ls = [dev(z[i]) for i in range(k)]
    out_t = _fwd_twice(ls)
    out = host(out_t)
    res = PO.check_pyramid_fwd(r, out, "fwd %s" % ((k, n, c, v),))
    print("fwd", (k, n, c, v), {a: round(x, 4) for a, x in res.items()})
    gs = torch.tensor([GS], dtype=torch.float32, device="cuda")
    d1 = ops.ssl_pyramid_bwd(ls, out_t, gs)
    d2 = ops.ssl_pyramid_bwd(ls, out_t, gs)
    dz, bound = PO.pyramid_grad_ref(z, out, GS)
    for j in range(k):
        assert torch.equal(_bits(d1[j]), _bits(d2[j]))
        q = PO.ratio(host(d1[j]), dz[j], bound[j])
        print("bwd", (k, n, c, v), j, round(q, 4))
        assert q <= 1.0, (j, q)
    assert float(np.abs(dz).max()) > 0


@pytest.mark.parametrize("n0,n,c,v,aligned", [(1, 3, 3, 5, False), (1, 2, 2, 9240, True), (2, 3, 8, 63, True)])
def test_the_node_reads_the_unlabelled_rows_and_zeroes_the_rest(n0, n, c, v, aligned):
    """fplx.pyramid_consistency_loss over the joint batch: rows n0: are contiguous views whose base need not be 16-byte aligned
    (n0 = 1, C = 3, V = 5: 60 bytes in - the one-voxel path); a gradient scale other than 1 comes in through autograd"""
    import fplx
    k = 3
    full = PO.logits_case("gpu.node.%d.%d.%d.%d" % (n0, n, c, v), k, n, c, v)
    ts = [dev(full[i]).requires_grad_(True) for i in range(k)]
    assert (ts[0][n0:].data_ptr() % 16 == 0) == aligned
    holder = {}
    loss = fplx.pyramid_consistency_loss(ts, n0, holder)
    (loss * GS).backward()
    z = np.ascontiguousarray(full[:, n0:])
    r = PO.pyramid_ref(z, GS)
    out = host(holder["out"])
    PO.check_pyramid_fwd(r, out, "node")
    assert float(loss.detach()) == float(np.float32(out[4 * k]))
    dz, bound = PO.pyramid_grad_ref(z, out, GS)
    for j in range(k):
        g = host(ts[j].grad)
        assert g.shape == full[j].shape and not g[:n0].any()                 # exactly 0
        assert PO.ratio(g[n0:], dz[j], bound[j]) <= 1.0, j


# ---------------------------------------------------------------- CPS's pseudo labels

@pytest.mark.parametrize("k,n,c,v", [(1, 1, 2, 1), (2, 3, 3, 5), (3, 1, 8, 63), (2, 3, 2, 9240), (3, 1, 3, 9240), (2, 1, 8, 9240)])
def test_pseudo_onehot_is_the_references_bit_for_bit(k, n, c, v):
    from fplx import ops
    z = PO.onehot_case("gpu.onehot.%d.%d.%d.%d" % (k, n, c, v), k, n, c, v)
    assert PO.grid_is_separated(z)
    ls = [dev(z[i]) for i in range(k)]
    a, b = ops.ssl_pseudo_onehot(ls), ops.ssl_pseudo_onehot(ls)
    want = PO.pseudo_onehot(z)
    for j in range(k):
        assert torch.equal(a[j], b[j])
        soft = torch.softmax(torch.from_numpy(z[j]), dim=1)                  # ssl_cps.py:94,103-106 (get_soft_label: a scatter of ones)
        ref = torch.zeros_like(soft).scatter_(1, torch.argmax(soft, dim=1, keepdim=True), 1.0).numpy()
        got = host(a[j])
        assert got.dtype == np.float32 and got.tobytes() == ref.tobytes() and np.array_equal(got, want[j]), j


def test_cross_pseudo_labels_are_detached_views_of_any_alignment():
    import fplx
    z = PO.onehot_case("gpu.onehot.node", 2, 3, 3, 5)
    ts = [dev(z[i]).requires_grad_(True) for i in range(2)]
    oh = fplx.cross_pseudo_labels([t[1:] for t in ts])
    want = PO.pseudo_onehot(z[:, 1:])
    for j in range(2):
        assert not oh[j].requires_grad and np.array_equal(host(oh[j]), want[j])


# ---------------------------------------------------------------- one iteration of each trainer end to end

NAME = "u3d4_ds"
ITER_MAX = 10
REG_W_CFG = 5.0 / float(np.exp(-5.0))          # regular_w = 5 at glob_it = 0: the regulariser's gradient is well above the tolerance


def _params(deep):
    return dict(C.NETS[NAME], deep_supervise=deep, precision="fp32")


def _weights(member, deep):
    """member 0: the fixture's draw; member 1: every float tensor nudged by the draw `cps2` (variances kept positive).  The draw
    `nll1` is not used: tests/test_gpu_nll.py records that UNet3D's parameter gradients differ from tests/nets3d_ref.py by up to
    1.4e-2 with it - one LeakyReLU sign that the device and the CPU take differently, not a fault of the backward
    (tests/test_gpu_net_backward_exact.py, case u3d4_ds.plain.nll1)."""
    import detdata
    w = dict(C.weights_for(NAME))
    if not deep:
        w = {k: v for k, v in w.items() if not k.startswith(("out_conv1", "out_conv2", "out_conv3"))}
    if member:
        for k, v in w.items():
            if v.dtype == np.float32 and not k.endswith("running_var"):
                w[k] = (v + 0.02 * detdata.normal("cps%d.%s" % (member + 1, k), v.shape)).astype(np.float32)
    return w


def _data():
    x, y = torch.from_numpy(C.input_for(NAME)), torch.from_numpy(C.label_for(NAME))
    return x[:1], y[:1], x[1:]


def _compare_grads(prm, named, what, g_other=None):
    checked = moved = 0
    for i, (k, t) in enumerate(prm.items()):
        if t.grad is None:
            continue
        ref, got = t.grad.numpy(), host(named[k].grad)
        parts = k.rsplit(".", 2)
        if k.endswith("bias") and ".conv_conv." in k and parts[1] in ("0", "4"):      # in front of train-mode BatchNorm: exactly 0
            assert np.abs(got).max() == 0.0 and np.abs(ref).max() < 1e-5, k
            continue
        tol = max(GRAD_TOL * np.abs(ref).max(), 2e-7)
        np.testing.assert_allclose(got, ref, atol=tol, rtol=0, err_msg="%s %s" % (what, k))
        checked += 1
        if g_other is not None and g_other[i] is not None and float((t.grad - g_other[i]).abs().max()) > 10 * tol:
            moved += 1
    assert checked >= 10
    return moved


def _urpc_reg(outputs, n0):
    """ssl_urpc.py:76-91 with torch operations, fp32 on the CPU"""
    kl_distance = torch.nn.KLDivLoss(reduction='none')
    soft = [torch.softmax(o, dim=1) for o in outputs]
    avg = torch.mean(torch.stack(soft), dim=0)[n0:] * 0.99 + 0.005
    loss_reg = 0.0
    for s in soft:
        p1_i = s[n0:] * 0.99 + 0.005
        var = torch.sum(kl_distance(torch.log(p1_i), avg), dim=1, keepdim=True)
        exp_var = torch.exp(-var)
        loss_reg = loss_reg + torch.mean(torch.square(avg - p1_i) * exp_var) / (torch.mean(exp_var) + 1e-8) + torch.mean(var)
    return loss_reg / len(outputs)


def _agent(tmp_path, method, iter_valid=2, regularize_w=0.1, learning_rate=1e-2, optimizer="SGD"):
    import fplx
    net = dict(_params(method == "URPC"), net_type="UNet3D")
    cfg = {"dataset": {"tensor_type": "float", "root_dir": str(tmp_path)},
           "network": net,
           "training": {"gpus": [0], "loss_type": "DiceLoss", "optimizer": optimizer, "learning_rate": learning_rate, "weight_decay": 0.0,
                        "momentum": 0.0, "lr_scheduler": None, "iter_start": 0, "iter_max": ITER_MAX, "iter_valid": iter_valid,
                        "iter_save": iter_valid, "dual": False, "ckpt_save_dir": str(tmp_path / "model" / method)},
           "testing": {"gpus": [0], "domian_label": 0},
           "semi_supervised_learning": {"ssl_method": method, "regularize_w": regularize_w}}
    torch.manual_seed(5)
    return fplx.ssl_agent_class_all(method)(cfg, "train")


def test_urpc_iteration_matches_the_cpu_restatement(tmp_path):
    """UNet3D with deep supervision (four full-resolution outputs), DiceLoss through DeepSuperviseLoss on the labelled row, the
    pyramid regulariser on the unlabelled one.  Weights: the fixture's own draw (not `nll1`, see _weights)."""
    import fplx
    import nets3d_ref as R3
    from oracle import torch_ref as R
    x0, y0, x1 = _data()
    regular_w = REG_W_CFG * fplx.get_rampup_ratio(0, 0, ITER_MAX, "sigmoid")
    p = _params(True)
    sd, prm = R.split_state(_weights(0, True))
    outputs = R3.forward(sd, p, torch.cat([x0, x1], dim=0), True)
    assert isinstance(outputs, (list, tuple)) and len(outputs) == 4
    loss_sup = R3.loss_of([o[:1] for o in outputs], y0)
    loss_reg = _urpc_reg(outputs, 1)
    g_sup = torch.autograd.grad(loss_sup, list(prm.values()), retain_graph=True, allow_unused=True)
    (loss_sup + regular_w * loss_reg).backward()
    # ---- the same iteration on the GPU
    net = fplx.UNet3D(p)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in _weights(0, True).items()}, strict=True)
    net.cuda().train()
    out = net(torch.cat([x0, x1], dim=0).cuda())
    assert isinstance(out, (list, tuple)) and len(out) == 4
    lc = fplx.DeepSuperviseLoss({'deep_supervise_weight': None, 'base_loss': fplx.DiceLoss()})
    l_sup = lc({"prediction": [o[:1] for o in out], "ground_truth": y0.cuda()})
    l_reg = fplx.pyramid_consistency_loss(out, 1)
    loss = l_sup + regular_w * l_reg
    loss.backward()
    for a, b in zip(out, outputs):
        assert float((a.detach().cpu() - b.detach()).abs().max()) < LOGIT_TOL
    assert abs(float(l_sup) - float(loss_sup)) < 1e-5 and abs(float(l_reg) - float(loss_reg)) < 1e-5 * max(1.0, float(loss_reg) * 100)
    moved = _compare_grads(prm, dict(net.named_parameters()), "URPC", g_sup)
    assert moved >= 10, "the regulariser's share of the gradient is below the tolerance: the comparison would not see it"
    # ---- the agent runs this very iteration: same parameters after the step, bit for bit
    opt = fplx.get_optimizer("SGD", net, {"learning_rate": 0.05, "momentum": 0.0, "weight_decay": 0.0})
    opt.step()
    agent = _agent(tmp_path, "URPC", iter_valid=1, regularize_w=REG_W_CFG, learning_rate=0.05)
    net2 = fplx.UNet3D(p)
    net2.load_state_dict({k: torch.from_numpy(v) for k, v in _weights(0, True).items()}, strict=True)
    agent.net = net2.cuda().train()
    agent.create_optimizer()
    agent.create_loss_calculator(1.0)
    agent.set_loaders([{"image": x0, "label_prob": y0}])
    agent.set_unlabeled_loader([{"image": x1}])
    agent.glob_it = 0
    res = agent.training()
    assert torch.equal(net2.flat_params, net.flat_params)
    assert abs(res["loss"] - float(loss)) < 1e-6 and abs(res["loss_reg"] - float(l_reg)) < 1e-7 and res["regular_w"] == regular_w
    assert sorted(res) == ["avg_dice", "class_dice", "loss", "loss_reg", "loss_sup", "regular_w"]


def test_cps_iteration_matches_the_cpu_restatement(tmp_path):
    """BiNet of two UNet3D, DiceLoss four times (ssl_cps.py:99-116).  The pseudo labels are the device's (piecewise constant: no
    gradient flows through them, and logits that differ by LOGIT_TOL may order two nearly equal classes differently).
    Weights: the fixture's draw and its `cps2` nudge (not `nll1`, see _weights)."""
    import fplx
    import nets3d_ref as R3
    from oracle import torch_ref as R
    x0, y0, x1 = _data()
    regular_w = REG_W_CFG * fplx.get_rampup_ratio(0, 0, ITER_MAX, "sigmoid")
    p = _params(False)

    def group():
        g = fplx.BiNet(dict(p, net_type="UNet3D"))
        for i, m in enumerate(g.members()):
            m.load_state_dict({k: torch.from_numpy(v) for k, v in _weights(i, False).items()}, strict=True)
        return g.cuda().train()

    net = group()
    o1, o2 = net(torch.cat([x0, x1], dim=0).cuda())
    pse1, pse2 = fplx.cross_pseudo_labels([o1[1:], o2[1:]])
    for o, ps in ((o1, pse1), (o2, pse2)):
        assert torch.equal(ps.argmax(1), o[1:].argmax(1)) and float(ps.sum()) == ps[:, 0].numel()
    dice = fplx.DiceLoss()
    y0d = y0.cuda()
    ls = [dice({"prediction": o1[:1], "ground_truth": y0d}), dice({"prediction": o2[:1], "ground_truth": y0d}),
          dice({"prediction": o1[1:], "ground_truth": pse2}), dice({"prediction": o2[1:], "ground_truth": pse1})]
    loss = (ls[0] + regular_w * ls[2]) + (ls[1] + regular_w * ls[3])
    loss.backward()
    # ---- the CPU restatement
    prms, outs = [], []
    for j in range(2):
        sd, prm = R.split_state(_weights(j, False))
        o = R3.forward(sd, p, torch.cat([x0, x1], dim=0), True)
        assert float(((o1, o2)[j].detach().cpu() - o.detach()).abs().max()) < LOGIT_TOL
        prms.append(prm)
        outs.append(o)
    ref = [R.dice_loss(outs[0][:1], y0), R.dice_loss(outs[1][:1], y0), R.dice_loss(outs[0][1:], pse2.cpu()),
           R.dice_loss(outs[1][1:], pse1.cpu())]
    g_sup = [torch.autograd.grad(ref[j], list(prms[j].values()), retain_graph=True, allow_unused=True) for j in range(2)]
    ((ref[0] + regular_w * ref[2]) + (ref[1] + regular_w * ref[3])).backward()
    for a, b in zip(ls, ref):
        assert abs(float(a) - float(b)) < 1e-5
    for j in range(2):
        moved = _compare_grads(prms[j], dict(net.members()[j].named_parameters()), "CPS net%d" % (j + 1), g_sup[j])
        assert moved >= 10, "the pseudo-supervised share of the gradient is below the tolerance"
    # ---- the agent runs this very iteration
    opt = fplx.GroupOptimizer([fplx.get_optimizer("SGD", m, {"learning_rate": 0.05, "momentum": 0.0, "weight_decay": 0.0})
                               for m in net.members()])
    opt.step()
    agent = _agent(tmp_path, "CPS", iter_valid=1, regularize_w=REG_W_CFG, learning_rate=0.05)
    agent.net = group()
    agent.create_optimizer()
    assert type(agent.optimizer) is fplx.GroupOptimizer
    agent.create_loss_calculator(1.0)
    agent.set_loaders([{"image": x0, "label_prob": y0}])
    agent.set_unlabeled_loader([{"image": x1}])
    agent.glob_it = 0
    res = agent.training()
    for a, b in zip(agent.net.members(), net.members()):
        assert torch.equal(a.flat_params, b.flat_params)
    assert sorted(res) == ["avg_dice", "class_dice", "loss", "loss_pse_sup1", "loss_pse_sup2", "loss_sup1", "loss_sup2", "regular_w"]
    for name, t in (("loss", loss), ("loss_sup1", ls[0]), ("loss_sup2", ls[1]), ("loss_pse_sup1", ls[2]), ("loss_pse_sup2", ls[3])):
        assert abs(res[name] - float(t)) < 1e-6, name
    assert res["regular_w"] == regular_w


# ---------------------------------------------------------------- the two agents

@pytest.mark.parametrize("method", ["URPC", "CPS"])
def test_agents_run_one_round_and_reload_their_checkpoint(tmp_path, method):
    import fplx
    x0, y0, x1 = _data()
    agent = _agent(tmp_path, method)
    agent.config["training"]["iter_max"] = 2
    agent.create_network()
    nets = agent.net.members() if method == "CPS" else [agent.net]
    assert type(agent.net) is (fplx.BiNet if method == "CPS" else fplx.UNet3D) and agent.net_ema is None
    agent.set_loaders([{"image": x0, "label_prob": y0}])
    agent.set_unlabeled_loader([{"image": x1}])
    agent.valid_loader_1 = [{"image": x0, "label_prob": y0}]
    for m in nets:
        m._ensure_flat()
    before = [m.flat_params.clone() for m in nets]
    written = []
    if method == "CPS":
        class Writer(object):
            def add_scalars(self, tag, scalars, step):
                written.append((tag, sorted(scalars), step))
        agent.summ_writer = Writer()
    hist = agent.train_valid()
    assert len(hist) == 1
    glob_it, _, tr, va = hist[0]
    assert glob_it == 2 and np.isfinite(va["loss"]) and tr["class_dice"].shape == (3,)
    assert tr["regular_w"] == 0.1 * fplx.get_rampup_ratio(0, 0, 2, "sigmoid")
    if method == "URPC":
        assert sorted(tr) == ["avg_dice", "class_dice", "loss", "loss_reg", "loss_sup", "regular_w"]
        assert tr["loss_reg"] > 0 and abs(tr["loss"] - (tr["loss_sup"] + tr["regular_w"] * tr["loss_reg"])) < 1e-5
    else:
        assert sorted(tr) == ["avg_dice", "class_dice", "loss", "loss_pse_sup1", "loss_pse_sup2", "loss_sup1", "loss_sup2", "regular_w"]
        total = tr["loss_sup1"] + tr["loss_sup2"] + tr["regular_w"] * (tr["loss_pse_sup1"] + tr["loss_pse_sup2"])
        assert abs(tr["loss"] - total) < 1e-5 and tr["loss_pse_sup1"] > 0 and tr["loss_pse_sup2"] > 0
        tags = [w[0] for w in written]
        assert tags == ["loss", "loss_sup", "loss_pseudo_sup", "regular_w", "lr", "dice", "class_0_dice", "class_1_dice", "class_2_dice"]
        assert written[1][1] == ["net1", "net2"] and all(w[2] == 2 for w in written)
    for b, m in zip(before, nets):
        assert not torch.equal(b, m.flat_params)
    ck = tmp_path / "model" / method
    files = sorted(os.listdir(str(ck)))
    assert any(f.endswith("_latest.txt") for f in files) and any(f.endswith("_2.pt") for f in files)
    pt = torch.load(str(ck / [f for f in files if f.endswith("_2.pt")][0]), map_location="cpu", weights_only=False)
    keys = list(pt["model_state_dict"])
    assert keys == list(agent.net.state_dict())
    if method == "CPS":
        assert keys[0].startswith("net1.") and keys[-1].startswith("net2.")
        assert sorted(pt["optimizer_state_dict"]) == ["members", "param_groups"] and len(pt["optimizer_state_dict"]["members"]) == 2
    agent.config["testing"]["ckpt_mode"] = 0
    test = (fplx.SSLCPS if method == "CPS" else fplx.SegmentationAgent)(agent.config, "test")
    test.create_network()
    test.set_loaders(test_loader=[{"image": x0, "names": ["case0.nii.gz"]}])
    pred = test.infer()
    for k, v in agent.net.state_dict().items():
        assert torch.equal(test.net.state_dict()[k].cpu(), v.cpu()), k
    assert pred["case0.nii.gz"].shape == tuple(x0.shape[2:])


# ---------------------------------------------------------------- python -m fplx.ssl_main train config.cfg

@pytest.mark.parametrize("method,deep", [("URPC", True), ("CPS", False)])
def test_ssl_main_trains_and_tests_from_a_cfg(tmp_path, method, deep):
    """the configuration of tests/test_gpu_ssl.py's ssl_main test with the two new methods: two validation rounds with
    checkpoints, then the best checkpoint predicts the test case (CPS: the BiNet's eval output)"""
    import test_gpu_ssl as T1
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
    net_keys = T1.NET_KEYS["UNet3D"].replace("deep_supervise = False", "deep_supervise = %s" % deep)
    cfg = root / "ssl.cfg"
    cfg.write_text(T1.SSL_CFG.format(root=str(root), method=method, net_type="UNet3D", net_keys=net_keys))
    import random
    random.seed(3)
    ssl_main.main(["fplx.ssl_main", "train", str(cfg)])
    files = sorted(os.listdir(str(root / "model" / "ssl")))
    assert "ssl_latest.txt" in files and "ssl_best.txt" in files and "log_train.txt" in files and "ssl_4.pt" in files
    pt = torch.load(str(root / "model" / "ssl" / "ssl_4.pt"), map_location="cpu", weights_only=False)
    assert any(k.startswith("net2.") for k in pt["model_state_dict"]) == (method == "CPS")
    m = nifti.load_nifty_volume_as_4d_array(str(root / "result" / "ssl_test" / names[5]))
    ref = nifti.load_nifty_volume_as_4d_array(str(root / "img" / names[5]))
    assert m["data_array"].dtype == np.uint8 and m["data_array"].shape == ref["data_array"].shape
    assert set(np.unique(m["data_array"]).tolist()) <= {0, 1}
    os.remove(str(root / "result" / "ssl_test" / names[5]))
    ssl_main.main(["fplx.ssl_main", "test", str(cfg)])             # the test stage alone: the same prediction from the best checkpoint
    m2 = nifti.load_nifty_volume_as_4d_array(str(root / "result" / "ssl_test" / names[5]))
    assert np.array_equal(m2["data_array"], m["data_array"])
