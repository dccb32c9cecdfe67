"""-m gpu tests of the noisy-label kernels (csrc/nll.hip through fplx.ops / fplx.nll) against tests/nlloracle.py - the masks and
counts bit for bit, the losses, sums and gradients inside the derived bounds, every kernel twice for the same bits - then the
node against the steps recorded from the reference (tests/golden/nll_steps.npz), one CoTeaching and one TriNet iteration end to
end against the CPU restatement of the networks, one train_valid round of each agent and `nll_main` train -> test."""
import os

import numpy as np
import pytest
import torch

import nets3d_cfg as C
import nlloracle as NO

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nll_steps.npz")
CASES = ["%s.%s.%s" % (m, s, g) for m in ("CoTeaching", "TriNet") for s in ("a", "b") for g in ("mid", "start")]
MASK_NS = (1, 5, 63, 257, 9240, 300001)   # the last: more than 1024 blocks x 256 threads, a block's chunk exceeds its thread count
GRAD_TOL, LOGIT_TOL = 1e-3, 1e-3          # tests/test_gpu_ssl.py / test_gpu_nets3d.py: the floor every config sits at, max-normalised


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------- select_mask

@pytest.mark.parametrize("kind", ["equal", "two", "nan"])
@pytest.mark.parametrize("n", MASK_NS)
def test_rank_mask_is_the_head_of_a_stable_argsort(n, kind):
    from fplx import ops
    x = NO.tie_case("gpu.rank.%s.%d" % (kind, n), n, kind)
    dx = dev(x)
    order = np.argsort(x, kind="stable")                   # NaN last, ties in index order
    kk = NO.keys(x)
    less = int((kk < np.sort(kk)[n // 2]).sum())
    for k in sorted({0, 1, less, min(less + 1, n), n - 1, n}):
        want = np.zeros(n, np.uint8)
        want[order[:k]] = 1
        a = ops.nll_select_mask(dx, ops.NLL_RANK, num_remb=k)
        b = ops.nll_select_mask(dx, ops.NLL_RANK, num_remb=k)
        assert torch.equal(a, b)
        got = host(a)
        assert int(got.sum()) == k and np.array_equal(got, want), (n, kind, k, int(got.sum()))
        assert np.array_equal(got.astype(bool), NO.rank_mask(x, k))


@pytest.mark.parametrize("kind", ["ties", "random", "nan"])
@pytest.mark.parametrize("n", MASK_NS)
def test_below_mask_equals_torch_quantile(n, kind):
    from fplx import ops
    x = NO.tie_case("gpu.below.%s.%d" % (kind, n), n, kind)
    dx = dev(x)
    for q in (0.0, 0.3, 0.72, 1.0):
        thr = torch.quantile(torch.from_numpy(x), q)
        want = (torch.from_numpy(x) < thr).numpy()
        a = ops.nll_select_mask(dx, ops.NLL_BELOW, q=q)
        b = ops.nll_select_mask(dx, ops.NLL_BELOW, q=q)
        assert torch.equal(a, b)
        assert np.array_equal(host(a).astype(bool), want), (n, kind, q, int(host(a).sum()), int(want.sum()))
        if kind == "nan" and n > 2:
            assert not want.any()                            # torch.quantile is NaN: nothing is below it


def test_below_mask_with_a_weight_that_rounds_away():
    """adjacent floats: a + w (b - a) rounds to a for every w < 0.5, and b - (b - a)(1 - w) to b for w > 0.5"""
    from fplx import ops
    a = np.float32(1.0)
    b = np.nextafter(a, np.float32(2.0))
    x = np.array([b, a, b, a, b], np.float32)
    for q in (0.1, 0.3, 0.45, 0.7):
        k, w = ops.nll_quantile_rank(q, 5)
        want = (torch.from_numpy(x) < torch.quantile(torch.from_numpy(x), q)).numpy()
        got = host(ops.nll_select_mask(dev(x), ops.NLL_BELOW, q=q)).astype(bool)
        assert np.array_equal(got, want), (q, k, w)
    x2 = np.array([a, b], np.float32)                      # k = 0, w = 0.4: the threshold is a itself, nothing is below
    assert ops.nll_quantile_rank(0.4, 2) == (0, float(np.float32(0.4)))
    assert not host(ops.nll_select_mask(dev(x2), ops.NLL_BELOW, q=0.4)).any()
    assert host(ops.nll_select_mask(dev(x2), ops.NLL_BELOW, q=0.7)).tolist() == [1, 0]


# ---------------------------------------------------------------- voxel_ce_fwd

def _ce_twice(logits, y):
    from fplx import ops
    la, pa = ops.nll_voxel_ce_fwd(logits, y)
    lb, pb = ops.nll_voxel_ce_fwd(logits, y)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(la, lb)) and torch.equal(pa, pb)
    return la, pa


@pytest.mark.parametrize("v", (1, 5, 63, 9240))
@pytest.mark.parametrize("c", (2, 3, 8))
@pytest.mark.parametrize("n", (1, 3))
def test_voxel_ce_inside_the_bounds(n, c, v):
    for k in (1, 2, 3):
        logits, y = NO.logits_case("gpu.ce.%d.%d.%d.%d" % (n, c, v, k), k, n, c, v)
        loss, part = _ce_twice([dev(l) for l in logits], dev(y))
        assert len(loss) == k and tuple(part.shape[:2]) == (k, n)
        for j in range(k):
            r = NO.voxel_ce(logits[j], y)
            assert NO.ratio(host(loss[j]), r.L, NO.GAMMA_SLACK * r.e_L) <= 1.0, (k, j)
            total = float(host(part[j]).astype(np.float64).sum())
            assert abs(total - r.L.sum()) <= NO.all_sum_bound(r, n, v), (k, j, total, r.L.sum())


def test_voxel_ce_of_saturated_logits_is_the_fp32_expression():
    """logits +-60: p is exactly 1 and 0, the loss exactly -ln(fl(0.999 + 5e-4)) where the label names the winner and
    -ln(fl(5e-4)) where it names the loser - the fp32 product, sum and logarithm"""
    from fplx import ops
    n, c, v = 1, 2, 9240
    win = (np.arange(v) % 2).astype(np.int64)
    lab = ((np.arange(v) // 2) % 2).astype(np.int64)
    lg = np.full((n, c, v), -60.0, np.float32)
    np.put_along_axis(lg, win[None, None, :], 60.0, 1)
    y = np.zeros((n, c, v), np.float32)
    np.put_along_axis(y, lab[None, None, :], 1.0, 1)
    loss, _ = _ce_twice([dev(lg)], dev(y))
    got = host(loss[0])
    f = np.float32
    hi, lo = f(f(1.0) * f(0.999)) + f(5e-4), f(f(0.0) * f(0.999)) + f(5e-4)
    on_device = host(-torch.log(torch.tensor([hi, lo], dtype=torch.float32, device="cuda")))
    exact = np.array([-np.log(np.float64(hi)), -np.log(np.float64(lo))])
    assert np.all(np.abs(on_device.astype(np.float64) - exact) <= NO.E_LOG * NO.U * np.abs(exact))
    want = np.where(win == lab, on_device[0], on_device[1]).astype(np.float32)
    assert np.array_equal(got, want)
    ref, _ = NO.ce_fp32(lg, y)
    assert np.abs(got.astype(np.float64) - ref).max() <= NO.E_LOG * NO.U * np.abs(exact).max()


# ---------------------------------------------------------------- select_fwd / select_bwd on the kernel's own losses

@pytest.mark.parametrize("mode,ratio", [("CoTeaching", 0.83), ("TriNet", 0.8)])
@pytest.mark.parametrize("n,c,v", [(3, 3, 9240), (1, 2, 63), (2, 8, 5)])
def test_selected_means_and_gradients(n, c, v, mode, ratio):
    from fplx import ops
    k = len(NO.USES[mode])
    logits, y = NO.logits_case("gpu.sel.%s.%d.%d.%d" % (mode, n, c, v), k, n, c, v)
    dl, dy = [dev(l) for l in logits], dev(y)
    loss, part = ops.nll_voxel_ce_fwd(dl, dy)
    nv = n * v
    if mode == "CoTeaching":
        masks = [ops.nll_select_mask(l, ops.NLL_RANK, num_remb=int(ratio * nv)) for l in loss]
        want = [NO.rank_mask(host(l), int(ratio * nv)) for l in loss]
    else:
        masks = [ops.nll_select_mask(l, ops.NLL_BELOW, q=ratio) for l in loss]
        want = [NO.below_mask(host(l), ratio) for l in loss]
    for m, w in zip(masks, want):                           # exact, given the device's own fp32 losses
        assert np.array_equal(host(m).astype(bool), w)
    uses = ops.NLL_USES[mode]
    out = ops.nll_select_fwd(loss, masks, uses, part)
    out2 = ops.nll_select_fwd(loss, masks, uses, part)
    assert torch.equal(out.view(torch.int64), out2.view(torch.int64))
    refs = [NO.voxel_ce(l, y) for l in logits]
    ref_out, bound, keeps = NO.selected(refs, want, uses)
    got = host(out)
    gs = dev(np.array([0.75], np.float32))
    wj = 1.0 if mode == "CoTeaching" else 1.0 / 3.0
    d = ops.nll_select_bwd(dl, dy, masks, uses, out, gs, wj)
    d2 = ops.nll_select_bwd(dl, dy, masks, uses, out, gs, wj)
    for j in range(k):
        assert got[j, 1] == ref_out[j, 1] > 0, (j, got[j, 1], ref_out[j, 1])
        assert abs(got[j, 0] - ref_out[j, 0]) <= bound[j, 0] and abs(got[j, 2] - ref_out[j, 2]) <= bound[j, 2], (j, got[j], ref_out[j])
        assert abs(got[j, 3] - ref_out[j, 3]) <= NO.all_sum_bound(refs[j], n, v)
        assert got[j, 2] == got[j, 0] / got[j, 1]
        assert torch.equal(d[j].view(torch.int32), d2[j].view(torch.int32))
        g64 = 0.75 * float(np.float32(wj))
        ref_d, ref_b = NO.grad(refs[j], y, keeps[j], int(ref_out[j, 1]), g64)
        assert NO.ratio(host(d[j]), ref_d, ref_b) <= 1.0, j
        assert np.abs(ref_d).max() > 1e3 * ref_b.max()
        assert not host(d[j]).reshape(n, c, v)[np.broadcast_to(~keeps[j].reshape(n, 1, v), (n, c, v))].any()


def test_an_empty_selection_gives_nan_and_zero_gradients():
    from fplx import ops
    logits, y = NO.logits_case("gpu.empty", 2, 1, 3, 63)
    dl, dy = [dev(l) for l in logits], dev(y)
    loss, part = ops.nll_voxel_ce_fwd(dl, dy)
    none = [ops.nll_select_mask(l, ops.NLL_RANK, num_remb=0) for l in loss]
    assert not any(host(m).any() for m in none)
    out = ops.nll_select_fwd(loss, none, (2, 1), part)
    got = host(out)
    assert np.all(got[:, 0] == 0) and np.all(got[:, 1] == 0) and np.all(np.isnan(got[:, 2])) and np.all(got[:, 3] > 0)
    d = ops.nll_select_bwd(dl, dy, none, (2, 1), out, dev(np.ones(1, np.float32)), 1.0)
    assert all(not host(t).any() for t in d)
    every = [ops.nll_select_mask(l, ops.NLL_RANK, num_remb=63) for l in loss]
    assert all(host(m).all() for m in every)
    got = host(ops.nll_select_fwd(loss, every, (2, 1), part))
    assert np.all(got[:, 1] == 63)


# ---------------------------------------------------------------- the node against the reference's recorded steps

@pytest.mark.parametrize("tag", CASES)
def test_node_reproduces_the_reference_step(tag):
    import fplx
    z = np.load(GOLDEN)
    method = tag.split(".")[0]
    k = 2 if method == "CoTeaching" else 3
    logits = [z[tag + ".logits%d" % (j + 1)] for j in range(k)]
    y, ratio = z[tag + ".label"], float(z[tag + ".ratio"])
    r = NO.node(logits, y, method, ratio)
    assert r.undecided == 0
    leaves = [dev(l).requires_grad_(True) for l in logits]
    holder = {}
    loss = fplx.selective_ce_loss(leaves, dev(y), method, ratio, holder)
    loss.backward()
    out = host(holder["out"])
    for j in range(k):
        assert out[j, 1] == r.out[j, 1], (tag, j, out[j, 1], r.out[j, 1])                 # kept counts: exact
        assert np.array_equal(host(holder["masks"][j]).astype(bool), r.masks[j])
        # device against the fixture: the device's bound plus the reference's own fp32 error (nlloracle, "the reference")
        tol = 2.0 * r.grad_bounds[j]
        assert NO.ratio(host(leaves[j].grad), z[tag + ".dlogits%d" % (j + 1)], tol) <= 1.0, (tag, j)
    n = r.refs[0].L.size
    for j in range(2):
        keep, m = r.keeps[j], int(r.out[j, 1])
        ref_b = NO.GAMMA_SLACK * (float(r.refs[j].e_L[keep].sum()) / m + (m + 1) * NO.U * float(np.abs(r.refs[j].L[keep]).mean())) \
            + NO.U * abs(r.out[j, 2])
        assert abs(out[j, 2] - float(z[tag + ".loss%d" % (j + 1)])) <= r.out_bound[j, 2] + ref_b, (tag, j)
        ref_bn = NO.GAMMA_SLACK * (float(r.refs[j].e_L.sum()) / n + (n + 1) * NO.U * float(np.abs(r.refs[j].L).mean()))
        assert abs(out[j, 3] / n - float(z[tag + ".loss_no_select%d" % (j + 1)])) <= NO.all_sum_bound(r.refs[j], y.shape[0], n // y.shape[0]) / n + ref_bn
    assert abs(float(loss.detach()) - r.scalar) <= r.scalar_bound + NO.U * abs(r.scalar)              # the fp32 result of the double scalar


# ---------------------------------------------------------------- one iteration end to end

NAME = "u3d4_ds"


def _plain_params():
    return dict(C.NETS[NAME], deep_supervise=False, precision="fp32")


def _weights(member):
    """three points of one family: every float tensor of member 1, 2 nudged (draws nll2, nll3), variances kept positive.
    The draw nll1 is not used: with it UNet3D's parameter gradients differ from tests/nets3d_ref.py by up to 1.4e-2
    (max-normalised) under a plain cross entropy, logits agreeing to 1e-5, while seven other draws sit at 1e-5.  That is no fault
    of the backward: with nll1 the device takes ONE LeakyReLU sign differently from the CPU (a pre-activation of 2e-6, inside its
    own round-off), and against float64 with the device's decisions forced every gradient is within round-off
    (tests/test_gpu_net_backward_exact.py, case u3d4_ds.plain.nll1).  A comparison with the free restatement at
    1e-3, as below, still has to avoid such a draw."""
    import detdata
    w = {k: v for k, v in C.weights_for(NAME).items() if not k.startswith(("out_conv1", "out_conv2", "out_conv3"))}
    if member:
        for k, v in w.items():
            if v.dtype == np.float32 and not k.endswith("running_var"):
                w[k] = (v + 0.02 * detdata.normal("nll%d.%s" % (member + 1, k), v.shape)).astype(np.float32)
    return w


def _noisy_label():
    y = C.label_for(NAME).copy()
    y[:, :, 3:6, 2:9, 4:11] = 0.0                          # a block of wrong labels: class 0 everywhere in it
    y[:, 0, 3:6, 2:9, 4:11] = 1.0
    y[:, :, 9:12, 6:13, 3:8] = 0.0
    y[:, 1, 9:12, 6:13, 3:8] = 1.0
    return y


@pytest.mark.parametrize("method,ratio", [("CoTeaching", 0.8), ("TriNet", 0.8)])
def test_one_iteration_matches_the_cpu_restatement(method, ratio):
    """The networks' forward and backward in torch on the CPU (tests/nets3d_ref.py), the reference's loss statements on the CPU
    logits with the selection the GPU made (the masks are piecewise constant: no gradient flows through them, and logits that
    differ by LOGIT_TOL may order two nearly equal losses differently), then every parameter gradient of every member."""
    import fplx
    import nets3d_ref as R3
    from oracle import torch_ref as R
    k = 2 if method == "CoTeaching" else 3
    p = _plain_params()
    x, y = torch.from_numpy(C.input_for(NAME)), torch.from_numpy(_noisy_label())
    group = (fplx.BiNet if method == "CoTeaching" else fplx.TriNet)(dict(p, net_type="UNet3D"))
    for i, m in enumerate(group.members()):
        m.load_state_dict({kk: torch.from_numpy(v) for kk, v in _weights(i).items()}, strict=True)
    group.cuda().train()
    outs = group(x.cuda())
    assert isinstance(outs, tuple) and len(outs) == k
    holder = {}
    loss = fplx.selective_ce_loss(outs, y.cuda(), method, ratio, holder)
    loss.backward()
    masks = [holder["masks"][j].cpu().bool() for j in range(k)]
    for j in range(k):                                     # the selection is exact on the device's own losses
        lj = host(holder["losses"][j])
        want = NO.rank_mask(lj, int(ratio * lj.size)) if method == "CoTeaching" else NO.below_mask(lj, ratio)
        assert np.array_equal(masks[j].numpy(), want)
    # ---- the CPU restatement
    c = y.shape[1]
    y2d = y.reshape(y.shape[0], c, -1).permute(0, 2, 1).reshape(-1, c)
    prms, losses = [], []
    for j in range(k):
        sd, prm = R.split_state(_weights(j))
        o = R3.forward(sd, p, x, True)
        assert float((outs[j].detach().cpu() - o.detach()).abs().max()) < LOGIT_TOL
        prob = torch.softmax(o, dim=1)
        p2d = prob.reshape(prob.shape[0], c, -1).permute(0, 2, 1).reshape(-1, c) * 0.999 + 5e-4
        losses.append(torch.sum(-y2d * torch.log(p2d), dim=1))
        prms.append(prm)
    if method == "CoTeaching":
        means = [losses[0][masks[1]].mean(), losses[1][masks[0]].mean()]
        total = means[0] + means[1]
    else:
        m12, m13, m23 = masks[0] & masks[1], masks[0] & masks[2], masks[1] & masks[2]
        means = [torch.sum(losses[0] * m23) / m23.sum(), torch.sum(losses[1] * m13) / m13.sum(), torch.sum(losses[2] * m12) / m12.sum()]
        total = (means[0] + means[1] + means[2]) / 3
    total.backward()
    out = host(holder["out"])
    assert abs(float(loss.detach()) - float(total.detach())) < 1e-5 * max(1.0, abs(float(total)) * 100)
    for j in range(k):
        assert abs(out[j, 2] - float(means[j])) < 1e-5 * max(1.0, abs(float(means[j])) * 100)
        named = dict(group.members()[j].named_parameters())
        checked = 0
        for kk, t in prms[j].items():
            if t.grad is None:
                continue
            ref, got = t.grad.numpy(), host(named[kk].grad)
            parts = kk.rsplit(".", 2)
            if kk.endswith("bias") and ".conv_conv." in kk and parts[1] in ("0", "4"):    # in front of train-mode BatchNorm: exactly 0
                assert np.abs(got).max() == 0.0 and np.abs(ref).max() < 1e-5, kk
                continue
            np.testing.assert_allclose(got, ref, atol=max(GRAD_TOL * np.abs(ref).max(), 2e-7), rtol=0, err_msg="net%d.%s" % (j + 1, kk))
            checked += 1
        assert checked >= 10


# ---------------------------------------------------------------- the agents

def _agent(tmp_path, method, optimizer="SGD", iter_valid=2):
    import fplx
    net = dict(_plain_params(), net_type="UNet3D")
    cfg = {"dataset": {"tensor_type": "float", "root_dir": str(tmp_path)},
           "network": net,
           "training": {"gpus": [0], "loss_type": "CrossEntropyLoss", "optimizer": optimizer, "learning_rate": 1e-2, "weight_decay": 0.0,
                        "momentum": 0.9, "lr_scheduler": "MultiStepLR", "lr_gamma": 0.5, "lr_milestones": [1], "iter_start": 0,
                        "iter_max": 2, "iter_valid": iter_valid, "iter_save": iter_valid, "ckpt_save_dir": str(tmp_path / "model" / method)},
           "testing": {"gpus": [0], "domian_label": 0},
           "noisy_label_learning": {"nll_method": method, "co_teaching_select_ratio": 0.6, "trinet_select_ratio": 0.6,
                                    "rampup_start": 0, "rampup_end": 2}}
    torch.manual_seed(5)
    return fplx.nll_agent_class(method)(cfg, "train")


@pytest.mark.parametrize("method,optimizer", [("CoTeaching", "Adam"), ("TriNet", "SGD")])
def test_agents_run_one_round_and_reload_their_checkpoint(tmp_path, method, optimizer):
    import fplx
    x, y = torch.from_numpy(C.input_for(NAME)), torch.from_numpy(_noisy_label())
    agent = _agent(tmp_path, method, optimizer)
    agent.create_network()
    count = 2 if method == "CoTeaching" else 3
    assert type(agent.net) is (fplx.BiNet if count == 2 else fplx.TriNet)
    assert [m.dropout_seed for m in agent.net.members()] == [1 + i for i in range(count)]
    agent.set_loaders([{"image": x, "label_prob": y}])
    agent.valid_loader_1 = [{"image": x, "label_prob": y}]
    for m in agent.net.members():
        m._ensure_flat()
    before = [m.flat_params.clone() for m in agent.net.members()]
    hist = agent.train_valid()
    assert len(hist) == 1
    glob_it, lr_value, tr, va = hist[0]
    assert glob_it == 2 and lr_value == 1e-2 and agent.optimizer.param_groups[0]['lr'] == 5e-3      # the scheduler drives the group
    assert all(m.param_groups[0]['lr'] in (1e-2, 5e-3) for m in agent.optimizer.members)
    assert sorted(tr) == ["avg_dice", "class_dice", "loss", "loss1", "loss2", "loss_no_select1", "loss_no_select2", "select_ratio"]
    for kk in ("loss", "loss1", "loss2", "loss_no_select1", "loss_no_select2", "avg_dice"):
        assert np.isfinite(tr[kk]), (kk, tr[kk])
    assert abs(tr["loss"] - (tr["loss1"] + tr["loss2"]) / 2) < 1e-6
    mode = "sigmoid" if method == "CoTeaching" else "linear"
    assert tr["select_ratio"] == 1 - (1 - 0.6) * fplx.get_rampup_ratio(0, 0, 2, mode)
    assert tr["class_dice"].shape == (3,) and np.isfinite(va["loss"])
    for b, m in zip(before, agent.net.members()):
        assert not torch.equal(b, m.flat_params)
    ck = tmp_path / "model" / method
    files = sorted(os.listdir(str(ck)))
    assert any(f.endswith("_latest.txt") for f in files) and any(f.endswith("_2.pt") for f in files)
    pt = torch.load(str(ck / [f for f in files if f.endswith("_2.pt")][0]), map_location="cpu", weights_only=False)
    keys = list(pt["model_state_dict"])
    assert keys == list(agent.net.state_dict()) and keys[0].startswith("net1.") and keys[-1].startswith("net%d." % count)
    assert sorted(pt["optimizer_state_dict"]) == ["members", "param_groups"] and len(pt["optimizer_state_dict"]["members"]) == count
    agent.config["testing"]["ckpt_mode"] = 0
    test = fplx.nll_agent_class(method)(agent.config, "test")
    test.create_network()
    test.set_loaders(test_loader=[{"image": x[:1], "names": ["case0.nii.gz"]}])
    pred = test.infer()
    for kk, v in agent.net.state_dict().items():
        assert torch.equal(test.net.state_dict()[kk].cpu(), v.cpu()), kk
    assert pred["case0.nii.gz"].shape == tuple(x.shape[2:])


# ---------------------------------------------------------------- python -m fplx.nll_main train config.cfg

NLL_CFG = """
[dataset]
tensor_type = float
task_type = seg
root_dir  = {root}
train_csv = {root}/train.csv
valid_csv = {root}/valid.csv
test_csv  = {root}/test.csv
train_batch_size = 2
modal_num = 1

train_transform = [NormalizeWithMeanStd, Pad, RandomCrop, RandomFlip, LabelToProbability]
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
net_type = UNet3D
class_num     = 2
in_chns       = 1
feature_chns  = [8, 16, 32, 64]
dropout       = [0.0, 0.0, 0.3, 0.4]
trilinear     = False
deep_supervise = False

[training]
gpus       = [0]
loss_type     = CrossEntropyLoss
optimizer     = Adam
learning_rate = 1e-2
momentum      = 0.9
weight_decay  = 1e-5
lr_scheduler  = MultiStepLR
lr_gamma      = 0.5
lr_milestones = [10000, 20000]
ckpt_save_dir    = {root}/model/nll
iter_start = 0
iter_max   = 4
iter_valid = 2
iter_save  = 2

[noisy_label_learning]
nll_method = {method}
co_teaching_select_ratio = 0.8
trinet_select_ratio = 0.8
rampup_start = 0
rampup_end = 4

[testing]
gpus       = [0]
ckpt_mode         = 1
output_dir        = {root}/result
evaluation_mode   = True
sliding_window_enable = True
sliding_window_size   = [16, 32, 32]
sliding_window_stride = [16, 32, 32]
"""


@pytest.mark.parametrize("method", ["CoTeaching", "TriNet"])
def test_nll_main_trains_and_tests_from_a_cfg(tmp_path, method):
    """the reference's key surface over synthetic .nii.gz cases: two validation rounds with checkpoints that hold the whole
    BiNet / TriNet, then the NLL agent reloads the best one and predicts the test case"""
    from fplx import nll_main, nifti
    root = tmp_path
    rs = np.random.RandomState(9)
    (root / "img").mkdir()
    (root / "lab").mkdir()
    names = []
    for i in range(4):
        shp = (16, 30 + 2 * (i % 2), 44)
        lab = np.zeros(shp, np.uint8)
        lab[4:12, 8 + i:20 + i, 10:30] = 1
        img = rs.randn(*shp) * 15 + 90 + 70.0 * lab
        if i < 2:
            lab[2:5, 4:9, 30:40] = 1                        # the training labels are partly wrong
        nifti.write_nifti(str(root / "img" / ("c%d.nii.gz" % i)), img.astype(np.float32), (0.5, 0.5, 1.5))
        nifti.write_nifti(str(root / "lab" / ("c%d.nii.gz" % i)), lab, (0.5, 0.5, 1.5))
        names.append("c%d.nii.gz" % i)
    (root / "train.csv").write_text("image,label\n" + "\n".join("img/%s,lab/%s" % (n, n) for n in names[:2]) + "\n")
    (root / "valid.csv").write_text("image,label\n" + "img/%s,lab/%s" % (names[2], names[2]) + "\n")
    (root / "test.csv").write_text("image\n" + "img/" + names[3] + "\n")
    cfg = root / "nll.cfg"
    cfg.write_text(NLL_CFG.format(root=str(root), method=method))
    import random
    random.seed(3)
    nll_main.main(["fplx.nll_main", "train", str(cfg)])
    files = sorted(os.listdir(str(root / "model" / "nll")))
    assert "nll_latest.txt" in files and "nll_best.txt" in files and "log_train.txt" in files and "log_test.txt" not in files
    assert "nll_4.pt" in files
    pt = torch.load(str(root / "model" / "nll" / "nll_4.pt"), map_location="cpu", weights_only=False)
    prefixes = sorted({k.split(".")[0] for k in pt["model_state_dict"]})
    assert prefixes == ["net1", "net2"] + (["net3"] if method == "TriNet" else [])
    m = nifti.load_nifty_volume_as_4d_array(str(root / "result" / "nll_test" / names[3]))
    ref = nifti.load_nifty_volume_as_4d_array(str(root / "img" / names[3]))
    assert m["data_array"].dtype == np.uint8 and m["data_array"].shape == ref["data_array"].shape
