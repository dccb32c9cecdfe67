"""GPU parity of UNet2D5 / UNet3D (fplx/nets3d.py: one schedule over the C ABI, the 1x1x1 head and deep-supervision
interpolation kernels of csrc/head.hip) and DeepSuperviseLoss against
 (a) the fixtures produced by running the reference (fp32: logits <= 1e-3, every output of a list),
 (b) the CPU restatement tests/nets3d_ref.py rounding to bf16 at the stored tensors (bf16),
then checkpoints, the eight fused optimisers, the agent's loops with a four-output network, and the dropout stream."""
import os

import numpy as np
import pytest
import torch

import nets3d_cfg as C

pytestmark = pytest.mark.gpu

# max-normalised gradient tolerance: twice the reference's own fp32 noise - the gap between the reference's fixture and the CPU
# restatement of the same operators, measured per config by tests/test_nets3d_cpu.py - and not below 1e-3.  The measured gap
# is 0 for all five configs (the restatement calls the reference's operators in the reference's order: bit-identical gradients
# on the CPU that wrote the fixtures), so every config sits at the floor.
GRAD_TOL = {"u25": 1e-3, "u25bl3": 1e-3, "u3d": 1e-3, "u3dtri_ds": 1e-3, "u3d4_ds": 1e-3}
LOGIT_TOL = 1e-3


def _net(name, precision="fp32", **over):
    import fplx
    p = dict(C.NETS[name], precision=precision, **over)
    net = fplx.SegNetDict[p["net_type"]](p)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in C.weights_for(name).items()}, strict=True)
    return net.cuda(), p


def _as_list(o):
    return list(o) if isinstance(o, (list, tuple)) else [o]


def _is_bn_fed_bias(k):
    """bias of a 3x3(x3) convolution in front of train-mode BatchNorm: the true gradient is exactly 0"""
    parts = k.rsplit(".", 2)
    return k.endswith("bias") and ".conv_conv." in k and parts[1] in ("0", "4")


@pytest.mark.parametrize("name", C.NAMES)
def test_fp32_forward_backward_matches_reference(golden_dir, name):
    import fplx
    g = np.load(os.path.join(golden_dir, "nets3d_%s.npz" % name))
    x = torch.from_numpy(C.input_for(name)).cuda()
    y = torch.from_numpy(C.label_for(name)).cuda()
    s = int(g["logit_stride"])
    net, p = _net(name)
    net.eval()
    with torch.no_grad():
        le = _as_list(net(x))
    assert len(le) == C.n_outputs(name)
    for i, o in enumerate(le):
        assert o.shape == y.shape
        assert np.abs(o.cpu().numpy().reshape(-1)[::s] - g["logitsub%d_eval.%d" % (s, i)]).max() < LOGIT_TOL, i
    net, p = _net(name)                                # fresh: the running statistics update once
    net.train()
    lt = net(x, domain_label=torch.zeros(x.shape[0], dtype=torch.long))        # the agent's call; the label is ignored
    for i, o in enumerate(_as_list(lt)):
        assert np.abs(o.detach().cpu().numpy().reshape(-1)[::s] - g["logitsub%d_train.%d" % (s, i)]).max() < LOGIT_TOL, i
    base = fplx.DiceLoss()
    if isinstance(lt, list):
        lossf = fplx.DeepSuperviseLoss({"deep_supervise_weight": [1.0, 0.5, 0.25, 0.125], "base_loss": base})
    else:
        lossf = base
    loss = lossf({"prediction": lt, "ground_truth": y})
    assert abs(loss.item() - float(g["loss"])) < 1e-5
    loss.backward()
    sd = net.state_dict()
    named = dict(net.named_parameters())
    for k in g.files:
        if k.startswith("stat."):
            np.testing.assert_allclose(sd[k[5:]].cpu().numpy(), g[k], atol=2e-5, rtol=1e-4, err_msg=k)
        if k.startswith("gradsub"):
            head, kk = k.split(".", 1)
            ref, got = g[k], named[kk].grad.cpu().numpy().reshape(-1)[::int(head[len("gradsub"):])]
            if _is_bn_fed_bias(kk):
                # the reference returns fp32 cancellation noise, fplx returns 0
                assert np.abs(got).max() == 0.0 and np.abs(ref).max() < 1e-6, k
                continue
            tol = max(GRAD_TOL[name] * np.abs(ref).max(), 2e-7)
            np.testing.assert_allclose(got, ref, atol=tol, rtol=0, err_msg=k)
    keys = [str(k) for k in g["gradnorm_keys"]]
    assert sorted(k for k, t in named.items() if t.grad is not None) == keys     # exactly the reference's set
    for k, v in zip(keys, g["gradnorm_vals"]):
        if _is_bn_fed_bias(k):
            assert float(named[k].grad.abs().max()) == 0.0, k
            continue
        assert abs(float(named[k].grad.norm()) - v) <= max(GRAD_TOL[name] * v, 1e-6), (k, v)


SLOPE_CANCEL = 0.01      # tests/test_gpu_net_parity.py: bound on |error| / sum |terms| of a PReLU slope gradient


@pytest.mark.parametrize("name", ["u3dtri_ds", "u25"])
def test_bf16_matches_the_bf16_rounding_restatement(name):
    """bf16 activations, fp32 master weights: against tests/nets3d_ref.py rounding to bf16 at the stored tensors - every output
    within 2e-2 of its range, every gradient within max(0.1 |r|, 1.5 gap) in L2, gap = the restatement's own fp32-vs-bf16
    difference (tests/test_gpu_net_parity.py:234-304; a PReLU slope gradient also within SLOPE_CANCEL of its terms' sum).
    At this size 2e-2 of the range is close to what another order of fp32 additions alone moves the logits by;
    measured on an MI355X: u3dtri_ds 1.88 / 1.75 / 1.45 / 1.92 % for its four outputs, u25 1.01 %."""
    import fplx
    import nets3d_ref as R3
    from oracle import torch_ref as R
    x, y = torch.from_numpy(C.input_for(name)), torch.from_numpy(C.label_for(name))
    net, p = _net(name, "bf16")
    net.train()
    lt = net(x.cuda())
    base = fplx.DiceLoss()
    lossf = fplx.DeepSuperviseLoss({"base_loss": base}) if isinstance(lt, list) else base
    loss = lossf({"prediction": lt, "ground_truth": y.cuda()})
    loss.backward()
    # which stem kernel runs decides whether the fp32 input is rounded to bf16 on its way in (FPLX_KERNEL_STEM = 6: MFMA operands)
    from util import plan_kernel
    n_, cin_, D_, H_, W_ = x.shape
    rin = plan_kernel(n_, D_, H_, W_, cin_, p["feature_chns"][0], x_dt=0, y_dt=1) == 6
    sd, prm = R.split_state(C.weights_for(name))
    R.PRELU_TAPS = []
    try:
        ref = R3.forward(sd, p, x, True, act_dtype=torch.bfloat16, round_input=rin)
        rl = R3.loss_of(ref, y)
        rl.backward()
        slope_terms = {id(sl): float((ng.grad / float(sl.detach()) * ng.detach()).abs().sum())
                       for sl, ng in R.PRELU_TAPS if ng.grad is not None}
    finally:
        R.PRELU_TAPS = None
    sd32, prm32 = R.split_state(C.weights_for(name))
    ref32 = R3.forward(sd32, p, x, True)
    R3.loss_of(ref32, y).backward()
    figs = []
    for i, (o, r, r32) in enumerate(zip(_as_list(lt), _as_list(ref), _as_list(ref32))):
        rng = float(r.detach().abs().max())
        err = float(np.abs(o.detach().cpu().numpy() - r.detach().numpy()).max())
        lgap = float((r32.detach() - r.detach()).abs().max())
        print("%s output %d: max err %.4g = %.4f of range %.4g (restatement fp32-vs-bf16 gap %.4g), input rounded: %s" % (
            name, i, err, err / rng, rng, lgap, rin))
        figs.append((i, err, rng))
    print("%s loss %.6f vs %.6f" % (name, loss.item(), rl.item()))
    named = dict(net.named_parameters())
    bad = {}
    for k, t in prm.items():
        if t.grad is None:
            continue
        gq = named[k].grad.cpu().numpy().reshape(-1).astype(np.float64)
        if _is_bn_fed_bias(k):
            assert np.abs(gq).max() == 0.0
            continue
        r = t.grad.numpy().reshape(-1).astype(np.float64)
        r32 = prm32[k].grad.numpy().reshape(-1).astype(np.float64)
        e, nr, gap = float(np.linalg.norm(gq - r)), float(np.linalg.norm(r)), float(np.linalg.norm(r32 - r))
        tol = max(0.1 * nr, 1.5 * gap)
        if r.size == 1 and id(t) in slope_terms:
            tol = max(tol, SLOPE_CANCEL * slope_terms[id(t)])
        if e > tol:
            bad[k] = (e / max(nr, 1e-30), gap / max(nr, 1e-30))
    print("%s gradients outside max(0.1 |r|, 1.5 gap): %s" % (name, bad))
    for i, err, rng in figs:
        assert err < 2e-2 * rng, (i, err, rng)
    assert abs(loss.item() - rl.item()) < 1e-3
    assert not bad, bad


@pytest.mark.parametrize("name", C.NAMES)
def test_checkpoint_keys_and_adam_state_interop(name):
    """the fixture's weights load by reference key (strict); state_dict() carries exactly the reference's keys; after three
    FusedAdam steps optimizer.state_dict() loads into torch.optim.Adam over a same-shaped parameter list, and back"""
    import fplx
    net, p = _net(name)
    want = C.key_shapes(name)
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == want
    x = torch.from_numpy(C.input_for(name)).cuda()
    y = torch.from_numpy(C.label_for(name)).cuda()
    opt = fplx.get_optimizer("Adam", net, {"learning_rate": 1e-3, "weight_decay": 1e-5})
    lossf = fplx.DiceLoss()
    if C.n_outputs(name) > 1:
        lossf = fplx.DeepSuperviseLoss({"base_loss": lossf})
    net.train()
    start = net.flat_params.detach().clone()
    for _ in range(3):
        opt.zero_grad()
        lossf({"prediction": net(x), "ground_truth": y}).backward()
        opt.step()
    assert opt.seg_steps == [3] and float((net.flat_params.detach() - start).abs().max()) > 0
    sd = opt.state_dict()
    pnames = [k for k, _ in net.named_parameters()]
    assert sorted(sd["state"]) == list(range(len(pnames)))
    shapes = dict(want)
    prm = [torch.nn.Parameter(torch.zeros(shapes[k])) for k in pnames]
    ref = torch.optim.Adam(prm, 1e-3, weight_decay=1e-5)
    ref.load_state_dict(sd)
    st = ref.state[prm[0]]
    assert float(st["step"]) == 3.0 and float(st["exp_avg"].abs().max()) > 0
    o, n, shp = net._layout[pnames[0]]
    assert torch.equal(st["exp_avg"].cpu(), opt.exp_avg[o:o + n].view(shp).cpu())
    opt2 = fplx.FusedAdam(net, 0.5)
    opt2.load_state_dict(ref.state_dict())
    assert opt2.seg_steps == [3] and opt2.param_groups[0]["lr"] == 1e-3
    for k in pnames:
        o, n, _ = net._layout[k]
        assert torch.equal(opt2.exp_avg_sq[o:o + n], opt.exp_avg_sq[o:o + n]), k
    from fplx.checkpoint import reference_model_state_dict
    assert list(reference_model_state_dict(net)) == [k for k, _ in want]


@pytest.mark.parametrize("kind", ["Adam", "SGD", "Adadelta", "Adagrad", "Adamax", "ASGD", "RMSprop", "Rprop"])
def test_one_step_of_every_fused_optimiser_on_unet3d(kind):
    """get_optimizer(name, UNet3D) and one step on given gradients against torch.optim.<name> fed the same: Adam within 2e-6
    (tests/test_gpu_kernels.py), the seven others inside optimoracle's float64 bound (Rprop: equal to the fp32 evaluation)"""
    import fplx
    import optimoracle as O
    net, p = _net("u3d")
    net._ensure_flat()
    opt = fplx.get_optimizer(kind, net, {"learning_rate": 1e-2, "weight_decay": 1e-5, "momentum": 0.9})
    assert type(opt).__name__ == "Fused" + kind and opt.seg_ranges == [(0, net.flat_params.numel())]
    gen = torch.Generator().manual_seed(11)
    gflat = (torch.randn(net.flat_params.numel(), generator=gen) * 0.01).cuda()
    p0 = net.flat_params.detach().cpu().clone()
    names = [k for k, _ in net.named_parameters()]
    for k in names:
        o, n, shp = net._layout[k]
        net.get_param(k).grad = gflat[o:o + n].view(shp)
    opt.step()
    torch.cuda.synchronize()
    got = net.flat_params.detach().cpu().numpy()
    assert opt.seg_steps == [1]
    h = dict(lr=1e-2, weight_decay=1e-5) if kind == "Adam" else O.named_hp(kind, 1e-2, 1e-5, 0.9)
    prm = []
    for k in names:
        o, n, shp = net._layout[k]
        q = torch.nn.Parameter(p0[o:o + n].view(shp).clone())
        q.grad = gflat[o:o + n].view(shp).cpu().clone()
        prm.append(q)
    ref = getattr(torch.optim, kind)(prm, foreach=False, **h)
    ref.step()
    g = gflat.cpu().numpy()
    worst = {"torch": 0.0, "fused": 0.0}
    for k, q in zip(names, prm):
        o, n, _ = net._layout[k]
        sl = slice(o, o + n)
        tq = q.detach().numpy().reshape(-1)
        if kind == "Adam":
            assert float(np.abs(got[sl] - tq).max()) < 2e-6, k
            continue
        hp = O.abi_hp(kind, h, 1)
        zeros = [np.zeros(n, np.float32) for _ in range(2)]
        if kind == "Rprop":
            r = O.optim_f32(kind, p0.numpy()[sl], g[sl], zeros[0], zeros[1], hp, 1)
            assert np.array_equal(tq, r[0]) and np.array_equal(got[sl], r[0]), k
            continue
        r = O.optim_ref(kind, p0.numpy()[sl], g[sl], zeros[0], zeros[1], hp, 1)
        worst["torch"] = max(worst["torch"], O.ratio(tq, r[0], r[3]))
        worst["fused"] = max(worst["fused"], O.ratio(got[sl], r[0], r[3]))
    assert all(v <= 1.0 for v in worst.values()), worst
    assert float(np.abs(got - p0.numpy()).max()) > 0


def _agent(tmp_path, stage="train", **net_over):
    import fplx
    net = dict(C.NETS["u3d4_ds"], net_type="UNet3D", num_domains=1, deep_supervise=True,
               deep_supervise_weight=[1.0, 0.5, 0.25, 0.125], **net_over)
    cfg = {"dataset": {"tensor_type": "float", "root_dir": str(tmp_path), "test_csv": "config/test.csv"},
           "network": net,
           "training": {"gpus": [0], "loss_type": "DiceLoss", "optimizer": "Adam", "learning_rate": 1e-3, "weight_decay": 1e-5,
                        "momentum": 0.9, "lr_scheduler": None, "iter_valid": 2, "ckpt_save_dir": str(tmp_path / "model" / "ds")},
           "testing": {"gpus": [0], "domian_label": 0, "evaluation_mode": True, "output_dir": str(tmp_path / "out")}}
    torch.manual_seed(5)
    agent = fplx.SegmentationAgent(cfg, stage)
    agent.create_network()
    return agent


def test_agent_trains_and_infers_with_a_four_output_network(tmp_path):
    import fplx
    from fplx import nifti
    name = "u3d4_ds"
    x, y = torch.from_numpy(C.input_for(name)), torch.from_numpy(C.label_for(name))
    for dual in (False, True):
        agent = _agent(tmp_path)
        assert type(agent.net) is fplx.UNet3D and agent.net.deep_sup
        agent.create_optimizer()
        agent.create_loss_calculator(0.0 if dual else 1.0)
        lc = agent.loss_calculator
        assert type(lc) is fplx.DeepSuperviseLoss and lc.deep_sup_weight is None     # the weights of the config are not read
        assert agent._engine_step() is None                                          # the autograd route
        agent.set_loaders([{"image": x, "label_prob": y}])
        before = agent.net.state_dict()["out_conv3.weight"].clone()
        res = agent.training_all() if dual else agent.training()
        assert lc.deep_sup_weight == [1.0, 1.0, 1.0, 1.0]
        assert np.isfinite(res["loss"]) and np.isfinite(res["avg_dice"]) and res["class_dice"].shape == (3,)
        assert not torch.equal(before, agent.net.state_dict()["out_conv3.weight"])   # the deep heads train
        agent.valid_loader_1 = [{"image": x, "label_prob": y}]
        v = agent.validation()
        assert np.isfinite(v["loss"]) and v["class_dice"].shape == (3,)
    # inference: the mask comes from output 0 and is written with the input's geometry
    nifti.write_nifti(str(tmp_path / "case0.nii.gz"), x[0, 0].numpy(), (1.0, 1.0, 1.0))
    agent.stage = "test"
    agent.set_loaders(test_loader=[{"image": x[:1], "names": ["case0.nii.gz"]}])
    agent.inferer = None
    out = agent.infer()
    agent.net.eval()
    with torch.no_grad():
        direct = agent.net(x[:1].cuda())
    assert isinstance(direct, list) and len(direct) == 4
    assert torch.equal(out["case0.nii.gz"].cpu(), direct[0].argmax(1)[0].to(torch.uint8).cpu())
    assert os.path.exists(os.path.join(agent.output_dir, "case0.nii.gz"))


def test_class_dice_is_taken_from_output_zero():
    import fplx
    name = "u3d4_ds"
    net, p = _net(name)
    net.eval()
    x, y = torch.from_numpy(C.input_for(name)).cuda(), torch.from_numpy(C.label_for(name)).cuda()
    with torch.no_grad():
        outs = net(x)
        ds = fplx.DeepSuperviseLoss({"base_loss": fplx.DiceLoss()})
        total = ds({"prediction": outs, "ground_truth": y})
        dice0 = ds.last_out.clone()
        single = fplx.DiceLoss()
        vals = [single({"prediction": o, "ground_truth": y}) for o in outs]
        first = fplx.DiceLoss()
        first({"prediction": outs[0], "ground_truth": y})
    assert torch.equal(dice0, first.last_out)
    assert abs(float(total) - float(sum(vals)) / 4) < 1e-6
    assert not torch.equal(outs[0], outs[3])


def test_dropout_stream_is_keyed_by_seed_and_step():
    net, p = _net("u3d", dropout=[0, 0, 0.3, 0.4, 0.5])
    x = torch.from_numpy(C.input_for("u3d")).cuda()
    net.train()
    net.dropout_seed = 9
    with torch.no_grad():
        net._fwd_counter = 4
        a = net(x).clone()
        net._fwd_counter = 4
        b = net(x).clone()
        c = net(x)                     # step 5
    assert torch.equal(a, b)
    assert float((a - c).abs().max()) > 1e-3


def test_existing_registry_entry_and_engine_route_are_unchanged(tmp_path):
    import fplx
    from fplx.net import UNet2D5_dsbn
    from fplx.engine import Engine
    assert fplx.SegNetDict["UNet2D5_dsbn"] is UNet2D5_dsbn is fplx.UNet2D5_dsbn
    cfg_net = dict(in_chns=1, feature_chns=[4, 4, 8, 8, 8], dropout=[0] * 5, conv_dims=[3] * 5, class_num=2, bilinear=False,
                   num_domains=2, net_type="UNet2D5_dsbn")
    cfg = {"dataset": {"tensor_type": "float"}, "network": cfg_net,
           "training": {"gpus": [0], "loss_type": "DiceLoss", "optimizer": "Adam", "learning_rate": 1e-3, "weight_decay": 1e-5,
                        "lr_scheduler": None, "iter_valid": 1}, "testing": {"gpus": [0]}}
    agent = fplx.SegmentationAgent(cfg, "train")
    agent.create_network()
    agent.create_optimizer()
    agent.create_loss_calculator()
    assert type(agent.net) is UNet2D5_dsbn and type(agent.net.engine) is Engine
    assert type(agent.loss_calculator) is fplx.DiceLoss
    assert agent._engine_step() is not None


def test_bad_spatial_sizes_are_refused_before_any_launch():
    net, p = _net("u3d4_ds")
    with pytest.raises(ValueError):
        net(torch.zeros(1, 1, 16, 16, 20).cuda())            # 20 % 8 != 0
    with pytest.raises(ValueError):
        net(torch.zeros(1, 2, 16, 16, 16).cuda())            # channels
    with pytest.raises(ValueError):
        net(torch.zeros(1, 16, 16, 16).cuda())               # 4-D
    net5, _ = _net("u25")
    with pytest.raises(ValueError):
        net5(torch.zeros(1, 1, 8, 32, 40).cuda())            # 40 % 16 != 0 (the depth 8 is fine: two of the levels are 2D)
