"""UNet2D5 / UNet3D / DeepSuperviseLoss without a GPU: registry, constructors, state_dict keys against the key list dumped from
the reference, the loss wrapper's host logic, the torch restatement tests/nets3d_ref.py against the fixtures produced by running
the reference (tests/golden/make_golden_nets3d.py), and the premise of the exact GPU oracles (tests/headoracle.py)."""
import os

import numpy as np
import pytest
import torch

import nets3d_cfg as C
import nets3d_ref as R3
import headoracle as O
from oracle import torch_ref as R
from test_gpu_nets3d import GRAD_TOL


def _build(name, **over):
    import fplx
    p = dict(C.NETS[name], **over)
    return fplx.SegNetDict[p["net_type"]](p), p


def test_registry_holds_the_two_networks_and_keeps_the_old_ones():
    import fplx
    from fplx.net import UNet2D5_dsbn
    assert set(fplx.SegNetDict) == {"UNet2D5_dsbn", "UNet3D_dsbn", "UNet2D5", "UNet3D"}
    assert fplx.SegNetDict["UNet2D5_dsbn"] is UNet2D5_dsbn and fplx.SegNetDict["UNet3D_dsbn"] is UNet2D5_dsbn
    assert fplx.SegNetDict["UNet2D5"] is fplx.UNet2D5 and fplx.SegNetDict["UNet3D"] is fplx.UNet3D
    assert "DeepSuperviseLoss" not in fplx.SegLossDictAll and hasattr(fplx, "DeepSuperviseLoss")
    for n in ("UNet2D5", "UNet3D", "DeepSuperviseLoss"):
        assert n in fplx.__all__


def test_constructors_refuse_what_the_reference_refuses():
    import fplx
    with pytest.raises(AssertionError):                                   # unet2d5.py:180
        fplx.UNet2D5(dict(C.NETS["u25"], feature_chns=[8, 16, 32, 64], dropout=[0] * 4, conv_dims=[2, 2, 3, 3]))
    for ft in ([8, 16, 32], [8, 16, 32, 64, 128, 256]):                   # unet3d.py:114
        with pytest.raises(AssertionError):
            fplx.UNet3D(dict(C.NETS["u3d"], feature_chns=ft, dropout=[0] * len(ft)))
    with pytest.raises(ValueError):
        fplx.UNet2D5(dict(C.NETS["u25"], conv_dims=[2, 2, 3, 3, 4]))
    with pytest.raises(ValueError):
        fplx.UNet3D(dict(C.NETS["u3d"], precision="fp16"))
    with pytest.raises(ValueError):                                       # the 1x1x1 head kernels: C % 8 == 0, <= 8 classes
        fplx.UNet3D(dict(C.NETS["u3d"], feature_chns=[2, 8, 32, 64], dropout=[0] * 4))
    with pytest.raises(ValueError):
        fplx.UNet3D(dict(C.NETS["u3d"], class_num=9))
    net = fplx.UNet3D(dict(C.NETS["u3d"]))
    with pytest.raises(RuntimeError):                                     # no CPU path
        net(torch.zeros(1, 1, 16, 16, 16))


@pytest.mark.parametrize("name", C.NAMES)
def test_state_dict_keys_and_shapes_are_the_references(name):
    net, _ = _build(name)
    ours = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    assert ours == C.key_shapes(name)                                      # same keys, same order, same shapes
    from fplx.checkpoint import param_names_of
    buffers = ("running_mean", "running_var", "num_batches_tracked")
    assert param_names_of(net) == [k for k, _ in C.key_shapes(name) if k.rsplit(".", 1)[1] not in buffers]
    net.load_state_dict({k: torch.from_numpy(v) for k, v in C.weights_for(name).items()}, strict=True)


def test_deep_supervise_loss_host_logic():
    import fplx
    base = fplx.DiceLoss()
    ds = fplx.DeepSuperviseLoss({"deep_supervise_weight": [1.0, 0.5, 0.25, 0.125], "base_loss": base})
    assert ds.deep_sup_weight is None                                     # the key the agent passes is not the key read
    with pytest.raises(ValueError):
        ds({"prediction": torch.zeros(1, 2, 2, 2, 2), "ground_truth": torch.zeros(1, 2, 2, 2, 2)})
    ds2 = fplx.DeepSuperviseLoss({"deep_suervise_weight": [1.0, 0.5], "base_loss": base})
    assert ds2.deep_sup_weight == [1.0, 0.5]
    with pytest.raises(AssertionError):                                   # deep_sup.py:33, before the base loss runs
        ds2({"prediction": [torch.zeros(1, 2, 2, 2, 2)] * 3, "ground_truth": torch.zeros(1, 2, 2, 2, 2)})
    with pytest.raises(KeyError):
        fplx.DeepSuperviseLoss({"deep_suervise_weight": None})
    assert R3.deep_supervise_loss([1.0, 3.0], lambda p: p, [1.0, 0.5]) == pytest.approx(2.5 / 1.5)


def measure(name, golden_dir):
    """the restatement against the reference's fixture -> (max logit error, loss error, {key: max-normalised gradient gap})"""
    g = np.load(os.path.join(golden_dir, "nets3d_%s.npz" % name))
    p = C.NETS[name]
    x, y = torch.from_numpy(C.input_for(name)), torch.from_numpy(C.label_for(name))
    s = int(g["logit_stride"])
    lerr = 0.0
    sd, _ = R.split_state(C.weights_for(name), requires_grad=False)
    with torch.no_grad():
        outs = R3.forward(sd, p, x, train=False)
    outs = outs if isinstance(outs, list) else [outs]
    assert len(outs) == C.n_outputs(name)
    for i, o in enumerate(outs):
        lerr = max(lerr, float(np.abs(o.numpy().reshape(-1)[::s] - g["logitsub%d_eval.%d" % (s, i)]).max()))
    sd, prm = R.split_state(C.weights_for(name))
    outs = R3.forward(sd, p, x, train=True)
    for i, o in enumerate(outs if isinstance(outs, list) else [outs]):
        lerr = max(lerr, float(np.abs(o.detach().numpy().reshape(-1)[::s] - g["logitsub%d_train.%d" % (s, i)]).max()))
    loss = R3.loss_of(outs, y)
    loss.backward()
    for k in g.files:
        if k.startswith("stat."):
            np.testing.assert_allclose(sd[k[5:]].numpy(), g[k], atol=2e-6, rtol=1e-5, err_msg=k)
    assert sorted(k for k, t in prm.items() if t.grad is not None) == [str(k) for k in g["gradnorm_keys"]]
    gaps = {}
    for k in g.files:
        if k.startswith("gradsub"):
            head, kk = k.split(".", 1)
            ref, got = g[k], prm[kk].grad.numpy().reshape(-1)[::int(head[len("gradsub"):])]
            gaps[kk] = float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))
    return lerr, abs(float(loss.item()) - float(g["loss"])), gaps


@pytest.mark.parametrize("name", C.NAMES)
def test_restatement_matches_the_reference_fixtures(golden_dir, name):
    """logits within 1e-5; gradients: the restatement-vs-reference gap is the reference's own fp32 noise (two arrangements of
    the same ATen operators) - GRAD_TOL[name], the GPU test's tolerance, is twice it and not below 1e-3"""
    lerr, loss_err, gaps = measure(name, golden_dir)
    live = {k: v for k, v in gaps.items() if not (k.endswith("bias") and ".conv_conv." in k and k.rsplit(".", 2)[1] in "04")}
    worst = max(live.values())
    print("%s: logits %.3g, loss %.3g, worst gradient gap %.3g (%s)" % (name, lerr, loss_err, worst, max(live, key=live.get)))
    assert lerr < 1e-5
    assert loss_err < 1e-6
    assert 2.0 * worst <= GRAD_TOL[name] and GRAD_TOL[name] >= 1e-3


@pytest.mark.parametrize("case", O.HEAD_CASES, ids=O.head_id)
def test_head_oracle_data_is_exact_in_float32(case):
    d = O.head_data(case)
    r32, r64 = O.head_ref(d, torch.float32), O.head_ref(d, torch.float64)
    for k in r64:
        assert torch.equal(r32[k].double(), r64[k]), k
    assert float(r64["da_acc"].abs().max()) <= 256 and float(r64["da_acc"].abs().max()) > 0     # exact in bf16 too
    for k in ("a", "w", "dlogits", "da0"):
        t = torch.from_numpy(d[k])
        assert torch.equal(t.to(torch.bfloat16).double(), t)


@pytest.mark.parametrize("case", O.INTERP_CASES, ids=O.interp_id)
def test_interp_oracle_data_is_exact_in_float32(case):
    d = O.interp_data(case)
    r32, r64 = O.interp_ref(case, d, torch.float32), O.interp_ref(case, d, torch.float64)
    assert torch.equal(r32["y"].double(), r64["y"]) and torch.equal(r32["dx"].double(), r64["dx"])
    assert float(r64["dx"].abs().max()) > 0


@pytest.mark.parametrize("name", ["u25", "u3d"])
def test_agent_refuses_the_new_networks_under_a_process_group(name):
    import fplx
    cfg = {"dataset": {"tensor_type": "float"}, "network": dict(C.NETS[name], num_domains=1),
           "training": {"gpus": [0], "loss_type": "DiceLoss"}, "testing": {"gpus": [0]}}
    agent = fplx.SegmentationAgent(cfg, "train")
    agent.distributed = True                   # what ddp.init_from_env reports under torch.distributed.run
    with pytest.raises(ValueError, match="single process"):
        agent.create_network()
    agent.create_loss_calculator()
    assert type(agent.loss_calculator) is fplx.DiceLoss and agent.loss_calculator.dist_sync
    cfg["network"]["deep_supervise"] = True
    agent.create_loss_calculator()
    lc = agent.loss_calculator
    assert type(lc) is fplx.DeepSuperviseLoss and lc.dist_sync and lc.base_loss.dist_sync     # the full-batch loss is the base's
