"""CPU tests of the noisy-label layer: the fp32 quantile rank against torch.quantile bit for bit, the oracle (tests/nlloracle.py)
against numpy's stable argsort and against the fixture recorded from the reference (tests/golden/nll_steps.npz), BiNet / TriNet,
the optimiser group, the refusals, the C ABI's error codes before any launch and the package surface."""
import os

import numpy as np
import pytest
import torch

import fplx
from fplx import _lib
from fplx import nll as fnll
from fplx import ops

import nlloracle as NO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nll_steps.npz")
CASES = ["%s.%s.%s" % (m, s, g) for m in ("CoTeaching", "TriNet") for s in ("a", "b") for g in ("mid", "start")]


# ---------------------------------------------------------------- the fp32 rank and torch's lerp

@pytest.mark.parametrize("n", [1, 2, 1001, 70001, 4096001])
def test_quantile_rank_and_lerp_equal_torch_quantile_bit_for_bit(n):
    x = torch.rand(n, generator=torch.Generator().manual_seed(n)) * 3.0
    s = np.sort(x.numpy())
    for q in (0, 0.3, 0.72, 0.8123, 1):
        want = torch.quantile(x, q).numpy()
        k, w = ops.nll_quantile_rank(q, n)
        assert (k, np.float32(w)) == NO.quantile_rank(q, n)
        assert 0 <= k <= n - 1 and 0.0 <= w < 1.0
        got = NO.lerp32(s[k], s[k] if w == 0 else s[min(k + 1, n - 1)], w)
        assert got.tobytes() == want.astype(np.float32).tobytes(), (n, q, k, w, got, want)
        assert NO.quantile32(x.numpy(), q).tobytes() == want.astype(np.float32).tobytes()
    with pytest.raises(ValueError):
        ops.nll_quantile_rank(1.5, n)


def test_quantile_restatement_propagates_nan_and_keeps_nothing():
    x = NO.tie_case("cpu.nan", 257, "nan")
    assert np.isnan(torch.quantile(torch.from_numpy(x), 0.5).item()) and np.isnan(NO.quantile32(x, 0.5))
    assert not NO.below_mask(x, 0.5).any()


# ---------------------------------------------------------------- the stable-rank mask

@pytest.mark.parametrize("kind", ["equal", "two", "ties", "nan", "random"])
@pytest.mark.parametrize("n", [1, 5, 63, 257, 9240])
def test_rank_mask_is_the_head_of_a_stable_argsort(n, kind):
    x = NO.tie_case("cpu.rank.%s.%d" % (kind, n), n, kind)
    order = np.argsort(x, kind="stable")                   # numpy sorts NaN last, as the keys do
    less = int((NO.keys(x) < np.sort(NO.keys(x))[n // 2]).sum())
    for k in sorted({0, 1, less, min(less + 1, n), n - 1, n}):
        want = np.zeros(n, bool)
        want[order[:k]] = True
        got = NO.rank_mask(x, k)
        assert got.sum() == k and np.array_equal(got, want), (n, kind, k)


def test_keys_preserve_the_order_of_fp32_values():
    x = np.array([-np.inf, -3.5, -1e-40, 0.0, 1e-40, 2.0, np.inf, np.nan], np.float32)
    k = NO.keys(x).astype(np.int64)
    assert (np.diff(k) > 0).all() and k[-1] == 0xFFFFFFFF


# ---------------------------------------------------------------- the oracle against the reference's recorded steps

def _case(z, tag):
    method = tag.split(".")[0]
    k = 2 if method == "CoTeaching" else 3
    logits = [z[tag + ".logits%d" % (j + 1)] for j in range(k)]
    return method, logits, z[tag + ".label"], float(z[tag + ".ratio"])


def test_fixture_ratios_are_the_agents_ramps():
    z = np.load(GOLDEN)
    iter_max, sel = int(z["iter_max"]), float(z["select_ratio"])
    for tag in CASES:
        mode = "sigmoid" if tag.startswith("CoTeaching") else "linear"
        ramp = fplx.get_rampup_ratio(int(z[tag + ".glob_it"]), 0, iter_max, mode)
        assert float(z[tag + ".ratio"]) == 1 - (1 - sel) * ramp, tag
    assert float(z["TriNet.a.start.ratio"]) == 1.0          # q = 1: the voxels with the maximum loss are dropped


@pytest.mark.parametrize("tag", CASES)
def test_oracle_reproduces_the_reference_within_its_bound(tag):
    z = np.load(GOLDEN)
    method, logits, y, ratio = _case(z, tag)
    r = NO.node(logits, y, method, ratio)
    assert r.undecided == 0
    n = r.refs[0].L.size
    if method == "CoTeaching":
        assert all(int(m.sum()) == int(ratio * n) for m in r.masks)
    elif ratio == 1.0:
        assert all(int(m.sum()) == n - int((rf.L == rf.L.max()).sum()) for m, rf in zip(r.masks, r.refs))
    # loss1, loss2: fp32 means of the reference; (m + 1) u mean |L| + the per-voxel bounds (nlloracle, "the reference")
    for j in range(2):
        keep, m = r.keeps[j], int(r.out[j, 1])
        b = NO.GAMMA_SLACK * (float(r.refs[j].e_L[keep].sum()) / m + (m + 1) * NO.U * float(np.abs(r.refs[j].L[keep]).mean())) \
            + NO.U * abs(r.out[j, 2])
        assert abs(float(z[tag + ".loss%d" % (j + 1)]) - r.out[j, 2]) <= b, (tag, j)
        bn = NO.GAMMA_SLACK * (float(r.refs[j].e_L.sum()) / n + (n + 1) * NO.U * float(np.abs(r.refs[j].L).mean()))
        assert abs(float(z[tag + ".loss_no_select%d" % (j + 1)]) - r.out[j, 3] / n) <= bn, (tag, j)
    for j in range(len(logits)):
        assert NO.ratio(z[tag + ".dlogits%d" % (j + 1)], r.grads[j], r.grad_bounds[j]) <= 1.0, (tag, j)
        assert np.abs(r.grads[j]).max() > 1e3 * r.grad_bounds[j].max()          # the bound is a test, not a blanket


def test_fp32_restatement_of_the_cross_entropy_is_inside_its_bound():
    for c, v in ((2, 63), (3, 9240), (8, 5)):
        logits, y = NO.logits_case("cpu.ce.%d.%d" % (c, v), 1, 3, c, v)
        r = NO.voxel_ce(logits[0], y)
        got, _ = NO.ce_fp32(logits[0], y)
        assert NO.ratio(got, r.L, NO.GAMMA_SLACK * r.e_L) <= 1.0
        assert r.e_L.max() < 1e-4 * np.abs(r.L).max()


# ---------------------------------------------------------------- BiNet / TriNet, the optimiser group

class _Toy(torch.nn.Module):
    def __init__(self, params):
        super(_Toy, self).__init__()
        self.conv = torch.nn.Conv3d(1, params['class_num'], 1)
        self.dropout_seed = params['dropout_seed']

    def forward(self, x, domain_label=None):
        return self.conv(x)


def _net_params():
    import nets3d_cfg as C
    return dict(C.NETS["u3d4_ds"], deep_supervise=False, precision="fp32", net_type="UNet3D")


def test_group_state_dict_keys_are_the_references():
    p = _net_params()
    one = list(fplx.UNet3D(p).state_dict())
    for cls, count in ((fplx.BiNet, 2), (fplx.TriNet, 3)):
        net = cls(p)
        want = ["net%d.%s" % (i + 1, k) for i in range(count) for k in one]
        assert list(net.state_dict()) == want
        assert [m.dropout_seed for m in net.members()] == [p.get('dropout_seed', 1) + i for i in range(count)]
        from fplx import checkpoint
        sd = checkpoint.reference_model_state_dict(net)
        assert list(sd) == want and all(torch.equal(sd[k], v) for k, v in net.state_dict().items())


def test_group_eval_output_is_the_sum_over_three_for_binet_too():
    torch.manual_seed(3)
    x = torch.randn(2, 1, 2, 3, 4)
    params = {'net_type': 'Toy', 'class_num': 3, 'dropout_seed': 7}
    for cls, count in ((fplx.BiNet, 2), (fplx.TriNet, 3)):
        net = cls(params, {'Toy': _Toy})
        outs = net(x, domain_label=torch.zeros(2, dtype=torch.long))
        assert isinstance(outs, tuple) and len(outs) == count
        net.eval()
        acc = outs[0]
        for o in outs[1:]:
            acc = acc + o
        assert torch.equal(net(x), acc / 3)                  # (out1 + out2) / 3: the reference's literal
    with pytest.raises(ValueError, match="Undefined network"):
        fplx.BiNet({'net_type': 'Nope'}, {'Toy': _Toy})


@pytest.mark.parametrize("name", ["SGD", "Adam", "Adadelta", "Adagrad", "Adamax", "ASGD", "RMSprop", "Rprop"])
def test_optimiser_group_round_trips_its_state(name):
    p = _net_params()
    tr = {"learning_rate": 0.02, "momentum": 0.9, "weight_decay": 1e-4}

    def group():
        net = fplx.BiNet(p)
        return net, fplx.GroupOptimizer([fplx.get_optimizer(name, m, tr) for m in net.members()])

    net, opt = group()
    assert isinstance(opt, torch.optim.Optimizer) and len(opt.param_groups) == 1 and opt.param_groups[0]['lr'] == 0.02
    assert len(opt.param_groups[0]['params']) == len(list(net.parameters()))
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, [1], 0.5)
    g = torch.Generator().manual_seed(5)
    for i, m in enumerate(opt.members):
        for st in m._active_state():
            m._buffer(st).copy_(torch.rand(m._buffer(st).shape, generator=g) + 0.1)
        m.seg_steps = [3 + i]
        if name == "ASGD":                                  # host scalars a first step would have set
            m.seg_eta, m.seg_mu = [0.015625], [1.0]
    opt._opt_called = True
    sched.step()
    assert opt.param_groups[0]['lr'] == 0.01
    sd = opt.state_dict()
    assert sorted(sd) == ["members", "param_groups"] and len(sd["members"]) == 2 and sd["param_groups"][0]["lr"] == 0.01
    _, opt2 = group()
    opt2.load_state_dict(sd)
    assert opt2.param_groups[0]['lr'] == 0.01
    for a, b in zip(opt.members, opt2.members):
        assert a.seg_steps == b.seg_steps or not a.HAS_STEP        # torch's SGD keeps no step count
        sa, sb = a.state_dict()["state"], b.state_dict()["state"]      # per parameter: the flat buffers' padding is not state
        assert len(sa) == len(sb) > 0
        for i in sa:
            assert sorted(sa[i]) == sorted(sb[i])
            for st in sa[i]:
                assert torch.equal(torch.as_tensor(sa[i][st]), torch.as_tensor(sb[i][st])), (i, st)
    for p1, p2 in zip(net.parameters(), opt.param_groups[0]['params']):
        assert p1 is p2
    opt.zero_grad()
    with pytest.raises(ValueError, match="members"):
        opt2.load_state_dict({"members": sd["members"][:1], "param_groups": sd["param_groups"]})


# ---------------------------------------------------------------- registry and refusals

def _cfg(method="CoTeaching", net_type="UNet3D", loss_type="CrossEntropyLoss"):
    return {"dataset": {"tensor_type": "float"},
            "network": {"net_type": net_type, "class_num": 2},
            "training": {"gpus": [0], "loss_type": loss_type, "iter_max": 10, "iter_valid": 2},
            "noisy_label_learning": {"nll_method": method, "co_teaching_select_ratio": 0.6, "trinet_select_ratio": 0.6}}


def test_method_dict_and_refusals(monkeypatch, caplog):
    assert sorted(fplx.NLLMethodDict) == ["CoTeaching", "TriNet"]
    assert fplx.nll_agent_class("CoTeaching") is fplx.NLLCoTeaching and fplx.nll_agent_class("TriNet") is fplx.NLLTriNet
    for cls in fplx.NLLMethodDict.values():
        assert issubclass(cls, fplx.NLLSegAgent) and issubclass(cls, fplx.SegmentationAgent)
    with pytest.raises(ValueError, match="DAST needs a two-branch network"):
        fplx.nll_agent_class("DAST")
    with pytest.raises(ValueError, match="Undefined noisy-label method"):
        fplx.nll_agent_class("NoSuchMethod")
    for name in ("UNet2D5_dsbn", "UNet3D_dsbn"):
        for cls in fplx.NLLMethodDict.values():
            with pytest.raises(ValueError, match="domain-specific-BatchNorm"):
                cls(_cfg(net_type=name))
        with pytest.raises(ValueError, match="domain-specific-BatchNorm"):
            fplx.BiNet({"net_type": name})
    ag = fplx.NLLTriNet(_cfg("TriNet"))
    assert ag.config["network"]["num_domains"] == 1 and ag.mode == "TriNet" and ag.ramp_mode == "linear"
    ag.glob_it = 5
    assert ag._remb_ratio() == 1 - (1 - 0.6) * fplx.get_rampup_ratio(5, 0, 10, "linear")
    import logging
    with caplog.at_level(logging.WARNING):
        co = fplx.NLLCoTeaching(_cfg(loss_type="DiceLoss"))
    assert "only CrossEntropyLoss supported for coteaching" in caplog.text
    co.glob_it = 5
    assert co._remb_ratio() == 1 - (1 - 0.6) * fplx.get_rampup_ratio(5, 0, 10, "sigmoid")
    monkeypatch.setattr(fplx.ddp, "init_from_env", lambda device=None: True)
    for cls in fplx.NLLMethodDict.values():
        with pytest.raises(ValueError, match="single process"):
            cls(_cfg())


def test_loss_calculator_ignores_the_entropy_weight():
    ag = fplx.NLLCoTeaching.__new__(fplx.NLLCoTeaching)
    ag.loss_dict, ag.distributed = None, False
    ag.config = {"training": {"loss_type": "CrossEntropyLoss"}, "network": {}}
    ag.create_loss_calculator(1.0)
    assert type(ag.loss_calculator) is fplx.CrossEntropyLoss and ag.loss_calculator.terms[3] == 0.0


def test_selective_ce_loss_refusals():
    t = torch.zeros(1, 2, 4)
    with pytest.raises(ValueError, match="mode"):
        fplx.selective_ce_loss([t, t], t, "DAST", 0.5)
    with pytest.raises(RuntimeError):                     # GPU only, no CPU fallback
        fplx.selective_ce_loss([t, t], t, "CoTeaching", 0.5)
    assert ops.NLL_USES == NO.USES


# ---------------------------------------------------------------- the C ABI's refusals (before any launch)

E_BADSHAPE, E_WORKSPACE, E_NULL = -1, -3, -5
_buf = np.zeros(64, np.float32)
P = _buf.ctypes.data          # a non-null pointer for the calls that are refused before they read it


def _rc(name, *args):
    rc = getattr(_lib.lib(), name)(*args)
    return rc, _lib.last_error()


def _pp(*ptrs):
    import ctypes
    return (ctypes.c_void_p * 3)(*ptrs)


def test_abi_refusals():
    import ctypes
    uses = (ctypes.c_int * 3)(2, 1, 0)
    three = _pp(P, P, P)
    hole = _pp(P, None, P)
    for k, n, c, v in ((0, 1, 2, 8), (4, 1, 2, 8), (2, 0, 2, 8), (2, 1, 1, 8), (2, 1, 9, 8), (2, 1, 2, 0), (2, 4, 2, 1 << 29)):
        rc, msg = _rc("fplx_nll_voxel_ce_fwd", three, k, P, n, c, v, three, P, None)
        assert rc == E_BADSHAPE and "nll_voxel_ce_fwd" in msg, (k, n, c, v)
        rc, msg = _rc("fplx_nll_select_bwd", three, P, three, uses, k, P, P, 1.0, n, c, v, three, None)
        assert rc == E_BADSHAPE and "nll_select_bwd" in msg, (k, n, c, v)
    for args in ((None, 2, P, 1, 2, 8, three, P), (three, 2, None, 1, 2, 8, three, P), (three, 2, P, 1, 2, 8, None, P),
                 (three, 2, P, 1, 2, 8, three, None), (hole, 2, P, 1, 2, 8, three, P), (three, 2, P, 1, 2, 8, hole, P)):
        assert _rc("fplx_nll_voxel_ce_fwd", *(args + (None,)))[0] == E_NULL
    ws_m, ws_s = _lib.lib().fplx_nll_mask_ws_bytes(), _lib.lib().fplx_nll_select_ws_bytes()
    assert ws_m >= 4 * (3 * 1024 + 1) and ws_s >= 4 * (4 + 6 * 1024)
    mask = lambda *a: _rc("fplx_nll_select_mask", *(a + (None,)))
    assert mask(None, 8, 0, 4, 0.0, P, None, P, P, ws_m)[0] == E_NULL
    assert mask(P, 8, 0, 4, 0.0, P, None, None, P, ws_m)[0] == E_NULL
    assert mask(P, 8, 0, 4, 0.0, None, None, P, P, ws_m)[0] == E_NULL
    assert mask(P, 8, 0, 4, 0.0, P, None, P, None, ws_m)[0] == E_NULL
    assert mask(P, 8, 1, 0, 0.5, None, None, P, None, 0)[0] == E_NULL
    assert mask(P, 8, 0, 4, 0.0, P, None, P, P, ws_m - 1)[0] == E_WORKSPACE
    for n, mode, k, w in ((0, 0, 0, 0.0), (1 << 31, 0, 1, 0.0), (8, 2, 1, 0.0), (8, 0, 9, 0.0), (8, 0, -1, 0.0), (8, 1, 0, 1.0), (8, 1, 0, -0.5)):
        rc, msg = mask(P, n, mode, k, w, P, None, P, P, ws_m)
        assert rc == E_BADSHAPE and "nll_select_mask" in msg, (n, mode, k, w)
    fwd = lambda *a: _rc("fplx_nll_select_fwd", *(a + (None,)))
    assert fwd(three, three, uses, 2, 8, P, 1, P, P, ws_s - 1)[0] == E_WORKSPACE
    for args in ((None, three, uses, 2, 8, P, 1, P, P, ws_s), (three, None, uses, 2, 8, P, 1, P, P, ws_s), (three, three, None, 2, 8, P, 1, P, P, ws_s),
                 (three, three, uses, 2, 8, None, 1, P, P, ws_s), (three, three, uses, 2, 8, P, 1, None, P, ws_s),
                 (three, three, uses, 2, 8, P, 1, P, None, ws_s), (hole, three, uses, 2, 8, P, 1, P, P, ws_s)):
        assert fwd(*args)[0] == E_NULL, args
    bad_uses = (ctypes.c_int * 3)(4, 1, 0)                 # mask 2 of two
    for args in ((three, three, uses, 0, 8, P, 1, P, P, ws_s), (three, three, uses, 2, 0, P, 1, P, P, ws_s),
                 (three, three, uses, 2, 8, P, 0, P, P, ws_s), (three, three, bad_uses, 2, 8, P, 1, P, P, ws_s)):
        rc, msg = fwd(*args)
        assert rc == E_BADSHAPE and "nll_select_fwd" in msg, args
    for args in ((None, P, three, uses, 2, P, P, 1.0, 1, 2, 8, three), (three, None, three, uses, 2, P, P, 1.0, 1, 2, 8, three),
                 (three, P, None, uses, 2, P, P, 1.0, 1, 2, 8, three), (three, P, three, None, 2, P, P, 1.0, 1, 2, 8, three),
                 (three, P, three, uses, 2, None, P, 1.0, 1, 2, 8, three), (three, P, three, uses, 2, P, None, 1.0, 1, 2, 8, three),
                 (three, P, three, uses, 2, P, P, 1.0, 1, 2, 8, None), (three, P, three, uses, 2, P, P, 1.0, 1, 2, 8, hole)):
        assert _rc("fplx_nll_select_bwd", *(args + (None,)))[0] == E_NULL, args
    with pytest.raises(ValueError):                      # the wrapper raises what the library refuses
        _lib.call("fplx_nll_select_mask", P, 0, 0, 0, 0.0, P, None, P, P, ws_m, None)


def test_package_surface_and_exports():
    for n in ("nll", "NLLSegAgent", "NLLCoTeaching", "NLLTriNet", "NLLMethodDict", "nll_agent_class", "BiNet", "TriNet",
              "GroupOptimizer", "selective_ce_loss"):
        assert n in fplx.__all__ and hasattr(fplx, n), n
    for n in ("nll_voxel_ce_fwd", "nll_select_mask", "nll_select_fwd", "nll_select_bwd", "nll_quantile_rank"):
        assert callable(getattr(fplx.ops, n)), n
    declared = set(_lib.declared_symbols())
    new = {"fplx_nll_voxel_ce_fwd", "fplx_nll_select_mask", "fplx_nll_select_fwd", "fplx_nll_select_bwd", "fplx_nll_mask_ws_bytes",
           "fplx_nll_select_ws_bytes", "fplx_nll_ce_rows"}
    assert new <= declared
    import subprocess
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split() and l.split()[-1].startswith("fplx_")}
    assert exported == declared
    from fplx import nll_main
    assert nll_main.main(["nll_main"]) == 1
    assert fnll.NLLMethodDict is fplx.NLLMethodDict
