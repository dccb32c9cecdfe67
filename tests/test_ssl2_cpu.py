"""Host side of the CPS / URPC feature without a GPU: the oracle of tests/pyramidoracle.py checked against itself (the float64
closed forms equal float64 autograd of the reference's statements inside every reference call, the fp32 restatement passes,
every mutation trips a bound), the fixture tests/golden/ssl2_steps.npz (the reference's own training loops), the refusals of the
three C entry points, the second method registry, the agents' refusals and the package surface."""
import ctypes
import os

import numpy as np
import pytest
import torch

import fplx
from fplx import _lib
from fplx import ssl as fssl

import pyramidoracle as PO

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ssl2_steps.npz")

# ---------------------------------------------------------------- the oracle against itself

CASES = [(2, 1, 2, 63), (3, 3, 3, 9240), (4, 1, 8, 9240), (4, 3, 3, 5), (2, 1, 3, 1)]


def _z(k, n, c, v):
    return PO.logits_case("cpu.%d.%d.%d.%d" % (k, n, c, v), k, n, c, v)


@pytest.mark.parametrize("k,n,c,v", CASES)
def test_fp32_restatement_is_inside_the_bounds(k, n, c, v):
    z = _z(k, n, c, v)
    r = PO.pyramid_ref(z, 0.7)                       # asserts closed form == float64 autograd, value and gradient
    out = PO.pyramid_fwd(z, F32)
    res = PO.check_pyramid_fwd(r, out, "restatement")
    assert max(res["B1"], res["A1"]) > 0 or v < 64   # the fp32 evaluation does differ: the bound is not vacuous
    dz, bound = PO.pyramid_grad_ref(z, out, 0.7)
    assert PO.ratio(PO.pyramid_bwd(z, out, 0.7, F32), dz, bound) <= 1.0
    assert float(r.out[4 * k]) > 1e-3                # the scales do disagree: the regulariser is not trivially 0


def test_the_mean_carries_gradient_and_the_scales_sum_to_the_loss():
    z = _z(3, 1, 3, 63)
    r = PO.pyramid_ref(z)
    assert abs(r.out[3:12:4].sum() / 3 - r.out[12]) <= 1e-15
    full = PO.pyramid_bwd(z, r.out, 1.0)
    cut = PO.pyramid_bwd(z, r.out, 1.0, mut="mean_detached")
    assert np.abs(full - cut).max() > 0.1 * np.abs(full).max()


def test_exact_case_gives_zero_and_m_in_the_fp32_restatement():
    for k in (2, 4):
        for (n, c, v) in [(1, 2, 63), (3, 8, 9240), (1, 3, 5)]:
            z1 = PO.exact_case("exact.cpu", n, c, v)
            out = PO.pyramid_fwd(np.stack([z1] * k), F32)
            M = float(n * v)
            for i in range(k):
                assert out[4 * i] == 0.0 and out[4 * i + 1] == M and out[4 * i + 2] == 0.0 and out[4 * i + 3] == 0.0
            assert out[4 * k] == 0.0


def _trips(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("mut", PO.MUTATIONS)
def test_every_mutation_trips_its_bound(mut):
    k, n, c, v = 4, 3, 3, 9240
    z = _z(k, n, c, v)
    r = PO.pyramid_ref(z)
    good = PO.pyramid_fwd(z, F32)
    PO.check_pyramid_fwd(r, good, "good")
    dz, bound = PO.pyramid_grad_ref(z, good, 1.3)
    assert PO.ratio(PO.pyramid_bwd(z, good, 1.3, F32), dz, bound) <= 1.0
    value_trips = _trips(lambda: PO.check_pyramid_fwd(r, PO.pyramid_fwd(z, F32, mut), mut))
    grad_ratio = PO.ratio(PO.pyramid_bwd(z, good, 1.3, F32, mut), dz, bound)
    if mut == "mean_detached":                       # the value does not see it; the gradient does
        assert not value_trips and grad_ratio > 1.0
    elif mut == "no_eps":                            # 1e-8 next to B / M ~ 1 is below the fp32 sums' bound: the double re-evaluation sees it
        assert value_trips
    else:
        assert value_trips and grad_ratio > 1.0


# ---------------------------------------------------------------- the fixture: the reference's own loops

def _golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("tag", ["URPC.a.mid", "URPC.a.end", "URPC.b.mid", "URPC.b.end"])
def test_oracle_reproduces_the_references_urpc_iteration(tag):
    g = _golden()
    n0 = int(g[tag + ".n0"])
    full = np.stack([g[tag + ".logits%d" % (j + 1)] for j in range(4)])
    k, n = full.shape[:2]
    c = full.shape[2]
    z = np.ascontiguousarray(full[:, n0:].reshape(k, n - n0, c, -1))
    w = float(g[tag + ".regular_w"])
    assert w == float(g["regularize_w"]) * fplx.get_rampup_ratio(int(g[tag + ".glob_it"]), 0, int(g["iter_max"]), "sigmoid")
    r = PO.pyramid_ref(z, w)
    loss_reg = float(g[tag + ".loss_reg"])
    assert abs(loss_reg - r.out[4 * k]) <= r.bound[4 * k] + PO.U * abs(loss_reg)        # torch's fp32 evaluation: inside the bound
    assert abs(float(g[tag + ".loss"]) - (float(g[tag + ".loss_sup"]) + w * loss_reg)) <= 4 * PO.U * abs(float(g[tag + ".loss"]))
    # rows >= n0 take gradient from the regulariser alone: regular_w d loss_reg / d logits
    dz, bound = PO.pyramid_grad_ref(z, r.out, w)
    for j in range(k):
        got = g[tag + ".dlogits%d" % (j + 1)][n0:].reshape(n - n0, c, -1)
        assert PO.ratio(got, dz[j], bound[j]) <= 1.0, j
        assert np.abs(got).max() > 0


@pytest.mark.parametrize("tag", ["CPS.a.mid", "CPS.a.end", "CPS.b.mid", "CPS.b.end"])
def test_oracle_reproduces_the_references_cps_iteration(tag):
    from oracle import torch_ref as R
    g = _golden()
    n0 = int(g[tag + ".n0"])
    z = [torch.from_numpy(g[tag + ".logits%d" % (j + 1)].astype(np.float64)) for j in range(2)]
    y0 = torch.from_numpy(g[tag + ".label"].astype(np.float64))
    c = z[0].shape[1]
    pse = [torch.from_numpy(PO.pseudo_onehot(t[n0:].numpy().reshape(t.shape[0] - n0, c, -1)).astype(np.float64)).reshape(t[n0:].shape)
           for t in z]
    sup = [float(R.dice_loss(z[j][:n0], y0)) for j in range(2)]
    cross = [float(R.dice_loss(z[0][n0:], pse[1])), float(R.dice_loss(z[1][n0:], pse[0]))]
    w = float(g[tag + ".regular_w"])
    for name, ref in (("loss_sup1", sup[0]), ("loss_sup2", sup[1]), ("loss_pse_sup1", cross[0]), ("loss_pse_sup2", cross[1]),
                      ("loss", sup[0] + w * cross[0] + sup[1] + w * cross[1])):
        assert abs(float(g[tag + "." + name]) - ref) <= 2e-6, (name, float(g[tag + "." + name]), ref)


def test_pseudo_onehot_takes_the_first_maximum():
    z = PO.onehot_case("cpu.onehot", 2, 2, 3, 65)
    assert PO.grid_is_separated(z)
    oh = PO.pseudo_onehot(z)
    assert oh.dtype == np.float32 and oh.shape == z.shape and np.array_equal(oh.sum(2), np.ones((2, 2, 65), np.float32))
    ties = (z == z.max(2, keepdims=True)).sum(2) > 1
    assert ties.any() and (~ties).any()
    first = np.argmax(z == z.max(2, keepdims=True), axis=2)
    assert np.array_equal(oh.argmax(2), first)
    # on this grid torch's softmax keeps every order and every tie: the reference's pseudo label is the same array
    soft = torch.softmax(torch.from_numpy(z), dim=2)
    idx = torch.argmax(soft, dim=2, keepdim=True)
    ref = torch.zeros_like(soft).scatter_(2, idx, 1.0).numpy()
    assert np.array_equal(ref, oh)


# ---------------------------------------------------------------- the C ABI's refusals (before any launch)

E_BADSHAPE, E_NULL = -1, -5
_buf = np.zeros(64, np.float32)
P = _buf.ctypes.data          # a non-null pointer for the calls that are refused before they read it


def _table(n_valid, n_total=4):
    """a host table of n_total pointers, the first n_valid non-null"""
    return (ctypes.c_void_p * n_total)(*([P] * n_valid + [None] * (n_total - n_valid)))


def _rc(name, *args):
    rc = getattr(_lib.lib(), name)(*args)
    return rc, _lib.last_error()


def test_pyramid_refusals():
    fwd = lambda tab, k, n, c, v, part, out: _rc("fplx_ssl_pyramid_fwd", tab, k, n, c, v, part, out, None)
    bwd = lambda tab, out, gs, k, n, c, v, dtab: _rc("fplx_ssl_pyramid_bwd", tab, out, gs, k, n, c, v, dtab, None)
    T = _table(4)
    for k in (1, 5, 0, -2):
        rc, msg = fwd(T, k, 1, 2, 8, P, P)
        assert rc == E_BADSHAPE and "ssl_pyramid_fwd" in msg, (k, rc, msg)
        rc, msg = bwd(T, P, P, k, 1, 2, 8, T)
        assert rc == E_BADSHAPE and "ssl_pyramid_bwd" in msg, (k, rc, msg)
    for n, c, v in ((0, 2, 8), (-1, 2, 8), (1, 1, 8), (1, 9, 8), (1, 2, 0), (1, 2, -4)):
        assert fwd(T, 2, n, c, v, P, P)[0] == E_BADSHAPE, (n, c, v)
        assert bwd(T, P, P, 2, n, c, v, T)[0] == E_BADSHAPE, (n, c, v)
    for args in ((None, 2, 1, 2, 8, P, P), (T, 2, 1, 2, 8, None, P), (T, 2, 1, 2, 8, P, None),
                 (_table(1), 2, 1, 2, 8, P, P), (_table(3), 4, 1, 2, 8, P, P)):
        assert fwd(*args)[0] == E_NULL, args
    for args in ((None, P, P, 2, 1, 2, 8, T), (T, None, P, 2, 1, 2, 8, T), (T, P, None, 2, 1, 2, 8, T), (T, P, P, 2, 1, 2, 8, None),
                 (_table(2), P, P, 3, 1, 2, 8, T), (T, P, P, 3, 1, 2, 8, _table(2))):
        assert bwd(*args)[0] == E_NULL, args


def test_pseudo_onehot_refusals():
    call = lambda tab, k, n, c, v, otab: _rc("fplx_ssl_pseudo_onehot", tab, k, n, c, v, otab, None)
    T = _table(3)
    for k in (0, 4, -1):
        rc, msg = call(T, k, 1, 2, 8, T)
        assert rc == E_BADSHAPE and "ssl_pseudo_onehot" in msg
    for n, c, v in ((0, 2, 8), (1, 1, 8), (1, 9, 8), (1, 2, 0)):
        assert call(T, 1, n, c, v, T)[0] == E_BADSHAPE
    for args in ((None, 1, 1, 2, 8, T), (T, 1, 1, 2, 8, None), (_table(1), 2, 1, 2, 8, T), (T, 3, 1, 2, 8, _table(2))):
        assert call(*args)[0] == E_NULL, args
    with pytest.raises(ValueError):                      # the wrapper raises what the library refuses
        _lib.call("fplx_ssl_pseudo_onehot", T, 0, 1, 2, 8, T, None)


# ---------------------------------------------------------------- registry, agents, package surface

def _cfg(method, net_type="UNet3D", **net_over):
    return {"dataset": {"tensor_type": "float"},
            "network": dict({"net_type": net_type, "class_num": 2}, **net_over),
            "training": {"gpus": [0], "loss_type": "DiceLoss", "iter_max": 10, "iter_valid": 2},
            "semi_supervised_learning": {"ssl_method": method}}


def test_second_registry_and_the_first_one_unchanged():
    assert sorted(fplx.SSLMethodDictAll) == ["CPS", "EntropyMinimization", "MeanTeacher", "UAMT", "URPC"]
    assert sorted(fplx.SSLMethodDict) == ["EntropyMinimization", "MeanTeacher", "UAMT"]
    assert fplx.SSLMethodDictAll["CPS"] is fplx.SSLCPS and fplx.SSLMethodDictAll["URPC"] is fplx.SSLURPC
    for name, cls in fplx.SSLMethodDictAll.items():
        assert fplx.ssl_agent_class_all(name) is cls and issubclass(cls, fplx.SSLSegAgent)
        if name in fplx.SSLMethodDict:
            assert fplx.SSLMethodDict[name] is cls
    with pytest.raises(ValueError, match="pymic.net.net2d"):
        fplx.ssl_agent_class_all("CCT")
    with pytest.raises(ValueError, match="Undefined"):
        fplx.ssl_agent_class_all("NoSuchMethod")
    for name in ("CCT", "CPS", "URPC"):
        with pytest.raises(ValueError, match="multi-decoder or two-branch networks"):
            fssl.ssl_agent_class(name)


def test_agents_refuse_the_wrong_deep_supervise_and_dsbn_networks():
    with pytest.raises(ValueError, match="deep_supervise = True"):
        fplx.SSLURPC(_cfg("URPC", deep_supervise=False))
    with pytest.raises(ValueError, match="deep_supervise = True"):
        fplx.SSLURPC(_cfg("URPC"))
    with pytest.raises(ValueError, match="deep_supervise = False"):
        fplx.SSLCPS(_cfg("CPS", deep_supervise=True))
    for name in ("UNet2D5_dsbn", "UNet3D_dsbn"):
        with pytest.raises(ValueError, match="domain-specific-BatchNorm"):
            fplx.SSLURPC(_cfg("URPC", net_type=name, deep_supervise=True))
        with pytest.raises(ValueError, match="domain-specific-BatchNorm"):
            fplx.SSLCPS(_cfg("CPS", net_type=name))


def test_the_loss_node_refuses_bad_inputs_with_reasons():
    t = torch.zeros(2, 2, 4)
    with pytest.raises(ValueError, match="deep_supervise"):
        fplx.pyramid_consistency_loss(t, 1)
    for k in (1, 5):
        with pytest.raises(ValueError, match="2 to 4 output scales"):
            fplx.pyramid_consistency_loss([t] * k, 1)
    with pytest.raises(RuntimeError):                    # GPU only, no CPU fallback
        fplx.pyramid_consistency_loss([t, t], 1)
    with pytest.raises(RuntimeError):
        fplx.cross_pseudo_labels([t, t])


def test_netgroup_is_one_module_and_the_package_surface():
    from fplx import netgroup, nll
    for n in ("BiNet", "TriNet", "GroupOptimizer", "_NetGroup"):
        assert getattr(nll, n) is getattr(netgroup, n), n
    assert fplx.nll.BiNet is fplx.netgroup.BiNet is fplx.BiNet and fplx.GroupOptimizer is netgroup.GroupOptimizer
    for n in ("SSLCPS", "SSLURPC", "SSLMethodDictAll", "ssl_agent_class_all", "pyramid_consistency_loss", "cross_pseudo_labels",
              "netgroup"):
        assert n in fplx.__all__ and hasattr(fplx, n), n
    for n in ("ssl_pyramid_fwd", "ssl_pyramid_bwd", "ssl_pseudo_onehot"):
        assert callable(getattr(fplx.ops, n)), n
    assert {"fplx_ssl_pyramid_fwd", "fplx_ssl_pyramid_bwd", "fplx_ssl_pseudo_onehot"} <= set(_lib.declared_symbols())
    import subprocess
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split() and l.split()[-1].startswith("fplx_")}
    assert exported == set(_lib.declared_symbols())
