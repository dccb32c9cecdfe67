"""Host side of the semi-supervised feature without a GPU: the oracle of tests/ssloracle.py checked against itself (the fp32
restatement passes, every mutation trips its bound), get_rampup_ratio, the refusals of the six C entry points, the method
registry and the agents' refusals, and the package surface."""
import ctypes

import numpy as np
import pytest
import torch

import fplx
from fplx import _lib
from fplx import ssl as fssl

import ssloracle as SO

F32 = np.float32


# ---------------------------------------------------------------- the oracle against itself

CASES = [(1, 2, 63, 2), (3, 3, 9240, 8), (1, 8, 9240, 16), (3, 3, 9240, 0), (1, 2, 5, 0)]


def _case(n, c, v, t, ramp=0.3):
    s, q, mc = SO.logits_case("cpu.%d.%d.%d.%d" % (n, c, v, t), n, c, v, t)
    thr = SO.uamt_threshold(ramp, c) if t else 0.0
    return s, q, mc, thr


@pytest.mark.parametrize("n,c,v,t", CASES)
def test_fp32_restatement_is_inside_the_bounds(n, c, v, t):
    s, q, mc, thr = _case(n, c, v, t)
    r = SO.consistency_ref(s, q, mc, thr, True, 0.7)
    SO.check_case_is_a_real_test(r, n, v)
    out, keep, _, _ = SO.consistency_fwd(s, q, mc, thr, True, F32)
    res = SO.check_consistency_fwd(r, out, keep.astype(np.uint8) if t else None, "restatement")
    assert res["out0"] > 0 or v < 64                   # the fp32 evaluation does differ: the bound is not vacuous
    dl, bound = SO.consistency_grad_ref(s, q, keep, 0.7, t, True)
    got = SO.consistency_bwd(s, q, keep, 0.7, t, True, F32)
    assert SO.ratio(got, dl, bound) <= 1.0
    e = SO.entropy_ref(s, True, 0.7)
    eo, _ = SO.entropy_fwd(s, True, F32)
    assert SO.ratio(eo[0], e.out[0], e.out0_bound) <= 1.0 and SO.ratio(eo[2], e.out[2], e.loss_bound) <= 1.0
    assert SO.ratio(SO.entropy_bwd(s, 0.7, True, F32), e.dl, e.dl_bound) <= 1.0


def test_undecided_share_and_kept_share_of_the_issues_inputs():
    """C in {2, 3, 8}, T in {2, 8, 16}, ramps 0 and 0.3: at most 1 % undecided, kept share inside [0.2, 0.9]"""
    for c in (2, 3, 8):
        for t in (2, 8, 16):
            for ramp in (0.0, 0.3):
                s, q, mc = SO.logits_case("share.%d.%d" % (c, t), 1, c, 2048, t)
                r = SO.consistency_ref(s, q, mc, SO.uamt_threshold(ramp, c), True)
                SO.check_case_is_a_real_test(r, 1, 2048)


def test_exact_cases_have_no_undecided_voxel():
    for (n, c, v, t) in [(1, 2, 63, 2), (3, 8, 9240, 16), (3, 3, 5, 8)]:
        s, q, mc, thr = SO.exact_case("exact.cpu", n, c, v, t)
        SO.exact_pre(s, q)
        r = SO.consistency_ref(s, q, mc, thr, False)
        assert not r.undecided.any() and 0 < r.keep.sum() < r.keep.size or v < 10
        out, keep, _, _ = SO.consistency_fwd(s, q, mc, thr, False, F32)
        assert out[0] == r.out[0] and out[1] == r.out[1] and np.array_equal(keep, r.keep)     # fp32 in any order is exact here
    e, p = SO.ema_exact_case("ema.cpu", 1001)
    assert np.array_equal(SO.ema(e, p, 0.75, F32).astype(np.float64), SO.ema(e, p, 0.75))


def _trips(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("mut", SO.MUTATIONS)
def test_every_mutation_trips_its_bound(mut):
    n, c, v, t = 3, 3, 9240, 8
    s, q, mc, thr = _case(n, c, v, t)
    if mut in ("den_c", "drop_voxel", "row_twice"):
        r = SO.consistency_ref(s, q, mc, thr, True)
        out, keep, _, _ = SO.consistency_fwd(s, q, mc, thr, True, F32, mut)
        assert _trips(lambda: SO.check_consistency_fwd(r, out, keep.astype(np.uint8), mut))
        if mut != "den_c":                                  # MeanTeacher's sum too
            r0 = SO.consistency_ref(s, q, None, 0.0, True)
            out0, _, _, _ = SO.consistency_fwd(s, q, None, 0.0, True, F32, mut)
            assert _trips(lambda: SO.check_consistency_fwd(r0, out0, None, mut))
            e = SO.entropy_ref(s, True)
            assert SO.ratio(SO.entropy_fwd(s, True, F32, mut)[0][0], e.out[0], e.out0_bound) > 1.0
    elif mut == "unc_eps":
        # the 1e-6 is what keeps a class no pass predicts from giving 0 x log 0: probabilities with exact zeros
        s, q, mc, thr = SO.exact_case("mut.eps", n, c, v, t)
        r = SO.consistency_ref(s, q, mc, thr, False)
        out, keep, _, _ = SO.consistency_fwd(s, q, mc, thr, False, F32, mut)
        assert _trips(lambda: SO.check_consistency_fwd(r, out, keep.astype(np.uint8), mut))
    elif mut == "mask_le":
        # voxels no pass gives any probability: m = 0, unc = 0 exactly, bound 0 - decided, and NOT kept at thr = 0
        s, q, mc, _ = SO.exact_case("mut.le", n, c, v, t)
        mc[:, :, :, ::3] = 0.0
        r = SO.consistency_ref(s, q, mc, 0.0, False)
        assert not r.undecided[:, ::3].any() and not r.keep[:, ::3].any()
        good, keep_good, _, _ = SO.consistency_fwd(s, q, mc, 0.0, False, F32)
        SO.check_consistency_fwd(r, good, keep_good.astype(np.uint8), "strict")
        out, keep, _, _ = SO.consistency_fwd(s, q, mc, 0.0, False, F32, mut)
        assert _trips(lambda: SO.check_consistency_fwd(r, out, keep.astype(np.uint8), mut))
    elif mut == "grad_swap":
        keep = SO.consistency_fwd(s, q, mc, thr, True)[1]
        dl, bound = SO.consistency_grad_ref(s, q, keep, 1.0, t, True)
        assert SO.ratio(SO.consistency_bwd(s, q, keep, 1.0, t, True, F32, mut), dl, bound) > 1.0
    elif mut in ("ent_999", "ent_lnc"):
        e = SO.entropy_ref(s, True)
        assert SO.ratio(SO.entropy_fwd(s, True, F32, mut)[0][2], e.out[2], e.loss_bound) > 1.0
        assert SO.ratio(SO.entropy_bwd(s, 1.0, True, F32, mut), e.dl, e.dl_bound) > 1.0
    else:
        assert mut == "ema_swap"
        g = SO.LO.rng("ema.mut")
        e, p = g.standard_normal(4097).astype(F32), g.standard_normal(4097).astype(F32)
        ref, bound = SO.ema_ref(e, p, 0.99)
        assert SO.ratio(SO.ema(e, p, 0.99, F32), ref, bound) <= 1.0
        assert SO.ratio(SO.ema(e, p, 0.99, F32, mut), ref, bound) > 1.0


def test_clamped_normal_moments_against_quadrature():
    m2, m4 = SO.clamped_normal_moments(0.1, 0.2)
    z = np.linspace(-12, 12, 2400001)
    w = np.clip(0.1 * z, -0.2, 0.2)
    pdf = np.exp(-0.5 * z * z) / np.sqrt(2 * np.pi)
    dz = z[1] - z[0]
    assert abs((w ** 2 * pdf).sum() * dz - m2) < 1e-9 and abs((w ** 4 * pdf).sum() * dz - m4) < 1e-11


# ---------------------------------------------------------------- get_rampup_ratio (util/ramps.py:13-33)

def test_rampup_ratio_values():
    for i, start, end in [(0, 0, 100), (30, 0, 100), (100, 0, 100), (250, 0, 100), (5, 10, 20), (15, 10, 20)]:
        ic = min(max(i, start), end)
        lin = (ic - start) / (end - start)
        assert fplx.get_rampup_ratio(i, start, end, "linear") == lin
        assert fplx.get_rampup_ratio(i, start, end) == lin
        assert fplx.get_rampup_ratio(i, start, end, "sigmoid") == float(np.exp(-5.0 * (1.0 - lin) * (1.0 - lin)))
        assert fplx.get_rampup_ratio(i, start, end, "cosine") == float(.5 * (np.cos(np.pi * (1.0 - lin)) + 1))
    assert fplx.get_rampup_ratio(100, 0, 100, "sigmoid") == 1.0
    with pytest.raises(ValueError, match="Undefined rampup mode"):
        fplx.get_rampup_ratio(1, 0, 2, "exp")


# ---------------------------------------------------------------- the C ABI's refusals (before any launch)

E_BADSHAPE, E_NULL = -1, -5
_buf = np.zeros(64, np.float32)
P = _buf.ctypes.data          # a non-null pointer for the calls that are refused before they read it


def _rc(name, *args):
    rc = getattr(_lib.lib(), name)(*args)
    return rc, _lib.last_error()


def test_perturb_refusals():
    assert _rc("fplx_ssl_perturb", None, None, P, 8, 1, 0.1, 0.2, 0, 0, None)[0] == E_NULL
    assert _rc("fplx_ssl_perturb", P, None, None, 8, 1, 0.1, 0.2, 0, 0, None)[0] == E_NULL
    for n, reps, clip in ((0, 1, 0.2), (-3, 1, 0.2), (8, 0, 0.2), (8, 65, 0.2), (8, 1, -0.1)):
        rc, msg = _rc("fplx_ssl_perturb", P, P, P, n, reps, 0.1, clip, 0, 0, None)
        assert rc == E_BADSHAPE and "ssl_perturb" in msg, (n, reps, clip, rc, msg)


def test_consistency_refusals():
    fwd = lambda s, q, mc, t, n, c, v, mask, part, out: _rc("fplx_ssl_consistency_fwd", s, q, mc, t, n, c, v, 0.5, 1, mask, part, out,
                                                            None)
    bwd = lambda s, q, mask, out, gs, n, c, v, t, d: _rc("fplx_ssl_consistency_bwd", s, q, mask, out, gs, n, c, v, t, 1, d, None)
    for n, c, v in ((0, 2, 8), (-1, 2, 8), (1, 1, 8), (1, 9, 8), (1, 2, 0)):
        rc, msg = fwd(P, P, None, 0, n, c, v, None, P, P)
        assert rc == E_BADSHAPE and "ssl_consistency_fwd" in msg
        rc, msg = bwd(P, P, None, None, P, n, c, v, 0, P)
        assert rc == E_BADSHAPE and "ssl_consistency_bwd" in msg
    for t in (1, 3, 15, 18, -2):
        assert fwd(P, P, P, t, 1, 2, 8, P, P, P)[0] == E_BADSHAPE
        assert bwd(P, P, P, P, P, 1, 2, 8, t, P)[0] == E_BADSHAPE
    for args in ((None, P, None, 0, 1, 2, 8, None, P, P), (P, None, None, 0, 1, 2, 8, None, P, P), (P, P, None, 0, 1, 2, 8, None, None, P),
                 (P, P, None, 0, 1, 2, 8, None, P, None), (P, P, None, 2, 1, 2, 8, P, P, P), (P, P, P, 2, 1, 2, 8, None, P, P)):
        assert fwd(*args)[0] == E_NULL, args
    for args in ((None, P, None, None, P, 1, 2, 8, 0, P), (P, None, None, None, P, 1, 2, 8, 0, P), (P, P, None, None, None, 1, 2, 8, 0, P),
                 (P, P, None, None, P, 1, 2, 8, 0, None), (P, P, None, P, P, 1, 2, 8, 2, P), (P, P, P, None, P, 1, 2, 8, 2, P)):
        assert bwd(*args)[0] == E_NULL, args


def test_entropy_refusals():
    for n, c, v in ((0, 2, 8), (1, 1, 8), (1, 9, 8), (1, 2, 0), (1, 2, -4)):
        assert _rc("fplx_ssl_entropy_fwd", P, n, c, v, 1, P, P, None)[0] == E_BADSHAPE
        assert _rc("fplx_ssl_entropy_bwd", P, P, n, c, v, 1, P, None)[0] == E_BADSHAPE
    for args in ((None, 1, 2, 8, 1, P, P), (P, 1, 2, 8, 1, None, P), (P, 1, 2, 8, 1, P, None)):
        assert _rc("fplx_ssl_entropy_fwd", *(args + (None,)))[0] == E_NULL
    for args in ((None, P, 1, 2, 8, 1, P), (P, None, 1, 2, 8, 1, P), (P, P, 1, 2, 8, 1, None)):
        assert _rc("fplx_ssl_entropy_bwd", *(args + (None,)))[0] == E_NULL


def test_ema_refusals():
    assert _rc("fplx_ema_step", None, P, 8, 0.5, None)[0] == E_NULL
    assert _rc("fplx_ema_step", P, None, 8, 0.5, None)[0] == E_NULL
    for n, alpha in ((0, 0.5), (-1, 0.5), (8, 1.5), (8, -0.1)):
        rc, msg = _rc("fplx_ema_step", P, P, n, alpha, None)
        assert rc == E_BADSHAPE and "ema_step" in msg
    with pytest.raises(ValueError):                      # the wrapper raises what the library refuses
        _lib.call("fplx_ema_step", P, P, 0, 0.5, None)


# ---------------------------------------------------------------- registry, agents, package surface

def _cfg(method="MeanTeacher", net_type="UNet3D", **ssl_over):
    return {"dataset": {"tensor_type": "float"},
            "network": {"net_type": net_type, "class_num": 2},
            "training": {"gpus": [0], "loss_type": "DiceLoss", "iter_max": 10, "iter_valid": 2},
            "semi_supervised_learning": dict({"ssl_method": method}, **ssl_over)}


def test_method_dict_and_refused_methods():
    assert sorted(fplx.SSLMethodDict) == ["EntropyMinimization", "MeanTeacher", "UAMT"]
    assert fplx.SSLMethodDict["UAMT"] is fplx.SSLUncertaintyAwareMeanTeacher
    assert issubclass(fplx.SSLUncertaintyAwareMeanTeacher, fplx.SSLMeanTeacher)
    for cls in fplx.SSLMethodDict.values():
        assert issubclass(cls, fplx.SSLSegAgent) and issubclass(cls, fplx.SegmentationAgent)
        assert fssl.ssl_agent_class([k for k, v in fplx.SSLMethodDict.items() if v is cls][0]) is cls
    for name in ("CCT", "CPS", "URPC"):
        with pytest.raises(ValueError, match="multi-decoder or two-branch networks"):
            fssl.ssl_agent_class(name)
    with pytest.raises(ValueError):
        fssl.ssl_agent_class("NoSuchMethod")


def test_agents_refuse_odd_t_and_dsbn_networks():
    for t in (3, 7, 1, 18, 0):
        with pytest.raises(ValueError, match="uamt_mcdroput_n"):
            fplx.SSLUncertaintyAwareMeanTeacher(_cfg("UAMT", uamt_mcdroput_n=t))
    for name in ("UNet2D5_dsbn", "UNet3D_dsbn"):
        for cls in fplx.SSLMethodDict.values():
            with pytest.raises(ValueError, match="domain-specific-BatchNorm"):
                cls(_cfg(net_type=name))


def test_loss_calculator_ignores_the_entropy_weight():
    ag = fplx.SSLMeanTeacher.__new__(fplx.SSLMeanTeacher)
    ag.loss_dict, ag.distributed = None, False
    ag.config = {"training": {"loss_type": "DiceLoss"}, "network": {}}
    ag.create_loss_calculator(1.0)                        # what SegmentationAgent.train_valid passes when `dual` is false
    assert type(ag.loss_calculator) is fplx.DiceLoss and ag.loss_calculator.terms == (1.0, 0.0, 0.0, 0.0)
    base = fplx.SegmentationAgent.__new__(fplx.SegmentationAgent)
    base.loss_dict, base.distributed, base.config = None, False, ag.config
    base.create_loss_calculator(1.0)
    assert base.loss_calculator.terms[3] == 1.0           # the DSBN agent keeps its term


def test_entropy_loss_is_not_registered_and_constructs():
    assert "EntropyLoss" not in fplx.SegLossDict and "EntropyLoss" not in fplx.SegLossDictAll
    assert fplx.EntropyLoss().softmax is True and fplx.EntropyLoss({"loss_softmax": False}).softmax is False
    with pytest.raises(RuntimeError):                     # GPU only, no CPU fallback
        fplx.EntropyLoss()({"prediction": [torch.zeros(1, 2, 4)], "softmax": True})
    with pytest.raises(ValueError, match="go together"):
        fplx.consistency_loss(torch.zeros(1, 2, 4), torch.zeros(1, 2, 4), torch.zeros(2, 1, 2, 4))


def test_package_surface_and_exports():
    for n in ("ssl", "SSLSegAgent", "SSLEntropyMinimization", "SSLMeanTeacher", "SSLUncertaintyAwareMeanTeacher", "SSLMethodDict",
              "EntropyLoss", "consistency_loss", "ema_update", "get_rampup_ratio"):
        assert n in fplx.__all__ and hasattr(fplx, n), n
    for n in ("ssl_perturb", "ssl_consistency_fwd", "ssl_consistency_bwd", "ssl_entropy_fwd", "ssl_entropy_bwd", "ema_step"):
        assert callable(getattr(fplx.ops, n)), n
    declared = set(_lib.declared_symbols())
    new = {"fplx_ssl_perturb", "fplx_ssl_consistency_fwd", "fplx_ssl_consistency_bwd", "fplx_ssl_entropy_fwd", "fplx_ssl_entropy_bwd",
           "fplx_ema_step"}
    assert new <= declared
    import subprocess
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split() and l.split()[-1].startswith("fplx_")}
    assert exported == declared
    from fplx import ssl_main
    assert ssl_main.main(["ssl_main"]) == 1
