"""CPU tests of the confident-learning layer: the oracle (tests/cloracle.py) on the worked example of DESIGN 1q, the C x C host part
of fplx.confident against it, the refusals, the C ABI's error codes before any launch and the package surface."""
import ctypes
import subprocess
import sys

import numpy as np
import pytest
import torch

import fplx
from fplx import _lib
from fplx import confident as F
from fplx import nll_clslsr

import cloracle as O


# ---------------------------------------------------------------- the worked example

def test_worked_example():
    s, psx = O.exact_case(0, 2, 210)
    r = O.run(s, psx)
    assert r.undecided == 0
    assert r.joint.tolist() == [[51, 7], [8, 58]]
    assert r.calibrated.tolist() == [[84, 12], [14, 100]]
    assert r.P.tolist() == [[84, 14], [12, 100]]
    assert r.ne.tolist() == [12, 14]
    assert {k: int(v.sum()) for k, v in r.masks.items()} == {"prune_by_class": 14, "prune_by_noise_rate": 26, "both": 13}
    # the host part of the product on the same joint
    cal = F.calibrate_confident_joint(r.joint, r.counts)
    assert np.array_equal(cal, r.calibrated) and cal.dtype == np.int64
    assert np.array_equal(F.keep_at_least_n_per_class(cal.T), r.P)


@pytest.mark.parametrize("c,m", [(3, 384), (4, 2310), (8, 4096)])
def test_host_part_equals_the_oracle(c, m):
    s, psx = O.exact_case(1000 * c + m, c, m)
    r = O.run(s, psx)
    cal = F.calibrate_confident_joint(r.joint, r.counts)
    assert np.array_equal(cal, r.calibrated)
    assert np.array_equal(cal.sum(1), r.counts)              # rows keep the class counts
    assert np.array_equal(F.keep_at_least_n_per_class(cal.T), r.P)


def test_round_preserving_sum():
    for fn in (F.round_preserving_sum, O.round_preserving_sum):
        assert fn([1.4, 1.3, 1.3]).tolist() == [2, 1, 1]                  # +1 goes to the largest remainder
        assert fn([1.6, 1.7, 1.7]).tolist() == [1, 2, 2]                  # -1 to the smallest
        assert fn([1.4, 1.4, 1.2]).tolist() == [1, 2, 1]                  # a tie: the stable argsort, reversed, takes the later one
        assert fn([0.4, 0.4, 0.4, 0.4, 0.4]).sum() == 2                   # several changes (+2)
        assert fn([0.6, 0.6, 0.6, 0.6, 0.6]).sum() == 3                   # several changes (-2)
        assert fn([2.5, 3.5, 1.0]).tolist() == [2, 4, 1]                  # half to even, nothing to move
        rng = np.random.default_rng(7)
        for _ in range(50):
            row = rng.random(rng.integers(2, 9)) * 40
            got = fn(row)
            assert got.sum() == np.round(row.sum()) and np.abs(got - row).max() <= 1.5         # a rounding and one move
    for row in ([1.4, 1.4, 1.2], [1.6, 1.6, 0.8], [0.4] * 5, [0.6] * 5):
        assert F.round_preserving_sum(row).tolist() == O.round_preserving_sum(row).tolist()


def test_keep_at_least_n_per_class_raises_a_small_diagonal():
    P = np.array([[2, 10, 0], [30, 50, 4], [8, 0, 40]], np.float64)      # P[true][given], diag[0] = 2 < 5
    got = F.keep_at_least_n_per_class(P)
    assert got[0, 0] == 5 and got[1, 1] == 50 and got[2, 2] == 40
    # column 0 has two other non-zero entries: each gives up 3 / 2
    assert np.array_equal(got, O.keep_at_least_n_per_class(P))
    assert got[1, 0] in (28, 29) and got[2, 0] in (6, 7)
    assert (got >= 0).all()
    same = np.array([[9, 1], [2, 8]], np.float64)
    assert np.array_equal(F.keep_at_least_n_per_class(same), same.astype(np.int64))


def test_softmax_decisions_are_stable_on_the_seeded_inputs():
    """the inputs of the GPU test 'decisions forced': a softmax that differs from scipy's by the derived bound can decide at most
    0.1 % of the voxels differently (checked here, on the CPU, on the scipy-fed oracle alone).  The voxels that DEFINE a cut sit on
    it - C class cuts and up to C (C - 1) pair cuts - so the count is never 0 and M must be large enough for them."""
    from scipy.special import softmax
    for c, m, seed in O.FORCED_CASES:
        s, x = O.logits_case(seed, c, m)
        psx = softmax(x, axis=0).astype(np.float32)
        r = O.run(s, psx)
        _, bound = O.softmax64(x)
        close = O.decision_distance(s, psx, r) <= 2 * bound.max(0) + 2 * r.thr_err.max()
        assert close.sum() <= 1e-3 * m, (c, m, int(close.sum()))


# ---------------------------------------------------------------- refusals

def test_refusals_of_the_python_layer():
    s, psx = O.exact_case(0, 2, 210)
    with pytest.raises(ValueError, match="CL_type"):
        fplx.get_confident_map(s, psx.T, "nope")
    with pytest.raises(ValueError, match="prune_method"):
        fplx.get_noise_indices(s, psx.T, "nope")
    for c in (1, 9):
        with pytest.raises(ValueError, match="classes"):
            fplx.get_confident_map(s, np.zeros((210, c), np.float32))
    with pytest.raises(ValueError, match="labels for"):
        fplx.get_confident_map(s[:-1], psx.T)
    with pytest.raises(ValueError, match="class 1 has 5 voxels"):
        F.refuse_counts(np.array([100, 5, 0, 0]))
    F.refuse_counts(np.array([100, 6, 0, 0]))
    with pytest.raises(ValueError, match="label >= 2"):
        F.refuse_counts(np.array([100, 50, 3, 0]))
    with pytest.raises(ValueError, match="NaN"):
        F.refuse_counts(np.array([100, 50, 0, 1]))
    with pytest.raises(ValueError, match="labelled 1 is confident"):
        F.calibrate_confident_joint(np.array([[5, 1], [0, 0]]), np.array([6, 7]))
    with pytest.raises(RuntimeError):                      # GPU only, no CPU path
        fplx.get_confident_map(torch.from_numpy(s), torch.from_numpy(psx.T.copy()))


def _cfg(net_type="UNet3D", **net):
    return {"dataset": {"tensor_type": "float", "root_dir": "."},
            "network": dict({"net_type": net_type, "class_num": 2}, **net),
            "testing": {"gpus": [0], "ckpt_mode": 2, "ckpt_name": "none.pt"}}


def test_refusals_of_the_agent(monkeypatch):
    for name in ("UNet2D5_dsbn", "UNet3D_dsbn"):
        with pytest.raises(ValueError, match="domain-specific-BatchNorm"):
            fplx.NLLCLSLSR(_cfg(name))
    with pytest.raises(ValueError, match="several outputs"):
        fplx.NLLCLSLSR(_cfg(deep_supervise=True))
    cfg = _cfg()
    cfg["testing"]["ckpt_mode"] = 3
    with pytest.raises(ValueError, match="ckpt_mode = 3"):
        fplx.NLLCLSLSR(cfg)
    ag = fplx.NLLCLSLSR(_cfg())
    assert isinstance(ag, fplx.SegmentationAgent) and ag.stage == "test" and ag.config["network"]["num_domains"] == 1
    monkeypatch.setattr(fplx.ddp, "init_from_env", lambda device=None: True)
    with pytest.raises(ValueError, match="single process"):
        fplx.NLLCLSLSR(_cfg())


def test_tool_without_arguments_prints_the_usage():
    assert nll_clslsr.get_confidence_map(["nll_clslsr"]) == 1
    import os
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(sys.path))
    r = subprocess.run([sys.executable, "-m", "fplx.nll_clslsr"], capture_output=True, text=True, env=env)
    assert r.returncode == 1 and "python -m fplx.nll_clslsr config.cfg" in r.stdout


# ---------------------------------------------------------------- the C ABI's refusals (before any launch)

E_BADSHAPE, E_WORKSPACE, E_NULL = -1, -3, -5
_buf = np.zeros(256, np.float64)
P = _buf.ctypes.data          # a non-null, 8-byte aligned pointer for the calls that are refused before they read it


def _rc(name, *args):
    rc = getattr(_lib.lib(), name)(*args)
    return rc, _lib.last_error()


def test_abi_refusals():
    ws = _lib.lib().fplx_cl_stats_ws_bytes()
    assert ws >= 16 + 8 * 8 * 1024 + 4 * 10 * 1024
    act = (ctypes.c_uint8 * 64)()
    calls = {
        "fplx_cl_softmax": lambda c, m: (P, c, m, P, None),
        "fplx_cl_class_stats": lambda c, m: (P, P, c, m, P, ws, P, P, P, None),
        "fplx_cl_confident_joint": lambda c, m: (P, P, c, m, P, P, None),
        "fplx_cl_select_keys": lambda c, m: (P, P, c, m, 0, -1, P, None),
        "fplx_cl_noise_mask": lambda c, m: (P, P, c, m, 2, P, P, act, P, P, None),
    }
    for name, args in calls.items():
        for c, m in ((1, 8), (9, 8), (2, 0), (2, -1), (2, 1 << 31)):
            rc, msg = _rc(name, *args(c, m))
            assert rc == E_BADSHAPE and name[5:] in msg, (name, c, m)
        ok = args(2, 8)
        for i, a in enumerate(ok[:-1]):
            if a != P:
                continue
            if name == "fplx_cl_class_stats" and i == 8:
                continue                                      # thr may be NULL
            bad = ok[:i] + (None,) + ok[i + 1:]
            rc, msg = _rc(name, *bad)
            assert rc == E_NULL and name[5:] in msg, (name, i)
    assert _rc("fplx_cl_class_stats", P, P, 2, 8, P, ws - 1, P, P, P, None)[0] == E_WORKSPACE
    assert _rc("fplx_cl_class_stats", P, P, 2, 8, P + 4, ws, P, P, P, None)[0] == E_BADSHAPE      # misaligned workspace
    for k, j in ((-1, -1), (2, -1), (0, 0), (0, 2), (1, 1)):
        rc, msg = _rc("fplx_cl_select_keys", P, P, 2, 8, k, j, P, None)
        assert rc == E_BADSHAPE and "cl_select_keys" in msg, (k, j)
    for method in (-1, 3):
        assert _rc("fplx_cl_noise_mask", P, P, 2, 8, method, P, P, act, P, P, None)[0] == E_BADSHAPE
    # a table the method does not read may be NULL; one it reads may not
    assert _rc("fplx_cl_noise_mask", P, P, 2, 8, 0, None, P, act, P, P, None)[0] == E_NULL
    assert _rc("fplx_cl_noise_mask", P, P, 2, 8, 1, P, None, act, P, P, None)[0] == E_NULL
    assert _rc("fplx_cl_noise_mask", P, P, 2, 8, 1, P, P, None, P, P, None)[0] == E_NULL
    assert _rc("fplx_cl_noise_mask", P, P, 2, 8, 2, None, P, act, P, P, None)[0] == E_NULL
    with pytest.raises(ValueError):                      # the wrapper raises what the library refuses
        _lib.call("fplx_cl_softmax", P, 9, 8, P, None)


def test_package_surface_and_exports():
    for n in ("confident", "nll_clslsr", "get_confident_map", "get_noise_indices", "compute_confident_joint",
              "calibrate_confident_joint", "keep_at_least_n_per_class", "round_preserving_sum", "NLLCLSLSR", "get_confidence_map"):
        assert n in fplx.__all__ and hasattr(fplx, n), n
    for n in ("cl_softmax", "cl_class_stats", "cl_confident_joint", "cl_select_keys", "cl_noise_mask"):
        assert callable(getattr(fplx.ops, n)), n
    assert sorted(fplx.NLLMethodDict) == ["CoTeaching", "TriNet"]           # CLSLSR is a tool, not a trainer
    assert issubclass(fplx.NLLCLSLSR, fplx.SegmentationAgent)
    declared = set(_lib.declared_symbols())
    new = {"fplx_cl_softmax", "fplx_cl_class_stats", "fplx_cl_stats_ws_bytes", "fplx_cl_confident_joint", "fplx_cl_select_keys",
           "fplx_cl_noise_mask"}
    assert new <= declared
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split() and l.split()[-1].startswith("fplx_")}
    assert exported == declared
    assert (fplx.ops.CL_BY_CLASS, fplx.ops.CL_BY_NOISE_RATE, fplx.ops.CL_BOTH) == (0, 1, 2)
    assert sorted(F.PRUNE_METHODS) == sorted(O.METHODS)
