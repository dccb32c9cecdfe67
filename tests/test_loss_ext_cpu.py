"""Host side of the second loss family without a GPU: registry, constructors, CombinedLoss merging, dispatch, argument checks of
the C ABI, and the oracle of tests/lossoracle_ext.py checked against itself (fp32 emulation passes, every mutation is rejected)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import fplx
from fplx import _lib, ops
from fplx import loss as floss

import lossoracle as LO
import lossoracle_ext as LE
import losses_ext_cases as LC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---------------------------------------------------------------- registry and constructors

def test_registry_all_names():
    with np.load(os.path.join(GOLDEN, "losses_ext.npz")) as z:
        names = json.loads(bytes(z["names_json"]).decode())
    assert len(names) == 9
    assert sorted(fplx.SegLossDictAll) == sorted(names + ["DiceLoss_weight"])
    assert set(fplx.SegLossDict) == {"DiceLoss", "CrossEntropyLoss", "DiceLoss_weight"}
    for k, cls in fplx.SegLossDict.items():
        assert fplx.SegLossDictAll[k] is cls
    for cls in fplx.SegLossDictAll.values():
        assert issubclass(cls, fplx.loss.AbstractSegLoss)
        assert cls.forward is floss.AbstractSegLoss.forward and cls._run is floss.AbstractSegLoss._run      # engine step


def test_make_loss_default_dictionary_unchanged():
    with pytest.raises(ValueError):
        fplx.make_loss({"loss_type": "FocalDiceLoss", "focaldiceloss_beta": 2.0})
    m = fplx.make_loss({"loss_type": "FocalDiceLoss", "focaldiceloss_beta": 2.0}, fplx.SegLossDictAll)
    assert isinstance(m, fplx.FocalDiceLoss) and m.terms == (0.0, 0.0, 0.0, 0.0)


def test_agent_defaults_to_all(monkeypatch):
    ag = fplx.SegmentationAgent.__new__(fplx.SegmentationAgent)
    ag.loss_dict, ag.distributed = None, False
    ag.config = {"training": {"loss_type": "NoiseRobustDiceLoss", "noiserobustdiceloss_gamma": 1.5}}
    ag.create_loss_calculator()
    assert ag.loss_dict is fplx.SegLossDictAll and isinstance(ag.loss_calculator, fplx.NoiseRobustDiceLoss)
    ag.loss_dict = fplx.SegLossDict                      # a dictionary that was set is kept
    with pytest.raises(ValueError):
        ag.create_loss_calculator()


def test_constructor_keys_defaults_errors():
    for cls, key in ((fplx.FocalDiceLoss, "focaldiceloss_beta"), (fplx.NoiseRobustDiceLoss, "noiserobustdiceloss_gamma"),
                     (fplx.ExpLogLoss, "explogloss_w_dice"), (fplx.ExpLogLoss, "explogloss_gamma")):
        full = {"focaldiceloss_beta": 2.0, "noiserobustdiceloss_gamma": 1.5, "explogloss_w_dice": 0.8, "explogloss_gamma": 0.3}
        cls(full)
        del full[key]
        with pytest.raises(KeyError):
            cls(full)
    g = fplx.GeneralizedCELoss({})
    assert g.q == 0.5 and g.enable_pix_weight is False and g.cls_weight is None and g.softmax is True
    g = fplx.GeneralizedCELoss({"loss_gce_q": 0.7, "loss_with_pixel_weight": True, "loss_class_weight": [1, 2], "loss_softmax": False})
    assert g.ext_spec() == ((0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0), (1.0, 1.0, 0.5, 1.0, 0.7, 0.25, True, (1.0, 2.0)))
    assert g.softmax is False
    assert fplx.SLSRLoss().epsilon == 0.25 and fplx.SLSRLoss({"slsrloss_epsilon": 0.1}).epsilon == 0.1
    assert fplx.MSELoss().ext_spec()[0] == (0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)
    assert fplx.MAELoss().ext_spec()[0] == (0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0)
    assert fplx.DiceLoss().ext_spec() is None
    # GeneralizedCE with loss_with_pixel_weight and no map: the reference's error, before any GPU work
    with pytest.raises(ValueError, match="Pixel weight is enabled but not defined"):
        fplx.GeneralizedCELoss({"loss_with_pixel_weight": True})({"prediction": torch.zeros(1, 2, 1, 1, 1),
                                                                  "ground_truth": torch.zeros(1, 2, 1, 1, 1)})
    with pytest.raises(ValueError):
        ops.loss_ext_cfg((0, 0, 0, 0), fplx.GeneralizedCELoss({"loss_class_weight": [1, 2, 3]}).ext_spec(), 2)


def test_cfg_array_layout():
    spec = fplx.GeneralizedCELoss({"loss_gce_q": 0.7, "loss_class_weight": [1, 2]}).ext_spec()
    cfg = list(ops.loss_ext_cfg((0.5, 0.25, 0.0, 1.0), spec, 2))
    want = LE.cfg_array((0.5, 0.25, 0.0, 1.0), LE.weights(gce=1.0), LE.params(beta=1.0, gamma_nr=1.0, w_dice_el=0.5, gamma_el=1.0,
                                                                             q=0.7, class_weight=[1, 2]), 2)
    assert len(cfg) == 18 + 2 and np.array_equal(np.asarray(cfg, np.float32), np.asarray(want, np.float32))
    assert ops.loss_ext_k(3) == 37 and ops.loss_ext_nout(3) == 14 and ops.loss_ext_ncoef(2, 3) == 30


def test_combined_merging_and_refusal():
    cfg = dict(LC.PARAMS, loss_type=["DiceLoss", "NoiseRobustDiceLoss", "GeneralizedCELoss"], loss_weight=[0.5, 0.3, 0.2])
    c = fplx.CombinedLoss(cfg, fplx.SegLossDictAll)
    assert c.terms == (0.5, 0.0, 0.0, 0.0)
    w, prm = c.ext_spec()
    assert w == (0.0, 0.3, 0.0, 0.2, 0.0, 0.0, 0.0) and prm[1] == 1.5 and prm[4] == 0.7
    # the existing pin: old names only -> no second-family term, terms as before
    c = fplx.CombinedLoss({"loss_type": ["DiceLoss", "CrossEntropyLoss"], "loss_weight": [0.6, 0.4]}, fplx.SegLossDict)
    assert c.terms == (0.6, 0.4, 0.0, 0.0) and c.ext_spec() is None
    # the same loss twice with the same parameters adds up
    c = fplx.CombinedLoss(dict(LC.PARAMS, loss_type=["FocalDiceLoss", "FocalDiceLoss"], loss_weight=[0.25, 0.5]), fplx.SegLossDictAll)
    assert c.ext_spec()[0][0] == 0.75
    # a missing key is the constructor's KeyError
    with pytest.raises(KeyError):
        fplx.CombinedLoss({"loss_type": ["DiceLoss", "ExpLogLoss"], "loss_weight": [1, 1]}, fplx.SegLossDictAll)

    class Focal3(fplx.FocalDiceLoss):
        def __init__(self, params=None):
            super(Focal3, self).__init__(dict(params, focaldiceloss_beta=3.0))

    d = dict(fplx.SegLossDictAll, Focal3=Focal3)
    with pytest.raises(ValueError, match="one parameter slot"):
        fplx.CombinedLoss(dict(LC.PARAMS, loss_type=["FocalDiceLoss", "Focal3"], loss_weight=[0.5, 0.5]), d)
    # the entropy regulariser of training() combines with the new losses
    m = fplx.make_loss(dict(LC.PARAMS, loss_type="MSELoss"), fplx.SegLossDictAll, 1.0)
    assert m.terms == (0.0, 0.0, 0.0, 1.0) and m.ext_spec()[0][5] == 1.0


def test_dispatch_old_and_new(monkeypatch):
    calls = []

    def boom(*a, **k):
        raise AssertionError("the second family's pass was called for a loss without such a term")

    def fake(name):
        def f(*a, **k):
            calls.append(name)
        return f

    monkeypatch.setattr(ops, "require_gpu", lambda *a: None)
    x = {"prediction": torch.zeros(1, 2, 1, 2, 2, requires_grad=True), "ground_truth": torch.zeros(1, 2, 1, 2, 2)}
    for n in ("seg_loss_ext_fwd", "seg_loss_ext_bwd", "seg_loss_ext_fwd_dist"):
        monkeypatch.setattr(ops, n, boom)
    monkeypatch.setattr(ops, "seg_loss_fwd", fake("fwd"))
    monkeypatch.setattr(ops, "seg_loss_bwd", fake("bwd"))
    for mod in (fplx.DiceLoss(), fplx.CrossEntropyLoss(), fplx.EntropyTerm(),
                fplx.CombinedLoss({"loss_type": ["DiceLoss", "CrossEntropyLoss"], "loss_weight": [0.6, 0.4]}, fplx.SegLossDictAll)):
        del calls[:]
        mod(x).backward()
        assert calls == ["fwd", "bwd"] and mod.last_out.numel() == 4 + 2
    monkeypatch.setattr(ops, "seg_loss_fwd", boom)
    monkeypatch.setattr(ops, "seg_loss_bwd", boom)
    monkeypatch.setattr(ops, "seg_loss_ext_fwd", fake("ext_fwd"))
    monkeypatch.setattr(ops, "seg_loss_ext_bwd", fake("ext_bwd"))
    del calls[:]
    mod = fplx.make_loss(dict(LC.PARAMS, loss_type=["DiceLoss", "MAELoss"], loss_weight=[1, 1]), fplx.SegLossDictAll)
    mod(x).backward()
    assert calls == ["ext_fwd", "ext_bwd"] and mod.last_out.numel() == 4 + 2 + 7


def test_train_step_keyword():
    import inspect
    sig = inspect.signature(fplx.TrainStep.__init__)
    assert list(sig.parameters)[:3] == ["self", "net", "loss_terms"] and sig.parameters["loss_ext"].default is None


# ---------------------------------------------------------------- the C ABI refuses bad arguments before any launch

def _abi():
    lib = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    cfg = (ctypes.c_float * 26)()
    return lib, p, cfg, buf


@pytest.mark.parametrize("c", [0, 9, -1])
def test_abi_rejects_class_count(c):
    lib, p, cfg, _ = _abi()
    assert lib.fplx_seg_loss_ext_fwd(p, p, None, None, 1, c, 8, cfg, 1, p, p, p, None) == -1
    assert "c=%d" % c in _lib.last_error()
    assert lib.fplx_seg_loss_ext_sums(p, p, None, 1, c, 8, cfg, 1, p, p, p, None) == -1
    assert lib.fplx_seg_loss_ext_from_sums(p, p, None, 1, 1, c, 8, 0, cfg, p, p, None) == -1
    assert lib.fplx_seg_loss_ext_bwd(p, p, None, p, p, 1, c, 8, cfg, 1, p, None) == -1


def test_abi_rejects_shapes_and_nulls():
    lib, p, cfg, _ = _abi()
    assert lib.fplx_seg_loss_ext_fwd(p, p, None, None, 65, 2, 8, cfg, 1, p, p, p, None) == -1          # N > 64
    assert lib.fplx_seg_loss_ext_fwd(p, p, None, None, 1, 2, 0, cfg, 1, p, p, p, None) == -1           # no voxels
    assert lib.fplx_seg_loss_ext_from_sums(p, p, None, 2, 1, 2, 8, 0, cfg, p, p, None) == -1           # n_global < n
    assert lib.fplx_seg_loss_ext_fwd(p, p, None, None, 1, 2, 8, None, 1, p, p, p, None) == -5          # cfg
    for miss in range(5):
        a = [p, p, p, p, p]
        a[miss] = None
        assert lib.fplx_seg_loss_ext_fwd(a[0], a[1], None, None, 1, 2, 8, cfg, 1, a[2], a[3], a[4], None) == -5
        assert lib.fplx_seg_loss_ext_sums(a[0], a[1], None, 1, 2, 8, cfg, 1, a[2], a[3], a[4], None) == -5
        assert lib.fplx_seg_loss_ext_bwd(a[0], a[1], None, a[2], a[3], 1, 2, 8, cfg, 1, a[4], None) == -5
    for miss in range(4):
        a = [p, p, p, p]
        a[miss] = None
        assert lib.fplx_seg_loss_ext_from_sums(a[0], a[1], None, 1, 1, 2, 8, 0, cfg, a[2], a[3], None) == -5
    cfg[2] = 1.0                                                        # image-weighted Dice without its weights
    assert lib.fplx_seg_loss_ext_fwd(p, p, None, None, 1, 2, 8, cfg, 1, p, p, p, None) == -5
    cfg[2], cfg[7], cfg[17] = 0.0, 1.0, 1.0                             # GeneralizedCE by pixel weight without a map
    assert lib.fplx_seg_loss_ext_fwd(p, p, None, None, 1, 2, 8, cfg, 1, p, p, p, None) == -5
    assert lib.fplx_seg_loss_ext_bwd(p, p, None, p, p, 1, 2, 8, cfg, 1, p, None) == -5
    with pytest.raises(ValueError):
        _lib.check(-5)


# ---------------------------------------------------------------- the oracle against itself

ALL = LE.weights(focal=0.3, noise_robust=0.2, explog=0.4, gce=0.5, mae=0.6, mse=0.7, slsr=0.8)
TERMS = (0.5, 0.25, 0.0, 0.125)
N, C, V = 2, 3, 4650


def _data(softmax, exact=False):
    y = LO.hard_labels("ext.cpu.y", N, C, V)
    pw = LO.exact_weights("ext.cpu.w", N, V)
    if softmax:
        return LO.real_logits("ext.cpu.lg", N, C, V), y, pw
    return (LO.exact_probs("ext.cpu.pe", N, C, V) if exact else LO.real_probs("ext.cpu.p", N, C, V)), y, pw


def _ratios(r, sm, outs, dl):
    return dict(out=LO.ratio(outs[0], r.out, r.out_bound), dl=LO.ratio(dl, r.dl, r.dl_bound), sums=LO.ratio(sm, r.sums, r.sums_bound))


@pytest.fixture(scope="module")
def refs():
    out = {}
    prm = LE.params(use_pw=True, class_weight=[0.5, 1.5, 2.0])
    for softmax in (True, False):
        x, y, pw = _data(softmax)
        out[softmax] = (x, y, pw, ALL, prm, LE.reference_ext(x, y, pw, TERMS, ALL, prm, softmax, gscale=0.5))
    x, y, pw = _data(False, exact=True)
    w7 = LE.weights(mae=1.0, mse=0.5, noise_robust=0.25, focal=0.5)
    assert ((x == y).sum() > 100), "the sign mutation needs voxels with p == y"
    out["exact"] = (x, y, pw, w7, LE.PRM, LE.reference_ext(x, y, pw, TERMS, w7, LE.PRM, False, gscale=0.5))
    return out


@pytest.mark.parametrize("key", [True, False, "exact"])
def test_fp32_emulation_passes(refs, key):
    x, y, pw, w7, prm, r = refs[key]
    sm, tot, outs, dl = LE.restate_ext(x, y, pw, TERMS, w7, prm, key is True, gscale=0.5)
    res = LE.check_B(r, out=outs[0], dl=dl, sm=sm, totals=tot, what=str(key))
    assert max(res.values()) > 1e-4, "a bound a thousand times above the emulation's error checks nothing"
    # the split path: two ranks, totals added in float64
    sm2, tot2, outs2, dl2 = LE.restate_ext(x, y, pw, TERMS, w7, prm, key is True, gscale=0.5, shards=2)
    LE.check_B(r, out=outs2[0], dl=dl2, sm=sm2, what=str(key) + " split")


@pytest.mark.parametrize("mut", LE.MUTATIONS)
def test_mutations_are_rejected(refs, mut):
    keys = ["exact"] if mut == "sign0_one" else [True, False]
    for key in keys:
        x, y, pw, w7, prm, r = refs[key]
        with np.errstate(all="ignore"):
            sm, tot, outs, dl = LE.restate_ext(x, y, pw, TERMS, w7, prm, key is True, gscale=0.5, mut=mut)
        rr = _ratios(r, sm, outs, dl)
        assert max(rr.values()) > 1.0, "%s (%s) passes the bound: %s" % (mut, key, rr)


def test_exact_part_on_the_emulation():
    n, c, v = 2, 2, 4650
    pr, y = LO.exact_probs("ext.cpu.A", n, c, v), LO.hard_labels("ext.cpu.Ay", n, c, v)
    assert LE.exact_pre_ext(pr, y) < LO.EXACT_LIMIT
    w7 = LE.weights(mse=1.0, mae=1.0)
    sm = LE.sums_ext(pr, y, None, False, w7, LE.PRM, np.float32)
    assert LE.check_A(sm, sm.sum(0), pr, y, None) == n * (3 * c + 2)
    bad = LE.sums_ext(pr, y, None, False, w7, LE.PRM, np.float32, mut="drop_voxel")
    with pytest.raises(AssertionError):
        LE.check_A(bad, None, pr, y, None)
    with pytest.raises(AssertionError):                                # a row too long for exact fp32 sums is refused
        big = np.ones((1, 8, 4096 * 8), np.float32)
        LE.exact_pre_ext(big, np.zeros_like(big))
