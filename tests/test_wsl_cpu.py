"""Host side of the weakly-supervised feature without a GPU: the oracle of tests/wsloracle.py against the reference's recorded
results (tests/golden/wsl_losses.npz) and against itself (an fp32 evaluation passes, every mutation trips its bound), the
refusals of the six C entry points, the method registry, the agents' and losses' refusals, and the package surface."""
import os

import numpy as np
import pytest
import torch

import fplx
from fplx import _lib
from fplx import wsl as fwsl

import wsloracle as WO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wsl_losses.npz")
# The fixtures are the reference's own fp32 results: torch adds pairwise, so a sum of n <= 2^17 terms carries about
# log2(n) u <= 17 * 6e-8 = 1e-6 relative to the sum of magnitudes; the CRF's published form is a difference of two sums of which the
# result is no less than a tenth.  1e-5 of the value, and of the largest gradient entry, is an order above that.
FIXTURE_TOL = 1e-5


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.abs(got - want).max() <= FIXTURE_TOL * np.abs(want).max(), (what, float(np.abs(got - want).max()), float(np.abs(want).max()))


# ---------------------------------------------------------------- the oracle against the reference's recorded results

@pytest.mark.parametrize("name,radius", [("crf5", 5), ("crf2", 2)])
def test_crf_oracle_matches_the_reference_fixture(golden, name, radius):
    r = WO.crf_ref(golden[name + ".logits"], golden[name + ".image"], WO.DEFAULT_DESC, radius, True, 1.0)
    _close(r.out[2], golden[name + ".loss"], name)
    _close(r.dl, golden[name + ".dlogits"], name)


@pytest.mark.parametrize("tag,penalty,lam", [("l1", 1, 1.0), ("l2", 2, 0.25)])
def test_mumford_shah_oracle_matches_the_reference_fixture(golden, tag, penalty, lam):
    r = WO.ms_ref(golden["ms.logits"], golden["ms.image"], penalty, lam, True, 1.0)
    _close(r.out[2], golden["ms.%s.loss" % tag], tag)
    _close(r.dl, golden["ms.%s.dlogits" % tag], tag)


def test_tv_oracle_matches_the_reference_fixture(golden):
    x = golden["tv.logits"]
    r = WO.tv_ref(x, True, 1.0)
    WO.check_tv_case(r)
    _close(r.out[2], golden["tv.loss"], "tv")
    _close(WO.tv_grad_ref(x, r.count, 1.0, True)[0], golden["tv.dlogits"], "tv")


# ---------------------------------------------------------------- the oracle against itself

SHAPE = (2, 3, 3, 11, 9)                       # N D = 6 slices: a centroid that is not per slice shows


def _case(ci=2):
    return WO.logits_case("cpu.wsl", *SHAPE, ci=ci)


def test_fp32_evaluation_is_inside_the_bounds():
    x, im = _case()
    gs = 0.7
    r = WO.crf_ref(x, im, WO.DEFAULT_DESC, 2, True, gs)
    loss, dl, total = WO.autograd_crf(x, im, WO.DEFAULT_DESC, 2, True, gs, torch.float32)
    ratios = {"crf.out0": WO.ratio(total, r.out[0], r.out0_bound), "crf.dl": WO.ratio(dl, r.dl, r.dl_bound)}
    t = WO.tv_ref(x, True, gs)
    WO.check_tv_case(t)
    loss, dl, total = WO.autograd_tv(x, True, gs, torch.float32)
    ratios["tv.out0"] = WO.ratio(total, t.out[0], t.out0_bound)
    # the count of an fp32 evaluation: autograd of the SUM with respect to p' adds +-1.0, which is exact.  (The gradient of the
    # mean is not compared: torch adds +-g one by one and leaves a rounding residue where the counts cancel; the kernel counts
    # in integers.)
    pp = (torch.softmax(torch.from_numpy(x), 1) * 0.999 + 5e-4).requires_grad_(True)
    mn = -1 * torch.nn.functional.max_pool3d(-1 * pp, 3, 1, 1)
    torch.relu(torch.nn.functional.max_pool3d(mn, 3, 1, 1) - mn).sum().backward()
    assert np.array_equal(pp.grad.numpy()[t.count_free], t.count[t.count_free])
    for penalty, lam in ((1, 1.0), (2, 0.25)):
        m = WO.ms_ref(x, im, penalty, lam, True, gs)
        loss, dl, l0, l1 = WO.autograd_ms(x, im, penalty, lam, True, gs, torch.float32)
        ratios["ms%d.out0" % penalty] = WO.ratio(l0, m.out[0], m.out0_bound)
        ratios["ms%d.out1" % penalty] = WO.ratio(l1, m.out[1], m.out1_bound)
        ratios["ms%d.loss" % penalty] = WO.ratio(loss, m.out[2], m.loss_bound)
        ratios["ms%d.dl" % penalty] = WO.ratio(dl, m.dl, m.dl_bound)
    print(ratios)
    assert max(ratios.values()) <= 1.0, ratios
    assert min(ratios["crf.dl"], ratios["ms1.dl"]) > 0          # the fp32 evaluation does differ: the bounds are not vacuous


def test_undecided_share_of_the_issues_inputs():
    """logits of standard deviation 1.58 at 3 x 12 x 20 x 22: at most 1 % undecided voxels"""
    x, _ = WO.logits_case("cpu.wsl.share", 1, 3, 12, 20, 22)
    assert 1.4 < float(x.std()) < 1.8
    r = WO.tv_ref(x, True, 1.0, use_autograd=False)
    WO.check_tv_case(r)
    assert r.count.sum() == 0 and np.abs(r.count).max() > 0     # every +1 has its -1


@pytest.mark.parametrize("mut", WO.MUTATIONS)
def test_every_mutation_trips_its_bound(mut):
    x, im = _case()
    if mut.startswith("crf"):
        r = WO.crf_ref(x, im, WO.DEFAULT_DESC, 2, True, 1.0, use_autograd=False)
        m = WO.crf_ref(x, im, WO.DEFAULT_DESC, 2, True, 1.0, mut=mut)
        if mut == "crf_grad2":
            assert WO.ratio(m.dl, r.dl, r.dl_bound) > 1.0
        else:
            assert WO.ratio(m.out[0], r.out[0], r.out0_bound) > 1.0 and WO.ratio(m.out[2], r.out[2], r.loss_bound) > 1.0
            if mut != "crf_drop_oob":                           # a neighbour outside the slice adds nothing to kp either way
                assert WO.ratio(m.kp, r.kp, r.kp_bound) > 1.0 or mut == "crf_centre"
    elif mut.startswith("tv"):
        r = WO.tv_ref(x, True, 1.0, use_autograd=False)
        out, count, _ = WO.tv_fwd(x, True, mut)
        assert WO.ratio(out[0], r.out[0], r.out0_bound) > 1.0 and WO.ratio(out[2], r.out[2], r.loss_bound) > 1.0
        if mut == "tv_999":
            ref_dl, bound = WO.tv_grad_ref(x, r.count, 1.0, True)
            assert WO.ratio(WO.tv_bwd(x, r.count, 1.0, True, mut)[0], ref_dl, bound) > 1.0
        else:
            assert (count != r.count)[r.count_free].any()
    else:
        penalty, lam = 1, 1.0
        r = WO.ms_ref(x, im, penalty, lam, True, 1.0, use_autograd=False)
        out, cen, _ = WO.ms_fwd(x, im, penalty, lam, True, mut)
        dl = WO.ms_bwd(x, im, cen, penalty, lam, 1.0, True, mut)[0]
        assert WO.ratio(out[2], r.out[2], r.loss_bound) > 1.0 and WO.ratio(dl, r.dl, r.dl_bound) > 1.0
        if mut == "ms_volume":
            assert WO.ratio(cen, r.cen, r.cen_bound) > 1.0 and WO.ratio(out[0], r.out[0], r.out0_bound) > 1.0
        elif mut == "ms_l1l2":
            assert WO.ratio(out[1], r.out[1], r.out1_bound) > 1.0


def test_exact_families_are_exact():
    x = WO.tv_exact_case("cpu.tv.exact", 2, 3, 2, 3, 5)
    assert all(len(np.unique(row)) == row.size for row in x.reshape(6, -1))
    r = WO.tv_ref(x, False, 1.0)
    assert not r.undecided.any() and r.count_free.all()
    p, im = WO.dyadic_case("cpu.ms.exact", 2, 3, 3, 5, 7, 2)
    out, _, _ = WO.ms_fwd(p, im, 1, 1.0, False)
    assert out[1] * 64 == np.round(out[1] * 64) and out[1] * 64 < WO.LO.EXACT_LIMIT


# ---------------------------------------------------------------- the C ABI's refusals (before any launch)

E_BADSHAPE, E_NULL = -1, -5
_buf = np.zeros(64, np.float32)
P = _buf.ctypes.data          # a non-null pointer for the calls that are refused before they read it
_desc = np.array([1.0, 5.0, 0.1, 1.0, 3.0, 0.0], np.float32)
DESC = _desc.ctypes.data
BAD_SHAPES = ((0, 2, 1, 4, 4), (1, 1, 1, 4, 4), (1, 9, 1, 4, 4), (1, 2, 0, 4, 4), (1, 2, 1, 0, 4), (1, 2, 1, 4, -1), (1, 2, 2, 1 << 15, 1 << 15),
              (8192, 8, 1, 4, 4))


def _rc(name, *args):
    rc = getattr(_lib.lib(), name)(*args)
    return rc, _lib.last_error()


def _null_each(name, args, pointer_slots):
    for i in pointer_slots:
        a = list(args)
        a[i] = None
        assert _rc(name, *a)[0] == E_NULL, (name, i)


def test_gatedcrf_refusals():
    fwd = lambda n, c, ci, d, h, w, nk=2, r=5, desc=DESC: ("fplx_wsl_gatedcrf_fwd", P, P, n, c, ci, d, h, w, desc, nk, r, 1, P, P, P, None)
    bwd = lambda n, c, d, h, w: ("fplx_wsl_gatedcrf_bwd", P, P, P, n, c, d, h, w, 1, P, None)
    for n, c, d, h, w in BAD_SHAPES:
        rc, msg = _rc(*fwd(n, c, 1, d, h, w))
        assert rc == E_BADSHAPE and "wsl_gatedcrf_fwd" in msg
        rc, msg = _rc(*bwd(n, c, d, h, w))
        assert rc == E_BADSHAPE and "wsl_gatedcrf_bwd" in msg
    for ci, nk, r in ((0, 2, 5), (5, 2, 5), (1, 0, 5), (1, 5, 5), (1, 2, 0), (1, 2, 9)):
        assert _rc(*fwd(1, 2, ci, 1, 4, 4, nk, r))[0] == E_BADSHAPE, (ci, nk, r)
    for bad in ([1.0, 0.0, 0.0], [1.0, -1.0, 0.1], [1.0, 5.0, -0.1]):          # no modality; negative sigmas
        arr = np.array(bad, np.float32)
        rc, msg = _rc(*fwd(1, 2, 1, 1, 4, 4, 1, 5, arr.ctypes.data))
        assert rc == E_BADSHAPE and "descriptor 0" in msg
    f = fwd(1, 2, 1, 1, 4, 4)
    _null_each(f[0], f[1:], (0, 1, 8, 12, 13, 14))
    b = bwd(1, 2, 1, 4, 4)
    _null_each(b[0], b[1:], (0, 1, 2, 9))


def test_tv_refusals():
    fwd = lambda n, c, d, h, w, wsb=1 << 30: ("fplx_wsl_tv_fwd", P, n, c, d, h, w, 1, P, P, wsb, P, P, None)
    bwd = lambda n, c, d, h, w: ("fplx_wsl_tv_bwd", P, P, P, n, c, d, h, w, 1, P, None)
    for n, c, d, h, w in BAD_SHAPES:
        assert _rc(*fwd(n, c, d, h, w))[0] == E_BADSHAPE and _rc(*bwd(n, c, d, h, w))[0] == E_BADSHAPE
    rc, msg = _rc(*fwd(1, 2, 1, 4, 4, 12 * 32 - 1))
    assert rc == E_BADSHAPE and "workspace" in msg
    f = fwd(1, 2, 1, 4, 4)
    _null_each(f[0], f[1:], (0, 7, 8, 10, 11))
    b = bwd(1, 2, 1, 4, 4)
    _null_each(b[0], b[1:], (0, 1, 2, 9))


def test_mumford_shah_refusals():
    fwd = lambda n, c, ci, d, h, w, pen=1, lam=1.0: ("fplx_wsl_mumford_shah_fwd", P, P, n, c, ci, d, h, w, pen, lam, 1, P, P, P, None)
    bwd = lambda n, c, ci, d, h, w, pen=1, lam=1.0: ("fplx_wsl_mumford_shah_bwd", P, P, P, P, n, c, ci, d, h, w, pen, lam, 1, P, None)
    for n, c, d, h, w in BAD_SHAPES:
        assert _rc(*fwd(n, c, 1, d, h, w))[0] == E_BADSHAPE and _rc(*bwd(n, c, 1, d, h, w))[0] == E_BADSHAPE
    for ci, pen, lam in ((0, 1, 1.0), (5, 1, 1.0), (1, 0, 1.0), (1, 3, 1.0), (1, 1, -0.5)):
        assert _rc(*fwd(1, 2, ci, 1, 4, 4, pen, lam))[0] == E_BADSHAPE and _rc(*bwd(1, 2, ci, 1, 4, 4, pen, lam))[0] == E_BADSHAPE
    f = fwd(1, 2, 1, 1, 4, 4)
    _null_each(f[0], f[1:], (0, 1, 11, 12, 13))
    b = bwd(1, 2, 1, 1, 4, 4)
    _null_each(b[0], b[1:], (0, 1, 2, 3, 13))
    with pytest.raises(ValueError):                      # the wrapper raises what the library refuses
        _lib.call(*fwd(1, 1, 1, 1, 4, 4))


# ---------------------------------------------------------------- registry, agents, losses, package surface

def _cfg(method="GatedCRF", net_type="UNet3D", **wsl_over):
    return {"dataset": {"tensor_type": "float"},
            "network": {"net_type": net_type, "class_num": 2},
            "training": {"gpus": [0], "loss_type": "DiceLoss", "iter_max": 10, "iter_valid": 2},
            "weakly_supervised_learning": dict({"wsl_method": method}, **wsl_over)}


def test_method_dict_and_dmpls():
    assert sorted(fplx.WSLMethodDict) == ["EntropyMinimization", "GatedCRF", "MumfordShah", "TotalVariation", "USTM"]
    for name, cls in fplx.WSLMethodDict.items():
        assert issubclass(cls, fplx.WSLSegAgent) and issubclass(cls, fplx.SegmentationAgent)
        assert fwsl.wsl_agent_class(name) is cls
    with pytest.raises(ValueError, match="UNet2D_DualBranch / UNet3D_DualBranch"):
        fwsl.wsl_agent_class("DMPLS")
    with pytest.raises(ValueError):
        fwsl.wsl_agent_class("NoSuchMethod")


def test_agents_refuse_dsbn_networks_and_odd_t():
    for name in ("UNet2D5_dsbn", "UNet3D_dsbn"):
        for cls in fplx.WSLMethodDict.values():
            with pytest.raises(ValueError, match="domain-specific-BatchNorm"):
                cls(_cfg(net_type=name))
    for t in (3, 7, 1, 18, 0):
        with pytest.raises(ValueError, match="ustm_mcdroput_n"):
            fplx.WSLUSTM(_cfg("USTM", ustm_mcdroput_n=t))
    with pytest.raises(ValueError, match="not integral"):
        fplx.WSLGatedCRF(_cfg(gatedcrfloss_radius=2.5))
    ag = fplx.WSLGatedCRF(_cfg(gatedcrfloss_radius=5.0))           # the reference's default literal
    assert ag.radius == 5 and ag.kernels == [{'weight': 1.0, 'xy': 5, 'rgb': 0.1}, {'weight': 1.0, 'xy': 3}]


def test_loss_calculator_ignores_the_entropy_weight():
    ag = fplx.WSLTotalVariation.__new__(fplx.WSLTotalVariation)
    ag.loss_dict, ag.distributed = None, False
    ag.config = {"training": {"loss_type": "DiceLoss"}, "network": {}}
    ag.create_loss_calculator(1.0)
    assert type(ag.loss_calculator) is fplx.DiceLoss and ag.loss_calculator.terms == (1.0, 0.0, 0.0, 0.0)


def test_losses_construct_read_their_keys_and_refuse():
    for n in ("TotalVariationLoss", "MumfordShahLoss", "GatedCRFLoss"):
        assert n not in fplx.SegLossDict and n not in fplx.SegLossDictAll
    assert fplx.TotalVariationLoss().softmax is True and fplx.TotalVariationLoss({"loss_softmax": False}).softmax is False
    m = fplx.MumfordShahLoss({"MumfordShahLoss_penalty": "l2", "MumfordShahLoss_lambda": 0.25})
    assert (m.penalty, m.grad_w, m.softmax) == ("l2", 0.25, True)
    m = fplx.MumfordShahLoss({"mumfordshahloss_penalty": "l2", "mumfordshahloss_lambda": 0.25})      # what a parsed .cfg holds
    assert (m.penalty, m.grad_w) == ("l1", 1.0)
    with pytest.raises(ValueError, match="its 2-D branch is never taken"):
        fplx.TotalVariationLoss()({"prediction": torch.zeros(1, 2, 4, 4)})
    with pytest.raises(RuntimeError):                     # GPU only, no CPU fallback
        fplx.TotalVariationLoss()({"prediction": [torch.zeros(1, 2, 3, 4, 4)], "softmax": True})
    crf = fplx.GatedCRFLoss()
    y, desc, sample = torch.full((1, 2, 4, 4), 0.5), [{'weight': 1.0, 'xy': 5, 'rgb': 0.1}], {'rgb': torch.zeros(1, 1, 4, 4)}
    one = torch.ones(1, 1, 4, 4)
    for kw, reason in ((dict(mask_src=one), "masks are not built"), (dict(mask_dst=one), "masks are not built"),
                       (dict(compatibility=torch.zeros(2, 2)), "compatibility matrices are not built"),
                       (dict(custom_modality_downsamplers={}), "custom_modality_downsamplers are not built"),
                       (dict(out_kernels_vis=True), "out_kernels_vis is not built")):
        with pytest.raises(ValueError, match=reason):
            crf(y, desc, 5, sample, 4, 4, **kw)
    with pytest.raises(ValueError, match="different from the input's"):
        crf(y, desc, 5, sample, 8, 8)
    with pytest.raises(ValueError, match="not integral"):
        crf(y, desc, 2.5, sample, 4, 4)
    with pytest.raises(ValueError, match="'xy' and 'rgb' are built"):
        crf(y, [{'weight': 1.0, 'depth': 2.0}], 5, sample, 4, 4)
    with pytest.raises(RuntimeError):
        crf(y, desc, 5.0, sample, 4, 4)


def test_package_surface_and_exports():
    for n in ("wsl", "WSLSegAgent", "WSLEntropyMinimization", "WSLTotalVariation", "WSLMumfordShah", "WSLGatedCRF", "WSLUSTM",
              "WSLMethodDict", "TotalVariationLoss", "MumfordShahLoss", "GatedCRFLoss"):
        assert n in fplx.__all__ and hasattr(fplx, n), n
    new = {"fplx_wsl_gatedcrf_fwd", "fplx_wsl_gatedcrf_bwd", "fplx_wsl_tv_fwd", "fplx_wsl_tv_bwd", "fplx_wsl_mumford_shah_fwd",
           "fplx_wsl_mumford_shah_bwd"}
    for n in new:
        assert callable(getattr(fplx.ops, n[len("fplx_"):])), n
    declared = set(_lib.declared_symbols())
    assert new <= declared
    import subprocess
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split() and l.split()[-1].startswith("fplx_")}
    assert exported == declared
    from fplx import wsl_main
    assert wsl_main.main(["wsl_main"]) == 1
