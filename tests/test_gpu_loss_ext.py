"""The second loss family on the GPU: the reference's fixtures through SegLossDictAll and through TrainStep's loss path, the exact
and rounding-bound oracles of tests/lossoracle_ext.py, the split batch, GeneralizedCE's class and pixel weights against float64,
a SegmentationAgent run on the engine step, and the second family's pass without a term of its own against the first family's pass,
bit for bit."""
import os

import numpy as np
import pytest
import torch

import detdata
import lossoracle as LO
import lossoracle_ext as LE
import losses_ext_cases as LC
from make_golden_cfg import NETS, SHAPES
from util import load_det_weights

pytestmark = pytest.mark.gpu


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return LC.load(golden_dir)


@pytest.fixture(scope="module")
def tiny_net():
    import fplx
    p = dict(NETS["tiny"])
    net = fplx.UNet2D5_dsbn(p)
    load_det_weights(net, p, "cuda")
    return net


# ---------------------------------------------------------------- 1. the reference's fixtures

@pytest.mark.parametrize("skey", sorted(LC.SHAPES))
def test_fixture_cases_match_reference(golden, tiny_net, skey):
    import fplx
    logits, label, pw = LC.inputs(skey)
    lab, pwc = _cuda(label), _cuda(pw)
    opt = fplx.FusedAdam(tiny_net, 1e-3)
    for tag, (name, softmax, with_pw) in LC.CASES.items():
        cfg = LC.config(tag)
        mod = fplx.make_loss(cfg, fplx.SegLossDictAll)
        assert isinstance(mod, fplx.CombinedLoss) == isinstance(name, list)
        x = _cuda(logits if softmax else golden[skey + ".probs"]).requires_grad_(True)
        d = {"prediction": x, "ground_truth": lab}
        if with_pw:
            d["pixel_weight"] = pwc
        val = mod(d)
        val.backward()
        ref_v, ref_g = float(golden["%s.%s.loss" % (skey, tag)]), golden["%s.%s.dlogits" % (skey, tag)]
        got_g = x.grad.cpu().numpy()
        print("%s.%s value err %.3g grad err %.3g of max %.3g" % (skey, tag, abs(val.item() - ref_v), np.abs(got_g - ref_g).max(),
                                                                 np.abs(ref_g).max()))
        assert abs(val.item() - ref_v) < 1e-5, (skey, tag, val.item(), ref_v)
        np.testing.assert_allclose(got_g, ref_g, atol=2e-4 * np.abs(ref_g).max(), rtol=1e-3, err_msg="%s.%s" % (skey, tag))
        # the class Dice metric stays where the agent reads it; the new terms' values follow
        c = label.shape[1]
        assert mod.last_out.numel() == 4 + c + 7
        # TrainStep's loss path: same kernels, same buffers' contents -> the same bits
        ts = fplx.TrainStep(tiny_net, mod.terms, mod.softmax, optimizer=opt, loss_ext=mod.ext_spec())
        xs = x.detach()
        n, v = xs.shape[0], xs[0, 0].numel()
        part, coef = ts._loss_buffers(n, c, v, xs.device)
        out, dl = ts._loss_ext(xs, lab, pwc if with_pw else None, None, ts._one, part, coef)
        assert torch.equal(out, mod.last_out), (skey, tag)
        assert torch.equal(dl, x.grad), (skey, tag)


def test_gce_pixel_weight_without_map_raises():
    import fplx
    x = torch.zeros(1, 2, 1, 4, 4, device="cuda")
    with pytest.raises(ValueError, match="Pixel weight is enabled but not defined"):
        fplx.GeneralizedCELoss({"loss_with_pixel_weight": True})({"prediction": x, "ground_truth": x})


# ---------------------------------------------------------------- the raw ABI

def _dev(lg, y, pw, terms, w7, prm, softmax, gscale=1.0, n_global=None, totals_in=None):
    """sums -> (totals given or the kernel's) -> from_sums -> bwd on the device -> numpy (sums, totals, out, dlogits)"""
    from fplx import ops
    import ctypes
    n, c, v = lg.shape
    cfgl = LE.cfg_array(terms, w7, prm, c)
    cfg = (ctypes.c_float * len(cfgl))(*cfgl)
    L, Y, W = _cuda(lg), _cuda(y), _cuda(pw)
    k = ops.loss_ext_k(c)
    assert k == LE.ext_k(c)
    part = torch.empty((n, ops.loss_rows(v), k), dtype=torch.float32, device="cuda")
    sums = torch.empty((n + 1, k), dtype=torch.float64, device="cuda")
    ops.seg_loss_ext_sums(L.view(n, c, 1, 1, v), Y.view(n, c, 1, 1, v), W, cfg, softmax, part, sums[:n], sums[n])
    tot = sums[n] if totals_in is None else torch.from_numpy(totals_in).cuda()
    out = torch.empty(ops.loss_ext_nout(c), dtype=torch.float32, device="cuda")
    coef = torch.empty(ops.loss_ext_ncoef(n, c), dtype=torch.float32, device="cuda")
    ops.seg_loss_ext_from_sums(sums[:n], tot, None, n, n if n_global is None else n_global, c, v, pw is not None, cfg, out, coef)
    dl = torch.empty_like(L)
    gs = torch.full((1,), float(gscale), dtype=torch.float32, device="cuda")
    ops.seg_loss_ext_bwd(L.view(n, c, 1, 1, v), Y.view(n, c, 1, 1, v), W, coef, gs, cfg, softmax, dl.view(n, c, 1, 1, v))
    torch.cuda.synchronize()
    return sums[:n].cpu().numpy(), sums[n].cpu().numpy(), out.cpu().numpy(), dl.cpu().numpy()


NCV = [(s[0], s[1], int(np.prod(s[2:]))) for s in (LC.SHAPES[k] for k in sorted(LC.SHAPES))] + [(2, 1, 700), (2, 3, 1)]


# ---------------------------------------------------------------- 2a. exact oracle

@pytest.mark.parametrize("ncv", NCV)
@pytest.mark.parametrize("weighted", [False, True])
def test_exact_sums(ncv, weighted):
    n, c, v = ncv
    key = "ext.A.%d.%d.%d" % ncv
    pr, y = LO.exact_probs(key, n, c, v), LO.hard_labels(key + ".y", n, c, v)
    pw = LO.exact_weights(key + ".w", n, v) if weighted else None
    sm, tot, _, _ = _dev(pr, y, pw, (1.0, 0.0, 0.0, 0.0), LE.weights(mse=1.0, mae=1.0), LE.PRM, False)
    assert LE.check_A(sm, tot, pr, y, pw, what=key) == n * (3 * c + 2)
    # the first family's exact entries are the first family's: same positions, same values
    LO.check_A(sm[:, :6 * c + 3], tot[:6 * c + 3], None, pr, y, pw, False, what=key)


# ---------------------------------------------------------------- 2b. rounding-bound oracle

ALL = LE.weights(focal=0.3, noise_robust=0.2, explog=0.4, gce=0.5, mae=0.6, mse=0.7, slsr=0.8)
SINGLE = [LE.weights(**{k: 1.0}) for k in LE.EXT_TERMS]


@pytest.mark.parametrize("ncv", NCV)
@pytest.mark.parametrize("softmax", [True, False])
@pytest.mark.parametrize("weighted", [False, True])
def test_rounding_bound(ncv, softmax, weighted):
    n, c, v = ncv
    key = "ext.B.%d.%d.%d" % ncv
    x = LO.real_logits(key, n, c, v) if softmax else LO.real_probs(key, n, c, v)
    y = LO.hard_labels(key + ".y", n, c, v)
    pw = LO.exact_weights(key + ".w", n, v) if weighted else None
    prm = LE.params(use_pw=weighted, class_weight=[0.5 + 0.25 * k for k in range(c)])
    for tag, terms, w7 in [(LE.EXT_TERMS[i], (0.0, 0.0, 0.0, 0.0), w) for i, w in enumerate(SINGLE)] + \
                          [("all", (0.5, 0.25, 0.0, 0.125), ALL)]:
        r = LE.reference_ext(x, y, pw, terms, w7, prm, softmax, gscale=0.5)
        sm, tot, out, dl = _dev(x, y, pw, terms, w7, prm, softmax, gscale=0.5)
        res = {k: LO.ratio(g, w_, b) for k, (g, w_, b) in dict(out=(out, r.out, r.out_bound), dlogits=(dl, r.dl, r.dl_bound),
                                                               sums=(sm, r.sums, r.sums_bound)).items()}
        print("%s sm=%d w=%d %s: error / bound %s" % (key, softmax, weighted, tag, {k: "%.3g" % q for k, q in res.items()}))
        LE.check_B(r, out=out, dl=dl, sm=sm, totals=tot, what="%s %s" % (key, tag))


# ---------------------------------------------------------------- 3. split batch

@pytest.mark.parametrize("skey", ["a", "c"])
def test_split_batch_is_bit_identical(skey):
    s = LC.SHAPES[skey]
    n, c, v = s[0], s[1], int(np.prod(s[2:]))
    lg = LO.real_logits("ext.split." + skey, n, c, v)[:2]
    y = LO.hard_labels("ext.split.y." + skey, n, c, v)[:2]
    pw = LO.exact_weights("ext.split.w." + skey, n, v)[:2]
    terms, prm = (0.5, 0.25, 0.0, 0.125), LE.params(use_pw=True)
    sm, tot, out, dl = _dev(lg, y, pw, terms, ALL, prm, True, gscale=0.5)
    halves = [_dev(lg[i:i + 1], y[i:i + 1], pw[i:i + 1], terms, ALL, prm, True, gscale=0.5) for i in range(2)]
    added = halves[0][1] + halves[1][1]                                    # totals added on the host
    assert np.array_equal(added, tot)
    for i in range(2):
        _, _, o_i, dl_i = _dev(lg[i:i + 1], y[i:i + 1], pw[i:i + 1], terms, ALL, prm, True, gscale=0.5, n_global=2, totals_in=added)
        assert np.array_equal(o_i, out), (i, o_i, out)
        assert np.array_equal(dl_i, dl[i:i + 1]), i


# ---------------------------------------------------------------- 4. GeneralizedCE weights

def test_gce_class_and_pixel_weights():
    import fplx
    n, c, D, H, W = LC.SHAPES["b"][0] + 1, 3, 3, 7, 13
    v = D * H * W
    lg, y = LO.real_logits("ext.gce", n, c, v), LO.hard_labels("ext.gce.y", n, c, v)
    pw = LO.exact_weights("ext.gce.w", n, v)
    w7 = LE.weights(gce=1.0)
    L5 = lambda a: _cuda(a).view(a.shape[0], -1, D, H, W)
    for cw, use_pw in (([0.5, 1.5, 2.0], False), (None, True), ([0.5, 1.5, 2.0], True)):
        prm = LE.params(q=0.7, class_weight=cw, use_pw=use_pw)
        r = LE.reference_ext(lg, y, pw, (0.0,) * 4, w7, prm, True)
        cfg = {"loss_gce_q": 0.7, "loss_with_pixel_weight": use_pw}
        if cw is not None:
            cfg["loss_class_weight"] = cw
        x = L5(lg).requires_grad_(True)
        mod = fplx.GeneralizedCELoss(cfg)
        val = mod({"prediction": x, "ground_truth": L5(y), "pixel_weight": L5(pw)})
        val.backward()
        LE.check_B(r, out=mod.last_out.cpu().numpy(), dl=x.grad.cpu().numpy().reshape(n, c, v), what="gce %s %s" % (cw, use_pw))
        assert abs(val.item() - r.out[0]) <= r.out_bound[0]
    # the weighted mean is sum(gce w) / sum(w): twice the weights, the same loss
    a = fplx.GeneralizedCELoss({"loss_with_pixel_weight": True})({"prediction": L5(lg), "ground_truth": L5(y), "pixel_weight": L5(pw)})
    b = fplx.GeneralizedCELoss({"loss_with_pixel_weight": True})({"prediction": L5(lg), "ground_truth": L5(y),
                                                                  "pixel_weight": L5(pw * 2)})
    assert a.item() == b.item()
    # all-ones class weights are the unweighted loss, bit for bit
    res = []
    for cfg in ({}, {"loss_class_weight": [1, 1, 1]}):
        x = L5(lg).requires_grad_(True)
        mod = fplx.GeneralizedCELoss(cfg)
        mod({"prediction": x, "ground_truth": L5(y)}).backward()
        res.append((mod.last_out.clone(), x.grad.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


# ---------------------------------------------------------------- 5. the agent on the engine step

def _batches():
    n, _, D, H, W = SHAPES["tiny"]
    out = []
    for dom in (0, 1):
        b = {"image": torch.from_numpy(detdata.normal("ext.x.d%d" % dom, SHAPES["tiny"])),
             "label_prob": torch.from_numpy(detdata.ball_label((D, H, W), 5.0, n=n, offsets=[(dom, 1, -2), (1, -3, 2 + dom)]))}
        out.append(b)
    return out


def test_agent_runs_new_losses_on_the_engine_step():
    import fplx
    res = []
    for route in (True, False):
        tcfg = {"dis": False, "train_fpl_uda": True, "loss_type": ["DiceLoss", "NoiseRobustDiceLoss"], "loss_weight": [0.5, 0.5],
                "noiserobustdiceloss_gamma": 1.5, "optimizer": "Adam", "learning_rate": 1e-3, "momentum": 0.9, "weight_decay": 1e-5,
                "lr_scheduler": "MultiStepLR", "lr_gamma": 0.5, "lr_milestones": [2, 4], "iter_valid": 1, "gpus": [0]}
        cfg = {"dataset": {"tensor_type": "float"}, "network": dict(NETS["tiny"]), "training": tcfg, "testing": {}}
        agent = fplx.SegmentationAgent(cfg, "train")
        agent.create_network()
        load_det_weights(agent.net, cfg["network"], "cuda")
        agent.create_optimizer()
        agent.create_loss_calculator()
        assert agent.loss_dict is fplx.SegLossDictAll
        agent.engine_mode = route
        b = _batches()
        agent.set_loaders([b[0]], [b[1]])
        scs = [agent.training_all() for _ in range(2)]
        assert (agent._ts is not None) == route
        if route:
            assert agent._ts.loss_ext == agent.loss_calculator.ext_spec()
        res.append((agent.net.flat_params.detach().clone(), scs))
    (pa, sa), (pb, sb) = res
    for a, b_ in zip(sa, sb):
        assert np.isfinite(a["loss"]) and a["loss"] > 0
        assert abs(a["loss"] - b_["loss"]) < 1e-6 and np.abs(a["class_dice"] - b_["class_dice"]).max() < 1e-6
    assert float((pa - pb).abs().max()) <= 1e-6 * float(pb.abs().max())


# ---------------------------------------------------------------- 6. no second-family term: the first family's pass

def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


# Where the two passes differ, and did before they shared any code (the two copies of the forward loop fuse differently at
# C >= 3): the pixel-weighted intersection sums (column 6c + 2) and the CE numerator (column 6C) of single partial rows, by 1-2 ulp
# of fp32, and what the finalize computes from them - out[2], Dice coefficients B (odd indices of coef).  part: (n, row, column);
# out, coef: index.  Key: (n, c, v), softmax, weighted.  These entries must pass lossoracle.check_B on both sides; every other
# entry is bitwise.  The gradient has no list: from the SAME coefficients the two backward kernels must give the same bits
# everywhere, and from their own coefficients wherever those are bit-equal.
DIFFERED_BEFORE = {
    ((3, 3, 4099), True, True): dict(part=[(0, 0, 18), (1, 1, 18)]),
    ((3, 3, 4099), False, False): dict(part=[(1, 1, 18)], out=[2]),
    ((3, 3, 4099), False, True): dict(part=[(0, 1, 18), (1, 1, 18)]),
    ((2, 8, 9001), True, True): dict(part=[(0, 0, 14), (0, 1, 14), (0, 1, 26), (0, 2, 2), (0, 2, 20), (1, 0, 38), (1, 1, 14)], coef=[5]),
    ((2, 8, 9001), False, True): dict(part=[(0, 0, 20), (0, 0, 44), (0, 1, 32), (0, 1, 48), (0, 2, 14), (0, 2, 44), (1, 0, 2), (1, 0, 20),
                                            (1, 2, 44)], coef=[15, 27]),
}


@pytest.mark.parametrize("ncv", [(1, 2, 37), (2, 1, 700), (3, 3, 4099), (2, 8, 9001)])
@pytest.mark.parametrize("softmax", [True, False])
@pytest.mark.parametrize("weighted", [False, True])
def test_zero_ext_weights_is_the_first_family(ncv, softmax, weighted):
    """one short block, C = 1, two and three partial rows with ragged tails, odd N with odd K, C = MAXC; soft labels, real
    predictions and non-dyadic weights, so every product rounds.  The sums, values, coefficients and gradient the two passes
    share are compared as bit patterns, except at DIFFERED_BEFORE; the second family's backward is run once more on the first
    family's coefficients, and that gradient is bitwise everywhere."""
    from fplx import ops
    n, c, v = ncv
    key = "ext.same.%d.%d.%d" % ncv
    xh = LO.real_logits(key, n, c, v) if softmax else LO.real_probs(key, n, c, v)
    yh = LO.soft_labels(key + ".y", n, c, v)
    g = LO.rng(key + ".w")
    pwh = (g.random((n, v)) * 1.99 + 0.005).astype(np.float32) if weighted else None
    iwh = (g.random(n) * 1.99 + 0.005).astype(np.float32) if weighted else None
    x, y, pw, iw = _cuda(xh), _cuda(yh), _cuda(pwh), _cuda(iwh)
    terms = (0.5, 0.3, 0.2 if weighted else 0.0, 0.1)
    cfg = ops.loss_ext_cfg(terms, ((0.0,) * 7, ops.LOSS_EXT_DEFAULTS), c)
    gs = torch.full((1,), 0.7, dtype=torch.float32, device="cuda")
    rows, k0 = ops.loss_rows(v) - 5, 6 * c + 3
    got = []
    for k, nout, ncoef, fwd, bwd, how in (
            (ops.loss_k(c), 4 + c, n * c * 2 + 2, ops.seg_loss_fwd, ops.seg_loss_bwd, terms),
            (ops.loss_ext_k(c), ops.loss_ext_nout(c), ops.loss_ext_ncoef(n, c), ops.seg_loss_ext_fwd, ops.seg_loss_ext_bwd, cfg)):
        part = torch.zeros((n, ops.loss_rows(v), k), dtype=torch.float32, device="cuda")
        out = torch.zeros(nout, dtype=torch.float32, device="cuda")
        coef = torch.zeros(ncoef, dtype=torch.float32, device="cuda")
        dl = torch.zeros_like(x)
        fwd(x, y, pw, iw, how, softmax, part, out, coef)
        bwd(x, y, pw, coef, gs, how, softmax, dl)
        torch.cuda.synchronize()
        used = part.view(-1)[:n * rows * k].view(n, rows, k)[:, :, :k0]
        got.append(dict(part=used, out=out[:4 + c], coef=coef[:n * c * 2 + 2].clone(), dlogits=dl))
    coef[:n * c * 2 + 2] = got[0]["coef"]                  # the second family's backward on the first family's coefficients
    dl_same = torch.zeros_like(x)
    ops.seg_loss_ext_bwd(x, y, pw, coef, gs, cfg, softmax, dl_same)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(dl_same), _bits(got[0]["dlogits"])), "equal coefficients, different gradient bits"
    known = DIFFERED_BEFORE.get((ncv, softmax, weighted), {})
    differ = {name: _bits(got[0][name]) != _bits(got[1][name]) for name in got[0]}
    print("%s sm=%d w=%d: entries that differ %s" % (key, softmax, weighted, {k: int(m.sum()) for k, m in differ.items()}))
    for name in ("part", "out", "coef"):
        allowed = np.zeros_like(differ[name])
        for i in known.get(name, ()):
            allowed[i] = True
        assert not (differ[name] & ~allowed).any(), (name, np.argwhere(differ[name] & ~allowed)[:8].tolist())
    # from its own coefficients: bitwise unless a coefficient differs, then (as every listed entry) within the float64 bound
    assert not differ["dlogits"].any() or differ["coef"].any(), np.argwhere(differ["dlogits"])[:8].tolist()
    if known:
        r = LO.reference(xh, yh, pwh, iwh, terms, softmax, gscale=0.7)
        for side, t in zip(("first family", "second family"), got):
            res = LO.check_B(r, out=t["out"].cpu().numpy(), dl=t["dlogits"].cpu().numpy(),
                             sm=t["part"].double().sum(1).cpu().numpy(), what="%s %s" % (key, side))
            print("   %s: error / bound %s" % (side, {k: "%.3g" % q for k, q in res.items()}))
