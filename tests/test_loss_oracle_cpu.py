"""CPU self-tests of the loss oracles (tests/lossoracle.py): the fp32 numpy restatement of the loss kernels (their
operation order: partial rows in fp32, the rows in double, coefficients rounded to float) passes the exact oracle A and the
rounding oracle B, the closed-form float64 gradient equals autograd, the exact-data generators meet their own preconditions, and
each of these injected defects fails B by at least a factor 10 (and A where it touches the exact sums):

- ce_999       the CE gradient without its 0.999 factor;
- ent_eps      1e-6 in place of 1e-10 in the entropy term;
- last_max     the hard metric takes the last maximum instead of the first (seen on tied outputs);
- pw_missing   the pixel weight left out of the P sum;
- img_div_n    the image-weighted Dice divided by the local N instead of n_global;
- ce_norm_eps  ce_norm without the + 1e-5 (seen where the weights sum to little);
- drop_voxel   one voxel dropped at the end of a row;
- row_twice    one row partial counted twice.

Not listed, because not detectable: the p / ((p + 1e-10) ln 2) part of the entropy gradient cancels under the softmax Jacobian
(lossoracle's docstring)."""
import numpy as np
import pytest

import lossoracle as O

TERMS = (0.5, 0.3, 0.7, 0.2)
FACTOR = 10.0


def _real_case(softmax=True, small_weight=False):
    n, c, v = 4, 3, 5000
    lg = O.real_logits("cpu.lg", n, c, v, 2.0, gap=30.0, ties=0.05) if softmax else O.real_probs("cpu.p", n, c, v)
    y = O.hard_labels("cpu.y", n, c, v)
    pw = O.rng("cpu.w").random((n, v)).astype(np.float32)
    if small_weight:
        pw[:] = 0
        pw[:, 17] = np.float32(2.0 ** -9)
    iw = np.asarray([0.8, 0.45, 0.3, 1.0], np.float32)
    return lg, y, pw, iw


def _worst(r, sm, outs, dl, iw, shards):
    n = dl.shape[0]
    per = n // shards
    res = [O.ratio(dl, r.dl, r.dl_bound), O.ratio(sm, r.sums, r.sums_bound)]
    for i, o in enumerate(outs):
        res.append(O.ratio(o, O.rank_out_ref(r, slice(i * per, (i + 1) * per), iw, TERMS, True), r.out_bound))
    return max(res)


@pytest.mark.parametrize("softmax", [True, False])
@pytest.mark.parametrize("shards", [1, 2])
def test_restatement_passes_B(softmax, shards):
    lg, y, pw, iw = _real_case(softmax)
    r = O.reference(lg, y, pw, iw, TERMS, softmax, 0.5)
    sm, tot, outs, dl = O.restate(lg, y, pw, iw, TERMS, softmax, 0.5, shards=shards)
    w = _worst(r, sm, outs, dl, iw, shards)
    print("restatement softmax=%d shards=%d: worst error / bound %.3g (gamma %.0f u)" % (softmax, shards, w, r.gamma_units))
    assert w <= 1.0
    if shards == 1:
        O.check_B(r, outs[0], dl, sm, "restatement")


@pytest.mark.parametrize("scale", [0.01, 8.0, 20.0, 60.0])
@pytest.mark.parametrize("c", [2, 5])
def test_restatement_passes_B_over_logit_scales(c, scale):
    """at scales of 20 and more p underflows in fp32: only the additive underflow term keeps the bound sound there"""
    n, v = 2, 3001
    lg = O.real_logits("cpu.s%d.%g" % (c, scale), n, c, v, scale)
    y = O.soft_labels("cpu.sy", n, c, v)
    pw = O.exact_weights("cpu.sw", n, v)
    iw = np.asarray([0.6, 1.0], np.float32)
    r = O.reference(lg, y, pw, iw, TERMS, True, -2.0)
    sm, tot, outs, dl = O.restate(lg, y, pw, iw, TERMS, True, -2.0)
    O.check_B(r, outs[0], dl, sm, "scale %g" % scale)


@pytest.mark.parametrize("mut", O.MUTATIONS)
def test_mutation_fails_B(mut):
    shards = 2 if mut == "img_div_n" else 1
    lg, y, pw, iw = _real_case(True, small_weight=(mut == "ce_norm_eps"))
    r = O.reference(lg, y, pw, iw, TERMS, True, 0.5)
    sm, tot, outs, dl = O.restate(lg, y, pw, iw, TERMS, True, 0.5, shards=shards)
    assert _worst(r, sm, outs, dl, iw, shards) <= 1.0                  # the same case without the defect passes
    sm, tot, outs, dl = O.restate(lg, y, pw, iw, TERMS, True, 0.5, mut=mut, shards=shards)
    w = _worst(r, sm, outs, dl, iw, shards)
    print("mutation %s: worst error / bound %.3g" % (mut, w))
    assert w >= FACTOR, (mut, w)


def _exact_case(softmax, c=4, v=4097 * 3):
    n = 2
    lg = O.exact_logits("cpu.xl", n, c, v) if softmax else O.exact_probs("cpu.xp", n, c, v)
    return lg, O.hard_labels("cpu.xy", n, c, v), O.exact_weights("cpu.xw", n, v)


@pytest.mark.parametrize("softmax", [True, False])
def test_restatement_passes_A(softmax):
    lg, y, pw = _exact_case(softmax)
    sm, tot, outs, dl = O.restate(lg, y, pw, None, (1.0, 0.0, 0.0, 0.0), softmax)
    assert O.check_A(sm, tot, outs[0], lg, y, pw, softmax) == 2 * (6 * 4 + 1)


@pytest.mark.parametrize("mut", ["last_max", "pw_missing", "drop_voxel", "row_twice"])
def test_mutation_fails_A(mut):
    lg, y, pw = _exact_case(True)
    sm, tot, outs, dl = O.restate(lg, y, pw, None, (1.0, 0.0, 0.0, 0.0), True, mut=mut)
    with pytest.raises(AssertionError):
        O.check_A(sm, tot, outs[0], lg, y, pw, True)


def test_exact_generators_meet_their_preconditions():
    for c in range(1, 9):
        for v in (1, 63, 4097, 99991):
            O.exact_pre(O.exact_logits("pre", 2, c, v), O.hard_labels("prey", 2, c, v), O.exact_weights("prew", 2, v), True)
            O.exact_pre(O.exact_probs("prep", 2, c, v), O.hard_labels("prey", 2, c, v), None, False)
    assert O.row_terms(2457600) == 19 * 256 and O.row_terms(2048000) == 4096 and O.loss_rows(2457600) == 512
    # a precondition that does not hold is reported, not assumed: thirds are not exact
    bad = np.zeros((1, 3, 8), np.float32)
    with pytest.raises(AssertionError):
        O.exact_pre(bad, O.hard_labels("prey", 1, 3, 8), None, True)
    # exact probabilities: numpy's fp32 softmax gives exactly 1 / k and 0 on the generator's logits
    lg = O.exact_logits("prob", 3, 8, 1000)
    p = O.N.softmax(lg, 1)
    k = (lg == 0).sum(1, keepdims=True)
    assert np.array_equal(p, np.where(lg == 0, np.float32(1) / k.astype(np.float32), np.float32(0)))


@pytest.mark.parametrize("softmax", [True, False])
@pytest.mark.parametrize("weights", ["none", "fractional", "zero_sample", "zero_batch"])
def test_closed_form_gradient_equals_autograd(softmax, weights):
    """`reference` asserts the agreement (values 1e-11 relative, gradient 1e-11 of the un-cancelled magnitude) - here over soft
    labels, an absent class, zero weights for a sample and for the whole batch, both softmax settings"""
    n, c, v = 3, 4, 700
    lg = O.real_logits("ag.l", n, c, v, 3.0, gap=90.0, ties=0.02) if softmax else O.real_probs("ag.p", n, c, v)
    pw = None
    if weights != "none":
        pw = O.rng("ag.w").random((n, v)).astype(np.float32)
        if weights == "zero_sample":
            pw[1] = 0
        if weights == "zero_batch":
            pw[:] = 0
    iw = np.asarray([0.2, 1.0, 0.5], np.float32)
    for y in (O.soft_labels("ag.y", n, c, v), O.hard_labels("ag.y", n, c, v, absent=2)):
        terms = (0.5, 0.3, 0.0 if pw is None else 0.7, 0.2)
        r = O.reference(lg, y, pw, iw, terms, softmax, -2.0)
        assert np.isfinite(r.out).all() and np.isfinite(r.dl).all() and np.isfinite(r.dl_bound).all()


def test_adam_and_filter_references():
    """the float64 Adam step is AdamRef's; the float64 filter agrees with oracle/np_ref.fpl_filter on exact-probability data"""
    import torch
    from oracle import torch_ref as R
    g = O.rng("adam")
    p0, gr = g.standard_normal(1000).astype(np.float32), g.standard_normal(1000).astype(np.float32)
    prm = {"w": torch.from_numpy(p0.astype(np.float64)).requires_grad_(True)}
    opt = R.AdamRef(prm, float(np.float32(1e-3)), float(np.float32(1e-5)))
    m, v = np.zeros(1000), np.zeros(1000)
    p = p0.astype(np.float64)
    for step in range(1, 4):
        prm["w"].grad = torch.from_numpy(gr.astype(np.float64))
        opt.step()
        p, m, v = O.adam_ref(p, gr, m, v, 1e-3, step, 1e-5)[:3]
        # AdamRef uses the double constants 0.9 / 0.999, the kernel receives floats: equal to the constants' rounding
        assert np.allclose(prm["w"].detach().numpy(), p, rtol=0, atol=1e-9), step
    for t in (1, 2, 4, 7):
        st = O.exact_logits("flt", t, 3, 1021).reshape(t, 3, 1021)
        ref, f = O.filter_exact_vars(st)
        fr = O.filter_ref(st)
        assert np.array_equal(fr["hards"], f["hards"].reshape(t, -1))
        assert abs(fr["vars"] - ref) <= fr["vars_bound"] + 1e-12 * ref
        assert np.abs(fr["means"] - f["means"].reshape(-1)).max() <= 2.0 ** -24
