"""The exact oracle A and the rounding oracle B of tests/lossoracle.py applied to the loss, filter, hard-label and Adam kernels
through the C ABI (fplx.ops; ops.call for fplx_seg_loss_sums / fplx_seg_loss_from_sums).  Every case prints its worst error / bound
ratio; with FPLX_RATIO_LOG=<file> the same lines are written there (profiles/loss_oracle_ratios.txt is such a run)."""
import os

import numpy as np
import pytest
import torch

import lossoracle as O

pytestmark = pytest.mark.gpu

V_SMALL = (1, 63, 255, 257, 4095, 4096, 4097)
V_PRIME = 99991
V_BENCH = 80 * 160 * 160            # 2 048 000: the benchmark volume, just under the 512-row cap
V_OVER = 96 * 160 * 160             # 2 457 600: above it (grid-stride rows)
NS = (1, 2, 3, 5)
GSCALES = (1.0, 0.5, -2.0)
GAPS = (0.0, 1e-3, 30.0, 90.0, 200.0)
ALONE = ((1.0, 0.0, 0.0, 0.0), (0.0, 1.0, 0.0, 0.0), (0.0, 0.0, 1.0, 0.0), (0.0, 0.0, 0.0, 1.0))
ALL4 = (0.5, 0.3, 0.7, 0.2)
WEIGHTS = ("none", "fractional", "zero_sample", "zero_batch")
LABELS = ("onehot", "soft", "absent")
POISON = -777.0
_LINES = []


@pytest.fixture(scope="module", autouse=True)
def _ratio_log():
    yield
    path = os.environ.get("FPLX_RATIO_LOG")
    if path and _LINES:
        with open(path, "a") as f:
            f.write("\n".join(_LINES) + "\n")


def _log(case, res):
    line = "%-72s %s" % (case, "  ".join("%s %.3g" % kv for kv in sorted(res.items())))
    print(line)
    _LINES.append(line)


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _dev(lg, y, pw, iw, terms, softmax, gscale, shards=1):
    """the loss through the C ABI: fplx_seg_loss_sums per rank, totals added on the host in float64, fplx_seg_loss_from_sums,
    fplx_seg_loss_bwd; `part` is exactly the documented N x fplx_loss_rows x K floats with poison behind.  With one rank
    fplx_seg_loss_fwd on a second such buffer must give the same out / coef bits.  -> sums, totals, [out per rank], dlogits"""
    from fplx import ops
    n, c, v = lg.shape
    per, k, sm = n // shards, 6 * c + 3, 1 if softmax else 0
    need = per * ops.loss_rows(v) * k
    assert ops.loss_rows(v) == O.loss_rows(v) + 5
    ranks = []
    for i in range(shards):
        s = slice(i * per, (i + 1) * per)
        L, Y, W = _cuda(lg[s]), _cuda(y[s]), _cuda(None if pw is None else pw[s])
        IW = _cuda(None if iw is None else iw[s])
        arena = torch.full((need + 256,), POISON, dtype=torch.float32, device="cuda")
        sums = torch.full((per + 1, k), float("nan"), dtype=torch.float64, device="cuda")
        ops.call("fplx_seg_loss_sums", ops.ptr(L), ops.ptr(Y), ops.ptr(W), per, c, v, sm, ops.ptr(arena[:need]), ops.ptr(sums[:per]),
                 ops.ptr(sums[per]), ops.stream())
        ranks.append((L, Y, W, IW, arena, sums))
    torch.cuda.synchronize()
    totals = np.sum([r[5][per].cpu().numpy() for r in ranks], axis=0)                 # float64 on the host
    tot_dev = _cuda(totals)
    gs = torch.tensor([gscale], dtype=torch.float32, device="cuda")
    outs, dls, all_sums = [], [], []
    for (L, Y, W, IW, arena, sums) in ranks:
        out = torch.full((4 + c,), float("nan"), dtype=torch.float32, device="cuda")
        coef = torch.full((per * c * 2 + 2,), float("nan"), dtype=torch.float32, device="cuda")
        ops.call("fplx_seg_loss_from_sums", ops.ptr(sums[:per]), ops.ptr(tot_dev), ops.ptr(IW), per, n, c, v, 0 if W is None else 1,
                 terms[0], terms[1], terms[2], terms[3], ops.ptr(out), ops.ptr(coef), ops.stream())
        dl = torch.full_like(L, float("nan"))
        ops.seg_loss_bwd(L, Y, W, coef, gs, terms, softmax, dl)
        torch.cuda.synchronize()
        assert bool((arena[need:] == POISON).all()), "fplx_seg_loss_sums wrote behind N x fplx_loss_rows x K"
        if shards == 1:
            arena2 = torch.full((need + 256,), POISON, dtype=torch.float32, device="cuda")
            out2, coef2 = torch.empty_like(out), torch.empty_like(coef)
            ops.seg_loss_fwd(L, Y, W, IW if terms[2] != 0 else None, terms, softmax, arena2[:need], out2, coef2)
            torch.cuda.synchronize()
            assert bool((arena2[need:] == POISON).all()), "fplx_seg_loss_fwd wrote behind N x fplx_loss_rows x K"
            assert torch.equal(out2, out) and torch.equal(coef2, coef), "fplx_seg_loss_fwd != sums + from_sums"
        outs.append(out.cpu().numpy().astype(np.float64))
        dls.append(dl.cpu().numpy().astype(np.float64))
        all_sums.append(sums[:per].cpu().numpy())
    return np.concatenate(all_sums), totals, outs, np.concatenate(dls)


def _weights(kind, key, n, v, exact):
    if kind == "none":
        return None
    pw = O.exact_weights(key, n, v) if exact else O.rng(key).random((n, v)).astype(np.float32)
    if kind == "zero_sample":
        pw[n // 2] = 0
    if kind == "zero_batch":
        pw[:] = 0
    return pw


def _absent(lg, cls, softmax):
    """class `cls` (the last one) absent from the predictions as well: its probability is 0 everywhere (a logit of -200 below the
    others' minimum, which fp32 softmax turns into exactly 0), so the Dice epsilon alone decides its ratio"""
    if cls is None:
        return lg
    n, c, v = lg.shape
    if not softmax:
        lg = lg.copy()
        lg[:, cls] = 0
        return lg
    if cls == c:                                                          # exact logits generated for the other classes
        return np.ascontiguousarray(np.concatenate([lg, np.full((n, 1, v), -200.0, np.float32)], 1))
    lg = lg.copy()
    lg[:, cls] = lg[:, :cls].min(1) - np.float32(200.0)
    return lg


def _vs(c):
    return V_SMALL + ((V_PRIME,) if c <= 6 else ())


# ---------------------------------------------------------------- A

@pytest.mark.parametrize("softmax", [1, 0])
@pytest.mark.parametrize("c", range(1, 9))
def test_loss_sums_exact(c, softmax):
    """oracle A: the 6C + 1 exact entries of sums / totals bit for bit, out[4..] = float32(float64 hard-class Dice)"""
    for i, v in enumerate(_vs(c)):
        n = NS[(i + c) % 4]
        kind = WEIGHTS[(i + c + softmax) % 4]
        key = "A.%d.%d.%d" % (c, softmax, v)
        absent = c - 1 if (i % 3 == 0 and c > 1) else None
        lg = _absent(O.exact_logits(key, n, c - (absent is not None), v) if softmax else O.exact_probs(key, n, c, v), absent, softmax)
        y = O.hard_labels(key + "y", n, c, v, absent=absent)
        pw = _weights(kind, key + "w", n, v, True)
        sm, tot, outs, dl = _dev(lg, y, pw, None, ALONE[0], bool(softmax), 1.0)
        cnt = O.check_A(sm, tot, outs[0], lg, y, pw, bool(softmax), key)
        assert np.isfinite(dl).all()
        _log("A c=%d softmax=%d v=%d n=%d pw=%s" % (c, softmax, v, n, kind), {"exact_entries": cnt})


@pytest.mark.parametrize("v", [V_BENCH, V_OVER])
def test_loss_sums_exact_full_size(v):
    for softmax in (True, False):
        key = "A.full.%d.%d" % (v, softmax)
        lg = O.exact_logits(key, 1, 2, v) if softmax else O.exact_probs(key, 1, 2, v)
        y, pw = O.hard_labels(key + "y", 1, 2, v), O.exact_weights(key + "w", 1, v)
        sm, tot, outs, dl = _dev(lg, y, pw, None, ALONE[0], softmax, 1.0)
        cnt = O.check_A(sm, tot, outs[0], lg, y, pw, softmax, key)
        _log("A c=2 softmax=%d v=%d n=1 pw=fractional" % (softmax, v), {"exact_entries": cnt})


# ---------------------------------------------------------------- B

def _labels(kind, key, n, c, v):
    if kind == "soft":
        return O.soft_labels(key, n, c, v)
    return O.hard_labels(key, n, c, v, absent=(c - 1 if kind == "absent" else None))


def _b_case(tag, lg, y, pw, iw, terms, softmax, gscale, shards=1):
    if pw is None or iw is None:
        terms = (terms[0], terms[1], 0.0, terms[3])
    r = O.reference(lg, y, pw, iw, terms, softmax, gscale)
    sm, tot, outs, dl = _dev(lg, y, pw, iw, terms, softmax, gscale, shards)
    per = lg.shape[0] // shards
    res = {"dlogits": O.ratio(dl, r.dl, r.dl_bound), "sums": O.ratio(sm, r.sums, r.sums_bound), "out": 0.0}
    for i, o in enumerate(outs):
        want = r.out if shards == 1 else O.rank_out_ref(r, slice(i * per, (i + 1) * per), iw, terms, pw is not None)
        res["out"] = max(res["out"], O.ratio(o, want, r.out_bound))
    _log(tag, res)
    assert all(x <= 1.0 for x in res.values()), (tag, res)
    return res


@pytest.mark.parametrize("softmax", [1, 0])
@pytest.mark.parametrize("c", range(1, 9))
def test_loss_rounding_bound(c, softmax):
    """oracle B over the voxel counts, batch sizes, term sets, gradient scales, weights, labels and logit gaps; with zero weights
    for a sample or the whole batch loss and gradient must stay finite and equal to float64 (a NaN is an infinite ratio)"""
    j = 0
    for i, v in enumerate(_vs(c)):
        for terms in (ALONE[(i + c) % 4], ALL4):
            j += 1
            n, gsc = NS[(j + c) % 4], GSCALES[(j + softmax) % 3]
            kind, lab, gap = WEIGHTS[(j + 2 * c) % 4], LABELS[j % 3], GAPS[(j + c) % 5]
            if terms[2] != 0 and terms[0] == 0 and kind == "none":
                kind = "fractional"                                      # the image-weighted Dice alone needs weights
            key = "B.%d.%d.%d.%d" % (c, softmax, v, j)
            lg = O.real_logits(key, n, c, v, 2.0, gap=gap, ties=0.05 if gap == 0 else 0.0) if softmax else O.real_probs(key, n, c, v)
            lg = _absent(lg, c - 1 if (lab == "absent" and c > 1) else None, softmax)
            y, pw = _labels(lab, key + "y", n, c, v), _weights(kind, key + "w", n, v, False)
            iw = None if pw is None else (0.1 + O.rng(key + "i").random(n)).astype(np.float32)
            _b_case("B c=%d softmax=%d v=%d n=%d terms=%s gs=%g pw=%s y=%s gap=%g" % (c, softmax, v, n, terms, gsc, kind, lab, gap),
                    lg, y, pw, iw, terms, bool(softmax), gsc)


@pytest.mark.parametrize("v,softmax", [(V_BENCH, True), (V_OVER, True), (V_OVER, False)])
def test_loss_rounding_bound_full_size(v, softmax):
    key = "B.full.%d.%d" % (v, softmax)
    lg = O.real_logits(key, 1, 2, v, 3.0, gap=30.0) if softmax else O.real_probs(key, 1, 2, v)
    y, pw = O.hard_labels(key + "y", 1, 2, v), O.rng(key + "w").random((1, v)).astype(np.float32)
    _b_case("B c=2 softmax=%d v=%d n=1 terms=%s gs=0.5 pw=fractional y=onehot gap=30" % (softmax, v, ALL4), lg, y, pw,
            np.asarray([0.8], np.float32), ALL4, softmax, 0.5)


@pytest.mark.parametrize("softmax", [True, False])
def test_entropy_term_follows_the_reference_softmax(softmax):
    """the entropy regulariser applies softmax to the outputs whatever loss_softmax says (agent_seg.py:353): with softmax = 0 and
    an entropy weight, alone and next to the other terms, loss and gradient are the float64 reference's"""
    for c, v in ((2, 4097), (3, 257), (8, 63)):
        key = "ent.%d.%d" % (c, softmax)
        lg = O.real_logits(key, 2, c, v, 2.0, gap=30.0) if softmax else O.real_probs(key, 2, c, v)
        y, pw = O.hard_labels(key + "y", 2, c, v), O.rng(key + "w").random((2, v)).astype(np.float32)
        for terms in ((0.0, 0.0, 0.0, 1.0), (0.5, 0.0, 0.7, 0.2)):
            res = _b_case("entropy c=%d softmax=%d v=%d terms=%s" % (c, softmax, v, terms), lg, y, pw, np.asarray([0.8, 0.4], np.float32),
                          terms, softmax, 1.0)
            assert np.isfinite(list(res.values())).all()


@pytest.mark.parametrize("c,shards", [(2, 2), (3, 3)])
def test_loss_split_path_adds_up_to_the_full_batch(c, shards):
    """shards of unequal content, n_global = 2n and 3n, totals added on the host in float64, all four terms with image weights: the
    ranks' gradients are the float64 full-batch gradient within B, each rank's out its share"""
    per, v = 2, 3 * 4096 + 77
    n = per * shards
    key = "split.%d.%d" % (c, shards)
    lg = O.real_logits(key, n, c, v, 2.0, gap=30.0)
    lg[per:] *= np.float32(0.25)                                        # the ranks see different content
    y = O.soft_labels(key + "y", n, c, v)
    pw = O.rng(key + "w").random((n, v)).astype(np.float32)
    pw[1] = 0
    iw = (0.1 + O.rng(key + "i").random(n)).astype(np.float32)
    _b_case("split c=%d ranks=%d n_global=%d v=%d terms=%s" % (c, shards, n, v, ALL4), lg, y, pw, iw, ALL4, True, 0.5, shards)


def test_loss_refusals():
    from fplx import ops, _lib
    err = (ValueError, _lib.FplxError)
    v = 64
    buf = torch.zeros(65 * 9 * 2 * v, dtype=torch.float32, device="cuda")
    part = torch.zeros(65 * ops.loss_rows(v) * ops.loss_k(8), dtype=torch.float32, device="cuda")
    out, coef = torch.zeros(16, device="cuda"), torch.zeros(65 * 9 * 2 + 2, device="cuda")
    dsum = torch.zeros((66, ops.loss_k(8)), dtype=torch.float64, device="cuda")

    def fwd(n, c, pw=0, iw=0, wi=0.0):
        ops.call("fplx_seg_loss_fwd", ops.ptr(buf), ops.ptr(buf), pw, iw, n, c, v, 1.0, 0.0, wi, 0.0, 1, ops.ptr(part), ops.ptr(out),
                 ops.ptr(coef), ops.stream())
    for n, c in ((1, 0), (1, 9), (65, 2)):
        with pytest.raises(err):
            fwd(n, c)
        with pytest.raises(err):
            ops.call("fplx_seg_loss_sums", ops.ptr(buf), ops.ptr(buf), 0, n, c, v, 1, ops.ptr(part), ops.ptr(dsum), ops.ptr(dsum[65]),
                     ops.stream())
        with pytest.raises(err):
            ops.call("fplx_seg_loss_from_sums", ops.ptr(dsum), ops.ptr(dsum[65]), 0, n, n, c, v, 0, 1.0, 0.0, 0.0, 0.0, ops.ptr(out),
                     ops.ptr(coef), ops.stream())
        with pytest.raises(err):
            ops.call("fplx_seg_loss_bwd", ops.ptr(buf), ops.ptr(buf), 0, ops.ptr(coef), ops.ptr(out), n, c, v, 1.0, 0.0, 0.0, 0.0, 1,
                     ops.ptr(buf), ops.stream())
    for pw, iw in ((0, 0), (ops.ptr(buf), 0), (0, ops.ptr(buf))):        # w_dice_img without image or pixel weights
        with pytest.raises(err):
            fwd(2, 2, pw, iw, 0.5)
    with pytest.raises(err):
        ops.call("fplx_seg_loss_from_sums", ops.ptr(dsum), ops.ptr(dsum[65]), 0, 2, 2, 2, v, 1, 1.0, 0.0, 0.5, 0.0, ops.ptr(out),
                 ops.ptr(coef), ops.stream())
    fwd(2, 2, ops.ptr(buf), ops.ptr(buf), 0.5)                            # and the complete call is accepted
    torch.cuda.synchronize()


# ---------------------------------------------------------------- mc_filter

MC_V = (4, 1020, 1021, 65536 + 4)


def _mc(stack, misalign):
    from fplx import ops
    t = torch.from_numpy(stack).cuda()
    if misalign:
        flat = torch.zeros(stack.size + 1, dtype=torch.float32, device="cuda")
        flat[1:] = t.reshape(-1)
        t = flat[1:].view(stack.shape)
        assert t.data_ptr() % 16 == 4
    r = ops.mc_filter(t, 0.01, True, True)
    torch.cuda.synchronize()
    return {k: x.cpu().numpy() for k, x in r.items()}


@pytest.mark.parametrize("T", [1, 2, 3, 4, 7, 15, 16])
@pytest.mark.parametrize("c", [2, 3, 4])
def test_mc_filter_against_numpy_and_float64(c, T):
    from oracle import np_ref as N
    for v in MC_V:
        for misalign in (False, True):
            # exact probabilities: hards, means bit for bit, boundary exact, vars exact terms (T a power of two) or within the bound
            st = O.exact_logits("mc.%d.%d.%d" % (c, T, v), T, c, v).reshape(T, c, v)
            got = _mc(st, misalign)
            want_vars, f = O.filter_exact_vars(st)
            fr = O.filter_ref(st)
            assert np.array_equal(got["hards"], f["hards"].reshape(T, v))
            assert np.array_equal(got["means"], f["means"].reshape(v))
            assert int(got["stats"][1]) == f["boundary"]
            assert np.abs(got["uncertainty"] - f["uncertainty"].reshape(v)).max() <= 2e-7
            if T & (T - 1) == 0:
                assert abs(got["stats"][0] - want_vars) <= 1e-12 * want_vars
            r_exact = abs(got["stats"][0] - fr["vars"]) / fr["vars_bound"]
            uo = 1.0 if f["boundary"] < 50 else float(np.float32(got["stats"][0])) / f["boundary"]
            assert got["stats"][2] == uo
            # random logits (top two at least 1e-3 apart) against the float64 restatement
            st = O.separated_logits("mcr.%d.%d.%d" % (c, T, v), (T, c, v), 2.5)
            got = _mc(st, misalign)
            fr = O.filter_ref(st)
            assert np.array_equal(got["hards"], fr["hards"])
            res = {"vars_exact_data": r_exact, "vars": abs(got["stats"][0] - fr["vars"]) / fr["vars_bound"],
                   "means": O.ratio(got["means"], fr["means"], fr["means_bound"])}
            f = N.fpl_filter(st.reshape(T, c, 1, 1, v))
            assert np.array_equal(got["hards"], f["hards"].reshape(T, v)) and int(got["stats"][1]) == f["boundary"]
            assert np.abs(got["uncertainty"] - f["uncertainty"].reshape(v)).max() <= 2e-7
            _log("mc_filter c=%d T=%d v=%d misaligned=%d" % (c, T, v, misalign), res)
            assert all(x <= 1.0 for x in res.values()), res


def test_mc_filter_refusals():
    from fplx import ops, _lib
    for t, c in ((17, 2), (4, 5), (4, 1), (17, 5)):
        with pytest.raises((ValueError, _lib.FplxError)):
            ops.mc_filter(torch.zeros((t, c, 64), device="cuda"), 0.01)


# ---------------------------------------------------------------- hard_label

@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("c", range(1, 9))
def test_hard_label_against_numpy(c, n):
    from fplx import ops
    from oracle import np_ref as N
    for v in _vs(c) + ((V_OVER,) if (c, n) == (2, 1) else ()):
        lg = O.exact_logits("hl.%d.%d" % (c, v), n, c, v)             # ties everywhere: the first class of the tied maxima
        got = ops.hard_label(_cuda(lg)).cpu().numpy()
        assert np.array_equal(got, N.hard_label(lg)) and np.array_equal(got, lg.argmax(1))
        lg = O.separated_logits("hlr.%d.%d" % (c, v), (n, c, v), 2.0)
        assert np.array_equal(ops.hard_label(_cuda(lg)).cpu().numpy(), N.hard_label(lg))


# ---------------------------------------------------------------- Adam

def _place(a, mode):
    """a on the device at a 16-byte-aligned base ('a') or one float behind one ('o')"""
    buf = torch.zeros(a.size + 8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    off = 1 if mode == "o" else 0
    v = buf[off:off + a.size]
    v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return v


def _adam_case(n, steps, gscale, wd, zero=False, modes="aaaa"):
    """modes: placement of p, g, m, v - 'aaaa' the 16-byte body, 'oooo' scalar head + body + tail, 'oaoo' (p and g on different
    alignments) the all-scalar kernel"""
    from fplx import ops
    g = O.rng("adam.%d.%g.%g" % (n, gscale, wd))
    p = _place(g.standard_normal(n).astype(np.float32), modes[0])
    m = _place(np.zeros(n, np.float32), modes[2])
    v = _place(np.zeros(n, np.float32), modes[3])
    if steps[0] > 1 and not zero:                                       # a state as it is late in training
        m.copy_(torch.from_numpy((g.standard_normal(n) * 1e-2).astype(np.float32)))
        v.copy_(torch.from_numpy((g.random(n) * 1e-4).astype(np.float32)))
    worst = {}
    for step in steps:
        gr = np.zeros(n, np.float32) if zero else (g.standard_normal(n) * 10.0 ** g.integers(-6, 1)).astype(np.float32)
        gd = _place(gr, modes[1])
        before = [t.cpu().numpy() for t in (p, m, v)]
        ops.adam_step(p, gd, m, v, 1e-3, step, wd, gscale)
        torch.cuda.synchronize()
        p2, m2, v2, bp, bm, bv = O.adam_ref(before[0], gr, before[1], before[2], 1e-3, step, wd, gscale)
        res = {"p": O.ratio(p.cpu().numpy(), p2, bp), "m": O.ratio(m.cpu().numpy(), m2, bm), "v": O.ratio(v.cpu().numpy(), v2, bv)}
        if zero and wd == 0:
            assert np.array_equal(p.cpu().numpy(), before[0]) and not m.any() and not v.any()
        for k, x in res.items():
            worst[k] = max(worst.get(k, 0.0), x)
    _log("adam n=%d steps=%s grad_scale=%g wd=%g zero=%d %s" % (n, list(steps), gscale, wd, zero, modes), worst)
    assert all(x <= 1.0 for x in worst.values()), worst


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 10007])
def test_adam_step_against_float64(n):
    for modes in ("aaaa", "oooo", "oaoo"):
        for gscale in (1.0, 0.125):
            for wd in (0.0, 1e-5):
                _adam_case(n, (1, 2, 3, 4, 5), gscale, wd, modes=modes)
                _adam_case(n, (1000, 100000), gscale, wd, modes=modes)
        _adam_case(n, (1, 2), 1.0, 0.0, zero=True, modes=modes)
        _adam_case(n, (1, 1000), 0.125, 1e-5, zero=True, modes=modes)


def test_adam_step_against_float64_full_size():
    _adam_case(22600000, (1, 1000), 0.125, 1e-5)
