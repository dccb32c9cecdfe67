"""Float64 oracles for the semi-supervised kernels (fpl-plus_amd/csrc/ssl.hip), on top of tests/lossoracle.py: same two oracles,
same notation (u = 2^-24, ETA, E_EXP, E_LOG, dp(D), ra, GAMMA_SLACK) and NO new measured constant.

The passes under test.  Logits [N, C, V]; p = softmax(student), q = softmax(teacher) (softmax = 0: the inputs themselves).
    consistency   k_v = 1 (MeanTeacher, t = 0) or [unc_v < thr] with m_c = (sum_t softmax(mc_t)_c) / T, unc = -sum_c m_c log(m_c + 1e-6)
                  out0 = sum_v k_v sum_c (p_c - q_c)^2, out1 = sum_v k_v, loss = out0 / (N C V) (t = 0) or out0 / (2 out1 + 1e-16)
                  dstudent_c = gs p_c (e_c - sum_j p_j e_j), e_c = 2 (p_c - q_c) k / D        (softmax = 0: gs e_c)
    entropy       p' = 0.999 p + 5e-4, out0 = sum_v -sum_c p'_c ln p'_c, loss = out0 / (ln C N V)
                  dlogits_c = gs p_c (g_c - sum_j p_j g_j), g_c = -0.999 (ln p'_c + 1) / (ln C N V)    (softmax = 0: gs g_c)
    ema           e' = alpha e + (1 - alpha) p
The float64 closed forms below are asserted in every call against float64 autograd of the reference's own statements written
with torch operations (ssl_mt.py:90-100, ssl_uamt.py:77-100, loss/seg/ssl.py:40-43), 1e-11 of the magnitude.

Partial rows.  A block of 256 lanes takes the voxels (scalar form) or the quads of four voxels (V a multiple of 4) that fall
to it; a lane adds its at most ceil(V / (256 rows)) + 3 terms one after the other (the + 3: a lane's last quad is added whole), then
6 shuffles and 3 additions in LDS: ra' = ra + 3 additions between a voxel's term and its row, ra = ROW_TERMS / 256 + 9 as in
lossoracle.  The rows are added in double (exact next to u).

A - exact part.  softmax = 0 with p, q multiples of 2^-6: p - q is exact, (p - q)^2 a multiple of 2^-12, and while a sample's sum of
    them in that unit stays below 2^24 (asserted on the data, `exact_pre`) every partial sum is exact in fp32 in any order: out0
    and out1 equal the float64 values bit for bit.  The mask goes through logf; the exact cases keep every voxel's uncertainty
    far from the threshold (no undecided voxel, asserted).  EMA with alpha = 3/4 and multiples of 2^-10 below 4 in magnitude:
    every product and the sum are multiples of 2^-12 below 8 - exact.
B - rounding part.  With D = max - min of a voxel's logits, dp(D) = 2 D + 4 E_EXP + C + 1 [u] is the relative error of a probability
    (lossoracle), ep = dp u p its absolute error (0 with softmax = 0).
    squared error   d = p - q: ed = ep_p + ep_q + u |d|;  d^2: 2 |d| ed + u d^2;  the C additions: C u sum d^2.  Per voxel
                    e_sq = sum_c 2 |d_c| ed_c + (C + 1) u sq;  out0: sum_kept e_sq + ra' u sum_kept sq.
    uncertainty     m_c: em = u (sum_t dp_t p_t / T + (T + 1) m)  (T - 1 additions of positive terms, one division, the int -> float
                    of T exact);  a = m + 1e-6: ea = em + 2 u a (the constant, the addition);  log a: el = ea / a + E_LOG u |log a|;
                    m log a: em |log a| + m el + u |m log a|;  the C subtractions: C u sum |m log a|.
                    e_unc = sum_c (em |log a| + m el) + (C + 1) u sum_c |m log a| + 16 C ETA (underflow: |d unc / d m| < 16;
                    not with softmax = 0, where nothing can underflow).  A bound of 0 (a voxel whose m is 0 in every class:
                    unc = 0 exactly) means the device's value IS the float64 one: such a voxel is decided, which is what tells
                    `<` from `<=` at thr = 0.
                    A voxel with |unc - thr| <= GAMMA_SLACK e_unc is UNDECIDED: the device may keep it or not.  It is excluded
                    from the mask comparison; the bound of out0 grows by its squared error, out1 may differ by their number, and
                    the loss is bounded by interval arithmetic over both.  thr is the fp32 value the kernel receives.
    gradient        on un-cancelled magnitudes, with the device's own mask (the kept count is then exact and D is known):
                    E_c = |e_c|, ee_c = k2 ed_c + 2 u E_c (k2 = float(2 / D), the product);  S_c = |gs| p_c (E_c + sum_j p_j E_j);
                    |err| <= GAMMA_SLACK (|gs| p_c (ee_c + sum_j (p_j ee_j + dp u p_j E_j)) + (dp + C + 5) u S_c) + ETA (1 + |gs| (E_c + sum E))
                    (the dot product: C fma and the p_j again; the subtraction; x p_c, whose own error is dp u; x gs).
                    softmax = 0: 4 u |gs e_c| + ETA.
    entropy         p': epp = 0.999 ep + 4 u p' (two constants, a product, a sum - not fused);  ln p': el = epp / p' + E_LOG u |ln p'|;
                    p' ln p': epp |ln p'| + p' el + u |p' ln p'|;  per voxel e_h = sum_c (epp |ln p'| + p' el) + (C + 1) u h;
                    out0: sum e_h + ra' u sum h + 2000 N V C ETA.  Gradient as above with G_c = coef (|ln p'_c| + 1),
                    eg_c = coef el_c + 3 u G_c (the sum with 1, the product, coef's own rounding), coef = 0.999 / (ln C N V).
                    softmax = 0: |gs| (eg_c + u G_c) + ETA.
    ema             2 u |(1 - alpha) p| + u |e'|  (1 - alpha rounded once, the product, the fma) + ETA, alpha the fp32 value.
    Scalars evaluated in double from out0 / out1 by one thread: their error is out0's through the division.
    What makes a UAMT case a real test is asserted on the oracle's side before anything is compared (`check_case_is_a_real_test`):
    at most 1 % undecided voxels, and a kept share inside [0.2, 0.9] - the latter only where the case has at least 100 voxels:
    below that a share is a multiple of more than 1 % and says nothing about the data (V = 1 can only give 0 or 1).

Clamped normal (the Philox route of ssl_perturb): for z ~ N(0, 1), w = clamp(sigma z, -c, c), k = c / sigma:
    E w = 0, E w^2 = sigma^2 ((2 Phi(k) - 1) - 2 k phi(k)) + 2 c^2 (1 - Phi(k)),
    E w^4 = sigma^4 (3 (2 Phi(k) - 1) - 2 phi(k) (k^3 + 3 k)) + 2 c^4 (1 - Phi(k)).

Pure numpy / torch on the CPU; tests/test_ssl_cpu.py checks the oracle itself, tests/test_gpu_ssl.py applies it."""
import math

import numpy as np
import torch

import lossoracle as LO
from lossoracle import U, ETA, E_EXP, E_LOG, GAMMA_SLACK, ratio  # noqa: F401

EXACT_LIMIT = LO.EXACT_LIMIT
MUTATIONS = ("den_c", "unc_eps", "ent_999", "ent_lnc", "grad_swap", "drop_voxel", "row_twice", "mask_le", "ema_swap")
MAX_UNDECIDED = 0.01
KEPT_SHARE = (0.2, 0.9)


def ra_ssl(v):
    return LO.row_terms(v) / 256 + 9 + 3


# ---------------------------------------------------------------- generators

def logits_case(key, n, c, v, t):
    """the issue's inputs: base [N, C, V] * 1.5 + jitter * 0.5, both standard normal -> student, teacher [N, C, V], mc [T, N, C, V]
    (None for t = 0), float32"""
    g = LO.rng(key)
    base = g.standard_normal((n, c, v)) * 1.5
    f = lambda a: np.ascontiguousarray(a.astype(np.float32))
    student = f(base + g.standard_normal((n, c, v)) * 0.5)
    teacher = f(base + g.standard_normal((n, c, v)) * 0.5)
    mc = f(base[None] + g.standard_normal((t, n, c, v)) * 0.5) if t else None
    return student, teacher, mc


def uamt_threshold(ramp, c):
    """ssl_uamt.py:98"""
    return (0.75 + 0.25 * ramp) * np.log(c)


def exact_case(key, n, c, v, t):
    """softmax = 0 data of oracle A: student, teacher multiples of 2^-6 in [0, 1/4]; mc in {0, 1}: a voxel's passes all name one
    class (uncertainty about 0) or alternate between two (ln 2) -> student, teacher, mc, thr = 0.3"""
    g = LO.rng(key)
    student = (g.integers(0, 17, (n, c, v)) / 64.0).astype(np.float32)
    teacher = (g.integers(0, 17, (n, c, v)) / 64.0).astype(np.float32)
    mc = None
    if t:
        a = g.integers(0, c, (n, v))
        b = (a + 1 + g.integers(0, c - 1, (n, v))) % c
        split = g.random((n, v)) < 0.4
        mc = np.zeros((t, n, c, v), np.float32)
        for i in range(t):
            cls = np.where(split & (i % 2 == 1), b, a)
            np.put_along_axis(mc[i], cls[:, None, :], 1.0, 1)
    return student, teacher, mc, 0.3


def exact_pre(student, teacher):
    assert np.array_equal(student * 64, np.round(student * 64)) and np.array_equal(teacher * 64, np.round(teacher * 64))
    d = student.astype(np.float64) - teacher.astype(np.float64)
    worst = float((d * d * 4096.0).sum((1, 2)).max())
    assert worst < EXACT_LIMIT, "a sample's sum of squares reaches %g units >= 2^24" % worst
    return worst


def ema_exact_case(key, n):
    g = LO.rng(key)
    return ((g.integers(-4096, 4097, n) / 1024.0).astype(np.float32), (g.integers(-4096, 4097, n) / 1024.0).astype(np.float32))


# ---------------------------------------------------------------- float64 closed forms (dt = float32: the kernels' arithmetic, with mutations)

def _softmax(l, axis):
    m = l.max(axis, keepdims=True)
    e = np.exp(l - m)
    return e / e.sum(axis, keepdims=True)


def _row_sum(x, dt, mut):
    """[N, V] -> float64 total: exact in float64; in fp32 partial rows in fp32 (scalar form's rows), the rows in double"""
    if dt == np.float64:
        return float(x.astype(np.float64).sum())
    return float(LO._reduce(x, dt, mut if mut in ("drop_voxel", "row_twice") else None).sum())


def uncertainty(mc, softmax, dt=np.float64, mut=None):
    """-> unc [N, V]"""
    t = mc.shape[0]
    l = mc.astype(dt)
    pr = _softmax(l, 2) if softmax else l
    m = pr[0].copy()
    for i in range(1, t):
        m = m + pr[i]
    m = m / dt(t)
    eps = dt(0.0) if mut == "unc_eps" else dt(1e-6)
    with np.errstate(divide="ignore", invalid="ignore"):
        term = m * np.log(m + eps)              # without the 1e-6 a class nobody predicts gives 0 x -inf
    unc = np.zeros(m[:, 0].shape, dt)
    for k in range(m.shape[1]):
        unc = unc - term[:, k]
    return unc


def consistency_fwd(student, teacher, mc, thr, softmax, dt=np.float64, mut=None):
    """-> (out [3]: masked sum of squares, kept count, loss; mask [N, V] bool; sq [N, V]; unc [N, V] or None)"""
    n, c, v = student.shape
    s, q = student.astype(dt), teacher.astype(dt)
    p, r = (_softmax(s, 1), _softmax(q, 1)) if softmax else (s, q)
    d = p - r
    sq = np.zeros((n, v), dt)
    for k in range(c):
        sq = sq + d[:, k] * d[:, k]
    unc = None
    keep = np.ones((n, v), bool)
    if mc is not None:
        unc = uncertainty(mc, softmax, dt, mut)
        th = dt(np.float32(thr))
        keep = (unc <= th) if mut == "mask_le" else (unc < th)
    out0 = _row_sum(np.where(keep, sq, dt(0)), dt, mut)
    out1 = _row_sum(keep.astype(dt), dt, mut)
    if mc is None:
        loss = out0 / (float(n) * c * v)
    else:
        loss = out0 / ((c if mut == "den_c" else 2.0) * out1 + 1e-16)
    return np.array([out0, out1, loss]), keep, sq, unc


def consistency_bwd(student, teacher, mask, gs, t, softmax, dt=np.float64, mut=None, want_mag=False):
    """dstudent [N, C, V] for the kept flags `mask` [N, V] (t = 0: all ones)"""
    n, c, v = student.shape
    s, q = student.astype(dt), teacher.astype(dt)
    p, r = (_softmax(s, 1), _softmax(q, 1)) if softmax else (s, q)
    keep = np.ones((n, v), bool) if t == 0 else np.asarray(mask, bool)
    den = float(n) * c * v if t == 0 else 2.0 * float(keep.sum()) + 1e-16
    k2 = dt(np.float32(2.0 / den)) if dt == np.float32 else 2.0 / den
    d = (r - p) if mut == "grad_swap" else (p - r)
    e = d * k2 * keep[:, None].astype(dt)
    g = dt(np.float32(gs))
    if softmax:
        dl = g * (p * (e - (e * p).sum(1, keepdims=True)))
    else:
        dl = g * e
    if not want_mag:
        return dl
    return dl, p, r, np.abs(e), float(k2)


def entropy_fwd(logits, softmax, dt=np.float64, mut=None):
    """-> (out [3]: sum of -sum_c p' ln p', N V, loss; h [N, V])"""
    n, c, v = logits.shape
    l = logits.astype(dt)
    p = _softmax(l, 1) if softmax else l
    pp = p if mut == "ent_999" else p * dt(0.999) + dt(5e-4)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(pp > 0, pp * np.log(pp), dt(0))
    h = np.zeros((n, v), dt)
    for k in range(c):
        h = h - t[:, k]
    out0 = _row_sum(h, dt, mut)
    lnc = 1.0 if mut == "ent_lnc" else np.log(float(c))
    return np.array([out0, float(n) * v, out0 / (lnc * n * v)]), h


def entropy_bwd(logits, gs, softmax, dt=np.float64, mut=None, want_mag=False):
    n, c, v = logits.shape
    l = logits.astype(dt)
    p = _softmax(l, 1) if softmax else l
    pp = p * dt(0.999) + dt(5e-4)
    lnc = 1.0 if mut == "ent_lnc" else np.log(float(c))
    coef = 0.999 / (lnc * n * v)
    coef = dt(np.float32(coef)) if dt == np.float32 else coef
    if mut == "ent_999":
        g = -(coef / dt(0.999)) * (np.log(np.maximum(p, dt(1e-30))) + dt(1.0))
    else:
        g = -coef * (np.log(pp) + dt(1.0))
    gsc = dt(np.float32(gs))
    dl = gsc * (p * (g - (g * p).sum(1, keepdims=True))) if softmax else gsc * g
    if not want_mag:
        return dl
    return dl, p, pp, float(coef)


def ema(e, p, alpha, dt=np.float64, mut=None):
    a = float(np.float32(alpha))
    if dt == np.float32:
        oma = np.float32(1.0 - a)
        a32 = np.float32(a)
        if mut == "ema_swap":
            a32, oma = oma, a32
        return (a32.astype(np.float64) * e.astype(np.float64) + (oma * p.astype(np.float32)).astype(np.float64)).astype(np.float32)
    if mut == "ema_swap":
        a = 1.0 - a
    return a * e.astype(np.float64) + (1.0 - a) * p.astype(np.float64)


# ---------------------------------------------------------------- float64 autograd of the reference's statements

def _t(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def autograd_consistency(student, teacher, mc, thr, softmax, gs):
    """ssl_mt.py:90-100 / ssl_uamt.py:77-100 in float64 -> (masked sum, kept count, loss, dstudent)"""
    S = _t(student).requires_grad_(True)
    Q = _t(teacher)
    p1 = torch.softmax(S, dim=1) if softmax else S
    p1e = torch.softmax(Q, dim=1) if softmax else Q
    if mc is None:
        loss_reg = torch.nn.MSELoss()(p1, p1e)
        out0, out1 = torch.sum(torch.square(p1 - p1e)).item(), float(student.shape[0] * student.shape[2])
    else:
        square_error = torch.square(p1 - p1e)
        preds = _t(mc)
        preds = torch.softmax(preds, dim=2) if softmax else preds
        preds = torch.mean(preds, dim=0)
        unc = -1.0 * torch.sum(preds * torch.log(preds + 1e-6), dim=1, keepdim=True)
        mask = (unc < float(np.float32(thr))).double()
        loss_reg = torch.sum(mask * square_error) / (2 * torch.sum(mask) + 1e-16)
        out0, out1 = torch.sum(mask * square_error).item(), torch.sum(mask).item()
    (loss_reg * float(np.float32(gs))).backward()
    return out0, out1, loss_reg.item(), S.grad.numpy()


def autograd_entropy(logits, softmax, gs):
    """loss/seg/ssl.py:36-43 in float64"""
    L = _t(logits).requires_grad_(True)
    predict = torch.nn.Softmax(dim=1)(L) if softmax else L
    predict = predict * 0.999 + 5e-4
    C = list(predict.shape)[1]
    entropy = torch.sum(-predict * torch.log(predict), dim=1) / np.log(C)
    avg_ent = torch.mean(entropy)
    (avg_ent * float(np.float32(gs))).backward()
    return avg_ent.item(), L.grad.numpy()


# ---------------------------------------------------------------- references with bounds

class Ref(object):
    pass


def _dp(l64, c, softmax):
    """[N, 1, V] (or with leading axes): dp(D) in units of u; 0 without softmax"""
    if not softmax:
        return np.zeros(l64.max(-2, keepdims=True).shape)
    D = l64.max(-2, keepdims=True) - l64.min(-2, keepdims=True)
    return 2.0 * D + 4.0 * E_EXP + c + 1


def consistency_ref(student, teacher, mc, thr, softmax=True, gs=1.0):
    """float64 values of the forward with their bounds.  r.out [3], r.keep (float64 mask), r.undecided [N, V] bool,
    r.out0_bound, r.out1_slack (how many voxels the count may differ by), r.loss_bound"""
    n, c, v = student.shape
    t = 0 if mc is None else mc.shape[0]
    r = Ref()
    out, keep, sq, unc = consistency_fwd(student, teacher, mc, thr, softmax)
    a0, a1, al, adl = autograd_consistency(student, teacher, mc, thr, softmax, gs)
    mag = max(float(sq.sum()), 1e-300)
    assert abs(a0 - out[0]) <= 1e-11 * mag and a1 == out[1] and abs(al - out[2]) <= 1e-11 * max(abs(al), 1e-300), (a0, a1, al, out)
    dl = consistency_bwd(student, teacher, keep, gs, t, softmax)
    assert float(np.abs(adl - dl).max()) <= 1e-11 * max(float(np.abs(dl).max()), 1e-300), "closed-form gradient differs from autograd"
    r.out, r.keep, r.sq, r.unc, r.t = out, keep, sq, unc, t
    s64, q64 = student.astype(np.float64), teacher.astype(np.float64)
    p, q = (_softmax(s64, 1), _softmax(q64, 1)) if softmax else (s64, q64)
    dps, dpq = _dp(s64, c, softmax), _dp(q64, c, softmax)
    d = np.abs(p - q)
    ed = (dps * p + dpq * q) * U + U * d
    e_sq = (2.0 * d * ed).sum(1) + (c + 1) * U * sq
    und = np.zeros((n, v), bool)
    if t:
        l64 = mc.astype(np.float64)
        pr = _softmax(l64, 2) if softmax else l64
        dpt = _dp(l64, c, softmax)
        m = pr.mean(0)
        em = U * ((dpt * pr).sum(0) / t + (t + 1) * m)
        a = m + 1e-6
        la = np.abs(np.log(a))
        ea = em + 2 * U * a
        el = ea / a + E_LOG * U * la
        e_unc = (em * la + m * el).sum(1) + (c + 1) * U * (m * la).sum(1) + (16 * c * ETA if softmax else 0.0)
        r.unc_bound = GAMMA_SLACK * e_unc
        und = (np.abs(unc - float(np.float32(thr))) <= r.unc_bound) & (r.unc_bound > 0)
    r.undecided = und
    dec = keep & ~und
    r.out0_bound = GAMMA_SLACK * (float(e_sq[dec].sum()) + ra_ssl(v) * U * float(sq[dec].sum())) + n * v * c * ETA \
        + float((sq[und] + GAMMA_SLACK * e_sq[und]).sum())
    r.out1_slack = int(und.sum())
    if t == 0:
        r.loss_bound = r.out0_bound / (float(n) * c * v) + 1e-15 * abs(out[2])
    else:
        k_lo, k_hi = float(dec.sum()), float(dec.sum() + und.sum())
        s_lo = max(float(sq[dec].sum()) - r.out0_bound, 0.0)
        s_hi = float(sq[keep | und].sum()) + r.out0_bound
        lo, hi = s_lo / (2 * k_hi + 1e-16), s_hi / (2 * k_lo + 1e-16)
        r.loss_bound = max(hi - out[2], out[2] - lo) * (1 + 1e-12) + 1e-300
    return r


def check_case_is_a_real_test(r, n, v):
    """the oracle-side preconditions of a UAMT case: at most 1 % undecided voxels, and - where the case has at least 100 voxels, so
    that a share is more than a coin or two - a kept share inside [0.2, 0.9]"""
    share_und = float(r.undecided.mean())
    assert share_und <= MAX_UNDECIDED, "undecided share %g" % share_und
    if r.t and n * v >= 100:
        kept = float(r.keep.mean())
        assert KEPT_SHARE[0] <= kept <= KEPT_SHARE[1], "kept share %g" % kept


def check_consistency_fwd(r, out_got, mask_got, what=""):
    """device out [>= 3] and mask [N, V] (None for t = 0) against the reference -> dict of error / bound ratios (asserted <= 1)"""
    res = {}
    if r.t:
        mg = np.asarray(mask_got).reshape(r.keep.shape).astype(bool)
        assert set(np.unique(np.asarray(mask_got)).tolist()) <= {0, 1}, "%s: mask values" % what
        bad = (mg != r.keep) & ~r.undecided
        assert not bad.any(), "%s: %d decided voxels differ in the mask" % (what, int(bad.sum()))
        assert float(out_got[1]) == float(mg.sum()), "%s: out1 %r is not the mask's count %d" % (what, out_got[1], mg.sum())
    else:
        assert float(out_got[1]) == r.out[1], (what, out_got[1], r.out[1])
    assert abs(float(out_got[1]) - r.out[1]) <= r.out1_slack
    res["out0"] = ratio(out_got[0], r.out[0], r.out0_bound)
    res["loss"] = ratio(out_got[2], r.out[2], r.loss_bound)
    bad = {k: x for k, x in res.items() if not x <= 1.0}
    assert not bad, "%s: error / bound = %s" % (what, bad)
    return res


def consistency_grad_ref(student, teacher, mask, gs, t, softmax=True):
    """float64 dstudent for the DEVICE's mask, with its bound -> (dl, bound)"""
    n, c, v = student.shape
    dl, p, q, E, k2 = consistency_bwd(student, teacher, mask, gs, t, softmax, want_mag=True)
    g = abs(float(np.float32(gs)))
    if not softmax:
        return dl, 4 * U * np.abs(dl) + ETA
    s64, q64 = student.astype(np.float64), teacher.astype(np.float64)
    dps, dpq = _dp(s64, c, True), _dp(q64, c, True)
    ed = (dps * p + dpq * q) * U + U * np.abs(p - q)
    keepf = (np.ones((n, 1, v)) if t == 0 else np.asarray(mask, bool).reshape(n, 1, v).astype(np.float64))
    ee = k2 * ed * keepf + 2 * U * E
    S = g * p * (E + (p * E).sum(1, keepdims=True))
    inner = ee + (p * ee + dps * U * p * E).sum(1, keepdims=True)
    bound = GAMMA_SLACK * (g * p * inner + (dps + c + 5) * U * S) + ETA * (1 + g * (E + E.sum(1, keepdims=True)))
    return dl, bound


def entropy_ref(logits, softmax=True, gs=1.0):
    """r.out [3], r.out0_bound, r.loss_bound, r.dl, r.dl_bound"""
    n, c, v = logits.shape
    r = Ref()
    out, h = entropy_fwd(logits, softmax)
    al, adl = autograd_entropy(logits, softmax, gs)
    assert abs(al - out[2]) <= 1e-11 * max(abs(al), 1e-300), (al, out)
    dl, p, pp, coef = entropy_bwd(logits, gs, softmax, want_mag=True)
    assert float(np.abs(adl - dl).max()) <= 1e-11 * max(float(np.abs(dl).max()), 1e-300), "closed-form gradient differs from autograd"
    l64 = logits.astype(np.float64)
    dp = _dp(l64, c, softmax)
    ep = dp * U * p
    lp = np.abs(np.log(pp))
    epp = 0.999 * ep + 4 * U * pp
    el = epp / pp + E_LOG * U * lp
    e_h = (epp * lp + pp * el).sum(1) + (c + 1) * U * np.abs(h)
    r.out = out
    r.out0_bound = GAMMA_SLACK * (float(e_h.sum()) + ra_ssl(v) * U * float(np.abs(h).sum())) + 2000.0 * n * v * c * ETA
    r.loss_bound = r.out0_bound / (np.log(float(c)) * n * v) + 1e-15 * abs(out[2])
    g = abs(float(np.float32(gs)))
    G = coef * (lp + 1.0)
    eg = coef * el + 3 * U * G
    r.dl = dl
    if softmax:
        S = g * p * (G + (p * G).sum(1, keepdims=True))
        inner = eg + (p * eg + dp * U * p * G).sum(1, keepdims=True)
        r.dl_bound = GAMMA_SLACK * (g * p * inner + (dp + c + 5) * U * S) + ETA * (1 + g * (G + G.sum(1, keepdims=True) + 2000 * coef))
    else:
        r.dl_bound = GAMMA_SLACK * g * (eg + U * G) + ETA
    return r


def ema_ref(e, p, alpha):
    """-> (e', bound)"""
    a = float(np.float32(alpha))
    out = ema(e, p, alpha)
    return out, GAMMA_SLACK * (2 * U * np.abs((1.0 - a) * p.astype(np.float64)) + U * np.abs(out)) + ETA


def clamped_normal_moments(sigma, clip):
    """-> (variance, fourth moment) of clamp(sigma z, -clip, clip), z ~ N(0, 1); the mean is 0"""
    k = clip / sigma
    Phi = 0.5 * (1.0 + math.erf(k / math.sqrt(2.0)))
    phi = math.exp(-0.5 * k * k) / math.sqrt(2.0 * math.pi)
    m2 = sigma ** 2 * ((2 * Phi - 1) - 2 * k * phi) + 2 * clip ** 2 * (1 - Phi)
    m4 = sigma ** 4 * (3 * (2 * Phi - 1) - 2 * phi * (k ** 3 + 3 * k)) + 2 * clip ** 4 * (1 - Phi)
    return m2, m4
