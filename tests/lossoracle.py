"""Order-independent float64 oracles for the loss, filter, hard-label and Adam kernels ("two oracles").

The kernels under test (fpl-plus_amd/csrc/loss_filter.hip): per sample, partial ROWS of fp32 sums - row r of rows = fplx_loss_rows(V)
- 5 takes the voxels v with (v // 256) % rows == r, at most ROW_TERMS(V) = 256 ceil(V / (256 rows)) of them - then the rows in
double to `sums[N][K]` and `totals[K]`, K = 6C + 3: per class (Yw, Pw, Iw, Yh, Ph, Ih) = sums of (y w, p w, y p w, y, h, y h) with
p the prediction (softmax(l), or l itself with softmax = 0) and h the one-hot argmax of the raw outputs (first maximum); then the CE
numerator sum w (-sum_c y_c log(0.999 p_c + 5e-4)), sum w, and the entropy sum -sum_c q_c log2(q_c + 1e-10), q = softmax(l) ALWAYS.
Values come from oracle/torch_ref.py run in float64, gradients from autograd; `sums` / `from_sums` / `bwd` in float64 state the same in closed form (asserted
against autograd, 1e-11 of the magnitude, in every `reference` call) because the bounds need the un-cancelled magnitudes, which autograd does not give.

A - exact oracle.  y in {0, 1}, w in {0, 1/4, 1/2, 1}; softmax = 0: p a multiple of 2^-6 in [0, 1]; softmax = 1: logits in
    {0, -200} per class with a power-of-two number k of zeros per voxel: expf(0) = 1 and expf(-200) = 0 exactly (e^-200 is far below
    the smallest denormal), the sum is k, p is 1/k or 0 exactly.  Every term of the 6C + 1 Dice / hard-Dice / weight sums is then a
    multiple of 2^-8 (softmax 0: 2^-2 x 2^-6) and, while a row's sum of magnitudes in that unit stays below 2^24 (asserted on the
    data, `exact_pre`), every partial sum is exact in fp32 in ANY order; the double sum of the rows is exact as well.  These entries
    of sums / totals equal the float64 sums bit for bit, and out[4..] (evaluated in double from them by the same expression) equals
    float32(float64 value).  The CE numerator and the entropy sum go through logf / log2f: oracle B.
B - rounding oracle.  u = 2^-24.  Named constants: E_EXP = E_LOG = 3 ulp = 6 u relative for expf / logf / log2f.  ROCm's table of
    the HIP math functions' accuracy is not among this project's files, and nobody measured the device functions for this bound:
    the figure is the OpenCL C full-profile limit for exp / log / log2 (<= 3 ulp), which is what the device math library these
    functions resolve to is specified against.  The mutation tests (tests/test_loss_oracle_cpu.py) keep the bound honest.
    With D = max_k (max - l_k) of a voxel:
      dp(D) = 2 D + 4 E_EXP + C + 1   [u]  relative error of a probability: l - max rounds (<= u D in each exponent: numerator
              and sum), two expf, C - 1 additions of positive terms, one division;
      ra    = ROW_TERMS / 256 + 9          additions on the way from a voxel's term to its row (grid-stride, 6 shuffles, 3 in LDS);
      dsum  = dp(D_max) + ra + 3      [u]  relative error of a sum of non-negative terms (two products, the adds);
      eg    = 3 dsum + 3 dp(D) + 2 E_LOG + 10   covers each gradient term relative to ITS magnitude: Dice A y + B (B ~ num / den^2:
              three sums, double -> float, fma, x w), CE (the ce_norm, p in the denominator, the constants 0.999f, 5e-4f, 3 products
              and a division), entropy (log2f of a rounded argument: (dp + 1) / ln 2 absolute, 2 E_LOG relative, the p / (p + eps)
              part twice dp).
    dlogits_c = gs p_c (g_c - sum_k g_k p_k) cancels, so the bound is on the un-cancelled magnitude: with G_c = w (|A| y_c + |B|) +
    |CE term| + cent (|log2(p_c + 1e-10)| + 1 / ln 2),
      S_c = |gs| p_c (G_c + sum_k p_k G_k),     |err| <= GAMMA_SLACK (eg + 2 dp(D) + C + 3) u S_c + ETA (1 + |gs| (G_c + sum p G + LIP)).
    (the dot product: C fma and the p_k again; the subtraction; x p_c; x gs).  GAMMA_SLACK = 1.01 covers the second-order products
    of errors all below 1e-3.  With softmax = 0 the Dice / CE part goes to dlogits directly (p = l is exact) and S_c = |gs| (G_c +
    q_c (Ge_c + sum q Ge)).  ETA = 2^-126 is the underflow term: where expf's result is denormal the device may keep it (gradual
    underflow, error <= 2^-149) or flush it to zero (error < 2^-126) - the bound assumes neither, it takes the larger; p's absolute
    error is then <= ETA, which enters p_c's factor directly and the terms through their derivatives, LIP = cce w y 0.999^2 / 5e-4^2
    + 2 cent 1e10 / ln 2; one more ETA for a flushed result.
    Scalars, same reasoning on sum |terms|: the CE numerator (2 E_LOG + C + 3 + ra) u sum w y |log| + (dp + 3) u sum w y (the
    argument's error, slope <= 1); the entropy sum (2 E_LOG + dp + C + 2 + ra) u sum q |log2| + (dp + 1) u / ln 2 sum q; Dice ratios
    (2 dsum + 4) u each; every out[] one more u for its float.  The hard-class Dice compares raw fp32 logits exactly, so only its
    sums round: (2 ra + 4) u.

mc_filter: on the exact-probability data numpy's softmax and the device's agree on every probability, so hards, means (a sequential
    fp32 sum of multiples of 1/8 and ONE correctly rounded division) and the boundary count are determined.  The per-voxel variance
    terms are exact only when T is a power of two (then the mean is exact); otherwise `s2 += d * d` may or may not contract to an
    fma and the comparison is the bound below.  Random data against `filter_ref` (float64): per class d = q - mean has absolute
    error (dp + T + 1) u (q + mean), vars <= sum [2 |d| err(d) + (T + 2) u d^2] / T + C u vsum; means (dp + T + 1) u m + ETA.
    `uncertainty` uses logf and keeps the absolute 2e-7 of the fixture test.
Adam: one step from the device's own fp32 state against float64 (oracle.torch_ref.AdamRef's formulas): gi = wd p + g gs (2 u on
    Gi = |wd p| + |g gs|), m' (that x (1 - b1), + 2 u (|b1 m| + (1 - b1) Gi)), v' (2 Gi err(gi) (1 - b2) + 3 u v' + ETA), sqrt
    (min(E_v / 2 sqrt v', sqrt E_v) + u sqrt v'), denominator (x 1/sqrt(bc2), 2 u, + u denom), update step m' / denom (E_m / denom +
    |m'| E_den / denom^2, 3 u, the rounded step size), p' (+ u (|p| + |update|)).

Excluded mutation: the p / ((p + 1e-10) ln 2) part of the entropy gradient is the same constant 1 / ln 2 for every class (up to
1e-10 / p) and cancels under the softmax Jacobian (sum_c p_c (k - sum_k k p_k) = 0): changing it is not detectable and is not listed.

Pure numpy / torch on the CPU; tests/test_loss_oracle_cpu.py checks the oracle itself, tests/test_gpu_loss_exact.py applies it."""
import zlib

import numpy as np
import torch

from oracle import np_ref as N
from oracle import torch_ref as R

U = 2.0 ** -24
ETA = 2.0 ** -126
E_EXP = 6.0                 # 3 ulp in units of u
E_LOG = 6.0
GAMMA_SLACK = 1.01
EXACT_LIMIT = float(1 << 24)
INV_LN2 = 1.0 / np.log(2.0)
MUTATIONS = ("ce_999", "ent_eps", "last_max", "pw_missing", "img_div_n", "ce_norm_eps", "drop_voxel", "row_twice")


def rng(key):
    return np.random.default_rng(zlib.crc32(key.encode()))


def loss_rows(v):
    return int(min(512, max(1, (v + 4095) // 4096)))


def row_terms(v):
    return 256 * (-(-v // (256 * loss_rows(v))))


def row_of(v):
    return (np.arange(v) // 256) % loss_rows(v)


# ---------------------------------------------------------------- generators

def one_hot(idx, c):
    """idx [N, V] -> float32 [N, C, V]"""
    return np.ascontiguousarray(np.moveaxis(np.eye(c, dtype=np.float32)[idx], -1, 1))


def exact_logits(key, n, c, v, lead=()):
    """logits in {0, -200} with a power-of-two number of zeros per voxel -> float32 lead + [N, C, V]"""
    g = rng(key)
    shape = tuple(lead) + (n, v)
    ks = [k for k in (1, 2, 4, 8) if k <= c]
    k = np.asarray(ks)[g.integers(0, len(ks), shape)]
    rank = np.argsort(g.random(shape + (c,)), axis=-1)               # a random permutation of the classes per voxel
    lg = np.where(rank < k[..., None], 0.0, -200.0).astype(np.float32)
    return np.ascontiguousarray(np.moveaxis(lg, -1, -2))


def exact_probs(key, n, c, v):
    """softmax = 0 predictions: multiples of 2^-6 in [0, 1]"""
    return (rng(key).integers(0, 65, (n, c, v)) / 64.0).astype(np.float32)


def exact_weights(key, n, v):
    return np.asarray([0.0, 0.25, 0.5, 1.0], np.float32)[rng(key).integers(0, 4, (n, v))]


def hard_labels(key, n, c, v, absent=None):
    """one-hot labels; class `absent` never occurs"""
    idx = rng(key).integers(0, c, (n, v))
    if absent is not None and c > 1:
        idx = np.where(idx == absent, (absent + 1) % c, idx)
    return one_hot(idx, c)


def soft_labels(key, n, c, v):
    y = rng(key).random((n, c, v)).astype(np.float32) + 0.05
    return (y / y.sum(1, keepdims=True)).astype(np.float32)


def real_logits(key, n, c, v, scale=2.0, gap=None, ties=0.0):
    """N(0, scale^2) logits; gap: class 0 leads every other class by exactly that much in a third of the voxels; ties: that fraction
    of the voxels has l_1 = l_0 (C >= 2)"""
    g = rng(key)
    lg = (g.standard_normal((n, c, v)) * scale).astype(np.float32)
    if gap is not None:
        sel = g.random((n, v)) < 1.0 / 3
        top = lg.max(1)
        for k in range(1, c):
            lg[:, k] = np.where(sel, top - np.float32(gap), lg[:, k])
        lg[:, 0] = np.where(sel, top, lg[:, 0])
    if ties and c > 1:
        sel = g.random((n, v)) < ties
        lg[:, 1] = np.where(sel, lg[:, 0], lg[:, 1])
    return lg


def real_probs(key, n, c, v):
    return soft_labels(key, n, c, v)


def separated_logits(key, shape_ncv, scale=2.0, min_gap=1e-3):
    """random logits whose two largest per voxel differ by at least min_gap (axis -2 is the class axis)"""
    lg = (rng(key).standard_normal(shape_ncv) * scale).astype(np.float32)
    if lg.shape[-2] > 1:
        srt = np.sort(lg, axis=-2)
        close = (srt[..., -1, :] - srt[..., -2, :]) < np.float32(2 * min_gap)
        top = lg.argmax(-2)
        bump = np.where(close, np.float32(16 * min_gap), np.float32(0))
        np.put_along_axis(lg, top[..., None, :], np.take_along_axis(lg, top[..., None, :], -2) + bump[..., None, :], -2)
    return lg


# ---------------------------------------------------------------- the three stages of the C ABI, in float64 or as an fp32 restatement

def _softmax(l):
    m = l.max(1, keepdims=True)
    e = np.exp(l - m)
    s = e[:, :1].copy()
    for c in range(1, l.shape[1]):
        s = s + e[:, c:c + 1]
    return e / s


def _reduce(x, dt, mut):
    """[N, V] terms -> [N] float64: exact in float64; in fp32 the kernel's order - partial rows in fp32, the rows in double"""
    if dt == np.float64:
        return x.astype(np.float64).sum(1)
    v = x.shape[1]
    r = row_of(v)
    order = np.argsort(r, kind="stable")
    starts = np.searchsorted(r[order], np.arange(loss_rows(v)))
    xs = x[:, order].astype(np.float32)
    if mut == "drop_voxel":
        xs = xs.copy()
        xs[:, (starts[1] if len(starts) > 1 else v) - 1] = 0          # the last voxel of row 0
    parts = np.add.reduceat(xs, starts, axis=1, dtype=np.float32).astype(np.float64)
    s = parts.sum(1)
    return s + parts[:, 0] if mut == "row_twice" else s


def _argmax(l, mut):
    c = l.shape[1]
    return c - 1 - l[:, ::-1].argmax(1) if mut == "last_max" else l.argmax(1)


def sums(lg, y, pw, softmax, dt=np.float64, mut=None):
    """fplx_seg_loss_sums -> sums [N, K] float64"""
    n, c, v = lg.shape
    l, yy = lg.astype(dt), y.astype(dt)
    w = np.ones((n, v), dt) if pw is None else pw.astype(dt)
    q = _softmax(l)
    p = q if softmax else l
    am = _argmax(l, mut)
    out = np.zeros((n, 6 * c + 3))
    ce = np.zeros((n, v), dt)
    ent = np.zeros((n, v), dt)
    eps = dt(1e-6 if mut == "ent_eps" else 1e-10)
    for k in range(c):
        h = (am == k).astype(dt)
        cols = (yy[:, k] * w, p[:, k] if mut == "pw_missing" else p[:, k] * w, yy[:, k] * p[:, k] * w, yy[:, k], h, yy[:, k] * h)
        for j, x in enumerate(cols):
            out[:, 6 * k + j] = _reduce(x, dt, mut)
        ce = ce - yy[:, k] * np.log(p[:, k] * dt(0.999) + dt(5e-4))
        ent = ent - q[:, k] * np.log2(q[:, k] + eps)
    out[:, 6 * c] = _reduce(w * ce, dt, mut)
    out[:, 6 * c + 1] = _reduce(w, dt, mut)
    out[:, 6 * c + 2] = _reduce(ent, dt, mut)
    return out


def from_sums(sm, totals, iw, n_global, v, has_pw, terms, dt=np.float64, mut=None):
    """fplx_seg_loss_from_sums -> (out [4 + C], coef dict A, B [N, C] (global Dice, image-weighted Dice), cce, cent) in double; the
    fp32 restatement rounds out and the coefficients to float as the kernel does"""
    n, kk = sm.shape
    c = (kk - 3) // 6
    wd, wc, wi, we = [float(np.float32(t)) for t in terms]
    t = totals.reshape(-1)
    T6, S6 = t[:6 * c].reshape(c, 6), sm[:, :6 * c].reshape(n, c, 6)
    den, num = T6[:, 0] + T6[:, 1] + 1e-5, 2.0 * T6[:, 2] + 1e-5
    Ld = 1.0 - (num / den).sum() / c
    hard = (2.0 * T6[:, 5] + 1e-5) / (T6[:, 3] + T6[:, 4] + 1e-5)
    Ag = np.broadcast_to(wd * (-2.0 / (c * den)), (n, c)).copy()
    Bg = np.broadcast_to(wd * (num / (c * den * den)), (n, c)).copy()
    Ai, Bi, Limg, ratios_img = np.zeros((n, c)), np.zeros((n, c)), 0.0, 0.0
    if wi != 0.0:
        f = np.asarray(iw, np.float64).reshape(n) / (n if mut == "img_div_n" else n_global)
        dn, nm = S6[:, :, 0] + S6[:, :, 1] + 1e-5, 2.0 * S6[:, :, 2] + 1e-5
        Ai, Bi = wi * f[:, None] * (-2.0 / (c * dn)), wi * f[:, None] * (nm / (c * dn * dn))
        Limg = float((f * (1.0 - (nm / dn).sum(1) / c)).sum())
        ratios_img = float((np.abs(f) * (1.0 + (nm / dn).sum(1) / c)).sum())
    cenum, wsum, ent = t[6 * c], t[6 * c + 1], t[6 * c + 2]
    with np.errstate(divide="ignore"):
        ce_norm = (1.0 / (wsum + (0.0 if mut == "ce_norm_eps" else 1e-5))) if has_pw else 1.0 / (n_global * float(v))
    Lce, Lent = cenum * ce_norm, ent / (n_global * float(v))
    out = np.concatenate([[wd * Ld + wi * Limg + wc * Lce + we * Lent, wd * Ld + wi * Limg, Lce, Lent], hard])
    coef = dict(Ag=Ag, Bg=Bg, Ai=Ai, Bi=Bi, cce=wc * ce_norm, cent=we / (n_global * float(v)), ce_norm=ce_norm,
                dice_mag=abs(wd) * (1.0 + (num / den).sum() / c) + abs(wi) * ratios_img)
    if dt == np.float32:
        out = out.astype(np.float32).astype(np.float64)
        f32 = lambda a: np.asarray(a, np.float32)
        coef.update(Ag=f32(f32(Ag) + f32(Ai)), Ai=np.zeros((n, c), np.float32), Bg=f32(f32(Bg) + f32(Bi)),
                    Bi=np.zeros((n, c), np.float32), cce=f32(coef["cce"]), cent=f32(coef["cent"]))
    return out, coef


def bwd(lg, y, pw, coef, gscale, terms, softmax, dt=np.float64, mut=None, want_mag=False):
    """fplx_seg_loss_bwd -> dlogits [N, C, V] (and, for the bound, S and the underflow factor)"""
    n, c, v = lg.shape
    l, yy = lg.astype(dt), y.astype(dt)
    w = (np.ones((n, v), dt) if pw is None else pw.astype(dt))[:, None]
    wd, wc, wi, we = terms
    q = _softmax(l)
    p = q if softmax else l
    A = (coef["Ag"] + coef["Ai"]).astype(dt)[:, :, None]
    B = (coef["Bg"] + coef["Bi"]).astype(dt)[:, :, None]
    cce, cent, gs = dt(coef["cce"]), dt(coef["cent"]), dt(gscale)
    eps = dt(1e-6 if mut == "ent_eps" else 1e-10)
    g = np.zeros_like(l)
    ge = np.zeros_like(l)
    if wd != 0 or wi != 0:
        g = g + w * (A * yy + B)
    if wc != 0:
        g = g - cce * w * yy * dt(1.0 if mut == "ce_999" else 0.999) / (p * dt(0.999) + dt(5e-4))
    if we != 0:
        ge = -cent * (np.log2(q + eps) + q * dt(INV_LN2) / (q + eps))
    if softmax:
        g = g + ge
        dl = gs * (p * (g - (g * p).sum(1, keepdims=True)))
    else:
        dl = gs * (g + q * (ge - (ge * q).sum(1, keepdims=True)))
    if not want_mag:
        return dl
    mA = np.abs(coef["Ag"])[:, :, None] + np.abs(coef["Ai"])[:, :, None]
    mB = np.abs(coef["Bg"])[:, :, None] + np.abs(coef["Bi"])[:, :, None]
    G = np.zeros_like(l)
    Ge = np.zeros_like(l)
    lip = np.zeros_like(l)
    if wd != 0 or wi != 0:
        G = G + w * (mA * yy + mB)
    if wc != 0:
        G = G + np.abs(cce * w * yy * 0.999 / (p * 0.999 + 5e-4))
        lip = lip + np.abs(cce) * w * yy * (0.999 / 5e-4) ** 2
    if we != 0:
        Ge = np.abs(cent) * (np.abs(np.log2(q + 1e-10)) + INV_LN2)
        lip = lip + 2.0 * np.abs(cent) * 1e10 * INV_LN2
    if softmax:
        G = G + Ge
        tot = G + (p * G).sum(1, keepdims=True)
        S = np.abs(gs) * p * tot
    else:
        tot = G + Ge + (q * Ge).sum(1, keepdims=True)
        S = np.abs(gs) * (G + q * (Ge + (q * Ge).sum(1, keepdims=True)))
    return dl, S, np.abs(gs) * (tot + lip)


# ---------------------------------------------------------------- the float64 reference with its bounds

def autograd(lg, y, pw, iw, terms, softmax, gscale=1.0):
    """oracle/torch_ref.py in float64 -> (out [4], class Dice [C], dlogits): values and autograd gradient, shapes [N, C, V]"""
    n, c, v = lg.shape
    t5 = lambda a: None if a is None else torch.from_numpy(np.asarray(a, np.float64)).reshape(a.shape[0], -1, 1, 1, v)
    L = t5(lg).requires_grad_(True)
    Y, W = t5(y), t5(pw)
    wd, wc, wi, we = [float(np.float32(t)) for t in terms]
    dice = torch.zeros((), dtype=torch.float64)
    if wd != 0:
        dice = dice + wd * R.dice_loss(L, Y, W, softmax)
    if wi != 0:
        dice = dice + wi * R.dice_loss_image_weighted(L, Y, W, torch.from_numpy(np.asarray(iw, np.float64)), softmax)
    ce, ent = R.ce_loss(L, Y, W, softmax), R.entropy_term(L)
    total = dice + wc * ce + we * ent
    (total * float(gscale)).backward()
    out = np.array([t.item() for t in (total.detach(), dice.detach(), ce.detach(), ent.detach())])
    return out, R.hard_dice_metric(L.detach(), Y).numpy(), L.grad.numpy().reshape(n, c, v)


class Ref(object):
    pass


def reference(lg, y, pw, iw, terms, softmax=True, gscale=1.0, use_autograd=True):
    """float64 values and the bounds of oracle B for ONE loss over the batch (lg, y [N, C, V]; pw [N, V] or None; iw [N] or None).
    The values are torch_ref's and autograd's; the closed form must agree with them (asserted) and supplies the magnitudes."""
    n, c, v = lg.shape
    assert float(y.min()) >= 0 and (pw is None or float(pw.min()) >= 0), "the bounds assume non-negative labels and weights"
    r = Ref()
    gscale = float(np.float32(gscale))
    sm = sums(lg, y, pw, softmax)
    r.sums, r.totals = sm, sm.sum(0)
    out, coef = from_sums(sm, r.totals, iw, n, v, pw is not None, terms)
    dl, S, under = bwd(lg, y, pw, coef, gscale, terms, softmax, want_mag=True)
    r.out, r.dl, r.S = out, dl, S
    if use_autograd:
        ao, ah, adl = autograd(lg, y, pw, iw, terms, softmax, gscale)
        assert np.allclose(ao, out[:4], rtol=1e-11, atol=1e-13), (ao, out[:4])
        assert np.allclose(ah, out[4:], rtol=1e-11, atol=0)
        scale = max(float(S.max()), 1e-300)
        assert float(np.abs(adl - dl).max()) <= 1e-11 * scale, "closed-form gradient differs from autograd"
        r.out, r.dl = np.concatenate([ao, ah]), adl
    # ---- bounds
    l64 = lg.astype(np.float64)
    D = (l64.max(1, keepdims=True) - l64.min(1, keepdims=True)) if softmax or terms[3] != 0 else np.zeros((n, 1, v))
    dp = 2.0 * D + 4.0 * E_EXP + c + 1
    dpm = float(dp.max())
    ra = row_terms(v) / 256 + 9
    dsum = dpm + ra + 3
    gam = GAMMA_SLACK * (3 * dsum + 5 * dp + 2 * E_LOG + c + 13) * U
    r.gamma_units = float(gam.max() / U)
    r.dl_bound = gam * S + ETA * (1.0 + under)
    # sums: the Dice entries are sums of non-negative terms; the two transcendental ones as derived in the docstring
    w = np.ones((n, v)) if pw is None else pw.astype(np.float64)
    q = _softmax(l64)
    p = q if softmax else l64
    y64 = y.astype(np.float64)
    sb = GAMMA_SLACK * dsum * U * np.abs(sm) + v * ETA
    lgs = np.abs(np.log(p * 0.999 + 5e-4))
    t1, t2 = (w[:, None] * y64 * lgs).sum((1, 2)), (w[:, None] * y64).sum((1, 2))
    sb[:, 6 * c] = GAMMA_SLACK * U * ((2 * E_LOG + c + 3 + ra) * t1 + (dpm + 3) * t2) + v * ETA
    e1, e2 = (q * np.abs(np.log2(q + 1e-10))).sum((1, 2)), q.sum((1, 2))
    sb[:, 6 * c + 2] = GAMMA_SLACK * U * ((2 * E_LOG + dpm + c + 2 + ra) * e1 + (dpm + 1) * INV_LN2 * e2) + v * ETA * 1e10
    r.sums_bound = sb
    wd, wc, wi, we = [abs(float(t)) for t in terms]
    ob = np.zeros(4 + c)
    ob[1] = GAMMA_SLACK * (2 * dsum + 4) * U * coef["dice_mag"]
    ce_norm = coef["ce_norm"]
    ob[2] = sb[:, 6 * c].sum() * ce_norm + GAMMA_SLACK * (dsum + 2) * U * abs(out[2])
    ob[3] = sb[:, 6 * c + 2].sum() / (n * float(v))
    ob[0] = ob[1] + wc * ob[2] + we * ob[3]
    ob[:4] += U * np.abs(out[:4]) + ETA
    ob[4:] = GAMMA_SLACK * (2 * ra + 4) * U * np.abs(out[4:])
    r.out_bound = ob
    return r


def ratio(got, ref, bound):
    """max |got - ref| / bound (NaN / inf -> inf; 0 / 0 -> 0): <= 1 passes"""
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    if got.size == 0:
        return 0.0
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bound)
    q = np.where(np.isfinite(got) & ~np.isnan(q), q, np.inf)
    return float(q.max())


def check_B(r, out=None, dl=None, sm=None, what=""):
    """oracle B: each given output against the reference -> dict of worst error / bound ratios (asserted <= 1)"""
    res = {}
    if out is not None:
        res["out"] = ratio(out, r.out, r.out_bound)
    if dl is not None:
        res["dlogits"] = ratio(dl, r.dl, r.dl_bound)
    if sm is not None:
        res["sums"] = ratio(sm, r.sums, r.sums_bound)
    bad = {k: v for k, v in res.items() if not v <= 1.0}
    assert not bad, "%s: error / bound = %s" % (what, bad)
    return res


# ---------------------------------------------------------------- oracle A

def exact_cols(c):
    """the 6C + 1 exact entries of a sums row"""
    return list(range(6 * c)) + [6 * c + 1]


def exact_pre(lg, y, pw, softmax):
    """precondition of oracle A, asserted on the data: labels in {0, 1}, dyadic weights, exact probabilities, and per partial row
    the sum of the magnitudes in units of the smallest term (2^-8) below 2^24"""
    n, c, v = lg.shape
    assert np.isin(y, (0.0, 1.0)).all()
    w = np.ones((n, v)) if pw is None else pw.astype(np.float64)
    assert np.array_equal(w * 4, np.round(w * 4)) and w.min() >= 0 and w.max() <= 1
    if softmax:
        assert np.isin(lg, (0.0, -200.0)).all()
        k = (lg == 0).sum(1)
        assert np.isin(k, (1, 2, 4, 8)).all(), "the number of tied maxima must be a power of two"
    else:
        assert np.array_equal(lg * 64, np.round(lg * 64)) and lg.min() >= 0 and lg.max() <= 1
    # every term is at most 1 = 2^8 units: a row of t terms sums to at most t 2^8
    worst = row_terms(v) * 256.0
    assert worst < EXACT_LIMIT, "a row's sum of |terms| reaches %g units >= 2^24" % worst
    return worst


def check_A(sm_got, totals_got, out_got, lg, y, pw, softmax, what=""):
    """oracle A on fplx_seg_loss_sums' sums / totals and on out[4..] -> number of entries compared"""
    exact_pre(lg, y, pw, softmax)
    c = lg.shape[1]
    # the probabilities fp32 determines on this data: 1 / k on the k tied maxima, 0 elsewhere (float64's e^-200 is not 0); the
    # first maximum of the raw outputs is the first of these as well
    pr = np.where(lg == 0, 1.0 / (lg == 0).sum(1, keepdims=True), 0.0) if softmax else lg
    ref = sums(pr, y, pw, False)
    cols = exact_cols(c)
    sm_got = np.asarray(sm_got, np.float64)
    bad = ~(sm_got[:, cols] == ref[:, cols])
    assert not bad.any(), "%s: %d of %d exact sums differ (first: got %r, want %r)" % (
        what, int(bad.sum()), bad.size, sm_got[:, cols][bad][0], ref[:, cols][bad][0])
    if totals_got is not None:
        tg = np.asarray(totals_got, np.float64)
        assert np.array_equal(tg[cols], ref.sum(0)[cols]), "%s: totals differ" % what
    if out_got is not None:
        t6 = ref.sum(0)[:6 * c].reshape(c, 6)
        want = ((2.0 * t6[:, 5] + 1e-5) / (t6[:, 3] + t6[:, 4] + 1e-5)).astype(np.float32)
        assert np.array_equal(np.asarray(out_got, np.float32)[4:], want), "%s: hard-class Dice %r != %r" % (what, out_got[4:], want)
    return bad.size


# ---------------------------------------------------------------- the fp32 restatement as one call (tests/test_loss_oracle_cpu.py)

def restate(lg, y, pw, iw, terms, softmax=True, gscale=1.0, mut=None, shards=1, dt=np.float32):
    """the kernels' arithmetic in fp32 numpy: sums -> from_sums -> bwd, optionally over `shards` equal ranks whose totals are
    added in float64 (the split path) -> (sums [N, K], totals, [out of each rank], dlogits [N, C, V])"""
    n, c, v = lg.shape
    per = n // shards
    sl = [slice(i * per, (i + 1) * per) for i in range(shards)]
    sub = lambda a, s: None if a is None else a[s]
    sms = [sums(lg[s], y[s], sub(pw, s), softmax, dt, mut) for s in sl]
    totals = np.sum([s.sum(0) for s in sms], axis=0)
    outs, dls = [], []
    for s, sm in zip(sl, sms):
        out, coef = from_sums(sm, totals, sub(iw, s), n, v, pw is not None, terms, dt, mut)
        outs.append(out)
        dls.append(bwd(lg[s], y[s], sub(pw, s), coef, np.float32(gscale), terms, softmax, dt, mut).astype(np.float64))
    return np.concatenate(sms), totals, outs, np.concatenate(dls)


def rank_out_ref(r, rank_slice, iw, terms, has_pw):
    """float64 out[] of ONE rank of the split path: the global terms from the full-batch totals plus ITS samples' share of the
    image-weighted Dice (the caller's all-reduce completes the number); bounded by the full batch's out_bound"""
    n, v = r.S.shape[0], r.S.shape[2]
    return from_sums(r.sums[rank_slice], r.totals, None if iw is None else iw[rank_slice], n, v, has_pw, terms)[0]


# ---------------------------------------------------------------- mc_filter / hard_label

def filter_ref(stack):
    """float64 restatement of the filter on fp32 logits [T, C, V] -> dict(vars, vars_bound, means, means_bound, hards)"""
    t, c, v = stack.shape
    l = stack.astype(np.float64)
    q = _softmax(l)
    mean = q.sum(0) / t
    d = q - mean
    s2 = (d * d).sum(0)
    vsum = (s2 / t).sum(0)
    D = l.max(1, keepdims=True) - l.min(1, keepdims=True)
    dp = 2.0 * D + 4.0 * E_EXP + c + 1
    errd = (dp + t + 1) * U * (q + mean)
    vb = ((2.0 * np.abs(d) * errd + (t + 2) * U * d * d).sum(0) / t).sum(0) + c * U * vsum
    return dict(vars=float(vsum.sum()), vars_bound=GAMMA_SLACK * float(vb.sum()) + v * c * ETA, means=mean[1 if c > 1 else 0],
                means_bound=GAMMA_SLACK * (float(dp.max()) + t + 1) * U * mean[1 if c > 1 else 0] + ETA,
                hards=np.asarray(q.argmax(1), np.uint8))


def filter_exact_vars(stack):
    """per-voxel variance terms of exact-probability data in fp32, summed in float64 (exact when T is a power of two)"""
    f = N.fpl_filter(stack.reshape(stack.shape[:2] + (1, 1, -1)))
    return float(f["maps"].var(axis=0).sum(0).astype(np.float64).sum()), f


# ---------------------------------------------------------------- Adam

def adam_ref(p, g, m, v, lr, step, wd, gscale=1.0, b1=0.9, b2=0.999, eps=1e-8):
    """one Adam step in float64 from fp32 state -> (p', m', v', bound p', bound m', bound v'); AdamRef's formulas with the
    constants as the kernel receives them (floats)"""
    f = lambda x: float(np.float32(x))
    lr, wd, gscale, b1, b2, eps = f(lr), f(wd), f(gscale), f(b1), f(b2), f(eps)
    p, g, m, v = [np.asarray(a, np.float64) for a in (p, g, m, v)]
    gi = wd * p + g * gscale
    Gi = np.abs(wd * p) + np.abs(g * gscale)
    e_gi = 2 * U * Gi
    m2 = b1 * m + (1 - b1) * gi
    e_m = (1 - b1) * e_gi + 2 * U * (np.abs(b1 * m) + (1 - b1) * Gi)
    v2 = b2 * v + (1 - b2) * gi * gi
    e_v = (1 - b2) * 2 * Gi * e_gi + 3 * U * (b2 * np.abs(v) + (1 - b2) * Gi * Gi) + ETA
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    sq = np.sqrt(v2)
    with np.errstate(divide="ignore", invalid="ignore"):
        e_sq = np.minimum(np.where(sq > 0, e_v / (2 * sq), np.inf), np.sqrt(e_v)) + U * sq
    isb = 1 / np.sqrt(bc2)
    den = sq * isb + eps
    e_den = (e_sq + 2 * U * sq) * isb + U * den
    upd = (lr / bc1) * m2 / den
    e_upd = (lr / bc1) * (e_m / den + np.abs(m2) * e_den / (den * den)) + 4 * U * np.abs(upd)
    p2 = p - upd
    e_p = GAMMA_SLACK * (e_upd + U * (np.abs(p) + np.abs(upd))) + ETA
    return p2, m2, v2, e_p, GAMMA_SLACK * e_m + U * np.abs(m2) + ETA, GAMMA_SLACK * e_v + U * np.abs(v2) + ETA
