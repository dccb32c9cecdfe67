"""Float64 oracles for the second loss family (fpl-plus_amd/csrc/loss_ext.hip), on top of tests/lossoracle.py (same partial rows,
same two oracles, same notation: u = 2^-24, dp(D), ra, dsum).

The pass under test: per sample the 6C + 3 sums of the first family, then per class c at 6C + 3 + 4c: sum p, sum y p (unweighted),
sum |p - y|^g_nr, sum y L^g_el with L = -log(0.005 + 0.99 p); then at 10C + 3: the GeneralizedCE numerator sum w' sum_c cw_c y_c
(1 - p_c^q) / q (w' = w with use_pw, else 1), sum (p - y)^2, sum |p - y|, the SLSR numerator -sum_c sy_c log(0.999 p_c + 5e-4), sy =
(y - 1/2)(1/2 - eps) / (1/2) + 1/2 where a weight map is given and w > 0, else y.  With M = n_global V:
    FocalDice        1 - mean_c dice_c^(1/beta),  dice_c = (2 I_c + 1e-5) / (Y_c + P_c + 1e-5)  (unweighted sums)
    NoiseRobustDice  mean_c NR_c / (P_c + Y_c + 1e-5)
    ExpLog           w_d mean_c (-log(0.005 + 0.99 dice_c))^g_el + (1 - w_d) sum_c wc_c E_c / M,  wc_c = (Y_c / M + 0.1)^(-1/2)
    GeneralizedCE    numerator / M, with use_pw numerator / sum w (no epsilon)
    MSE, MAE         sum / (M C);   SLSR  numerator / M
`sums_ext` / `from_sums_ext` / `bwd_ext` state sums, values, coefficient table and gradient in closed form, in float64 or - as an
fp32 restatement of the kernels, with mutations - in float32.  `reference_ext` asserts the float64 closed form against float64
autograd of the same definitions written with torch operations (1e-11 of the magnitude) in every call.

A - exact part.  softmax = 0, p a multiple of 2^-6 in [0, 1], y in {0, 1}: p, y p and |p - y| are multiples of 2^-6, (p - y)^2 of 2^-12,
    none above 1.  While a row's sum of magnitudes in units of 2^-12 stays below 2^24 - asserted ON THE DATA by `exact_pre_ext`,
    the worst case of these shapes would not pass - every partial sum is exact in fp32 in any order, fused or not: the entries
    sum (p - y)^2, sum |p - y| and the unweighted P, I, Y of sums / totals equal the float64 sums bit for bit.
B - rounding part, for everything through powf / logf / expf.  E_EXP, E_LOG as in lossoracle; E_POW = 16 ulp = 32 u relative for
    powf: the OpenCL C full-profile limit for pow.  It has the same standing as E_EXP / E_LOG there: nobody measured the device
    function, the figure is what the device math library is specified against; the mutation tests keep the bound honest.
    With ep = dp(D) u p the absolute error of a probability (0 with softmax = 0) and ed = ep + u |d| that of d = p - y:
      |d|^g        g max(|d|, ed)^(g - 1) ed + (E_POW + 1) u |d|^g                                   (g >= 1)
      y L^g        eL = 0.99 ep / s + (E_LOG |L| + 3) u;   y (|g| L^(g - 1) eL + (E_POW + 2) u L^g)
      gce          cw y w' / q ((E_POW + q dp) u p^q + 6 u (1 + p^q))
      (p - y)^2    2 |d| ed + 2 u d^2;    |p - y|   ed;    SLSR as the CE numerator with sy (4 u more for sy itself)
    each summed over the row plus (ra + C) u sum |term|.
    Values and coefficients are evaluated in double from the totals by one thread: their error is the totals' error through the
    derivative - taken numerically, |dF / dT_j| sb_j summed over j - plus the rounding to float.
    Gradient, on un-cancelled magnitudes: every term t of g_c = dLoss / dp_c gets an absolute bound Eg_t:
      Dice-type  w (dA y + dB) + 3 u w (|A| y + |B|)                          (dA, dB: the coefficients' bounds)
      CE, SLSR   t (dc / |c| + 8 u + 0.999 ep / (0.999 p + 5e-4))
      NoiseRobust  dc |d|^(g-1) + |c| (min(ed^(g-1), 2 (g-1) |d|^(g-2) ed) + (E_POW + 4) u |d|^(g-1) + [|d| <= ed] |d|^(g-1))
                 for 1 <= g <= 2 (Hoelder: |a^s - b^s| <= |a - b|^s for s <= 1); the last part is the sign, which the device may
                 take as 0 where the true difference does not vanish.  MAE the same with g = 1: dc + |c| [|d| <= ed]
      MSE        dc |d| + |c| (ep + 3 u |d|)
      ExpLog     t (dc / |c| + |g - 1| eL / L + 0.99 ep / s + (E_POW + 8) u)
      gce        t (dc / |c| + |q - 1| dp u + (E_POW + 6) u)
    and dlogits_c = gs p_c (g_c - sum_k g_k p_k):  |err| <= GAMMA_SLACK (|gs| p_c (Eg_c + sum_k p_k Eg_k) + (2 dp + 2 C + 16) u S_c)
    + ETA with S_c = |gs| p_c (G_c + sum_k p_k G_k), G the sum of the terms' magnitudes; softmax = 0: |gs| (Eg_c + (T + 2) u G_c)
    (T terms added), the entropy term through its own softmax as in lossoracle.  Underflow is excluded, not bounded: a
    probability that underflows makes p^(q - 1) infinite (no guard), so `reference_ext` asserts D < 80.

Pure numpy / torch on the CPU; tests/test_loss_ext_cpu.py checks the oracle itself, tests/test_gpu_loss_ext.py applies it."""
import numpy as np
import torch

import lossoracle as LO
from lossoracle import U, ETA, E_EXP, E_LOG, GAMMA_SLACK, INV_LN2

E_POW = 32.0                # 16 ulp in units of u
EXT_TERMS = ("focal", "noise_robust", "explog", "gce", "mae", "mse", "slsr")
PRM = dict(beta=2.0, gamma_nr=1.5, w_dice_el=0.8, gamma_el=0.3, q=0.7, epsilon=0.25, use_pw=False, class_weight=None)
MUTATIONS = ("gce_q", "explog_999", "wc_no_01", "mse_div_m", "focal_weighted_p", "sign0_one", "drop_voxel", "row_twice")
_ROW_MUT = ("drop_voxel", "row_twice")


def ext_k(c):
    return 10 * c + 7


def weights(**kw):
    """(w_focal, ..., w_slsr) from keywords named as EXT_TERMS"""
    assert set(kw) <= set(EXT_TERMS)
    return tuple(float(kw.get(k, 0.0)) for k in EXT_TERMS)


def params(**kw):
    p = dict(PRM)
    assert set(kw) <= set(p)
    p.update(kw)
    return p


def cfg_array(terms, w7, prm, c):
    """the host array of the C ABI (include/fplx.h) as a list of floats"""
    cw = [1.0] * c if prm["class_weight"] is None else list(prm["class_weight"])
    return ([float(t) for t in terms] + [float(t) for t in w7] +
            [prm["beta"], prm["gamma_nr"], prm["w_dice_el"], prm["gamma_el"], prm["q"], prm["epsilon"],
             1.0 if prm["use_pw"] else 0.0] + cw)


def _f32(x):
    return float(np.float32(x))


def _prm32(prm, c):
    """the parameters as the kernels receive them (floats)"""
    q = {k: _f32(prm[k]) for k in ("beta", "gamma_nr", "w_dice_el", "gamma_el", "q", "epsilon")}
    q["use_pw"] = bool(prm["use_pw"])
    cw = prm["class_weight"]
    q["cw"] = np.ones(c) if cw is None else np.asarray([_f32(t) for t in cw], np.float64)
    return q


def _slsr_label(yy, w, has_pw, eps, dt):
    if not has_pw:
        return yy
    sm = (yy - dt(0.5)) * (dt(0.5) - dt(eps)) / dt(0.5) + dt(0.5)
    return np.where(w > 0, sm, yy)


# ---------------------------------------------------------------- the three stages of the C ABI

def sums_ext(lg, y, pw, softmax, w7, prm, dt=np.float64, mut=None):
    """fplx_seg_loss_ext_sums -> sums [N, 10C + 7] float64 (terms whose weight is 0 leave their entries 0, as the kernel does)"""
    n, c, v = lg.shape
    rm = mut if mut in _ROW_MUT else None
    q = _prm32(prm, c)
    W = dict(zip(EXT_TERMS, w7))
    out = np.zeros((n, ext_k(c)))
    out[:, :6 * c + 3] = LO.sums(lg, y, pw, softmax, dt, rm)
    l, yy = lg.astype(dt), y.astype(dt)
    w = np.ones((n, v), dt) if pw is None else pw.astype(dt)
    p = LO._softmax(l) if softmax else l
    red = lambda x: LO._reduce(x, dt, rm)
    d = p - yy
    k0, s0 = 6 * c + 3, 10 * c + 3
    c99 = dt(0.999 if mut == "explog_999" else 0.99)
    for k in range(c):
        out[:, k0 + 4 * k] = red(p[:, k])
        out[:, k0 + 4 * k + 1] = red(yy[:, k] * p[:, k])
        if W["noise_robust"]:
            out[:, k0 + 4 * k + 2] = red(np.abs(d[:, k]) ** dt(q["gamma_nr"]))
        if W["explog"]:
            out[:, k0 + 4 * k + 3] = red(yy[:, k] * (-np.log(dt(0.005) + p[:, k] * c99)) ** dt(q["gamma_el"]))
    if W["gce"]:
        g = np.zeros((n, v), dt)
        for k in range(c):
            g = g + (dt(1.0) - p[:, k] ** dt(q["q"])) / dt(q["q"]) * yy[:, k] * dt(q["cw"][k])
        out[:, s0] = red(g * w if q["use_pw"] else g)
    if W["mse"] or W["mae"]:
        s2, s1 = np.zeros((n, v), dt), np.zeros((n, v), dt)
        for k in range(c):
            s2, s1 = s2 + d[:, k] * d[:, k], s1 + np.abs(d[:, k])
        out[:, s0 + 1], out[:, s0 + 2] = red(s2), red(s1)
    if W["slsr"]:
        s = np.zeros((n, v), dt)
        for k in range(c):
            s = s - _slsr_label(yy[:, k], w, pw is not None, q["epsilon"], dt) * np.log(p[:, k] * dt(0.999) + dt(5e-4))
        out[:, s0 + 3] = red(s)
    return out


COEF_KEYS = ("Ag", "Bg", "cce", "cent", "Au", "Bu", "cnr", "cel", "cgce", "cmse2", "cmae", "cslsr")


def from_sums_ext(sm, totals, n_global, v, has_pw, terms, w7, prm, dt=np.float64, mut=None):
    """fplx_seg_loss_ext_from_sums -> (out [4 + C + 7], coef dict) in double; the fp32 restatement rounds both to float.  The
    image-weighted Dice is the first family's alone (lossoracle): terms[2] must be 0 here."""
    n, kk = sm.shape
    c = (kk - 7) // 10
    assert terms[2] == 0
    q = _prm32(prm, c)
    wf, wn, we, wg, wa, ws, wl = [_f32(t) for t in w7]
    t = np.asarray(totals, np.float64).reshape(-1)
    o0, c0 = LO.from_sums(sm[:, :6 * c + 3], t[:6 * c + 3], None, n_global, v, has_pw, terms, np.float64)
    T6 = t[:6 * c].reshape(c, 6)
    X = t[6 * c + 3:10 * c + 3].reshape(c, 4)
    M = n_global * float(v)
    Y, P, I, NR, E = T6[:, 3], X[:, 0], X[:, 1], X[:, 2], X[:, 3]
    if mut == "focal_weighted_p":
        Pf = T6[:, 1]
    else:
        Pf = P
    ext = np.zeros(7)
    Au, Bu, cnr, cel = np.zeros(c), np.zeros(c), np.zeros(c), np.zeros(c)
    mag = np.zeros(7)                                                    # un-cancelled magnitude of each value
    den, num = Y + P + 1e-5, 2.0 * I + 1e-5
    dice = num / den
    if wf != 0:
        denf = Y + Pf + 1e-5
        dcf = num / denf
        ext[0] = 1.0 - (dcf ** (1.0 / q["beta"])).sum() / c
        mag[0] = 1.0 + (dcf ** (1.0 / q["beta"])).sum() / c
        k = wf / (c * q["beta"]) * dcf ** (1.0 / q["beta"] - 1.0)
        Au, Bu = Au + k * (-2.0 / denf), Bu + k * (num / (denf * denf))
    if wn != 0:
        ext[1] = (NR / den).sum() / c
        mag[1] = ext[1]
        cnr = wn * q["gamma_nr"] / (c * den)
        Bu = Bu - wn * NR / (c * den * den)
    if we != 0:
        s = 0.005 + dice * 0.99
        ls = -np.log(s)
        k = we * q["w_dice_el"] / c * q["gamma_el"] * ls ** (q["gamma_el"] - 1.0) * 0.99 / s
        Au, Bu = Au + k * (-2.0 / den), Bu + k * (num / (den * den))
        wc = (1.0 / (Y / M + (0.0 if mut == "wc_no_01" else 0.1))) ** 0.5
        ext[2] = (ls ** q["gamma_el"]).sum() / c * q["w_dice_el"] + (wc * E).sum() / M * (1.0 - q["w_dice_el"])
        mag[2] = abs(ext[2]) + (ls ** q["gamma_el"]).sum() / c * abs(q["w_dice_el"])
        cel = we * (1.0 - q["w_dice_el"]) * wc / M * q["gamma_el"]
    gnorm = 1.0 / t[6 * c + 1] if q["use_pw"] else 1.0 / M
    mc = M if mut == "mse_div_m" else M * c
    S = t[10 * c + 3:]
    ext[3], ext[4], ext[5], ext[6] = (wg != 0) * S[0] * gnorm, (wa != 0) * S[2] / mc, (ws != 0) * S[1] / mc, (wl != 0) * S[3] / M
    mag[3:] = np.abs(ext[3:])
    w7f = np.asarray([wf, wn, we, wg, wa, ws, wl])
    total = o0[0] + (w7f * ext).sum()
    out = np.concatenate([[total], o0[1:], ext])
    coef = dict(Ag=c0["Ag"][0].copy(), Bg=c0["Bg"][0].copy(), cce=c0["cce"], cent=c0["cent"], Au=Au, Bu=Bu, cnr=cnr, cel=cel,
                cgce=wg * gnorm, cmse2=2.0 * ws / mc, cmae=wa / mc, cslsr=wl / M)
    coef["total_mag"] = c0["dice_mag"] + abs(terms[1]) * abs(o0[2]) + abs(terms[3]) * abs(o0[3]) + (np.abs(w7f) * mag).sum()
    coef["ext_mag"] = mag
    if dt == np.float32:
        out = out.astype(np.float32).astype(np.float64)
        for k in COEF_KEYS:
            coef[k] = np.asarray(coef[k], np.float32)
    return out, coef


def _terms_g(lg, y, pw, coef, terms, w7, prm, softmax, dt, mut=None):
    """per class: the gradient with respect to the prediction, every term (g), the entropy term's own (ge, softmax = 0), p, q"""
    n, c, v = lg.shape
    pr = _prm32(prm, c)
    W = dict(zip(EXT_TERMS, w7))
    l, yy = lg.astype(dt), y.astype(dt)
    w = (np.ones((n, v), dt) if pw is None else pw.astype(dt))[:, None]
    qs = LO._softmax(l)
    p = qs if softmax else l
    cv = lambda k: np.asarray(coef[k]).astype(dt).reshape(1, c, 1)
    sc = lambda k: dt(coef[k])
    g = np.zeros_like(l)
    ge = np.zeros_like(l)
    if terms[0] != 0:
        g = g + w * (cv("Ag") * yy + cv("Bg"))
    if terms[1] != 0:
        g = g - sc("cce") * w * yy * dt(0.999) / (p * dt(0.999) + dt(5e-4))
    if terms[3] != 0:
        ge = -sc("cent") * (np.log2(qs + dt(1e-10)) + qs * dt(INV_LN2) / (qs + dt(1e-10)))
    if W["focal"] or W["noise_robust"] or W["explog"]:
        g = g + (cv("Au") * yy + cv("Bu"))
    d = p - yy
    sg = np.sign(d)
    if mut == "sign0_one":
        sg = np.where(d == 0, dt(1.0), sg)
    with np.errstate(divide="ignore", invalid="ignore"):
        if W["noise_robust"]:
            g = g + cv("cnr") * np.abs(d) ** dt(dt(pr["gamma_nr"]) - dt(1.0)) * sg
        if W["mse"]:
            g = g + sc("cmse2") * d
        if W["mae"]:
            g = g + sc("cmae") * sg
        if W["explog"]:
            s = dt(0.005) + p * dt(0.999 if mut == "explog_999" else 0.99)
            g = g - cv("cel") * yy * (-np.log(s)) ** dt(dt(pr["gamma_el"]) - dt(1.0)) * dt(0.99) / s
        if W["gce"]:
            wg = w if pr["use_pw"] else dt(1.0)
            ex = dt(pr["q"]) if mut == "gce_q" else dt(dt(pr["q"]) - dt(1.0))
            g = g - sc("cgce") * wg * pr["cw"].astype(dt).reshape(1, c, 1) * yy * p ** ex
        if W["slsr"]:
            g = g - sc("cslsr") * _slsr_label(yy, w, pw is not None, pr["epsilon"], dt) * dt(0.999) / (p * dt(0.999) + dt(5e-4))
    return g, ge, p, qs


def bwd_ext(lg, y, pw, coef, gscale, terms, w7, prm, softmax, dt=np.float64, mut=None):
    """fplx_seg_loss_ext_bwd -> dlogits [N, C, V]"""
    g, ge, p, qs = _terms_g(lg, y, pw, coef, terms, w7, prm, softmax, dt, mut)
    gs = dt(gscale)
    if softmax:
        g = g + ge
        return gs * (p * (g - (g * p).sum(1, keepdims=True)))
    return gs * (g + qs * (ge - (ge * qs).sum(1, keepdims=True)))


def restate_ext(lg, y, pw, terms, w7, prm, softmax=True, gscale=1.0, mut=None, shards=1, dt=np.float32):
    """the kernels' arithmetic in fp32 numpy: sums -> from_sums -> bwd, optionally over `shards` equal ranks whose totals are
    added in float64 -> (sums, totals, [out of each rank], dlogits)"""
    n, c, v = lg.shape
    per = n // shards
    sl = [slice(i * per, (i + 1) * per) for i in range(shards)]
    sub = lambda a, s: None if a is None else a[s]
    sms = [sums_ext(lg[s], y[s], sub(pw, s), softmax, w7, prm, dt, mut) for s in sl]
    totals = np.sum([s.sum(0) for s in sms], axis=0)
    outs, dls = [], []
    for s, sm in zip(sl, sms):
        out, coef = from_sums_ext(sm, totals, n, v, pw is not None, terms, w7, prm, dt, mut)
        outs.append(out)
        dls.append(bwd_ext(lg[s], y[s], sub(pw, s), coef, np.float32(gscale), terms, w7, prm, softmax, dt, mut).astype(np.float64))
    return np.concatenate(sms), totals, outs, np.concatenate(dls)


# ---------------------------------------------------------------- float64 autograd of the definitions

def torch_losses(P, Y, W, prm, c):
    """the seven losses on predictions P [M, C] (float64 tensors), labels Y [M, C], weights W [M] or None, written with torch
    operations from the table in the module docstring -> list of seven scalars"""
    q = _prm32(prm, c)
    cw = torch.from_numpy(q["cw"])
    M = P.shape[0]
    dice = (2.0 * (Y * P).sum(0) + 1e-5) / (Y.sum(0) + P.sum(0) + 1e-5)
    focal = 1.0 - torch.pow(dice, 1.0 / q["beta"]).mean()
    nr = (torch.pow(torch.abs(P - Y), q["gamma_nr"]).sum(0) / ((P + Y).sum(0) + 1e-5)).mean()
    wc = torch.pow(1.0 / (Y.mean(0) + 0.1), 0.5)
    el = (torch.pow(-torch.log(0.005 + dice * 0.99), q["gamma_el"]).mean() * q["w_dice_el"] +
          (Y * wc * torch.pow(-torch.log(0.005 + P * 0.99), q["gamma_el"])).sum(1).mean() * (1.0 - q["w_dice_el"]))
    gce = ((1.0 - torch.pow(P, q["q"])) / q["q"] * Y * cw).sum(1)
    gce = (gce * W).sum() / W.sum() if q["use_pw"] else gce.mean()
    mae, mse = torch.abs(P - Y).mean(), torch.square(P - Y).mean()
    sy = Y
    if W is not None:
        m = (W > 0).to(Y.dtype)[:, None]
        sy = m * ((Y - 0.5) * (0.5 - q["epsilon"]) / 0.5 + 0.5) + (1 - m) * Y
    slsr = (-(sy * torch.log(P * 0.999 + 5e-4)).sum(1)).mean()
    return [focal, nr, el, gce, mae, mse, slsr]


def autograd_ext(lg, y, pw, terms, w7, prm, softmax, gscale=1.0):
    """float64 autograd of the whole mixture -> (out [4 + C + 7], dlogits)"""
    n, c, v = lg.shape
    ao, ah, adl = LO.autograd(lg, y, pw, None, terms, softmax, gscale)
    L = torch.from_numpy(lg.astype(np.float64)).requires_grad_(True)
    P = torch.softmax(L, 1) if softmax else L
    P2 = P.permute(0, 2, 1).reshape(-1, c)
    Y2 = torch.from_numpy(y.astype(np.float64)).permute(0, 2, 1).reshape(-1, c)
    W2 = None if pw is None else torch.from_numpy(pw.astype(np.float64)).reshape(-1)
    vals = torch_losses(P2, Y2, W2, prm, c)
    tot = torch.zeros((), dtype=torch.float64)
    ext = np.zeros(7)
    for i, (wt, val) in enumerate(zip(w7, vals)):
        if wt != 0:
            tot = tot + _f32(wt) * val
            ext[i] = val.item()
    if tot.requires_grad:
        (tot * float(gscale)).backward()
        adl = adl + L.grad.numpy()
    out = np.concatenate([[ao[0] + tot.item()], ao[1:], ah, ext])
    return out, adl


# ---------------------------------------------------------------- the reference with its bounds

def _coef_vec(out, coef):
    return np.concatenate([np.ravel(out)] + [np.ravel(np.asarray(coef[k], np.float64)) for k in COEF_KEYS])


def reference_ext(lg, y, pw, terms, w7, prm, softmax=True, gscale=1.0, n_global=None):
    """float64 values and the bounds of oracle B for ONE mixture over the batch (lg, y [N, C, V]; pw [N, V] or None)"""
    n, c, v = lg.shape
    ng = n if n_global is None else n_global
    pr = _prm32(prm, c)
    W = dict(zip(EXT_TERMS, [_f32(t) for t in w7]))
    assert float(y.min()) >= 0 and (pw is None or float(pw.min()) >= 0)
    assert not W["noise_robust"] or 1.0 <= pr["gamma_nr"] <= 2.0, "the gradient bound of |d|^g is derived for 1 <= g <= 2"
    r = LO.Ref()
    gscale = _f32(gscale)
    sm = sums_ext(lg, y, pw, softmax, w7, prm)
    r.sums, r.totals = sm, sm.sum(0)
    out, coef = from_sums_ext(sm, r.totals, ng, v, pw is not None, terms, w7, prm)
    dl = bwd_ext(lg, y, pw, coef, gscale, terms, w7, prm, softmax)
    if ng == n:
        ao, adl = autograd_ext(lg, y, pw, terms, w7, prm, softmax, gscale)
        assert np.allclose(ao, out, rtol=1e-11, atol=1e-13), (ao, out)
    # ---- per-voxel quantities
    l64, y64 = lg.astype(np.float64), y.astype(np.float64)
    D = (l64.max(1, keepdims=True) - l64.min(1, keepdims=True)) if softmax or terms[3] != 0 else np.zeros((n, 1, v))
    assert float(D.max()) < 80.0, "underflowing probabilities are excluded from this oracle"
    dp = 2.0 * D + 4.0 * E_EXP + c + 1
    dpm = float(dp.max())
    ra = LO.row_terms(v) / 256 + 9
    dsum = dpm + ra + 3
    w = (np.ones((n, v)) if pw is None else pw.astype(np.float64))[:, None]
    qs = LO._softmax(l64)
    p = qs if softmax else l64
    ep = dp * U * np.abs(p) if softmax else np.zeros_like(p)
    d = p - y64
    ad = np.abs(d)
    ed = ep + U * ad
    # ---- sums
    base = LO.reference(lg, y, pw, None, terms, softmax, gscale, use_autograd=False)
    sb = GAMMA_SLACK * dsum * U * np.abs(sm) + v * ETA
    sb[:, :6 * c + 3] = base.sums_bound
    k0, s0 = 6 * c + 3, 10 * c + 3
    rs = lambda x: x.reshape(n, -1).sum(1)
    gn, gl, qq = pr["gamma_nr"], pr["gamma_el"], pr["q"]
    s = 0.005 + p * 0.99
    Lg = -np.log(s)
    eL = 0.99 * ep / s + (E_LOG * np.abs(Lg) + 3) * U
    for k in range(c):
        if W["noise_robust"]:
            e = gn * np.maximum(ad[:, k], ed[:, k]) ** (gn - 1) * ed[:, k] + (E_POW + 1) * U * ad[:, k] ** gn
            sb[:, k0 + 4 * k + 2] = GAMMA_SLACK * (rs(e) + (ra + c) * U * rs(ad[:, k] ** gn)) + v * ETA
        if W["explog"]:
            e = y64[:, k] * (abs(gl) * Lg[:, k] ** (gl - 1) * eL[:, k] + (E_POW + 2) * U * Lg[:, k] ** gl)
            sb[:, k0 + 4 * k + 3] = GAMMA_SLACK * (rs(e) + (ra + c) * U * rs(y64[:, k] * Lg[:, k] ** gl)) + v * ETA
    cwv = pr["cw"].reshape(1, c, 1)
    wgv = w if pr["use_pw"] else np.ones_like(w)
    if W["gce"]:
        pq = np.abs(p) ** qq
        m = cwv * y64 * wgv / qq
        e = m * ((E_POW + qq * dp) * U * pq + 6 * U * (1 + pq))
        sb[:, s0] = GAMMA_SLACK * (rs(e) + (ra + c) * U * rs(m * (1 + pq))) + v * ETA
    if W["mse"] or W["mae"]:
        sb[:, s0 + 1] = GAMMA_SLACK * (rs(2 * ad * ed + 2 * U * d * d) + (ra + c) * U * rs(d * d)) + v * ETA
        sb[:, s0 + 2] = GAMMA_SLACK * (rs(ed) + (ra + c) * U * rs(ad)) + v * ETA
    sy = _slsr_label(y64, w, pw is not None, pr["epsilon"], np.float64)
    lgs = np.abs(np.log(p * 0.999 + 5e-4))
    if W["slsr"]:
        sb[:, s0 + 3] = GAMMA_SLACK * U * ((2 * E_LOG + c + 7 + ra) * rs(sy * lgs) + (dpm + 7) * rs(sy)) + v * ETA
    r.sums_bound = sb
    tb = sb.sum(0) * (ng / float(n))           # the other ranks' samples carry the same kind of error
    r.totals_bound = sb.sum(0)
    # ---- values and coefficients: the totals' error through the derivative (central differences in float64)
    f0 = _coef_vec(out, coef)
    err = np.zeros_like(f0)
    for j in range(ext_k(c)):
        if tb[j] == 0:
            continue
        h = max(abs(r.totals[j]) * 1e-6, 1e-9)
        tp, tm = r.totals.copy(), r.totals.copy()
        tp[j] += h
        tm[j] -= h
        fp = _coef_vec(*from_sums_ext(sm, tp, ng, v, pw is not None, terms, w7, prm))
        fm = _coef_vec(*from_sums_ext(sm, tm, ng, v, pw is not None, terms, w7, prm))
        err += np.abs(fp - fm) / (2 * h) * tb[j]
    err = GAMMA_SLACK * err + 2 * U * np.abs(f0) + ETA
    no = out.size
    ob = err[:no].copy()
    ob[0] += U * coef["total_mag"]
    ob[1:4] = np.maximum(ob[1:4], base.out_bound[1:4])
    ob[4:4 + c] = np.maximum(ob[4:4 + c], base.out_bound[4:])
    ob[0] = max(ob[0], ob[1] + abs(terms[1]) * ob[2] + abs(terms[3]) * ob[3] +
                float((np.abs(np.asarray(w7, np.float64)) * (ob[4 + c:] + U * coef["ext_mag"])).sum()) + U * coef["total_mag"])
    r.out, r.out_bound = out, ob
    dc, off = {}, no
    for k in COEF_KEYS:
        sz = np.size(coef[k])
        dc[k] = err[off:off + sz].reshape(np.shape(coef[k]))
        off += sz
    # ---- gradient
    cv = lambda a: np.asarray(a, np.float64).reshape(1, c, 1)
    G, Eg = np.zeros_like(p), np.zeros_like(p)
    nterm = 0

    def add(mag, e):
        nonlocal G, Eg, nterm
        G, Eg, nterm = G + mag, Eg + e, nterm + 1
    if terms[0] != 0:
        add(w * (np.abs(cv(coef["Ag"])) * y64 + np.abs(cv(coef["Bg"]))),
            w * (cv(dc["Ag"]) * y64 + cv(dc["Bg"])) + 3 * U * w * (np.abs(cv(coef["Ag"])) * y64 + np.abs(cv(coef["Bg"]))))
    rel = lambda k: dc[k] / max(abs(float(coef[k])), 1e-300)
    if terms[1] != 0:
        t = np.abs(coef["cce"]) * w * y64 * 0.999 / (np.abs(p) * 0.999 + 5e-4)
        add(t, t * (rel("cce") + 8 * U + 0.999 * ep / (np.abs(p) * 0.999 + 5e-4)))
    if W["focal"] or W["noise_robust"] or W["explog"]:
        add(np.abs(cv(coef["Au"])) * y64 + np.abs(cv(coef["Bu"])),
            cv(dc["Au"]) * y64 + cv(dc["Bu"]) + 3 * U * (np.abs(cv(coef["Au"])) * y64 + np.abs(cv(coef["Bu"]))))
    flip = (ad <= ed) & (ad > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        if W["noise_robust"]:
            pw1 = np.where(ad > 0, ad ** (gn - 1), 1.0 if gn == 1 else 0.0)
            hold = ed ** (gn - 1) if gn > 1 else np.zeros_like(ed)
            lin = np.where(ad > 0, 2 * (gn - 1) * ad ** (gn - 2) * ed, np.inf) if gn > 1 else np.zeros_like(ed)
            add(np.abs(cv(coef["cnr"])) * pw1,
                cv(dc["cnr"]) * pw1 + np.abs(cv(coef["cnr"])) * (np.minimum(hold, lin) + (E_POW + 4) * U * pw1 + flip * pw1))
        if W["mse"]:
            add(abs(float(coef["cmse2"])) * ad, dc["cmse2"] * ad + abs(float(coef["cmse2"])) * (ep + 3 * U * ad))
        if W["mae"]:
            add(abs(float(coef["cmae"])) * (ad > 0), dc["cmae"] + abs(float(coef["cmae"])) * flip)
        if W["explog"]:
            t = np.abs(cv(coef["cel"])) * y64 * Lg ** (gl - 1) * 0.99 / s
            relc = cv(dc["cel"]) / np.maximum(np.abs(cv(coef["cel"])), 1e-300)
            add(t, t * (relc + abs(gl - 1) * eL / Lg + 0.99 * ep / s + (E_POW + 8) * U))
        if W["gce"]:
            t = np.where(y64 > 0, abs(float(coef["cgce"])) * wgv * cwv * y64 * np.abs(p) ** (qq - 1), 0.0)
            add(t, t * (rel("cgce") + abs(qq - 1) * (dp * U if softmax else 0.0) + (E_POW + 6) * U))
        if W["slsr"]:
            t = abs(float(coef["cslsr"])) * sy * 0.999 / (np.abs(p) * 0.999 + 5e-4)
            add(t, t * (rel("cslsr") + 12 * U + 0.999 * ep / (np.abs(p) * 0.999 + 5e-4)))
    Ge = np.zeros_like(p)
    Ege = np.zeros_like(p)
    if terms[3] != 0:
        lq = np.abs(np.log2(qs + 1e-10)) + INV_LN2
        Ge = np.abs(coef["cent"]) * lq
        eq = dp * U * qs
        Ege = Ge * (rel("cent") + (2 * E_LOG + 6) * U) + np.abs(coef["cent"]) * 3 * INV_LN2 * eq / (qs + 1e-10)
    ags = abs(gscale)
    jac = (2 * dp + 2 * c + 16) * U
    if softmax:
        G, Eg = G + Ge, Eg + Ege
        S = ags * p * (G + (p * G).sum(1, keepdims=True))
        bound = ags * p * (Eg + (p * Eg).sum(1, keepdims=True)) + jac * S
    else:
        Se = ags * qs * (Ge + (qs * Ge).sum(1, keepdims=True))
        S = ags * G + Se
        bound = ags * (Eg + (nterm + 2) * U * G) + ags * qs * (Ege + (qs * Ege).sum(1, keepdims=True)) + jac * Se + U * S
    r.S = S
    r.dl_bound = GAMMA_SLACK * bound + ETA
    if ng == n:
        scale = max(float(S.max()), 1e-300)
        assert float(np.abs(adl - dl).max()) <= 1e-11 * scale, "closed-form gradient differs from autograd"
        r.out, r.dl = ao, adl
    else:
        r.dl = dl
    return r


def check_B(r, out=None, dl=None, sm=None, totals=None, what=""):
    """oracle B: each given output against the reference -> dict of worst error / bound ratios (asserted <= 1)"""
    res = {}
    if out is not None:
        res["out"] = LO.ratio(out, r.out, r.out_bound)
    if dl is not None:
        res["dlogits"] = LO.ratio(dl, r.dl, r.dl_bound)
    if sm is not None:
        res["sums"] = LO.ratio(sm, r.sums, r.sums_bound)
    if totals is not None:
        res["totals"] = LO.ratio(totals, r.totals, r.totals_bound)
    bad = {k: v for k, v in res.items() if not v <= 1.0}
    assert not bad, "%s: error / bound = %s" % (what, bad)
    return res


# ---------------------------------------------------------------- oracle A

def exact_cols_ext(c):
    """the entries of a sums row that oracle A compares: unweighted Y, P, I per class, sum (p - y)^2, sum |p - y|"""
    cols = []
    for k in range(c):
        cols += [6 * k + 3, 6 * c + 3 + 4 * k, 6 * c + 3 + 4 * k + 1]
    return cols + [10 * c + 4, 10 * c + 5]


def exact_pre_ext(pr, y):
    """precondition of oracle A, asserted on the data: p a multiple of 2^-6 in [0, 1], y in {0, 1}, and per partial row the sum
    of the magnitudes of every compared entry, in units of 2^-12, below 2^24 -> the largest such sum"""
    n, c, v = pr.shape
    assert np.isin(y, (0.0, 1.0)).all()
    assert np.array_equal(pr * 64, np.round(pr * 64)) and pr.min() >= 0 and pr.max() <= 1
    p, yy = pr.astype(np.float64), y.astype(np.float64)
    row = LO.row_of(v)
    worst = 0.0
    d = p - yy
    for x in [(d * d).sum(1), np.abs(d).sum(1)] + [p[:, k] for k in range(c)] + [yy[:, k] for k in range(c)]:
        for rr in range(LO.loss_rows(v)):
            worst = max(worst, float(np.abs(x[:, row == rr]).sum(1).max()) * 4096.0)
    assert worst < LO.EXACT_LIMIT, "a row's sum of |terms| reaches %g units >= 2^24" % worst
    return worst


def check_A(sm_got, totals_got, pr, y, pw, what=""):
    """oracle A on fplx_seg_loss_ext_sums' sums / totals (softmax = 0, MSE and MAE asked for) -> number of entries compared"""
    exact_pre_ext(pr, y)
    c = pr.shape[1]
    ref = sums_ext(pr, y, pw, False, weights(mse=1.0, mae=1.0), PRM)
    cols = exact_cols_ext(c)
    sm_got = np.asarray(sm_got, np.float64)
    bad = ~(sm_got[:, cols] == ref[:, cols])
    assert not bad.any(), "%s: %d of %d exact sums differ (first: got %r, want %r)" % (
        what, int(bad.sum()), bad.size, sm_got[:, cols][bad][0], ref[:, cols][bad][0])
    if totals_got is not None:
        assert np.array_equal(np.asarray(totals_got, np.float64)[cols], ref.sum(0)[cols]), "%s: totals differ" % what
    return bad.size
