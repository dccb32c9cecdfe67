"""Float64 oracles for the weakly-supervised kernels (fpl-plus_amd/csrc/wsl.hip), on top of tests/lossoracle.py as
tests/ssloracle.py is: same notation (u = 2^-24, ETA, E_EXP, E_LOG, dp(D), GAMMA_SLACK) and NO new measured constant.

The passes under test.  Logits [N, C, D, H, W], image [N, Ci, D, H, W]; p = softmax over C (softmax = 0: the input itself); a slice
is an (n, d) plane; S = N D slices.
    gatedcrf   k_ij = sum_desc w exp(-1/2 (|xy_i - xy_j|^2 / sxy^2 + sum_ch (I_i - I_j)^2 / srgb^2)) for the (2 r + 1)^2 - 1 window
               positions j != i; a j outside the slice has xy = 0, I = 0, p = 0 (the reference's zero-padded unfold);
               out0 = sum_i sum_j k_ij (1 - p(i) . p(j)), out3 = S H W, loss = out0 / out3; kp_c(i) = sum_{j inside} k_ij p_c(j);
               dL/dp_c(i) = -2 kp_c(i) / out3 (k is symmetric between pixels of the slice)
    tv         p' = 0.999 p + 5e-4; e = min of p' over the in-bounds 3x3x3 window; o = max of e over the window;
               out0 = sum relu(o - e), loss = out0 / (N C V); count: +1 at the p' voxel whose value o_v is, -1 at the argmin of v's
               own window, for every v with o_v - e_v > 0; dL/dp_c = 0.999 count_c / (N C V)
    mumford    per slice, class c, channel ch: cen = sum I p / sum p; out0 = sum (I - cen)^2 p; out1 = sum of |forward differences|
               of p along H and W (l2: their squares); loss = (out0 + lambda out1) / (N C V);
               dL/dp_c(v) = (sum_ch (I - cen)^2 + lambda stencil) / (N C V) - the centroid's own derivative vanishes
    then dlogits_c = gs p_c (e_c - sum_j p_j e_j) with e = dL/dp (softmax = 0: gs e_c).
Each closed form is asserted in every call against float64 autograd of the reference's own statements written with torch
operations (F.unfold: gatedcrf.py:52-102, 121-169; max_pool3d: loss/seg/ssl.py:76-86; the channel loop: mumford_shah.py:32-95),
1e-11 of the magnitude.

Rounding bounds.  ep = dp u p is the absolute error of a probability (0 with softmax = 0), ra(n) = row_terms(n) / 256 + 12 the
additions between a term and its double sum (ssloracle.ra_ssl).  Every bound is multiplied by GAMMA_SLACK.
    gatedcrf   One Gaussian factor exp(-a), a = a_xy + a_rgb:  1 / sigma^2 is formed in double and rounded once (u); a_xy = d2 ixy / 2
               with d2 an exact integer: 2 u a_xy;  a_rgb: a difference of exact inputs (u), its square (3 u), Ci additions, the
               product with irgb and irgb's own rounding: (5 + Ci) u a_rgb;  two exponentials (the xy table, the rgb factor), their
               product and the weight: (2 E_EXP + 2) u.  rel = 2 a_xy + (5 + Ci) a_rgb + 2 E_EXP + 2 [u], plus 4 ETA |w| for a factor
               that underflows.  A position outside the slice: a = (h^2 + w^2) ixy / 2 + sum I^2 irgb / 2 in one exponential:
               rel = (5 + Ci) a + E_EXP + 1.  k: the descriptors' errors plus nk u |k|.
               dot = p(i) . p(j): sum_c (p_i ep_j + p_j ep_i) + (C + 1) u dot;  T = k (1 - dot):
               eT = ek |1 - dot| + k (e_dot + u |1 - dot|) + u |T|;  a lane adds its (2 r + 1)^2 - 1 terms one after the other, then
               the block's 6 shuffles and 3 additions: out0: sum eT + ((2 r + 1)^2 + 9) u sum |T|.
               kp_c(i): sum_j (ek p_j + k ep_j) + (2 r + 1)^2 u sum_j |k| p_j.
    tv         p': epp = 0.999 ep + 4 u p' (ssloracle's entropy).  min and max are 1-Lipschitz in the sup norm: the error of e_v is at
               most the largest epp in its window, that of o_v the largest of those in its window;  contour: eo + ee + u contour;
               out0: their sum + ra(V) u out0.  The sum needs no decision.  The COUNT does: a voxel is UNDECIDED when the runner-up
               of its argmin (another p' voxel), or of its max of minima (a minimum that comes from another p' voxel - one minimum
               serves many windows, and such ties are the same voxel), is within twice the error, or when its contour is positive
               but within the error.  An undecided voxel can move counts only inside its 5x5x5 neighbourhood: these entries are
               taken out of the count comparison, and the sum's bound grows by the undecided voxels' own errors once more.
               `check_tv_case` asserts at most MAX_UNDECIDED (1 %, ssloracle) undecided voxels before anything is compared.
    mumford    S0 = sum p: sum ep + ra(HW) u S0;  S1 = sum I p: sum |I| ep + (ra(HW) + 1) u sum |I| p;  cen = S1 / S0 in double,
               rounded once: ecen = eS1 / S0 + |cen| eS0 / S0 + u |cen|.  t = I - cen: et = ecen + u |t|;  t t:
               et2 = 2 |t| et + et^2 + u (|t| + et)^2 - in full, because a one-pixel slice has I = cen and the first-order term
               vanishes;  t t p: t^2 ep + (p + ep) et2 + u (t^2 + et2) p;  a lane adds C Ci terms per pixel: out0: the sum + (C Ci row_terms(HW) / 256
               + 12) u sum.  A difference d = q - p: ed = ep_q + ep_p + u |d| (l2: 2 |d| ed + u d^2); a lane adds 2 C terms per
               pixel: out1: the sum + (2 C row_terms(HW) / 256 + 12) u sum.
               Gradient: lev_c = sum_ch t^2: sum et2 + Ci u (lev + sum et2);  stencil, l1: a sign is undecided (slack 2) where
               |d| <= ed, else exact;  l2: 2 ed per difference + 4 u sum |2 d|;  (lev + lambda st) / numel: 4 u more.
    gradients  E = |e| on un-cancelled magnitudes, ee its error; S_c = |gs| p_c (E_c + sum_j p_j E_j);
               |err| <= |gs| p_c (ee_c + sum_j (p_j ee_j + dp u p_j E_j)) + (dp + C + 5) u S_c + ETA (1 + |gs| (E_c + sum E))
               (ssloracle's consistency gradient);  softmax = 0: |gs| (ee_c + u E_c) + ETA.

Pure numpy / torch on the CPU; tests/test_wsl_cpu.py checks the oracle itself, tests/test_gpu_wsl.py applies it."""
import numpy as np
import torch
import torch.nn.functional as F

import lossoracle as LO
import ssloracle as SO
from lossoracle import U, ETA, E_EXP, E_LOG, GAMMA_SLACK, ratio  # noqa: F401

MAX_UNDECIDED = SO.MAX_UNDECIDED
MUTATIONS = ("crf_centre", "crf_drop_oob", "crf_sigma", "crf_grad2", "tv_999", "tv_2d", "tv_swap", "ms_volume", "ms_l1l2", "ms_numel")
DEFAULT_DESC = ((1.0, 5.0, 0.1), (1.0, 3.0, 0.0))          # the agent's pair: {w0, xy0, rgb}, {w1, xy1}


class Ref(object):
    pass


def ra(n):
    return LO.row_terms(n) / 256 + 12


# ---------------------------------------------------------------- generators

def logits_case(key, n, c, d, h, w, ci=1, scale=1.5):
    """-> logits [N, C, D, H, W] (standard deviation about 1.58, as ssloracle.logits_case), image [N, Ci, D, H, W] in [0, 1] with
    structure (a ramp and a blob plus noise), float32"""
    g = LO.rng(key)
    lg = g.standard_normal((n, c, d, h, w)) * scale + g.standard_normal((n, c, d, h, w)) * 0.5
    yy, xx = np.mgrid[0:h, 0:w]
    base = 0.5 + 0.3 * np.sin(0.7 * yy + 0.3) * np.cos(0.5 * xx)
    im = base[None, None, None] + 0.15 * g.standard_normal((n, ci, d, h, w))
    f = lambda a: np.ascontiguousarray(a.astype(np.float32))
    return f(lg), f(np.clip(im, 0.0, 1.0))


def tv_exact_case(key, n, c, d, h, w):
    """softmax = 0: every (n, c) row a random permutation of 0 .. V - 1 times 2^-14 - distinct values"""
    g = LO.rng(key)
    v = d * h * w
    assert v <= 1 << 14
    x = np.stack([g.permutation(v) for _ in range(n * c)]).astype(np.float32) / np.float32(16384.0)
    return np.ascontiguousarray(x.reshape(n, c, d, h, w))


def dyadic_case(key, n, c, d, h, w, ci):
    """softmax = 0: p multiples of 2^-6 in [0, 1], I multiples of 2^-4 in [0, 2]"""
    g = LO.rng(key)
    p = (g.integers(0, 65, (n, c, d, h, w)) / 64.0).astype(np.float32)
    im = (g.integers(0, 33, (n, ci, d, h, w)) / 16.0).astype(np.float32)
    return p, im


def one_hot_case(key, n, c, d, h, w, ci):
    g = LO.rng(key)
    idx = g.integers(0, c, (n, d, h, w))
    p = np.zeros((n, c, d, h, w), np.float32)
    np.put_along_axis(p, idx[:, None], 1.0, 1)
    return p, logits_case(key + ".im", n, c, d, h, w, ci)[1]


# ---------------------------------------------------------------- shared pieces

def _probs(x, softmax):
    x = np.asarray(x, np.float64)
    if not softmax:
        return x
    m = x.max(1, keepdims=True)
    e = np.exp(x - m)
    return e / e.sum(1, keepdims=True)


def _dp(x, softmax):
    """[N, 1, ...]: dp(D) in units of u; 0 without softmax"""
    x = np.asarray(x, np.float64)
    c = x.shape[1]
    if not softmax:
        return np.zeros(x.max(1, keepdims=True).shape)
    return 2.0 * (x.max(1, keepdims=True) - x.min(1, keepdims=True)) + 4.0 * E_EXP + c + 1


def _slices(x):
    n, c, d, h, w = x.shape
    return np.ascontiguousarray(x.transpose(0, 2, 1, 3, 4)).reshape(n * d, c, h, w)


def _unslices(x, n, d):
    s, c, h, w = x.shape
    return np.ascontiguousarray(x.reshape(n, d, c, h, w).transpose(0, 2, 1, 3, 4))


def jacobian(p, e, gs, softmax):
    g = float(np.float32(gs))
    return g * (p * (e - (e * p).sum(1, keepdims=True))) if softmax else g * e


def jacobian_bound(p, dps, E, ee, gs, softmax):
    g = abs(float(np.float32(gs)))
    c = p.shape[1]
    if not softmax:
        return GAMMA_SLACK * g * (ee + U * E) + ETA
    S = g * p * (E + (p * E).sum(1, keepdims=True))
    inner = ee + (p * ee + dps * U * p * E).sum(1, keepdims=True)
    return GAMMA_SLACK * (g * p * inner + (dps + c + 5) * U * S) + ETA * (1 + g * (E + E.sum(1, keepdims=True)))


def _t(a, dt=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64))).to(dt)


# ---------------------------------------------------------------- GatedCRF

def _desc32(desc):
    return [tuple(float(np.float32(x)) for x in row) for row in desc]


def crf_eval(P, I, desc, r, EP=None, mut=None):
    """P [S, C, H, W] probabilities, I [S, Ci, H, W] (float64) -> Ref with out0, kp [S, C, H, W] and, where EP (the probabilities'
    absolute errors) is given, out0_bound and kp_bound"""
    S, C, H, W = P.shape
    Ci = I.shape[1]
    desc = _desc32(desc)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    pad = lambda a: np.pad(a, ((0, 0), (0, 0), (r, r), (r, r)))
    Pp, Ip = pad(P), pad(I)
    EPp = None if EP is None else pad(EP)
    want = EP is not None
    out0 = 0.0
    sumT = sum_eT = 0.0
    kp = np.zeros_like(P)
    ekp, kpabs = np.zeros_like(P), np.zeros_like(P)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if dy == 0 and dx == 0 and mut != "crf_centre":
                continue
            inb = (ys + dy >= 0) & (ys + dy < H) & (xs + dx >= 0) & (xs + dx < W)
            Pj = Pp[:, :, r + dy:r + dy + H, r + dx:r + dx + W]
            Ij = Ip[:, :, r + dy:r + dy + H, r + dx:r + dx + W]
            xj, yj = np.where(inb, xs + dx, 0.0), np.where(inb, ys + dy, 0.0)
            d2 = (xs - xj) ** 2 + (ys - yj) ** 2
            rgb2 = ((I - Ij) ** 2).sum(1)
            k = np.zeros((S, H, W))
            ek = np.zeros((S, H, W))
            kabs = np.zeros((S, H, W))
            for wt, sxy, srgb in desc:
                a_xy = 0.5 * d2 / (sxy if mut == "crf_sigma" else sxy * sxy) if sxy > 0 else np.zeros_like(d2)
                a_rgb = 0.5 * rgb2 / (srgb if mut == "crf_sigma" else srgb * srgb) if srgb > 0 else np.zeros_like(rgb2)
                kd = wt * np.exp(-(a_xy[None] + a_rgb))
                k += kd
                if want:
                    rel = np.where(inb[None], 2 * a_xy[None] + (5 + Ci) * a_rgb + 2 * E_EXP + 2,
                                   (5 + Ci) * (a_xy[None] + a_rgb) + E_EXP + 1)
                    ek += np.abs(kd) * rel * U + 4 * ETA * abs(wt)
                    kabs += np.abs(kd)
            if mut == "crf_drop_oob":
                k = k * inb[None]
            dot = (P * Pj).sum(1)
            T = k * (1.0 - dot)
            out0 += float(T.sum())
            kin = k * inb[None]
            kp += kin[:, None] * Pj
            if want:
                ek += len(desc) * U * kabs
                EPj = EPp[:, :, r + dy:r + dy + H, r + dx:r + dx + W]
                e_dot = (P * EPj + Pj * EP).sum(1) + (C + 1) * U * dot
                eT = ek * np.abs(1.0 - dot) + kabs * (e_dot + U * np.abs(1.0 - dot)) + U * np.abs(T)
                sum_eT += float(eT.sum())
                sumT += float(np.abs(T).sum())
                ein = (ek * inb[None])[:, None]
                ekp += ein * Pj + np.abs(kin)[:, None] * EPj
                kpabs += np.abs(kin)[:, None] * Pj
    res = Ref()
    res.out0, res.kp = out0, kp
    if want:
        nt = (2 * r + 1) ** 2
        res.out0_bound = GAMMA_SLACK * (sum_eT + (nt + 9) * U * sumT) + S * H * W * nt * ETA
        res.kp_bound = GAMMA_SLACK * (ekp + nt * U * kpabs) + nt * ETA
    return res


def crf_statements(X, im, desc, r, softmax):
    """wsl_gatedcrf.py:80-93 and gatedcrf.py:52-102, 121-169 with torch operations on the tensors X [N, C, D, H, W] and im
    [N, Ci, D, H, W] (any float dtype; X may be part of a graph) -> (loss, kernels.sum() - (..).sum())"""
    dt = X.dtype
    n, c, d, h, w = X.shape
    soft = torch.softmax(X, dim=1) if softmax else X
    y = torch.reshape(torch.transpose(soft, 1, 2), [n * d, c, h, w])
    rgb = torch.reshape(torch.transpose(im, 1, 2), [n * d, im.shape[1], h, w])
    N = n * d
    dia = 2 * r + 1
    unfold = lambda t: F.unfold(t, dia, 1, r).view(t.shape[0], t.shape[1], dia, dia, h, w)
    mesh = torch.cat((torch.arange(0, w, 1, dtype=dt, device=X.device).view(1, 1, 1, w).repeat(N, 1, h, 1),
                      torch.arange(0, h, 1, dtype=dt, device=X.device).view(1, 1, h, 1).repeat(N, 1, 1, w)), 1)
    kernels = None
    for wt, sxy, srgb in _desc32(desc):
        feats = []
        if sxy > 0:
            feats.append(mesh / sxy)
        if srgb > 0:
            feats.append(rgb / srgb)
        feats = torch.cat(feats, dim=1)
        k = unfold(feats)
        k = k - k[:, :, r, r, :, :].view(N, feats.shape[1], 1, 1, h, w)
        k = (-0.5 * k ** 2).sum(dim=1, keepdim=True).exp()
        k[:, :, r, r, :, :] = 0
        k = wt * k
        kernels = k if kernels is None else k + kernels
    prod = (kernels * unfold(y)).view(N, c, dia * dia, h, w).sum(dim=2, keepdim=False)
    total = kernels.sum() - (prod * y).sum()
    return total / (N * h * w), total


def autograd_crf(x, image, desc, r, softmax, gs, dt=torch.float64):
    """-> (loss, dx, total) of crf_statements"""
    X = _t(x, dt).requires_grad_(True)
    loss, total = crf_statements(X, _t(image, dt), desc, r, softmax)
    (loss * float(np.float32(gs))).backward()
    return loss.item(), X.grad.double().numpy(), total.item()


def crf_ref(x, image, desc, r, softmax=True, gs=1.0, mut=None, use_autograd=True):
    """r.out [4] (sum, 0, loss, S H W), r.kp, r.dl with r.out0_bound, r.loss_bound, r.kp_bound, r.dl_bound"""
    n, c, d, h, w = x.shape
    p5 = _probs(x, softmax)
    dps5 = _dp(x, softmax)
    P, I = _slices(p5), _slices(np.asarray(image, np.float64))
    EP = _slices(dps5 * U * p5)
    ev = crf_eval(P, I, desc, r, EP, mut)
    numel = float(n * d * h * w)
    res = Ref()
    res.out = np.array([ev.out0, 0.0, ev.out0 / numel, numel])
    res.kp = _unslices(ev.kp, n, d)
    coef = (-1.0 if mut == "crf_grad2" else -2.0) / numel
    e = coef * res.kp
    res.dl = jacobian(p5, e, gs, softmax)
    if use_autograd and mut is None:
        al, adl, atot = autograd_crf(x, image, desc, r, softmax, gs)
        assert abs(atot - ev.out0) <= 1e-11 * max(abs(ev.out0), 1e-300), (atot, ev.out0)
        assert abs(al - res.out[2]) <= 1e-11 * max(abs(al), 1e-300)
        assert float(np.abs(adl - res.dl).max()) <= 1e-11 * max(float(np.abs(res.dl).max()), 1e-300), "CRF gradient differs from autograd"
    res.out0_bound = ev.out0_bound
    res.loss_bound = ev.out0_bound / numel + 1e-15 * abs(res.out[2])
    res.kp_bound = _unslices(ev.kp_bound, n, d)
    E = np.abs(e)
    ee = abs(coef) * res.kp_bound + 2 * U * E
    res.dl_bound = jacobian_bound(p5, dps5, E, ee, gs, softmax)
    return res


# ---------------------------------------------------------------- TotalVariation

def _window(x, mode, src=None, two_d=False):
    """x [R, D, H, W] -> (extreme value over the in-bounds 3x3x3 window, flat offset of the FIRST one in (d, h, w) scan order,
    gap to the runner-up).  src [R, D, H, W]: the runner-up is taken among entries whose src differs from the winner's"""
    R, D, H, W = x.shape
    sgn = 1.0 if mode == "min" else -1.0
    big = np.inf
    xp = np.pad(sgn * x, ((0, 0), (1, 1), (1, 1), (1, 1)), constant_values=big)
    flat = np.arange(D * H * W).reshape(1, D, H, W)
    fp = np.pad(np.broadcast_to(flat, x.shape), ((0, 0), (1, 1), (1, 1), (1, 1)), constant_values=-1)
    sp = None if src is None else np.pad(src, ((0, 0), (1, 1), (1, 1), (1, 1)), constant_values=-1)
    vals, idxs, srcs = [], [], []
    for dd in ((1,) if two_d else (0, 1, 2)):
        for hh in range(3):
            for ww in range(3):
                sl = (slice(None), slice(dd, dd + D), slice(hh, hh + H), slice(ww, ww + W))
                vals.append(xp[sl])
                idxs.append(fp[sl])
                srcs.append((fp if sp is None else sp)[sl])
    vals, idxs, srcs = np.stack(vals), np.stack(idxs), np.stack(srcs)
    first = vals.argmin(0)                                   # numpy: the first minimum
    take = lambda a: np.take_along_axis(a, first[None], 0)[0]
    best, bidx, bsrc = take(vals), take(idxs), take(srcs)
    other = np.where(srcs != bsrc[None], vals, big)
    gap = other.min(0) - best                                # inf where the window holds one source only
    return sgn * best, bidx, gap


def _maxpool_abs(x):
    return F.max_pool3d(torch.from_numpy(np.ascontiguousarray(x)), 3, 1, 1).numpy()


def tv_fwd(x, softmax, mut=None):
    """-> (out [4], count int64 [N, C, D, H, W], pieces)"""
    n, c, d, h, w = x.shape
    p = _probs(x, softmax)
    pp = p if mut == "tv_999" else p * 0.999 + 5e-4
    rows = pp.reshape(n * c, d, h, w)
    two_d = mut == "tv_2d"
    first, second = ("max", "min") if mut == "tv_swap" else ("min", "max")
    e, amin, gap_e = _window(rows, first, None, two_d)
    o, amax, gap_o = _window(e, second, amin, two_d)
    ct = np.maximum(o - e, 0.0) if mut != "tv_swap" else np.maximum(e - o, 0.0)
    pos = ct > 0
    V = d * h * w
    count = np.zeros((n * c, V), np.int64)
    rix = np.broadcast_to(np.arange(n * c)[:, None], (n * c, V))
    src_of_max = np.take_along_axis(amin.reshape(n * c, V), amax.reshape(n * c, V), 1)
    np.add.at(count, (rix[pos.reshape(n * c, V)], src_of_max[pos.reshape(n * c, V)]), 1)
    np.add.at(count, (rix[pos.reshape(n * c, V)], amin.reshape(n * c, V)[pos.reshape(n * c, V)]), -1)
    numel = float(n * c * V)
    out0 = float(ct.sum())
    return np.array([out0, 0.0, out0 / numel, numel]), count.reshape(x.shape), (p, pp, ct.reshape(x.shape), gap_e, gap_o)


def tv_bwd(x, count, gs, softmax, mut=None):
    n, c, d, h, w = x.shape
    p = _probs(x, softmax)
    coef = (1.0 if mut == "tv_999" else 0.999) / float(n * c * d * h * w)
    e = coef * np.asarray(count, np.float64)
    return jacobian(p, e, gs, softmax), p, e


def tv_statements(X, softmax):
    """loss/seg/ssl.py:72-86 on the tensor X (may be part of a graph) -> (length, contour)"""
    predict = torch.nn.Softmax(dim=1)(X) if softmax else X
    predict = predict * 0.999 + 5e-4
    pred_min = -1 * F.max_pool3d(-1 * predict, (3, 3, 3), 1, 1)
    pred_max = F.max_pool3d(pred_min, (3, 3, 3), 1, 1)
    contour = torch.relu(pred_max - pred_min)
    return torch.mean(contour), contour


def autograd_tv(x, softmax, gs, dt=torch.float64):
    X = _t(x, dt).requires_grad_(True)
    length, contour = tv_statements(X, softmax)
    (length * float(np.float32(gs))).backward()
    return length.item(), X.grad.double().numpy(), contour.sum().item()


def tv_ref(x, softmax=True, gs=1.0, use_autograd=True):
    """r.out, r.count, r.undecided (voxels), r.count_free (entries no undecided voxel can move), r.out0_bound, r.loss_bound"""
    n, c, d, h, w = x.shape
    out, count, (p, pp, ct, gap_e, gap_o) = tv_fwd(x, softmax)
    res = Ref()
    res.out, res.count = out, count
    if use_autograd:
        al, adl, asum = autograd_tv(x, softmax, gs)
        assert abs(asum - out[0]) <= 1e-11 * max(abs(out[0]), 1e-300) and abs(al - out[2]) <= 1e-11 * max(abs(al), 1e-300)
        dl = tv_bwd(x, count, gs, softmax)[0]
        assert float(np.abs(adl - dl).max()) <= 1e-11 * max(float(np.abs(dl).max()), 1e-300), "TV count form differs from autograd"
    dps = _dp(x, softmax)
    epp = (0.999 * dps * U * p + 4 * U * pp).reshape(n * c, d, h, w)
    ee = _maxpool_abs(epp)
    eo = _maxpool_abs(ee)
    ctr = ct.reshape(n * c, d, h, w)
    und = (gap_e <= 2 * GAMMA_SLACK * ee) | (gap_o <= 2 * GAMMA_SLACK * eo) | ((ctr > 0) & (ctr <= GAMMA_SLACK * (eo + ee)))
    res.undecided = und.reshape(x.shape)
    near = F.max_pool3d(torch.from_numpy(und.astype(np.float32)), 5, 1, 2).numpy() > 0
    res.count_free = ~near.reshape(x.shape)
    e_ct = eo + ee + U * ctr
    res.out0_bound = GAMMA_SLACK * (float(e_ct.sum()) + ra(d * h * w) * U * out[0]) + float(e_ct[und].sum()) + n * c * d * h * w * ETA
    res.loss_bound = res.out0_bound / out[3] + 1e-15 * abs(out[2])
    return res


def check_tv_case(r):
    share = float(r.undecided.mean())
    assert share <= MAX_UNDECIDED, "undecided share %g" % share


def tv_grad_ref(x, count, gs, softmax=True):
    """float64 dlogits for the DEVICE's count, with its bound (the count is an integer: coef's rounding and one product)"""
    dl, p, e = tv_bwd(x, count, gs, softmax)
    E = np.abs(e)
    return dl, jacobian_bound(p, _dp(x, softmax), E, 2 * U * E, gs, softmax)


# ---------------------------------------------------------------- Mumford-Shah

def ms_fwd(x, image, penalty, lam, softmax, mut=None):
    """-> (out [4], cen [N, D, Ci, C], p)"""
    n, c, d, h, w = x.shape
    p = _probs(x, softmax)
    im = np.asarray(image, np.float64)
    ax = (2, 3, 4) if mut == "ms_volume" else (3, 4)
    S0 = p.sum(ax, keepdims=True)                                            # [N, C, D or 1, 1, 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        cen = (im[:, :, None] * p[:, None]).sum(tuple(a + 1 for a in ax), keepdims=True) / S0[:, None]     # [N, Ci, C, D, 1, 1]
    t = im[:, :, None] - cen
    out0 = float((t * t * p[:, None]).sum())
    dH, dW = np.abs(p[:, :, :, 1:] - p[:, :, :, :-1]), np.abs(p[:, :, :, :, 1:] - p[:, :, :, :, :-1])
    l2 = (penalty == 2) != (mut == "ms_l1l2")
    out1 = float((dH * dH).sum() + (dW * dW).sum()) if l2 else float(dH.sum() + dW.sum())
    numel = float(n * d * h * w) * (1 if mut == "ms_numel" else c)
    cen_out = np.broadcast_to(cen, (n, im.shape[1], c, d, 1, 1))[..., 0, 0].transpose(0, 3, 1, 2)
    return np.array([out0, out1, (out0 + float(np.float32(lam)) * out1) / numel, numel]), np.ascontiguousarray(cen_out), p


def ms_stencil(p, penalty):
    """-> (stencil, sum of the magnitudes of its terms) per element of p [N, C, D, H, W]"""
    st, mag = np.zeros_like(p), np.zeros_like(p)
    for axis in (3, 4):
        dlt = np.diff(p, axis=axis)                                          # q - p at the lower index
        g = 2.0 * dlt if penalty == 2 else np.sign(dlt)
        lo = [slice(None)] * 5
        hi = [slice(None)] * 5
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        st[tuple(hi)] += g
        st[tuple(lo)] -= g
        mag[tuple(hi)] += np.abs(g)
        mag[tuple(lo)] += np.abs(g)
    return st, mag


def ms_bwd(x, image, cen, penalty, lam, gs, softmax, mut=None):
    """cen [N, D, Ci, C] (the device's or the oracle's)"""
    n, c, d, h, w = x.shape
    p = _probs(x, softmax)
    im = np.asarray(image, np.float64)
    cn = np.asarray(cen, np.float64).transpose(0, 2, 3, 1)[..., None, None]  # [N, Ci, C, D, 1, 1]
    t = im[:, :, None] - cn
    lev = (t * t).sum(1)
    st, mag = ms_stencil(p, 3 - penalty if mut == "ms_l1l2" else penalty)
    numel = float(n * d * h * w) * (1 if mut == "ms_numel" else c)
    lam = float(np.float32(lam))
    e = (lev + lam * st) / numel
    return jacobian(p, e, gs, softmax), p, t, lev, mag, numel


def ms_statements(X, image, penalty, lam, softmax):
    """mumford_shah.py:32-95 on the tensors X [N, C, D, H, W] (may be part of a graph) and image -> (loss, loss0, loss1)"""
    predict = torch.nn.Softmax(dim=1)(X) if softmax else X
    n, c, d, h, w = predict.shape
    predict = torch.reshape(torch.transpose(predict, 1, 2), [n * d, c, h, w])
    image = torch.reshape(torch.transpose(image, 1, 2), [n * d, image.shape[1], h, w])
    outshape, tarshape = predict.shape, image.shape
    loss0 = 0.0
    for ich in range(tarshape[1]):
        target_ = torch.unsqueeze(image[:, ich], 1)
        target_ = target_.expand(tarshape[0], outshape[1], tarshape[2], tarshape[3])
        pcentroid = torch.sum(target_ * predict, (2, 3)) / torch.sum(predict, (2, 3))
        pcentroid = pcentroid.view(tarshape[0], outshape[1], 1, 1)
        plevel = target_ - pcentroid.expand(tarshape[0], outshape[1], tarshape[2], tarshape[3])
        loss0 = loss0 + torch.sum(plevel * plevel * predict)
    dH = torch.abs(predict[:, :, 1:, :] - predict[:, :, :-1, :])
    dW = torch.abs(predict[:, :, :, 1:] - predict[:, :, :, :-1])
    if penalty == 2:
        dH, dW = dH * dH, dW * dW
    loss1 = torch.sum(dH) + torch.sum(dW)
    return (loss0 + float(np.float32(lam)) * loss1) / torch.numel(predict), loss0, loss1


def autograd_ms(x, image, penalty, lam, softmax, gs, dt=torch.float64):
    X = _t(x, dt).requires_grad_(True)
    loss, loss0, loss1 = ms_statements(X, _t(image, dt), penalty, lam, softmax)
    (loss * float(np.float32(gs))).backward()
    return loss.item(), X.grad.double().numpy(), loss0.item(), loss1.item()


def ms_ref(x, image, penalty, lam, softmax=True, gs=1.0, use_autograd=True):
    """r.out, r.cen, r.dl with r.out0_bound, r.out1_bound, r.loss_bound, r.cen_bound, r.dl_bound (for the oracle's centroids; the
    device's own lie within cen_bound of them, which the gradient's bound carries)"""
    n, c, d, h, w = x.shape
    im = np.asarray(image, np.float64)
    ci = im.shape[1]
    out, cen, p = ms_fwd(x, image, penalty, lam, softmax)
    dl, _, t, lev, mag, numel = ms_bwd(x, image, cen, penalty, lam, gs, softmax)
    res = Ref()
    res.out, res.cen, res.dl = out, cen, dl
    if use_autograd:
        # the magnitude: (I - cen)^2 is made of I^2, I cen and cen^2, and autograd's gradient also carries the centroid's own
        # derivative, which cancels only up to rounding (a 1 x 1 slice has I = cen: everything there is cancellation)
        al, adl, a0, a1 = autograd_ms(x, image, penalty, lam, softmax, gs)
        top = (float(np.abs(im).max()) + float(np.abs(cen).max())) ** 2
        m0 = max(abs(out[0]), top * float(np.abs(p).sum()) * ci)
        assert abs(a0 - out[0]) <= 1e-11 * m0 and abs(a1 - out[1]) <= 1e-11 * max(abs(out[1]), 1e-300)
        assert abs(al - out[2]) <= 1e-11 * max(abs(al), m0 / out[3])
        mg = max(float(np.abs(dl).max()), abs(float(np.float32(gs))) * (top * ci + float(np.float32(lam)) * float(mag.max())) / numel)
        assert float(np.abs(adl - dl).max()) <= 1e-11 * mg, "Mumford-Shah gradient differs from autograd"
    hw = h * w
    lam = float(np.float32(lam))
    dps = _dp(x, softmax)
    ep = dps * U * p                                                         # [N, C, D, H, W]
    S0 = p.sum((3, 4), keepdims=True)
    eS0 = ep.sum((3, 4), keepdims=True) + ra(hw) * U * S0
    aI = np.abs(im)[:, :, None]                                              # [N, Ci, 1, D, H, W]
    S1a = (aI * p[:, None]).sum((4, 5), keepdims=True)
    eS1 = (aI * ep[:, None]).sum((4, 5), keepdims=True) + (ra(hw) + 1) * U * S1a
    cn = cen.transpose(0, 2, 3, 1)[..., None, None]                          # [N, Ci, C, D, 1, 1]
    ecen = eS1 / S0[:, None] + np.abs(cn) * eS0[:, None] / S0[:, None] + U * np.abs(cn)
    res.cen_bound = GAMMA_SLACK * ecen[..., 0, 0].transpose(0, 3, 1, 2) + ETA
    et = ecen + U * np.abs(t)
    t2 = t * t
    # the square's error in full: where I = cen (a one-pixel slice) the first-order term vanishes and et^2 is all there is
    et2 = 2 * np.abs(t) * et + et * et + U * (np.abs(t) + et) ** 2
    e_term = t2 * ep[:, None] + (p + ep)[:, None] * et2 + U * (t2 + et2) * p[:, None]
    res.out0_bound = GAMMA_SLACK * (float(e_term.sum()) + (c * ci * LO.row_terms(hw) / 256 + 12) * U * (out[0] + float(e_term.sum()))) \
        + n * c * ci * d * hw * ETA
    e1 = 0.0
    e_st = np.zeros_like(p)
    for axis in (3, 4):
        dlt = np.abs(np.diff(p, axis=axis))
        lo = [slice(None)] * 5
        hi = [slice(None)] * 5
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        ed = ep[tuple(lo)] + ep[tuple(hi)] + U * dlt
        e1 += float((2 * dlt * ed + ed * ed + U * (dlt + ed) ** 2).sum()) if penalty == 2 else float(ed.sum())
        s = 2.0 * ed if penalty == 2 else 2.0 * ((dlt <= GAMMA_SLACK * ed) & (ed > 0))     # exact inputs: sign(0) = 0 on both sides
        e_st[tuple(lo)] += s
        e_st[tuple(hi)] += s
    res.out1_bound = GAMMA_SLACK * (e1 + (2 * c * LO.row_terms(hw) / 256 + 12) * U * out[1]) + 2 * n * c * d * hw * ETA
    res.loss_bound = (res.out0_bound + lam * res.out1_bound) / out[3] + 1e-15 * abs(out[2])
    if penalty == 2:
        e_st = e_st + 4 * U * mag
    e_lev = et2.sum(1) + ci * U * (lev + et2.sum(1))
    E = (lev + lam * mag) / numel
    ee = (e_lev + lam * e_st) / numel + 4 * U * (E + e_lev / numel)
    res.dl_bound = jacobian_bound(p, dps, E + ee, ee, gs, softmax)
    return res
