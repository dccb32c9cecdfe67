"""Float64 oracle for URPC's pyramid consistency and CPS's pseudo labels (fpl-plus_amd/csrc/ssl.hip: fplx_ssl_pyramid_fwd / _bwd,
fplx_ssl_pseudo_onehot), on top of tests/lossoracle.py and tests/ssloracle.py: same notation (u = 2^-24, ETA, E_EXP, E_LOG,
dp(D), ra', GAMMA_SLACK) and NO new measured constant.

The pass under test.  K logit tensors z_k [N, C, V] (N: the unlabelled rows), M = N V.  Per voxel (ssl_urpc.py:76-90)
    p_k = softmax(z_k), m = (p_1 + .. + p_K) / K, a = 0.99 m + 0.005, q_k = 0.99 p_k + 0.005, dl_kc = ln a_c - ln q_kc,
    var_k = sum_c a_c dl_kc, e_k = exp(-var_k), s_k = sum_c (a_c - q_kc)^2
    A_k = sum_v s_k e_k, B_k = sum_v e_k, V_k = sum_v var_k, L_k = (A_k / (C M)) / (B_k / M + 1e-8) + V_k / M, loss = sum_k L_k / K
    alpha_k = 1 / (C M (B_k / M + 1e-8)), beta_k = -(A_k / (C M)) / (B_k / M + 1e-8)^2 / M,
    g_k = 1 / M - e_k (alpha_k s_k + beta_k), h_k = alpha_k e_k,
    dL/dp_jc = (0.99 / K) [(1 / K) sum_k (g_k (dl_kc + 1) + 2 h_k (a_c - q_kc)) - g_j a_c / q_jc - 2 h_j (a_c - q_jc)],
    dz_jc = gs p_jc (dL/dp_jc - sum_i p_ji dL/dp_ji).
The closed forms are asserted in every reference call against float64 autograd of the reference's own statements written with
torch operations (softmax, stack, mean, KLDivLoss(reduction='none'), exp, square, mean), 1e-11 of the magnitude.

A - exact part.  K in {2, 4} IDENTICAL tensors of dyadic logits: the sum of 2 or 4 equal floats and its division by K are exact,
    so m = p_k, a = q_k bit for bit, ln a - ln q = 0, var = 0, e = exp(-0) = 1, s = 0: A_k = 0, V_k = 0, B_k = M (a count, exact in
    fp32 partial rows below 2^24 per row and in the double sum), L_k = 0 / (1 + 1e-8) + 0 = 0, loss = 0 - bit for bit.
B - rounding part.  First order in u, every term on un-cancelled magnitudes, times GAMMA_SLACK.  With D_k = max - min of a
    voxel's logits of scale k, dp_k = 2 D_k + 4 E_EXP + C + 1 [u] and ep_kc = dp_k u p_kc (lossoracle).
    m_c     K - 1 additions of positive terms and one division:  em = u (sum_k dp_k p_kc / K + K m)
    a_c     two constants, a product, a sum (not fused):         ea = 0.99 em + 4 u a;   likewise eq_kc = 0.99 ep_kc + 4 u q
    ln      ela = ea / a + E_LOG u |ln a|,  elq = eq / q + E_LOG u |ln q|
    dl_kc   edl = ela + elq + u (|ln a| + |ln q|)   (the difference's rounding is u |dl| <= this; the larger form also covers
            torch's a ln a - a ln q, which the fixture's fp32 numbers were computed with)
    var_k   e_var = sum_c (ea |dl| + a edl) + (C + 1) u sum_c a |dl|
    e_k     ee = e (e_var + E_EXP u)
    s_k     d = a - q: ed = ea + eq + u |d|;  es = sum_c 2 |d| ed + (C + 1) u s
    s e     ese = es e + s ee + u s e
    sums    A_k: sum_v ese + ra' u sum_v s e;  B_k: sum_v ee + ra' u sum_v e;  V_k: sum_v e_var + ra' u sum_v sum_c a |dl|
            (ra' = ssloracle.ra_ssl(V): a lane's chain, 6 shuffles, 3 additions in LDS; the rows are added in double), each
            plus N V C ETA for the underflow of exp(z - max).
    L_k     evaluated in double by one thread from A_k, B_k, V_k.  Two checks: against the float64 truth with the bound
            eA / (C M den) + (A / (C M)) / den^2 eB / M + eV / M, den = B / M + 1e-8; and against the SAME formula evaluated
            here from the device's own sums, where only double roundings remain: 16 x 2^-53 of (|first term| + |V / M|).  The
            second is what sees a missing 1e-8 or a C M written as M, which the fp32 sums' bound would hide.
    gradient  with the DEVICE's A_k, B_k (alpha, beta are then known up to their rounding to fp32):
            t2 = alpha s + beta: T2 = alpha s + |beta|, et2 = alpha es + 2 u alpha s + u |beta| + u T2
            g = 1 / M - e t2:    G = 1 / M + e T2,  eg = ee T2 + e et2 + u e T2 + u / M + u G
            h2 = 2 alpha e:      eh2 = 2 (alpha ee + 2 u alpha e)
            t_c = (1 / K) sum_k (g_k (dl_kc + 1) + h2_k d_kc):  MT = (1 / K) sum_k (G (|dl| + 1) + h2 |d|),
                  eT = (1 / K) sum_k (eg (|dl| + 1) + G (edl + 2 u (|dl| + 1)) + eh2 |d| + h2 ed + u h2 |d|) + (2 K + 1) u MT
            r = g a / q:  R = G a / q, er = eg a / q + G ea / q + G a eq / q^2 + 2 u R;   x = h2 d: X = h2 |d|, ex = eh2 |d| + h2 ed + u X
            gp = w (t - r - x), w = 0.99 / K in fp32:  GP = w (MT + R + X), egp = w (eT + er + ex + 5 u (MT + R + X))
            softmax Jacobian as in ssloracle: S_c = |gs| p_c (GP_c + sum_i p_i GP_i),
            |err| <= GAMMA_SLACK (|gs| p_c (egp_c + sum_i (p_i egp_i + dp u p_i GP_i)) + (dp + C + 5) u S_c) + ETA (1 + |gs| (GP_c + sum GP))

Pure numpy / torch on the CPU; tests/test_ssl2_cpu.py checks the oracle itself, tests/test_gpu_ssl2.py applies it."""
import numpy as np
import torch

import lossoracle as LO
import ssloracle as SO
from lossoracle import U, ETA, E_EXP, E_LOG, GAMMA_SLACK, ratio  # noqa: F401

MUTATIONS = ("a_from_q", "mean_detached", "cm_swap", "no_eps")
EPS64 = 2.0 ** -53


# ---------------------------------------------------------------- generators

def logits_case(key, k, n, c, v):
    """K scales of one prediction: base [N, C, V] * 1.5 + jitter * 0.5 per scale, standard normal -> float32 [K, N, C, V]"""
    g = LO.rng(key)
    base = g.standard_normal((n, c, v)) * 1.5
    return np.ascontiguousarray((base[None] + g.standard_normal((k, n, c, v)) * 0.5).astype(np.float32))


def exact_case(key, n, c, v):
    """dyadic logits, multiples of 1/8 in [-4, 4] -> float32 [N, C, V] (the K tensors are copies of it)"""
    g = LO.rng(key)
    return np.ascontiguousarray((g.integers(-32, 33, (n, c, v)) / 8.0).astype(np.float32))


def onehot_case(key, k, n, c, v):
    """logits on the grid j / 8, |j| <= 32, with ties (a third of the voxels repeat their first class's value in the last class,
    a tenth are constant over C) -> float32 [K, N, C, V]"""
    g = LO.rng(key)
    z = g.integers(-32, 33, (k, n, c, v)).astype(np.float64)
    tie = g.random((k, n, v)) < 1.0 / 3.0
    z[:, :, c - 1, :] = np.where(tie, z[:, :, 0, :], z[:, :, c - 1, :])
    flat = g.random((k, n, v)) < 0.1
    z = np.where(flat[:, :, None, :], z[:, :, :1, :], z)
    return np.ascontiguousarray((z / 8.0).astype(np.float32))


# ---------------------------------------------------------------- closed forms (dt = float32: the kernels' arithmetic, with mutations)

def _voxel_terms(z, dt, mut=None):
    """z [K, N, C, V] -> p, a [N, C, V], q, dl [K, N, C, V], var, e, s [K, N, V] in dt, in the kernel's order of operations"""
    k, n, c, v = z.shape
    p = SO._softmax(z.astype(dt), 2)
    q = p * dt(0.99) + dt(0.005)
    src = q if mut == "a_from_q" else p
    m = src[0].copy()
    for i in range(1, k):
        m = m + src[i]
    m = m / dt(k)
    a = m * dt(0.99) + dt(0.005)
    dl = np.log(a)[None] - np.log(q)
    var = np.zeros((k, n, v), dt)
    s = np.zeros((k, n, v), dt)
    for ci in range(c):
        d = a[None, :, ci] - q[:, :, ci]
        var = var + a[None, :, ci] * dl[:, :, ci]
        s = s + d * d
    e = np.exp(-var)
    return p, a, q, dl, var, e, s


def _total(x, dt):
    """[N, V] -> float64: exact in float64; in fp32 the scalar form's partial rows in fp32, the rows in double"""
    if dt == np.float64:
        return float(x.astype(np.float64).sum())
    return float(LO._reduce(x, dt, None).sum())


def scale_loss(A, B, V, c, M, mut=None):
    """L_k in double from the three sums"""
    cm = M if mut == "cm_swap" else c * M
    eps = 0.0 if mut == "no_eps" else 1e-8
    return (A / cm) / (B / M + eps) + V / M


def pyramid_fwd(z, dt=np.float64, mut=None):
    """-> out float64 [4 K + 2]: A_k, B_k, V_k, L_k per scale; loss_reg; 0"""
    k, n, c, v = z.shape
    _, _, _, _, var, e, s = _voxel_terms(z, dt, mut)
    M = float(n) * v
    out = np.zeros(4 * k + 2)
    for i in range(k):
        A, B, V = _total(s[i] * e[i], dt), _total(e[i], dt), _total(var[i], dt)
        out[4 * i:4 * i + 4] = A, B, V, scale_loss(A, B, V, c, M, mut)
    out[4 * k] = out[3:4 * k:4].sum() / k
    return out


def pyramid_bwd(z, out, gs, dt=np.float64, mut=None):
    """dz [K, N, C, V] for the sums A_k, B_k of `out`"""
    k, n, c, v = z.shape
    p, a, q, dl, var, e, s = _voxel_terms(z, dt, mut)
    M = float(n) * v
    cm = M if mut == "cm_swap" else c * M
    eps = 0.0 if mut == "no_eps" else 1e-8
    f = (lambda x: dt(np.float32(x))) if dt == np.float32 else (lambda x: x)
    g, h2 = [], []
    for i in range(k):
        den = out[4 * i + 1] / M + eps
        al, be = f(1.0 / (cm * den)), f(-(out[4 * i] / cm) / (den * den) / M)
        g.append(f(1.0 / M) - e[i] * (al * s[i] + be))
        h2.append(dt(2) * (al * e[i]))
    d = a[None] - q
    t = np.zeros((n, c, v), dt)
    if mut != "mean_detached":
        for i in range(k):
            t = t + (g[i][:, None] * (dl[i] + dt(1)) + h2[i][:, None] * d[i])
        t = t / dt(k)
    w = dt(np.float32(0.99) / np.float32(k)) if dt == np.float32 else 0.99 / k
    gsc = dt(np.float32(gs))
    dz = np.zeros((k, n, c, v), dt)
    for j in range(k):
        gp = w * (t - g[j][:, None] * a / q[j] - h2[j][:, None] * d[j])
        dz[j] = gsc * (p[j] * (gp - (gp * p[j]).sum(1, keepdims=True)))
    return dz


# ---------------------------------------------------------------- float64 autograd of the reference's statements

def autograd_pyramid(z, gs):
    """ssl_urpc.py:76-91 in float64 over the unlabelled rows -> (out [4 K + 2], dz [K, N, C, V])"""
    k, n, c, v = z.shape
    outputs_list = [torch.from_numpy(z[i].astype(np.float64)).requires_grad_(True) for i in range(k)]
    kl_distance = torch.nn.KLDivLoss(reduction='none')
    outputs_soft_list = [torch.softmax(item, dim=1) for item in outputs_list]
    outputs_soft_avg = torch.mean(torch.stack(outputs_soft_list), dim=0)
    p1_avg = outputs_soft_avg * 0.99 + 0.005
    loss_reg = 0.0
    out = np.zeros(4 * k + 2)
    for i, soft_i in enumerate(outputs_soft_list):
        p1_i = soft_i * 0.99 + 0.005
        var = torch.sum(kl_distance(torch.log(p1_i), p1_avg), dim=1, keepdim=True)
        exp_var = torch.exp(-var)
        square_e = torch.square(p1_avg - p1_i)
        loss_i = torch.mean(square_e * exp_var) / (torch.mean(exp_var) + 1e-8) + torch.mean(var)
        loss_reg = loss_reg + loss_i
        out[4 * i:4 * i + 4] = (square_e * exp_var).sum().item(), exp_var.sum().item(), var.sum().item(), loss_i.item()
    loss_reg = loss_reg / k
    out[4 * k] = loss_reg.item()
    (loss_reg * float(np.float32(gs))).backward()
    return out, np.stack([t.grad.numpy() for t in outputs_list])


# ---------------------------------------------------------------- references with bounds

class Ref(object):
    pass


def _errors(z):
    """float64 per-voxel values and their first-order fp32 error terms (the docstring's table) -> a namespace"""
    k, n, c, v = z.shape
    z64 = z.astype(np.float64)
    t = Ref()
    t.p, t.a, t.q, t.dl, t.var, t.e, t.s = _voxel_terms(z64, np.float64)
    D = z64.max(2, keepdims=True) - z64.min(2, keepdims=True)
    t.dp = 2.0 * D + 4.0 * E_EXP + c + 1                                    # [K, N, 1, V]
    ep = t.dp * U * t.p
    m = t.p.mean(0)
    em = U * ((t.dp * t.p).sum(0) / k + k * m)
    t.ea = 0.99 * em + 4 * U * t.a
    t.eq = 0.99 * ep + 4 * U * t.q
    la, lq = np.abs(np.log(t.a)), np.abs(np.log(t.q))
    ela = t.ea / t.a + E_LOG * U * la
    elq = t.eq / t.q + E_LOG * U * lq
    t.edl = ela[None] + elq + U * (la[None] + lq)
    t.adl = (t.a[None] * np.abs(t.dl)).sum(2)                               # sum_c a |dl|  [K, N, V]
    t.e_var = (t.ea[None] * np.abs(t.dl) + t.a[None] * t.edl).sum(2) + (c + 1) * U * t.adl
    t.ee = t.e * (t.e_var + E_EXP * U)
    t.d = t.a[None] - t.q
    t.ed = t.ea[None] + t.eq + U * np.abs(t.d)
    t.es = (2 * np.abs(t.d) * t.ed).sum(2) + (c + 1) * U * t.s
    t.ese = t.es * t.e + t.s * t.ee + U * t.s * t.e
    return t


def pyramid_ref(z, gs=1.0):
    """float64 values of the forward with their bounds: r.out [4 K + 2], r.bound [4 K + 2] (A_k, B_k, V_k, L_k, loss_reg, 0)"""
    k, n, c, v = z.shape
    M = float(n) * v
    r = Ref()
    r.k, r.c, r.M = k, c, M
    r.out = pyramid_fwd(z)
    aout, adz = autograd_pyramid(z, gs)
    mag = np.maximum(np.abs(aout), 1e-300)
    assert (np.abs(aout - r.out) <= 1e-11 * mag).all(), (aout, r.out)
    dz = pyramid_bwd(z, r.out, gs)
    assert float(np.abs(adz - dz).max()) <= 1e-11 * max(float(np.abs(dz).max()), 1e-300), "closed-form gradient differs from autograd"
    t = _errors(z)
    ra, floor = SO.ra_ssl(v), n * v * c * ETA
    r.bound = np.zeros(4 * k + 2)
    for i in range(k):
        eA = GAMMA_SLACK * (float(t.ese[i].sum()) + ra * U * float((t.s[i] * t.e[i]).sum())) + floor
        eB = GAMMA_SLACK * (float(t.ee[i].sum()) + ra * U * float(t.e[i].sum())) + floor
        eV = GAMMA_SLACK * (float(t.e_var[i].sum()) + ra * U * float(t.adl[i].sum())) + floor
        A, B = r.out[4 * i], r.out[4 * i + 1]
        den = B / M + 1e-8
        eL = eA / (c * M * den) + (A / (c * M)) / (den * den) * eB / M + eV / M
        r.bound[4 * i:4 * i + 4] = eA, eB, eV, eL * (1 + 1e-9) + 1e-15 * abs(r.out[4 * i + 3])
    r.bound[4 * k] = r.bound[3:4 * k:4].sum() / k + 1e-15 * abs(r.out[4 * k])
    return r


def check_pyramid_fwd(r, got, what=""):
    """device out [4 K + 2] against the reference -> dict of error / bound ratios (asserted <= 1)"""
    k, c, M = r.k, r.c, r.M
    got = np.asarray(got, np.float64)
    assert got.shape == (4 * k + 2,) and got[4 * k + 1] == 0.0, (what, got.shape)
    res = {}
    names = ("A", "B", "V", "L")
    for i in range(k):
        for j in range(4):
            res["%s%d" % (names[j], i + 1)] = ratio(got[4 * i + j], r.out[4 * i + j], r.bound[4 * i + j])
        A, B, V = got[4 * i:4 * i + 3]
        first = (abs(A) / (c * M)) / (B / M + 1e-8)
        res["L%d.own" % (i + 1)] = ratio(got[4 * i + 3], scale_loss(A, B, V, c, M), 16 * EPS64 * (first + abs(V) / M))
    res["loss"] = ratio(got[4 * k], r.out[4 * k], r.bound[4 * k])
    res["loss.own"] = ratio(got[4 * k], got[3:4 * k:4].sum() / k, 16 * EPS64 * float(np.abs(got[3:4 * k:4]).sum()) / k)
    bad = {n: x for n, x in res.items() if not x <= 1.0}
    assert not bad, "%s: error / bound = %s" % (what, bad)
    return res


def pyramid_grad_ref(z, out_got, gs):
    """float64 dz for the DEVICE's sums A_k, B_k, with its bound -> (dz, bound), both [K, N, C, V]"""
    k, n, c, v = z.shape
    M = float(n) * v
    out_got = np.asarray(out_got, np.float64)
    dz = pyramid_bwd(z, out_got, gs)
    t = _errors(z)
    g = abs(float(np.float32(gs)))
    G, eg, h2, eh2 = [], [], [], []
    for i in range(k):
        den = out_got[4 * i + 1] / M + 1e-8
        al, be = 1.0 / (c * M * den), abs((out_got[4 * i] / (c * M)) / (den * den) / M)
        T2 = al * t.s[i] + be
        et2 = al * t.es[i] + 2 * U * al * t.s[i] + U * be + U * T2
        Gi = 1.0 / M + t.e[i] * T2
        G.append(Gi)
        eg.append(t.ee[i] * T2 + t.e[i] * et2 + U * t.e[i] * T2 + U / M + U * Gi)
        h2.append(2 * al * t.e[i])
        eh2.append(2 * (al * t.ee[i] + 2 * U * al * t.e[i]))
    adl, ad = np.abs(t.dl), np.abs(t.d)
    MT = np.zeros((n, c, v))
    eT = np.zeros((n, c, v))
    for i in range(k):
        Gi, egi, hi, ehi = G[i][:, None], eg[i][:, None], h2[i][:, None], eh2[i][:, None]
        MT += Gi * (adl[i] + 1) + hi * ad[i]
        eT += egi * (adl[i] + 1) + Gi * (t.edl[i] + 2 * U * (adl[i] + 1)) + ehi * ad[i] + hi * t.ed[i] + U * hi * ad[i]
    MT /= k
    eT = eT / k + (2 * k + 1) * U * MT
    w = 0.99 / k
    bound = np.zeros((k, n, c, v))
    for j in range(k):
        Gj, egj, hj, ehj = G[j][:, None], eg[j][:, None], h2[j][:, None], eh2[j][:, None]
        R = Gj * t.a / t.q[j]
        er = egj * t.a / t.q[j] + Gj * t.ea / t.q[j] + Gj * t.a * t.eq[j] / t.q[j] ** 2 + 2 * U * R
        X = hj * ad[j]
        ex = ehj * ad[j] + hj * t.ed[j] + U * X
        GP = w * (MT + R + X)
        egp = w * (eT + er + ex + 5 * U * (MT + R + X))
        p, dp = t.p[j], t.dp[j]
        S = g * p * (GP + (p * GP).sum(1, keepdims=True))
        inner = egp + (p * egp + dp * U * p * GP).sum(1, keepdims=True)
        bound[j] = GAMMA_SLACK * (g * p * inner + (dp + c + 5) * U * S) + ETA * (1 + g * (GP + GP.sum(1, keepdims=True)))
    return dz, bound


# ---------------------------------------------------------------- CPS's pseudo labels

def pseudo_onehot(z):
    """[.., C, V] logits (axis -2 is C) -> float32 one-hot of the first maximum of the LOGITS"""
    idx = np.argmax(z, axis=-2)
    return np.ascontiguousarray(np.moveaxis(np.eye(z.shape[-2], dtype=np.float32)[idx], -1, -2))


def grid_is_separated(z):
    """the precondition of the bit-for-bit comparison with get_soft_label(argmax(softmax)): every logit on the grid j / 8"""
    return bool(np.array_equal(z * 8, np.round(z * 8)) and np.abs(z).max() <= 4.0)
