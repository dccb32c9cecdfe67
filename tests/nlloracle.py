"""Float64 oracle for the noisy-label kernels (fpl-plus_amd/csrc/nll.hip), on top of tests/lossoracle.py: same notation
(u = 2^-24, ETA, E_EXP, E_LOG, dp(D), GAMMA_SLACK) and NO new measured constant.

The passes under test.  K logit tensors [N, C, V] and one soft label y [N, C, V]; a voxel has the flat index n V + v.
    voxel_ce      p = softmax(logits_k), p' = 0.999 p + 5e-4, L_k = sum_c (-y_c) ln p'_c
    rank mask     the first num_remb entries of a STABLE ascending argsort of L (NaN last): every L < t, t = s[num_remb - 1], and
                  of the voxels with L == t the first num_remb - #{L < t} in index order
    below mask    L < torch.quantile(L, q): pos = float32(q) float32(n - 1) in fp32, k = floor(pos), w = pos - k,
                  thr = lerp(s[k], s[ceil(pos)], w) with torch's lerp in fp32; a NaN anywhere keeps nothing
    selected      keep_j = AND of the masks in uses[j];  out_j = (sum keep_j L_j, sum keep_j, their quotient, sum L_j)
    scalar        CoTeaching: out_0[2] + out_1[2];  TriNet: (out_0[2] + out_1[2] + out_2[2]) / 3
    gradient      e_c = -0.999 y_c / p'_c keep_j / count_j,  dlogits_j,c = gs w_j p_c (e_c - sum_i p_i e_i)
The closed forms are asserted against float64 autograd of the reference's own statements written with torch operations
(nll_co_teaching.py:100-118, nll_trinet.py:66-120), 1e-11 of the magnitude (`node`).

Exact part: the masks.  Comparisons and integer counts have no rounding: given the fp32 losses the device's masks must equal
`rank_mask` / `below_mask` of THOSE losses bit for bit, and the kept counts are exact.
Rounding part.  With D = max - min of a voxel's logits, dp(D) = 2 D + 4 E_EXP + C + 1 [u] is the relative error of a probability
(lossoracle), ep = dp u p.
    p'            epp = 0.999 ep + 4 u p'  (two constants, a product, a sum - not fused)
    ln p'         el = epp / p' + E_LOG u |ln p'|
    L             e_L = sum_c |y_c| el_c + (C + 1) u sum_c |y_c ln p'_c| + ETA   (the negation is exact; C products, C additions)
    sums          a lane adds its terms one after the other, then 6 shuffles and 3 additions in LDS; the rows are added in double.
                  sum of all L_k (the partial rows of voxel_ce, lossoracle's row geometry): sum e_L + (ROW_TERMS / 256 + 12) u sum |L|.
                  kept sum (a flat pass over n = N V: at most 1024 blocks of 256 lanes, a lane takes quads):
                  T(n) = 4 ceil((n / 4) / (256 G)) + 4 terms per lane, G = min(1024, max(1, ceil(n / 1024))), bound
                  sum_kept e_L + (T(n) + 9) u sum_kept |L|;  the mean divides by an exact count in double.
    selection     a voxel whose |L - thr| <= GAMMA_SLACK (e_L + e_thr) is UNDECIDED (the device may keep it or not); the fixtures
                  and cases are asserted to have none, so the float64 masks ARE the device's (`node`'s `undecided`).
    gradient      E_c = |e_c|, ee_c = E_c (epp_c / p'_c + 5 u) (p', the constant, product, quotient, product, 1 / count rounded
                  once); S_c = |g| p_c (E_c + sum_j p_j E_j), g = gs w_j (w_j = 1/3 rounded once, one product);
                  |err| <= GAMMA_SLACK (|g| p_c (ee_c + sum_j (p_j ee_j + dp u p_j E_j)) + (dp + C + 7) u S_c) + ETA (1 + |g| (E_c + sum E))
                  - ssloracle's gradient form with two more roundings for g.
    the reference The fixture tests/golden/nll_steps.npz holds what the reference computed in fp32 on the CPU.  Its per-voxel
                  losses obey e_L (torch's exp / log are inside E_EXP / E_LOG); its mean over m kept values is an fp32 sum in
                  SOME order - at most (m - 1) u sum |L| / m - and one division: ref_scalar_bound = sum_kept e_L / m + (m + 1) u
                  mean_kept |L| per network, added over the networks (+ 2 u |scalar| for the final additions / division).  Its
                  backward evaluates the same gradient expression with no more roundings than the kernel, so it obeys the
                  gradient bound too: device and fixture differ by at most the sum of their bounds.

Pure numpy / torch on the CPU; tests/test_nll_cpu.py checks the oracle itself, tests/test_gpu_nll.py applies it."""
import numpy as np
import torch

import lossoracle as LO
from lossoracle import U, ETA, E_EXP, E_LOG, GAMMA_SLACK, ratio  # noqa: F401

USES = {"CoTeaching": (2, 1), "TriNet": (6, 5, 3)}


# ---------------------------------------------------------------- generators

def logits_case(key, k, n, c, *spatial, noise=0.25):
    """K logit tensors [N, C, *spatial] around one base (the networks agree mostly) and a one-hot label [N, C, *spatial] that is
    the base's argmax with a share `noise` of the voxels relabelled at random - float32"""
    g = LO.rng(key)
    shape = (n, c) + tuple(spatial)
    base = g.standard_normal(shape) * 1.5
    logits = [np.ascontiguousarray((base + g.standard_normal(shape) * 0.7).astype(np.float32)) for _ in range(k)]
    cls = base.argmax(1)
    flip = g.random(cls.shape) < noise
    cls = np.where(flip, g.integers(0, c, cls.shape), cls)
    y = np.zeros(shape, np.float32)
    np.put_along_axis(y, cls[:, None], 1.0, 1)
    return logits, y


def tie_case(key, n, kind):
    """losses [n] float32 for the mask tests: 'equal' (one value), 'two' (two values in runs that cross every chunk boundary),
    'ties' (few distinct values), 'nan' (random with NaNs), 'random'"""
    g = LO.rng(key)
    if kind == "equal":
        return np.full(n, 0.75, np.float32)
    if kind == "two":
        return np.where((np.arange(n) // 7) % 2 == 0, 0.5, 0.25).astype(np.float32)
    if kind == "ties":
        return (g.integers(0, 5, n) / 4.0).astype(np.float32)
    x = g.random(n).astype(np.float32)
    if kind == "nan":
        x[g.random(n) < 0.1] = np.nan
        if n > 2:
            x[n // 2] = np.nan
    return x


# ---------------------------------------------------------------- exact part: keys, ranks, masks

def keys(x):
    """the order-preserving uint32 key of select_kth: negative floats all bits flipped, others sign bit set, every NaN 0xFFFFFFFF"""
    x = np.ascontiguousarray(x, np.float32)
    u = x.view(np.uint32)
    k = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isnan(x), np.uint32(0xFFFFFFFF), k)


def rank_mask(loss, num_remb):
    """bool [n]: every key below t = sorted_keys[num_remb - 1], and the first num_remb - #less of the keys equal to t in index order"""
    k = keys(loss)
    if num_remb <= 0:
        return np.zeros(k.shape, bool)
    t = np.sort(k)[num_remb - 1]
    less, eq = k < t, k == t
    need = num_remb - int(less.sum())
    return less | (eq & (np.cumsum(eq) <= need))


def quantile_rank(q, n):
    """(k, w) of torch.quantile on n float32 values: the rank is formed in float32"""
    pos = np.float32(q) * np.float32(n - 1)
    k = np.floor(pos)
    if k >= n - 1:
        return n - 1, np.float32(0.0)
    return int(k), np.float32(pos - k)


def lerp32(a, b, w):
    """torch's lerp on float32 scalars: a + w (b - a) below w = 0.5, else b - (b - a) (1 - w)"""
    a, b, w = np.float32(a), np.float32(b), np.float32(w)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.float32(b - a)
        return np.float32(a + np.float32(w * d)) if w < 0.5 else np.float32(b - np.float32(d * np.float32(np.float32(1.0) - w)))


def quantile32(loss, q):
    """torch.quantile(loss, q) of a float32 array, restated: NaN if any NaN"""
    x = np.asarray(loss, np.float32).reshape(-1)
    if np.isnan(x).any():
        return np.float32(np.nan)
    s = np.sort(x)
    k, w = quantile_rank(q, x.size)
    return lerp32(s[k], s[k] if w == 0 else s[min(k + 1, x.size - 1)], w)


def below_mask(loss, q):
    with np.errstate(invalid="ignore"):
        return np.asarray(loss, np.float32) < quantile32(loss, q)


# ---------------------------------------------------------------- float64 closed forms with bounds

def _softmax(l):
    m = l.max(1, keepdims=True)
    e = np.exp(l - m)
    return e / e.sum(1, keepdims=True)


def _dp(l64, c):
    D = l64.max(1, keepdims=True) - l64.min(1, keepdims=True)
    return 2.0 * D + 4.0 * E_EXP + c + 1


class Ref(object):
    pass


def voxel_ce(logits, y):
    """one network: logits, y [N, C, V] -> Ref with L [N V] float64, e_L [N V] (the bound of an fp32 evaluation), p, pp, epp, dp"""
    l64, y64 = logits.astype(np.float64), y.astype(np.float64)
    n, c, v = l64.shape
    r = Ref()
    r.p = _softmax(l64)
    r.dp = _dp(l64, c)
    r.pp = 0.999 * r.p + 5e-4
    r.epp = 0.999 * r.dp * U * r.p + 4 * U * r.pp
    ln = np.log(r.pp)
    el = r.epp / r.pp + E_LOG * U * np.abs(ln)
    r.L = (-y64 * ln).sum(1).reshape(-1)
    r.e_L = ((np.abs(y64) * el).sum(1) + (c + 1) * U * np.abs(y64 * ln).sum(1)).reshape(-1) + ETA
    return r


def ce_fp32(logits, y):
    """the kernel's expression operation by operation in float32 with numpy's exp / log (saturated cases: exact values)"""
    f = np.float32
    l = logits.astype(f)
    m = l.max(1, keepdims=True)
    e = np.exp(l - m).astype(f)
    s = np.zeros_like(m)
    for c in range(l.shape[1]):
        s = (s + e[:, c:c + 1]).astype(f)
    p = (e / s).astype(f)
    pp = ((p * f(0.999)).astype(f) + f(5e-4)).astype(f)
    acc = np.zeros(l[:, 0].shape, f)
    for c in range(l.shape[1]):
        acc = (acc + ((-y[:, c].astype(f)) * np.log(pp[:, c]).astype(f)).astype(f)).astype(f)
    return acc.reshape(-1), pp


def all_sum_bound(r, n, v):
    """bound of sum over all voxels of L (voxel_ce's partial rows, then double)"""
    return GAMMA_SLACK * (float(r.e_L.sum()) + (LO.row_terms(v) / 256 + 12) * U * float(np.abs(r.L).sum()))


def lane_terms(n):
    g = min(1024, max(1, -(-n // 1024)))
    return 4 * (-(-(-(-n // 4)) // (256 * g))) + 4


def kept_sum_bound(r, keep):
    n = r.L.size
    return GAMMA_SLACK * (float(r.e_L[keep].sum()) + (lane_terms(n) + 9) * U * float(np.abs(r.L[keep]).sum()))


def selected(refs, masks, uses):
    """-> out [K, 4] float64 and its bounds [K, 4] (the count's bound is 0), keeps: list of bool [n]"""
    k = len(refs)
    out, bound, keeps = np.zeros((k, 4)), np.zeros((k, 4)), []
    for j in range(k):
        keep = np.ones(refs[j].L.shape, bool)
        for i in range(k):
            if uses[j] >> i & 1:
                keep &= np.asarray(masks[i], bool)
        keeps.append(keep)
        s, m = float(refs[j].L[keep].sum()), int(keep.sum())
        out[j] = (s, m, s / m if m else np.nan, float(refs[j].L.sum()))
        bound[j, 0] = kept_sum_bound(refs[j], keep)
        bound[j, 2] = bound[j, 0] / m if m else 0.0
    return out, bound, keeps


def grad(r, y, keep, count, g):
    """closed form and bound of dlogits of one network [N, C, V]; keep [n] bool; g = gs w_j as float64"""
    n, c, v = r.p.shape
    y64 = y.astype(np.float64)
    kj = (keep.reshape(n, 1, v) / count) if count else np.zeros((n, 1, v))
    e = -0.999 * y64 / r.pp * kj
    dot = (r.p * e).sum(1, keepdims=True)
    d = g * r.p * (e - dot)
    E = np.abs(e)
    ee = E * (r.epp / r.pp + 5 * U)
    S = abs(g) * r.p * (E + (r.p * E).sum(1, keepdims=True))
    err = GAMMA_SLACK * (abs(g) * r.p * (ee + (r.p * ee + r.dp * U * r.p * E).sum(1, keepdims=True)) + (r.dp + c + 7) * U * S) \
        + ETA * (1 + abs(g) * (E + E.sum(1, keepdims=True)))
    return d, err


def autograd_node(logits_list, y, mode, masks, gs):
    """the reference's statements in float64 with the masks given -> (scalar, per-network means, grads)"""
    Ls = [torch.from_numpy(l.astype(np.float64)).requires_grad_(True) for l in logits_list]
    y2 = torch.from_numpy(y.astype(np.float64))
    c = y2.shape[1]
    y2d = y2.reshape(y2.shape[0], c, -1).permute(0, 2, 1).reshape(-1, c)
    loss = []
    for L in Ls:
        prob = torch.softmax(L, dim=1)
        p2d = prob.reshape(prob.shape[0], c, -1).permute(0, 2, 1).reshape(-1, c) * 0.999 + 5e-4
        loss.append(torch.sum(-y2d * torch.log(p2d), dim=1))
    mk = [torch.from_numpy(np.asarray(m, bool)) for m in masks]
    if mode == "CoTeaching":
        means = [loss[0][mk[1]].mean(), loss[1][mk[0]].mean()]
        total = means[0] + means[1]
    else:
        m12, m13, m23 = (mk[0] & mk[1]).double(), (mk[0] & mk[2]).double(), (mk[1] & mk[2]).double()
        means = [torch.sum(loss[0] * m23) / m23.sum(), torch.sum(loss[1] * m13) / m13.sum(), torch.sum(loss[2] * m12) / m12.sum()]
        total = (means[0] + means[1] + means[2]) / 3
    (total * gs).backward()
    return total.item(), [m.item() for m in means], [L.grad.numpy() for L in Ls]


def num_remb_of(ratio, n):
    return int(ratio * n)


def node(logits_list, y, mode, ratio, gs=1.0):
    """the whole node in float64: logits [N, C, *spatial] -> Ref with refs (per network), masks, keeps, out, out_bound, scalar,
    scalar_bound, grads, grad_bounds, undecided (voxels whose side of the threshold an fp32 evaluation may change),
    ref_scalar_bound (an fp32 torch evaluation's own error, see the module text)"""
    k = len(logits_list)
    n, c = y.shape[0], y.shape[1]
    v = int(np.prod(y.shape[2:]))
    y3 = y.reshape(n, c, v)
    refs = [voxel_ce(l.reshape(n, c, v), y3) for l in logits_list]
    nv = n * v
    r = Ref()
    r.refs, r.masks, r.undecided = refs, [], 0
    for rf in refs:
        if mode == "CoTeaching":
            nr = num_remb_of(ratio, nv)
            m = _rank64(rf.L, nr)
            # undecided: the num_remb-th and the next loss closer than their bounds
            if 0 < nr < nv:
                order = np.argsort(rf.L, kind="stable")
                a, b = order[nr - 1], order[nr]
                if rf.L[b] - rf.L[a] <= GAMMA_SLACK * (rf.e_L[a] + rf.e_L[b]):
                    r.undecided += 1
        else:
            s = np.sort(rf.L)
            kq, w = quantile_rank(ratio, nv)
            a, b = s[kq], (s[kq] if w == 0 else s[min(kq + 1, nv - 1)])
            thr = a + float(w) * (b - a)
            m = rf.L < thr
            e_thr = rf.e_L.max() + 4 * U * abs(thr)
            r.undecided += int((np.abs(rf.L - thr) <= GAMMA_SLACK * (rf.e_L + e_thr)).sum()) if w > 0 else \
                int(((np.abs(rf.L - thr) <= GAMMA_SLACK * (rf.e_L + e_thr)) & (rf.L != thr)).sum())
        r.masks.append(m)
    uses = USES[mode]
    r.out, r.out_bound, r.keeps = selected(refs, r.masks, uses)
    wj = 1.0 if mode == "CoTeaching" else float(np.float32(1.0 / 3.0))
    r.scalar = float(r.out[:, 2].sum()) if mode == "CoTeaching" else float(r.out[:, 2].sum()) / 3.0
    r.scalar_bound = float(r.out_bound[:, 2].sum()) * (1.0 if mode == "CoTeaching" else 1.0 / 3.0) + 3 * U * abs(r.scalar)
    g = float(np.float32(gs)) * wj
    r.grads, r.grad_bounds = [], []
    for j in range(k):
        d, e = grad(refs[j], y3, r.keeps[j], int(r.out[j, 1]), g)
        r.grads.append(d.reshape(logits_list[j].shape))
        r.grad_bounds.append(e.reshape(logits_list[j].shape))
    ref_b = 0.0
    for j in range(k):
        keep, m = r.keeps[j], int(r.out[j, 1])
        if m:
            ref_b += float(refs[j].e_L[keep].sum()) / m + (m + 1) * U * float(np.abs(refs[j].L[keep]).mean())
    r.ref_scalar_bound = GAMMA_SLACK * ref_b * (1.0 if mode == "CoTeaching" else 1.0 / 3.0) + 3 * U * abs(r.scalar)
    # the closed forms against float64 autograd of the reference's statements
    if all(int(x) > 0 for x in r.out[:, 1]):
        tot, means, ag = autograd_node(logits_list, y, mode, r.masks, float(np.float32(gs)))
        assert abs(tot - r.scalar) <= 1e-11 * max(abs(tot), 1e-300), (tot, r.scalar)
        for j in range(k):
            gj = r.grads[j] * (1.0 if mode == "CoTeaching" else (1.0 / 3.0) / wj)
            assert float(np.abs(ag[j] - gj).max()) <= 1e-11 * max(float(np.abs(gj).max()), 1e-300), "closed-form gradient differs from autograd"
    return r


def _rank64(L, num_remb):
    """rank_mask on float64 values (no NaN): the first num_remb of a stable ascending argsort"""
    m = np.zeros(L.shape, bool)
    m[np.argsort(L, kind="stable")[:num_remb]] = True
    return m
