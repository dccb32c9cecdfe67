"""numpy restatement of confident learning as fplx.confident runs it: what the reference's get_confident_map gets from cleanlab
1.0's get_noise_indices(s, psx, prune_method=...) with frac_noise = 1, MIN_NUM_PER_CLASS = 5 and calibrate = True.

Parity with cleanlab ITSELF is unpinned: cleanlab is installed on no machine this project is built or tested on, so this file is
written from the algorithm's description, not checked against a cleanlab
run - the GeodisTK precedent of fplx/evaluation.py.  It is written from that text, not from the kernels.

psx is float32 PLANAR [C, M], s uint8 / integer [M].  Every intermediate is exposed on the result of `run`:
thr (float64, the exactly rounded float64 sum of the members' values divided once), thr_err (what a float64 sum in another
order may differ from it by), joint, calibrated, P, ne, class_cut, pair_cut, pair_active, the three masks, and `undecided`: the
voxels whose double(psx) lies within thr_err of thr - 1e-6, the only ones a different summation order could decide differently.

Softmax bound (the derivation of tests/lossoracle.py, oracle B): u = 2^-24, E_EXP = 3 ulp = 6 u for expf; with D = max_k (max -
x_k) of a voxel the relative error of a probability is dp(D) = (2 D + 4 E_EXP + C + 1) u - x - max rounds (<= u D in each
exponent: numerator and sum), two expf, C - 1 additions of positive terms, one division - times GAMMA_SLACK = 1.01 for the
second-order products, plus ETA = 2^-126 absolute where expf's result is denormal and may be flushed."""
import math

import numpy as np

U = 2.0 ** -24
E_EXP = 6.0
GAMMA_SLACK = 1.01
ETA = 2.0 ** -126
METHODS = ("prune_by_class", "prune_by_noise_rate", "both")
FORCED_CASES = ((2, 70001, 11), (4, 70001, 12))            # (C, M, seed) of the softmax-route tests


class Result(object):
    pass


def round_preserving_sum(row):
    row = np.asarray(row, np.float64)
    ints = np.round(row)                                    # half to even
    target = np.round(row.sum())
    while target != ints.sum():
        d = target - ints.sum()
        inc = 1 if d > 0 else -1
        order = np.argsort(row - ints, kind="stable")[::-inc]
        for i in order[:int(min(abs(d), row.size))]:
            ints[i] += inc
    return ints.astype(np.int64)


def round_rows(mat):
    return np.stack([round_preserving_sum(r) for r in np.asarray(mat, np.float64)])


def thresholds(s, psx):
    c = psx.shape[0]
    cnt = np.array([(s == k).sum() for k in range(c)], np.int64)
    sums = np.array([math.fsum(psx[k][s == k].astype(np.float64)) for k in range(c)], np.float64)
    mag = np.array([math.fsum(np.abs(psx[k][s == k]).astype(np.float64)) for k in range(c)], np.float64)
    thr = sums / cnt
    # a float64 sum of n terms in any order: <= (n - 1) 2^-53 sum |x| (1 + O(n 2^-53)); the division and the quotient's use add 2 ulp
    thr_err = (cnt * 2.0 ** -53 * mag * 1.01) / cnt + 4 * 2.0 ** -53 * np.abs(thr)
    return cnt, sums, thr, thr_err


def confident_joint(s, psx, thr):
    c, m = psx.shape
    p64 = psx.astype(np.float64)
    conf = p64 >= (thr - 1e-6)[:, None]
    nc = conf.sum(0)
    guess = np.where(nc == 1, conf.argmax(0), psx.argmax(0))
    joint = np.zeros((c, c), np.int64)
    ok = nc > 0
    np.add.at(joint, (s[ok].astype(np.int64), guess[ok]), 1)
    return joint


def calibrate(joint, cnt):
    joint = joint.astype(np.float64)
    cnt = cnt.astype(np.float64)
    cal = (joint.T / joint.sum(axis=1) * cnt).T
    cal = cal / cal.sum() * cnt.sum()
    return round_rows(cal)


def keep_at_least_n_per_class(P, n=5):
    P = np.asarray(P, np.float64)
    diag = np.diagonal(P).copy()
    nd = np.maximum(diag, n)
    diff = nd - diag
    nn = np.maximum(np.count_nonzero(P, axis=0) - 1, 1)
    P = np.clip(P - diff / nn, 0, None)
    np.fill_diagonal(P, nd)
    return round_rows(P)


def run(s, psx):
    """every intermediate of the algorithm"""
    s = np.asarray(s)
    psx = np.ascontiguousarray(psx, np.float32)
    c, m = psx.shape
    r = Result()
    r.counts, r.sums, r.thr, r.thr_err = thresholds(s, psx)
    r.undecided = int((np.abs(psx.astype(np.float64) - (r.thr - 1e-6)[:, None]) <= r.thr_err[:, None]).any(0).sum())
    r.joint = confident_joint(s, psx, r.thr)
    r.calibrated = calibrate(r.joint, r.counts)
    r.P = keep_at_least_n_per_class(r.calibrated.T, 5)
    r.ne = r.counts - np.diagonal(r.P)
    r.class_cut = np.zeros(c, np.float32)
    r.pair_cut = np.zeros((c, c), np.float32)
    r.pair_active = np.zeros((c, c), np.uint8)
    by_class = np.zeros(m, bool)
    by_rate = np.zeros(m, bool)
    for k in range(c):
        mem = s == k
        vals = np.sort(psx[k][mem])
        r.class_cut[k] = vals[r.ne[k]]
        by_class |= mem & (psx[k] < r.class_cut[k])
        for j in range(c):
            n_jk = int(r.P[j][k])
            if j == k or n_jk <= 0:
                continue
            margin = psx[j] - psx[k]                        # float32, one rounding
            cut = np.sort(margin[mem])[::-1][n_jk - 1]
            r.pair_cut[k][j] = cut
            r.pair_active[k][j] = 1
            by_rate |= mem & (margin >= cut)
    wrong = psx.argmax(0) != s
    r.masks = {"prune_by_class": by_class & wrong, "prune_by_noise_rate": by_rate & wrong, "both": by_class & by_rate & wrong}
    return r


# ---------------------------------------------------------------- inputs

def exact_case(seed, c, m, flip=0.15, levels=None):
    """(s uint8 [m], psx float32 planar [c, m]) built like the worked example: seeded true labels, `flip` of them redrawn, normal
    logits with +2 at the true class, rounded to multiples of 1/16 (sums and margins are exact in any order).  levels: clip the
    values to that many distinct multiples per class, so that many voxels tie at every cut."""
    rng = np.random.default_rng(seed)
    true = rng.integers(0, c, m)
    s = true.copy()
    f = rng.random(m) < flip
    s[f] = rng.integers(0, c, int(f.sum()))
    lg = rng.normal(0, 1, (m, c)).astype(np.float32)
    lg[np.arange(m), true] += 2
    psx = np.round(lg * 16) / 16
    if levels is not None:
        psx = np.clip(np.round(psx), 0, levels - 1)
    return s.astype(np.uint8), np.ascontiguousarray(psx.T.astype(np.float32))


def logits_case(seed, c, m, flip=0.15, scale=1.0):
    """random normal logits for the softmax routes: (s, x planar [c, m])"""
    rng = np.random.default_rng(seed)
    true = rng.integers(0, c, m)
    s = true.copy()
    f = rng.random(m) < flip
    s[f] = rng.integers(0, c, int(f.sum()))
    lg = (rng.normal(0, 1, (m, c)) * scale).astype(np.float32)
    lg[np.arange(m), true] += np.float32(2)
    return s.astype(np.uint8), np.ascontiguousarray(lg.T)


def softmax64(x):
    """float64 softmax over axis 0 of float32 logits and the per-element bound of the fp32 kernel's result"""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    c = x64.shape[0]
    mx = x64.max(0, keepdims=True)
    e = np.exp(x64 - mx)
    p = e / e.sum(0, keepdims=True)
    D = mx - x64.min(0, keepdims=True)
    dp = (2.0 * D + 4.0 * E_EXP + c + 1) * U
    return p, GAMMA_SLACK * dp * p + ETA


def decision_distance(s, psx, r):
    """per voxel, the smallest distance of a compared quantity to what it is compared with: psx[k] to thr[k] - 1e-6 (all k),
    psx[s] to class_cut[s], the margins psx[j] - psx[s] to pair_cut[s][j] (active pairs), and the two largest values to each
    other (the argmax)."""
    s = np.asarray(s).astype(np.int64)
    p = psx.astype(np.float64)
    c, m = p.shape
    d = np.abs(p - (r.thr - 1e-6)[:, None]).min(0)
    own = p[s, np.arange(m)]
    d = np.minimum(d, np.abs(own - r.class_cut.astype(np.float64)[s]))
    for j in range(c):
        act = r.pair_active[s, j] > 0
        dj = np.abs((p[j] - own) - r.pair_cut.astype(np.float64)[s, j])
        d = np.where(act, np.minimum(d, dj), d)
    top = np.sort(p, axis=0)
    return np.minimum(d, top[-1] - top[-2])
