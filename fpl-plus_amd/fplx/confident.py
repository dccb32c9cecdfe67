"""Confident learning: which labels of a training set are suspect (the pixel_weight > 0 mask SLSRLoss smooths with).

What the reference's get_confident_map (PyMIC/pymic/net_run_nll/nll_clslsr.py:19-46) gets from cleanlab 1.0's
get_noise_indices(s, psx, prune_method=...) with its defaults frac_noise = 1, MIN_NUM_PER_CLASS = 5, calibrate = True, as
streaming passes over psx fp32 planar [C, M] and the labels s uint8 [M] (csrc/cl.hip):

  1. thr[k] = mean of psx[k] over s == k                               (cl_class_stats: float64 sum in a fixed order, one division)
  2. the confident joint, joint[s][guess]                              (cl_confident_joint)
  3. calibration and 4. the prune counts P[true][given], C x C, float64 on the host after ONE device -> host read
  5. by class: the ne-th smallest psx[k] of class k, 6. by noise rate: the m-th largest margin psx[j] - psx[k]
                                                                       (cl_select_keys + select_kth; the cuts stay on the device)
  7. the mask, and pred != s                                           (cl_noise_mask)

Different from cleanlab, on purpose: the thresholds are float64 (cleanlab: float32 pairwise mean and a float32 thr - 1e-6); all
C classes are always present in the joint (cleanlab's tables shrink when a class is absent); a class with 5 voxels or fewer, a
joint row that sums to 0, a prune count that reaches the class size, a label >= C and a NaN in psx are refused with ValueError
(cleanlab skips, divides by zero or sorts the NaN somewhere).  cleanlab is installed on no machine this project is built or
tested on: parity with cleanlab itself is unpinned (tests/cloracle.py restates the algorithm in numpy).

numpy in gives numpy out, a device tensor in gives a device tensor out; there is no CPU path."""
import numpy as np
import torch

from . import ops

PRUNE_METHODS = {"prune_by_class": ops.CL_BY_CLASS, "prune_by_noise_rate": ops.CL_BY_NOISE_RATE, "both": ops.CL_BOTH}
CL_TYPES = ("both", "Qij", "Cij", "intersection", "union", "prune_by_class", "prune_by_noise_rate")
MIN_NUM_PER_CLASS = 5


# ---------------------------------------------------------------- the C x C host part (float64)

def round_preserving_sum(row):
    """cleanlab's round_preserving_sum: round half to even, then move the entries with the largest (smallest) remainders by one
    until the integers add up to the rounded total of the row"""
    row = np.asarray(row, np.float64)
    ints = np.round(row)
    target = np.round(row.sum())
    while target != ints.sum():
        d = target - ints.sum()
        inc = 1 if d > 0 else -1
        order = np.argsort(row - ints, kind="stable")[::-inc]
        ints[order[:int(min(abs(d), row.size))]] += inc
    return ints.astype(np.int64)


def _round_rows(mat):
    return np.stack([round_preserving_sum(r) for r in np.asarray(mat, np.float64)])


def calibrate_confident_joint(joint, counts):
    """joint int64 [C, C] (joint[given][guess]), counts [C] -> the calibrated joint: rows scaled to the class counts, the whole
    to the number of voxels, every row rounded with its total preserved"""
    joint = np.asarray(joint, np.float64)
    counts = np.asarray(counts, np.float64)
    rows = joint.sum(axis=1)
    if (rows == 0).any():
        k = int(np.flatnonzero(rows == 0)[0])
        raise ValueError("fplx confident: no voxel labelled {0:} is confident of any class (its row of the confident joint is "
                         "empty); the noise map is undefined".format(k))
    cal = (joint.T / rows * counts).T
    cal = cal / cal.sum() * counts.sum()
    return _round_rows(cal)


def keep_at_least_n_per_class(P, n=MIN_NUM_PER_CLASS):
    """P[true][given] -> the prune counts with at least n voxels kept on the diagonal, what is added there taken evenly from
    the rest of the column, rows rounded with their totals preserved"""
    P = np.array(P, np.float64)
    diag = np.diagonal(P).copy()
    nd = np.maximum(diag, n)
    nn = np.maximum(np.count_nonzero(P, axis=0) - 1, 1)
    P = np.clip(P - (nd - diag) / nn, 0, None)
    np.fill_diagonal(P, nd)
    return _round_rows(P)


# ---------------------------------------------------------------- inputs

def _to_device(s, psx, planar):
    """-> (s uint8 [M], psx float32 planar [C, M], host): host = the inputs were numpy arrays"""
    host = not isinstance(psx, torch.Tensor)
    if host != (not isinstance(s, torch.Tensor)):
        raise ValueError("fplx confident: labels and psx must both be numpy arrays or both device tensors")
    if len(psx.shape) != 2 or len(s.shape) != 1:
        raise ValueError("fplx confident: labels [M] and psx {0:} expected, got {1:} and {2:}".format(
            "[C, M]" if planar else "[M, C]", tuple(s.shape), tuple(psx.shape)))
    c, m = (int(psx.shape[0]), int(psx.shape[1])) if planar else (int(psx.shape[1]), int(psx.shape[0]))
    if not 2 <= c <= 8:
        raise ValueError("fplx confident: {0:} classes (2..8 supported)".format(c))
    if int(s.shape[0]) != m:
        raise ValueError("fplx confident: {0:} labels for {1:} voxels".format(int(s.shape[0]), m))
    if m >= 1 << 31:
        raise ValueError("fplx confident: {0:} voxels, fewer than 2^31 supported (select_kth's bound)".format(m))
    if host:
        if not torch.cuda.is_available():
            raise RuntimeError("fplx: confident learning runs on the GPU (HIP path only, no CPU fallback)")
        s = torch.from_numpy(np.require(s, requirements=["C", "W"])).cuda()              # a read-only array is copied first
        psx = torch.from_numpy(np.require(psx, np.float32, ["C", "W"])).cuda()
    ops.require_gpu(s, psx)
    if not planar:
        psx = psx.t()
    if psx.dtype != torch.float32 or not psx.is_contiguous():
        psx = psx.to(torch.float32).contiguous()
    if s.dtype != torch.uint8:
        if s.dtype.is_floating_point or s.dtype == torch.bool:
            s = s.to(torch.int64)
        s = torch.where((s < 0) | (s > 255), 255, s).to(torch.uint8)        # 255 >= C: counted and refused below
    return s.contiguous(), psx, host


class NoiseAnalysis(object):
    """every intermediate of one run: counts, sums, thr, joint, calibrated, P, ne (host numpy); class_cut, pair_cut (device),
    pair_active (host); mask uint8 [M] and count int64 [1] (device)"""


def refuse_counts(counts_all):
    """counts_all int64 [C + 2] of cl_class_stats (classes | labels >= C | voxels with a NaN): what cannot give a map raises"""
    c = len(counts_all) - 2
    if counts_all[c] != 0:
        raise ValueError("fplx confident: {0:} voxels carry a label >= {1:} (psx has {1:} classes)".format(int(counts_all[c]), c))
    if counts_all[c + 1] != 0:
        raise ValueError("fplx confident: {0:} voxels have a NaN in psx".format(int(counts_all[c + 1])))
    for k in range(c):
        if counts_all[k] <= MIN_NUM_PER_CLASS:
            raise ValueError("fplx confident: class {0:} has {1:} voxels; more than {2:} are needed (cleanlab would skip the class "
                             "and the map would mean nothing for it)".format(k, int(counts_all[k]), MIN_NUM_PER_CLASS))


def _joint(s, psx):
    c = psx.shape[0]
    sums, counts, thr = ops.cl_class_stats(psx, s)
    joint = ops.cl_confident_joint(psx, s, thr)
    # the one device -> host read: counts | joint | the bits of thr and sums
    h = torch.cat([counts, joint.reshape(-1), thr.view(torch.int64), sums.view(torch.int64)]).cpu().numpy()
    a = NoiseAnalysis()
    a.counts_all = h[:c + 2].copy()
    a.counts = h[:c].copy()
    a.joint = h[c + 2:c + 2 + c * c].reshape(c, c).copy()
    a.thr = h[c + 2 + c * c:c + 2 + c * c + c].copy().view(np.float64)
    a.sums = h[c + 2 + c * c + c:].copy().view(np.float64)
    a.thr_dev = thr
    refuse_counts(a.counts_all)
    return a


def compute_confident_joint(s, psx, planar=False):
    """-> (joint int64 [C, C], thr float64 [C], counts int64 [C]) as numpy arrays: joint[given][guess] over the voxels that are
    confident of at least one class"""
    s, psx, _ = _to_device(s, psx, planar)
    a = _joint(s, psx)
    return a.joint, a.thr, a.counts


def analyse(s, psx, prune_method="prune_by_noise_rate", planar=False):
    """get_noise_indices with every intermediate kept (NoiseAnalysis); s, psx as there"""
    if prune_method not in PRUNE_METHODS:
        raise ValueError("fplx confident: prune_method {0:} is not one of {1:}".format(prune_method, sorted(PRUNE_METHODS)))
    s, psx, host = _to_device(s, psx, planar)
    c, m = int(psx.shape[0]), int(psx.shape[1])
    a = _joint(s, psx)
    a.host = host
    a.calibrated = calibrate_confident_joint(a.joint, a.counts)
    a.P = keep_at_least_n_per_class(a.calibrated.T, MIN_NUM_PER_CLASS)
    a.ne = a.counts - np.diagonal(a.P)
    method = PRUNE_METHODS[prune_method]
    dev = psx.device
    keys = torch.empty(m, dtype=torch.float32, device=dev)
    a.class_cut = a.pair_cut = None
    a.pair_active = np.zeros((c, c), np.uint8)
    if method != ops.CL_BY_NOISE_RATE:
        a.class_cut = torch.zeros(c, dtype=torch.float32, device=dev)
        for k in range(c):
            if not 0 <= a.ne[k] < a.counts[k]:
                raise ValueError("fplx confident: class {0:} would lose {1:} of its {2:} voxels".format(k, int(a.ne[k]), int(a.counts[k])))
            ops.cl_select_keys(psx, s, k, -1, out=keys)
            a.class_cut[k].copy_(ops.select_kth(keys, [int(a.ne[k])])[0, 0])
    if method != ops.CL_BY_CLASS:
        a.pair_cut = torch.zeros((c, c), dtype=torch.float32, device=dev)
        for k in range(c):
            for j in range(c):
                n_jk = int(a.P[j][k])
                if j == k or n_jk <= 0:
                    continue
                if n_jk > a.counts[k]:
                    raise ValueError("fplx confident: {0:} voxels labelled {1:} are to be pruned as class {2:}, the class has {3:}".format(
                        n_jk, k, j, int(a.counts[k])))
                ops.cl_select_keys(psx, s, k, j, out=keys)
                torch.neg(ops.select_kth(keys, [n_jk - 1])[0, 0], out=a.pair_cut[k, j])      # the key is the negated margin
                a.pair_active[k, j] = 1
    a.mask, a.count = ops.cl_noise_mask(psx, s, method, a.class_cut, a.pair_cut, a.pair_active)
    return a


def get_noise_indices(s, psx, prune_method="prune_by_noise_rate", planar=False):
    """cleanlab.pruning.get_noise_indices(s, psx, prune_method): s the given labels [M], psx [M, C] (planar=True: a device tensor
    [C, M], used without a transpose) -> uint8 mask [M], 1 = the label is suspect"""
    a = analyse(s, psx, prune_method, planar)
    return a.mask.cpu().numpy() if a.host else a.mask


def get_confident_map(gt, pred, CL_type="both", planar=False):
    """nll_clslsr.py:19-46: gt the given labels [M], pred the network's raw outputs [M, C] (planar=True: device [C, M]).
    'both' / 'Qij': both prune rules on the softmax; 'Cij': on pred itself; 'intersection' / 'union': the two combined;
    'prune_by_class' / 'prune_by_noise_rate': that rule on the softmax.  -> uint8 mask [M]"""
    if CL_type not in CL_TYPES:
        raise ValueError("fplx confident: CL_type {0:} is not one of {1:}".format(CL_type, list(CL_TYPES)))
    s, x, host = _to_device(gt, pred, planar)
    need_q = CL_type != "Cij"
    prob = ops.cl_softmax(x) if need_q else None
    if CL_type in ("both", "Qij"):
        noise = analyse(s, prob, "both", True).mask
    elif CL_type == "Cij":
        noise = analyse(s, x, "both", True).mask
    elif CL_type in ("intersection", "union"):
        q, cij = analyse(s, prob, "both", True).mask, analyse(s, x, "both", True).mask
        noise = (q & cij) if CL_type == "intersection" else (q | cij)
    else:
        noise = analyse(s, prob, CL_type, True).mask
    return noise.cpu().numpy() if host else noise
