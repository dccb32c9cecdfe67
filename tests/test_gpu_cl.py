"""-m gpu tests of the confident-learning kernels (csrc/cl.hip through fplx.ops / fplx.confident) against tests/cloracle.py:
on inputs whose values are multiples of 1/16 every count, sum, threshold, cut and mask exactly; the softmax inside its derived
bound; on the softmax routes the oracle fed with the device's own psx buffer exactly (decisions forced) and the scipy-fed oracle
different only next to a threshold or a cut; the modes; two runs for the same bits; the tool end to end on three NIfTI cases."""
import functools
import os

import numpy as np
import pytest
import torch

import cloracle as O

pytestmark = pytest.mark.gpu

EXACT = [(2, 210), (3, 384), (4, 2310), (8, 4096), (2, 70001)]   # scalar path; vector path; ...; the class limit; several blocks + a tail


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()             # a copy: the cached inputs are read-only


def host(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def exact(c, m, levels=None):
    s, psx = O.exact_case(1000 * c + m if (c, m) != (2, 210) else 0, c, m, levels=levels)
    psx.setflags(write=False)
    s.setflags(write=False)
    return s, psx, O.run(s, psx)


def check_against(a, r, method, s, psx):
    """a: fplx.confident.NoiseAnalysis of `method`, r: the oracle's result on the same psx"""
    c = psx.shape[0]
    assert np.array_equal(a.counts, r.counts) and a.counts_all[c] == 0 and a.counts_all[c + 1] == 0
    assert np.array_equal(a.joint, r.joint)
    assert np.array_equal(a.calibrated, r.calibrated) and np.array_equal(a.P, r.P) and np.array_equal(a.ne, r.ne)
    if method != "prune_by_noise_rate":
        assert np.array_equal(host(a.class_cut), r.class_cut)
    if method != "prune_by_class":
        assert np.array_equal(a.pair_active, r.pair_active)
        on = r.pair_active > 0
        assert np.array_equal(host(a.pair_cut)[on], r.pair_cut[on])
    want = r.masks[method]
    got = host(a.mask)
    assert got.dtype == np.uint8 and set(np.unique(got)) <= {0, 1}
    assert np.array_equal(got.astype(bool), want), (method, int(got.sum()), int(want.sum()))
    assert int(host(a.count)[0]) == int(want.sum())


# ---------------------------------------------------------------- exact

@pytest.mark.parametrize("method", O.METHODS)
@pytest.mark.parametrize("c,m", EXACT)
def test_exact_inputs_equal_the_oracle(c, m, method):
    from fplx import confident
    s, psx, r = exact(c, m)
    assert r.counts.min() > 5 and r.undecided == 0 and (r.joint.sum(1) > 0).all()          # nothing refused, nothing skipped
    assert (r.ne < r.counts).all() and (r.P.T <= r.counts[:, None]).all()
    a = confident.analyse(dev(s), dev(psx), method, planar=True)
    assert np.array_equal(a.sums, r.sums) and np.array_equal(a.thr, r.thr)                 # exact sums: any order, one division
    check_against(a, r, method, s, psx)
    if (c, m) == (2, 210) and method == "both":
        assert int(host(a.count)[0]) == 13                                                  # the worked example


def test_numpy_in_numpy_out_and_the_row_major_layout():
    import fplx
    s, psx, r = exact(3, 384)
    got = fplx.get_noise_indices(s, np.ascontiguousarray(psx.T), "both")
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got.astype(bool), r.masks["both"])
    got = fplx.get_noise_indices(dev(s), dev(np.ascontiguousarray(psx.T)))                  # the default method is cleanlab's
    assert isinstance(got, torch.Tensor) and got.is_cuda and np.array_equal(host(got).astype(bool), r.masks["prune_by_noise_rate"])
    joint, thr, counts = fplx.compute_confident_joint(s, np.ascontiguousarray(psx.T))
    assert np.array_equal(joint, r.joint) and np.array_equal(thr, r.thr) and np.array_equal(counts, r.counts)
    got = fplx.get_confident_map(s.astype(np.int64), np.ascontiguousarray(psx.T), "Cij")    # labels of another integer type
    assert np.array_equal(got.astype(bool), r.masks["both"])


def test_misaligned_base_falls_back_to_one_voxel_per_lane():
    from fplx import confident, ops
    c, m = 3, 384
    s, psx, r = exact(c, m)
    buf = torch.zeros(c * m + 1, dtype=torch.float32, device="cuda")
    view = buf[1:].view(c, m)
    view.copy_(dev(psx))
    assert view.data_ptr() % 16 == 4
    sbuf = torch.zeros(m + 1, dtype=torch.uint8, device="cuda")
    sview = sbuf[1:]
    sview.copy_(dev(s))
    for method in O.METHODS:
        check_against(confident.analyse(sview, view, method, planar=True), r, method, s, psx)
    keys_a = ops.cl_select_keys(view, sview, 1, 2)
    keys_b = ops.cl_select_keys(dev(psx), dev(s), 1, 2)
    assert host(keys_a).tobytes() == host(keys_b).tobytes()


def test_select_keys():
    from fplx import ops
    s, psx, _ = exact(4, 2310)
    for k, j in ((0, -1), (3, -1), (1, 2), (2, 0)):
        got = host(ops.cl_select_keys(dev(psx), dev(s), k, j))
        want = np.where(s == k, psx[k] if j < 0 else -(psx[j] - psx[k]), np.float32(np.nan)).astype(np.float32)
        assert np.array_equal(np.isnan(got), s != k) and np.array_equal(got[s == k], want[s == k])


@pytest.mark.parametrize("c,m", [(3, 4096), (2, 1001)])
def test_ties_at_the_cuts(c, m):
    """psx takes 4 distinct values per class: many voxels tie at r and at cut, and are kept or dropped together"""
    from fplx import confident
    s, psx, r = exact(c, m, 4)
    assert all(len(np.unique(psx[k])) <= 4 for k in range(c))
    tied = [int((psx[k][s == k] == r.class_cut[k]).sum()) for k in range(c)]
    assert min(tied) > 10
    for method in O.METHODS:
        check_against(confident.analyse(dev(s), dev(psx), method, planar=True), r, method, s, psx)


def test_refusals_on_the_device_counts():
    import fplx
    s, psx, _ = exact(2, 210)
    bad = s.copy()
    bad[7] = 2
    with pytest.raises(ValueError, match="label >= 2"):
        fplx.get_noise_indices(bad, psx.T)
    p = psx.copy()
    p[1, 100] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        fplx.get_noise_indices(s, p.T)
    few = np.zeros(210, np.uint8)
    few[:5] = 1
    with pytest.raises(ValueError, match="class 1 has 5 voxels"):
        fplx.get_noise_indices(few, psx.T)


# ---------------------------------------------------------------- softmax

@pytest.mark.parametrize("c,m", [(2, 210), (3, 384), (8, 4096), (4, 70001)])
def test_softmax_is_inside_its_bound(c, m):
    from fplx import ops
    _, x = O.logits_case(100 + c, c, m, scale=3.0)
    x[:, :8] = np.array([0, -50, 20, -20, 1e-3, 10, -10, 5], np.float32)[None, :] * np.arange(1, c + 1, dtype=np.float32)[:, None]
    got = host(ops.cl_softmax(dev(x))).astype(np.float64)
    p, bound = O.softmax64(x)
    ratio = np.abs(got - p) / bound
    print("softmax c=%d m=%d: max |err| / bound = %.3f" % (c, m, ratio.max()))
    assert ratio.max() <= 1.0
    assert bound.max() < 1e-4                                                  # the bound is a test, not a blanket
    assert (np.abs(got.sum(0) - 1.0) <= bound.sum(0) + 2.0 ** -50).all()      # the planes of one voxel sum to 1 within the bound


# ---------------------------------------------------------------- decisions forced

@pytest.mark.parametrize("c,m,seed", O.FORCED_CASES)
def test_softmax_route_is_the_oracle_on_the_devices_psx(c, m, seed):
    from fplx import confident, ops
    from scipy.special import softmax
    s, x = O.logits_case(seed, c, m)
    psx_d = ops.cl_softmax(dev(x))
    psx = host(psx_d)
    r = O.run(s, psx)
    assert r.undecided == 0                    # no voxel within the summation-order error of its threshold
    masks = {}
    for method in O.METHODS:
        a = confident.analyse(dev(s), psx_d, method, planar=True)
        assert (np.abs(a.thr - r.thr) <= r.thr_err).all()
        check_against(a, r, method, s, psx)
        masks[method] = host(a.mask).astype(bool)
    got = host(confident.get_confident_map(dev(s), dev(x), "Qij", planar=True)).astype(bool)
    assert np.array_equal(got, r.masks["both"])
    # scipy's softmax instead of the device's: differences only where a compared value is within the bound of what it is compared with
    ps = softmax(x, axis=0).astype(np.float32)
    rs = O.run(s, ps)
    _, bound = O.softmax64(x)
    near = O.decision_distance(s, ps, rs) <= 2 * bound.max(0) + 2 * rs.thr_err.max()
    for method in O.METHODS:
        diff = rs.masks[method] != masks[method]
        print("c=%d %s: %d voxels differ from the scipy-fed oracle, %d near a decision" % (c, method, int(diff.sum()), int(near.sum())))
        assert not (diff & ~near).any()
    assert np.abs(rs.joint - r.joint).sum() <= 2 * near.sum()


# ---------------------------------------------------------------- modes, determinism

def test_modes_and_determinism():
    from fplx import confident
    c, m, seed = O.FORCED_CASES[0]
    s, x = O.logits_case(seed, c, m)
    ds, dx = dev(s), dev(x)
    out = {t: confident.get_confident_map(ds, dx, t, planar=True) for t in confident.CL_TYPES}
    again = {t: confident.get_confident_map(ds, dx, t, planar=True) for t in confident.CL_TYPES}
    for t in confident.CL_TYPES:
        assert out[t].dtype == torch.uint8 and host(out[t]).tobytes() == host(again[t]).tobytes(), t
    assert torch.equal(out["both"], out["Qij"])
    assert torch.equal(out["intersection"], out["Qij"] & out["Cij"])
    assert torch.equal(out["union"], out["Qij"] | out["Cij"])
    assert torch.equal(out["both"], out["prune_by_class"] & out["prune_by_noise_rate"])
    assert 0 < int(out["intersection"].sum()) <= int(out["union"].sum()) < m
    r = O.run(s, x)                                                           # Cij: the raw outputs as psx
    assert np.array_equal(host(out["Cij"]).astype(bool), r.masks["both"])


# ---------------------------------------------------------------- python -m fplx.nll_clslsr config.cfg

CL_CFG = """
[dataset]
tensor_type = float
task_type = seg
root_dir  = {root}
train_csv = {root}/train.csv
modal_num = 1

valid_transform = [NormalizeWithMeanStd, Pad, LabelToProbability]
NormalizeWithMeanStd_channels = [0]
NormalizeWithMeanStd_mean = None
NormalizeWithMeanStd_std  = None
NormalizeWithMeanStd_inverse = False
Pad_output_size = [16, 32, 32]
Pad_ceil_mode   = False
Pad_inverse     = True
LabelToProbability_class_num = 2
LabelToProbability_inverse   = False

[network]
net_type = UNet3D
class_num     = 2
in_chns       = 1
feature_chns  = [8, 8, 8, 8]
dropout       = [0.0, 0.0, 0.0, 0.0]
trilinear     = False
deep_supervise = False

[training]
gpus       = [0]
ckpt_save_dir    = {root}/model/cl
slsrloss_epsilon = 0.25

[testing]
gpus       = [0]
ckpt_mode  = 2
ckpt_name  = {root}/model/cl/seeded.pt
evaluation_mode   = True
sliding_window_enable = False
"""


def test_tool_end_to_end(tmp_path):
    import fplx
    from fplx import nifti, nll_clslsr
    from fplx.config import parse_config, synchronize_config
    root = tmp_path
    (root / "img").mkdir()
    (root / "lab").mkdir()
    (root / "model" / "cl").mkdir(parents=True)
    rs = np.random.RandomState(4)
    names, labs = [], []
    for i in range(3):
        shp = (16, 32, 32)
        lab = np.zeros(shp, np.uint8)
        lab[3:12, 6 + i:22 + i, 8:26] = 1
        img = rs.randn(*shp) * 15 + 90 + 70.0 * lab
        lab[1:4, 2:8, 20:30] = 1                              # partly wrong labels
        nifti.write_nifti(str(root / "img" / ("c%d.nii.gz" % i)), img.astype(np.float32), (0.5, 0.75, 1.5))
        nifti.write_nifti(str(root / "lab" / ("c%d.nii.gz" % i)), lab, (0.5, 0.75, 1.5))
        names.append("c%d.nii.gz" % i)
        labs.append(lab)
    (root / "train.csv").write_text("image,label\n" + "\n".join("img/%s,lab/%s" % (n, n) for n in names) + "\n")
    cfg = root / "cl.cfg"
    cfg.write_text(CL_CFG.format(root=str(root)))
    config = synchronize_config(parse_config(str(cfg)))
    torch.manual_seed(5)
    net = fplx.UNet3D(dict(config["network"]))
    torch.save({"model_state_dict": net.state_dict()}, str(root / "model" / "cl" / "seeded.pt"))
    agent = nll_clslsr.get_confidence_map(["fplx.nll_clslsr", str(cfg)])
    # the oracle on the agent's own logits
    logits, gt = host(agent.cl_logits), host(agent.cl_labels)
    assert logits.shape == (2, 3 * 16 * 32 * 32) and np.array_equal(gt, np.concatenate([l.reshape(-1) for l in labs]))
    psx = host(fplx.ops.cl_softmax(agent.cl_logits))
    r = O.run(gt, psx)
    assert r.undecided == 0
    want = r.masks["both"].reshape(3, 16, 32, 32)
    for i, n in enumerate(names):
        got = nifti.load_nifty_volume_as_4d_array(str(root / "slsr_conf" / n))
        ref = nifti.load_nifty_volume_as_4d_array(str(root / "lab" / n))
        vol = got["data_array"]
        assert vol.dtype == np.uint8 and vol.shape == ref["data_array"].shape and set(np.unique(vol)) <= {0, 255}
        for key in ("spacing", "origin", "direction"):
            assert np.array_equal(np.asarray(got[key]), np.asarray(ref[key])), key
        assert np.array_equal(vol.reshape(16, 32, 32) == 255, want[i]), n
    assert want.any()
    import pandas as pd
    df = pd.read_csv(str(root / "train_clslsr.csv"))
    assert list(df.columns) == ["image", "pixel_weight", "label"]
    assert list(df["pixel_weight"]) == ["slsr_conf/" + n for n in names] and list(df["label"]) == ["lab/" + n for n in names]
    # the second stage reads it: NiftyDataset -> SLSRLoss, one forward
    ds = fplx.NiftyDataset(str(root), str(root / "train_clslsr.csv"), 1, True, fplx.transform.Compose(agent.transform_list), "cuda:0")
    sample = ds[0]
    pw = sample["pixel_weight"][None]
    assert pw.shape == (1, 1, 16, 32, 32) and pw.dtype == torch.float32
    net.cuda().eval()
    with torch.no_grad():
        pred = net(sample["image"][None])
    loss = fplx.SLSRLoss(dict(config["training"]))({"prediction": pred, "ground_truth": sample["label_prob"][None], "pixel_weight": pw})
    assert torch.isfinite(loss).all()
