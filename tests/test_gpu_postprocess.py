"""Connected components and KeepLargestComponent on the GPU (csrc/postprocess.hip through fplx.ops / fplx.postprocess /
SegmentationAgent) against the scipy restatement of tests/test_postprocess_cpu.py and the reference's fixture."""
import os

import numpy as np
import pytest
import torch

import detdata
from test_postprocess_cpu import canonical_labels, keep_largest_ref

pytestmark = pytest.mark.gpu


def _snake3d(shape):
    """one-voxel-wide boustrophedon path through every other row of every other plane, planes joined at alternating
    corners: one component that crosses every tile many times"""
    d, h, w = shape
    s = np.zeros(shape, np.uint8)
    corner = []
    for z in range(0, d, 2):
        rows = list(range(0, h, 2))
        for k, y in enumerate(rows):
            s[z, y, :] = 1
            if k + 1 < len(rows):
                s[z, y + 1, w - 1 if k % 2 == 0 else 0] = 1
        last_x = w - 1 if (len(rows) - 1) % 2 == 0 else 0
        corner.append((z, rows[-1], last_x))
    for z, y, x in corner[:-1]:
        s[z + 1, y, x] = 1
    return s


def _spiral2d(n):
    s = np.zeros((n, n), np.uint8)
    lo, hi = 0, n - 1
    while lo <= hi:
        s[lo, lo:hi + 1] = 1
        s[lo:hi + 1, hi] = 1
        s[hi, lo:hi + 1] = 1
        s[lo + 2:hi + 1, lo] = 1
        if lo + 2 <= hi:
            s[lo + 2, lo:lo + 3] = 1
        lo += 2
        hi -= 2
    return s


def _comb(shape):
    s = np.zeros(shape, np.uint8)
    s[:, 0, :] = 1
    s[:, :, ::2] = 1
    s[::3, 1:, 1::4] = 2
    return s


def _checker(shape):
    zz, yy, xx = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    return (((zz + yy + xx) % 2) * (1 + (xx // 3) % 3)).astype(np.uint8)


def _smooth_classes(name, shape, ncls):
    f = detdata.normal(name, shape).astype(np.float64)
    for ax in range(3):
        f = (f + np.roll(f, 1, ax) + np.roll(f, -1, ax) + np.roll(f, 2, ax)) / 4.0
    q = np.floor((f - f.min()) / (f.max() - f.min() + 1e-12) * ncls).astype(np.int64)
    return np.clip(q, 0, ncls - 1).astype(np.uint8)


def _percolation(name, shape, p, ncls=1):
    u = detdata.uniform(name, shape)
    c = (detdata.uniform(name + ".c", shape) * ncls).astype(np.uint8) + 1
    return np.where(u < p, c, 0).astype(np.uint8)


def realistic(name, shape):
    """the argmax of a smooth random two-class map plus a few islands (an inference-like mask)"""
    f = detdata.normal(name, shape).astype(np.float64)
    for _ in range(3):
        for ax in range(3):
            f = (np.roll(f, -2, ax) + np.roll(f, -1, ax) + f + np.roll(f, 1, ax) + np.roll(f, 2, ax)) / 5.0
    s = (f > 0.25 * f.std()).astype(np.uint8)
    u = detdata.uniform(name + ".islands", (30, 3))
    for row in u:
        z, y, x = [int(row[a] * (shape[a] - 2)) for a in range(3)]
        s[z:z + 2, y:y + 2, x:x + 1] = 1
    return s


def small_cases():
    out = []
    for p in (0.05, 0.2, 0.31, 0.45, 0.7, 0.95):
        out.append(("perc%.2f" % p, _percolation("pp.perc%.2f" % p, (19, 45, 83), p, 3)))
    out.append(("perc2d", _percolation("pp.perc2d", (131, 197), 0.55, 2)))
    out.append(("snake", _snake3d((7, 69, 150))))
    out.append(("spiral", _spiral2d(259)))
    out.append(("spiral3d", np.stack([_spiral2d(97)] * 3)))
    out.append(("comb", _comb((5, 70, 141))))
    out.append(("checker", _checker((9, 20, 31))))
    out.append(("full", np.ones((6, 33, 70), np.uint8)))
    out.append(("full255", np.full((3, 17, 129), 255, np.uint8)))
    out.append(("empty", np.zeros((5, 21, 67), np.uint8)))
    corners = np.zeros((9, 70, 131), np.uint8)
    for z in (0, -1):
        for y in (0, -1):
            for x in (0, -1):
                corners[z, y, x] = 1 + (z & 1) + 2 * (y & 1) + 4 * (x & 1)
    out.append(("corners", corners))
    out.append(("single", np.ones((1, 1, 1), np.uint8)))
    for shp in ((1, 1, 300), (1, 300, 1), (300, 1, 1), (7, 1, 130), (1, 70, 1), (65, 65, 1), (3, 129, 65)):
        out.append(("thin%s" % (shp,), _percolation("pp.thin%s" % (shp,), shp, 0.6, 2)))
    out.append(("cls255", _smooth_classes("pp.cls255", (13, 40, 70), 256)))
    out.append(("cls255rand", _percolation("pp.cls255rand", (11, 31, 77), 0.9, 255)))
    return out


def big_cases():
    return [("real48", realistic("pp.real48", (48, 160, 272))), ("perc48", _percolation("pp.perc48", (48, 160, 272), 0.31)),
            ("real128", realistic("pp.real128", (128, 256, 256))), ("perc128", _percolation("pp.perc128", (128, 256, 256), 0.31))]


def _check_labels_and_keep(name, seg):
    import fplx
    t = torch.from_numpy(seg).cuda()
    for per_class in (False, True):
        got = fplx.ops.connected_components(t, per_class=per_class).cpu().numpy()
        assert got.dtype == np.int32 and got.shape == seg.shape
        want = canonical_labels(seg, per_class)
        assert np.array_equal(got, want), (name, per_class, int((got != want).sum()))
    for mode in (1, 2):
        got = fplx.ops.keep_largest_component(t, mode).cpu().numpy()
        assert np.array_equal(got, keep_largest_ref(seg, mode)), (name, mode)


@pytest.mark.parametrize("case", [c[0] for c in small_cases()])
def test_labels_and_keep_largest_match_scipy(case):
    seg = dict(small_cases())[case]
    _check_labels_and_keep(case, seg)


def test_labels_and_keep_largest_match_scipy_at_inference_sizes():
    for name, seg in big_cases():
        _check_labels_and_keep(name, seg)


def test_cases_are_what_they_claim():
    cases = dict(small_cases())
    assert canonical_labels(cases["snake"]).max() == 0                 # one component, first voxel 0
    assert canonical_labels(cases["spiral"]).max() == 0
    lab = canonical_labels(cases["checker"])                           # all singletons
    assert np.array_equal(lab[lab >= 0], np.flatnonzero(cases["checker"].ravel()))
    assert cases["cls255"].max() == 255 and len(np.unique(cases["cls255"])) > 100
    assert cases["perc0.31"].any() and not cases["empty"].any()


def test_matches_the_reference_fixture(golden_dir):
    import fplx
    z = np.load(os.path.join(golden_dir, "postprocess.npz"))
    for n in [str(v) for v in z["names"]]:
        seg = z[n + ".seg"]
        for mode in (1, 2):
            want = z["%s.mode%d" % (n, mode)]
            assert np.array_equal(fplx.PostKeepLargestComponent({"keeplargestcomponent_mode": mode})(seg), want), (n, mode)
            t = torch.from_numpy(seg).cuda()
            assert np.array_equal(fplx.ops.keep_largest_component(t, mode).cpu().numpy(), want)
        if seg.any():
            g = fplx.get_largest_k_components(seg)
            assert g.dtype == seg.dtype and np.array_equal(g, (z[n + ".mode1"] > 0).astype(seg.dtype))


def test_numpy_and_tensor_contract():
    import fplx
    seg = _percolation("pp.contract", (6, 20, 30), 0.4, 3).astype(np.int64)
    p = fplx.PostKeepLargestComponent({"keeplargestcomponent_mode": 2})
    out = p(seg)
    assert isinstance(out, np.ndarray) and out.dtype == np.int64 and np.array_equal(out, keep_largest_ref(seg, 2))
    t = torch.from_numpy(seg.astype(np.uint8)).cuda()
    o2 = p(t)
    assert isinstance(o2, torch.Tensor) and o2.is_cuda and np.array_equal(o2.cpu().numpy(), out)
    empty = np.zeros((4, 5, 6), np.uint8)
    assert fplx.get_largest_k_components(empty) is empty
    assert not p(empty).any() and not fplx.PostKeepLargestComponent({})(empty).any()
    m = fplx.get_largest_k_components(torch.from_numpy((seg > 0).astype(np.uint8)).cuda())
    assert m.is_cuda and np.array_equal(m.cpu().numpy(), (keep_largest_ref(seg, 1) > 0).astype(np.uint8))


def test_repeated_runs_are_bitwise_identical():
    import fplx
    for name, seg in big_cases():
        t = torch.from_numpy(seg).cuda()
        runs = [(fplx.ops.connected_components(t, per_class=True).cpu().numpy(), fplx.ops.keep_largest_component(t, 2).cpu().numpy())
                for _ in range(3)]
        for lab, keep in runs[1:]:
            assert np.array_equal(lab, runs[0][0]) and np.array_equal(keep, runs[0][1]), name


# ---- end to end through SegmentationAgent.save_outputs
class _FixedInferer(object):
    """stands in for the sliding-window inferer: speckled two-class logits, a pure function of the input's shape, so that
    the argmax masks have many components"""

    def run(self, model, image, domain_label=None):
        shp = (image.shape[0], 2) + tuple(image.shape[2:])
        return torch.from_numpy(detdata.normal("pp.e2e%s" % (shp,), shp)).to(image.device)


def test_agent_writes_post_processed_masks(tmp_path):
    import fplx
    from fplx import nifti
    rs = np.random.RandomState(3)
    root = tmp_path / "data"
    (root / "img").mkdir(parents=True)
    shapes = [(11, 30, 37), (9, 33, 40)]
    for i, shp in enumerate(shapes):
        nifti.write_nifti(str(root / "img" / ("c%d.nii.gz" % i)), rs.randn(*shp) * 40 + 150, (0.5, 0.6, 1.2), (3.0, -4.0, 5.0))
    (tmp_path / "test.csv").write_text("image\nimg/c0.nii.gz\nimg/c1.nii.gz\n")
    net_cfg = dict(net_type="UNet2D5_dsbn", in_chns=1, feature_chns=[8, 16, 32, 32, 32], dropout=[0.0, 0.0, 0.2, 0.2, 0.2],
                   conv_dims=[3, 3, 3, 3, 3], class_num=2, bilinear=False, num_domains=2, precision="fp32")
    testing = {"gpus": [0], "domian_label": 1, "evaluation_mode": True}
    config = {
        "dataset": {"root_dir": str(root), "test_csv": str(tmp_path / "test.csv"), "tensor_type": "float",
                    "test_transform": ["NormalizeWithMeanStd", "Pad"], "normalizewithmeanstd_channels": [0],
                    "pad_output_size": [16, 32, 48], "pad_inverse": True},
        "network": net_cfg,
        "training": {"ckpt_save_dir": "model/vs_t1s_g", "random_seed": 1},
        "testing": dict(testing),
    }
    torch.manual_seed(0)
    agent = fplx.SegmentationAgent(config, "test")
    agent.create_dataset()
    agent.create_network()
    agent.set_inferer(_FixedInferer())

    def run(tag, **extra):
        config["testing"] = dict(testing, output_dir=str(tmp_path / tag), **extra)
        agent.postprocessor = None                       # built again from this run's testing section
        out = agent.infer()
        d = tmp_path / tag / "vs_t1s_g_test"
        assert sorted(os.listdir(str(d))) == ["c0.nii.gz", "c1.nii.gz"]
        files = [nifti.load_nifty_volume_as_4d_array(str(d / ("c%d.nii.gz" % i)))["data_array"][0] for i in range(2)]
        return {k: v.cpu().numpy() for k, v in out.items()}, files

    # today's contract: no post_process, the files are the argmax masks infer() returns
    raw_out, raw = run("raw")
    for i in range(2):
        assert raw[i].shape == shapes[i] and np.array_equal(raw[i], raw_out["img/c%d.nii.gz" % i])
        assert not np.array_equal(keep_largest_ref(raw[i], 1), raw[i])          # the masks have islands to remove
    # mode 1 (the default)
    out, files = run("pp1", post_process="KeepLargestComponent")
    assert isinstance(agent.postprocessor, fplx.PostKeepLargestComponent) and agent.postprocessor.mode == 1
    for i in range(2):
        assert np.array_equal(files[i], keep_largest_ref(raw[i], 1))
        assert np.array_equal(out["img/c%d.nii.gz" % i], raw[i])               # infer() still returns the raw masks
    # mode 2 after label conversion, in the reference's order (convert_label, then the post-processor)
    _, files = run("pp2", post_process="KeepLargestComponent", keeplargestcomponent_mode=2, label_source=[0, 1],
                   label_target=[1, 0])
    for i in range(2):
        conv = (raw[i] == 0).astype(np.uint8)
        assert np.array_equal(files[i], keep_largest_ref(conv, 2))
    # a plugin's own numpy post-processor wins over the config's
    calls = []

    def mine(seg):
        assert isinstance(seg, np.ndarray) and seg.dtype == np.uint8 and seg.ndim == 3
        calls.append(seg.shape)
        return (seg == 0).astype(np.uint8) * 3

    agent.set_postprocessor(mine)
    config["testing"] = dict(testing, output_dir=str(tmp_path / "mine"), post_process="KeepLargestComponent")
    agent.infer()
    assert sorted(calls) == sorted(shapes)
    for i in range(2):
        got = nifti.load_nifty_volume_as_4d_array(str(tmp_path / "mine" / "vs_t1s_g_test" / ("c%d.nii.gz" % i)))["data_array"][0]
        assert np.array_equal(got, (raw[i] == 0).astype(np.uint8) * 3)
    # an unknown name fails as the reference's dictionary lookup does
    agent.postprocessor = None
    config["testing"] = dict(testing, output_dir=str(tmp_path / "bad"), post_process="KeepLargestComponents")
    with pytest.raises(KeyError):
        agent.infer()
