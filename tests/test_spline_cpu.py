"""CPU tests of cubic-spline resampling and the dataset preparation tools:
 - tests/splineoracle.py, the numpy restatement of csrc/spline.hip's rules, against scipy.ndimage.zoom(order=3) and
   spline_filter themselves, with the counts printed; its outside mask against scipy's zeros; the derived bound against the
   restatement's own error and against the cap;
 - the reflection and weight rules against brute force;
 - the C ABI's refusals, which run before any launch;
 - the host logic of fplx.resample (the kernels replaced by the restatement) and fplx.preprocess (crop boxes against a literal
   restatement of data/preprocess_vs.py, the spacing permutation, the command line's parser)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import detdata
import resample_ref as R
import splineoracle as S

SHAPES = [(12, 40, 50), (9, 33, 31), (1, 37, 29), (7, 1, 23), (11, 19, 1), (5, 5, 5), (16, 32, 48), (3, 64, 17), (13, 27, 45),
          (2, 3, 2), (40, 64, 64)]
ZOOMS = [(4.0 / 3, 1.2, 0.96), (0.83, 1.21, 0.9), (2.0, 2.0, 2.0), (0.5, 0.5, 0.5), (1.0, 0.7, 1.6), (1.37, 1.41, 1.96)]


@pytest.fixture(scope="module")
def against_scipy():
    """the restatement against scipy over every shape and zoom, computed once: totals and the largest float64 distances in
    units of max|x|"""
    from scipy import ndimage
    r = {"total": 0, "differing": 0, "outside": 0, "interp": 0.0, "filter": 0.0}
    for shape in SHAPES:
        x = (detdata.normal("sp.cpu%s" % (shape,), (1,) + shape) * 100.0).astype(np.float32)
        xmax = float(np.abs(x).max())
        coef = S.prefilter(x)
        ref = ndimage.spline_filter(x[0].astype(np.float64), 3, output=np.float64, mode="mirror")
        r["filter"] = max(r["filter"], float(np.abs(coef[0] - ref).max()) / xmax)
        for zoom in ZOOMS:
            out = R.zoom_size(shape, zoom)
            if min(out) < 1:
                continue
            m, t = R.zoom_affine(shape, out)
            ref32 = ndimage.zoom(x, [1.0] + list(zoom), order=3)
            ref64 = ndimage.zoom(x, [1.0] + list(zoom), order=3, output=np.float64)
            got64 = S.interpolate(coef, m, t, out, np.float64)
            mask = S.outside(shape, m, t, out)
            assert not ref32[:, mask].any() and not ref64[:, mask].any(), (shape, zoom)      # the mask is scipy's zeros
            assert ref64[:, ~mask].all(), (shape, zoom)                                      # and nothing else is 0
            r["outside"] += int(mask.sum())
            r["total"] += got64.size
            r["differing"] += int((got64.astype(np.float32) != ref32).sum())
            r["interp"] = max(r["interp"], float(np.abs(got64 - ref64).max()) / xmax)
    return r


def test_restatement_equals_scipy(against_scipy):
    r = against_scipy
    print("restatement vs scipy.ndimage.zoom(order=3): %d outputs, %d float32 elements not identical, %d outside; largest "
          "float64 distance 2^%.1f max|x| (zoom), 2^%.1f max|x| (spline_filter)" % (
              r["total"], r["differing"], r["outside"], math.log2(r["interp"]), math.log2(r["filter"])))
    assert r["total"] >= 100000 and r["outside"] > 0
    assert r["differing"] <= S.MAX_DIFFERING_SHARE * r["total"]


def test_bound_covers_the_restatement_and_stays_under_the_cap(against_scipy):
    for xmax in (1.0, 437.5):
        assert S.prefilter_bound(xmax) <= S.interp_bound(xmax) <= S.CAP * xmax
    assert against_scipy["interp"] <= S.interp_bound(1.0) and against_scipy["filter"] <= S.prefilter_bound(1.0)
    # the constants of the derivation: the pole, the gain 6, the per-axis figure below K, a wrong tap far above B
    a = abs(S.Z)
    r = 1.0 / (1.0 - a)
    assert abs(S.GAIN - 6.0) < 1e-14 and abs(a * r - 0.366) < 1e-3
    startup = 7.6 * (a * r * r + 6 * a * r) + 28 * 6 * r + 6.01 * r + 3 * 6 * r
    causal = startup + 24 * r + (1 + 2 * a) * 6 * r * r
    output = a * r * causal + 18 + 9 * r
    print("per-axis rounding figure %.0f u A (start-up %.0f, causal %.0f); K = %.0f" % (output, startup, causal, S.K_AXIS))
    assert output <= S.K_AXIS
    assert 2.0 ** -10 > 1000 * S.interp_bound(1.0)


def test_outside_mask_matters():
    """a restatement without the mask is wrong by about max|x| at the far border"""
    from scipy import ndimage
    hits = 0
    for shape in SHAPES[:2]:
        x = (detdata.normal("sp.cpu.mask", (1,) + shape) * 100.0).astype(np.float32)
        for zoom in ZOOMS:
            out = R.zoom_size(shape, zoom)
            m, t = R.zoom_affine(shape, out)
            mask = S.outside(shape, m, t, out)
            if not mask.any():
                continue
            hits += 1
            ref = ndimage.zoom(x, [1.0] + list(zoom), order=3)
            assert not ref[:, mask].any() and not S.resample(x, m, t, out)[:, mask].any()
            c, _ = S.coordinates(shape, m, t, out)
            assert max(float((ci - (n - 1)).max()) for ci, n in zip(c, shape)) < 1e-12      # outside by an ulp or so, no more
    assert hits > 0


def test_reflection_against_brute_force():
    for n in (1, 2, 3, 4, 5, 9):
        if n == 1:
            table = {i: 0 for i in range(-12, 13)}
        else:
            walk = list(range(n)) + list(range(n - 2, 0, -1))          # one period of the mirror image
            table = {i: walk[i % len(walk)] for i in range(-4 * n, 4 * n + 1)}
        idx = np.array(sorted(table))
        assert list(S.reflect(idx, n)) == [table[i] for i in idx], n


def test_weights_against_the_cubic_b_spline():
    def beta3(x):
        x = abs(x)
        return 2.0 / 3 - x * x + x ** 3 / 2 if x < 1 else ((2 - x) ** 3 / 6 if x < 2 else 0.0)
    c = np.concatenate([np.linspace(0.0, 7.0, 113), [3.0, 2.9999999999, 0.5, 1e-12]])
    f, w = S.weights(c)
    assert np.array_equal(f, np.floor(c).astype(np.int64))
    for k in range(4):
        want = np.array([beta3(ci - (fi - 1 + k)) for ci, fi in zip(c, f)])
        assert np.abs(w[k] - want).max() <= 8 * S.U, k
        assert (w[k] >= -4 * S.U).all()
    assert np.abs(sum(w) - 1.0).max() <= 4 * S.U
    # on a sample (c = 3.0) the weights are (1/6, 4/6, 1/6, 0)
    assert float(c[113]) == 3.0 and abs(float(w[0][113]) - 1.0 / 6) <= S.U and abs(float(w[1][113]) - 4.0 / 6) <= S.U
    assert abs(float(w[2][113]) - 1.0 / 6) <= S.U and abs(float(w[3][113])) <= 2 * S.U


def test_prefilter_inverts_the_interpolation_at_the_samples():
    """the defining property: the spline through the coefficients passes through the samples"""
    x = (detdata.normal("sp.cpu.identity", (2, 6, 7, 9)) * 100.0).astype(np.float32)
    got = S.resample(x, np.eye(3), np.zeros(3), x.shape[1:], np.float64)
    assert np.abs(got - x).max() <= S.interp_bound(float(np.abs(x).max()))


def test_abi_rejects_bad_arguments_before_any_launch():
    from fplx import _lib
    lib = _lib.lib()
    x = (ctypes.c_float * 64)()
    y = (ctypes.c_float * 64)()
    coef = (ctypes.c_double * 64)()
    m = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    t = (ctypes.c_double * 3)()
    bad_extents = ((0, 4, 4, 4), (1, 0, 4, 4), (1, 4, -1, 4), (1, 4, 4, 0), (2, 1 << 10, 1 << 10, 1 << 10),
                   (1 << 30, 1 << 30, 1 << 30, 1 << 30))
    f = lib.fplx_spline_prefilter
    assert f(None, coef, 1, 4, 4, 4, 3, None) == -5
    assert f(x, None, 1, 4, 4, 4, 3, None) == -5 and "spline_prefilter" in _lib.last_error()
    for c, d, h, w in bad_extents:
        assert f(x, coef, c, d, h, w, 3, None) == -1, (c, d, h, w)
    for order in (-1, 0, 1, 2, 4, 5):
        assert f(x, coef, 1, 4, 4, 4, order, None) == -1 and "built: 3" in _lib.last_error(), order
    g = lib.fplx_resample_spline
    assert g(None, y, 1, 4, 4, 4, 4, 4, 4, m, t, 3, None) == -5
    assert g(coef, None, 1, 4, 4, 4, 4, 4, 4, m, t, 3, None) == -5
    assert g(coef, y, 1, 4, 4, 4, 4, 4, 4, None, t, 3, None) == -5
    assert g(coef, y, 1, 4, 4, 4, 4, 4, 4, m, None, 3, None) == -5 and "resample_spline" in _lib.last_error()
    for c, d, h, w in bad_extents:
        assert g(coef, y, c, d, h, w, 4, 4, 4, m, t, 3, None) == -1, (c, d, h, w)
    for od, oh, ow in ((0, 4, 4), (4, -1, 4), (4, 4, 0), (1 << 11, 1 << 10, 1 << 10), (1 << 30, 1 << 30, 1 << 30)):
        assert g(coef, y, 1, 4, 4, 4, od, oh, ow, m, t, 3, None) == -1, (od, oh, ow)
    for order in (-1, 0, 1, 2, 4, 5):
        assert g(coef, y, 1, 4, 4, 4, 4, 4, 4, m, t, order, None) == -1 and "built: 3" in _lib.last_error(), order
    with pytest.raises(ValueError, match="built: 3"):
        _lib.check(g(coef, y, 1, 4, 4, 4, 4, 4, 4, m, t, 2, None))
    # the order-0 / order-1 entry point still refuses order 3: the spline has its own
    assert lib.fplx_resample_affine(x, y, 4, 3, 1, 4, 4, 4, 4, 4, 4, m, t, None) == -1
    assert {"fplx_spline_prefilter", "fplx_resample_spline"} <= set(_lib.declared_symbols())
    import fplx
    with pytest.raises(RuntimeError, match="must live on the GPU"):                          # no CPU fallback
        fplx.ops.spline_prefilter(torch.zeros((1, 4, 4, 4)))
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        fplx.ops.resample_spline(torch.zeros((1, 4, 4, 4)), np.eye(3), (0, 0, 0), (4, 4, 4))


# ---- host logic of fplx.resample on the restatement

@pytest.fixture
def host_resample(monkeypatch):
    """fplx.resample with the kernels replaced by the numpy restatements and the device check switched off; the calls are
    recorded"""
    from fplx import ops, resample
    calls = []

    def affine(x, matrix, offset, out_size, order):
        calls.append(("affine", order, [list(r) for r in matrix], list(offset), list(out_size)))
        return torch.from_numpy(R.resample_affine(x.numpy(), matrix, offset, [int(v) for v in out_size], order))

    def spline(x, matrix, offset, out_size, order=3):
        calls.append(("spline", order, [list(r) for r in matrix], list(offset), list(out_size)))
        return torch.from_numpy(S.resample(x.numpy(), matrix, offset, [int(v) for v in out_size]))

    monkeypatch.setattr(ops, "resample_affine", affine)
    monkeypatch.setattr(ops, "resample_spline", spline)
    monkeypatch.setattr(ops, "require_gpu", lambda *ts: None)
    return resample, calls


def test_resample_dispatch_extents_and_steps(host_resample):
    from scipy import ndimage
    resample, calls = host_resample
    shape = (6, 11, 13)
    x = (detdata.normal("sp.cpu.api", (2,) + shape) * 100.0).astype(np.float32)
    xt = torch.from_numpy(x)
    zoom = (1.37, 0.7, 1.21)
    for order in (0, 1, 3):
        got = resample.zoom(xt, zoom, order).numpy()
        kind, o, m, t, out = calls[-1]
        assert kind == ("spline" if order == 3 else "affine") and o == order
        assert out == [int(round(n * z)) for n, z in zip(shape, zoom)] and t == [0.0, 0.0, 0.0]
        assert [m[i][i] for i in range(3)] == [(n - 1.0) / (s - 1.0) for n, s in zip(shape, out)]
        ref = ndimage.zoom(x, [1.0] + list(zoom), order=order)
        assert got.shape == ref.shape and int((got != ref).sum()) == 0, order
    assert resample.zoom(xt, 2, 3).shape == (2, 12, 22, 26) and calls[-1][0] == "spline"          # scalar factor, default order
    assert resample.zoom(xt, (1.0, 1.0, 1.0 / 13)).shape == (2, 6, 11, 1) and calls[-1][2][2][2] == 1.0       # out == 1: step 1.0
    got = resample.rotate(xt, 90.0, (-1, -2)).numpy()
    assert calls[-1][0] == "spline" and calls[-1][4] == list(shape)
    ref = ndimage.rotate(x, 90.0, (-1, -2), reshape=False, order=3)
    assert int((got != ref).sum()) <= 1
    resample.rotate(xt, 17.0, (-1, -3), 1)
    assert calls[-1][0] == "affine" and calls[-1][1] == 1
    resample.affine(xt, np.eye(3), (0.5, 0, 0), (3, 4, 5), 0)
    assert calls[-1] == ("affine", 0, np.eye(3).tolist(), [0.5, 0, 0], [3, 4, 5])


def test_resample_to_spacing_permutes_as_the_reference_does(host_resample):
    from scipy import ndimage
    resample, calls = host_resample
    assert resample.spacing_zoom((0.5, 0.8, 1.5), (1, 1, 1)) == [1.5, 0.5, 0.8]
    assert resample.spacing_zoom((0.4, 0.4, 1.5), (0.8, 0.8, 1.5)) == [1.0, 0.5, 0.5]
    x = (detdata.normal("sp.cpu.spacing", (1, 6, 20, 15)) * 100.0).astype(np.float32)
    got, spacing = resample.resample_to_spacing(torch.from_numpy(x), (0.5, 0.8, 1.5), [1, 1, 1], 3)
    assert spacing == (1.0, 1.0, 1.0) and tuple(got.shape) == (1, 9, 10, 12)
    ref = ndimage.zoom(x[0], [1.5, 0.5, 0.8], order=3)
    assert int((got.numpy()[0] != ref).sum()) == 0
    with pytest.raises(ValueError):
        resample.spacing_zoom((1, 1), (1, 1, 1))


def lab_like(x):
    return torch.zeros(tuple(x.shape), dtype=torch.uint8)


def test_resample_argument_checks(host_resample):
    resample, calls = host_resample
    x = torch.zeros((1, 4, 5, 6))
    for order in (2, 4, 5, -1, 1.5, True, "3"):
        with pytest.raises(ValueError, match="built: 0, 1, 3"):
            resample.zoom(x, 1.5, order)
    for order in (None, [3], np.float32(2.0)):
        with pytest.raises(ValueError, match="built: 0, 1, 3"):
            resample.zoom(x, 1.5, order)
    assert resample.ORDERS == (0, 1, 3)
    for factor in (np.float32(1.5), np.float64(1.5), np.int64(2), 2):                 # numpy scalars are single factors too
        assert tuple(resample.zoom(lab_like(x), factor, np.int64(0)).shape) == (1,) + tuple(int(round(n * float(factor))) for n in (4, 5, 6))
    with pytest.raises(ValueError, match=r"\[C,D,H,W\]"):
        resample.zoom(x[0], 1.5)
    with pytest.raises(ValueError, match=r"\[C,D,H,W\]"):
        resample.affine(np.zeros((1, 4, 5, 6), np.float32), np.eye(3), (0, 0, 0), (4, 5, 6))
    with pytest.raises(ValueError, match="one per axis"):
        resample.zoom(x, (1.5, 1.5))
    lab = torch.zeros((1, 4, 5, 6), dtype=torch.uint8)
    for order in (1, 3):
        with pytest.raises(ValueError, match="uint8"):
            resample.zoom(lab, 1.5, order)
    assert resample.zoom(lab, 1.5, 0).dtype == torch.uint8
    assert all(c[0] == "affine" and c[1] == 0 for c in calls)              # nothing refused reached a kernel


def test_resample_refuses_host_tensors():
    from fplx import resample
    for order in (0, 1, 3):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            resample.zoom(torch.zeros((1, 4, 5, 6)), 1.5, order)


# ---- fplx.preprocess: the boxes of data/preprocess_vs.py, restated literally

def _ref_source_crop(img, lab, spacing):
    D, H, W = img.shape
    d0 = int(D - 153 / spacing[2])
    d1 = int(D - 93 / spacing[2])
    h0, h1 = 190, 350
    w0, w1 = 120, 392
    img_sub = img[d0:d1, h0:h1, w0:w1]
    lab_sub = lab[d0:d1, h0:h1, w0:w1]
    assert lab_sub.sum() == lab.sum()
    return img_sub, lab_sub


def _ref_target_box(shape, spacing):
    D, H, W = shape
    if D < 50:
        d0, d1 = 5, D - 5
    elif spacing[2] == 1.0:
        d0, d1 = 8, 48
    elif spacing[2] == 1.5:
        d0, d1 = 8, 48
    else:
        raise ValueError("undefined case")
    h0, h1 = 120, 376
    w0, w1 = 120, 376
    h0, h1 = int(h0 * H / 512), int(h1 * H / 512)
    w0, w1 = int(w0 * W / 512), int(w1 * W / 512)
    return d0, d1, h0, h1, w0, w1


def test_vs_target_boxes():
    from fplx import preprocess as P
    cases = [((14, 96, 96), 1.5), ((49, 512, 512), 1.2), ((60, 512, 512), 1.0), ((80, 448, 448), 1.5), ((120, 384, 320), 1.0),
             ((50, 100, 300), 1.5), ((20, 511, 513), 1.0)]
    for shape, sz in cases:
        assert P.vs_target_box(shape, (0.41, 0.41, sz)) == _ref_target_box(shape, (0.41, 0.41, sz)), (shape, sz)
    assert P.vs_target_box((14, 96, 96), (0.4, 0.4, 1.5)) == (5, 9, 22, 70, 22, 70)
    assert P.vs_target_box((60, 512, 512), (0.4, 0.4, 1.0)) == (8, 48, 120, 376, 120, 376)
    for shape, sz in (((60, 512, 512), 1.2), ((50, 96, 96), 0.999)):
        with pytest.raises(ValueError, match="undefined case"):
            P.vs_target_box(shape, (0.4, 0.4, sz))


def test_vs_source_crop_equals_the_literal_restatement():
    from fplx import preprocess as P
    rs = np.random.RandomState(3)
    for D, sz in ((120, 1.5), (160, 1.0), (140, 1.2)):
        img = rs.randn(D, 360, 400).astype(np.float32)
        lab = np.zeros((D, 360, 400), np.uint8)
        d0, d1 = P.vs_source_box(img.shape, (0.4, 0.4, sz))[:2]
        assert (d0, d1) == (int(D - 153 / sz), int(D - 93 / sz)) and 0 <= d0 < d1 <= D
        lab[d0 + 1:d1 - 1, 200:340, 130:390] = 1
        got, want = P.vs_source_crop(img, lab, (0.4, 0.4, sz)), _ref_source_crop(img, lab, (0.4, 0.4, sz))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert got[0].shape == (d1 - d0, 160, 272)
        lab[d1, 200, 130] = 1                                                # one voxel below the box
        with pytest.raises(AssertionError):
            P.vs_source_crop(img, lab, (0.4, 0.4, sz))


def test_source_crop_refuses_an_image_that_would_be_its_own_label(tmp_path):
    from fplx import preprocess as P
    (tmp_path / "in").mkdir()
    (tmp_path / "in" / "vs_005_t1.nii").write_bytes(b"")              # no "ceT1" in the name: replace() would change nothing
    with pytest.raises(ValueError, match="own label"):
        P.source_image_crop(str(tmp_path / "in"), str(tmp_path))


def test_command_line_parser():
    from fplx import preprocess as P
    p = P.build_parser()
    a = p.parse_args(["transform", "t.cfg", "in.nii.gz", "out.nii.gz"])
    assert (a.command, a.cfg, a.img_in, a.img_out, a.lab_in, a.lab_out) == ("transform", "t.cfg", "in.nii.gz", "out.nii.gz",
                                                                            None, None)
    a = p.parse_args(["transform", "t.cfg", "i", "o", "li", "lo"])
    assert (a.lab_in, a.lab_out) == ("li", "lo")
    a = p.parse_args(["vs-source", "a", "b"])
    assert (a.command, a.in_dir, a.out_dir) == ("vs-source", "a", "b")
    a = p.parse_args(["vs-target", "a", "b"])
    assert (a.command, a.in_dir, a.out_dir) == ("vs-target", "a", "b")
    for bad in ([], ["vs-source", "a"], ["transform", "t.cfg", "i"], ["vs-other", "a", "b"], ["vs-target", "a", "b", "c"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    with pytest.raises(SystemExit):
        P.main(["transform", "t.cfg", "i", "o", "li"])                      # a label input without its output


def test_transform_list_from_cfg(tmp_path):
    from fplx import preprocess as P
    from fplx import transform as T
    cfg = tmp_path / "t.cfg"
    cfg.write_text("[dataset]\ntransform = [NormalizeWithMeanStd, CenterCrop]\nnormalizewithmeanstd_channels = [0]\n"
                   "centercrop_output_size = [4, 8, 8]\n")
    ts = P.get_transform_list(str(cfg))
    assert [type(t) for t in ts] == [T.NormalizeWithMeanStd, T.TransformDict["CenterCrop"]]
    cfg.write_text("[dataset]\ntransform = [NoSuchTransform]\n")
    with pytest.raises(ValueError, match="Undefined transform NoSuchTransform"):
        P.get_transform_list(str(cfg))
