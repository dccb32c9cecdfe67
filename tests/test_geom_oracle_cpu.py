"""The references of tests/geomoracle.py, proved on the CPU on exactly the data of tests/test_gpu_geom_exact.py:
max-pooling - float64 max_pool3d and its autograd equal the written-out first-maximum-wins pooling bit for bit, and dx is exact
in bf16; upsampling - the written-out interpolation equals float64 F.interpolate, float32 CPU torch lies inside the derived
bound (the largest error / bound is printed per case) and every mutant lands at least 10 x outside it; sliding window - the
numpy loops equal Inferer._run_generic on the CPU bit for bit, and merging the extracted patches returns the image."""
import numpy as np
import pytest
import torch

import geomoracle as O
from convoracle import bf16_rne

_RATIOS = {}


# ---------------------------------------------------------------- max-pooling

@pytest.mark.parametrize("case", O.POOL_CASES, ids=O.pool_id)
def test_pool_reference_is_first_maximum_wins_and_exact(case):
    d = O.pool_data(case)
    y, grad = O.pool_ref_numpy(d["x"], d["dy"], case["pd"])
    for got, want in ((d["y"], y), (d["grad"], grad)):
        assert np.array_equal(got.view(np.int64), want.view(np.int64))                 # bits: -0 is not +0
    dx = O.pool_dx(case, d)
    assert np.abs(dx).max() <= 16 and np.array_equal(dx, np.round(dx))
    for a in (d["x"], d["y"], dx):
        fin = np.where(np.isfinite(a), a, 0.0)
        assert np.array_equal(bf16_rne(fin).numpy(), fin)                               # nothing rounds, in either type
    if case["kind"] == "equal":
        g = grad.reshape(grad.shape[:2] + (-1, case["pd"], grad.shape[3] // 2, 2, grad.shape[4] // 2, 2))
        assert not g[:, :, :, 1:].any() and not g[..., 1, :, :].any() and not g[..., 1].any()   # window position 0 only
    if case["kind"] == "special":
        assert np.isneginf(y).any() and np.isposinf(y).any() and (np.signbit(y) & (y == 0)).any() and (~np.signbit(y) & (y == 0)).any()


def test_pool_grid_cases_exceed_the_grid_cap():
    for case in O.POOL_GRID_CASES:
        assert O.pool_items(case) > O.EW_GRID_CAP * O.EW_THREADS, O.pool_id(case)
        assert O.pool_items(case) < 1.2 * O.EW_GRID_CAP * O.EW_THREADS
    for case in O.POOL_CASES:
        assert O.pool_items(case) <= O.EW_GRID_CAP * O.EW_THREADS


# ---------------------------------------------------------------- upsampling

def _up_sides(case):
    which = case.get("which", "both")
    return [s for s in ("fwd", "bwd") if which in ("both", s)]


@pytest.mark.parametrize("case", O.UP_CASES, ids=O.up_id)
def test_upsample_bound_holds_float32_torch_and_rejects_the_mutants(case):
    sd, bf16 = case["sd"], case["dt"] == "bf16"
    d = O.up_data(case)
    x, dy = d.get("x"), d.get("dy")
    y64, dx64 = O.up_torch(x, dy, sd)
    y32, dx32 = O.up_torch(x, dy, sd, torch.float32)
    res = {}
    if x is not None:
        own = O.up_forward_own(x, sd)
        # axis_table describes the reference (whose own float64 coordinate carries two roundings of 2^-53 (in - 1))
        assert np.abs(own - y64).max() <= 2.0 ** -50 * max(case["dhw"]) * max(1.0, np.abs(x).max())
        bound = O.up_fwd_bound(x, y64, sd, bf16)
        got = bf16_rne(y32).numpy() if bf16 else y32
        res["fwd"] = O.ratio(got, y64, bound)
        assert res["fwd"] <= 1.0, res
        if bf16 and got.size >= 1000:
            res["fwd.bias"] = O.check_bf16_bias(got, y64, "fwd")
        for m in O.FWD_MUTANTS:
            mut = O.up_mutant_fwd(m, x, sd)
            if np.array_equal(mut, y64):
                continue
            if not np.isnan(mut).any():
                assert np.abs(mut - y64).max() > 1e-9, m                                # differs in exact arithmetic, not by float64 noise
            res["fwd." + m] = O.ratio(mut, y64, bound)
            assert res["fwd." + m] >= O.SEPARATION, (m, res)
    if dy is not None:
        own = O.up_backward_own(dy, sd)
        assert np.abs(own - dx64).max() <= 2.0 ** -50 * max(case["dhw"]) * max(1.0, np.abs(dx64).max())
        bound = O.up_bwd_bound(dy, dx64, sd, bf16)
        got = bf16_rne(dx32).numpy() if bf16 else dx32
        res["bwd"] = O.ratio(got, dx64, bound)
        assert res["bwd"] <= 1.0, res
        if bf16 and got.size >= 1000:
            res["bwd.bias"] = O.check_bf16_bias(got, dx64, "bwd")
        for m in O.BWD_MUTANTS:
            mut = O.up_mutant_bwd(m, dy, sd)
            if np.abs(mut - dx64).max() <= 1e-9:
                continue
            res["bwd." + m] = O.ratio(mut, dx64, bound)
            assert res["bwd." + m] >= O.SEPARATION, (m, res)
    if max(case["dhw"]) > 1:
        for side in _up_sides(case):                                                    # every mutant of the side is visible here
            names = O.FWD_MUTANTS if side == "fwd" else O.BWD_MUTANTS
            assert all(side + "." + m in res for m in names), res
    _RATIOS[O.up_id(case)] = res
    print("%-44s %s" % (O.up_id(case), "  ".join("%s %.3g" % kv for kv in sorted(res.items()))))


def test_upsample_grid_cases_exceed_the_grid_cap():
    big = [c for c in O.UP_CASES if c["which"] != "both"]
    assert sorted(c["which"] for c in big) == ["bwd", "fwd"]
    for c in big:
        assert O.UP_GRID_CAP * O.UP_THREADS < O.up_items(c, c["which"]) < 1.01 * O.UP_GRID_CAP * O.UP_THREADS
    for c in O.UP_CASES:
        if c["which"] == "both":
            assert max(O.up_items(c, "fwd"), O.up_items(c, "bwd")) <= O.UP_GRID_CAP * O.UP_THREADS


@pytest.mark.parametrize("case", O.UP_EXACT_CASES, ids=O.up_id)
def test_upsample_exact_family_is_replication_and_a_sum(case):
    d = O.up_exact_data(case)
    y, dx = O.up_exact_ref(case, d)
    for dtype in (torch.float64, torch.float32):
        yt, dxt = O.up_torch(d["x"], d["dy"], case["sd"], dtype)
        assert np.array_equal(yt, y) and np.array_equal(dxt, dx)
    assert np.abs(dx).max() <= 32 and np.array_equal(bf16_rne(dx).numpy(), dx)


def test_a_narrow_backward_window_fails_the_transpose_check():
    """the GPU file's transpose check on the oracle itself: exact weights pass with error 0, a window one output short does not"""
    for n, dhw, sd in O.UP_TRANSPOSE_CASES:
        dy = O.ints("upt.%dx%dx%d.%d" % (dhw + (sd,)), (n, 3, dhw[0] * sd, 2 * dhw[1], 2 * dhw[2]), -4, 4)
        weights = {}
        for L in O.UP_TRANSPOSE_LENGTHS:
            i0, i1, l0, l1, _ = O.axis_table(L, 2 * L)
            w = np.zeros((2 * L, L))
            np.add.at(w, (np.arange(2 * L), i0), l0)
            np.add.at(w, (np.arange(2 * L), i1), l1)
            weights[L] = w
        dx, S, nterm = O.kron_transpose(dy, sd, weights)
        bound = O.gamma(3 + nterm) * S
        assert O.ratio(O.up_backward_own(dy, sd), dx, np.maximum(bound, 1e-12)) <= 1.0
        assert O.ratio(O.up_backward_own(dy, sd, mutant="window_too_narrow"), dx, bound) >= O.SEPARATION
        assert O.ratio(O.up_backward_own(dy, sd, mutant="skips_last_output"), dx, bound) >= O.SEPARATION


# ---------------------------------------------------------------- sliding window

def test_axis_starts_keep_the_duplicates():
    from fplx.infer import _axis_starts, _FLIPS_TTA
    assert O.axis_starts(32, 16, 8) == [0, 8, 16, 16] and O.axis_starts(20, 16, 4) == [0, 4, 4, 4, 4]
    assert O.axis_starts(64, 1, 1) == list(range(64))
    for size, window, stride in ((32, 16, 8), (20, 16, 4), (12, 8, 3), (7, 4, 3), (9, 4, 2), (64, 1, 1), (8, 8, 8)):
        assert O.axis_starts(size, window, stride) == _axis_starts(size, window, stride)
    assert tuple(_FLIPS_TTA) == O.FLIPS_TTA


@pytest.mark.parametrize("case", O.SW_CASES, ids=O.sw_id)
def test_merging_the_extracted_patches_returns_the_image(case):
    name, tta = case
    dhw, window, stride = O.SW_PLANS[name]
    window, starts = O.sw_starts(dhw, window, stride)
    img = O.sw_image(name, 2, 3, dhw, "int")
    p = O.sw_extract_ref(img, starts, window, O.sw_flips(tta))
    back = O.sw_merge_ref(p, dhw, starts, window, O.sw_flips(tta))
    assert back.dtype == np.float32 and np.array_equal(back.view(np.int32), img.view(np.int32))


@pytest.mark.parametrize("kind", ["int", "real"])
@pytest.mark.parametrize("case", O.SW_CASES, ids=O.sw_id)
def test_numpy_loops_equal_the_generic_inferer_on_the_cpu(case, kind):
    import fplx
    name, tta = case
    dhw, window, stride = O.SW_PLANS[name]
    cfg = dict(sliding_window_enable=True, sliding_window_size=list(window), sliding_window_stride=list(stride), tta_mode=tta, class_num=3)
    img = O.sw_image(name + ".toy", 2, 1, dhw, kind)
    toy = O.Toy(3)
    got = fplx.Inferer(cfg).run(toy, torch.from_numpy(img), torch.zeros(2, dtype=torch.long)).numpy()
    want = O.toy_inferer_ref(img, cfg)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("name", sorted(O.INFERER_CASES))
def test_inferer_surface_cases_on_the_cpu(name):
    import fplx
    n, dhw, cfg, train = O.INFERER_CASES[name]
    img = O.sw_image("inferer." + name, n, 1, dhw, "int")
    toy = O.Toy(cfg["class_num"]).train(train)
    got = fplx.Inferer(cfg).run(toy, torch.from_numpy(img), torch.zeros(n, dtype=torch.long)).numpy()
    want = O.toy_inferer_ref(img, cfg)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    mc = fplx.Inferer(cfg).run_mc(toy, torch.from_numpy(img), torch.zeros(n, dtype=torch.long), 2).numpy()
    assert mc.shape == (2,) + want.shape and all(np.array_equal(m.view(np.int32), want.view(np.int32)) for m in mc)


def test_mc_layout_is_chunks_then_passes():
    per = np.arange(3 * 7, dtype=np.float32).reshape(3, 7, 1)               # value = pass * 7 + patch
    lay = O.sw_mc_layout(per, 3)[:, 0]
    assert lay.tolist() == [0, 1, 2, 7, 8, 9, 14, 15, 16, 3, 4, 5, 10, 11, 12, 17, 18, 19, 6, 13, 20]


def test_sliding_window_grid_cases_exceed_the_grid_cap():
    cap = O.SW_GRID_CAP * O.SW_THREADS
    b = O.SW_BIG_EXTRACT
    window, starts = O.sw_starts(b["dhw"], b["window"], b["stride"])
    tiles = len(O.sw_tiles(starts))
    assert len(O.sw_flips(b["tta"])) * tiles * b["n"] * b["c"] * int(np.prod(window)) > cap
    b = O.SW_BIG_MERGE
    _, starts = O.sw_starts(b["dhw"], b["window"], b["stride"])
    assert b["n"] * b["c"] * int(np.prod(b["dhw"])) > cap and len(O.sw_tiles(starts)) > 1
    b = O.SW_BIG_WHOLE
    assert b["n"] * b["c"] * int(np.prod(b["dhw"])) // 4 > cap and b["dhw"][2] % 4 == 0
    assert len(O.axis_starts(64, 1, 1)) == O.SW_MAX and len(O.axis_starts(65, 1, 1)) == O.SW_MAX + 1
