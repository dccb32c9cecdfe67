"""CPU self-tests of the convolution oracles (tests/convoracle.py): bf16 rounding against torch's own
conversion, a simulated correct kernel passes both oracles, and each of these injected defects fails them:

- a truncating bf16 conversion (round toward zero instead of to nearest even);
- one input channel missing from one interior tap on one face (outputs at w = 0, tap kw = 2, which reads w = 1 inside the
  volume);
- a halo that reads the first voxel of the next row instead of zero at w = W - 1;
- 16 voxels missing from the BatchNorm statistics;
- one 16-voxel row missing from the weight gradient dw;
- one statistics row left unwritten (its NaN sentinel survives).

The first three are real-valued cases for oracle B (exact integer data cannot see rounding), the last three fail oracle A.  For
the truncation and the statistics defect, the tolerance formulas the older kernel tests use (2e-2 x max|ref| on outputs;
2e-2 max|ref| sqrt(V) on the sum and rtol 8e-2 on the sum of squares of the statistics) are shown to ACCEPT them."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import convoracle as O

SHAPE = (1, 64, 32, 7, 24, 64)          # n, Cin, Cout, D, H, W
DROP = slice(0, 16)                     # the 16 voxels of the defects: the first w-row segment (d = 0, h = 0, w = 0..15)


def _stat_rows(y2d, rows):
    """fp32 partial rows [rows][2][C] over a partition of the voxels - the layout the convolution kernels write"""
    out = []
    for part in torch.tensor_split(y2d.float(), rows):
        out.append(torch.stack([part.sum(0), (part * part).sum(0)]))
    return torch.stack(out)


def _missing_channel(x, wt, y, ci=5):
    """outputs at w = 0 without input channel ci of tap (kd, kh, kw) = (1, 1, 2), which reads w = 1 (inside the volume)"""
    y = y.double().clone()
    y[..., 0] -= wt[:, ci, 1, 1, 2].double().view(1, -1, 1, 1) * x[:, ci:ci + 1, :, :, 1].double()
    return y


def _halo_next_row(x, wt, b):
    """at w = W - 1 the taps kw = 2 read x[.., h + 1, 0] (the next row's first voxel, zero past the last row) instead of zero"""
    nxt = torch.zeros_like(x[..., :1])
    nxt[..., :-1, :] = x[..., 1:, :1]
    return F.conv3d(torch.cat([x, nxt], -1), wt, b, padding=1)[..., :x.shape[-1]]


@pytest.fixture(scope="module")
def real_case():
    n, cin, cout, d, h, w = SHAPE
    x = O.real_operand("cpu.x", (n, cin, d, h, w))
    wt = O.real_operand("cpu.w", (cout, cin, 3, 3, 3), 0.2)
    b = O.real_operand("cpu.b", (cout,), 0.1)
    ref, S = O.conv3d_ref(x, wt, b, 1), O.conv3d_abs(x, wt, b, 1)
    y32 = F.conv3d(x, wt, b, padding=1)         # an fp32 accumulation in another order: a correct kernel before its rounding
    return x, wt, b, ref, S, y32, cin * 27 + 1


@pytest.fixture(scope="module")
def int_case():
    n, cin, cout, d, h, w = SHAPE
    p = O.density_for(n * d * h * w, cin * 27)
    x = O.int_operand("cpu.ix", (n, cin, d, h, w), p)
    wt = O.int_weight("cpu.iw", (cout, cin, 3, 3, 3))
    b = O.int_operand("cpu.ib", (cout,), 0.7, 3)
    dy = O.int_operand("cpu.idy", (n, cout, d, h, w), 0.5)
    O.assert_exact_pre(O.conv3d_abs(x, wt, b, 1), "y")
    ref = O.conv3d_ref(x, wt, b, 1)
    stats = O.stats_ref(O.cl(ref))
    dwr = O.wgrad_ref(x, dy, wt.shape, 1)
    return x, wt, b, dy, ref, stats, dwr


def test_bf16_rne_agrees_with_torch_including_ties():
    assert O.bf16_rne(torch.tensor([257.0, 259.0, -257.0, -259.0])).tolist() == [256.0, 260.0, -256.0, -260.0]
    halves = [s * np.ldexp(q, e) for e in (-30, -9, -1, 0, 1, 5, 9, 17, 40)
              for q in (128.5, 129.5, 130.5, 200.5, 254.5, 255.5) for s in (1.0, -1.0)]
    t = torch.tensor(halves, dtype=torch.float32)        # every halfway pattern is a float32 value
    assert torch.equal(O.bf16_rne(t), t.bfloat16().double())
    g = torch.Generator().manual_seed(0)
    r = torch.randn(200000, generator=g) * torch.exp(torch.randn(200000, generator=g) * 6)
    assert torch.equal(O.bf16_rne(r), r.bfloat16().double())
    assert O.bf16_trunc(torch.tensor([259.0, -259.0, 257.5])).tolist() == [258.0, -258.0, 256.0]
    assert O.ulp_bf16(torch.tensor([1.0, 1.5, 256.0, 300.0, -0.75])).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0, 2.0, 2.0 ** -8]


def test_rounding_oracle_passes_a_correct_result(real_case):
    x, wt, b, ref, S, y32, K = real_case
    ratio, bias = O.check_rounding(O.bf16_rne(y32), ref, S, K, "simulated round-to-nearest-even")
    assert ratio < 1.0 and abs(bias) < 0.05
    # an fp32 output (dw, logits) accumulated in fp32: within gamma S
    assert O.bound_ratio(y32, ref, S, K, bf16_out=False) <= 1.0


def test_rounding_oracle_fails_truncation_that_the_old_tolerance_accepts(real_case):
    x, wt, b, ref, S, y32, K = real_case
    yt = O.bf16_trunc(y32)
    assert float((yt - ref).abs().max()) < 2e-2 * float(ref.abs().max())        # the old bar lets it through
    assert O.bound_ratio(yt, ref, S, K) > 1.0
    assert O.rounding_bias(yt, ref) < -0.4
    with pytest.raises(AssertionError):
        O.check_rounding(yt, ref, S, K, "truncation")


def test_rounding_oracle_fails_a_missing_channel_and_a_halo_read(real_case):
    x, wt, b, ref, S, y32, K = real_case
    assert O.bound_ratio(O.bf16_rne(_missing_channel(x, wt, y32)), ref, S, K) > 10
    assert O.bound_ratio(O.bf16_rne(_halo_next_row(x, wt, b)), ref, S, K) > 10


def test_old_statistics_tolerance_accepts_16_missing_voxels(real_case):
    x, wt, b, ref, S, y32, K = real_case
    yc, yr = O.cl(y32).double(), O.cl(ref)
    keep = torch.ones(yc.shape[0], dtype=torch.bool)
    keep[DROP] = False
    scale = float(ref.abs().max())
    np.testing.assert_allclose(yc[keep].sum(0).numpy(), yr.sum(0).numpy(), atol=2e-2 * scale * yc.shape[0] ** 0.5 + 1e-3)
    np.testing.assert_allclose((yc[keep] ** 2).sum(0).numpy(), (yr * yr).sum(0).numpy(), rtol=8e-2)


def test_exact_oracle_passes_a_correct_result(int_case):
    x, wt, b, dy, ref, (s1, s2), dwr = int_case
    y32 = F.conv3d(x, wt, b, padding=1)
    O.assert_exact(O.bf16_rne(y32), O.bf16_rne(ref), "y")
    g1, g2 = O.stats_sum(_stat_rows(O.cl(y32), 37))
    O.assert_exact(g1, s1, "sum y")
    O.assert_exact(g2, s2, "sum y^2")
    O.assert_exact(torch.nn.grad.conv3d_weight(x, wt.shape, dy, padding=1), dwr, "dw")
    # the sparse scatter reference of the benchmark-size case agrees with the dense one
    O.assert_exact(O.conv3d_sparse_ref(x, wt, b), O.cl(ref), "sparse reference")


def test_exact_oracle_fails_each_defect(int_case):
    x, wt, b, dy, ref, (s1, s2), dwr = int_case
    y32 = F.conv3d(x, wt, b, padding=1)
    want = O.bf16_rne(ref)
    assert O.exact_mismatches(O.bf16_rne(_missing_channel(x, wt, y32)), want) > 0
    assert O.exact_mismatches(O.bf16_rne(_halo_next_row(x, wt, b)), want) > 0
    # 16 voxels missing from the statistics
    yc = O.cl(y32)
    keep = torch.ones(yc.shape[0], dtype=torch.bool)
    keep[DROP] = False
    g1, g2 = O.stats_sum(_stat_rows(yc[keep], 37))
    assert O.exact_mismatches(g1, s1) + O.exact_mismatches(g2, s2) > 0
    # one 16-voxel row of dy never read by the weight gradient
    dyd = dy.clone()
    dyd[0, :, 3, 5, 16:32] = 0
    assert float(dy[0, :, 3, 5, 16:32].abs().sum()) > 0
    assert O.exact_mismatches(torch.nn.grad.conv3d_weight(x, wt.shape, dyd, padding=1), dwr) > 0
    # one statistics row left unwritten: the NaN the buffer was filled with survives into the host sum
    rows = _stat_rows(yc, 37)
    rows[11] = float("nan")
    g1, g2 = O.stats_sum(rows)
    assert O.exact_mismatches(g1, s1) == yc.shape[1] and O.exact_mismatches(g2, s2) == yc.shape[1]


def test_precondition_is_enforced():
    with pytest.raises(AssertionError):
        O.assert_exact_pre(torch.tensor([float(1 << 24)]), "y")
    with pytest.raises(AssertionError):
        O.stats_ref(torch.full((5000, 2), 64.0))            # sum y^2 = 2^24 * 20 / 16 > 2^24
