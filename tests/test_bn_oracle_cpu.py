"""CPU self-tests of the BatchNorm oracles (tests/bnoracle.py): the fp32 numpy restatement of every kernel of
the family (same rounding points; partial rows dealt by the kernels' own rule, any rows x lanes partition) passes the exact oracle A
bit for bit and the rounding oracle B with ratio <= 1, the closed forms equal float64 autograd, `exact_pre` refuses data that is
not exact, the host-side mirrors agree with the library, and each of these injected defects is rejected by A or B at shapes the
GPU test uses (tests/test_gpu_bn_exact.py):

wrong voxels       drop_last (last voxel of a stride dropped), twice (one voxel counted twice), skip_tail (tail loop skipped)
PReLU / dropout / pooling   ge_zero (z >= 0 for z > 0), no_inv_keep_bwd, mask_ld (mask index built with ld), last_max,
                   col_tie_larger (tie between the two columns of the col kernels resolved to the larger index)
backward           dslope_kept_out (slope sum takes dropped elements), xh_scale (scale where rstd belongs), k1_sign,
                   coef_train0 (coef not zeroed with train = 0), swap_dgamma_dbeta
statistics         biased_rv, momentum_side, count1_guard (n / (n - 1) at n = 1), nbt_stuck, eval_eps_outside (1 / sqrt(rv) + eps)
pool rounding      a2_cmp_unrounded (a2 compared before its bf16 rounding), dv_unrounded (dv summed before its bf16 rounding)

None is excluded.  ge_zero is visible to A only (bnoracle's docstring)."""
import numpy as np
import pytest

import bnoracle as O

SEED, SID = 77, 5
SITES = [(True, 32, 257, 0.5), (True, 8, 4097, 0.75), (True, 24, 255, 0.5), (True, 5, 63, 0.75), (True, 512, 500, 0.0),
         (False, 12, 257, 0.5), (False, 5, 63, 0.0), (True, 8, 1, 0.5)]
POOLS = [((1, 2, 4, 6), 32, 2, 1), ((2, 3, 6, 8), 16, 1, 1), ((1, 4, 4, 4), 64, 2, 0), ((1, 2, 2, 2), 512, 2, 1)]


def _site(bf16, c, v, p, exact, tag=""):
    gm = O.reduce_geom(v, c, O.vec_of(bf16, c))
    if exact:
        k, coef = O.exact_consts("cpu.k%d%s" % (c, tag), c)
        y, d = O.exact_acts("cpu.a%d.%d%s" % (c, v, tag), v, c)
    else:
        p = 0.3 if p == 0.75 else p
        y, d = O.real_acts("cpu.r%d.%d%s" % (c, v, tag), v, c, bf16)
        k, coef = O.real_consts("cpu.rk", y)
    return y, d, k, coef, p, gm


@pytest.mark.parametrize("bf16,c,v,p", SITES)
def test_site_restatement_passes_A_and_B(bf16, c, v, p):
    for exact in (True, False):
        y, d, k, coef, q, gm = _site(bf16, c, v, p, exact)
        got = O.restate_site(y, d, k, coef, q, SEED, SID, bf16, gm)
        res = O.check_site(got, y, d, k, coef, q, SEED, SID, bf16, gm, exact, use_autograd=True)
        print("%s bf16=%d c=%d v=%d p=%g: %s" % ("A" if exact else "B", bf16, c, v, q, res))
        got0 = O.restate_site(y, d, k, coef, q, SEED, SID, bf16, gm, train=0)
        O.check_site(got0, y, d, k, coef, q, SEED, SID, bf16, gm, exact, train=0)


def test_any_partition_into_rows_passes():
    """the oracle does not depend on how the voxels are dealt: other rows x lanes partitions pass A bit for bit as well"""
    y, d, k, coef, p, gm = _site(True, 32, 257, 0.5, True)
    for rows, lanes in ((1, 1), (3, 7), (64, 2)):
        g2 = dict(gm, idx=O.deal(np.arange(257)[:, None], rows, lanes), rows=rows, lanes=lanes, pow2=False)
        O.check_site(O.restate_site(y, d, k, coef, p, SEED, SID, True, g2), y, d, k, coef, p, SEED, SID, True, g2, True)


def _pool(dims, c, pd, col, exact):
    n, d, h, w = dims
    v, vo = n * d * h * w, n * (d // pd) * (h // 2) * (w // 2)
    gm = O.pool_geom(dims, c, pd, col)
    if exact:
        k, _ = O.exact_consts("cpu.pk%d" % c, c, fine=False)          # coarse z: the slope sum's terms are dv z
        y, _ = O.exact_acts("cpu.pa%d.%d" % (c, v), v, c, fine=False)
        dskip, g = O.exact_pool_grads("cpu.pg%d" % c, v, vo, c)
    else:
        y, dskip = O.real_acts("cpu.pr%d.%d" % (c, v), v, c, True)
        k, _ = O.real_consts("cpu.prk", y)
        g = O.real_acts("cpu.prg", vo, c, True)[1]
    return y, g, dskip, k, gm


@pytest.mark.parametrize("dims,c,pd,col", POOLS)
def test_pool_restatement_passes_A_and_B(dims, c, pd, col):
    for exact in (True, False):
        y, g, dskip, k, gm = _pool(dims, c, pd, col, exact)
        for ds in (dskip, None):
            res = O.check_pool(O.restate_pool(y, g, ds, k, gm), y, g, ds, k, gm, exact, use_autograd=ds is not None)
        print("%s pool %s c=%d pd=%d col=%d: %s" % ("A" if exact else "B", dims, c, pd, gm["col"], res))


def _finalize_case(c=8, count=64, rows=5):
    stats, gamma, beta, rm, rv = O.dyadic_rows("cpu.fin", c, count, rows)
    return stats, count, gamma, beta, rm, rv


def test_train_finalize_restatement_passes_A_and_B():
    stats, count, gamma, beta, rm, rv = _finalize_case()
    r = O.train_finalize(stats, count, gamma, beta, rm, rv, 3, 0.25, 1e-5)
    assert r["var_raw"][1] < 0 and r["var"][1] == 0 and r["var"][2] == 0
    for mom, exact in ((0.25, True), (0.1, False)):
        got = O.restate_train_finalize(stats, count, gamma, beta, rm, rv, 3, mom, 1e-5)
        print(O.check_train_finalize(got, stats, count, gamma, beta, rm, rv, 3, mom, 1e-5, exact))
        got = O.restate_train_finalize(stats, count, gamma, beta, None, None, None, mom, 1e-5)
        O.check_train_finalize(got, stats, count, gamma, beta, None, None, None, mom, 1e-5, exact)


@pytest.mark.parametrize("bf16", [True, False])
@pytest.mark.parametrize("ratio", [0.0, 8.0, 64.0])
def test_statistics_path_restatement(bf16, ratio):
    """channel_stats -> bn_train_finalize in fp32 against the float64 statistics of the data, with a constant channel"""
    v, c = 4097, 96
    y, _ = O.real_acts("cpu.st%g" % ratio, v, c, bf16, ratio)
    y[:, 3] = np.float32(3.0)
    gm = O.stats_geom(v)
    part = O.channel_stats(y, gm, np.float32)
    O.check_stats(part, y, gm, False)
    g = O.rng("cpu.stg")
    gamma, beta = (0.5 + g.random(c)).astype(np.float32), g.standard_normal(c).astype(np.float32)
    got = O.restate_train_finalize(part, v, gamma, beta, None, None, None, 0.1, 1e-5)
    m, var, dm, dvar, amp = O.stats_path_bounds(y, gm)
    res = O.check_train_finalize(got, part, v, gamma, beta, None, None, None, 0.1, 1e-5, False, data_bounds=(m, var, dm, dvar))
    print("mean/sigma %g bf16=%d: amplification %.4g, %s" % (ratio, bf16, np.median(amp[np.isfinite(amp)]), res))
    ye, _ = O.exact_acts("cpu.ste", v, c)
    O.check_stats(O.channel_stats(ye, gm, np.float32), ye, gm, True)


def test_eval_prepare_restatement():
    g = O.rng("cpu.ev")
    c = 40
    gamma, beta, rm = g.integers(-8, 9, c) / 8.0, g.integers(-8, 9, c) / 8.0, g.integers(-8, 9, c) / 4.0
    rv = 4.0 ** g.integers(-2, 3, c)
    sc, sh = O.eval_prepare(gamma, beta, rm, rv, 0.0, np.float32)
    O.check_eval_prepare(sc, sh, gamma, beta, rm, rv, 0.0, True)
    rv = 0.1 + g.random(c)
    sc, sh = O.eval_prepare(gamma, beta, rm, rv.astype(np.float32), 1e-5, np.float32)
    O.check_eval_prepare(sc, sh, gamma, beta, rm, rv.astype(np.float32), 1e-5, False)


def _rejected(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("mut", O.MUTATIONS)
def test_mutation_is_rejected(mut):
    """the unmutated restatement passes the very check that rejects the mutated one"""
    hits = []
    if mut in ("drop_last", "twice", "skip_tail", "ge_zero", "no_inv_keep_bwd", "mask_ld", "dslope_kept_out", "xh_scale", "k1_sign",
               "coef_train0", "swap_dgamma_dbeta"):
        train = 0 if mut == "coef_train0" else 1
        for exact in (True, False):
            for (bf16, c, v, p) in ((True, 32, 257, 0.5), (True, 24, 255, 0.5), (True, 512, 500, 0.5)):    # the last: 4 trips per lane, ragged end
                y, d, k, coef, q, gm = _site(bf16, c, v, p, exact, "m")
                gmm = O.reduce_geom(v, c, O.vec_of(bf16, c), mut)
                O.check_site(O.restate_site(y, d, k, coef, q, SEED, SID, bf16, gm, train, None, 2 * c), y, d, k, coef, q, SEED, SID, bf16, gm, exact, train)
                if _rejected(lambda: O.check_site(O.restate_site(y, d, k, coef, q, SEED, SID, bf16, gmm, train, mut, 2 * c), y, d, k, coef, q,
                                                  SEED, SID, bf16, gm, exact, train)):
                    hits.append("%s c=%d" % ("A" if exact else "B", c))
    elif mut in ("last_max", "col_tie_larger", "a2_cmp_unrounded", "dv_unrounded"):
        for exact in (True, False):
            for (dims, c, pd, col) in (((1, 2, 4, 6), 32, 2, 1), ((2, 3, 6, 8), 16, 1, 1), ((1, 8, 16, 16), 8, 2, 1)):
                y, g, dskip, k, gm = _pool(dims, c, pd, col, exact)
                O.check_pool(O.restate_pool(y, g, dskip, k, gm), y, g, dskip, k, gm, exact)
                if _rejected(lambda: O.check_pool(O.restate_pool(y, g, dskip, k, gm, mut), y, g, dskip, k, gm, exact)):
                    hits.append("%s %s" % ("A" if exact else "B", dims))
    elif mut == "eval_eps_outside":
        g = O.rng("cpu.mev")
        gamma, beta, rm, rv = 0.5 + g.random(9), g.standard_normal(9), g.standard_normal(9), (0.1 + g.random(9)).astype(np.float32)
        sc, sh = O.eval_prepare(gamma.astype(np.float32), beta.astype(np.float32), rm.astype(np.float32), rv, 1e-5, np.float32, mut)
        if _rejected(lambda: O.check_eval_prepare(sc, sh, gamma.astype(np.float32), beta.astype(np.float32), rm.astype(np.float32), rv, 1e-5, False)):
            hits.append("B")
    else:
        stats, count, gamma, beta, rm, rv = _finalize_case()
        if mut == "count1_guard":                          # one voxel: the row IS the voxel, var = 0
            count, stats = 1, np.stack([np.full((1, 8), 1.5, np.float32), np.full((1, 8), 2.25, np.float32)], 1)
        O.check_train_finalize(O.restate_train_finalize(stats, count, gamma, beta, rm, rv, 3, 0.25, 1e-5), stats, count, gamma, beta, rm, rv, 3,
                               0.25, 1e-5, True)
        if _rejected(lambda: O.check_train_finalize(O.restate_train_finalize(stats, count, gamma, beta, rm, rv, 3, 0.25, 1e-5, mut), stats, count,
                                                    gamma, beta, rm, rv, 3, 0.25, 1e-5, True)):
            hits.append("A")
    print("mutation %s rejected by: %s" % (mut, ", ".join(hits)))
    assert hits, "mutation %s passes both oracles" % mut


@pytest.mark.parametrize("p", [0.0, 0.3])
def test_closed_forms_equal_autograd(p):
    """`autograd_check` asserts 1e-11 of the magnitude on out, dgamma, dbeta, dslope, dx - site and both pool depths; a wrong
    closed form is reported (the k1 sign)"""
    y, d = O.real_acts("cpu.ag", 700, 12, True)
    g = O.rng("cpu.agp")
    gamma, beta = 0.5 + g.random(12), g.standard_normal(12)
    gamma[3] = -gamma[3]
    assert O.autograd_check(y, d, gamma, beta, 0.25, p, SEED, SID)
    for pd, dims in ((2, (1, 4, 6, 10)), (1, (2, 3, 6, 10))):
        n = int(np.prod(dims))
        yy, ds = O.real_acts("cpu.agpool%d" % pd, n, 16, True)
        gg = O.real_acts("cpu.agg", n // (4 * pd), 16, True)[1]
        assert O.autograd_check(yy, None, 0.5 + g.random(16), g.standard_normal(16), 0.25, 0.0, 0, 0, pool=(dims, pd, gg, ds))
    orig = O.apply_dy
    try:
        O.apply_dy = lambda e, k, coef, dt=np.float64, mut=None: orig(e, k, coef, dt, "k1_sign")
        with pytest.raises(AssertionError):
            O.autograd_check(y, d, gamma, beta, 0.25, p, SEED, SID)
    finally:
        O.apply_dy = orig


def test_exact_pre_refuses_data_that_is_not_exact():
    c, v = 32, 257
    gm = O.reduce_geom(v, c, 8)
    k, coef = O.exact_consts("cpu.pre", c)
    y, d = O.exact_acts("cpu.prea", v, c)
    assert 0 < O.exact_pre(y, d, k, coef, 0.5, True, gm) < O.EXACT_LIMIT
    with pytest.raises(AssertionError):                    # thirds are not dyadic
        O.exact_pre(y, d, dict(k, mean=k["mean"] + np.float32(1.0 / 3.0)), coef, 0.5, True, gm)
    with pytest.raises(AssertionError):                    # not a bf16 value
        O.exact_pre(y + np.float32(2.0 ** -12), d, k, coef, 0.5, True, gm)
    with pytest.raises(AssertionError):                    # p = 0.3: 1 / (1 - p) is no power of two
        O.exact_pre(y, d, k, coef, 0.3, True, gm)
    # over-large data: one row for everything and large magnitudes - the chain of the slope sum passes 2^24 units
    big = dict(gm, idx=O.deal(np.arange(v)[:, None], 1, 1), rows=1, lanes=1)
    with pytest.raises(AssertionError, match="2\\^24"):
        O.exact_pre(y * np.float32(64), d * np.float32(64), k, coef, 0.5, True, big)
    with pytest.raises(AssertionError):
        O.check_stats(O.channel_stats(y * np.float32(1024), dict(big, vec=1), np.float32), y * np.float32(1024), dict(big, vec=1), True)


def test_mirrors_of_the_host_code():
    """fplx_num_partials from the library itself (a host function), the grid and the loop plans"""
    from fplx import _lib
    lib = _lib.lib()
    for v in (1, 16, 17, 63, 255, 257, 500, 4095, 4097, 32768, 32769, 65573, 98341, 4096000):
        assert O.num_partials(v) == lib.fplx_num_partials(v)
    assert O.ew_grid(1) == 1 and O.ew_grid(257) == 2 and O.ew_grid(10 ** 9) == 4096
    assert O.loop_plan(10, 0, 4, 2) == (1, 1) and O.loop_plan(3, 0, 4, 4) == (0, 1) and O.loop_plan(16, 3, 4, 4) == (1, 0)
    pl = O.apply_plan(65573, 512, 8, True, 4)
    assert pl["grid"] == 4096 and pl["st"] == 4096 * 4 and O.plan_enters_main_and_tail(pl)
    assert not O.plan_enters_main_and_tail(O.apply_plan(16384, 32, 8, True, 4))
    assert O.reduce_geom(500, 512, 8)["iters"] > 1 and O.reduce_geom(500, 512, 8)["lanes"] == 4
    assert O.store(np.float32(1.00390625), True) == 1.0 and O.store(1.01171875, True) == 1.015625       # ties to even
