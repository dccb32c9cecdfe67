"""Order-independent float64 oracles for the BatchNorm kernel family of fpl-plus_amd/csrc/elementwise.hip ("two
oracles"): channel_stats, bn_train_finalize, bn_eval_prepare, bn_act_fwd, bn_act_bwd_reduce / _finalize / _apply and the fused
DownBlock tail bn_act_pool_fwd / pool_bwd_bn_reduce.

The kernels in closed form.  Activations are [V, C] (voxel-major, leading dimension ld >= C); every kernel takes its per-channel
constants as fp32 INPUTS: mean m, rstd r, scale s, shift t (bnbuf rows 0..3), the PReLU slope a, coef k0 / k1.
  z = y s + t (one fma);  pos = z > 0;  keep = Philox mask at the flat index v C + c (oracle.np_ref.philox_keep_mask; C, not ld),
  ik = float(1 / (1 - float(p)));
  bn_act_fwd        out = keep ? (pos ? z : z a) ik : 0
  bn_act_bwd_reduce da = keep ? dout ik : 0;  dz = pos ? da : da a;  xh = (y - m) r;  per partial row: sum dz, sum dz xh per channel
                    and ONE sum over all channels of (pos ? 0 : da z), the slope gradient
  bn_act_bwd_finalize  rows in double: dbeta += float(S0), dgamma += float(S1), dslope += float(Ss), coef = float(S / count) (0 with
                    train = 0: running statistics are constants)
  bn_act_bwd_apply  dy = s (dz - k0 - xh k1)
  bn_act_pool_fwd   a2 = store(pos ? z : z a);  pooled = max of the STORED a2 over the (pd, 2, 2) window
  pool_bwd_bn_reduce  arg = first maximum of the stored a2 in window order t = 4 dd + 2 hh + ww;  dv = store(dskip + (arg == t ?
                    g : 0)) = dx;  the three sums as above with da = dv (the STORED value), no dropout
  channel_stats     per partial row and channel: sum y, sum y^2
  bn_train_finalize rows in double: m = S1 / n, var = max(S2 / n - m m, 0), r = float(1 / sqrt(var + eps)), s = gamma r, t = beta -
                    float(m) s, running mean / variance (1 - mom) old + mom new with the UNBIASED variance var n / (n - 1) (n > 1),
                    num_batches_tracked + 1
  bn_eval_prepare   r = 1 / sqrtf(rv + eps), s = gamma r, t = beta - rm s (all fp32)
`reference_site` / `reference_pool` assert these closed forms against float64 autograd of BatchNorm(train) -> PReLU -> dropout ->
{skip, MaxPool} (1e-11 of the magnitude) before they return, because the bounds need the un-cancelled magnitudes autograd does not give.

A - exact oracle.  The constants are handed in as powers of two (r, s, ik in {1, 2, 4}, a in {1/4, 1/2}) or small dyadic numbers
    (m, t, k0, k1), y / dout / dskip / g small multiples of a power of two, all bf16-representable.  Then z, dz, xh, every product
    and the inner expression of dy have well under 24 significant bits (asserted on the data: the fp32 evaluation equals the
    float64 one element for element) and every TERM of a sum is a multiple of one power of two; while a partial row's sum of
    |terms| in that unit stays below 2^24 (asserted on the data for the kernel's own row partition, `exact_pre`), every partial sum
    is exact in fp32 in ANY order.  Criteria: partial rows summed in float64 equal the float64 sums bit for bit; dgamma / dbeta /
    dslope / coef equal float32(float64 value); out / dy / a2 / pooled / dx equal the float64 value rounded ONCE to the storage type
    (round to nearest even); ties in the pooling window are many and the first maximum wins.
    bn_train_finalize on dyadic rows with a power-of-two count: mean, running mean and num_batches_tracked are +, -, x and one
    division by a power of two - bit equality with the same double expression.  r goes through a double sqrt and a double
    division: two evaluations may differ in the last place of the DOUBLE result (relative 2^-53); the two doubles round to the
    same float unless a rounding boundary of the float grid lies between them, and then to ADJACENT floats: at most 1 fp32 ulp on
    r, and the same on the running variance (a division by n - 1).  s and t are then exact functions of the r the device stored:
    s = float(gamma r) bit for bit, t = float(beta - mf s) with or without contraction of the product into an fma (both legal).
B - rounding oracle.  u = 2^-24, GAMMA_SLACK = 1.01 for second-order terms, ETA = 2^-126 absolute.  hb = 2^-8 (half a bf16 ulp: 8 significant bits,
    relative) where the result is stored in bf16, 0 in fp32.  Per element (each op rounds once, relative to ITS result):
      z: 1 u (fma).  The sign of z is the exact sign (a correctly rounded fma of fp32 inputs cannot underflow to 0 here), so `pos`
      and the keep mask are the same decisions in both evaluations.
      out: 3 u |out| (fma, x a, x ik) + hb (|out| + that).
      dz: 2 u |dz|;  xh: 2 u |xh|;  dz xh: 5 u;  da z: 3 u.
      dy: inner = dz - k0 - xh k1 cancels: bound on M = |dz| + |k0| + |xh k1|: 7 u |s| M (2 + 3 from dz and xh k1, two subtractions
      or one and an fma, x s) + hb (|dy| + that).
    Sums: a partial row adds its terms along a chain of at most `chain` additions from a term to the row's entry - L = (voxels a
      lane takes, from the row-dealing rule: row = (unit / lanes) mod rows, rows = fplx_num_partials) sequential adds, then either
      log2(64 / G) shuffles + 4 wave totals through LDS (G = C / VEC a power of two <= 64) or the serial LDS sum over the VL =
      256 / G lanes; the slope sum takes L VEC + shuffles + 4 G (or VL G) additions.  |err(row)| <= GAMMA_SLACK (e + chain) u sum
      |terms| with e the per-term figure above.  Finalize: the rows in double (rows 2^-52 sum |rows|, any order) and one float
      cast (u |S|), coef one division more (2 u).  End to end dgamma / dbeta / dslope: the rows' bounds added, + u |S|.
    Pool tail: a2 against 2 u |a2| + hb; then the arg-max is taken from the DEVICE's stored a2, so every voxel is compared and
      none is left out: dx = store(dskip + g) against u + hb, and the sums are referred to the device's stored dx.
    Statistics: channel_stats rows (L + 3) u sum |y| and (L + 4) u sum y^2.  Variance as E[y^2] - m^2 from fp32 rows: the absolute
      error of var is dV = E2 / n + 2 |m| E1 / n + (E1 / n)^2 with E1, E2 the totals' bounds, i.e. about chain u (m^2 + sigma^2):
      RELATIVE to sigma^2 it carries the factor (m^2 + sigma^2) / sigma^2 = 1 + (m / sigma)^2 - 1, 65, 4097 at m / sigma = 0, 8, 64.
      r = (var + eps)^-1/2 is monotone, the clamp keeps var' in [max(var - dV, 0), var + dV]: |dr| <= the larger of the two ends'
      distances + u r.  A constant channel has var = 0 in float64 and whatever 0 <= var' <= dV on the device.
    bn_eval_prepare: r 5 u (add, sqrtf and the division at <= 1 ulp each), s 6 u, t u |beta| + 8 u |rm s|.

Mutations (tests/test_bn_oracle_cpu.py) - none is excluded: every listed defect is rejected by A or B at the GPU test's shapes.
`ge_zero` (z >= 0 for z > 0) changes nothing in the forward (both branches give 0 at z = 0) and only dz at z == 0 in the
backward: A sees it (its data has many z == 0), B on continuous data cannot, which is why both oracles run on every case.

Pure numpy / torch on the CPU; tests/test_bn_oracle_cpu.py checks the oracle itself, tests/test_gpu_bn_exact.py applies it."""
import zlib

import numpy as np
import torch

from oracle import np_ref as N

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
HB = 2.0 ** -8
ETA = 2.0 ** -126
GAMMA_SLACK = 1.01
EXACT_LIMIT = float(1 << 24)
EW_THREADS = 256
MUTATIONS = ("drop_last", "twice", "skip_tail",
             "ge_zero", "no_inv_keep_bwd", "mask_ld", "last_max", "col_tie_larger",
             "dslope_kept_out", "xh_scale", "k1_sign", "coef_train0", "swap_dgamma_dbeta",
             "biased_rv", "momentum_side", "count1_guard", "nbt_stuck", "eval_eps_outside",
             "a2_cmp_unrounded", "dv_unrounded")


def rng(key):
    return np.random.default_rng(zlib.crc32(key.encode()))


# ---------------------------------------------------------------- mirrors of the host code (elementwise.hip, common.h)

def num_partials(v, small_div=16):
    """fplx_num_partials: one row per 16 voxels up to 32768 voxels, per 64 above, at most 512"""
    div = small_div if v <= 32768 else 64
    return int(min(512, max(1, -(-v // div))))


def ew_grid(total):
    return int(min(4096, max(1, -(-total // EW_THREADS))))


def vec_of(bf16, c, aligned=True):
    """channels per lane: 8 bf16 / 4 fp32 when C, every ld and every pointer allow 16-byte accesses, else 1"""
    n = 8 if bf16 else 4
    return n if (aligned and c % n == 0) else 1


def group_form(bf16, c, vec, ew_group=1):
    """True where bn_act_fwd / bn_act_bwd_apply take the channel-group-stationary kernels"""
    return bool(bf16 and vec == 8 and ew_group and c // 8 <= EW_THREADS and EW_THREADS % (c // 8) == 0)


def loop_plan(n, start, st, unroll):
    """trips of `for (i = start; i + (U - 1) st < n; i += U st)` and of the tail `for (; i < n; i += st)` -> (main, tail)"""
    main = max(0, -(-(n - start - (unroll - 1) * st) // (unroll * st)))
    i = start + main * unroll * st
    return main, max(0, -(-(n - i) // st))


def apply_plan(v, c, vec, group, unroll):
    """the launch of bn_act_fwd / bn_act_bwd_apply -> dict(grid, stride, n) in loop units (voxels for the group form, vectors for the flat one)"""
    g = c // vec
    grid = ew_grid(v * g)
    if group:
        return dict(grid=grid, st=grid * (EW_THREADS // g), n=v, unroll=unroll)
    return dict(grid=grid, st=grid * EW_THREADS, n=v * g, unroll=4)


def plan_enters_main_and_tail(pl):
    """some lane runs the unrolled loop at least once and some lane runs the tail at least once"""
    ends = [loop_plan(pl["n"], s, pl["st"], pl["unroll"]) for s in (0, pl["st"] - 1)]
    return any(m > 0 for m, _ in ends) and any(t > 0 for _, t in ends)


def deal(units, rows, lanes):
    """the row-dealing rule of every reduction here: unit i goes to row (i / lanes) mod rows, lane i mod lanes, trip i / (lanes
    rows); a unit is one voxel (bn_act_bwd_reduce), the 4 pd voxels of a pooling window or the 2 pd of one of its columns.
    units int [n, m] of voxel ids -> idx [rows, L, lanes], -1 = nothing"""
    units = np.asarray(units, np.int64)
    n, m = units.shape
    i = np.arange(n)
    it = i // (lanes * rows)
    idx = np.full((rows, int(it.max()) + 1, m, lanes), -1, np.int64)
    idx[(i // lanes) % rows, it, :, i % lanes] = units
    return idx.reshape(rows, -1, lanes)


def reduce_geom(v, c, vec, mut=None):
    """bn_act_bwd_reduce_k's partition: G = C / VEC channel groups, VL = 256 / G voxel lanes, rows = fplx_num_partials(V)"""
    g = c // vec
    lanes = EW_THREADS // g
    rows = num_partials(v)
    return dict(idx=_mutate_idx(deal(np.arange(v)[:, None], rows, lanes), v, mut), rows=rows, lanes=lanes, vec=vec, g=g,
                iters=-(-v // (rows * lanes)), pow2=(g & (g - 1)) == 0 and g <= 64)


def stats_geom(v, mut=None):
    """channel_stats_k: 4 voxel lanes per block, a thread per channel"""
    rows = num_partials(v)
    return dict(idx=_mutate_idx(deal(np.arange(v)[:, None], rows, 4), v, mut), rows=rows, lanes=4, vec=1, g=64, pow2=False,
                iters=-(-v // (rows * 4)))


def windows(dims, pd):
    """voxel ids of every pooling window in the order t = 4 dd + 2 hh + ww -> int [Vo, 4 pd]"""
    n, d, h, w = dims
    ids = np.arange(n * d * h * w).reshape(n, d // pd, pd, h // 2, 2, w // 2, 2)
    return ids.transpose(0, 1, 3, 5, 2, 4, 6).reshape(-1, 4 * pd)


def pool_geom(dims, c, pd, col, mut=None):
    """pool_bwd_bn_reduce_k (a lane per pooled voxel) / _col_k (a lane per window column; C / 8 <= 32 and knob pool_col)"""
    n, d, h, w = dims
    v = n * d * h * w
    g = c // 8
    win = windows(dims, pd)
    col = bool(col and g <= 32)
    if col:
        u = np.arange(2 * win.shape[0])
        units = np.stack([win[u >> 1, 2 * t + (u & 1)] for t in range(2 * pd)], 1)      # t8 = 2 t + ww
    else:
        units = win
    rows, lanes = num_partials(v), EW_THREADS // g
    return dict(idx=_mutate_idx(deal(units, rows, lanes), v, mut), rows=rows, lanes=lanes, vec=8, g=g, pow2=True, col=col, win=win, dims=dims, pd=pd,
                iters=-(-units.shape[0] // (rows * lanes)))


def _mutate_idx(idx, v, mut):
    if mut == "drop_last":
        idx = np.where(idx == v - 1, -1, idx)
    elif mut == "twice":
        extra = np.full((idx.shape[0], 1, idx.shape[2]), -1, np.int64)
        extra[0, 0, 0] = 0
        idx = np.concatenate([idx, extra], 1)
    elif mut == "skip_tail":
        idx = idx.copy()
        last = np.where((idx >= 0).any((0, 2)))[0].max()
        idx[:, last] = -1
    return idx


def chains(gm):
    """(additions from a term to its row entry, the same for the slope sum) - see B in the module docstring"""
    big_l = gm["idx"].shape[1]
    if gm["pow2"]:
        sh = int(np.log2(64 // gm["g"])) if gm["g"] < 64 else 0
        return big_l + sh + 4, big_l * gm["vec"] + sh + 4 * gm["g"]
    return big_l + gm["lanes"], big_l * gm["vec"] + gm["lanes"] * gm["g"]


# ---------------------------------------------------------------- number formats

def store(x, bf16):
    """x rounded ONCE (to nearest even) to the storage type -> float64"""
    x = np.asarray(x, F64)
    if not bf16:
        return x.astype(F32).astype(F64)
    m, e = np.frexp(x)
    return np.ldexp(np.rint(m * 256.0) / 256.0, e)


def ulps32(got, want):
    """distance in fp32 ulps of `want`"""
    got, want = np.asarray(got, F64), np.asarray(want, F32)
    return np.abs(got - want.astype(F64)) / np.spacing(np.abs(want)).astype(F64)


def _fma(a, b, c, dt):
    if dt is F64:
        return a * b + c
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)      # the product of two floats is exact in double


def _tree(x, axis):
    x = np.moveaxis(x, axis, 0)
    n = 1
    while n < x.shape[0]:
        n *= 2
    if n != x.shape[0]:
        x = np.concatenate([x, np.zeros((n - x.shape[0],) + x.shape[1:], x.dtype)], 0)
    while x.shape[0] > 1:
        x = x[: x.shape[0] // 2] + x[x.shape[0] // 2:]
    return x[0]


def _seq(x, axis):
    return np.take(np.add.accumulate(x, axis=axis, dtype=x.dtype), -1, axis=axis)


def rowsum(t, gm, dt, t2=None):
    """per-channel terms t (x t2, accumulated with an fma) [V, C] -> [rows, C]: float64 in any order, or fp32 in the kernel's
    order - a lane's voxels one after the other, then the lanes"""
    pad = lambda a: np.concatenate([a, np.zeros((1, a.shape[1]), a.dtype)], 0)[gm["idx"]]
    g = pad(t)
    if dt is F64:
        return (g if t2 is None else g * pad(t2)).sum((1, 2))
    if t2 is None:
        return _tree(_seq(g, 1), 1)
    g2 = pad(t2)
    acc = np.zeros(g.shape[:1] + g.shape[2:], F32)
    for i in range(g.shape[1]):
        acc = _fma(g[:, i], g2[:, i], acc, F32)
    return _tree(acc, 1)


def rowsum_all(t, gm, dt):
    """the slope sum: ONE number per row over all channels -> [rows]"""
    g = np.concatenate([t, np.zeros((1, t.shape[1]), t.dtype)], 0)[gm["idx"]]
    if dt is F64:
        return g.sum((1, 2, 3))
    r, big_l, lanes, c = g.shape
    g = g.reshape(r, big_l, lanes, c // gm["vec"], gm["vec"]).transpose(0, 2, 3, 1, 4).reshape(r, lanes, c // gm["vec"], -1)
    return _seq(_tree(_seq(g, 3), 1), 1)


# ---------------------------------------------------------------- generators

def exact_consts(key, c, fine=True):
    """dyadic per-channel constants: r, |s| powers of two, m / t / k0 / k1 small multiples of a power of two, slope 1/4 or 1/2"""
    g = rng(key)
    k = dict(mean=g.integers(-8, 9, c) / 8.0 if fine else g.integers(-2, 3, c) / 2.0, rstd=2.0 ** g.integers(-1, 2, c),
             scale=2.0 ** g.integers(-1, 2, c) * g.choice([1.0, 1.0, -1.0], c),
             shift=g.integers(-32, 33, c) / 64.0 if fine else g.integers(-8, 9, c) / 4.0,
             slope=float(g.choice([0.25, 0.5])))
    coef = np.stack([g.integers(-8, 9, c) / 16.0, g.integers(-8, 9, c) / 16.0])
    return {n: (np.asarray(x, F32) if n != "slope" else x) for n, x in k.items()}, coef.astype(F32)


def exact_acts(key, v, c, fine=True):
    """y and dout: multiples of 1/8 in [-4, 4] / [-2, 2] (fine) or of 1/2 in [-2, 2] / [-1, 1]; bf16-representable"""
    g = rng(key)
    if fine:
        return (g.integers(-32, 33, (v, c)) / 8.0).astype(F32), (g.integers(-16, 17, (v, c)) / 8.0).astype(F32)
    return (g.integers(-4, 5, (v, c)) / 2.0).astype(F32), (g.integers(-2, 3, (v, c)) / 2.0).astype(F32)


def dyadic_rows(key, c, count, rows):
    """dyadic partial rows of channel_stats for bn_train_finalize with a power-of-two count; channel 1 comes out NEGATIVE before
    the clamp (s2 / n = m^2 (1 - 2^-10)), channel 2 is constant -> stats [rows, 2, C], gamma, beta, running mean, running variance"""
    g = rng(key)
    stats = np.zeros((rows, 2, c), F32)
    stats[:, 0] = g.integers(-64, 65, (rows, c)) / 4.0
    m = stats[:, 0].astype(F64).sum(0) / count
    stats[:, 1] = (count * (m * m + 2.0 ** g.integers(-3, 3, c)) / rows).astype(F32)
    stats[:, 1, 1] = F32(count * (m[1] * m[1]) / rows * (1 - 2.0 ** -10))
    stats[:, 1, 2] = F32(count * (m[2] * m[2]) / rows)
    gamma, beta = 2.0 ** g.integers(-1, 2, c) * g.choice([1.0, -1.0], c), g.integers(-8, 9, c) / 8.0
    rm, rv = g.integers(-8, 9, c) / 8.0, 2.0 ** g.integers(-2, 3, c)
    return stats, gamma.astype(F32), beta.astype(F32), rm.astype(F32), rv.astype(F32)


def exact_pool_grads(key, v, vo, c):
    """dskip in {0, +-1/2, +-1} (half of them 0), g multiples of 1/256 in [-1/4, 1/4]: bf16 values whose sum needs 9 bits where
    |dskip| = 1, so dx rounds; small enough for the slope sum's 2^24 units at 16384 terms a row"""
    g = rng(key)
    return g.choice(np.asarray([-1, -0.5, 0, 0, 0, 0, 0.5, 1], F32), (v, c)), (g.integers(-64, 65, (vo, c)) / 256.0).astype(F32)


def real_acts(key, v, c, bf16, ratio=None):
    """N(0, 1)-like y with per-channel offsets and scales (mean / sigma = ratio where given), dout ~ 0.01 N(0, 1); values of
    the storage type"""
    g = rng(key)
    sig = 0.5 + g.random(c)
    off = g.standard_normal(c) if ratio is None else ratio * sig
    y = g.standard_normal((v, c)) * sig + off
    return store(y, bf16).astype(F32), store(0.01 * g.standard_normal((v, c)), bf16).astype(F32)


def real_consts(key, y, eps=1e-5):
    """the site's true constants from y (float64 statistics, then floats) and the coefficients a dout of 0.01 N(0, 1) gives"""
    g = rng(key)
    c = y.shape[1]
    yd = y.astype(F64)
    m, var = yd.mean(0), yd.var(0)
    gamma, beta = 0.5 + g.random(c), 0.3 * g.standard_normal(c)
    gamma[::5] *= -1.0
    rs = 1.0 / np.sqrt(var + eps)
    k = dict(mean=m.astype(F32), rstd=rs.astype(F32), scale=(gamma * rs).astype(F32), shift=(beta - m * gamma * rs).astype(F32),
             slope=float(F32(0.25)))
    return k, (1e-3 * g.standard_normal((2, c))).astype(F32)


def dropout(p, seed, sid, v, c, ld=None):
    """keep mask [V, C] at the flat index v C + c (ld: what a kernel indexing with its leading dimension would draw) and ik"""
    if p <= 0:
        return None, 1.0
    ld = c if ld is None else ld
    keep = N.philox_keep_mask(seed, sid, v * ld, p).reshape(v, ld)[:, :c]
    return keep, float(F32(1.0 / (1.0 - float(F32(p)))))


# ---------------------------------------------------------------- the kernels, float64 (dt = F64) or fp32 in their own order

def elem(y, dout, k, keep, ik, dt=F64, mut=None):
    """per-element quantities of a site -> dict(z, pos, act, out, da, dz, xh, ts)"""
    f = lambda a: np.asarray(a, dt)
    y, sc, sh, m, rs = f(y), f(k["scale"]), f(k["shift"]), f(k["mean"]), f(k["rstd"])
    sl, zero = dt(k["slope"]), dt(0)
    z = _fma(y, np.broadcast_to(sc, y.shape), np.broadcast_to(sh, y.shape), dt)
    pos = z >= 0 if mut == "ge_zero" else z > 0
    act = np.where(pos, z, z * sl)
    r = dict(z=z, pos=pos, act=act, out=act if keep is None else np.where(keep, act * dt(ik), zero))
    if dout is not None:
        d = f(dout) * dt(1.0 if mut == "no_inv_keep_bwd" else ik)
        da = d if keep is None else np.where(keep, d, zero)
        r["da"] = da
        r["dz"] = np.where(pos, da, da * sl)
        r["xh"] = (y - m) * (sc if mut == "xh_scale" else rs)
        r["ts"] = np.where(pos, zero, (d if mut == "dslope_kept_out" else da) * z)
    return r


def part_rows(e, gm, dt):
    """partial rows [rows, 2 C + 1] of a reduction from the per-element dz, xh, ts"""
    return np.concatenate([rowsum(e["dz"], gm, dt), rowsum(e["dz"], gm, dt, e["xh"]), rowsum_all(e["ts"], gm, dt)[:, None]], 1)


def bwd_finalize(part, c, count, train, mut=None):
    """float64 of bn_act_bwd_finalize on given rows -> dbeta, dgamma, dslope (increments), coef [2, C]"""
    s = np.asarray(part, F64).sum(0)
    db, dg = s[:c], s[c:2 * c]
    if mut == "swap_dgamma_dbeta":
        db, dg = dg, db
    coef = np.stack([s[:c], s[c:2 * c]]) / float(count)
    if not train and mut != "coef_train0":
        coef = np.zeros_like(coef)
    return db, dg, s[2 * c], coef


def apply_dy(e, k, coef, dt=F64, mut=None):
    k0, k1, sc = np.asarray(coef[0], dt), np.asarray(coef[1], dt), np.asarray(k["scale"], dt)
    xk = e["xh"] * k1
    return sc * ((e["dz"] - k0) + xk if mut == "k1_sign" else (e["dz"] - k0) - xk)


def first_max(a, mut=None):
    """a [Vo, T, C] -> index of the window's maximum: the FIRST one in window order"""
    if mut == "last_max":
        return a.shape[1] - 1 - np.argmax(a[:, ::-1], 1)
    if mut == "col_tie_larger":                       # the pair of columns resolves a tie to the larger window index
        t = np.arange(a.shape[1])
        best, arg = [], []
        for ww in (0, 1):
            sub = a[:, t[t % 2 == ww]]
            i = np.argmax(sub, 1)
            best.append(np.take_along_axis(sub, i[:, None], 1)[:, 0])
            arg.append(2 * i + ww)
        other = (best[1] > best[0]) | ((best[1] == best[0]) & (arg[1] > arg[0]))
        return np.where(other, arg[1], arg[0])
    return np.argmax(a, 1)


def pool_fwd(y, k, gm, dt=F64, mut=None, bf16=True):
    """-> a2 as stored, pooled as stored, the unrounded activation"""
    e = elem(y, None, k, None, 1.0, dt, mut)
    a2 = store(e["act"], bf16)
    cmp_ = e["act"].astype(F64) if mut == "a2_cmp_unrounded" else a2
    return a2, store(cmp_[gm["win"]].max(1), bf16), e


def pool_bwd(y, g, dskip, k, gm, a2, dt=F64, mut=None, bf16=True, dx_stored=None):
    """a2: the stored activation the arg-max is taken from.  dx_stored: take the sums from this stored d(a2) (oracle B refers
    them to the device's own).  -> dx as stored, partial rows, per-element dict"""
    win = gm["win"]
    v, c = y.shape
    e = elem(y, None, k, None, 1.0, dt, mut)
    if mut == "a2_cmp_unrounded":
        a2 = e["act"].astype(F64)
    arg = first_max(np.asarray(a2, F64)[win], mut)                                      # [Vo, C]
    add = np.zeros((v, c), F64)
    add[np.take_along_axis(win, arg, 1), np.arange(c)[None, :]] = np.asarray(g, F64)
    exact = add + (0.0 if dskip is None else np.asarray(dskip, F64))
    if dt is F32:
        exact = exact.astype(F32).astype(F64)
    dx = store(exact, bf16)
    dv = (exact if mut == "dv_unrounded" else dx if dx_stored is None else np.asarray(dx_stored, F64)).astype(dt)
    e["da"] = dv
    e["dz"] = np.where(e["pos"], dv, dv * dt(k["slope"]))
    e["xh"] = (np.asarray(y, dt) - np.asarray(k["mean"], dt)) * np.asarray(k["rstd"], dt)
    e["ts"] = np.where(e["pos"], dt(0), dv * e["z"])
    e["routed"] = add != 0
    return dx, part_rows(e, gm, dt), e


def channel_stats(y, gm, dt=F64):
    """-> part [rows, 2, C]"""
    y = np.asarray(y, dt)
    return np.stack([rowsum(y, gm, dt), rowsum(y, gm, dt, y)], 1)


def train_finalize(stats, count, gamma, beta, rm, rv, nbt, mom, eps, mut=None):
    """the double expression of bn_train_finalize_k on given rows; float casts where the kernel has them -> dict"""
    s = np.asarray(stats, F64).sum(0)
    n = float(count)
    m = s[0] / n
    raw = s[1] / n - m * m
    var = np.maximum(raw, 0.0)
    rs = 1.0 / np.sqrt(var + float(F32(eps)))
    mf, rsf = m.astype(F32), rs.astype(F32)
    sc = (np.asarray(gamma, F32) * rsf).astype(F32)
    momf, one_m = F32(mom), F32(1.0) - F32(mom)
    r = dict(m=m, var=var, var_raw=raw, rs=rs, mean=mf, rstd=rsf, scale=sc, nbt=None if nbt is None else int(nbt) + (0 if mut == "nbt_stuck" else 1),
             shift=(np.asarray(beta, F64) - mf.astype(F64) * sc.astype(F64)))
    if mut == "count1_guard":
        with np.errstate(divide="ignore", invalid="ignore"):
            unb = var * n / (n - 1.0)
    else:
        unb = var * n / (n - 1.0) if n > 1 else var
    if mut == "biased_rv":
        unb = var
    a, b = (momf, one_m) if mut == "momentum_side" else (one_m, momf)
    r["unb"] = unb
    r["rm"] = None if rm is None else F64(a) * np.asarray(rm, F64) + F64(b) * mf.astype(F64)
    r["rv"] = None if rv is None else F64(a) * np.asarray(rv, F64) + F64(b) * np.asarray(unb, F32).astype(F64)
    return r


def eval_prepare(gamma, beta, rm, rv, eps, dt=F64, mut=None):
    f = lambda a: np.asarray(a, dt)
    e = dt(F32(eps))
    rs = (dt(1) / np.sqrt(f(rv)) + e) if mut == "eval_eps_outside" else dt(1) / np.sqrt(f(rv) + e)
    sc = f(gamma) * rs
    return sc, f(beta) - f(rm) * sc


# ---------------------------------------------------------------- the closed forms against float64 autograd

def _close(a, b, mag, what):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    lim = 1e-11 * (float(np.max(np.abs(mag))) + 1e-300)
    assert float(np.max(np.abs(a - b))) <= lim, "%s: closed form and autograd differ by %g (limit %g)" % (what, np.max(np.abs(a - b)), lim)


def autograd_check(y, dout, gamma, beta, slope, p, seed, sid, eps=1e-5, pool=None):
    """BatchNorm(train) -> PReLU -> dropout [-> {skip, MaxPool}] in float64 torch against the closed forms above evaluated with
    the float64 constants of the same data.  pool = (dims, pd, g, dskip): the pooling sees the bf16-stored a2 (straight-through)."""
    v, c = y.shape
    yd = torch.from_numpy(np.asarray(y, F64)).requires_grad_(True)
    gd, bd = torch.from_numpy(np.asarray(gamma, F64)).requires_grad_(True), torch.from_numpy(np.asarray(beta, F64)).requires_grad_(True)
    sd = torch.tensor([float(slope)], dtype=torch.float64, requires_grad=True)
    mean, var = yd.mean(0), yd.var(0, unbiased=False)
    z = (yd - mean) * torch.rsqrt(var + eps) * gd + bd
    a = torch.where(z > 0, z, z * sd)
    keep, ik = dropout(p, seed, sid, v, c)
    if keep is not None:
        a = a * torch.from_numpy(keep.astype(F64)) * ik
    m64, v64 = np.asarray(y, F64).mean(0), np.asarray(y, F64).var(0)
    rs = 1.0 / np.sqrt(v64 + eps)
    k = dict(mean=m64, rstd=rs, scale=np.asarray(gamma, F64) * rs, shift=np.asarray(beta, F64) - m64 * np.asarray(gamma, F64) * rs, slope=float(slope))
    one = dict(idx=np.arange(v).reshape(1, v, 1), vec=1, g=c, lanes=1, pow2=False)
    if pool is None:
        a.backward(torch.from_numpy(np.asarray(dout, F64)))
        e = elem(y, dout, k, keep, ik)
        _close(e["out"], a.detach().numpy(), e["out"], "out")
    else:
        dims, pd, g, dskip = pool
        n, d, h, w = dims
        gm = dict(one, win=windows(dims, pd))
        a2, pooled, _ = pool_fwd(y, k, gm)
        aq = a + (torch.from_numpy(store(a.detach().numpy(), True)) - a.detach())
        pr = torch.nn.functional.max_pool3d(aq.view(n, d, h, w, c).permute(0, 4, 1, 2, 3), (pd, 2, 2), (pd, 2, 2))
        pr = pr.permute(0, 2, 3, 4, 1).reshape(-1, c)
        _close(pooled, pr.detach().numpy(), pooled, "pooled")
        ((pr * torch.from_numpy(np.asarray(g, F64))).sum() + (aq * torch.from_numpy(np.asarray(dskip, F64))).sum()).backward()
        # autograd does not round d(a2) to bf16: compare with the unrounded routing (fp32 storage = identity on these sums)
        _, _, e = pool_bwd(y, g, dskip, k, gm, a2, mut="dv_unrounded")
    part = part_rows(e, one, F64)
    db, dg, ds, coef = bwd_finalize(part, c, v, 1)
    _close(db, bd.grad.numpy(), np.abs(e["dz"]).sum(0), "dbeta")
    _close(dg, gd.grad.numpy(), np.abs(e["dz"] * e["xh"]).sum(0), "dgamma")
    _close(ds, sd.grad.numpy(), np.abs(e["ts"]).sum(), "dslope")
    dy = apply_dy(e, k, coef)
    mag = np.abs(k["scale"]) * (np.abs(e["dz"]) + np.abs(coef[0]) + np.abs(e["xh"] * coef[1]))
    _close(dy, yd.grad.numpy(), mag, "dy")
    return True


# ---------------------------------------------------------------- checks: A (exact) and B (bound)

def ratio(got, ref, bound):
    """max |got - ref| / bound (NaN / inf -> inf; 0 / 0 -> 0): <= 1 passes"""
    got, ref, bound = np.asarray(got, F64), np.asarray(ref, F64), np.asarray(bound, F64)
    if got.size == 0:
        return 0.0
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bound)
    q = np.where(np.isfinite(got) & ~np.isnan(q), q, np.inf)
    return float(q.max())


def _finish(res, exact, what):
    bad = {n: r for n, r in res.items() if not r <= (0.0 if exact else 1.0)}
    assert not bad, "%s (%s): %s" % (what, "A: entries that differ" if exact else "B: error / bound", bad)
    return res


def _same(got, want):
    """number of entries that differ (NaN differs from everything)"""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float((~(got == want)).sum())


def _unit_bits(t):
    for b in range(0, 24):
        if np.array_equal(t * 2.0 ** b, np.round(t * 2.0 ** b)):
            return b
    raise AssertionError("terms are not multiples of 2^-23: the data is not exact")


def exact_rows_pre(e, gm):
    """precondition of oracle A on the data: per sum, all terms multiples of one power of two and every row's sum of |terms| in
    that unit below 2^24 -> the largest such sum"""
    worst = 0.0
    for t, whole in ((np.abs(e["dz"]), False), (np.abs(e["dz"] * e["xh"]), False), (np.abs(e["ts"]), True)):
        t = np.asarray(t, F64)
        b = _unit_bits(t)
        mag = rowsum_all(t, gm, F64) if whole else rowsum(t, gm, F64)
        worst = max(worst, float(mag.max()) * 2.0 ** b)
    assert worst < EXACT_LIMIT, "a row's sum of |terms| reaches %g units >= 2^24" % worst
    return worst


def exact_pre(y, dout, k, coef, p, bf16=True, gm=None):
    """precondition of oracle A, asserted on the data: dyadic constants, power-of-two r, s, ik, storage-representable y / dout,
    every per-element intermediate exact in fp32, and (with a row partition) `exact_rows_pre`"""
    assert p in (0.0, 0.5, 0.75) and k["slope"] in (0.25, 0.5)
    for n in ("rstd", "scale"):
        assert np.all(np.abs(np.frexp(np.asarray(k[n], F64))[0]) == 0.5), "%s must be powers of two" % n
    for a in (k["mean"], k["shift"]) + (() if coef is None else (coef,)):
        assert np.array_equal(np.asarray(a, F64) * 1024, np.round(np.asarray(a, F64) * 1024))
    for a in (y, dout):
        assert a is None or np.array_equal(store(a, bf16), np.asarray(a, F64)), "y / dout must be values of the storage type"
    keep = None if p == 0 else np.ones(y.shape, bool)
    ik = 1.0 / (1.0 - p)
    e64, e32 = elem(y, dout, k, keep, ik, F64), elem(y, dout, k, keep, ik, F32)
    names = ["z", "out"] + (["dz", "xh", "ts"] if dout is not None else [])
    for n in names:
        assert np.array_equal(e64[n], e32[n].astype(F64)), "%s is not exact in fp32 on this data" % n
    if dout is not None:
        assert np.array_equal(e64["dz"] * e64["xh"], (e32["dz"] * e32["xh"]).astype(F64))
        if coef is not None:
            assert np.array_equal(apply_dy(e64, k, coef) / np.asarray(k["scale"], F64),
                                  (apply_dy(e32, k, coef, F32) / np.asarray(k["scale"], F32)).astype(F64)), "dy's inner expression is not exact"
        if gm is not None:
            return exact_rows_pre(e64, gm)
    return 0.0


def check_fwd(out_got, y, k, p, seed, sid, bf16, exact, what="fwd"):
    keep, ik = dropout(p, seed, sid, y.shape[0], y.shape[1])
    e = elem(y, None, k, keep, ik)
    res = {}
    if exact:
        exact_pre(y, None, k, None, p, bf16)
        res["out"] = _same(out_got, store(e["out"], bf16))
    else:
        b = 3 * U * np.abs(e["out"])
        res["out"] = ratio(out_got, e["out"], GAMMA_SLACK * (b + (HB if bf16 else 0) * (np.abs(e["out"]) + b)) + ETA)
    if keep is not None:                                   # the mask itself: exactly the oracle's Philox stream
        og = np.asarray(out_got, F64)
        assert np.all(og[~keep] == 0) and np.all((og != 0) | ~keep | (e["out"] == 0) | (np.abs(e["out"]) < 1e-30)), "%s: dropout mask differs" % what
    return _finish(res, exact, what)


def rows_bounds(e, gm):
    """bounds [rows, 2 C + 1] of a reduction's partial rows"""
    ch, chs = chains(gm)
    f = lambda n: np.asarray(e[n], F64)
    return GAMMA_SLACK * U * np.concatenate([(2 + ch) * rowsum(np.abs(f("dz")), gm, F64), (5 + ch) * rowsum(np.abs(f("dz") * f("xh")), gm, F64),
                                             (3 + chs) * rowsum_all(np.abs(f("ts")), gm, F64)[:, None]], 1) + ETA


def check_rows(part_got, e, gm, exact, what):
    """partial rows of bn_act_bwd_reduce / pool_bwd_bn_reduce.  A: the rows summed in float64 equal the float64 sums bit for
    bit (and so does every row).  B: every row within its bound, and the totals within the rows' bounds added."""
    ref = part_rows(e, gm, F64)
    pg = np.asarray(part_got, F64)
    if exact:
        exact_rows_pre(e, gm)
        return {"rows": _same(pg, ref), "totals": _same(pg.sum(0), ref.sum(0))}
    b = rows_bounds(e, gm)
    return {"rows": ratio(pg, ref, b), "totals": ratio(pg.sum(0), ref.sum(0), b.sum(0))}


def check_finalize(got, part, c, count, train, exact, what="finalize", acc0=0.0):
    """got = (dbeta, dgamma, dslope, coef) of bn_act_bwd_finalize on the rows `part` (the accumulators started at acc0)"""
    db, dg, ds, coef = bwd_finalize(part, c, count, train)
    res = {}
    mag = np.abs(np.asarray(part, F64)).sum(0)
    eps_d = part.shape[0] * 2.0 ** -52 * mag
    for n, g_, r_, m_ in (("dbeta", got[0], db, eps_d[:c]), ("dgamma", got[1], dg, eps_d[c:2 * c]), ("dslope", got[2], ds, eps_d[2 * c])):
        if exact:
            res[n] = _same(g_, (F32(acc0) + np.asarray(r_, F32)).astype(F64) if acc0 else np.asarray(r_, F32))
        else:
            res[n] = ratio(g_, acc0 + r_, GAMMA_SLACK * (U * (np.abs(r_) + np.abs(acc0 + r_) * (acc0 != 0)) + m_) + ETA)
    if exact or not train:
        res["coef"] = _same(got[3], coef.astype(F32))
    else:
        res["coef"] = ratio(got[3], coef, GAMMA_SLACK * (2 * U * np.abs(coef) + np.stack([eps_d[:c], eps_d[c:2 * c]]) / count) + ETA)
    return _finish(res, exact, what)


def check_apply(dy_got, e, k, coef, bf16, exact, what="apply"):
    dy = apply_dy(e, k, coef)
    if exact:
        return _finish({"dy": _same(dy_got, store(dy, bf16))}, True, what)
    mag = np.abs(np.asarray(k["scale"], F64)) * (np.abs(e["dz"]) + np.abs(np.asarray(coef[0], F64)) + np.abs(e["xh"] * np.asarray(coef[1], F64)))
    b = 7 * U * mag
    return _finish({"dy": ratio(dy_got, dy, GAMMA_SLACK * (b + (HB if bf16 else 0) * (np.abs(dy) + b)) + ETA)}, False, what)


def check_site(got, y, dout, k, coef, p, seed, sid, bf16, gm, exact, train=1, what="site", use_autograd=False, acc0=0.0):
    """a whole BatchNorm site: got = dict(out, part, dbeta, dgamma, dslope, coef, dy) - any subset; the finalize is referred to
    the rows it was given, the apply pass to the coef it was given (`coef`; None: got["coef"])."""
    v, c = y.shape
    keep, ik = dropout(p, seed, sid, v, c)
    if exact:
        exact_pre(y, dout, k, coef, p, bf16, gm)
    if use_autograd:
        reference_site(y, dout, p, seed, sid)
    e = elem(y, dout, k, keep, ik)
    res = {}
    if "out" in got:
        res.update(check_fwd(got["out"], y, k, p, seed, sid, bf16, exact, what))
    if "part" in got:
        res.update(_finish(check_rows(got["part"], e, gm, exact, what), exact, what))
        if "dbeta" in got:
            res.update(check_finalize((got["dbeta"], got["dgamma"], got["dslope"], got["coef"]), got["part"], c, v, train, exact, what, acc0))
            if not exact and train:                        # end to end: the gradients against the float64 sums over the data
                ref = part_rows(e, gm, F64).sum(0)
                b = rows_bounds(e, gm).sum(0) + GAMMA_SLACK * U * np.abs(ref) + ETA
                end = np.concatenate([got["dbeta"], got["dgamma"], np.reshape(got["dslope"], 1)]).astype(F64) - acc0
                res["end_to_end"] = ratio(end, ref, b + GAMMA_SLACK * U * abs(acc0))
    if "dy" in got:
        res.update(check_apply(got["dy"], e, k, got["coef"] if coef is None else coef, bf16, exact, what))
    return _finish(res, exact, what)


def reference_site(y, dout, p, seed, sid, pool=None):
    """the self-check every reference run carries: the closed forms against float64 autograd on THIS y / dout (affine parameters
    drawn here; the closed forms take whatever constants they are handed, autograd needs the data's own statistics)"""
    g = rng("ag%d" % y.shape[1])
    c = y.shape[1]
    if y.shape[0] < 2 or float(np.asarray(y, F64).var(0).min()) == 0:
        return False
    return autograd_check(y, dout, 0.5 + g.random(c), 0.3 * g.standard_normal(c), 0.25, p, seed, sid, pool=pool)


def check_pool(got, y, g, dskip, k, gm, exact, what="pool", use_autograd=False):
    """the fused tail: got = dict(a2, pooled, dx, part).  B takes the arg-max from the device's stored a2 (after a2 passed its own
    bound) and refers the sums to the device's stored dx (after dx passed its own): no voxel is left out."""
    if use_autograd:
        reference_site(y, None, 0.0, 0, 0, pool=(gm["dims"], gm["pd"], g, np.zeros_like(y) if dskip is None else dskip))
    a2, pooled, e0 = pool_fwd(y, k, gm)
    res = {}
    if exact:
        exact_pre(y, None, k, None, 0.0, True)
        res["a2"], res["pooled"] = _same(got["a2"], a2), _same(got["pooled"], pooled)
        if "dx" in got:
            dx, _, e = pool_bwd(y, g, dskip, k, gm, a2)
            res["dx"] = _same(got["dx"], dx)
            res.update(check_rows(got["part"], e, gm, True, what))
        return _finish(res, True, what)
    act = np.abs(e0["act"])
    res["a2"] = ratio(got["a2"], e0["act"], GAMMA_SLACK * (2 * U * act + HB * (1 + 2 * U) * act) + ETA)
    _finish(res, False, what)
    a2g = np.asarray(got["a2"], F64)
    res["pooled"] = _same(got["pooled"], a2g[gm["win"]].max(1))                        # the maximum of the stored values: exact
    assert res.pop("pooled") == 0, "%s: pooled is not the maximum of the stored a2" % what
    if "dx" in got:
        _, _, e = pool_bwd(y, g, dskip, k, gm, a2g, mut="dv_unrounded")
        ex = np.abs(e["da"])
        res["dx"] = ratio(got["dx"], e["da"], np.where(e["routed"], GAMMA_SLACK * (U + HB) * ex + ETA, 0.0))
        _finish(res, False, what)
        _, _, e = pool_bwd(y, g, dskip, k, gm, a2g, dx_stored=got["dx"])
        res.update(check_rows(got["part"], e, gm, False, what))
    return _finish(res, False, what)


def check_stats(part_got, y, gm, exact, what="stats"):
    """channel_stats rows [rows, 2, C]"""
    yd = np.asarray(y, F64)
    ref = channel_stats(yd, gm)
    pg = np.asarray(part_got, F64)
    if exact:
        b = _unit_bits(yd * yd)
        assert float(rowsum(yd * yd, gm, F64).max()) * 2.0 ** b < EXACT_LIMIT
        return _finish({"rows": _same(pg, ref)}, True, what)
    big_l = gm["idx"].shape[1]
    bound = GAMMA_SLACK * U * np.stack([(big_l + 3) * rowsum(np.abs(yd), gm, F64), (big_l + 4) * ref[:, 1]], 1) + ETA
    return _finish({"rows": ratio(pg, ref, bound)}, False, what)


def check_train_finalize(got, stats, count, gamma, beta, rm, rv, nbt, mom, eps, exact, what="train_finalize", data_bounds=None):
    """got = dict(mean, rstd, scale, shift, rm, rv, nbt).  exact: the A criteria of the module docstring on dyadic rows.  Else B
    on the given rows; data_bounds = (m, var, dm, dvar) refers mean / rstd / scale / shift to the float64 statistics of the DATA
    with the absolute errors the fp32 rows add (the statistics path)."""
    r = train_finalize(stats, count, gamma, beta, rm, rv, nbt, mom, eps)
    res = {}
    gamma, beta = np.asarray(gamma, F64), np.asarray(beta, F64)
    if got.get("nbt") is not None:
        assert int(got["nbt"]) == r["nbt"], "%s: num_batches_tracked %d != %d" % (what, got["nbt"], r["nbt"])
    if exact:
        res["mean"] = _same(got["mean"], r["mean"])
        res["rstd"] = float((~(ulps32(got["rstd"], r["rstd"]) <= 1)).sum())
        rs_g, sc_g, mf = np.asarray(got["rstd"], F64), np.asarray(got["scale"], F64), r["mean"].astype(F64)
        res["scale"] = _same(got["scale"], (gamma * rs_g).astype(F32))
        sh = np.asarray(got["shift"], F64)
        res["shift"] = float((~((sh == (beta - mf * sc_g).astype(F32)) | (sh == (beta - (mf * sc_g).astype(F32)).astype(F32)))).sum())
        if rm is not None:
            res["rm"] = _same(got["rm"], r["rm"].astype(F32))
            res["rv"] = float((~(ulps32(got["rv"], r["rv"].astype(F32)) <= 1)).sum())
        return _finish(res, True, what)
    rows = np.asarray(stats).shape[0]
    m, var = (r["m"], r["var"]) if data_bounds is None else data_bounds[:2]
    e2 = np.abs(np.asarray(stats, F64)).sum(0)[1] / count
    dm = rows * 2.0 ** -52 * np.abs(np.asarray(stats, F64)).sum(0)[0] / count
    dvar = (rows + 4) * 2.0 ** -52 * (e2 + m * m)
    if data_bounds is not None:
        dm, dvar = dm + data_bounds[2], dvar + data_bounds[3]
    epsf = float(F32(eps))
    rs = 1.0 / np.sqrt(var + epsf)
    lo, hi = np.maximum(var - dvar, 0.0), var + dvar
    drs = np.maximum(np.abs(1.0 / np.sqrt(lo + epsf) - rs), np.abs(1.0 / np.sqrt(hi + epsf) - rs)) + 2 * U * rs
    res["mean"] = ratio(got["mean"], m, GAMMA_SLACK * (U * np.abs(m) + dm) + ETA)
    res["rstd"] = ratio(got["rstd"], rs, GAMMA_SLACK * drs)
    dsc = np.abs(gamma) * drs + U * np.abs(gamma * rs)
    res["scale"] = ratio(got["scale"], gamma * rs, GAMMA_SLACK * dsc)
    res["shift"] = ratio(got["shift"], beta - m * gamma * rs,
                         GAMMA_SLACK * (U * np.abs(beta) + 4 * U * np.abs(m * gamma * rs) + np.abs(m) * dsc + (U * np.abs(m) + dm) * np.abs(gamma * rs)) + ETA)
    if rm is not None and data_bounds is None:
        res["rm"] = ratio(got["rm"], r["rm"], GAMMA_SLACK * 3 * U * (np.abs(np.asarray(rm, F64)) + np.abs(m)) + ETA)
        unb = np.asarray(r["unb"], F64)
        res["rv"] = ratio(got["rv"], (1.0 - float(F32(mom))) * np.asarray(rv, F64) + float(F32(mom)) * unb,
                          GAMMA_SLACK * (4 * U * (np.abs(np.asarray(rv, F64)) + unb) + dvar * 2) + ETA)
    return _finish(res, False, what)


def stats_path_bounds(y, gm):
    """float64 mean / variance of the data and the absolute errors fp32 partial rows add to them -> m, var, dm, dvar, amplification
    (m^2 + sigma^2) / sigma^2 of the variance's relative error"""
    yd = np.asarray(y, F64)
    n = yd.shape[0]
    big_l = gm["idx"].shape[1]
    m, var = yd.mean(0), yd.var(0)
    e1 = GAMMA_SLACK * U * (big_l + 3) * np.abs(yd).sum(0) / n
    e2 = GAMMA_SLACK * U * (big_l + 4) * (yd * yd).sum(0) / n
    with np.errstate(divide="ignore"):
        amp = (m * m + var) / var
    return m, var, e1, e2 + 2 * np.abs(m) * e1 + e1 * e1, amp


def check_eval_prepare(got_scale, got_shift, gamma, beta, rm, rv, eps, exact, what="eval_prepare"):
    sc, sh = eval_prepare(gamma, beta, rm, rv, eps)
    if exact:
        assert eps == 0 and np.all(np.abs(np.frexp(np.sqrt(np.asarray(rv, F64)))[0]) == 0.5), "A needs eps = 0 and rv a power of four"
        return _finish({"scale": _same(got_scale, sc.astype(F32)), "shift": _same(got_shift, sh.astype(F32))}, True, what)
    return _finish({"scale": ratio(got_scale, sc, GAMMA_SLACK * 6 * U * np.abs(sc)),
                    "shift": ratio(got_shift, sh, GAMMA_SLACK * (U * np.abs(np.asarray(beta, F64)) + 8 * U * np.abs(np.asarray(rm, F64) * sc)) + ETA)},
                   False, what)


# ---------------------------------------------------------------- the fp32 restatement (tests/test_bn_oracle_cpu.py)

def restate_site(y, dout, k, coef, p, seed, sid, bf16, gm, train=1, mut=None, ld=None):
    """the site's kernels in fp32 numpy with their rounding points and row partition -> the dict `check_site` takes"""
    v, c = y.shape
    keep, ik = dropout(p, seed, sid, v, c, ld if mut == "mask_ld" else None)
    e = elem(y, dout, k, keep, ik, F32, mut)
    part = part_rows(e, gm, F32)
    db, dg, ds, cf = bwd_finalize(part, c, v, train, mut)
    return dict(out=store(e["out"], bf16), part=part, dbeta=db.astype(F32), dgamma=dg.astype(F32), dslope=F32(ds), coef=cf.astype(F32),
                dy=store(apply_dy(e, k, coef, F32, mut), bf16))


def restate_pool(y, g, dskip, k, gm, mut=None):
    a2, pooled, _ = pool_fwd(y, k, gm, F32, mut)
    dx, part, _ = pool_bwd(y, g, dskip, k, gm, a2, F32, mut)
    return dict(a2=a2, pooled=pooled, dx=dx, part=part)


def restate_train_finalize(stats, count, gamma, beta, rm, rv, nbt, mom, eps, mut=None):
    r = train_finalize(stats, count, gamma, beta, rm, rv, nbt, mom, eps, mut)
    return dict(mean=r["mean"], rstd=r["rstd"], scale=r["scale"], shift=(np.asarray(beta, F64) - (r["mean"].astype(F64) * r["scale"].astype(F64))).astype(F32),
                rm=None if rm is None else r["rm"].astype(F32), rv=None if rv is None else np.asarray(r["rv"], F64).astype(F32), nbt=r["nbt"])
