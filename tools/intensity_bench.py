"""Secondary measurement (not a bench.py line): the intensity kernels (csrc/intensity.hip) on one 1x48x160x272 volume (the
VS inference size), one channel.  Per pass it reports
  device   HIP events around `iters` back-to-back calls into preallocated buffers after warm-up: min-max normalisation
           (reduction + apply, no host synchronisation), the selection behind the percentiles alone (3 ranks: the two
           percentiles and the largest element) and the whole percentile normalisation (selection, one device->host copy
           of 6 floats, the apply), gamma (reduction + apply), and both noise paths (the float64 add of an uploaded host
           draw - the draw and the upload are timed apart, by wall clock - and the Philox generator);
  copy     fplx_crop_flip writing a volume of the same size: the project's plain-copy yardstick;
  numpy    the reference's numpy pass on the same array on this machine's CPU (wall clock, median).
Outputs are compared in the same run (differing elements; for gamma the distance from the float64 evaluation).
usage: python tools/intensity_bench.py [--iters N] [--reps N] [--out FILE.json]"""
import argparse
import ctypes
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
for p in ("..", os.path.join("..", "fpl-plus_amd"), os.path.join("..", "tests", "golden"), os.path.join("..", "tests")):
    sys.path.insert(0, os.path.join(HERE, p))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import detdata  # noqa: E402
import fplx  # noqa: E402,F401
import intensity_ref as IR  # noqa: E402
from fplx import _lib, ops  # noqa: E402
from fplx._lib import call  # noqa: E402

SHAPE = (48, 160, 272)
Q = (1.0, 99.0)
GAMMA = 1.3
SEED, STREAM, MEAN, STD = 0x5EED5EED5EED5EED, 0, 0.0, 0.1


def event_ms(once, iters):
    for _ in range(5):
        once()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        once()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def wall_ms(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def bits_differ(a, b):
    return int((np.ascontiguousarray(a, np.float32).view(np.uint32) != np.ascontiguousarray(b, np.float32).view(np.uint32)).sum())


def np_minmax(x):
    y = x.copy()
    v0, v1 = y.min(), y.max()
    y[y < v0] = v0
    y[y > v1] = v1
    return (y - v0) / (v1 - v0)


def np_percentiles(x):
    y = x.copy()
    v0, v1 = np.percentile(y, Q[0]), np.percentile(y, Q[1])
    y[y < v0] = v0
    y[y > v1] = v1
    return (y - v0) / (v1 - v0)


def np_gamma(x):
    v_min, v_max = x.min(), x.max()
    y = (x - v_min) / (v_max - v_min)
    return np.power(y, GAMMA) * (v_max - v_min) + v_min


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    x = (np.exp(detdata.normal("bench.it.image", SHAPE) * 0.8) * 90.0 - 40.0).astype(np.float32).reshape(-1)
    n = x.size
    xd = torch.from_numpy(x).cuda()
    y = torch.empty_like(xd)
    st = ops.stream()
    mm = torch.empty(4, dtype=torch.float32, device="cuda:0")
    mmws = torch.empty(4, dtype=torch.int32, device="cuda:0")
    selws = torch.empty(_lib.lib().fplx_select_ws_bytes() // 4, dtype=torch.int32, device="cuda:0")
    sel = torch.empty((3, 2), dtype=torch.float32, device="cuda:0")
    ranks = [ops.percentile_index(n, q)[0] for q in Q] + [n - 1]
    rk = (ctypes.c_int64 * 3)(*ranks)
    p, X, Y = lambda t: t.data_ptr(), xd.data_ptr(), y.data_ptr()

    def minmax():
        call("fplx_channel_minmax", X, n, 0.0, 0, 0.0, 0, p(mmws), 16, p(mm), st)

    def minmax_norm():
        minmax()
        call("fplx_clip_affine_dev", X, Y, n, p(mm), p(mm) + 4, p(mm), p(mm) + 4, st)

    def select():
        call("fplx_select_kth", X, n, rk, 3, p(sel), p(selws), selws.numel() * 4, st)

    def percentile_norm():
        v0, v1 = ops.percentiles(xd, list(Q))
        ops.clip_affine(xd, v0, v1, v0, v1 - v0, out=y)

    def gamma():
        minmax()
        call("fplx_gamma", X, Y, n, p(mm), p(mm) + 4, float(np.float32(GAMMA)), st)

    np.random.seed(1)
    noise = np.random.normal(MEAN, STD, x.shape)
    nd = torch.from_numpy(noise).cuda()

    def noise_f64():
        call("fplx_add_noise_f64", X, p(nd), Y, n, st)

    def noise_philox():
        call("fplx_add_noise_philox", X, Y, n, SEED, STREAM, MEAN, STD, 0, st)

    def copy():
        call("fplx_crop_flip", X, Y, 4, 1, SHAPE[0], SHAPE[1], SHAPE[2], 0, 0, 0, SHAPE[0], SHAPE[1], SHAPE[2], 0, st)

    copy_ms = event_ms(copy, a.iters)
    rows = []

    def row(name, once, ref, compare, iters=a.iters, **extra):
        ms = event_ms(once, iters)
        once()
        torch.cuda.synchronize()
        r = dict(name=name, device_ms=round(ms, 4), vs_copy=round(ms / copy_ms, 2))
        if ref is not None:
            want = ref()
            r["numpy_ms"] = round(wall_ms(ref, a.reps), 2)
            r["numpy_over_device"] = round(r["numpy_ms"] / ms, 1)
            r.update(compare(y.cpu().numpy(), want))
        r.update(extra)
        rows.append(r)
        print(json.dumps(r), flush=True)

    differ = lambda got, want: dict(differing_from_numpy=bits_differ(got, want))
    row("crop_flip (copy yardstick)", copy, None, None)
    row("channel_minmax (reduction alone)", minmax, None, None)
    row("min-max normalisation (reduction + apply)", minmax_norm, lambda: np_minmax(x), differ)
    row("select_kth, 3 ranks (selection alone)", select, None, None)
    s = np.sort(x)
    select()
    rows[-1]["differing_from_numpy_sort"] = bits_differ(sel.cpu().numpy(), [[s[k], s[min(k + 1, n - 1)]] for k in ranks])
    row("percentile normalisation (selection + host interpolation + apply)", percentile_norm, lambda: np_percentiles(x), differ,
        iters=max(a.iters // 5, 20))

    def gamma_cmp(got, want):
        u = IR.ulp_unit(x.min(), x.max())
        f64 = IR.gamma_f64(x, GAMMA)
        return dict(differing_from_numpy=bits_differ(got, want), share_differing=round(bits_differ(got, want) / float(n), 4),
                    device_max_ulp_from_f64=round(float(np.abs(got - f64).max() / u), 4),
                    numpy_max_ulp_from_f64=round(float(np.abs(want - f64).max() / u), 4))
    row("gamma (reduction + apply, fp64 pow)", gamma, lambda: np_gamma(x), gamma_cmp)
    row("noise, host draw: float64 add on the device", noise_f64, lambda: (x + noise).astype(np.float32), differ,
        host_draw_ms=round(wall_ms(lambda: np.random.normal(MEAN, STD, x.shape), a.reps), 2),
        upload_ms=round(wall_ms(lambda: (torch.from_numpy(noise).cuda(), torch.cuda.synchronize()), a.reps), 2))

    def philox_cmp(got, want):
        d = got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)
        return dict(differing_from_restatement=int((d != 0).sum()), max_ulp_from_restatement=int(np.abs(d).max()))
    row("noise, device Philox + Box-Muller (fp64)", noise_philox, lambda: IR.philox_noise(x, SEED, STREAM, MEAN, STD)[0],
        philox_cmp)
    res = dict(tool="tools/intensity_bench.py --iters %d --reps %d" % (a.iters, a.reps), device=torch.cuda.get_device_name(0),
               host_cpus=len(os.sched_getaffinity(0)), voxels=n,
               note="device_ms by HIP events over back-to-back calls after warm-up (the percentile row includes its device->host "
                    "copy and the host interpolation); numpy_ms by wall clock on the GPU machine's CPU (median); the numpy_ms "
                    "of the Philox row is the numpy restatement of the generator, not a reference pass", rows=rows)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
