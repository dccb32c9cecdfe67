"""Host dispatch plan of the convolution paths, recorded from the commit BEFORE the dispatch refactor.

    python tests/golden/make_golden_dispatch.py <checkout of PARENT, built with `make -C fpl-plus_amd/csrc`>

writes tests/golden/dispatch_plan.json.  Run it against a build of PARENT, never against the tree under test: the
fixture pins what the dispatch answered before it was rewritten as one plan per path.  It stores the rows at the shipped
knobs in full and, for every other knob setting, only the cells that differ (expand() rebuilds every row).  Every value is an integer a host
query of the public ABI (include/fplx.h) returns - no GPU is needed.  tests/test_host_cpu.py replays GRID under every
setting of KNOBS against the built library and requires equality of every integer.

The settings march=0 and brick=0,march=0 were recorded again from a build of 348c0c2, the commit before the slab-stream forward
(plan kernel 3) was removed, with that kernel's minimum-width knob of that commit at 1 << 30 besides: it then accepts no layer and
the layers fall through to the next entry of fwd_plan's order, which is the plan without that kernel.  Only grid points whose
plan kernel was 3 changed (27 and 33 points; 159 and 177 cells differ in all), and under march=0 six of the 159 are
conv2d_stats_rows at other points (volumes 0, 5 and 10 at 64 -> 64 | 128): the 3D plan there is the brick kernel, which has no
Conv2d form, so the 2.5D plan had been kernel 3 too.  Every other line of the fixture is the first recording's.
"""
import ctypes
import json
import os
import sys

PARENT = "6d2c953"
VOLUMES = [(2, 80, 160, 160), (2, 40, 80, 80), (2, 20, 40, 40), (2, 10, 20, 20), (2, 5, 10, 10), (8, 28, 128, 128),
           (8, 28, 64, 64), (8, 14, 32, 32), (8, 7, 16, 16), (8, 7, 8, 8), (1, 48, 160, 272), (1, 4, 16, 64), (1, 4, 8, 64),
           (1, 3, 16, 64), (2, 8, 8, 8), (1, 6, 24, 72), (1, 5, 12, 20), (3, 9, 17, 33), (1, 16, 16, 16), (1, 8, 40, 96)]
CHANNELS = [(16, 32), (32, 32), (64, 32), (32, 64), (64, 64), (128, 64), (64, 128), (128, 128), (256, 128), (256, 256),
            (256, 512), (512, 512), (512, 256), (48, 48), (96, 64), (32, 96)]
# each applied over the shipped defaults
KNOBS = [{}, {"brick": 0}, {"brick": 3}, {"march": 0}, {"brick": 0, "march": 0}, {"mid_tile": 0}, {"wg_roll": 0},
         {"wg_roll2d": 0}, {"wg_vox": 0}, {"wg_vox": 2}, {"tile_ks": 9}, {"rows_small_div": 64}, {"brick_geo": 1, "brick_ksplit": 2},
         {"march128": 0}, {"march32_v2": 0}, {"march64_fw": 16}]
STEM_CIN, OUT_CLASSES = 1, 2            # the stem reads in_chns = 1, the out_conv writes two classes
COLUMNS = ["plan.kernel", "plan.geometry", "plan.ksplit", "plan.stats_rows", "conv3d_stats_rows", "conv3d_fwd_ws_bytes",
           "conv2d_stats_rows", "conv2d_fwd_ws_bytes", "conv3d_wgrad_ws_bytes.333", "conv3d_wgrad_ws_bytes.133",
           "conv3d_wgrad_ws_bytes.111", "conv2d_wgrad_ws_bytes", "conv3d_cat2_ok", "fwd_act_ok.mid0.cat0", "fwd_act_ok.mid0.cat1",
           "fwd_act_ok.mid1.cat0", "fwd_act_ok.mid1.cat1", "deconv2_wgrad_ws_bytes", "deconv122_wgrad_ws_bytes",
           "outconv_bn_rows", "outconv_wgrad_bn_ws_bytes", "stem.kernel", "stem.geometry", "stem.ksplit", "stem.stats_rows",
           "outconv.kernel", "outconv.geometry", "outconv.ksplit", "outconv.stats_rows"]
F32, BF16 = 0, 1


def knob_key(kn):
    return ",".join("%s=%d" % kv for kv in kn.items())


def grid():
    return [v + c for v in VOLUMES for c in CHANNELS]


def query_row(lib, n, d, h, w, ci, co):
    """every recorded integer of one (volume, channel pair), in COLUMNS order"""
    def plan(ci_, co_, kd, xdt, ydt):
        o = [ctypes.c_int() for _ in range(4)]
        rc = lib.fplx_conv3d_plan_query(n, d, h, w, ci_, co_, kd, 3, 3, xdt, ydt, *[ctypes.byref(x) for x in o])
        assert rc == 0, rc
        return [x.value for x in o]

    s = (n, d, h, w, ci, co)
    return (plan(ci, co, 3, BF16, BF16) +
            [lib.fplx_conv3d_stats_rows(*s, 3, 3, 3, BF16, BF16), lib.fplx_conv3d_fwd_ws_bytes(*s, 3, 3, 3, BF16, BF16),
             lib.fplx_conv2d_stats_rows(*s, BF16, BF16), lib.fplx_conv2d_fwd_ws_bytes(*s, BF16, BF16),
             lib.fplx_conv3d_wgrad_ws_bytes(*s, 3, 3, 3), lib.fplx_conv3d_wgrad_ws_bytes(*s, 1, 3, 3),
             lib.fplx_conv3d_wgrad_ws_bytes(*s, 1, 1, 1), lib.fplx_conv2d_wgrad_ws_bytes(*s), lib.fplx_conv3d_cat2_ok(*s)] +
            [lib.fplx_conv3d_fwd_act_ok(*s, mid, cat2) for mid in (0, 1) for cat2 in (0, 1)] +
            [lib.fplx_deconv2_wgrad_ws_bytes(*s), lib.fplx_deconv122_wgrad_ws_bytes(*s),
             lib.fplx_outconv_bn_rows(n, d, h, w, ci, OUT_CLASSES), lib.fplx_outconv_wgrad_bn_ws_bytes(n, d, h, w, ci, OUT_CLASSES)] +
            plan(STEM_CIN, co, 3, F32, BF16) + plan(ci, OUT_CLASSES, 1, BF16, F32))


def replay(_lib):
    """{knob setting: [row of integers per grid point]} from the library _lib has loaded; every knob it touches is put back
    to the value fplx_get_tuning gave before the change"""
    lib, out = _lib.lib(), {}
    for kn in KNOBS:
        before = {k: _lib.get_tuning(k) for k in kn}
        try:
            for k, v in kn.items():
                _lib.set_tuning(k, v)
            out[knob_key(kn)] = [query_row(lib, *g) for g in grid()]
        finally:
            for k, v in before.items():
                _lib.set_tuning(k, v)
    return out


def expand(doc):
    """{knob setting: [row per grid point]} from the fixture: the rows at the shipped defaults, and for every other knob
    setting the cells that differ from them (changes[knobs][column][grid index] = value)"""
    col = {c: i for i, c in enumerate(doc["columns"])}
    out = {}
    for kn in doc["knobs"]:
        rows = [list(r) for r in doc["default"]]
        for c, cells in doc["changes"].get(kn, {}).items():
            for i, v in cells.items():
                rows[int(i)][col[c]] = v
        out[kn] = rows
    return out


if __name__ == "__main__":
    parent = os.path.abspath(sys.argv[1])
    sys.path.insert(0, os.path.join(parent, "fpl-plus_amd"))
    from fplx import _lib
    assert os.path.dirname(os.path.dirname(_lib.LIB_PATH)) == os.path.join(parent, "fpl-plus_amd"), _lib.LIB_PATH
    got = replay(_lib)
    base, changes = got[""], {}
    for kn, rows in got.items():
        for c, name in enumerate(COLUMNS):
            cells = {str(i): r[c] for i, (r, b) in enumerate(zip(rows, base)) if r[c] != b[c]}
            if cells:
                changes.setdefault(kn, {})[name] = cells
    dumps = lambda o: json.dumps(o, separators=(",", ":"))
    head = {"_comment": "host dispatch plan recorded from a build of commit %s (tests/golden/make_golden_dispatch.py).  default[i] "
                        "holds `columns` for grid point i = volumes x channels (channels fastest) at the shipped knobs; "
                        "changes[knobs][column][i] the cells that differ under another setting of `knobs` (every other cell "
                        "equals default).  stem.* is the plan query fp32 -> bf16 3x3x3 with cin = %d, outconv.* the plan query "
                        "bf16 -> fp32 1x3x3 with cout = %d, outconv_* take (c0 = cin, classes = %d)" % (
                            PARENT, STEM_CIN, OUT_CLASSES, OUT_CLASSES),
            "parent": PARENT, "volumes": VOLUMES, "channels": CHANNELS, "knobs": [knob_key(k) for k in KNOBS], "columns": COLUMNS}
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dispatch_plan.json")
    with open(dst, "w") as f:           # one line per grid point and per (knob setting, column): a diff of the fixture reads
        f.write("{" + ",\n".join("%s:%s" % (dumps(k), dumps(v)) for k, v in head.items()))
        f.write(",\n\"default\":[\n" + ",\n".join(dumps(r) for r in base) + "],\n\"changes\":{\n")
        f.write(",\n".join("%s:{\n%s}" % (dumps(kn), ",\n".join(" %s:%s" % (dumps(c), dumps(v)) for c, v in cols.items()))
                           for kn, cols in changes.items()) + "}}\n")
    doc = json.load(open(dst))
    assert expand(doc) == got
    print(dst, os.path.getsize(dst), "bytes,", sum(len(v) for v in got.values()), "rows")
