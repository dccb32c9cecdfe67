"""The happens-before checker (tests/streamorder.py) against schedules with known answers, the header's read / write
classification, and the torch-op recorder on CPU tensors.  Host code only."""
import itertools
import os
import re

import pytest
import torch

import streamorder as S
from streamorder import launch, record, wait, sync, sync_all, sync_event, region

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fplx.h")
MAIN, SIDE, THIRD = 0, 0x7f00dead0000, 0x7f00beef0000
A, B = region(0x10000, 1, 4096), region(0x20000, 1, 4096)


def kinds(trace):
    return sorted((c.kind, c.first_name, c.second_name) for c in S.check(trace))


# ------------------------------------------------------------------------------------------------------------- regions
def _bytes(r):
    return {r[0] + i * r[3] + j for i in range(r[1]) for j in range(r[2])}


def test_overlap_is_never_under_reported_and_exact_where_promised():
    """every pair of a small family of regions against the byte sets themselves: a shared byte is always reported; equal
    pitch, and an interval against anything, are decided exactly"""
    fam = []
    for base, rows, w, pitch in itertools.product((0, 3, 8, 13, 24), (1, 2, 3), (1, 4, 8), (8, 12)):
        r = region(100 + base, rows, w, pitch)
        if r is not None and r not in fam:
            fam.append(r)
    exact = loose = 0
    for a, b in itertools.product(fam, fam):
        truth = bool(_bytes(a) & _bytes(b))
        got = S.overlap(a, b)
        assert got or not truth, (a, b)
        if a[1] == 1 or b[1] == 1 or a[3] == b[3]:
            assert got == truth, (a, b)
            exact += 1
        else:
            loose += got != truth
    assert exact > 1000 and loose > 0          # the family holds pairs of unequal pitch that only the bounds decide


def test_degenerate_regions_become_their_bounding_interval():
    assert region(0, 0, 8, 8) is None and region(0, 4, 0, 8) is None
    assert region(64, 4, 8, 8) == (64, 1, 32, 32)
    assert region(64, 4, 8, 0) == (64, 1, 8, 8)               # a broadcast row
    assert region(64, 3, 8, 4) == (64, 1, 16, 16)             # rows that overlap each other
    assert S.bounds(region(64, 3, 8, 32)) == (64, 64 + 2 * 32 + 8)


def test_column_slices_of_one_pitched_buffer():
    V, C, es = 50, 16, 2
    base, pitch = 0x40000, 2 * C * es
    skip, up = region(base, V, C * es, pitch), region(base + C * es, V, C * es, pitch)
    assert not S.overlap(skip, up) and not S.overlap(up, skip)
    both = [launch(MAIN, "dgrad", [], [skip]), launch(SIDE, "wgrad", [up], [])]
    assert S.check(both) == []
    wide = region(base + (C - 1) * es, V, C * es, pitch)      # columns C-1 .. 2C-2: one column of skip, all but one of up
    assert S.overlap(wide, skip) and S.overlap(wide, up)
    lower_rows = region(base + 10 * pitch + (C - 1) * es, 5, C * es, pitch)
    assert S.overlap(lower_rows, skip)
    assert kinds([launch(MAIN, "dgrad", [], [skip]), launch(SIDE, "wgrad", [lower_rows], [])]) == [("RAW", "dgrad", "wgrad")]
    past_rows = region(base + V * pitch + (C - 1) * es, 5, C * es, pitch)
    assert not S.overlap(past_rows, skip)
    # an interval inside the gap between two rows of a slice touches nothing; one byte further it does
    assert not S.overlap(region(base + C * es, 1, C * es), skip)
    assert S.overlap(region(base + C * es, 1, C * es + 1), skip)


# ------------------------------------------------------------------------------------------------------------ schedules
def test_missing_wait_is_a_raw():
    t = [launch(MAIN, "producer", [], [A]), launch(SIDE, "consumer", [A], [B])]
    assert kinds(t) == [("RAW", "producer", "consumer")]
    c = S.check(t)[0]
    assert (c.first_pos, c.second_pos, c.first_stream, c.second_stream) == (0, 1, MAIN, SIDE)
    ok = [launch(MAIN, "producer", [], [A]), record("e", MAIN), wait(SIDE, "e"), launch(SIDE, "consumer", [A], [B])]
    assert S.check(ok) == []


def test_in_place_overwrite_under_a_side_stream_reader_is_a_war():
    t = [launch(MAIN, "bn_bwd", [A], [A]), record("e", MAIN), wait(SIDE, "e"), launch(SIDE, "wgrad", [A], [B]),
         launch(MAIN, "next_bn_bwd", [A], [A])]
    assert kinds(t) == [("WAR", "wgrad", "next_bn_bwd")]
    t2 = t[:4] + [record("j", SIDE), wait(MAIN, "j"), t[4]]
    assert S.check(t2) == []


def test_two_writers_are_a_waw():
    t = [launch(MAIN, "zero", [], [A]), launch(SIDE, "wgrad", [B], [A])]
    assert kinds(t) == [("WAW", "zero", "wgrad")]


def test_an_event_recorded_before_the_producer_orders_nothing_after_it():
    t = [record("e", MAIN), launch(MAIN, "producer", [], [A]), wait(SIDE, "e"), launch(SIDE, "consumer", [A], [])]
    assert kinds(t) == [("RAW", "producer", "consumer")]
    # ... and a wait on an event that was never recorded is a no-op
    assert kinds([launch(MAIN, "producer", [], [A]), wait(SIDE, "never"), launch(SIDE, "consumer", [A], [])]) == \
        [("RAW", "producer", "consumer")]
    # re-recording moves the event: the second position is the one a later wait takes
    t3 = [record("e", MAIN), launch(MAIN, "producer", [], [A]), record("e", MAIN), wait(SIDE, "e"),
          launch(SIDE, "consumer", [A], [])]
    assert S.check(t3) == []


def test_order_through_a_third_stream():
    t = [launch(MAIN, "producer", [], [A]), record("e1", MAIN), wait(THIRD, "e1"), launch(THIRD, "relay", [], [B]),
         record("e2", THIRD), wait(SIDE, "e2"), launch(SIDE, "consumer", [A], [])]
    assert S.check(t) == []
    assert kinds(S.without(t, 2)) == [("RAW", "producer", "consumer")]      # the chain broken at its first link


def test_address_reuse_without_a_join():
    """what the caching allocator does once a tensor the side stream still reads is let go: the next allocation of the main
    stream gets the same block"""
    t = [launch(MAIN, "dgrad", [], [A]), record("e", MAIN), wait(SIDE, "e"), launch(SIDE, "wgrad", [A], [B]),
         launch(MAIN, "next_dgrad_in_the_same_block", [], [A])]
    assert kinds(t) == [("WAR", "wgrad", "next_dgrad_in_the_same_block")]
    part = region(A[0] + 512, 1, 256)                          # a smaller tensor inside the freed block
    assert kinds(t[:4] + [launch(MAIN, "small", [], [part])]) == [("WAR", "wgrad", "small")]


def test_host_synchronisation_is_a_barrier():
    head = [launch(SIDE, "wgrad", [A], [B])]
    tail = [launch(MAIN, "optimiser", [B], [A])]
    assert kinds(head + tail) == [("RAW", "wgrad", "optimiser"), ("WAR", "wgrad", "optimiser")]
    assert S.check(head + [sync_all()] + tail) == []
    assert S.check(head + [sync(SIDE)] + tail) == []
    assert len(S.check(head + [sync(MAIN)] + tail)) == 2      # the wrong stream
    assert len(S.check(head + [sync(THIRD)] + tail)) == 2
    assert S.check(head + [record("e", SIDE), sync_event("e")] + tail) == []
    assert len(S.check([record("e", SIDE)] + head + [sync_event("e")] + tail)) == 2
    # a barrier orders what came before it only
    assert len(S.check([sync_all()] + head + tail)) == 2


def test_no_implicit_order_with_the_default_stream():
    assert len(S.check([launch(0, "on_default", [], [A]), launch(SIDE, "on_pool_stream", [A], [])])) == 1
    assert len(S.check([launch(SIDE, "on_pool_stream", [], [A]), launch(0, "on_default", [A], [])])) == 1


def _collective(reg, cur):
    """the records Tracer.collective / collective_wait write (the contract of torch's NCCL / RCCL process group)"""
    return [record("to", cur), wait(S.COMM, "to"), launch(S.COMM, "all_reduce", [reg], [reg])]


def test_the_collective_model():
    g = region(0x80000, 1, 1 << 16)
    bucket = region(0x80000, 1, 1 << 12)
    later = region(0x80000 + (1 << 12), 1, 1 << 12)
    fold = launch(SIDE, "fold", [bucket, B], [bucket])
    base = [launch(MAIN, "bn_grads", [], [bucket]), record("e", MAIN), wait(SIDE, "e"), launch(SIDE, "wgrad", [], [bucket]), fold]
    coll = _collective(bucket, SIDE)
    done = [record("from", S.COMM), wait(MAIN, "from")]
    opt = [launch(MAIN, "adam", [g], [A])]
    join = [record("j", SIDE), wait(MAIN, "j")]
    # the main stream goes on writing LATER ranges while the bucket travels: clean; the optimiser behind work.wait(): clean
    ok = base + coll + [launch(MAIN, "later_grads", [], [later])] + join + done + opt
    assert S.check(ok) == []
    # no work.wait(): the optimiser reads what the collective still writes
    assert ("RAW", "all_reduce", "adam") in kinds(base + coll + join + opt)
    # the collective launched from the MAIN stream without the side stream's weight gradients: they race
    bad = base + _collective(bucket, MAIN)
    assert ("WAW", "wgrad", "all_reduce") in kinds(bad) and ("WAW", "fold", "all_reduce") in kinds(bad)
    # the main stream writing INTO the travelling bucket
    assert ("WAW", "all_reduce", "late_write") in kinds(base + coll + [launch(MAIN, "late_write", [], [bucket])])
    # work.wait() orders the waiting stream only
    assert ("RAW", "all_reduce", "reader") in kinds(base + coll + done + [launch(THIRD, "reader", [bucket], [])])


def test_removing_each_wait_of_a_minimal_two_stream_backward():
    d_out, gw, ws = region(0x1000, 1, 256), region(0x2000, 1, 256), region(0x3000, 1, 256)
    t = [launch(MAIN, "zero", [], [gw]), launch(MAIN, "bn_bwd", [d_out], [d_out]), record("e", MAIN), wait(SIDE, "e"),
         launch(SIDE, "wgrad", [d_out], [gw, ws]), record("j", SIDE), wait(MAIN, "j"), launch(MAIN, "adam", [gw], [])]
    assert S.check(t) == []
    ws_ = S.waits(t)
    assert ws_ == [3, 6]
    assert S.describe_wait(t, 3) == (SIDE, "wgrad", MAIN, "bn_bwd")
    assert S.describe_wait(t, 6) == (MAIN, "adam", SIDE, "wgrad")
    assert {c.kind for c in S.check(S.without(t, 3))} == {"RAW", "WAW"}
    assert kinds(S.without(t, 6)) == [("RAW", "wgrad", "adam")]
    assert S.streams_of(t) == [MAIN, SIDE]


def test_removing_every_wait_in_one_pass_equals_removing_each():
    g, bucket = region(0x80000, 1, 1 << 16), region(0x80000, 1, 1 << 12)
    t = []
    for it in range(2):
        t += [launch(MAIN, "zero", [], [g]), launch(MAIN, "bn_grads", [], [bucket]), record(("e", it), MAIN), wait(SIDE, ("e", it)),
              launch(SIDE, "wgrad", [A], [bucket]), record(("r", it), MAIN), wait(SIDE, ("r", it)), launch(SIDE, "fold", [bucket, B], [bucket]),
              record(("to", it), SIDE), wait(S.COMM, ("to", it)), launch(S.COMM, "all_reduce", [bucket], [bucket]),
              record(("j", it), SIDE), wait(MAIN, ("j", it)), record(("from", it), S.COMM), wait(MAIN, ("from", it)),
              launch(MAIN, "adam", [g], [A])]
    assert S.check(t) == []
    each = S.check_each_wait_removed(t)
    assert sorted(each) == S.waits(t) and len(each) == 10
    for pos, got in each.items():
        want = S.check(S.without(t, pos))
        assert [(c.kind, c.first_name, c.second_name) for c in got] == [(c.kind, c.first_name, c.second_name) for c in want]
        assert [(c.first_pos, c.second_pos) for c in got] == [(c.first_pos + (c.first_pos >= pos), c.second_pos + (c.second_pos >= pos))
                                                              for c in want]
    needed = sorted(p for p, c in each.items() if c)
    assert [t[p][2][0] for p in needed] == ["e", "to", "from", "e", "to", "from"]      # ready()'s edge and the join are covered twice


def test_unknown_record_is_refused():
    with pytest.raises(ValueError):
        S.check([("barrier",)])


# ------------------------------------------------------------------------------------------------- the header's classes
TABLE_FUNCTIONS = {
    "fplx_pack_conv_weights_batched": {"w": S.TABLE_READ, "wf": S.TABLE_WRITE, "wb": S.TABLE_WRITE, "stamp": S.TABLE_WRITE},
    "fplx_pack_weights_multi": {"w": S.TABLE_READ, "wf": S.TABLE_WRITE, "wb": S.TABLE_WRITE},
    "fplx_adam_pack_step": {"wf": S.TABLE_WRITE, "wb": S.TABLE_WRITE, "stamp": S.TABLE_WRITE},
    "fplx_optim_pack_step": {"wf": S.TABLE_WRITE, "wb": S.TABLE_WRITE, "stamp": S.TABLE_WRITE},
    "fplx_ssl_pyramid_fwd": {"logits": S.TABLE_READ},
    "fplx_ssl_pyramid_bwd": {"logits": S.TABLE_READ, "dlogits": S.TABLE_WRITE},
    "fplx_ssl_pseudo_onehot": {"logits": S.TABLE_READ, "onehot": S.TABLE_WRITE},
    "fplx_nll_voxel_ce_fwd": {"logits": S.TABLE_READ, "loss": S.TABLE_WRITE},
    "fplx_nll_select_fwd": {"loss": S.TABLE_READ, "mask": S.TABLE_READ},
    "fplx_nll_select_bwd": {"logits": S.TABLE_READ, "mask": S.TABLE_READ, "dlogits": S.TABLE_WRITE},
}


def test_param_classes():
    assert S.classify_param("int n") == S.SCALAR
    assert S.classify_param("int64_t  voxels_per_sample") == S.SCALAR
    assert S.classify_param("fplx_stream_t stream") == S.STREAM
    assert S.classify_param("const float* w") == S.READ
    assert S.classify_param("const void *x") == S.READ
    assert S.classify_param("void* wf") == S.READWRITE
    assert S.classify_param("float *part") == S.READWRITE
    assert S.classify_param("const float* const* w") == S.TABLE_READ
    assert S.classify_param("const uint8_t * const * mask") == S.TABLE_READ
    assert S.classify_param("void* const* wf") == S.TABLE_WRITE
    for bad in ("float** p", "const float** p", "float* const* const* p", "float (*f)(int)"):
        with pytest.raises(ValueError):
            S.classify_param(bad)


def test_header_classification_agrees_with_the_ctypes_binding_and_finds_every_table():
    from fplx import _lib
    protos = S.parse_prototypes(HEADER)
    bound = _lib.parse_header(HEADER)
    assert sorted(protos) == sorted(bound) and len(protos) >= 150
    for name, params in protos.items():
        assert len(params) == len(bound[name][1]), name
        classes = [k for k, _ in params]
        has_ptr = any(k not in (S.SCALAR, S.STREAM) for k in classes)
        if has_ptr and S.STREAM in classes:
            assert classes.count(S.STREAM) == 1, name
            assert classes[-1] == S.STREAM, name              # the convention the wrappers rely on
    # every launch the engine's schedules make takes a stream
    for name in ("fplx_conv3d_fwd", "fplx_conv3d_wgrad", "fplx_conv2d_wgrad", "fplx_conv3d_wgrad_cat2", "fplx_deconv2_wgrad",
                 "fplx_stem_wgrad_bn", "fplx_outconv_wgrad_bn", "fplx_bn_act_bwd_apply", "fplx_optim_step", "fplx_optim_pack_step"):
        assert [k for k, _ in protos[name]].count(S.STREAM) == 1, name
    # the pointer tables: what the classification finds is what the raw text of the header holds, and is the known list
    src = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    raw = {}
    for m in re.finditer(r"\b(fplx_\w+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        n = len(re.findall(r"\*\s*const\s*\*|\*\s*\*", m.group(2)))
        if n:
            raw[m.group(1)] = n
    found = {name: {d.split("*")[-1].strip(): k for k, d in params if k in (S.TABLE_READ, S.TABLE_WRITE)}
             for name, params in protos.items()}
    found = {k: v for k, v in found.items() if v}
    assert {k: len(v) for k, v in found.items()} == raw
    assert found == TABLE_FUNCTIONS


def test_const_is_kept_where_the_binding_drops_it():
    protos = S.parse_prototypes(HEADER)
    p = dict((d.split("*")[-1].split()[-1], k) for k, d in protos["fplx_optim_step"])
    assert (p["p"], p["g"], p["s0"], p["s1"], p["hp"], p["n"], p["stream"]) == \
        (S.READWRITE, S.READ, S.READWRITE, S.READWRITE, S.READ, S.SCALAR, S.STREAM)
    w = dict((d.split("*")[-1].split()[-1], k) for k, d in protos["fplx_conv3d_wgrad"])
    assert (w["x"], w["dy"], w["dw"], w["db"], w["ws"]) == (S.READ, S.READ, S.READWRITE, S.READWRITE, S.READWRITE)


def test_every_launch_of_the_package_goes_through_the_one_choke_point():
    """the tracer patches fplx._lib.call: an entry point reached as lib().fplx_x(...) instead would not be recorded - every
    such call in the package is a host-only query (no stream parameter)"""
    import glob
    protos = S.parse_prototypes(HEADER)
    pkg = os.path.join(os.path.dirname(HEADER), os.pardir, "fpl-plus_amd", "fplx")
    direct = set()
    for path in glob.glob(os.path.join(pkg, "*.py")):
        direct |= set(re.findall(r"lib\(\)\.(fplx_\w+)\(", open(path).read()))
    assert len(direct) >= 20 and direct <= set(protos)
    launching = sorted(n for n in direct if S.STREAM in [k for k, _ in protos[n]])
    assert launching == [], launching


# --------------------------------------------------------------------------------- the torch-op recorder, on CPU tensors
class _CpuTracer(S.Tracer):
    """the recorder with the device taken out: every tensor counts, everything is on stream 0"""

    def __init__(self):
        super(_CpuTracer, self).__init__()
        self._torch = torch

    def _cur(self):
        return 0


def _record(fn):
    tr = _CpuTracer()
    with pytest.MonkeyPatch().context() as mp:
        mp.setattr(S, "_is_device_tensor", lambda t: True)
        with S._make_mode(tr):
            fn()
    return tr.trace


def test_torch_ops_are_read_from_their_schemas():
    g, acc = torch.zeros(64), torch.ones(64)
    r = lambda t: S.tensor_region(t)
    tr = _record(lambda: g[8:24].add_(acc[8:24]))
    assert [x[2] for x in tr] == ["aten::add_"]               # the two slices are views: no launch
    assert tr[0][3] == (r(g[8:24]), r(acc[8:24])) and tr[0][4] == (r(g[8:24]),)
    tr = _record(lambda: g.zero_())
    assert tr[0][2] == "aten::zero_" and tr[0][4] == (r(g),)
    out = []
    tr = _record(lambda: out.append(g.clone()))
    assert tr[-1][2] == "aten::clone" and tr[-1][3] == (r(g),) and tr[-1][4] == (r(out[0]),)
    tr = _record(lambda: acc.copy_(g))
    assert tr[0][3] == (r(acc), r(g)) and tr[0][4] == (r(acc),)
    tr = _record(lambda: torch.add(g, acc, out=out[0]))
    assert tr[0][2] == "aten::add" and r(out[0]) in tr[0][4] and r(g) in tr[0][3]
    assert _record(lambda: torch.empty(16)) == [] and _record(lambda: g.view(8, 8)[:, 2:4].t()) == []
    buf = torch.zeros(10, 16)
    tr = _record(lambda: buf[:, 4:8].mul_(2.0))
    assert tr[0][4] == (region(buf.data_ptr() + 16, 10, 16, 64),)
    tr = _record(lambda: out.append(float(g.sum())))
    assert [x[0] for x in tr[-2:]] == ["launch", "sync"] and tr[-2][2] == "aten::_local_scalar_dense"
