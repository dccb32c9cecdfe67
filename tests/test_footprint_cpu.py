"""The footprint checker (tests/footprint.py) held to known answers, without a GPU: an arena on the CPU and fake "wrappers"
written in torch and numpy that reach fake "kernels" (numpy on raw addresses) through the same stand-in for `torch` and the
same recording `call` as fplx.ops does.  One wrapper is correct; every other one carries exactly one defect, which must be
reported under the right property and for the right tensor.  The completeness test holds the audit's case table
(test_gpu_footprint.AUDITED) and COVERED_ELSEWHERE against every pointer-taking prototype of include/fplx.h."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import footprint as fp
import streamorder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fplx.h")

FAKE_HEADER = """
int fplx_fake_scale(const float* x, float* y, int64_t n, float a, int defect, fplx_stream_t stream);
int fplx_fake_copy8(const uint8_t* in, uint8_t* out, int64_t n, int defect, fplx_stream_t stream);
int fplx_fake_sum(const float* x, int64_t n, int rows, float* part, double* out, int defect, fplx_stream_t stream);
int fplx_fake_never(const float* x, fplx_stream_t stream);
"""
ROW = 8                      # elements a partial row of fplx_fake_sum covers


def _f32(addr, n):
    return np.ctypeslib.as_array((ctypes.c_float * n).from_address(addr))


def _u8(addr, n):
    return np.ctypeslib.as_array((ctypes.c_uint8 * n).from_address(addr))


def _f64(addr, n):
    return np.ctypeslib.as_array((ctypes.c_double * n).from_address(addr))


def k_scale(x, y, n, a, defect, stream):
    X, Y = _f32(x, n + 1), _f32(y - 4, n + 2)[1:]            # Y[-1] is not reachable through a slice: see "before"
    m = n - 1 if defect == "unwritten" else n
    Y[:m] = np.float32(a) * X[:m]
    if defect == "past":
        Y[n] = 0.0
    if defect == "before":
        _f32(y - 4, 1)[0] = 0.0
    if defect == "const":
        X[0] = X[0] + np.float32(1)
    if defect == "align" and x % 256:
        Y[0] += np.float32(1)
    if defect == "discarded":
        _ = float(X[n])                                       # a load of the guard whose value goes nowhere


def k_copy8(src, dst, n, defect, stream):
    if defect == "tail":                                     # whole 16-byte stores; the lanes past n hold zero
        m = (n + 15) // 16 * 16
        v = np.zeros(m, np.uint8)
        v[:n] = _u8(src, n)
        _u8(dst, m)[:] = v
    else:
        _u8(dst, n)[:] = _u8(src, n)


def k_sum(x, n, rows, part, out, defect, stream):
    m = n + 1 if defect == "load" else n
    X = _f32(x, m)
    P = _f32(part, (rows + 1) * 1)
    for r in range(rows):
        P[r] = X[r * ROW:min((r + 1) * ROW, m)].sum(dtype=np.float32)
    if defect == "load" and m > rows * ROW:
        P[rows - 1] += X[m - 1]
    if defect in ("row", "row_wrapper"):
        P[rows] = 0.0                                        # a spare row behind the documented ones
    O = _f64(out, 1)
    if defect != "accumulate":
        O[0] = 0.0
    O[0] += P[:rows].astype(np.float64).sum()


KERNELS = {"fplx_fake_scale": k_scale, "fplx_fake_copy8": k_copy8, "fplx_fake_sum": k_sum}


def fake_call(name, *args):
    KERNELS[name](*args)


fake = types.SimpleNamespace(torch=torch, call=fake_call)     # the module the audit patches: `torch` and `call` are looked up here


def scale(x, a, defect=None, foreign_out=False):
    y = torch.zeros(x.shape, dtype=torch.float32) if foreign_out else fake.torch.empty_like(x)
    fake.call("fplx_fake_scale", x.data_ptr(), y.data_ptr(), x.numel(), float(a), defect, 0)
    return y


def copy8(x, defect=None):
    y = fake.torch.empty(x.numel(), dtype=torch.uint8, device=x.device)
    fake.call("fplx_fake_copy8", x.data_ptr(), y.data_ptr(), x.numel(), defect, 0)
    return y


def rows_of(n):
    return (n + ROW - 1) // ROW


def total(x, defect=None):
    rows = rows_of(x.numel())
    part = fake.torch.empty((rows + (1 if defect == "row_wrapper" else 0),), dtype=torch.float32)
    out = fake.torch.empty(1, dtype=torch.float64)
    fake.call("fplx_fake_sum", x.data_ptr(), x.numel(), rows, part.data_ptr(), out.data_ptr(), defect, 0)
    return out


@pytest.fixture(scope="module")
def target(tmp_path_factory):
    h = tmp_path_factory.mktemp("fake") / "fake.h"
    h.write_text(FAKE_HEADER)
    protos = streamorder.parse_prototypes(str(h))
    documented = {("fplx_fake_sum", "part"): lambda a: a["rows"] * 4}
    return fp.Target(fake, protos, documented, "cpu")


X = (np.arange(29, dtype=np.float32) - 7) / 4
B = (np.arange(29) * 7 % 251).astype(np.uint8)
CAP = 2 << 20


def _audit(target, run, symbols, pointwise=False, unguarded=()):
    fp.audit(fp.Case("fake", symbols, run, pointwise=pointwise, unguarded=unguarded), target, capacity=CAP)


def _rejects(target, run, symbols, prop, tensor, pointwise=False):
    with pytest.raises(fp.FootprintError) as e:
        _audit(target, run, symbols, pointwise)
    assert e.value.has(prop, tensor), e.value
    return e.value


def test_the_correct_wrappers_pass(target):
    _audit(target, lambda P: scale(P(X), 3.0), ["fplx_fake_scale"], pointwise=True)
    _audit(target, lambda P: copy8(P(B)), ["fplx_fake_copy8"], pointwise=True)
    _audit(target, lambda P: total(P(X)), ["fplx_fake_sum"])
    _audit(target, lambda P: (scale(P(X), 3.0), total(P(X)), scale(P(X[:5]), 2.0)), ["fplx_fake_scale", "fplx_fake_sum"])  # placed between calls
    assert fake.torch is torch and fake.call is fake_call     # the patches are gone


def test_a_store_one_element_past_an_output(target):
    e = _rejects(target, lambda P: scale(P(X), 3.0, "past"), ["fplx_fake_scale"], fp.W_GUARD, "y")
    assert not e.has(fp.READS) and not e.has(fp.W_CONST)


def test_a_store_one_element_before_an_output(target):
    e = _rejects(target, lambda P: scale(P(X), 3.0, "before"), ["fplx_fake_scale"], fp.W_GUARD, "y")
    assert any(f.prop == fp.W_GUARD and "[-4, -3, -2, -1]" in f.detail for f in e.findings), e


def test_a_16_byte_store_over_a_13_byte_tail(target):
    e = _rejects(target, lambda P: copy8(P(B), "tail"), ["fplx_fake_copy8"], fp.W_GUARD, "out")
    assert any("[29, 30, 31]" in f.detail for f in e.findings), e


def test_a_load_of_the_guard_that_reaches_the_result(target):
    e = _rejects(target, lambda P: total(P(X), "load"), ["fplx_fake_sum"], fp.READS, "result")
    assert not e.has(fp.W_GUARD)


def test_a_discarded_load_of_the_guard_passes(target):
    """the stated blind spot: nothing observable changes"""
    _audit(target, lambda P: scale(P(X), 3.0, "discarded"), ["fplx_fake_scale"], pointwise=True)


def test_an_accumulator_that_is_not_zeroed(target):
    _rejects(target, lambda P: total(P(X), "accumulate"), ["fplx_fake_sum"], fp.READS, "result")


def test_an_output_element_that_is_never_written(target):
    e = _rejects(target, lambda P: scale(P(X), 3.0, "unwritten"), ["fplx_fake_scale"], fp.READS, "result")
    assert any(f.prop == fp.READS and "first at byte 112 of 116" in f.detail for f in e.findings), e


def test_a_workspace_one_row_beyond_its_declared_size(target):
    e = _rejects(target, lambda P: total(P(X), "row_wrapper"), ["fplx_fake_sum"], fp.SIZES, "part")      # the wrapper makes room for it
    assert not e.has(fp.W_GUARD)
    e = _rejects(target, lambda P: total(P(X), "row"), ["fplx_fake_sum"], fp.W_GUARD, "part")            # the kernel just takes it
    assert not e.has(fp.SIZES)


def test_a_write_through_a_const_operand(target):
    _rejects(target, lambda P: scale(P(X), 3.0, "const"), ["fplx_fake_scale"], fp.W_CONST, "x")


def test_a_pointwise_result_that_changes_with_alignment(target):
    e = _rejects(target, lambda P: scale(P(X), 3.0, "align"), ["fplx_fake_scale"], fp.ALIGNMENT, "result", pointwise=True)
    assert not e.has(fp.READS)
    _audit(target, lambda P: scale(P(X), 3.0, "align"), ["fplx_fake_scale"], pointwise=False)         # not asserted for a reduction


def test_an_operand_that_did_not_come_from_the_arena(target):
    _rejects(target, lambda P: scale(P(X), 3.0, foreign_out=True), ["fplx_fake_scale"], fp.UNGUARDED, "y")
    _audit(target, lambda P: scale(P(X), 3.0, foreign_out=True), ["fplx_fake_scale"], unguarded=("y",))   # listed by parameter name


def test_a_listed_symbol_that_is_never_launched(target):
    _rejects(target, lambda P: scale(P(X), 3.0), ["fplx_fake_scale", "fplx_fake_never"], fp.COVERAGE, "fplx_fake_never")


def test_a_missing_documented_size_is_a_finding(target):
    t2 = fp.Target(fake, target.protos, {}, "cpu")
    with pytest.raises(fp.FootprintError) as e:
        fp.audit(fp.Case("fake", ["fplx_fake_sum"], lambda P: total(P(X))), t2, capacity=CAP)
    assert e.value.has(fp.SIZES, "part")


# ---------------------------------------------------------------------------------------------------------------- the arena
def test_arena_placement():
    a = fp.Arena("cpu", 0x5A, capacity=CAP)
    for mis, dt in ((0, np.float32), (1, np.float32), (1, np.uint8), (1, np.float64), (3, np.int32)):
        arr = np.arange(13).astype(dt)
        t = a.place(arr, misalign=mis)
        assert (t.data_ptr() - mis * arr.itemsize) % 256 == 0 and t.is_contiguous()
        assert np.array_equal(t.numpy(), arr)
        s = a.slot_of(t)
        assert s.end - s.start == arr.nbytes and s.start - s.pre >= fp.GUARD and s.post - s.end == fp.GUARD
    e = a.empty((3, 5), torch.float32)
    assert e.view(torch.uint8).eq(0x5A).all() and tuple(e.shape) == (3, 5)
    assert a.check() == {} and a.changed(a.snapshot()) == {}
    snap = a.snapshot()
    s = a.slot_of(e)
    a.buf[s.end] = 0                                           # the byte right behind the last one: no rounding up
    a.buf[s.start - 1] = 0
    e[0, 0] = 1.0
    assert a.check() == {s.index: [-1, 60]}
    assert sorted(a.changed(snap)) == [s.index]


def test_the_stand_in_hands_out_arena_memory_and_is_torch_otherwise():
    a = fp.Arena("cpu", 0xFF, capacity=CAP)
    t = fp.TorchStandIn(a)
    assert t.float32 is torch.float32 and t.tensor is torch.tensor and t.is_tensor(t.empty(3))
    for made in (t.empty(3, dtype=torch.int32), t.empty((2, 3), dtype=torch.float64, device="cpu"), t.empty_like(torch.zeros(4, 2))):
        assert a.find(made.data_ptr()) is not None
    assert a.find(t.zeros(3).data_ptr()) is None


# ---------------------------------------------------------------------------------------------------------------- completeness
def test_every_pointer_taking_prototype_is_accounted_for():
    import test_gpu_footprint as G
    protos = streamorder.parse_prototypes(HEADER)
    pointer = {k for k, v in protos.items() if any(c not in (streamorder.SCALAR, streamorder.STREAM) for c, _ in v)}
    audited = set(G.AUDITED)
    elsewhere = set(G.COVERED_ELSEWHERE)
    assert not (audited & elsewhere), sorted(audited & elsewhere)
    assert not (pointer - audited - elsewhere), "in neither table: %s" % sorted(pointer - audited - elsewhere)
    assert not ((audited | elsewhere) - pointer), "no such prototype: %s" % sorted((audited | elsewhere) - pointer)
    listed = {s for c in G.CASES for s in c.symbols}
    assert listed == audited                                   # AUDITED is what the cases list, and coverage holds them to it
    for sym, (path, mention) in sorted(G.COVERED_ELSEWHERE.items()):
        text = open(os.path.join(ROOT, path)).read()
        assert mention in text, "%s does not mention %s (for %s)" % (path, mention, sym)
    for (sym, pn) in G.DOCUMENTED:
        assert sym in audited and pn in [fp.param_name(d) for _, d in protos[sym]], (sym, pn)
    for sym in sorted(audited):                                # every ws / part of an audited symbol has a documented size
        for kind, decl in protos[sym]:
            if fp.param_name(decl) in fp.SIZED:
                assert (sym, fp.param_name(decl)) in G.DOCUMENTED, (sym, decl)
