"""Memory-footprint audit: which bytes does an entry point of the C ABI (include/fplx.h) touch?

Everything a case hands to the library lives in ONE byte buffer (Arena): every operand starts on a 256-byte boundary (plus
`misalign` elements), its last byte is followed at once - no rounding up - by a guard band, and guard bands and fresh outputs
hold a fill byte.  The wrappers of fplx.ops allocate their outputs and workspaces with torch.empty / torch.empty_like; for the
time of a case the name `torch` INSIDE fplx.ops is a stand-in whose empty / empty_like come from the arena (every other attribute
is torch's), and fplx.ops.call is a recorder that resolves every pointer argument, by the header's own `const`
(streamorder.parse_prototypes), to the arena tensor that contains it.  audit(case) runs the case under both fill bytes at two
placements and asserts:

  W  writes   no guard byte changes; a tensor reached only through `const` pointers (or not at all) keeps its bits
  R  reads    } the returned results are bit-identical under fill 0xFF and fill 0x5A: a load past an operand that reaches the
  U  uninit   } result, a workspace assumed to be zero and an output element that is never written all show here
  S  sizes    every `ws` / `part` argument is a tensor of exactly the documented number of bytes (Target.documented), and the
              ws_bytes argument next to it says the same
  A  align    for cases marked pointwise the results at misalign = 0 and misalign = 1 are bit-identical (a reduction may sum in
              another order on its scalar path; the value oracles bound both orders)
  plus        every pointer lies in an arena tensor ("unguarded operand") unless the case lists its parameter name, and every
              symbol the case lists was launched ("coverage")

Two blind spots, by construction.  An overrun of more than the guard band (64 KiB a side, four times the 16 KiB that 256 lanes
x 16 bytes x 4 loads in flight reach past an index) lands outside what the guards see.  A load past an operand whose value is
DISCARDED changes nothing that can be observed without provoking a fault, and is not looked for.
"""
import ctypes
import operator
import re

import numpy as np
import pytest
import torch

import streamorder

FILLS = (0xFF, 0x5A)
GUARD = 65536
ALIGN = 256

W_GUARD, W_CONST, READS, SIZES, ALIGNMENT, UNGUARDED, COVERAGE = "W:guard", "W:const", "R/U", "S", "A", "unguarded operand", "coverage"


class Finding(object):
    def __init__(self, prop, tensor, detail):
        self.prop, self.tensor, self.detail = prop, tensor, detail

    def __repr__(self):
        return "[%s] %s: %s" % (self.prop, self.tensor, self.detail)


class FootprintError(AssertionError):
    def __init__(self, case_id, findings):
        self.findings = list(findings)
        AssertionError.__init__(self, "%s: %d finding(s)\n  " % (case_id, len(self.findings)) + "\n  ".join(repr(f) for f in self.findings[:12]))

    def has(self, prop, tensor=None):
        return any(f.prop == prop and (tensor is None or f.tensor == tensor) for f in self.findings)


# ------------------------------------------------------------------------------------------------------------------ arena
class _Slot(object):
    """one placed tensor: bytes [start, end) of the arena; guards [pre, start) and [end, end + guard)"""

    def __init__(self, index, pre, start, end, post, name):
        self.index, self.pre, self.start, self.end, self.post, self.name = index, pre, start, end, post, name
        self.access = set()            # "r" / "w": how the recorded calls reached it
        self.bound = []                # (symbol, parameter) of every pointer that resolved to it
        self.origin = None             # the bytes copied in by place(); None: an empty() tensor, which held the fill byte

    def label(self):
        if self.name is not None:
            return self.name
        if self.bound:
            return self.bound[0][1]
        return "tensor#%d" % self.index


class Arena(object):
    """one byte buffer from torch, in a single allocation.  place() / empty() hand out contiguous views; nothing else of the
    buffer is ever written by the arena after construction, so every byte outside the views holds `fill`."""

    def __init__(self, device, fill, guard_bytes=GUARD, capacity=32 << 20):
        self.fill, self.guard, self.capacity = int(fill), int(guard_bytes), int(capacity)
        self.buf = torch.full((self.capacity,), self.fill, dtype=torch.uint8, device=device)
        self.base = self.buf.data_ptr()
        self.cursor = 0
        self.slots = []
        self.misalign_default = 0

    # ---- placing
    def _carve(self, shape, dtype, misalign, name):
        es = torch.empty((), dtype=dtype).element_size()
        n = 1
        for s in shape:
            n *= int(s)
        nbytes = n * es
        pre = self.cursor
        absolute = self.base + pre + self.guard
        absolute += (-absolute) % ALIGN
        start = absolute - self.base + int(misalign) * es
        end = start + nbytes
        post = end + self.guard
        if post > self.capacity:
            raise MemoryError("footprint arena: %d bytes asked, capacity %d" % (post, self.capacity))
        self.cursor = post
        slot = _Slot(len(self.slots), pre, start, end, post, name)
        self.slots.append(slot)
        view = self.buf[start:end].view(dtype).view(tuple(int(s) for s in shape))
        assert (n == 0 or view.data_ptr() == self.base + start) and view.is_contiguous()
        return view, slot

    def place(self, a, misalign=None, name=None):
        """copy an array or tensor in -> contiguous view of its dtype and shape, first byte on a 256-byte boundary plus
        `misalign` elements (None: the arena's default placement), the guard right behind its last byte"""
        t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
        view, slot = self._carve(t.shape, t.dtype, self.misalign_default if misalign is None else misalign, name)
        src = t.detach().cpu().contiguous()
        slot.origin = np.frombuffer(src.reshape(-1).view(torch.uint8).numpy().tobytes(), np.uint8) if src.numel() else np.zeros(0, np.uint8)
        view.copy_(src.to(self.buf.device))
        return view

    def empty(self, shape, dtype, misalign=None, name=None):
        """placed the same way; the tensor's own bytes hold the fill byte too"""
        if isinstance(shape, (int, np.integer)):
            shape = (int(shape),)
        view, _ = self._carve(tuple(shape), dtype, self.misalign_default if misalign is None else misalign, name)
        return view

    # ---- looking
    def find(self, addr):
        off = int(addr) - self.base
        for s in self.slots:
            if s.start <= off < s.end or (s.start == s.end == off):
                return s
        return None

    def slot_of(self, t):
        s = self.find(t.data_ptr())
        if s is None:
            raise KeyError("not an arena tensor")
        return s

    def host(self):
        if self.buf.is_cuda:
            torch.cuda.synchronize()
        return self.buf[:self.cursor].cpu().numpy()

    def check(self, host=None):
        """-> {slot index: byte offsets RELATIVE to the tensor's first byte at which a guard changed} (negative: in front of
        it; >= its size: behind it; at most the first 64 of either band); only tensors with a changed guard appear"""
        h = self.host() if host is None else host
        out = {}
        for s in self.slots:
            bad = []
            for lo, hi in ((s.pre, s.start), (s.end, s.post)):
                idx = np.nonzero(h[lo:hi] != self.fill)[0]
                bad.extend((idx[:64] + lo - s.start).tolist())
            if bad:
                out[s.index] = bad
        return out

    def snapshot(self):
        return self.host().copy()

    def rewritten(self, after=None, const_only=False):
        """-> {slot index: the first byte offsets (at most 64) inside the tensor that differ from what place() copied in
        (empty(): from the fill)}; const_only: tensors a recorded call reached through a non-const pointer are left out"""
        h = self.host() if after is None else after
        out = {}
        for s in self.slots:
            if const_only and "w" in s.access:
                continue
            now = h[s.start:s.end]
            idx = np.nonzero(now != (self.fill if s.origin is None else s.origin))[0]
            if len(idx):
                out[s.index] = idx[:64].tolist()
        return out

    def changed(self, before, after=None):
        """-> {slot index: byte offsets inside the tensor that differ from `before`}; a tensor placed after the snapshot
        was taken is compared with the fill byte it held"""
        h = self.host() if after is None else after
        out = {}
        for s in self.slots:
            now = h[s.start:s.end]
            if s.end <= len(before):
                was = before[s.start:s.end]
            else:
                was = np.full(s.end - s.start, self.fill, np.uint8)
            idx = np.nonzero(now != was)[0]
            if len(idx):
                out[s.index] = idx.tolist()
        return out


# ------------------------------------------------------------------------------------------- the stand-in and the recorder
class TorchStandIn(object):
    """stands where a wrapper module has `torch`: empty and empty_like come from the arena, everything else is torch's"""

    def __init__(self, arena):
        self._arena = arena

    def __getattr__(self, k):
        return getattr(torch, k)

    def empty(self, *size, **kw):
        dtype = kw.pop("dtype", None) or torch.get_default_dtype()
        kw.pop("device", None)
        assert not kw, "footprint stand-in: torch.empty(%s) is not modelled" % ", ".join(kw)
        if len(size) == 1 and not isinstance(size[0], (int, np.integer)):
            size = tuple(size[0])
        return self._arena.empty(size, dtype)

    def empty_like(self, t, dtype=None, device=None):
        return self._arena.empty(tuple(t.shape), dtype or t.dtype)


def param_name(decl):
    return re.findall(r"\w+", decl)[-1]


class Target(object):
    """what is audited: a module whose functions reach the library through its attributes `torch` and `call`, the prototypes of
    the entry points, and the documented sizes: {(symbol, parameter): f(args by parameter name) -> bytes} for every `ws` /
    `part` parameter of an audited symbol"""

    def __init__(self, module, protos, documented, device):
        self.module, self.protos, self.documented, self.device = module, protos, documented, device


SIZED = ("ws", "part")


class Recorder(object):
    def __init__(self, arena, target, unguarded):
        self.arena, self.target, self.unguarded = arena, target, set(unguarded)
        self.real = target.module.call
        self.seen, self.findings = [], []

    def _resolve(self, sym, pname, addr, mode):
        s = self.arena.find(addr)
        if s is None:
            if pname not in self.unguarded:
                self.findings.append(Finding(UNGUARDED, pname, "%s(%s) = %#x lies in no arena tensor" % (sym, pname, addr)))
            return None
        s.access.add(mode)
        s.bound.append((sym, pname))
        return s

    def __call__(self, name, *args):
        kinds = self.target.protos[name]
        assert len(kinds) == len(args), (name, len(kinds), len(args))
        self.seen.append(name)
        named, slots = {}, {}
        for (kind, decl), a in zip(kinds, args):
            pn = param_name(decl)
            named[pn] = getattr(a, "value", a) if isinstance(a, ctypes._SimpleCData) else a
            if kind in (streamorder.SCALAR, streamorder.STREAM) or a is None:
                continue
            if kind in (streamorder.READ, streamorder.READWRITE):
                if isinstance(a, ctypes.Array) or type(a).__name__ == "CArgObject":
                    continue                                  # a ctypes host array of scalars, or a byref
                if isinstance(a, ctypes._SimpleCData):
                    a = a.value
                a = operator.index(a or 0)
                if a == 0:
                    continue
                mode = "r" if kind == streamorder.READ else "w"
                slots[pn] = self._resolve(name, pn, a, mode)
            else:                                             # a table of pointers: the table itself, then each entry
                mode = "r" if kind == streamorder.TABLE_READ else "w"
                if not isinstance(a, ctypes.Array):
                    self._resolve(name, pn, operator.index(getattr(a, "value", a) or 0), "r")
                    continue
                for v in a:
                    if v:
                        self._resolve(name, pn, int(v), mode)
        for pn in SIZED:                                      # S
            if pn not in named or not named[pn]:
                continue
            doc = self.target.documented.get((name, pn))
            if doc is None:
                self.findings.append(Finding(SIZES, pn, "%s(%s): no documented size in the table" % (name, pn)))
                continue
            want = int(doc(named))
            s = slots.get(pn)
            if s is not None and s.end - s.start != want:
                self.findings.append(Finding(SIZES, pn, "%s(%s) has %d bytes, documented %d" % (name, pn, s.end - s.start, want)))
            if pn == "ws" and "ws_bytes" in named and int(named["ws_bytes"]) != want:
                self.findings.append(Finding(SIZES, pn, "%s: ws_bytes = %d, documented %d" % (name, int(named["ws_bytes"]), want)))
        return self.real(name, *args)


# ------------------------------------------------------------------------------------------------------------- the audit
class Case(object):
    """id; symbols the case must launch; run(P) -> results, P(array, aligned=False, name=None, misalign=None) places an input
    (aligned: an operand the header requires to be aligned - it keeps misalign = 0; misalign: that many elements off at both
    placements) and P.empty(shape, dtype, ...) an output or workspace the case hands in itself; pointwise: data movement or element-wise arithmetic (property A);
    unguarded: parameter names whose pointers a wrapper builds outside the arena (small host-built tables)"""

    def __init__(self, id, symbols, run, pointwise=False, unguarded=()):
        self.id, self.symbols, self.run, self.pointwise, self.unguarded = id, tuple(symbols), run, pointwise, tuple(unguarded)

    def __repr__(self):
        return self.id


class Placer(object):
    def __init__(self, arena, misalign):
        self.arena, self.misalign = arena, misalign

    def __call__(self, a, aligned=False, name=None, misalign=None):
        return self.arena.place(a, self._mis(aligned, misalign), name)

    def empty(self, shape, dtype, aligned=False, name=None, misalign=None):
        return self.arena.empty(shape, dtype, self._mis(aligned, misalign), name)

    def _mis(self, aligned, misalign):
        """aligned: stays on the 256-byte boundary at every placement; misalign = k: k elements off at EVERY placement"""
        return 0 if aligned else (self.misalign if misalign is None else int(misalign))


def _flatten(res, out, path="result"):
    if res is None:
        return
    if torch.is_tensor(res):
        out.append((path, res.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes() if res.numel() else b""))
    elif isinstance(res, np.ndarray):
        out.append((path, np.ascontiguousarray(res).tobytes()))
    elif isinstance(res, dict):
        for k in sorted(res):
            _flatten(res[k], out, "%s[%r]" % (path, k))
    elif isinstance(res, (list, tuple)):
        for i, r in enumerate(res):
            _flatten(r, out, "%s[%d]" % (path, i))
    else:
        out.append((path, np.asarray(res).tobytes()))


def audit(case, target, capacity=32 << 20):
    findings, results = [], {}
    for mis in (0, 1):
        for fill in FILLS:
            flat, found = _run_with_const_check(case, target, fill, mis, capacity)
            tag = "misalign=%d fill=%#x: " % (mis, fill)
            for f in found:
                f.detail = tag + f.detail
            findings.extend(found)
            results[(mis, fill)] = flat
    for mis in (0, 1):                                        # R / U
        a, b = results[(mis, FILLS[0])], results[(mis, FILLS[1])]
        findings.extend(_compare(a, b, READS, "misalign=%d: differs between fill %#x and fill %#x" % (mis, FILLS[0], FILLS[1])))
    if case.pointwise:                                        # A
        findings.extend(_compare(results[(0, FILLS[0])], results[(1, FILLS[0])], ALIGNMENT, "differs between misalign 0 and 1"))
    if findings:
        raise FootprintError(case.id, findings)


def _compare(a, b, prop, what):
    out = []
    if [p for p, _ in a] != [p for p, _ in b]:
        return [Finding(prop, "result", what + " (the results have another structure)")]
    for (p, x), (_, y) in zip(a, b):
        if x != y:
            n = min(len(x), len(y))
            first = next((i for i in range(n) if x[i] != y[i]), n)
            out.append(Finding(prop, p, "%s, first at byte %d of %d" % (what, first, len(x))))
    return out


def _run_with_const_check(case, target, fill, misalign, capacity):
    """one run of the case in a fresh arena -> (flattened results, findings): S and the unguarded operands from the recorder,
    both halves of W, coverage.  The const half compares every tensor that no call reached through a non-const pointer with
    what place() copied into it (an empty() tensor: with the fill); the wrappers' own torch calls only ever write tensors
    they made themselves, outside the arena."""
    arena = Arena(target.device, fill, capacity=capacity)
    arena.misalign_default = misalign
    rec = Recorder(arena, target, case.unguarded)
    real = rec.real
    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(target.module, "torch", TorchStandIn(arena))
        mp.setattr(target.module, "call", rec)
        res = case.run(Placer(arena, misalign))
        flat = []
        _flatten(res, flat)
    finally:
        mp.undo()
    assert target.module.call is real
    after = arena.host()
    found = list(rec.findings)
    for idx, offs in sorted(arena.check(after).items()):
        s = arena.slots[idx]
        found.append(Finding(W_GUARD, s.label(), "guard bytes changed at offsets %s relative to the tensor (%d bytes; bound to %s)" % (
            offs[:8], s.end - s.start, s.bound[:2])))
    for idx, offs in sorted(arena.rewritten(after, const_only=True).items()):
        s = arena.slots[idx]
        found.append(Finding(W_CONST, s.label(), "reached only through const pointers (%s), yet bytes %s changed" % (s.bound[:2], offs[:8])))
    missing = sorted(set(case.symbols) - set(rec.seen))
    if missing:
        found.append(Finding(COVERAGE, ", ".join(missing), "listed by the case, never launched (launched: %s)" % sorted(set(rec.seen))))
    return flat, found
