"""Stream-order audit: a happens-before checker over a recorded launch schedule, the read / write classification of the C
ABI (include/fplx.h) and the tracer that records a schedule while it runs.

The checker is host code over plain integers.  A trace is a list of records (the constructors below):

    launch(stream, name, reads, writes)     one kernel (or copy) enqueued on `stream`; reads / writes are lists of regions
    record(event, stream)                   the event takes the stream's position
    wait(stream, event)                     the stream waits for the position the event holds (a never-recorded event: no-op)
    sync(stream) / sync_all()               the HOST waits for one stream / for every stream: everything enqueued afterwards,
                                            on any stream, follows what that stream (every stream) held
    sync_event(event)                       the host waits for an event (Event.synchronize)

A region is (base address, rows, row bytes, pitch bytes): `rows` runs of `row bytes` bytes, `pitch bytes` apart.
Streams and events are any hashable names; no stream is special: the default stream (0) is ordered against a
torch.cuda.Stream by events only, as on the device (torch's pool streams are non-blocking).

Model: one vector clock per stream and one for the host.  clock[s][t] = how many launches of stream t are known to precede
the next launch of s.  An event carries a copy of the recording stream's clock, a wait joins it.  Launch a precedes launch b
iff they are on one stream (trace order) or b's clock at its launch holds a's sequence number.  check() returns every
pair of launches on different streams that share a byte, at least one writing, that neither order covers.

What is assumed, and said again in DESIGN.md: the header's `const` is truthful (a `const T*` is only read, a `T*` may be
both), a pointer the tracer never saw a tensor for spans the whole allocator block that holds it, and the collective
follows the contract of torch's NCCL / RCCL process group (below, at _DistShim).
"""
import collections
import ctypes
import operator
import re
import sys
import threading

# ----------------------------------------------------------------------------------------------------------------- regions


def region(base, rows=1, row_bytes=0, pitch=None):
    """normal form of a region, or None for an empty one.  Anything that is not `rows` disjoint runs in ascending order
    (pitch < row bytes, pitch <= 0) becomes its bounding interval: never smaller than the bytes it stands for."""
    base, rows, row_bytes = int(base), int(rows), int(row_bytes)
    pitch = row_bytes if pitch is None else int(pitch)
    if rows <= 0 or row_bytes <= 0:
        return None
    if rows == 1 or pitch == row_bytes:
        return (base, 1, rows * row_bytes, rows * row_bytes)
    if pitch < row_bytes:
        lo = min(base, base + (rows - 1) * pitch)
        hi = max(base, base + (rows - 1) * pitch) + row_bytes
        return (lo, 1, hi - lo, hi - lo)
    return (base, rows, row_bytes, pitch)


def bounds(r):
    return r[0], r[0] + (r[1] - 1) * r[3] + r[2]


def _ranges_meet(a0, a1, b0, b1):
    return max(a0, b0) < min(a1, b1)


def overlap(a, b):
    """do two normal-form regions share a byte?  Exact for two intervals, an interval against a pitched region and two
    regions of one pitch (column slices of one [V, ld] buffer, at any row offset); everything else is decided on the
    bounding intervals, which can only say 'yes' too often."""
    la, ha = bounds(a)
    lb, hb = bounds(b)
    if not _ranges_meet(la, ha, lb, hb):
        return False
    if a[1] == 1 and b[1] == 1:
        return True
    if a[1] == 1 or b[1] == 1:
        c, p = (a, b) if a[1] == 1 else (b, a)
        c0 = c[0] - p[0]
        c1 = c0 + c[2]
        rows, w, pitch = p[1], p[2], p[3]
        i = 0 if c0 < w else (c0 - w) // pitch + 1            # first row that ends behind c0
        return i < rows and i * pitch < c1
    if a[3] != b[3]:
        return True
    pitch = a[3]
    q, r = divmod(b[0] - a[0], pitch)                         # b's row j starts in a's row q + j, r bytes in
    if r < a[2] and _ranges_meet(q, q + b[1], 0, a[1]):
        return True
    if r + b[2] > pitch and _ranges_meet(q + 1, q + 1 + b[1], 0, a[1]):   # b's rows run over into the next row of a
        return True
    return False


# ------------------------------------------------------------------------------------------------------------------ traces
def launch(stream, name, reads=(), writes=()):
    return ("launch", stream, name, tuple(r for r in reads if r is not None), tuple(w for w in writes if w is not None))


def record(event, stream):
    return ("record", event, stream)


def wait(stream, event):
    return ("wait", stream, event)


def sync(stream):
    return ("sync", stream)


def sync_all():
    return ("sync_all",)


def sync_event(event):
    return ("sync_event", event)


Conflict = collections.namedtuple("Conflict", "kind first_pos first_name first_stream second_pos second_name second_stream")


def _join(into, other):
    for k, v in other.items():
        if into.get(k, 0) < v:
            into[k] = v


def _hull(regs):
    lo = hi = None
    for r in regs:
        a, b = bounds(r)
        lo = a if lo is None or a < lo else lo
        hi = b if hi is None or b > hi else hi
    return lo, hi


def _any_overlap(xs, ys):
    for x in xs:
        for y in ys:
            if overlap(x, y):
                return True
    return False


class _Run(object):
    """the checker's state: clocks of the streams and of the host, the events' clocks, the launches so far per stream"""

    def __init__(self):
        self.clocks, self.events, self.host = {}, {}, {}
        self.per_stream = {}                                  # stream -> [(seq, pos, name, reads, writes, hull)]
        self.out = []

    def fork(self):
        """a copy that can go on by itself (event clocks and launch tuples are never changed once stored)"""
        r = _Run()
        r.clocks = {s: dict(c) for s, c in self.clocks.items()}
        r.events, r.host = dict(self.events), dict(self.host)
        r.per_stream = {s: list(v) for s, v in self.per_stream.items()}
        r.out = list(self.out)
        return r

    def clk(self, s):
        c = self.clocks.setdefault(s, {})
        self.per_stream.setdefault(s, [])
        _join(c, self.host)
        return c

    def step(self, pos, rec):
        kind = rec[0]
        if kind == "launch":
            _, s, name, reads, writes = rec
            c = self.clk(s)
            lo, hi = _hull(reads + writes)
            if lo is not None:
                for t, items in self.per_stream.items():
                    if t == s:
                        continue
                    known = c.get(t, 0)
                    for seq, p2, n2, r2, w2, (lo2, hi2) in reversed(items):
                        if seq <= known:
                            break
                        if lo2 is None or not _ranges_meet(lo, hi, lo2, hi2):
                            continue
                        if w2 and reads and _any_overlap(w2, reads):
                            self.out.append(Conflict("RAW", p2, n2, t, pos, name, s))
                        if r2 and writes and _any_overlap(r2, writes):
                            self.out.append(Conflict("WAR", p2, n2, t, pos, name, s))
                        if w2 and writes and _any_overlap(w2, writes):
                            self.out.append(Conflict("WAW", p2, n2, t, pos, name, s))
            c[s] = c.get(s, 0) + 1
            self.per_stream[s].append((c[s], pos, name, reads, writes, (lo, hi)))
        elif kind == "record":
            self.events[rec[1]] = dict(self.clk(rec[2]))
        elif kind == "wait":
            c = self.clk(rec[1])
            if rec[2] in self.events:
                _join(c, self.events[rec[2]])
        elif kind == "sync":
            _join(self.host, self.clk(rec[1]))
        elif kind == "sync_all":
            for s in list(self.clocks):
                _join(self.host, self.clk(s))
        elif kind == "sync_event":
            if rec[1] in self.events:
                _join(self.host, self.events[rec[1]])
        else:
            raise ValueError("unknown trace record %r" % (rec,))

    def result(self):
        return sorted(self.out, key=lambda c: (c.second_pos, c.first_pos, c.kind))


def check(trace):
    """-> [Conflict]: kind RAW / WAR / WAW as seen from the launch that comes first in the trace (RAW: it writes what the
    later one reads), both names, both positions in the trace."""
    run = _Run()
    for pos, rec in enumerate(trace):
        run.step(pos, rec)
    return run.result()


def check_each_wait_removed(trace):
    """-> {position of a wait: check() of the trace without that wait}, the positions in the conflicts being those of the
    FULL trace.  The records in front of the wait are gone through once for all of them."""
    run, res = _Run(), {}
    for pos, rec in enumerate(trace):
        if rec[0] == "wait":
            alt = run.fork()
            for p2 in range(pos + 1, len(trace)):
                alt.step(p2, trace[p2])
            res[pos] = alt.result()
        run.step(pos, rec)
    return res


def waits(trace):
    """positions of the wait records"""
    return [i for i, r in enumerate(trace) if r[0] == "wait"]


def without(trace, pos):
    return trace[:pos] + trace[pos + 1:]


def describe_wait(trace, pos):
    """(waiting stream, name of the next launch on it, recording stream, name of the last launch in front of the record)"""
    _, s, ev = trace[pos]
    nxt = next((r[2] for r in trace[pos + 1:] if r[0] == "launch" and r[1] == s), None)
    src, prev = None, None
    for i in range(pos - 1, -1, -1):
        r = trace[i]
        if r[0] == "record" and r[1] == ev:
            src = r[2]
            prev = next((q[2] for q in reversed(trace[:i]) if q[0] == "launch" and q[1] == src), None)
            break
    return s, nxt, src, prev


def streams_of(trace):
    return sorted({r[1] for r in trace if r[0] == "launch"}, key=str)


# --------------------------------------------------------------------------------------------- the header's classification
SCALAR, STREAM, READ, READWRITE, TABLE_READ, TABLE_WRITE = "scalar", "stream", "read", "readwrite", "table_read", "table_write"
_TYPE = r"(const\s+)?\w+(\s+\w+)*?"
_TABLE = re.compile(r"^" + _TYPE + r"\s*\*\s*const\s*\*\s*\w*$")
_POINTER = re.compile(r"^" + _TYPE + r"\s*\*\s*\w*$")


def classify_param(decl):
    d = " ".join(decl.split())
    if "fplx_stream_t" in d:
        return STREAM
    stars = d.count("*")
    if stars == 0:
        return SCALAR
    if stars == 1 and _POINTER.match(d):
        return READ if d.startswith("const ") else READWRITE
    if stars == 2 and _TABLE.match(d):
        return TABLE_READ if d.startswith("const ") else TABLE_WRITE
    raise ValueError("include/fplx.h: parameter %r is no scalar, stream, pointer or pointer table" % d)


def parse_prototypes(path):
    """-> {function: [(class, declaration)]} for every prototype of the header, `const` kept (fplx._lib.parse_header
    drops it: ctypes has no use for it)"""
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"^\s*#.*$", " ", src, flags=re.M)
    out = {}
    for m in re.finditer(r"\b(int|size_t)\s+(fplx_\w+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        args = m.group(3).strip()
        params = []
        if args and args != "void":
            params = [(classify_param(a), " ".join(a.split())) for a in args.split(",")]
        out[m.group(2)] = params
    return out


# ------------------------------------------------------------------------------------------------------------- the tracer
COMM = "comm"


def _is_device_tensor(t):
    return t.is_cuda


def tensor_region(t):
    """the bytes a tensor view covers: exact for contiguous tensors and for 2-D views with unit column stride (a channel
    slice of a [V, ld] buffer); the bounding interval otherwise"""
    if t.numel() == 0:
        return None
    es, base = t.element_size(), t.data_ptr()
    if t.is_contiguous():
        return region(base, 1, t.numel() * es)
    if t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1]:
        return region(base, t.shape[0], t.shape[1] * es, t.stride(0) * es)
    lo = sum((n - 1) * s for n, s in zip(t.shape, t.stride()) if s < 0)
    hi = sum((n - 1) * s for n, s in zip(t.shape, t.stride()) if s > 0) + 1
    return region(base + lo * es, 1, (hi - lo) * es)


class Tracer(object):
    """with Tracer(...) as tr: ... -> tr.trace.  Holds no tensor: every extent is turned into integers at once (a kept
    reference would change which blocks the caching allocator hands out again, and hide exactly the hazard looked for).

    library launches   fplx._lib.call and every name it was imported under; the stream is the call's fplx_stream_t
                       argument, reads / writes follow the header; extents from the tensors the patched ops.ptr saw while
                       the call's arguments were formed, else the allocator block around the pointer
    torch's kernels    a TorchDispatchMode; writes are the op schema's write annotations plus fresh outputs; view ops
                       (outputs that alias without writing) and the empty* family launch nothing
    events             Event.record / wait / synchronize, Stream.wait_event / wait_stream / synchronize, cuda.synchronize
    collective         fplx.ddp's `dist` is replaced by _DistShim for the time of the trace
    delay = (which, cycles, main stream): enqueue torch.cuda._sleep(cycles) in front of every library launch on the main
    stream (which = "main") or on any other (which = "side") while self.delay_on is true; self.delays counts them."""

    def __init__(self, torch_ops=True, events=True, collective=True, delay=None):
        self.trace = []
        self.want_torch, self.want_events, self.want_coll = torch_ops, events, collective
        self.delay, self.delay_on, self.delays = delay, False, 0
        self._seen = {}
        self._events = {}
        self._fresh = 0
        self._snap_key, self._blocks = None, []
        self._tl = threading.local()
        self.block_resolved = 0

    # ---- patching
    def __enter__(self):
        import pytest
        import torch
        import fplx
        from fplx import _lib, ops, ddp
        self._mp = mp = pytest.MonkeyPatch()
        self._torch = torch
        self.protos = parse_prototypes(_lib.HEADER)
        real_call, real_ptr = _lib.call, ops.ptr
        tracer = self

        def call(name, *args):
            tracer._library_launch(name, args)
            real_call(name, *args)

        def ptr(t):
            if t is not None and t.is_cuda:
                tracer._saw(t)
            return real_ptr(t)

        for mod in list(sys.modules.values()):
            if getattr(mod, "__name__", "").split(".")[0] != "fplx":
                continue
            if getattr(mod, "call", None) is real_call:
                mp.setattr(mod, "call", call)
            if getattr(mod, "ptr", None) is real_ptr:
                mp.setattr(mod, "ptr", ptr)
        if self.want_coll:
            mp.setattr(ddp, "dist", _DistShim(ddp.dist, self))
        if self.want_events:
            self._patch_events(mp, torch)
        self._mode = None
        if self.want_torch:
            self._mode = _make_mode(self)
            self._mode.__enter__()
        return self

    def __exit__(self, *exc):
        if self._mode is not None:
            self._mode.__exit__(*exc)
        self._mp.undo()
        self._events.clear()
        return False

    # ---- streams and events
    def _cur(self):
        return int(self._torch.cuda.current_stream().cuda_stream)

    def _eid(self, ev):
        self._events[id(ev)] = ev           # an event is no tensor; kept so that its id is not handed out again
        return id(ev)

    def _outer(self):
        """true for the outermost patched event method (Stream.wait_stream is wait_event(record_event()) inside torch)"""
        return getattr(self._tl, "depth", 0) == 0

    def _patch_events(self, mp, torch):
        tracer, tl = self, self._tl
        Ev, St = torch.cuda.Event, torch.cuda.Stream

        def wrap(cls, name, note):
            real = getattr(cls, name)

            def method(self, *a, **k):
                if tracer._outer():
                    note(self, *a, **k)
                tl.depth = getattr(tl, "depth", 0) + 1
                try:
                    return real(self, *a, **k)
                finally:
                    tl.depth -= 1
            mp.setattr(cls, name, method)

        def sid(s):
            return tracer._cur() if s is None else int(s.cuda_stream)

        def wait_stream(self, other):
            tracer._fresh += 1
            ev = ("wait_stream", tracer._fresh)
            tracer.trace.append(record(ev, sid(other)))
            tracer.trace.append(wait(sid(self), ev))

        wrap(Ev, "record", lambda self, stream=None: tracer.trace.append(record(tracer._eid(self), sid(stream))))
        wrap(Ev, "wait", lambda self, stream=None: tracer.trace.append(wait(sid(stream), tracer._eid(self))))
        wrap(Ev, "synchronize", lambda self: tracer.trace.append(sync_event(tracer._eid(self))))
        wrap(St, "wait_event", lambda self, event: tracer.trace.append(wait(sid(self), tracer._eid(event))))
        wrap(St, "wait_stream", wait_stream)
        wrap(St, "synchronize", lambda self: tracer.trace.append(sync(sid(self))))
        real_sync = torch.cuda.synchronize

        def synchronize(device=None):
            tracer.trace.append(sync_all())
            return real_sync(device)
        mp.setattr(torch.cuda, "synchronize", synchronize)

    # ---- extents
    def _saw(self, t):
        r = tensor_region(t)
        if r is None:
            return
        a = t.data_ptr()
        old = self._seen.get(a)
        if old is not None and old != r:                      # two views at one address in one call: their hull
            lo = min(bounds(old)[0], bounds(r)[0])
            hi = max(bounds(old)[1], bounds(r)[1])
            r = region(lo, 1, hi - lo)
        self._seen[a] = r

    def _allocated_blocks(self):
        torch = self._torch
        st = torch.cuda.memory_stats()
        key = (st.get("allocation.all.allocated", 0), st.get("allocation.all.freed", 0))
        if key != self._snap_key:
            blocks = []
            for seg in torch.cuda.memory_snapshot():
                a = seg["address"]
                for b in seg["blocks"]:
                    addr = b.get("address", a)
                    if b["state"] == "active_allocated":
                        blocks.append((addr, b["size"]))
                    a = addr + b["size"]
            self._snap_key, self._blocks = key, blocks
        return self._blocks

    def _resolve(self, addr, what):
        r = self._seen.get(addr)
        if r is not None:
            return r
        for a, n in self._allocated_blocks():
            if a <= addr < a + n:
                self.block_resolved += 1
                return region(a, 1, n)
        raise AssertionError("%s: device pointer %#x lies in no allocated block of the caching allocator" % (what, addr))

    # ---- launches
    def _library_launch(self, name, args):
        kinds = self.protos[name]
        assert len(kinds) == len(args), (name, len(kinds), len(args))
        stream, reads, writes = None, [], []
        for i, ((kind, decl), a) in enumerate(zip(kinds, args)):
            if kind == STREAM:
                stream = int(getattr(a, "value", a) or 0)
                continue
            if kind == SCALAR or a is None:
                continue
            what = "%s(%s)" % (name, decl)
            if kind in (READ, READWRITE):
                if isinstance(a, ctypes.Array) or type(a).__name__ == "CArgObject":
                    continue                                  # a ctypes host array of scalars (hp, cout, off, ...) or a byref
                if isinstance(a, ctypes._SimpleCData):
                    a = a.value
                a = operator.index(a or 0)                    # anything else that is no integer is an error, not a skip
                if a == 0:
                    continue
                r = self._resolve(a, what)
                reads.append(r)
                if kind == READWRITE:
                    writes.append(r)
            else:                                             # a host table of device pointers
                for v in a:
                    if v:
                        r = self._resolve(int(v), what)
                        (writes if kind == TABLE_WRITE else reads).append(r)
        self._seen.clear()
        if stream is None:
            return                                            # a host-only entry point (plan queries, tuning knobs)
        if self.delay is not None and self.delay_on:
            which, cycles, main = self.delay
            if (stream == main) == (which == "main"):
                self._torch.cuda._sleep(int(cycles))          # goes to the current stream: the one the launch is made on
                self.delays += 1
        self.trace.append(launch(stream, name, reads, writes))

    def _torch_op(self, func, args, kwargs, out):
        torch = self._torch
        schema = func._schema
        name = schema.name
        rets = schema.returns
        if any(r.alias_info is not None and not r.alias_info.is_write for r in rets):
            return                                            # a view: no kernel
        short = name.split("::")[-1]
        if short.startswith(("empty", "new_empty", "_empty")):
            return

        def tensors(v):
            if isinstance(v, torch.Tensor):
                return [v] if _is_device_tensor(v) else []
            if isinstance(v, (list, tuple)):
                return [t for x in v for t in tensors(x)]
            return []

        reads, writes, given = [], [], set()
        for i, sa in enumerate(schema.arguments):
            if sa.kwarg_only or i >= len(args):
                if sa.name not in kwargs:
                    continue
                v = kwargs[sa.name]
            else:
                v = args[i]
            for t in tensors(v):
                r = tensor_region(t)
                reads.append(r)
                given.add(t.data_ptr())
                if sa.alias_info is not None and sa.alias_info.is_write:
                    writes.append(r)
        outs = out if isinstance(out, (list, tuple)) else (out,)
        for j, o in enumerate(outs):
            aliased = j < len(rets) and rets[j].alias_info is not None
            for t in tensors(o):
                if not aliased and t.data_ptr() not in given:      # (an input handed back, annotated or not: no new write)
                    writes.append(tensor_region(t))
        if not reads and not writes:
            return
        s = self._cur()
        self.trace.append(launch(s, name, reads, writes))
        if short == "_local_scalar_dense":                    # .item(): the host waits for the stream
            self.trace.append(sync(s))

    # ---- the collective
    def collective(self, reg):
        self._fresh += 1
        ev = ("to_comm", self._fresh)
        cur = self._cur()
        self.trace.append(record(ev, cur))
        self.trace.append(wait(COMM, ev))
        self.trace.append(launch(COMM, "all_reduce", [reg], [reg]))

    def collective_wait(self):
        self._fresh += 1
        ev = ("from_comm", self._fresh)
        self.trace.append(record(ev, COMM))
        self.trace.append(wait(self._cur(), ev))


def _make_mode(tracer):
    from torch.utils._python_dispatch import TorchDispatchMode

    class Mode(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            kwargs = kwargs or {}
            out = func(*args, **kwargs)
            tracer._torch_op(func, args, kwargs, out)
            return out
    return Mode()


class _Work(object):
    def __init__(self, tracer):
        self._tracer = tracer

    def wait(self):
        self._tracer.collective_wait()
        return True


class _DistShim(object):
    """stands where fplx.ddp has torch.distributed: everything but all_reduce is the real module's.

    The contract modelled is that of torch's NCCL / RCCL process group: the collective runs on the group's own
    communication stream, which first waits for the stream that was current when all_reduce was called; it reads and writes
    the tensor in place; work.wait() makes the stream that is current THEN wait for the communication stream (it does not
    block the host).  Nothing else orders the collective against anything."""

    def __init__(self, real, tracer):
        self._real, self._tracer = real, tracer

    def __getattr__(self, k):
        return getattr(self._real, k)

    def all_reduce(self, tensor, op=None, group=None, async_op=False):
        self._tracer.collective(tensor_region(tensor))
        w = _Work(self._tracer)
        if not async_op:
            w.wait()
            return None
        return w


def standin_reducer(bucket_ranges, domain_ranges):
    """a GradAllReducer that is enabled without a process group: pending / ready / reduce_domain / finish (and the fold in
    _reduce) are the product's; only the dist.all_reduce they reach is the tracer's (_DistShim)"""
    from fplx.ddp import GradAllReducer

    class StandInReducer(GradAllReducer):
        def __init__(self, buckets, domains):
            super(StandInReducer, self).__init__(buckets, domains)
            self.enabled, self.world = True, 1

    return StandInReducer(bucket_ranges, domain_ranges)
