"""Host-side happens-before and lifetime audit of the library's launches on more than one HIP stream.

The forward plan (dasr_amd/graph.py, tape.py) issues the depth branch of every SEAN on a side stream.  Two things keep that
correct and neither is visible to an op test: every cross-stream read is ordered behind its write by an event, and every
tensor that is allocated on one stream and used on the other is ``record_stream``ed before its last Python reference
goes (torch's caching allocator hands a freed block back to the pool of its ALLOCATION stream at once; only a
``record_stream`` makes it wait for the other stream's work).  ``with audit() as log:`` records what is needed to check
both, entirely on the host, and restores everything on exit:

* a proxy in place of the handle ``_lib.get()`` returns logs every ``dasr_*`` call whose last declared argument is the
  ``void* stream``: sequence number, name, stream handle and every pointer argument with its mode (``const T*`` read;
  ``T*`` / ``void*`` write, read-write counts as write).  The two job-table launches are resolved through their table (the
  host array of ``ops.PackJob`` / ``ops.SplitJob``), size queries have no stream argument and are not launches;
* ``_lib.ptr`` registers the storage (base address, bytes) of every tensor handed to the library; interior pointers
  (``buf[:na]``) resolve by range.  The allocation stream comes from the caching allocator (``torch.cuda.memory_snapshot()``
  segments), the time of the free from a ``weakref.finalize`` on the storage;
* ``torch.cuda.Stream.record_event / wait_event / wait_stream / synchronize``, ``torch.cuda.Event.record / wait /
  synchronize``, ``torch.cuda.synchronize`` and ``torch.Tensor.record_stream`` feed one vector clock per stream.

Two rules, one report line per violation (``log.reports``):

1. ORDER.  Launch L on stream s touches storage S; the last conflicting launch W (write/read, read/write, write/write on
   overlapping bytes) on every other stream must happen-before L in the vector clocks.
2. LIFETIME.  Storage S from stream a's pool was touched by launch L on another stream s.  When S is freed, either
   ``record_stream(s)`` was called on a tensor of S, or stream a had already joined a clock of s taken after L.

Every check is a property of the recorded trace: nothing is timed, slowed or repeated, and the audit never calls
``empty_cache``.

BLIND SPOT: torch's own kernels are not in the log - ``torch.zeros`` fills, ``torch.cat``, ``.to()``, the loss arithmetic,
autograd's gradient accumulation, the optimiser.  The audit is about the library's launches; a hazard between a torch op
and a launch, or between two torch ops, is not seen.  Host read-backs (``.item()``, ``.cpu()``) are not modelled as
synchronisation either, which can only add reports, never hide one.

OUT OF SCOPE: captured replays (a hipGraph replay issues no launch from Python), ``graph.WGRAD_STREAM`` and
``graph.TAIL_WGRAD_SIDE`` (both off in the product), more than one rank.

``Checker`` is the pure-Python core (no torch, no library): tests/test_stream_audit.py drives it with hand-written traces.
"""
import bisect
import collections
import contextlib
import os
import re
import sys
import threading
import weakref

SITE_FILES = ("graph.py", "harness.py", "video.py")
_SKIP_FILES = ("stream_audit.py", "ops.py", "_lib.py", "tape.py", "weakref.py")


def _hx(s):
    return "0x%x" % s if isinstance(s, int) else str(s)


class Storage:
    __slots__ = ("base", "nbytes", "alloc_stream", "accesses", "foreign", "recorded", "freed", "ref", "adopted", "__weakref__")

    def __init__(self, base, nbytes, alloc_stream):
        self.base, self.nbytes, self.alloc_stream = base, nbytes, alloc_stream
        self.accesses = []       # [(launch, arg index, lo, hi, is_write)], pruned as later accesses cover earlier ones
        self.foreign = {}        # stream != alloc_stream -> (last launch on it that touched this storage, arg index)
        self.recorded = set()    # streams given to record_stream
        self.freed = False
        self.ref = None          # (real audits) weak reference to the torch storage
        self.adopted = False     # (real audits) known from the allocator's block list only

    def describe(self):
        return "storage %d B @0x%x allocated on stream %s" % (self.nbytes, self.base, _hx(self.alloc_stream))


class Arg:
    __slots__ = ("index", "name", "mode", "storage", "lo", "hi", "writer")

    def __init__(self, index, name, mode, storage, lo, hi):
        self.index, self.name, self.mode, self.storage, self.lo, self.hi = index, name, mode, storage, lo, hi
        self.writer = None       # the launch that last wrote (part of) these bytes, if it is in the log


class Launch:
    __slots__ = ("seq", "name", "stream", "n", "site", "args")

    def __init__(self, seq, name, stream, n, site):
        self.seq, self.name, self.stream, self.n, self.site = seq, name, stream, n, site
        self.args = []

    def arg(self, index):
        for a in self.args:
            if a.index == index:
                return a
        return None

    def describe(self, index=None):
        s = "#%d %s" % (self.seq, self.name)
        a = self.arg(index) if index is not None else None
        if a is not None:
            s += " arg %d '%s' (%s)" % (a.index, a.name, "write" if a.mode == "w" else "read")
        return s + " on stream %s" % _hx(self.stream)


class Checker:
    """The trace and the two rules.  Streams and events are any hashable keys (raw handles in a real audit)."""

    def __init__(self):
        self.lock = threading.RLock()
        self.reports = []
        self.launches = []
        self.unresolved = 0          # pointer arguments that fell into no registered storage
        self.closed = False
        self._clock = {}             # stream -> {stream: launches of it known to happen before the next op issued here}
        self._count = {}             # stream -> launches issued
        self._host = {}              # what the host has waited for
        self._events = {}            # event key -> clock snapshot at its last record
        self._bases = []             # sorted base addresses of the live storages
        self._store = {}             # base -> Storage
        self._freed = collections.deque()   # (storage, site): frees wait here until the next operation (finalizers may
                                            # fire anywhere, also while this thread holds the lock)

    # ---- storages ---------------------------------------------------------------------------------------------
    def alloc(self, base, nbytes, stream):
        with self.lock:
            self._drain()
            i = bisect.bisect_left(self._bases, base)
            # whatever still overlaps the new block is gone (its free was not seen): it cannot be live any more
            while i > 0 and self._bases[i - 1] + self._store[self._bases[i - 1]].nbytes > base:
                i -= 1
            while i < len(self._bases) and self._bases[i] < base + nbytes:
                self._store.pop(self._bases.pop(i)).freed = True
            st = Storage(base, nbytes, stream)
            bisect.insort(self._bases, base)
            self._store[base] = st
            return st

    def resolve(self, ptr):
        """(storage, offset) of an address inside a live storage, else None."""
        i = bisect.bisect_right(self._bases, ptr) - 1
        if i >= 0:
            st = self._store[self._bases[i]]
            if ptr < st.base + st.nbytes:
                return st, ptr - st.base
        return None

    def lookup(self, base):
        return self._store.get(base)

    def free(self, storage, site=None):
        """May be called from a finalizer: only queues.  The rule is checked before the next operation changes a clock."""
        if not self.closed and storage is not None:
            self._freed.append((storage, site, self.launches[-1] if self.launches else None))

    def free_at(self, ptr, site=None):
        hit = self.resolve(ptr)
        self.free(hit[0] if hit else None, site)
        with self.lock:
            self._drain()

    def _drain(self):
        while self._freed:
            st, site, last = self._freed.popleft()
            if st.freed:
                continue
            st.freed = True
            if self._store.get(st.base) is st:
                del self._store[st.base]
                self._bases.pop(bisect.bisect_left(self._bases, st.base))
            a = st.alloc_stream
            for s, (L, idx) in sorted(st.foreign.items(), key=lambda kv: kv[1][0].seq):
                if s in st.recorded or self._clk(a).get(s, 0) >= L.n:
                    continue
                self.reports.append(
                    "LIFETIME %s is freed after %s%s, back to the pool of stream %s, with no record_stream(%s) and before "
                    "stream %s waited for %s; used at %s" % (
                        st.describe(), last.describe() if last is not None else "no launch",
                        " (free at %s)" % site if site else "", _hx(a), _hx(s), _hx(a), L.describe(idx), L.site or "?"))

    # ---- clocks -----------------------------------------------------------------------------------------------
    def _clk(self, s):
        c = self._clock.get(s)
        if c is None:
            c = self._clock[s] = dict(self._host)
        return c

    @staticmethod
    def _join(dst, src):
        for k, v in src.items():
            if dst.get(k, 0) < v:
                dst[k] = v

    def record_event(self, event, stream):
        with self.lock:
            self._drain()
            self._events[event] = dict(self._clk(stream))

    def wait_event(self, event, stream):
        with self.lock:
            self._drain()
            self._join(self._clk(stream), self._events.get(event, {}))      # an event never recorded orders nothing

    def wait_stream(self, waiter, waited):
        """``waiter.wait_stream(waited)``: a record on ``waited`` plus a wait on ``waiter``."""
        with self.lock:
            self._drain()
            self._join(self._clk(waiter), dict(self._clk(waited)))

    def _host_joined(self):
        for c in self._clock.values():
            self._join(c, self._host)

    def sync_stream(self, stream):
        with self.lock:
            self._drain()
            self._join(self._host, self._clk(stream))
            self._host_joined()

    def sync_event(self, event):
        with self.lock:
            self._drain()
            self._join(self._host, self._events.get(event, {}))
            self._host_joined()

    def sync_all(self):
        with self.lock:
            self._drain()
            for c in list(self._clock.values()):
                self._join(self._host, c)
            self._host_joined()

    def record_stream(self, ptr, stream):
        with self.lock:
            self._drain()
            hit = self.resolve(ptr)
            if hit is not None:
                hit[0].recorded.add(stream)

    # ---- launches ---------------------------------------------------------------------------------------------
    def launch(self, name, stream, args, site=None):
        """``args``: [(argument index, argument name, address, bytes or None, 'r' | 'w')]."""
        with self.lock:
            self._drain()
            clk = self._clk(stream)
            n = self._count.get(stream, 0) + 1
            self._count[stream] = n
            L = Launch(len(self.launches), name, stream, n, site)
            self.launches.append(L)
            for index, aname, ptr, nbytes, mode in args:
                hit = self.resolve(ptr)
                if hit is None:
                    self.unresolved += 1
                    continue
                st, lo = hit
                hi = st.nbytes if nbytes is None else min(st.nbytes, lo + nbytes)
                arg = Arg(index, aname, mode, st, lo, hi)
                L.args.append(arg)
                self._check_order(L, arg, clk)
                if st.alloc_stream is not None and stream != st.alloc_stream:
                    st.foreign[stream] = (L, index)
            for arg in L.args:                     # (after the checks: two arguments of one launch do not conflict)
                self._note(L, arg)
            clk[stream] = n
            return L

    def _check_order(self, L, arg, clk):
        write = arg.mode == "w"
        seen = set()
        for W, widx, lo, hi, wwrite in reversed(arg.storage.accesses):
            if hi <= arg.lo or arg.hi <= lo:
                continue
            if wwrite and arg.writer is None:
                arg.writer = W
            if not (write or wwrite) or W.stream == L.stream or W.stream in seen:
                continue
            seen.add(W.stream)                      # the last conflicting launch of that stream: its clock is monotonic
            if clk.get(W.stream, 0) < W.n:
                self.reports.append("ORDER %s is not ordered after %s; %s; at %s" % (
                    L.describe(arg.index), W.describe(widx), arg.storage.describe(), L.site or "?"))

    def _note(self, L, arg):
        acc = arg.storage.accesses
        write = arg.mode == "w"
        # covered by this access: every later launch that is ordered behind this one is ordered behind those too (or the
        # pair was reported just now)
        acc[:] = [a for a in acc if not (arg.lo <= a[2] and a[3] <= arg.hi and (write or (not a[4] and a[0].stream == L.stream)))]
        acc.append((L, arg.index, arg.lo, arg.hi, write))

    def close(self):
        with self.lock:
            self._drain()
            self.closed = True


# ---------------------------------------------------------------------------------------------------------------------
# the real thing: torch + the library
# ---------------------------------------------------------------------------------------------------------------------
def declared_arguments(header_path):
    """{function: [argument names]} of include/dasr.h (``_lib.declared_functions`` keeps the types only)."""
    text = open(header_path).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    out = {}
    for m in re.finditer(r"(int|size_t|const char\*)\s+(dasr_\w+)\s*\(([^)]*)\)\s*;", text):
        args = m.group(3).strip()
        names = []
        if args and args != "void":
            for a in args.split(","):
                a = " ".join(a.split())
                names.append("" if a.endswith("*") else a.rsplit(" ", 1)[1].lstrip("*"))
        out[m.group(2)] = names
    return out


def call_site():
    """``file:line (function)`` of the innermost frame in graph.py / harness.py / video.py, else of the innermost frame
    outside the plumbing."""
    f = sys._getframe(1)
    fallback = None
    while f is not None:
        base = os.path.basename(f.f_code.co_filename)
        if base in SITE_FILES:
            return "%s:%d (%s)" % (base, f.f_lineno, f.f_code.co_name)
        if fallback is None and base not in _SKIP_FILES:
            fallback = "%s:%d (%s)" % (base, f.f_lineno, f.f_code.co_name)
        f = f.f_back
    return fallback


_JOB_FIELDS = {  # job-table launches: (struct in dasr_amd.ops, [(field, mode)])
    "dasr_weight_pack_multi": ("PackJob", (("v", "r"), ("g", "r"), ("w", "w"), ("inv_norm", "w"), ("amax", "w"))),
    "dasr_conv3x3_split2_weights_multi": ("SplitJob", (("w_packed", "r"), ("wmax", "r"), ("w_split", "w"))),
}


class _Proxy:
    """Stands where the ctypes handle stood: launches are logged, everything else passes through."""

    def __init__(self, real, log):
        self._real, self._log, self._cache = real, log, {}

    def __getattr__(self, name):
        fn = self._cache.get(name)
        if fn is None:
            fn = self._log._wrap(name, getattr(self._real, name))
            self._cache[name] = fn
        return fn


class AuditLog(Checker):
    def __init__(self):
        super().__init__()
        from dasr_amd import _lib
        self._extent = {}            # address -> bytes of the tensor (view) last handed to the library at it
        self._segments = ([], [])    # allocator segments: sorted start addresses, [(start, end, stream)]
        self._keep = []              # events, kept alive so that their id() stays theirs
        self._is_device = _lib.is_device_build()
        types = _lib.declared_functions()
        names = declared_arguments(_lib.HEADER)
        self._sig = {}
        for fn, (_ret, argtypes) in types.items():
            if argtypes and argtypes[-1] == "void*" and names[fn][-1] == "stream":
                self._sig[fn] = [(i, names[fn][i], "r" if ty.startswith("const ") else "w")
                                 for i, ty in enumerate(argtypes[:-1]) if ty.endswith("*") and ty != "const char*"
                                 and "dasr_" not in ty]

    # ---- storages of real tensors -----------------------------------------------------------------------------
    def _alloc_stream(self, addr):
        import torch
        for attempt in (0, 1):
            starts, segs = self._segments
            i = bisect.bisect_right(starts, addr) - 1
            if i >= 0 and addr < segs[i][1]:
                return segs[i][2]
            if attempt == 0:
                segs = sorted((s["address"], s["address"] + s["total_size"], int(s["stream"]))
                              for s in torch.cuda.memory_snapshot())
                self._segments = ([s[0] for s in segs], segs)
        return None

    def register(self, t):
        """The Storage of tensor ``t`` (None for an empty one), known from now on."""
        st = t.untyped_storage()
        nbytes = st.nbytes()
        if nbytes == 0:
            return None
        base = st.data_ptr()
        with self.lock:
            rec = self.lookup(base)
            if rec is not None and rec.ref is None and rec.adopted:     # met before as a bare address (_adopt): same block
                rec.nbytes, rec.adopted = nbytes, False
            elif rec is None or rec.ref is None or rec.ref() is not st:
                rec = self.alloc(base, nbytes, self._alloc_stream(base) if t.is_cuda else None)
            else:
                return rec
            rec.ref = weakref.ref(st)
            weakref.finalize(st, self._on_free, rec).atexit = False
        return rec

    def _adopt(self, ptrs):
        """Addresses that reach a launch without having passed ``_lib.ptr`` in this audit (a job table built before it,
        whose jobs hold bare pointers): the allocator's own record of the live block around each - base, size and pool.
        Such a storage has no finalizer (its free is not seen; it is dropped when its address is handed out again)."""
        import torch
        if not any(self.resolve(p) is None for p in ptrs):
            return
        blocks = []
        for seg in torch.cuda.memory_snapshot():
            addr = seg["address"]
            for b in seg["blocks"]:
                addr = b.get("address", addr)
                if b["state"] == "active_allocated":
                    blocks.append((addr, b["size"], int(seg["stream"])))
                addr += b["size"]
        blocks.sort()
        starts = [b[0] for b in blocks]
        with self.lock:
            for p in ptrs:
                i = bisect.bisect_right(starts, p) - 1
                if self.resolve(p) is None and i >= 0 and p < blocks[i][0] + blocks[i][1]:
                    self.alloc(*blocks[i]).adopted = True

    def _on_free(self, rec):
        if not self.closed:
            self.free(rec, call_site() if rec.foreign else None)

    # ---- launches ---------------------------------------------------------------------------------------------
    def _wrap(self, name, fn):
        sig = self._sig.get(name)
        if sig is None:
            return fn
        table = _JOB_FIELDS.get(name)

        def launch(*args):
            stream = args[-1] or 0
            if table is not None:
                ptrs = self._table_args(table, args[0], args[2])
                if self._is_device:
                    self._adopt([p[2] for p in ptrs])
            else:
                ptrs = [(i, an, args[i], self._extent.get(args[i]), mode) for i, an, mode in sig if args[i]]
            self.launch(name, stream, ptrs, call_site())
            return fn(*args)

        return launch

    def _table_args(self, table, host_addr, n):
        from dasr_amd import ops
        struct, fields = table
        jobs = (getattr(ops, struct) * n).from_address(host_addr)
        out = []
        for j in range(n):
            for field, mode in fields:
                p = getattr(jobs[j], field)
                if p:
                    out.append((0, "jobs[%d].%s" % (j, field), p, self._extent.get(p), mode))
        return out

    def streams(self):
        return sorted({L.stream for L in self.launches})


_MISSING = object()


@contextlib.contextmanager
def audit():
    """Everything the module docstring lists, patched for the duration of the block."""
    import torch
    from dasr_amd import _lib
    log = AuditLog()
    saved = []
    tls = threading.local()

    def patch(obj, name, new):
        saved.append((obj, name, obj.__dict__.get(name, _MISSING)))
        setattr(obj, name, new)

    def outermost(orig, book):
        """Stream.record_event calls Event.record, wait_stream calls wait_event ...: only the outermost patched call of a
        thread does the bookkeeping, after the real call."""
        def wrapper(*a, **k):
            depth = getattr(tls, "depth", 0)
            tls.depth = depth + 1
            try:
                out = orig(*a, **k)
            finally:
                tls.depth = depth
            if depth == 0:
                book(out, *a, **k)
            return out
        return wrapper

    def h(stream):
        return (torch.cuda.current_stream() if stream is None else stream).cuda_stream

    def ev(e):
        log._keep.append(e)
        return id(e)

    S, E = torch.cuda.Stream, torch.cuda.Event
    real_get, real_ptr = _lib.get, _lib.ptr
    proxy = _Proxy(real_get(), log)

    def ptr(t, allow_none=False, dtype=torch.float32):
        p = real_ptr(t, allow_none, dtype)
        if t is not None and log.register(t) is not None:
            log._extent[p] = t.numel() * t.element_size()
        return p

    def record_stream(out, t, stream):
        if log.register(t) is not None:
            log.record_stream(t.untyped_storage().data_ptr(), stream.cuda_stream)

    patch(_lib, "get", lambda: proxy)
    patch(_lib, "ptr", ptr)
    patch(S, "record_event", outermost(S.record_event, lambda out, self, event=None: log.record_event(ev(out), self.cuda_stream)))
    patch(S, "wait_event", outermost(S.wait_event, lambda out, self, event: log.wait_event(id(event), self.cuda_stream)))
    patch(S, "wait_stream", outermost(S.wait_stream, lambda out, self, stream: log.wait_stream(self.cuda_stream, stream.cuda_stream)))
    patch(S, "synchronize", outermost(S.synchronize, lambda out, self: log.sync_stream(self.cuda_stream)))
    patch(E, "record", outermost(E.record, lambda out, self, stream=None: log.record_event(ev(self), h(stream))))
    patch(E, "wait", outermost(E.wait, lambda out, self, stream=None: log.wait_event(id(self), h(stream))))
    patch(E, "synchronize", outermost(E.synchronize, lambda out, self: log.sync_event(id(self))))
    patch(torch.cuda, "synchronize", outermost(torch.cuda.synchronize, lambda out, *a, **k: log.sync_all()))
    patch(torch.Tensor, "record_stream", outermost(torch.Tensor.record_stream, record_stream))
    try:
        yield log
    finally:
        for obj, name, old in reversed(saved):
            if old is _MISSING:
                delattr(obj, name)
            else:
                setattr(obj, name, old)
        log.close()
