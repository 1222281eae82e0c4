"""Where each weight-gradient product runs: on the current stream, forked to the side stream, or
queued and issued beside the next backward recurrence on a third stream."""
# The autograd ops (gemm_ops._on_side for dense.py, recurrent.py, encoder_stack.py, integrate.py) hand every parameter-gradient launch
# to on_side / side and bracket their backward recurrences with beside_recurrence; the streams, the
# waits, the captured graph's fork points and the end-of-backward join are decided here.  Nothing is
# imported from the op modules: a queued item's compute precision travels inside the callable handed in,
# and launch.set_grad_listener says whether deferral is allowed (allow_defer).
import collections
import contextlib
import ctypes
import os

import torch

from . import _lib

# --- weight gradients on a side stream
# Parameter gradients are consumed only by the optimizer / all-reduce, so the weight-gradient
# GEMMs (dW = dY^T X, fused bias sums) leave the backward's critical path: they run on one side
# stream per device, forked from the current stream when their operands are ready and joined back
# at the end of the backward pass (an autograd final callback), so `loss.backward()` returns with
# every gradient ordered before anything the caller issues next (graph capture included).  Their
# operands are record_stream'ed so the caching allocator does not recycle them early.  Products
# over fewer than _SIDE_MIN_ROWS rows (the T = 1 decode steps of the autoregressive loops, where
# a fork/join per frame costs more than it hides: C3 scheduled sampling 80 -> 130 ms measured)
# stay on the current stream; if the side stream already has work in this backward pass, the
# current stream first waits for it, so the writes into any one gradient buffer stay in order.
# MRG_WGRAD_STREAM=0 (or set_wgrad_stream(False)) issues everything on the current stream.
_WGRAD_SIDE = [os.environ.get("MRG_WGRAD_STREAM", "1") != "0"]
_SIDE_MIN_ROWS = 2048

# Deferred weight gradients (on by default, MRG_WGRAD_DEFER=0 turns it off; neutral in round 2, -0.34 ms/step
# with round 3's encoder wavefront, whose MFMA recurrences leave room on every CU): a side-stream product is not issued
# when its operands are ready but queued until the backward reaches its next persistent recurrence
# (beside_recurrence marks the current stream right before the recurrence launch and issues the queue
# right after it, ordered after the mark only), on the
# side stream with the GEMM grids capped at one block per CU while the recurrence runs at one
# workgroup per CU (mrg_lstm_set_blocks_per_cu): the latency-bound recurrence leaves most of each
# CU idle, and the dW products fill it instead of running beside the dX chain's GEMMs (which
# already fill the GPU).  The end-of-backward join issues whatever is still queued.  Queue order is
# side-stream order, so the writes into each gradient buffer keep their order; a write issued on the
# current stream (fewer than _SIDE_MIN_ROWS rows) first flushes the queue.  Not used while a
# gradient-ready listener (DDP bucket overlap) needs each write issued when it is reported.
_DEFER = [os.environ.get("MRG_WGRAD_DEFER", "1") == "1"]
_DEFER_ALLOWED = [True]   # False while a gradient-ready listener is set (launch.set_grad_listener)
# The queue flushed beside the recurrences runs on a stream of its own (the recurrence stream), the rest
# of the side work (the end-of-backward flush: the products of the layers below the last recurrence) on
# the side stream, so
# that flush starts when its operands are ready instead of behind the recurrence stream's backlog
# (in-graph wall-clock stamps, tools/side_timing.py: that backlog outlasts the main stream by ~1.7 ms;
# headline 20.55 -> 20.23 ms, A/B on one box).  Writes into one gradient buffer stay ordered: every
# queued item names the buffers it writes (on_side(writes=...)), and a flush on the side stream whose
# items touch a buffer the recurrence stream has written in this backward, or name none, waits for it
# first.  MRG_REC_STREAM=0 keeps everything on the side stream.
_REC_ON = [os.environ.get("MRG_REC_STREAM", "1") != "0"]
# MRG_SIDE_HOLD=0 turns the scratch hold off (diagnostic only: tests/test_gpu_capture.py)
_HOLD_SIDE_SCRATCH = [os.environ.get("MRG_SIDE_HOLD", "1") == "1"]


class _State:   # one device's scheduler state
    def __init__(self):
        self.side = self.rec = None   # the weight-gradient side stream, the recurrence-beside stream
        # Autograd graph-task id whose final callback will join the side streams back, or None.  The
        # task (torch._C._current_graph_task_id), not a bare flag: a backward that raised after a fork
        # never ran its callback, and a stale flag would make every later backward skip the join.
        self.join_task = None
        self.pending = []       # queued items (fn, keep, writes), in side-stream order
        self.rec_used = False   # the recurrence stream has work in this backward
        self.rec_writes = set()  # {(ptr, nbytes)} written on it in this backward (None: unknown)
        self.held = []          # side-stream scratch tensors kept alive until the join (hold_scratch)


_STATES = collections.defaultdict(_State)   # device index -> _State, made on first use


def set_wgrad_stream(on: bool) -> bool:
    """Enable / disable side-stream weight gradients; returns the previous setting."""
    prev = _WGRAD_SIDE[0]
    _WGRAD_SIDE[0] = bool(on)
    return prev


def set_wgrad_defer(on: bool) -> bool:
    """Enable / disable deferring side-stream weight gradients to the next recurrence; returns the old value."""
    prev = _DEFER[0]
    _DEFER[0] = bool(on)
    return prev


def allow_defer(on: bool) -> None:
    """Deferral is off while a gradient-ready listener needs each write issued when it is reported."""
    _DEFER_ALLOWED[0] = bool(on)


def side_stream(device):
    """The device's weight-gradient side stream, or None before its first fork."""
    # ddp.GradReducer orders its all-reduce stream after it.  The recurrence stream needs no such wait:
    # only deferred products use it, and deferral is off while a gradient-ready listener is set.
    return _STATES[torch.device(device).index or 0].side


def hold_scratch(t: torch.Tensor):
    """A scratch tensor allocated on the weight-gradient side stream stays referenced until the
    backward's join (see _drain).  Freed earlier, its block could go to an allocation on the
    main stream while the side-stream kernel that uses it has not run yet: inside a HIP-graph capture
    the private pool does not keep the two streams' blocks apart (measured: the encoder stack's
    replayed gradients were corrupted by split-K slabs reused as main-stream temporaries)."""
    st = _STATES.get(t.device.index or 0)
    if st is None or st.side is None or st.join_task is None or not _HOLD_SIDE_SCRATCH[0]:
        return
    cur = torch.cuda.current_stream(t.device)
    if (cur == st.side or cur == st.rec) and torch.cuda.is_current_stream_capturing():
        st.held.append(t)


# --- fork points under capture.  Measured (round 4, tools/tools_fork_variants.py, tools_fork_race.py):
# several side-stream forks from ONE point of the main stream (no main-stream node between them, e.g.
# one fork per weight-gradient product) capture into a graph whose edges are exactly the streams'
# order (tools/tools_capture_dot.py + tools_dot_deps.py), with no cross-stream address reuse
# (tools/tools_capture_alias.py) and no hand-off timeout, and the eager step is bitwise right with
# either stream delayed; yet its replay gives wrong gradients, deterministically, unless the HIP graph
# executor runs on one queue or a main-stream node separates the forks.
# So the executor mis-orders that topology (each fork's first side node has two predecessors: the
# same main node again and the previous side node).  The guard: a fork from the main-stream point
# the side stream already waited on adds no second wait (the side stream is ordered after that point
# already), so the redundant edges are never captured.
_HIP_CAPINFO = [None]
_LAST_FORK = {}   # key -> the capture point (capture id, main-stream dependency nodes) of the last fork
_FORK_GUARD = [os.environ.get("MRG_FORK_GUARD", "1") != "0"]   # 0: diagnostics only (tools_fork_variants.py)


def _capture_point(stream):
    """(capture id, the stream's current dependency node handles) while `stream` is capturing, else None."""
    if _HIP_CAPINFO[0] is None:
        f = ctypes.CDLL("libamdhip64.so").hipStreamGetCaptureInfo_v2
        f.restype = ctypes.c_int
        f.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_ulonglong),
                      ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.POINTER(ctypes.c_void_p)),
                      ctypes.POINTER(ctypes.c_size_t)]
        _HIP_CAPINFO[0] = f
    st, cid, graph = ctypes.c_int(0), ctypes.c_ulonglong(0), ctypes.c_void_p()
    deps, n = ctypes.POINTER(ctypes.c_void_p)(), ctypes.c_size_t(0)
    rc = _HIP_CAPINFO[0](ctypes.c_void_p(stream.cuda_stream), ctypes.byref(st), ctypes.byref(cid),
                         ctypes.byref(graph), ctypes.byref(deps), ctypes.byref(n))
    if rc != 0 or st.value != 1:   # hipStreamCaptureStatusActive
        return None
    return (cid.value,) + tuple(deps[i] for i in range(n.value))


def _fork(key, s, cur):
    """s.wait_stream(cur), skipped under capture when s already waited on cur's current point."""
    point = _capture_point(cur) if _FORK_GUARD[0] and torch.cuda.is_current_stream_capturing() else None
    if point is None or _LAST_FORK.get(key) != (point, s.cuda_stream):
        s.wait_stream(cur)
    _LAST_FORK[key] = None if point is None else (point, s.cuda_stream)


def reset_fork_point(key=None):
    """Forget the recorded fork point (all devices when key is None): called wherever the main and side
    streams are joined or ordered outside _fork, and at the end of every capture (graphs.capture), so
    the guard only ever skips a wait that an earlier _fork of the same capture really issued."""
    if key is None:
        _LAST_FORK.clear()
    else:
        _LAST_FORK.pop(key, None)


def _drain(key, cur, *, over, release=False):
    """Order `cur` after all of the device's weight-gradient work: issue the queue, wait for the side
    stream and, if it was used in this backward, the recurrence stream."""
    st = _STATES[key]
    _flush_deferred(key, cur.device)
    cur.wait_stream(st.side)
    if st.rec_used:
        cur.wait_stream(st.rec)
    # over: the backward that armed the join is over (its final callback, or a later backward that
    # finds the join of one that raised).  Mid-backward (a few-row write on the current stream) the
    # recurrence stream's bookkeeping and the join stay: the backward's later flushes still order
    # themselves after what the recurrence stream wrote, and its final callback still joins.
    if over:
        st.rec_used = False
        st.rec_writes = set()
        st.join_task = None
    reset_fork_point(key)
    if release:   # the final callback only: later work is ordered after its waits, the blocks are reusable
        st.held = []


def _begin(device):
    """(state, key, device, current stream, graph task) of a weight-gradient launch; a join left armed
    by a backward that did not finish is drained first (order after its side-stream work)."""
    dev = torch.device(device)
    key = dev.index or 0
    cur = torch.cuda.current_stream(dev)
    task = torch._C._current_graph_task_id()
    st = _STATES[key]
    if st.join_task is not None and st.join_task != task:
        _drain(key, cur, over=True)
    return st, key, dev, cur, task


def _arm_join(st, key, dev, cur, task):
    """The side stream (created on first use), with this backward's end-of-backward join queued."""
    if st.side is None:
        st.side = torch.cuda.Stream(device=dev)
    if st.join_task is None:
        torch.autograd.Variable._execution_engine.queue_callback(
            lambda: _drain(key, cur, over=True, release=True))
        st.join_task = task
    return st.side


def _defers(device, rows) -> bool:
    return (_WGRAD_SIDE[0] and _DEFER[0] and rows >= _SIDE_MIN_ROWS and _DEFER_ALLOWED[0]
            and torch._C._current_graph_task_id() >= 0)


def _flush_deferred(key, device, cap=0, after=None):
    """Issue the queued weight-gradient products on the side stream (GEMM grids capped at `cap`
    blocks per CU while they run beside a recurrence), ordered after event `after` when given, else
    after the current stream's work so far."""
    st = _STATES[key]
    items, st.pending = st.pending, []
    if not items:
        return
    dev = torch.device(device)
    cur = torch.cuda.current_stream(dev)
    s = st.side
    if _REC_ON[0] and after is not None:
        if st.rec is None:
            st.rec = torch.cuda.Stream(device=dev)
        s = st.rec
        st.rec_used = True
        for *_, writes in items:
            if writes is None or st.rec_writes is None:
                st.rec_writes = None
            else:
                st.rec_writes.update(writes)
        s.wait_event(after)
    else:
        if st.rec_used and _conflicts(items, st.rec_writes):
            s.wait_stream(st.rec)   # same gradient buffers (or unknown): keep their write order
        if after is None:
            _fork(key, s, cur)
        else:
            s.wait_event(after)
            _LAST_FORK[key] = None
    lib = _lib.load()
    prev = lib.mrg_gemm_set_blocks_per_cu(cap) if cap else None
    try:
        with torch.cuda.stream(s):
            for fn, keep, _ in items:
                for t in keep:
                    if t is not None:
                        t.record_stream(s)
                fn()
    finally:
        if cap:
            lib.mrg_gemm_set_blocks_per_cu(prev)


# Measured (r03, headline step, graph replay): issued BEFORE the recurrence launch the products were
# dispatched first and delayed its start (23.06 ms/step); issued after it, 21.80.  Joining the main
# stream to them right after (so they must finish beside this recurrence) measured 23.6: the
# recurrence runs ~25 % slower beside them and they outlast it, so the join is left to the end of
# the backward and the executor places them where the main stream leaves room.
@contextlib.contextmanager
def beside_recurrence(device):
    """Bracket of one backward recurrence launch: ``with beside_recurrence(dev) as cap:`` launch and
    check it.  cap is the recurrence's workgroups-per-CU cap (1 when deferring, else 0).  When products
    are queued, the current stream is marked right before the body and the queue is issued right after
    it, ordered after the mark (the work before the recurrence) but not after the recurrence; a body
    that raises issues nothing."""
    on = _WGRAD_SIDE[0] and _DEFER[0] and _DEFER_ALLOWED[0]
    dev = torch.device(device)
    key = dev.index or 0
    mark = None
    if on and _STATES[key].pending:
        mark = torch.cuda.Event()
        mark.record(torch.cuda.current_stream(dev))
    yield 1 if on else 0
    if mark is not None:
        _flush_deferred(key, device, cap=1, after=mark)


def _writes(tensors):
    """{(data_ptr, nbytes)} of the gradient buffers an item writes (None entries skipped)."""
    return {(t.data_ptr(), t.numel() * t.element_size()) for t in tensors if t is not None}


def _conflicts(items, rec_writes) -> bool:
    """True when an item of a flush writes a buffer the recurrence stream wrote (or either is unknown)."""
    if rec_writes is None:
        return True
    for *_, writes in items:   # an item's last field is its write set
        if writes is None:
            return True
        for p, n in writes:
            for q, m in rec_writes:
                if p < q + m and q < p + n:
                    return True
    return False


def on_side(device, rows, keep, fn, writes=None):
    """Run fn() (weight-gradient launches) on the side stream now, or queue it (see _DEFER).
    writes: the gradient tensors fn writes (ordering across the two side streams), None = unknown."""
    if not _defers(device, rows):
        with side(device, rows, keep):
            fn()
        return
    st, key, dev, cur, task = _begin(device)
    _arm_join(st, key, dev, cur, task)
    st.pending.append((fn, tuple(keep), None if writes is None else _writes(writes)))


class side:
    """Issue the enclosed launches on the device's weight-gradient stream (see above)."""
    __slots__ = ("dev", "rows", "keep", "ctx")

    def __init__(self, device, rows, keep=()):
        self.dev, self.rows, self.keep, self.ctx = device, rows, keep, None

    def __enter__(self):
        if not _WGRAD_SIDE[0]:
            return self
        st, key, dev, cur, task = _begin(self.dev)
        if self.rows < _SIDE_MIN_ROWS:
            if st.join_task is not None:  # order this write after the side streams' pending ones
                _drain(key, cur, over=False)
            return self
        if task < 0:  # not inside a backward pass: stay on the current stream
            return self
        s = _arm_join(st, key, dev, cur, task)
        _fork(key, s, cur)
        for t in self.keep:
            if t is not None:
                t.record_stream(s)
        self.ctx = torch.cuda.stream(s)
        self.ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if self.ctx is not None:
            self.ctx.__exit__(*exc)
        return False
