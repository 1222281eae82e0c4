"""What an op needs to call libmrg.so: pointers, the launch stream, workspace, the device error flag,
the kernel-timing probes, the gradient-ready listener and the precision context."""
import contextlib
import ctypes
import functools
from typing import Optional

import torch

from . import _lib
from .wgrad_streams import allow_defer, hold_scratch

# --- optional live kernel timing (bench.py).  Default: HIP events recorded on the launch stream
# around each library call.  kernel=True: the library times every kernel of a tagged call with
# kernel-bound events (mrg_probe_*, hipExtLaunchKernelGGL), i.e. the kernels' own execution as
# rocprofv3 reports it, without the packet dispatch a stream event pair also holds.
_PROBE_ON = set()
_PROBES = {}
_NATIVE = [False]
_CALLS = []          # native mode: (name, work) per tagged library call
_PROBE_CAP = 1 << 15


class _probe:
    """Bracket one library launch with timing events when ``name`` is being probed.

    ``work``: the launch's algorithmic FLOPs (or bytes), kept with its time for rooflines."""
    __slots__ = ("name", "e0", "work", "tagged")

    def __init__(self, name, work=0.0):
        self.name = name
        self.e0 = None
        self.work = work
        self.tagged = False

    def __enter__(self):
        if self.name in _PROBE_ON:
            if _NATIVE[0]:
                _lib.load().mrg_probe_tag(len(_CALLS))
                _CALLS.append((self.name, self.work))
                self.tagged = True
            else:
                self.e0 = torch.cuda.Event(enable_timing=True)
                self.e0.record()
        return self

    def __exit__(self, *exc):
        if self.tagged:
            _lib.load().mrg_probe_tag(-1)
        elif self.e0 is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            _PROBES.setdefault(self.name, []).append((self.e0, e1, self.work))
        return False


def probe_start(*names, kernel=False):
    _PROBE_ON.clear()
    _PROBE_ON.update(names)
    _PROBES.clear()
    _CALLS.clear()
    _NATIVE[0] = bool(kernel)
    if kernel:
        _lib.check(_lib.load().mrg_probe_start(_PROBE_CAP), "probe start")


def probe_stop(with_work=False):
    """Stop probing; returns {name: [ms per launch]} or, with_work, {name: [(ms, work)]} (synchronises).
    In kernel mode a launch's ms is the sum of its kernels' own execution times."""
    _PROBE_ON.clear()
    torch.cuda.synchronize()
    if _NATIVE[0]:
        _NATIVE[0] = False
        ms = (ctypes.c_float * _PROBE_CAP)()
        tags = (ctypes.c_int * _PROBE_CAP)()
        n = _lib.load().mrg_probe_stop(ms, tags, _PROBE_CAP)
        if n < 0:
            raise RuntimeError(f"probe stop: {_lib.load().mrg_last_error().decode()}")
        per_call = [0.0] * len(_CALLS)
        for i in range(n):
            per_call[tags[i]] += ms[i]
        out = {}
        for (name, work), t in zip(_CALLS, per_call):
            out.setdefault(name, []).append((t, work) if with_work else t)
        _CALLS.clear()
        return out
    if with_work:
        out = {k: [(a.elapsed_time(b), w) for a, b, w in v] for k, v in _PROBES.items()}
    else:
        out = {k: [a.elapsed_time(b) for a, b, _ in v] for k, v in _PROBES.items()}
    _PROBES.clear()
    return out


def _ptr(t: Optional[torch.Tensor], elem_offset: int = 0):
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr() + elem_offset * t.element_size())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ws(nbytes: int, device) -> torch.Tensor:
    t = torch.empty(max(1, (int(nbytes) + 3) // 4), dtype=torch.float32, device=device)
    hold_scratch(t)
    return t


def zero_(t: torch.Tensor) -> torch.Tensor:
    """In-place zero of a contiguous device tensor on the current stream (mrg_fill_zero)."""
    if t.numel():
        if not (t.is_cuda and t.is_contiguous()):
            raise ValueError("functional.zero_: contiguous device tensor required")
        _lib.check(_lib.load().mrg_fill_zero(_ptr(t), t.numel() * t.element_size(), _stream()), "fill zero")
    return t


def zeros(*shape, dtype=torch.float32, device=None) -> torch.Tensor:
    """torch.zeros through the library's fill kernel (no at::native kernel in the replayed step)."""
    return zero_(torch.empty(*shape, dtype=dtype, device=device))


_ERR = {}


def _err_flag(device) -> torch.Tensor:
    key = torch.device(device).index or 0
    if key not in _ERR:
        _ERR[key] = torch.zeros(1, dtype=torch.int32, device=device)
    return _ERR[key]


def check_errors(device=None):
    """Synchronise and raise if a persistent kernel reported a hand-off timeout."""
    for k, t in _ERR.items():
        if device is not None and (torch.device(device).index or 0) != k:
            continue
        if int(t.item()) != 0:
            t.zero_()
            raise RuntimeError("libmrg: LSTM recurrence hand-off timed out (grid not co-resident?)")


# --- gradient-ready listener (ddp.GradReducer with overlap): every parameter-gradient write goes
# through _gbuf() just before its launch, so a touched parameter is announced to the listener when
# the NEXT autograd Function's backward starts (every launch of the previous one is issued by then)
# or at the end of the backward pass.
_GRAD_LISTENER = [None]
_TOUCHED = []


def set_grad_listener(listener):
    """listener.ready(params) is called with parameters whose gradient writes have been issued
    (at most one autograd Function late); listener.end_of_backward() once per backward pass."""
    _GRAD_LISTENER[0] = listener
    _TOUCHED.clear()
    allow_defer(listener is None)   # each write is issued when it is reported


def _flush_touched():
    lst = _GRAD_LISTENER[0]
    if lst is not None and _TOUCHED:
        ready = list(_TOUCHED)
        _TOUCHED.clear()
        lst.ready(ready)


def _gbuf(p: torch.Tensor) -> Optional[torch.Tensor]:
    """The tensor a parameter's gradient accumulates into (created zero-filled on first use)."""
    if p is None or not p.requires_grad:
        return None
    if p.grad is None:
        p.grad = torch.zeros_like(p)
    if _GRAD_LISTENER[0] is not None:
        _GRAD_LISTENER[0].touch()
        _TOUCHED.append(p)
    return p.grad


# --- compute precision (mixed-precision configs, BASELINE configs[1] "bf16"): None = fp32 arithmetic
# (the library's GEMM mode: x6 split or exact f32), "bf16" = GEMM operands rounded to bf16 with fp32
# accumulation (mrg_gemm_bf16_ex).  Set by the model's forward; every autograd Function records it in
# forward and restores it around its backward (which runs on autograd's thread, after the context).
_ARITH = [None]
PRECISIONS = {None: None, "32": None, 32: None, "fp32": None, "32-true": None,
              "bf16": "bf16", "bf16-mixed": "bf16", "bf16-true": "bf16"}


@contextlib.contextmanager
def precision(p):
    """Compute precision of the enclosed ops: '32'/'fp32' or 'bf16'/'bf16-mixed' (Lightning names)."""
    if p not in PRECISIONS:
        raise ValueError(f"unsupported precision {p!r} (one of {sorted(map(str, PRECISIONS))})")
    prev = _ARITH[0]
    _ARITH[0] = PRECISIONS[p]
    try:
        yield
    finally:
        _ARITH[0] = prev


def _keeps_precision(fn):
    """Decorator for autograd Function forward/backward: forward records the active precision in ctx,
    backward runs under it."""
    @functools.wraps(fn)
    def wrapper(ctx, *args):
        if fn.__name__ == "forward":
            ctx.arith = _ARITH[0]
            return fn(ctx, *args)
        _flush_touched()  # the previous Function's gradient writes are all issued
        prev = _ARITH[0]
        _ARITH[0] = getattr(ctx, "arith", None)
        try:
            return fn(ctx, *args)
        finally:
            _ARITH[0] = prev
    return wrapper
