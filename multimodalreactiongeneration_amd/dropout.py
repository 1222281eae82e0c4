"""The device dropout RNG (csrc/rng.h, rng.py) and the flat dropout op: a per-device {seed, draw} state in
device memory.  An op that drops takes one draw with a one-thread kernel (a graph node: a replayed step takes
fresh draws) and keeps the 16-byte key tensor for its backward.  All DDP ranks share the default seed unless
the caller seeds per rank (manual_seed(base + rank))."""
import torch
from torch.autograd import Function

from . import _lib
from .launch import _flush_touched, _ptr, _stream

_RNG = {}


def _i64(v: int) -> int:
    v = int(v) & (2 ** 64 - 1)
    return v - 2 ** 64 if v >= 2 ** 63 else v


def _rng_device(device) -> torch.device:
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("the dropout RNG state lives on a HIP device")
    return torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)


def _rng_state(device) -> torch.Tensor:
    dev = _rng_device(device)
    if dev.index not in _RNG:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the dropout RNG state must exist before graph capture (run the step once, "
                               "or call functional.manual_seed, first)")
        from .rng import DEFAULT_SEED
        _RNG[dev.index] = torch.tensor([_i64(DEFAULT_SEED), 0], dtype=torch.int64, device=dev)
    return _RNG[dev.index]


def manual_seed(seed: int, device=None) -> None:
    """Reset the device's dropout RNG state to {seed, draw 0} (default seed: rng.DEFAULT_SEED)."""
    set_rng_state(device, (seed, 0))


def get_rng_state(device=None):
    """(seed, draw) of the device's dropout RNG state as Python ints (synchronises)."""
    seed, draw = _rng_state(device).tolist()
    return seed & (2 ** 64 - 1), draw & (2 ** 64 - 1)


def set_rng_state(device, state) -> None:
    seed, draw = state
    st = _rng_state(device)
    st.copy_(torch.tensor([_i64(seed), _i64(draw)], dtype=torch.int64))


def _drop_consts(p):
    """(thr, scale_keep) of a dropout probability (ValueError outside [0, 1))."""
    from .rng import threshold
    return threshold(p), 1.0 / (1.0 - float(p))


def _rng_draw(device) -> torch.Tensor:
    """Take one draw: the op's key tensor {seed, draw} (int64 [2], device memory)."""
    key = torch.empty(2, dtype=torch.int64, device=device)
    _lib.check(_lib.load().mrg_rng_draw(_ptr(_rng_state(device)), _ptr(key), _stream()), "rng draw")
    return key


def dropout_keep_mask(key: torch.Tensor, n: int, p: float) -> torch.Tensor:
    """uint8 [n]: the keep decisions functional.dropout makes with ``key`` (tests, debugging)."""
    thr, _ = _drop_consts(p)
    out = torch.empty(n, dtype=torch.uint8, device=key.device)
    _lib.check(_lib.load().mrg_dropout_keep_mask(n, thr, _ptr(key), _ptr(out), _stream()), "dropout keep mask")
    return out


def attention_keep_mask(key: torch.Tensor, B: int, heads: int, Tq: int, Tk: int, p: float) -> torch.Tensor:
    """uint8 [B, heads, Tq, Tk]: the keep decisions of an attention op that holds ``key``."""
    thr, _ = _drop_consts(p)
    out = torch.empty(B, heads, Tq, Tk, dtype=torch.uint8, device=key.device)
    _lib.check(_lib.load().mrg_attention_keep_mask(B, heads, Tq, Tk, thr, _ptr(key), _ptr(out), _stream()),
               "attention keep mask")
    return out


class _DropoutFn(Function):
    """y = keep ? x / (1 - p) : 0 with one draw; the backward runs the same kernel on the gradient with
    the saved key (no mask tensor is stored)."""

    @staticmethod
    def forward(ctx, x, p):
        _lib.require_device(x)
        thr, sk = _drop_consts(p)
        xc = x.contiguous()
        key = _rng_draw(xc.device)
        y = torch.empty_like(xc)
        _lib.check(_lib.load().mrg_dropout(xc.numel(), thr, sk, _ptr(key), _ptr(xc), _ptr(y), _stream()), "dropout")
        ctx.save_for_backward(key)
        ctx.consts = (thr, sk)
        return y

    @staticmethod
    def backward(ctx, dy):
        _flush_touched()
        (key,) = ctx.saved_tensors
        thr, sk = ctx.consts
        g = dy.contiguous()
        dx = torch.empty_like(g)
        _lib.check(_lib.load().mrg_dropout(g.numel(), thr, sk, _ptr(key), _ptr(g), _ptr(dx), _stream()), "dropout bwd")
        return dx, None


def dropout(x, p):
    """Inverted dropout (training mode) on the library's counter-based RNG.  p = 0 returns x."""
    thr, _ = _drop_consts(p)
    if x.dtype != torch.float32:
        raise ValueError("functional.dropout: float32 tensor required")
    if float(p) == 0.0:
        return x
    return _DropoutFn.apply(x, float(p))
