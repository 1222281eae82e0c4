"""Padding helpers, gradient clipping, the masked losses and the per-target metric updates."""
import ctypes
import math
from typing import Optional

import torch
from torch.autograd import Function

from . import _lib
from .launch import _ptr, _stream, _ws, zeros
from .wgrad_streams import hold_scratch


def padding_flags(x: torch.Tensor, padding_value: float = -100.0) -> torch.Tensor:
    """uint8 [B, T]: frame is padding (x[:, :, 0] == -100), as gen_attention_mask tests it
    (one library kernel on the device; torch on the host, e.g. for the CPU mask goldens)."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 3):
        return (x[:, :, 0] == padding_value).to(torch.uint8).contiguous()
    B, T, _ = x.shape
    out = torch.empty(B, T, dtype=torch.uint8, device=x.device)
    _lib.check(_lib.load().mrg_padding_flags(B, T, _ptr(x), x.stride(0), x.stride(1), float(padding_value), _ptr(out),
                                             _stream()), "padding flags")
    return out


def zero_padding(x: torch.Tensor, padding_value: float = -100.0) -> torch.Tensor:
    """x * (x != -100) (training_step's zeroing of padded motion_self frames, lstmformer.py:365-366)."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.data_ptr() % 16 == 0):
        return x * (x != padding_value).to(x.dtype)
    y = torch.empty_like(x)
    _lib.check(_lib.load().mrg_zero_padding(x.numel(), _ptr(x), float(padding_value), _ptr(y), _stream()),
               "zero padding")
    return y


# ------------------------------------------------------------------ gradient clipping
def _flat_f32(t: torch.Tensor, who: str):
    _lib.require_device(t)
    if t.dtype != torch.float32:
        raise ValueError(f"functional.{who}: float32 required (got {t.dtype})")
    if not t.is_contiguous():
        raise ValueError(f"functional.{who}: contiguous tensor required (it is clipped in place, not copied)")


def clip_grad_workspace(n: int, device) -> torch.Tensor:
    """The per-block partials buffer mrg_grad_clip_norm needs for n elements."""
    nbytes = _lib.load().mrg_grad_clip_workspace_bytes(int(n))
    return torch.empty(max(1, (nbytes + 3) // 4), dtype=torch.float32, device=device)


def _accum_i32(accum: torch.Tensor, who: str):
    if not (accum.is_cuda and accum.dtype == torch.int32 and accum.is_contiguous() and accum.numel() >= 2):
        raise ValueError(f"functional.{who}: accum must be a contiguous device int32[2] = {{micro, n}}")


def clip_grad_norm_(flat_grad: torch.Tensor, max_norm: float, clip_state: Optional[torch.Tensor] = None,
                    workspace: Optional[torch.Tensor] = None, accum: Optional[torch.Tensor] = None) -> torch.Tensor:
    """torch.nn.utils.clip_grad_norm_(norm_type=2, error_if_nonfinite=False) over one buffer, in place
    (mrg_grad_clip_norm).  Returns clip_state, a device float32[2] = {norm before clipping, coefficient
    applied}; nothing is read back.  max_norm = inf only measures.  clip_state / workspace
    (clip_grad_workspace) may be passed in so that the call allocates nothing.
    accum (an optimizer's accum_state, device int32 {micro, n}): the buffer holds a window's summed
    gradients; the call does nothing unless it closes the window, and then clips their mean
    (mrg_grad_clip_norm_accum; the fused step that follows must be given the same clip_state)."""
    _flat_f32(flat_grad, "clip_grad_norm_")
    if clip_state is None:
        clip_state = zeros(2, device=flat_grad.device)
    elif not (clip_state.is_cuda and clip_state.dtype == torch.float32 and clip_state.is_contiguous()
              and clip_state.numel() >= 2):
        raise ValueError("functional.clip_grad_norm_: clip_state must be a contiguous device float32[2]")
    n = flat_grad.numel()
    if workspace is None:
        workspace = clip_grad_workspace(n, flat_grad.device)
        hold_scratch(workspace)
    if accum is not None:
        _accum_i32(accum, "clip_grad_norm_")
        _lib.check(_lib.load().mrg_grad_clip_norm_accum(_ptr(flat_grad), n, float(max_norm), _ptr(clip_state),
                                                        _ptr(workspace), _ptr(accum), _stream()),
                   "grad clip norm (accumulation)")
        return clip_state
    _lib.check(_lib.load().mrg_grad_clip_norm(_ptr(flat_grad), n, float(max_norm), _ptr(clip_state),
                                              _ptr(workspace), _stream()), "grad clip norm")
    return clip_state


def clip_grad_value_(flat_grad: torch.Tensor, clip_value: float, accum: Optional[torch.Tensor] = None) -> torch.Tensor:
    """torch.clamp(g, -clip_value, clip_value) in place (mrg_grad_clip_value); a NaN stays NaN.
    accum: as in clip_grad_norm_; on the call that closes the window, clamp(g / n, -clip_value, clip_value)
    (mrg_grad_clip_value_accum; the fused step that follows must be told the division is done)."""
    _flat_f32(flat_grad, "clip_grad_value_")
    if accum is not None:
        _accum_i32(accum, "clip_grad_value_")
        _lib.check(_lib.load().mrg_grad_clip_value_accum(_ptr(flat_grad), flat_grad.numel(), float(clip_value),
                                                         _ptr(accum), _stream()), "grad clip value (accumulation)")
        return flat_grad
    _lib.check(_lib.load().mrg_grad_clip_value(_ptr(flat_grad), flat_grad.numel(), float(clip_value), _stream()),
               "grad clip value")
    return flat_grad


# ------------------------------------------------------------------ loss
_LOSS_TYPES = {"huber": 0, "mse": 1, "mae": 2, "smoothl1": 3}


class _LossFn(Function):
    @staticmethod
    def forward(ctx, y, target, lead, spec):
        _lib.require_device(y)
        y, target = y.contiguous(), target.contiguous()
        B, Ttot, F = y.shape
        T = target.shape[1]
        if Ttot - lead != T or target.shape[0] != B or target.shape[2] != F:
            raise RuntimeError(f"loss shape mismatch: y{tuple(y.shape)}[:, {lead}:] vs target{tuple(target.shape)}")
        lib = _lib.load()
        loss = torch.empty(1, device=y.device, dtype=torch.float32)
        ws = _ws(lib.mrg_loss_workspace_bytes(B, T, F), y.device)
        _lib.check(lib.mrg_masked_loss_fwd(B, T, F, _ptr(y, lead * F), Ttot * F, _ptr(target), *spec,
                                           _ptr(loss), _ptr(ws), _stream()), "loss fwd")
        ctx.save_for_backward(y, target)
        ctx.lead, ctx.spec = lead, spec
        return loss.view(())

    @staticmethod
    def backward(ctx, gout):
        y, target = ctx.saved_tensors
        B, Ttot, F = y.shape
        T = target.shape[1]
        dy = zeros(y.shape, dtype=y.dtype, device=y.device)
        go = gout.reshape(1).contiguous()
        _lib.check(_lib.load().mrg_masked_loss_bwd(B, T, F, _ptr(y, ctx.lead * F), Ttot * F, _ptr(target),
                                                   *ctx.spec, _ptr(go), _ptr(dy, ctx.lead * F), _stream()),
                   "loss bwd")
        return dy, None, None, None


def masked_loss(y, target, lead=0, loss_type="huber", delta=1.0, beta=1.0, mask_padding=True,
                delta_order=0, delta_loss_scale=1.0):
    """Masked regression loss of the reference training_step on y[:, lead:] vs target."""
    F = y.shape[2]
    spec = (_LOSS_TYPES[loss_type], float(delta), float(beta), int(mask_padding),
            int(F // (delta_order + 1)), float(math.sqrt(delta_loss_scale)))
    return _LossFn.apply(y, target, int(lead), spec)


class _BcastLossFn(Function):
    """Mean loss over the reference's broadcast [Tm, B, T, F] target, analytically."""

    @staticmethod
    def forward(ctx, y, target, ms, spec):
        _lib.require_device(y)
        y, target = y.contiguous(), target.contiguous()
        B, T, F = y.shape
        if tuple(target.shape) != (B, T, F) or ms.shape[0] != B or ms.shape[2] != F or ms.stride(2) != 1:
            raise RuntimeError(f"broadcast loss shapes: y{tuple(y.shape)} target{tuple(target.shape)} "
                               f"motion_self{tuple(ms.shape)}")
        lib = _lib.load()
        loss = torch.empty(1, device=y.device, dtype=torch.float32)
        ws = _ws(lib.mrg_broadcast_loss_workspace_bytes(B, T, F), y.device)
        _lib.check(lib.mrg_broadcast_loss_fwd(B, T, F, _ptr(y), T * F, _ptr(target), _ptr(ms), ms.stride(0),
                                              ms.stride(1), ms.shape[1], *spec, _ptr(loss), _ptr(ws), _stream()),
                   "broadcast loss fwd")
        ctx.save_for_backward(y, target, ms)
        ctx.spec = spec
        return loss.view(())

    @staticmethod
    def backward(ctx, gout):
        y, target, ms = ctx.saved_tensors
        B, T, F = y.shape
        lib = _lib.load()
        dy = torch.empty_like(y)
        ws = _ws(lib.mrg_broadcast_loss_workspace_bytes(B, T, F), y.device)
        go = gout.reshape(1).contiguous()
        _lib.check(lib.mrg_broadcast_loss_bwd(B, T, F, _ptr(y), T * F, _ptr(target), _ptr(ms), ms.stride(0),
                                              ms.stride(1), ms.shape[1], *ctx.spec, _ptr(go), _ptr(dy), _ptr(ws),
                                              _stream()), "broadcast loss bwd")
        return dy, None, None, None


def broadcast_masked_loss(pred, target, motion_self, loss_type="huber", delta=1.0, beta=1.0, scaler=True,
                          delta_order=0, delta_loss_scale=1.0):
    """The loss the reference takes on Metaformer.prediction's output (lstmformer.py:372-380 in the
    scheduled-sampling training_step, :413-418 in generation_step): pred [B, T, F] against
    target * motion_s_mask, which broadcasts to [Tm, B, T, F], mean over all of it.
    motion_self: the raw (-100 padded) self motion [B, Tm, F] the mask comes from.  scaler: the
    training step's sqrt(delta_loss_scale) on the T axis from T // (delta_order + 1)."""
    T = pred.shape[1]
    t_start = T // (delta_order + 1) if scaler else T + 1
    spec = (_LOSS_TYPES[loss_type], float(delta), float(beta), int(t_start),
            float(math.sqrt(delta_loss_scale)) if scaler else 1.0)
    return _BcastLossFn.apply(pred, target, motion_self, spec)


# ------------------------------------------------------------------ per-target metrics
# MultiTargetMetrics' updates (metrics.py): not autograd ops.  The inputs are detached, nothing is allocated
# but _ws workspace, and the accumulators are advanced by the kernels, so the calls may sit inside a captured
# step.  state: float64 [K, 2] on the device ({sum, count} per range); batch_out: float32 [K].
def _metric_ranges(ranges):
    K = len(ranges)
    if not 1 <= K <= 8:
        raise ValueError(f"target metrics: {K} ranges (1..8 supported)")
    arr = ctypes.c_int * K
    return K, arr(*[int(s) for s, _ in ranges]), arr(*[int(e) for _, e in ranges])


def _metric_buffers(y, state, batch_out, K):
    _lib.require_device(y)
    if not (state.is_cuda and state.dtype == torch.float64 and state.is_contiguous() and state.numel() == 2 * K
            and batch_out.is_cuda and batch_out.dtype == torch.float32 and batch_out.is_contiguous()
            and batch_out.numel() == K and state.device == y.device == batch_out.device):
        raise RuntimeError("target metrics: state must be float64 [K, 2] and batch_out float32 [K] on y's device")


def target_metrics_update(y, target, ranges, state, batch_out, lead=0, mask_padding=False, delta_order=0,
                          delta_loss_scale=1.0):
    """state += the squared-error sums / counts of y[:, lead:] vs target over each (start, end) of ranges,
    with masked_loss's padding mask and delta scaler; batch_out = this call's means."""
    y, target = y.detach(), target.detach()
    K, starts, ends = _metric_ranges(ranges)
    _metric_buffers(y, state, batch_out, K)
    if y.dtype != torch.float32 or target.dtype != torch.float32 or target.device != y.device:
        raise RuntimeError("target metrics: float32 tensors on one device required")
    y, target = y.contiguous(), target.contiguous()
    B, Ttot, F = y.shape
    T = target.shape[1]
    if Ttot - lead != T or target.shape[0] != B or target.shape[2] != F:
        raise RuntimeError(f"target metrics shape mismatch: y{tuple(y.shape)}[:, {lead}:] vs "
                           f"target{tuple(target.shape)}")
    lib = _lib.load()
    ws = _ws(lib.mrg_target_metrics_workspace_bytes(B, T, F), y.device)
    _lib.check(lib.mrg_target_metrics_update(B, T, F, _ptr(y, lead * F), Ttot * F, _ptr(target), int(mask_padding),
                                             int(F // (delta_order + 1)), float(math.sqrt(delta_loss_scale)), K,
                                             starts, ends, _ptr(state), _ptr(batch_out), _ptr(ws), _stream()),
               "target metrics update")
    return batch_out


def target_metrics_update_broadcast(pred, target, motion_self, ranges, state, batch_out, scaler=True, delta_order=0,
                                    delta_loss_scale=1.0):
    """The same over the reference's broadcast [Tm, B, T, F] target (broadcast_masked_loss),
    collapsed analytically; range k counts Tm * B * T * (end_k - start_k) elements."""
    pred, target, ms = pred.detach(), target.detach(), motion_self.detach()
    K, starts, ends = _metric_ranges(ranges)
    _metric_buffers(pred, state, batch_out, K)
    if any(t.dtype != torch.float32 or t.device != pred.device for t in (pred, target, ms)):
        raise RuntimeError("target metrics: float32 tensors on one device required")
    pred, target = pred.contiguous(), target.contiguous()
    B, T, F = pred.shape
    if tuple(target.shape) != (B, T, F) or ms.dim() != 3 or ms.shape[0] != B or ms.shape[2] != F or ms.stride(2) != 1:
        raise RuntimeError(f"broadcast metrics shapes: y{tuple(pred.shape)} target{tuple(target.shape)} "
                           f"motion_self{tuple(ms.shape)}")
    t_start = T // (delta_order + 1) if scaler else T + 1
    lib = _lib.load()
    ws = _ws(lib.mrg_target_metrics_workspace_bytes(B, T, F), pred.device)
    _lib.check(lib.mrg_target_metrics_update_broadcast(
        B, T, F, _ptr(pred), T * F, _ptr(target), _ptr(ms), ms.stride(0), ms.stride(1), ms.shape[1], int(t_start),
        float(math.sqrt(delta_loss_scale)) if scaler else 1.0, K, starts, ends, _ptr(state), _ptr(batch_out),
        _ptr(ws), _stream()), "target metrics update (broadcast)")
    return batch_out
