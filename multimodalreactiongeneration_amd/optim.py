"""Fused AdamW and SGD over one flat parameter buffer (one libmrg launch per step).

Stand in for ``torch.optim.AdamW(self.parameters(), lr, weight_decay)`` and
``torch.optim.SGD(self.parameters(), lr, momentum, weight_decay)`` of
``configure_optimizers`` (lstmformer.py:327-342, lstm_with_sample.py:248-263,
simple_lstm.py:193-208).  On construction every parameter is re-pointed into a
contiguous fp32 buffer and its ``.grad`` into a twin gradient buffer, so
``step()`` is a single kernel, ``zero_grad()`` a single memset and the DDP
reducer (``ddp.GradReducer``) all-reduces the gradient buffer in place.
They subclass ``torch.optim.Optimizer`` so torch LR schedulers
(CosineAnnealingLR) drive ``param_groups[0]['lr']``: the group is a dict whose
``'lr'`` assignment also writes the device-side LR the kernel reads, so a
scheduler stepped between HIP-graph replays takes effect in the replayed step.

Error surfacing: the persistent LSTM kernels OR a device flag on a hand-off
timeout; the update kernel reads it and skips the update (garbage gradients never
reach the weights, replayed graphs included), and ``step()`` raises at the next
step once the flag, copied to pinned host memory without a sync, reads non-zero.

Gradient accumulation (Lightning's ``accumulate_grad_batches = n``): a window is ``n`` consecutive
``step()`` calls with a backward pass before each and no ``zero_grad()`` in between, so the gradients sum
in ``flat_grad``.  Calls 1 .. n-1 change nothing but a micro-step counter on the device; call n takes the
mean, clips it, updates, zeroes ``flat_grad`` and counts one step.  The counter sits beside ``step_lr``
and the kernels branch on it themselves, so one captured ``step()`` replays a whole window correctly.

Checkpoints: ``state_dict()`` / ``load_state_dict()`` speak the layout of the torch
optimizer of the same name (per-parameter entries keyed by the parameter's index),
sliced out of / copied into the flat buffers, so a Lightning ``optimizer_states``
entry written by either side resumes on the other.
"""
from __future__ import annotations

from typing import Iterable

import torch

from . import _lib
from .launch import _err_flag, _ptr, _stream


def flatten_parameters(params, device=None):
    """Move parameters into one contiguous buffer; returns (flat_params, flat_grads, params)."""
    params = [p for p in params if p.requires_grad]
    if not params:
        raise ValueError("no trainable parameters")
    device = device or params[0].device
    n = sum(p.numel() for p in params)
    flat = torch.empty(n, dtype=torch.float32, device=device)
    gflat = torch.zeros(n, dtype=torch.float32, device=device)
    off = 0
    for p in params:
        k = p.numel()
        flat[off:off + k].copy_(p.detach().reshape(-1))
        p.data = flat[off:off + k].view_as(p)
        p.grad = gflat[off:off + k].view_as(p)
        off += k
    return flat, gflat, params


def _check_clipping(val, algorithm):
    if algorithm not in ("norm", "value"):
        raise ValueError(f"gradient_clip_algorithm {algorithm!r}: 'norm' or 'value'")
    if val is not None and not float(val) >= 0:
        raise ValueError(f"gradient_clip_val {val!r}: None, 0 (off) or a positive number")


def _check_accumulation(n):
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError(f"accumulate_grad_batches {n!r}: an int >= 1")


class _LRGroup(dict):
    """A param group whose 'lr' assignment (LR schedulers) is mirrored to the device buffer."""

    def __init__(self, group, opt):
        super().__init__(group)
        self._opt = opt

    def __setitem__(self, k, v):
        super().__setitem__(k, v)
        if k == "lr" and getattr(self, "_opt", None) is not None:
            self._opt._write_lr(v)


class _FlatOptimizer(torch.optim.Optimizer):
    """What the fused optimizers share: the flat parameter / gradient buffers, the device-side
    {completed steps, lr} pair, the asynchronous error check and the torch-layout state_dict.

    A subclass names its update (``_UPDATE``, for the error message), lists its per-parameter state
    (``_moments()``: torch's state key -> flat buffer) and refuses group options its kernel does not
    implement (``_check_group``)."""

    _UPDATE = ""

    def __init__(self, params: Iterable, defaults, gradient_clip_val=None, gradient_clip_algorithm="norm",
                 accumulate_grad_batches=1):
        params = list(params)
        _check_clipping(gradient_clip_val, gradient_clip_algorithm)   # before the parameters are re-pointed
        _check_accumulation(accumulate_grad_batches)
        super().__init__(params, defaults)
        if len(self.param_groups) != 1:
            raise ValueError(f"{type(self).__name__} takes one param group (one flat buffer, one device-side LR)")
        self._check_group(self.param_groups[0])
        self._all = list(self.param_groups[0]["params"])   # frozen parameters included: torch's indices
        self.flat, self.flat_grad, self.plist = flatten_parameters(self._all)
        lr = float(self.param_groups[0]["lr"])
        self.step_lr = torch.tensor([0.0, lr], dtype=torch.float32, device=self.flat.device)
        self._lr_on_device = lr
        self._wrap_groups()
        self._err_host = self._err_event = None
        self.clip_state = self._clip_ws = None
        self.set_gradient_clipping(gradient_clip_val, gradient_clip_algorithm)
        self.accum_state = None
        self.set_accumulation(accumulate_grad_batches)

    # ---- gradient accumulation (Lightning's trainer.accumulate_grad_batches).  An attribute of the
    # optimizer like clipping: not a group option, not in state_dict(), left alone by load_state_dict().
    def set_accumulation(self, n):
        """Update once per window of ``n`` ``step()`` calls, on the mean of the gradients the backward passes
        of the window summed into ``flat_grad`` (1: every call updates, the default).  ``step()`` zeroes
        ``flat_grad`` when it closes a window; calling ``zero_grad()`` inside a window discards the
        micro-batches summed so far and is not checked for.  Changing ``n`` restarts the window.  The device
        counter is allocated here, never in ``step()``, so call it before a step is captured into a graph."""
        _check_accumulation(n)
        if self.flat.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("set_accumulation inside a graph capture: a captured step holds the "
                               "launches it was recorded with; set it before graphs.capture")
        self.accumulate_grad_batches = n
        self._micro_host = 0   # the host's count of step() calls in the window (ddp.GradReducer reads it)
        if n > 1 or self.accum_state is not None:   # once allocated it stays: a captured step may hold its address
            state = torch.tensor([0, n], dtype=torch.int32)
            if self.accum_state is None:
                self.accum_state = state.to(self.flat.device)
            else:
                self.accum_state.copy_(state)

    @property
    def micro_step(self):
        """0-d device view: the step() calls made in the current window, 0 .. n-1 (no sync)."""
        if self.accum_state is None:
            raise RuntimeError("micro_step: accumulation is off (accumulate_grad_batches=1)")
        return self.accum_state[0]

    def closes_window(self):
        """Whether the next ``step()`` updates (True without accumulation).  Counted on the host from the
        ``step()`` calls made here, for what the host has to decide itself (the DDP all-reduce); a step
        that was captured into a graph advances the device counter only, and then this refuses."""
        if self.accumulate_grad_batches == 1:
            return True
        if self._micro_host is None:
            raise RuntimeError("accumulate_grad_batches > 1 with a step() captured into a graph: the host "
                               "cannot tell which replay closes a window (ddp.GradReducer needs an eager "
                               "step(); call set_accumulation to start over)")
        return self._micro_host == self.accumulate_grad_batches - 1

    def _accum_begin(self):
        """An accumulating step: clip launches first, then what the update has to know about the 1 / n
        (prescaled, clip_state) as mrg_*_step_accum takes it.  Advances the host's mirror."""
        if self.flat.is_cuda and torch.cuda.is_current_stream_capturing():
            self._micro_host = None
        elif self._micro_host is not None:
            self._micro_host = (self._micro_host + 1) % self.accumulate_grad_batches
        if not self.gradient_clip_val:
            return 0, None
        from . import functional as Fn
        if self.gradient_clip_algorithm == "norm":
            Fn.clip_grad_norm_(self.flat_grad, self.gradient_clip_val, self.clip_state, self._clip_ws,
                               accum=self.accum_state)
            return 0, self.clip_state
        Fn.clip_grad_value_(self.flat_grad, self.gradient_clip_val, accum=self.accum_state)
        return 1, None

    def _state_tensors(self, *tensors):
        return [t for t in tensors + (self.accum_state,) if t is not None]

    # ---- gradient clipping (Lightning's trainer.gradient_clip_val / gradient_clip_algorithm).  Attributes
    # of the optimizer, as they are the Trainer's there: not a group option, not in state_dict().
    def set_gradient_clipping(self, val, algorithm="norm"):
        """Clip ``flat_grad`` in ``step()``, just before the update: to a total 2-norm of ``val``
        (``"norm"``: torch.nn.utils.clip_grad_norm_) or elementwise to [-val, val] (``"value"``).  ``None`` or
        0 switches it off; ``inf`` with ``"norm"`` only measures (``grad_norm``).  The device buffers are
        allocated here, never in ``step()``, so call it before a step is captured into a graph."""
        _check_clipping(val, algorithm)
        if self.flat.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("set_gradient_clipping inside a graph capture: a captured step holds the "
                               "launches it was recorded with; set it before graphs.capture")
        self.gradient_clip_val = None if val is None else float(val)
        self.gradient_clip_algorithm = algorithm
        if self._norm_clipping():   # once allocated the buffers stay: a captured step may hold their addresses
            if self.clip_state is None:
                self.clip_state = torch.tensor([0.0, 1.0], dtype=torch.float32, device=self.flat.device)
            if self._clip_ws is None and self.flat.is_cuda:
                from . import functional as Fn
                self._clip_ws = Fn.clip_grad_workspace(self.flat_grad.numel(), self.flat.device)

    def _norm_clipping(self):
        return bool(self.gradient_clip_val) and self.gradient_clip_algorithm == "norm"

    def _clip_view(self, i, what):
        if not self._norm_clipping():
            raise RuntimeError(f"{what}: norm clipping is off (gradient_clip_val={self.gradient_clip_val!r}, "
                               f"gradient_clip_algorithm={self.gradient_clip_algorithm!r})")
        return self.clip_state[i]

    @property
    def grad_norm(self):
        """0-d device view: the total gradient norm the last step saw, before clipping (no sync)."""
        return self._clip_view(0, "grad_norm")

    @property
    def grad_clip_coef(self):
        """0-d device view: the coefficient the last step multiplied the gradients by (1: not clipped)."""
        return self._clip_view(1, "grad_clip_coef")

    def _clip_gradients(self):
        """Issued between _begin_step() and the update launch: every gradient write (side streams, the DDP
        all-reduce) is ordered before that point already."""
        from . import functional as Fn
        if self.gradient_clip_algorithm == "norm":
            Fn.clip_grad_norm_(self.flat_grad, self.gradient_clip_val, self.clip_state, self._clip_ws)
        else:
            Fn.clip_grad_value_(self.flat_grad, self.gradient_clip_val)

    def _check_group(self, group):
        pass

    def _moments(self):
        return {}

    def _wrap_groups(self):
        self.param_groups[0] = _LRGroup(self.param_groups[0], self)

    def _write_lr(self, lr):
        lr = float(lr)
        if lr != self._lr_on_device:
            self.step_lr[1].fill_(lr)  # stream-ordered: lands before the next (replayed) step
            self._lr_on_device = lr

    def _check_async(self):
        """Raise if an earlier step's persistent kernels reported a hand-off timeout (no sync: the
        flag is copied to pinned memory each step and read once that copy has completed)."""
        if not self.flat.is_cuda or torch.cuda.is_current_stream_capturing():
            return  # (no event queries inside a capture; replays are checked by check_errors())
        err = _err_flag(self.flat.device)
        if self._err_host is None:
            self._err_host = torch.zeros(1, dtype=torch.int32, pin_memory=True)
            self._err_event = torch.cuda.Event()
        elif self._err_event.query() and int(self._err_host[0]) != 0:
            self._err_host.zero_()
            err.zero_()
            raise RuntimeError("libmrg: LSTM recurrence hand-off timed out (grid not co-resident?); "
                               f"the {self._UPDATE} update of that step was skipped")
        self._err_host.copy_(err, non_blocking=True)
        self._err_event.record()

    def _begin_step(self):
        """The param group of this step, after the LR write and the error check every step starts with."""
        _lib.require_device(self.flat)
        g = self.param_groups[0]
        self._write_lr(g["lr"])
        self._check_async()
        return g

    def _end_step(self):
        from . import functional as Fn
        Fn.invalidate_weight_planes()  # the weights changed: their bf16 planes are stale

    def zero_grad(self, set_to_none: bool = False):
        # gradients stay views of the flat buffer (set_to_none would detach them from it)
        if self.flat_grad.is_cuda:
            from . import functional as Fn
            Fn.zero_(self.flat_grad)
        else:
            self.flat_grad.zero_()

    # ---- state in torch's layout
    def _slices(self):
        """(index among all parameters passed in, offset into the flat buffers, parameter) per trainable one."""
        out, off = [], 0
        for i, p in enumerate(self._all):
            if p.requires_grad:
                out.append((i, off, p))
                off += p.numel()
        return out

    def _entry(self, steps, tensors):
        """One parameter's state entry from its slices of _moments() (torch's keys, torch's order)."""
        return tensors

    def state_dict(self):
        sd = super().state_dict()   # param_groups with indices over every parameter; self.state is empty
        steps = float(self.step_lr[0])   # one device read: a checkpoint-time call, never inside a capture
        moments = self._moments()
        state = {}
        if steps > 0 and moments:
            for i, off, p in self._slices():
                state[i] = self._entry(steps, {k: buf[off:off + p.numel()].clone().view(p.shape)
                                               for k, buf in moments.items()})
        sd["state"] = state
        return sd

    def _steps_of(self, entries):
        """The completed-step count a loaded state stands for (entries: index -> {key: tensor})."""
        raise NotImplementedError

    def load_state_dict(self, state_dict):
        groups = state_dict["param_groups"]
        if len(groups) != 1:
            raise ValueError("loaded state dict has a different number of parameter groups")
        merged = dict(self.defaults)
        merged.update(groups[0])
        self._check_group(merged)
        slices = {i: (off, p) for i, off, p in self._slices()}
        keys = list(self._moments_for(merged))
        entries = {}
        for k, st in state_dict["state"].items():
            tensors = {name: st[name] for name in keys if st.get(name) is not None}
            if not tensors and "step" not in st:
                continue   # torch.optim.SGD without momentum leaves empty entries
            i = int(k)
            if i not in slices:
                raise ValueError(f"optimizer state for parameter {i}, which is not a trainable parameter here")
            if len(tensors) != len(keys):
                raise ValueError(f"optimizer state of parameter {i} lacks {sorted(set(keys) - set(tensors))}")
            for name, t in tensors.items():
                if tuple(t.shape) != tuple(slices[i][1].shape):
                    raise ValueError(f"optimizer state {name!r} of parameter {i} has shape {tuple(t.shape)}, "
                                     f"the parameter {tuple(slices[i][1].shape)}")
            entries[i] = dict(st)
        steps = self._steps_of(entries)
        # everything is checked: now the groups (torch restores them), then the flat buffers in place
        super().load_state_dict({"state": {}, "param_groups": [merged]})
        self._wrap_groups()
        self._write_lr(self.param_groups[0]["lr"])
        self._fit_moments(self.param_groups[0])
        with torch.no_grad():
            for name, buf in self._moments().items():
                buf.zero_()
                for i, st in entries.items():
                    off, p = slices[i]
                    buf[off:off + p.numel()].copy_(st[name].detach().reshape(-1))
            self.step_lr[0].fill_(float(steps))

    def _moments_for(self, group):
        """The state keys a param group with these options carries."""
        return self._moments()

    def _fit_moments(self, group):
        """Make the moment buffers fit a freshly loaded group."""


class FusedAdamW(_FlatOptimizer):
    _UPDATE = "AdamW"

    def __init__(self, params: Iterable, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                 gradient_clip_val=None, gradient_clip_algorithm="norm", accumulate_grad_batches=1):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False,
                                      maximize=False, decoupled_weight_decay=True),
                         gradient_clip_val, gradient_clip_algorithm, accumulate_grad_batches)
        self.exp_avg = torch.zeros_like(self.flat)
        self.exp_avg_sq = torch.zeros_like(self.flat)

    def _check_group(self, group):
        if group.get("amsgrad") or group.get("maximize") or not group.get("decoupled_weight_decay", True):
            raise ValueError("FusedAdamW implements torch.optim.AdamW without amsgrad / maximize")

    def _moments(self):
        return {"exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq}

    def _entry(self, steps, tensors):
        return {"step": torch.tensor(steps, dtype=torch.float32), **tensors}

    def _steps_of(self, entries):
        if any("step" not in st for st in entries.values()):
            raise ValueError("FusedAdamW: a state entry has moments but no 'step'")
        steps = {float(st["step"]) for st in entries.values()}
        if len(steps) > 1:
            raise ValueError(f"FusedAdamW keeps one step count for all parameters; the state has {sorted(steps)}")
        return steps.pop() if steps else 0.0

    def state_tensors(self):
        """Device state one update changes (graphs.capture(preserve=...) restores it after warm-up)."""
        return self._state_tensors(self.flat, self.exp_avg, self.exp_avg_sq, self.step_lr)

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        g = self._begin_step()
        b1, b2 = g["betas"]
        if self.accumulate_grad_batches > 1:
            prescaled, clip_state = self._accum_begin()
            _lib.check(_lib.load().mrg_adamw_step_accum(
                _ptr(self.flat), _ptr(self.flat_grad), _ptr(self.exp_avg), _ptr(self.exp_avg_sq),
                self.flat.numel(), _ptr(self.step_lr), float(g["weight_decay"]), float(b1), float(b2),
                float(g["eps"]), _ptr(_err_flag(self.flat.device)), _ptr(self.accum_state), prescaled,
                _ptr(clip_state), _stream()), "adamw (accumulation)")
            self._end_step()
            return loss
        if self.gradient_clip_val:
            self._clip_gradients()
        _lib.check(_lib.load().mrg_adamw_step(
            _ptr(self.flat), _ptr(self.flat_grad), _ptr(self.exp_avg), _ptr(self.exp_avg_sq),
            self.flat.numel(), _ptr(self.step_lr), float(g["weight_decay"]), float(b1), float(b2),
            float(g["eps"]), _ptr(_err_flag(self.flat.device)), _stream()), "adamw")
        self._end_step()
        return loss


class FusedSGD(_FlatOptimizer):
    """torch.optim.SGD(lr, momentum, weight_decay) with dampening = 0 and nesterov = False (mrg_sgd_step)."""

    _UPDATE = "SGD"

    def __init__(self, params: Iterable, lr, momentum=0.0, weight_decay=0.0, dampening=0.0, nesterov=False,
                 maximize=False, gradient_clip_val=None, gradient_clip_algorithm="norm", accumulate_grad_batches=1):
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                      nesterov=nesterov, maximize=maximize),
                         gradient_clip_val, gradient_clip_algorithm, accumulate_grad_batches)
        self.momentum_buf = None
        self._fit_moments(self.param_groups[0])

    def _check_group(self, group):
        if group.get("dampening") or group.get("nesterov") or group.get("maximize"):
            raise ValueError("FusedSGD implements torch.optim.SGD without dampening / nesterov / maximize")
        if group["momentum"] < 0 or group["weight_decay"] < 0:
            raise ValueError(f"FusedSGD: negative momentum {group['momentum']} or weight_decay "
                             f"{group['weight_decay']}")

    def _moments(self):
        return {} if self.momentum_buf is None else {"momentum_buffer": self.momentum_buf}

    def _moments_for(self, group):
        return ["momentum_buffer"] if group["momentum"] != 0 else []

    def _fit_moments(self, group):
        if group["momentum"] == 0:
            self.momentum_buf = None
        elif self.momentum_buf is None:
            self.momentum_buf = torch.zeros_like(self.flat)

    def _steps_of(self, entries):
        return 1.0 if entries else 0.0   # the kernel only asks whether the buffer has been seeded

    def state_tensors(self):
        """Device state one update changes (graphs.capture(preserve=...) restores it after warm-up)."""
        return self._state_tensors(self.flat, self.momentum_buf, self.step_lr)

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        g = self._begin_step()
        if self.accumulate_grad_batches > 1:
            prescaled, clip_state = self._accum_begin()
            _lib.check(_lib.load().mrg_sgd_step_accum(
                _ptr(self.flat), _ptr(self.flat_grad), _ptr(self.momentum_buf), self.flat.numel(),
                _ptr(self.step_lr), float(g["weight_decay"]), float(g["momentum"]),
                _ptr(_err_flag(self.flat.device)), _ptr(self.accum_state), prescaled, _ptr(clip_state),
                _stream()), "sgd (accumulation)")
            self._end_step()
            return loss
        if self.gradient_clip_val:
            self._clip_gradients()
        _lib.check(_lib.load().mrg_sgd_step(
            _ptr(self.flat), _ptr(self.flat_grad), _ptr(self.momentum_buf), self.flat.numel(),
            _ptr(self.step_lr), float(g["weight_decay"]), float(g["momentum"]),
            _ptr(_err_flag(self.flat.device)), _stream()), "sgd")
        self._end_step()
        return loss
