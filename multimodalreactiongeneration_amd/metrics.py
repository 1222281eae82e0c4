"""Per-target MSE metrics on the device: the reference's ``MultiTargetMetrics``
(mr_gen/utils/metrics/multi_modal_metrics.py:6-56), a torchmetrics ``MetricCollection`` of one
``MeanSquaredError`` per column slice of the pose vector (``gen_target_dict``: centroid, angle, delta1-*,
delta2-*), without torchmetrics and without torch math on the update path.

One module holds every slice: ``{sum of squared errors, element count}`` per slice in float64 device memory,
advanced by the library's kernels (csrc/metrics.hip, ``functional.target_metrics_update*``).  An update neither
allocates (beyond kernel workspace) nor synchronises with the host, so it may sit inside a captured step and a
replayed HIP graph keeps accumulating.  The state follows ``.to(device)`` and is never in ``state_dict()`` (the
reference's metric states are non-persistent too).
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch
from torch import nn

from . import functional as Fn


class MultiTargetMetrics(nn.Module):
    """``target_range``: {name: (start, end)} column slices of the last axis (end = -1: to the end; at most 8;
    slices may overlap).  Keys of ``compute()`` are ``prefix + name + postfix`` in ``target_range`` order."""

    def __init__(self, target_range: Dict[str, Tuple[int, int]], prefix: Optional[str] = None,
                 postfix: Optional[str] = None):
        super().__init__()
        if not 1 <= len(target_range) <= 8:
            raise ValueError(f"MultiTargetMetrics: {len(target_range)} target ranges (1..8 supported)")
        self.target_range = dict(target_range)
        self.prefix, self.postfix = prefix, postfix
        self._ranges = [(int(s), int(e)) for s, e in self.target_range.values()]
        K = len(self._ranges)
        # the float64 state is kept as its int64 bit pattern: Module.float() / .half() / .to(dtype) cast
        # floating-point buffers only, and an accumulator must not lose its precision to a model-wide cast
        self.register_buffer("_state_bits", torch.zeros(K, 2, dtype=torch.int64), persistent=False)
        self.register_buffer("_batch", torch.zeros(K, dtype=torch.float32), persistent=False)
        self._issued = 0         # updates issued from the host since the last reset()
        self._captured = False   # an update was recorded into a HIP graph: replays accumulate unseen by the host

    # ------------------------------------------------------------------ state
    @property
    def state(self) -> torch.Tensor:
        """float64 [K, 2] = {sum of squared errors, element count} per range (a view: writable in place)."""
        return self._state_bits.view(torch.float64)

    def keys(self):
        pre, post = self.prefix or "", self.postfix or ""
        return [pre + name + post for name in self.target_range]

    def reset(self) -> None:
        if self._state_bits.is_cuda:
            Fn.zero_(self._state_bits)
        else:
            self._state_bits.zero_()
        self._issued = 0

    def _note_update(self):
        self._issued += 1
        if torch.cuda.is_current_stream_capturing():
            self._captured = True

    # ------------------------------------------------------------------ updates
    def update(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        """torchmetrics' ``update(preds, target)``: same-shape float32 tensors, any leading dimensions."""
        if preds.shape != target.shape or preds.dim() < 1:
            raise RuntimeError(f"MultiTargetMetrics.update: shapes {tuple(preds.shape)} vs {tuple(target.shape)}")
        F = preds.shape[-1]
        Fn.target_metrics_update(preds.reshape(1, -1, F), target.reshape(1, -1, F), self._ranges, self.state,
                                 self._batch)
        self._note_update()

    def update_masked(self, y, target, lead=0, mask_padding=True, delta_order=0, delta_loss_scale=1.0) -> None:
        """The quantities ``functional.masked_loss`` sees: y[:, lead:] vs target under the -100 padding mask
        and the sqrt(delta_loss_scale) scaler on the delta features."""
        Fn.target_metrics_update(y, target, self._ranges, self.state, self._batch, lead, mask_padding, delta_order,
                                 delta_loss_scale)
        self._note_update()

    def update_broadcast(self, pred, target, motion_self, scaler=True, delta_order=0, delta_loss_scale=1.0) -> None:
        """The quantities ``functional.broadcast_masked_loss`` sees: the reference's [Tm, B, T, F] broadcast
        target of the generation paths, never materialised."""
        Fn.target_metrics_update_broadcast(pred, target, motion_self, self._ranges, self.state, self._batch, scaler,
                                           delta_order, delta_loss_scale)
        self._note_update()

    def forward(self, preds: torch.Tensor, target: torch.Tensor) -> Dict[str, torch.Tensor]:
        """Accumulate, and return this batch's values alone (torchmetrics' ``forward``)."""
        self.update(preds, target)
        batch = self._batch.clone()
        return {k: batch[i] for i, k in enumerate(self.keys())}

    # ------------------------------------------------------------------ results
    def compute(self) -> Dict[str, torch.Tensor]:
        """{key: 0-dim float32 tensor on the state's device}, without a host synchronisation.  Under an
        initialised torch.distributed the states of all ranks are summed first (torchmetrics'
        dist_reduce_fx="sum").  Raises when nothing has been accumulated: no update since construction or
        reset() (and none recorded into a HIP graph, whose replays the host cannot see), or, for a state in
        host memory, zero counts."""
        state = self.state
        if state.is_cuda:
            empty = self._issued == 0 and not self._captured
        else:
            empty = self._issued == 0 and not bool((state[:, 1] != 0).any())
        if empty:
            raise RuntimeError("MultiTargetMetrics.compute() before any update()")
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            state = state.clone()
            dist.all_reduce(state, op=dist.ReduceOp.SUM)
        values = (state[:, 0] / state[:, 1]).to(torch.float32)
        return {k: values[i] for i, k in enumerate(self.keys())}

    def items(self):
        """(key, value) pairs of ``compute()``."""
        return self.compute().items()

    def extra_repr(self):
        return f"keys={self.keys()}"
