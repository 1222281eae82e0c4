"""Scheduled-sampling training of the lstmformer in dependence levels instead of frames.

Reference: Metaformer.training_step with use_scheduled_sampling (lstmformer.py:357-385) ->
head_motion_generation (:466-521).  Generation is stateless: every frame is a T = 1 forward
from zero recurrent state whose rows are independent, and the only thing frame t >= 1 takes from another
frame is its self-motion input, ``mask[t-1] ? y(t-1) : ms[t-1]`` (frame 0 reads ms[0]).  So a frame depends
on its predecessor only inside a run of sampled frames.  With

    depth[0] = 0,    depth[t] = mask[t-1] ? depth[t-1] + 1 : 0

all frames of one depth are independent given the outputs of the depth below, and they run as ONE forward
of [n_d * B] samples with T = 1 through the same autograd ops the per-frame path uses.  The model is called
max(depth) + 1 times over the same T * B rows in total: once at sampling rate 0, about 8 times at rate 0.5
and T = 300, T times only for an all-sampled mask (which keeps the per-frame loop).

``plan_levels`` is the host planner, ``generate_levels`` the schedule, and ``gather`` / ``scatter`` /
``level_input`` the differentiable frame moves (ss_levels.hip: one launch each, no atomics).
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional

import numpy as np
import torch
from torch.autograd import Function

from . import _lib
from .launch import _ptr, _stream, zeros

I32 = np.int32
# rows (frames x batch) one forward may take; None: derived from the model (rows_cap_for).  Tests force a
# small one here to make the planner chunk.
_ROWS_CAP: List[Optional[int]] = [None]


class Level(NamedTuple):
    """The frames of one depth (or one chunk of them) as one forward."""
    depth: int
    frames: np.ndarray    # int32, ascending frame indices
    teacher: np.ndarray   # int32, max(t - 1, 0) per frame: the ms row a teacher-forced frame reads
    prev: np.ndarray      # int32, position of frame t - 1 in the previous depth's frames (all its chunks
                          # concatenated in order), or -1 when the frame reads the teacher


def plan_levels(mask, rows_cap: Optional[int] = None, B: int = 1) -> List[Level]:
    """mask: host bool [T].  One Level per depth, in depth order; a depth whose len(frames) * B exceeds
    rows_cap is split into consecutive chunks of at most max(1, rows_cap // B) frames."""
    m = np.asarray(mask.cpu() if torch.is_tensor(mask) else mask).astype(bool).reshape(-1)
    T = m.shape[0]
    by_depth: List[List[int]] = []
    d = 0
    for t in range(T):
        d = d + 1 if (t and m[t - 1]) else 0
        if d == len(by_depth):
            by_depth.append([])
        by_depth[d].append(t)
    per = None if rows_cap is None else max(1, int(rows_cap) // max(1, int(B)))
    levels, where = [], {}
    for d, frames in enumerate(by_depth):
        prev = [where[t - 1] if d else -1 for t in frames]
        where = {t: i for i, t in enumerate(frames)}
        step = len(frames) if per is None else per
        for s in range(0, len(frames), step):
            f = np.asarray(frames[s:s + step], dtype=I32)
            levels.append(Level(d, f, np.maximum(f - 1, 0).astype(I32), np.asarray(prev[s:s + step], dtype=I32)))
    return levels


def rows_cap_for(model, device) -> Optional[int]:
    """At ratio > 1 the audio stack of a level is a persistent recurrence over n * B sequences of r steps,
    whose grid must be resident: generate._RECURRENCE holds the sequences one launch takes per 8 CUs.  At
    ratio 1 every recurrent layer sees T = 1 and takes the cell / GEMM path (recurrent.lstm_layer), which has
    no such limit."""
    if _ROWS_CAP[0] is not None:
        return _ROWS_CAP[0]
    if model.ratio == 1:
        return None
    from .generate import _RECURRENCE
    entry = _RECURRENCE.get(model.other_mixer_type[0])
    if entry is None:
        return None
    return entry[1] * max(1, _lib.cu_count(torch.device(device).index or 0) // 8)


# ------------------------------------------------------------------ the frame moves
class Index(NamedTuple):
    """Frame indices on both sides: the host copy is what gets range-checked, the device copy is what the
    kernels read."""
    host: np.ndarray
    dev: torch.Tensor
    distinct: bool        # no non-negative value twice


def as_index(idx, device) -> Index:
    if isinstance(idx, Index):
        return idx
    host = np.ascontiguousarray(np.asarray(idx.cpu() if torch.is_tensor(idx) else idx).reshape(-1), dtype=I32)
    used = host[host >= 0]
    return Index(host, torch.from_numpy(host).to(device), len(np.unique(used)) == len(used))


def _within(ix: Index, lo: int, hi: int, what: str):
    if ix.host.size and (int(ix.host.min()) < lo or int(ix.host.max()) >= hi):
        raise IndexError(f"{what}: index outside [{lo}, {hi})")


def _frames3(x: torch.Tensor, what: str) -> torch.Tensor:
    _lib.require_device(x)
    if x.dim() != 3 or x.dtype != torch.float32:
        raise ValueError(f"{what}: a float32 [frames, B, W] tensor required, got {tuple(x.shape)} {x.dtype}")
    return x.contiguous()


def _run_gather(src, ix: Index):
    _, B, W = src.shape
    n = ix.host.size
    out = torch.empty(n, B, W, device=src.device, dtype=torch.float32)
    _lib.check(_lib.load().mrg_frame_gather(n, B, W, _ptr(src), _ptr(ix.dev), _ptr(out), _stream()), "frame gather")
    return out


def _run_scatter(src, ix: Index, dst):
    n, B, W = src.shape
    _lib.check(_lib.load().mrg_frame_scatter(n, B, W, _ptr(src), _ptr(ix.dev), _ptr(dst), _stream()),
               "frame scatter")


class _GatherFn(Function):
    @staticmethod
    def forward(ctx, src, ix):
        ctx.ix, ctx.shape = ix, src.shape
        return _run_gather(src, ix)

    @staticmethod
    def backward(ctx, dout):
        if not ctx.ix.distinct:
            raise RuntimeError("ss_levels.gather: the gradient needs distinct indices (a level's frames are)")
        dsrc = zeros(*ctx.shape, device=dout.device)
        _run_scatter(dout.contiguous(), ctx.ix, dsrc)
        return dsrc, None


class _ScatterFn(Function):
    @staticmethod
    def forward(ctx, buf, src, ix):
        ctx.ix = ix
        _run_scatter(src, ix, buf)
        ctx.mark_dirty(buf)
        return buf

    @staticmethod
    def backward(ctx, dout):
        # the frames named by ix held nothing differentiable before (scatter's contract), so the buffer's
        # own gradient passes through as it is
        dout = dout.contiguous()
        return dout, _run_gather(dout, ctx.ix), None


class _LevelInputFn(Function):
    @staticmethod
    def forward(ctx, y_prev, ms, prev, teacher, inv):
        ctx.inv = inv
        _, B, W = ms.shape
        n = prev.host.size
        out = torch.empty(n, B, W, device=ms.device, dtype=torch.float32)
        _lib.check(_lib.load().mrg_level_input(n, B, W, _ptr(y_prev), _ptr(prev.dev), _ptr(ms), _ptr(teacher.dev),
                                               _ptr(out), _stream()), "level input")
        return out

    @staticmethod
    def backward(ctx, dout):
        # row block j of the previous level: the gradient of the one consumer that names it, or zero
        if ctx.inv is None:   # depth 0: no previous level
            return None, None, None, None, None
        dout = dout.contiguous()
        _, B, W = dout.shape
        m = ctx.inv.host.size
        dy = torch.empty(m, B, W, device=dout.device, dtype=torch.float32)
        _lib.check(_lib.load().mrg_level_input(m, B, W, _ptr(dout), _ptr(ctx.inv.dev), None, None, _ptr(dy),
                                               _stream()), "level input bwd")
        return dy, None, None, None, None


def gather(src: torch.Tensor, idx) -> torch.Tensor:
    """out[i] = src[idx[i]] for time-major src [T, B, W].  Differentiable in src when the indices are
    distinct (the gradient is then a scatter into zeros; repeated indices raise in backward)."""
    src = _frames3(src, "ss_levels.gather")
    ix = as_index(idx, src.device)
    _within(ix, 0, src.shape[0], "ss_levels.gather")
    return _GatherFn.apply(src, ix)


def scatter(buf: torch.Tensor, src: torch.Tensor, idx) -> torch.Tensor:
    """buf[idx[i]] = src[i], in place, returns buf.  idx must be distinct.  Differentiable in src; the frames
    named by idx must not hold the result of an earlier differentiable write (the schedule writes every
    frame once), so buf's own gradient passes through unchanged."""
    src = _frames3(src, "ss_levels.scatter")
    ix = as_index(idx, src.device)
    _lib.require_device(buf)
    if not (buf.dim() == 3 and buf.is_contiguous() and buf.dtype == torch.float32 and buf.shape[1:] == src.shape[1:]):
        raise ValueError("ss_levels.scatter: buf must be a contiguous float32 [T, B, W] matching src")
    if ix.host.size != src.shape[0] or not ix.distinct:
        raise ValueError("ss_levels.scatter: one distinct index per source frame required")
    _within(ix, 0, buf.shape[0], "ss_levels.scatter")
    return _ScatterFn.apply(buf, src, ix)


def level_input(y_prev: Optional[torch.Tensor], prev, ms: torch.Tensor, teacher, inv=None) -> torch.Tensor:
    """out[i] = prev[i] >= 0 ? y_prev[prev[i]] : ms[teacher[i]].  Differentiable in y_prev: its gradient is
    read through ``inv``, the inverse of prev over y_prev's frames (computed here when not given).  y_prev may
    be None when every prev is -1 (depth 0)."""
    ms = _frames3(ms, "ss_levels.level_input")
    prev, teacher = as_index(prev, ms.device), as_index(teacher, ms.device)
    if prev.host.size != teacher.host.size or not prev.distinct:
        raise ValueError("ss_levels.level_input: prev and teacher of one length, prev without repeats")
    _within(teacher, 0, ms.shape[0], "ss_levels.level_input teacher")
    if y_prev is None:
        _within(prev, -1, 0, "ss_levels.level_input prev (no y_prev)")
        return _LevelInputFn.apply(None, ms, prev, teacher, None)
    y_prev = _frames3(y_prev, "ss_levels.level_input")
    if y_prev.shape[1:] != ms.shape[1:]:
        raise ValueError("ss_levels.level_input: y_prev and ms frames of one shape required")
    _within(prev, -1, y_prev.shape[0], "ss_levels.level_input prev")
    if inv is None:
        inv = inverse_map(prev.host, y_prev.shape[0])
    inv = as_index(inv, ms.device)
    if inv.host.size != y_prev.shape[0]:
        raise ValueError("ss_levels.level_input: inv must have one entry per y_prev frame")
    _within(inv, -1, prev.host.size, "ss_levels.level_input inv")
    return _LevelInputFn.apply(y_prev, ms, prev, teacher, inv)


def inverse_map(prev: np.ndarray, n_prev: int) -> np.ndarray:
    """inv[j] = the i with prev[i] == j, or -1."""
    inv = np.full(n_prev, -1, dtype=I32)
    pos = np.nonzero(prev >= 0)[0]
    inv[prev[pos]] = pos.astype(I32)
    return inv


# ------------------------------------------------------------------ the schedule
def _upload(levels: List[Level], device):
    """Every index of the plan in ONE host-to-device copy -> per level (frames, teacher, prev, inv) as Index.
    The planner built them, so they are in range and distinct by construction."""
    sizes = {}
    for lv in levels:
        sizes[lv.depth] = sizes.get(lv.depth, 0) + lv.frames.size
    parts = []
    for lv in levels:
        inv = inverse_map(lv.prev, sizes[lv.depth - 1]) if lv.depth else np.zeros(0, dtype=I32)
        parts.append((lv.frames, lv.teacher, lv.prev, inv))
    flat = np.concatenate([a for p in parts for a in p]) if parts else np.zeros(0, dtype=I32)
    dev = torch.from_numpy(flat).to(device)
    out, o = [], 0
    for p in parts:
        row = []
        for a in p:
            row.append(Index(a, dev[o:o + a.size], True))
            o += a.size
        out.append(row)
    return out


def generate_levels(model, fb, mp, ms, mask, levels: Optional[List[Level]] = None) -> torch.Tensor:
    """fb [T][B][r][Fa], mp / ms [T][B][1][F] (time-major, padding zeroed, as Metaformer._generate makes
    them), mask host bool [T] -> prediction [B, T, F]: the value of the per-frame loop, with one model
    forward per planned level."""
    from . import functional as Fn
    T, B = ms.shape[0], ms.shape[1]
    dev = ms.device
    if levels is None:
        levels = plan_levels(mask, rows_cap_for(model, dev), B)
    r, F = fb.shape[2], ms.shape[-1]
    fb3, mp3, ms3 = fb.reshape(T, B, -1), mp.reshape(T, B, -1), ms.reshape(T, B, F)
    index = _upload(levels, dev)
    if B * T >= 2048:
        # the bf16 planes of every weight once per step, as a whole-sequence training forward prepares them
        # (Metaformer.forward would do it once per level that has 2048 rows)
        Fn.prepare_weight_planes(model.parameters())
    pred = torch.empty(T, B, F, device=dev, dtype=torch.float32)
    below, here, depth = None, [], 0
    was = model._planes_prepared
    model._planes_prepared = True
    try:
        for lv, (frames, teacher, prev, inv) in zip(levels, index):
            if lv.depth != depth:
                below, here, depth = (here[0] if len(here) == 1 else torch.cat(here)), [], lv.depth
            n = lv.frames.size
            a = gather(fb3, frames).view(n * B, r, -1)
            p = gather(mp3, frames).view(n * B, 1, -1)
            x = level_input(below, prev, ms3, teacher, inv if lv.depth else None).view(n * B, 1, F)
            lead = [(torch.empty(n * B, 0, t.shape[-1], device=dev), None) for t in (a, p, x)]
            y, _ = model.forward((a, None), (p, None), (x, None), *lead, None)
            y = y.reshape(n, B, F)
            here.append(y)
            pred = scatter(pred, y, frames)
    finally:
        model._planes_prepared = was
    return pred.transpose(0, 1).contiguous()
