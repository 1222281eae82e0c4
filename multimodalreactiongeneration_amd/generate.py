"""lstmformer generation with the frame loop on the fused per-frame kernels (gen.hip).

Reference: Metaformer.prediction -> head_motion_generation -> generate_one_step
(mr_gen/model/lstmformer/lstmformer.py:426-521, form_generation_init :523-547).  Every frame is a
T = 1 forward of the whole model with zero recurrent state and empty lead inputs; the
frame's self-motion input is the previous prediction (mask true) or motion_s one frame late.

What this module hoists out of the frame loop (inference only, no autograd), because it does not
depend on the previous frame:

* the other modalities' block-0 encoders (feature Linear + every LSTM or GRU mixer block of the audio
  and partner-motion stacks), as [T * B]-row GEMMs, zero-state LSTM / GRU cells and LayerNorms;
* with one audio frame per prediction frame (ratio 1), each block's integrator attention output:
  the query sees exactly one key (generation zeroes the -100 padding, so no key is ever masked, and
  the block-causal rule admits key 0 for query 0), so the softmax weight is exactly 1 and
  MHA(q, kv) = out_proj(V(kv)) for any q -- two more [T * B]-row GEMMs per integrator;
* with r audio frames per prediction frame (1 < ratio <= 16) the audio encoder is a zero-state LSTM
  or GRU over the r steps of each of the [T * B] frames, and the audio integrator's query sees r keys: its
  output depends on the query, so only its key and value projections are hoisted ([T * B * r]-row
  GEMMs).  The partner-motion integrator still sees one key and stays hoisted as above.

The frame loop then runs the main chain only: five gen.hip launches per block and one for the
output FeedForward with the sampling select (5 x 5 + 1 = 26 per frame instead of ~145), every
LayerNorm computed in the prologue of the launch that consumes it.  At ratio > 1 a block takes three
more (the query projection, mrg_gen_attention over the frame's r keys, the output projection):
8 x 5 + 1 = 41 per frame, launch form only (the persistent loop is a ratio-1 path).  GenPlan._launches
builds the frame's launches once as a flat list (entry, probe FLOPs, error label, arguments); the frame
loop advances the few addresses that follow the frame and calls the list.

Each modality's embedding mixer is an LSTM or a GRU (config.yaml / config_gru.yaml, and any mix of the
two).  Only the recurrent cell of the frame chain knows which: a GRU main chain runs mrg_gen_gru where
the LSTM runs mrg_gen_lstm (the zero-state torch.nn.GRU step, which never reads W_hh), the same
launch counts.  The persistent loop's first stage is the LSTM cell, so it serves LSTM main chains
only, whatever the side stacks are (it reads their hoisted attention outputs); a GRU main chain at
ratio 1 runs the 26 launches.

Forms outside this plan (ratio > 16, integrator head widths other than 16 / 32 / 64 at ratio > 1,
widths other than E = 256 / bottleneck 64, mixers other than one-layer unidirectional LSTM / GRU
blocks, grad enabled) return None and the caller runs the per-frame module forward.
"""
from __future__ import annotations

import ctypes
import os
from typing import NamedTuple, Optional

import torch

from . import _lib
from . import functional as Fn
from .launch import _err_flag, _probe, _ptr, _stream, zeros
from .model import forms
from .model.metaformer import _FUSED_MIN_T

F32 = torch.float32
E_GEN, HB_GEN = 256, 64
# the whole frame loop as ONE persistent launch (gen.hip gen_loop_kernel) when its grid fits;
# MRG_GEN_LOOP=0 keeps the 26 launches per frame
_LOOP = [os.environ.get("MRG_GEN_LOOP", "1") == "1"]
# what mrg_gen_attention takes: keys per query, and head counts (D = 256 / heads in {64, 32, 16})
RATIO_MAX, ATT_HEADS = 16, (4, 8, 16)


def _arr(*ts):
    return (ctypes.c_void_p * len(ts))(*[t if isinstance(t, ctypes.c_void_p) else _ptr(t) for t in ts])


def _few_row_gemm(*args, **kw):
    """Fn.gemm as a launch-list entry: it raises on its own errors, so its return code is 0."""
    Fn.gemm(*args, **kw)
    return 0


# The r-step recurrences of the side stacks (r > 1): the layer function, and the sequences one launch takes
# per 8 CUs.  Each is one persistent launch whose whole grid must be resident, one workgroup per CU, so N
# sequences go through in chunks of that many times CUs / 8.
_RECURRENCE = {
    # at H = 256 eight workgroups serve at most 16 sequences (lstm_common.h launch_tiles, lstm_mx.hip): 512 on 256 CUs
    "lstm": (Fn.lstm_layer, 16),
    # the GRU's launch has the same residency rule and no fallback (gru_rec.hip: launch_tiles returns an
    # error when no batch tile fits): at H = 256 a ring of 4 or 8 workgroups (mrg_gru_config) serves at
    # most 8 sequences, so with the larger ring 256 on 256 CUs
    "gru": (Fn.gru_layer, 8),
}


class GenBlock(NamedTuple):
    """One Metaformer block as the frame chain reads it."""
    kind: str            # "lstm" | "gru": the main modality's embedding mixer
    mix: tuple           # its forms.LstmBlock / forms.GruBlock (the same fields)
    integ: tuple         # the (audio, partner-motion) integrators' parameter groups
    cat_w: torch.Tensor
    cat_b: torch.Tensor
    ffn: tuple           # forms.relu_ffn_form of the block's FeedForward (w1, b1, w2, b2, ln)
    heads: int           # of the integrators' attention


class Launch(NamedTuple):
    """One launch of a frame.  The FLOPs are the algorithmic ones of the "gen" probe: 2 x rows x outputs x K
    (the LayerNorms are O(rows x E))."""
    fn: object           # the library entry, or _few_row_gemm
    flops: float
    what: str            # the error label
    args: list
    kw: dict = {}


class GenPlan:
    """The parameters of Metaformer.metaformer arranged for the fused frame loop, or ``ok = False``."""

    def __init__(self, mf, ratio: int):
        self.ok = False
        if not (1 <= ratio <= RATIO_MAX) or mf.interlayer_residual or mf.repeat_with_encoder or mf.hidden_dim != E_GEN:
            return
        # (not _fast_eligible: that is the training schedules' predicate and takes LSTM embeddings only;
        # here every embedding is an LSTM or a GRU chain, forms.embedding_mixer_form below)
        if mf._module_path_only():
            return
        blocks = list(mf.metaformer_blocks)
        first = forms.embedding_mixer_form(blocks[0])
        if first is None or len(first[0]) != 3:
            return
        layers0, eps = first
        self.eps = eps
        self.ratio = ratio
        # block 0's audio / partner-motion stacks: ("lstm", [LstmBlock]) or ("gru", [GruBlock]) each
        self.enc = layers0[1:]
        self.fe = list(mf.feature_embedding)
        if any(e.bias is None for e in self.fe) or not self.fe[0].weight.is_cuda:
            return
        self.blocks = []
        for bi, blk in enumerate(blocks):
            got = forms.embedding_mixer_form(blk) if bi else first
            if got is None:
                return
            ((kind, main), *_others), blk_eps = got   # the main modality's chain: one Lstm- / GruBlock per block
            if len(main) != 1 or blk_eps != eps or any(v is None for v in main[0]):
                return
            # the frames are T = 1 calls of the fused integrator: its switches hold here too
            integ = forms.integrator_form(blk.integrator) if (blk.integrator.use_fused and _FUSED_MIN_T == 1) else None
            if integ is None or len(integ.integrators) != 2 or integ.eps != eps or integ.cat_w.shape[0] != E_GEN:
                return
            if ratio > 1 and integ.heads not in ATT_HEADS:
                return
            ffn = forms.relu_ffn_form(blk.feedforward, True)
            if ffn is None or ffn.w1.shape[0] != HB_GEN or ffn.ln.eps != eps:
                return
            self.blocks.append(GenBlock(kind, main[0], tuple(integ.integrators), integ.cat_w, integ.cat_b, ffn,
                                        integ.heads))
        out = forms.relu_ffn_form(mf.output_feedforward, False)
        if out is None or out.w1.shape[0] != HB_GEN or out.w2.shape[0] > 16:
            return
        self.out = out
        self.fm = out.w2.shape[0]
        if self.fe[0].weight.shape[1] != self.fm:
            return
        # the persistent loop's first stage is the LSTM cell
        self.loop_form = all(b.kind == "lstm" for b in self.blocks)
        self.ok = True

    # ---- frame-independent work over all T frames ([T * B] rows, time-major)
    def _side_stack(self, x, stack, r=1):
        """One of block 0's audio / partner-motion stacks over x [N * r, E], N = T * B sequences of r steps:
        per Lstm- / GruBlock the recurrent step from zero state, then LN1, the Linear and LN2 on all rows.
        r = 1: the step is the gate GEMM and the zero-state cell.  r > 1 (the audio stack): a
        zero-initial-state recurrence over the r steps of each sequence (W_hh matters here)."""
        kind, layers = stack
        N, H, dev = x.shape[0] // r, E_GEN, x.device
        if r == 1:
            lib = _lib.load()
            gates = torch.empty(N, (4 if kind == "lstm" else 3) * H, device=dev, dtype=F32)
            c = torch.empty(N, H, device=dev, dtype=F32)   # the LSTM's cell state; the GRU cell's gh_n + b_hn
        else:
            layer, per8 = _RECURRENCE[kind]
            limit = per8 * max(1, _lib.cu_count(dev.index or 0) // 8)
        for lay in layers:
            if r > 1:
                x3 = x.view(N, r, H)
                hs = [layer(x3[i:i + limit], lay.w_ih, lay.w_hh, lay.b_ih, lay.b_hh)[0] for i in range(0, N, limit)]
                h = (hs[0] if len(hs) == 1 else torch.cat(hs)).view(N * r, H)
            else:
                g = Fn.linear(x, lay.w_ih, lay.b_ih)
                h = torch.empty(N, H, device=dev, dtype=F32)
                if kind == "lstm":
                    _lib.check(lib.mrg_lstm_cell_fwd(N, H, _ptr(g), 4 * H, _ptr(lay.b_hh), None, _ptr(gates), _ptr(c),
                                                     _ptr(h), H, None, _stream()), "gen encoder cell")
                else:
                    # zero state: no previous h and no h W_hh^T product (gh null reads as zero)
                    _lib.check(lib.mrg_gru_cell_fwd(N, H, _ptr(g), 3 * H, None, _ptr(lay.b_hh), None, H, _ptr(h), H,
                                                    _ptr(gates), 3 * H, _ptr(c), H, _stream()), "gen encoder gru cell")
            y = Fn.residual_layernorm(h, x, lay.ln1_w, lay.ln1_b, self.eps)
            x = Fn.residual_layernorm(Fn.linear(y, lay.ff_w, lay.ff_b), y, lay.ln2_w, lay.ln2_b, self.eps)
        return x

    def _hoist(self, fb, mp):
        """-> att, kvs.  att[block][i] [T * B, 256]: integrator i's attention output at one visible key,
        out_proj(V(kv)) (None for the audio integrator at r > 1).  kvs[block] (r > 1 only): the audio
        integrator's K(kv) and V(kv), rows in [T][B][r] order."""
        E, r = E_GEN, self.ratio
        T, B = fb.shape[:2]
        fa = Fn.linear(fb.reshape(T * B * r, -1), self.fe[1].weight, self.fe[1].bias)
        others = [self._side_stack(fa, self.enc[0], r),
                  self._side_stack(Fn.linear(mp.reshape(T * B, -1), self.fe[2].weight, self.fe[2].bias), self.enc[1])]
        att, kvs = [], []
        for blk in self.blocks:
            att.append([Fn.linear(Fn.linear(kv, ip.in_w[2 * E:], ip.in_b[2 * E:]), ip.out_w, ip.out_b)
                        if (r == 1 or i == 1) else None for i, (kv, ip) in enumerate(zip(others, blk.integ))])
            if r > 1:
                ip = blk.integ[0]
                kvs.append((Fn.linear(others[0], ip.in_w[E:2 * E], ip.in_b[E:2 * E]),
                            Fn.linear(others[0], ip.in_w[2 * E:], ip.in_b[2 * E:])))
        return att, kvs

    def generate(self, fb, mp, ms, mask):
        """fb [T][B][r][Fa], mp / ms [T][B][1][fm] (time-major, padding zeroed), mask [T] bool ->
        prediction [B, T, fm].

        At ratio r > 1 every block keeps the audio integrator's hoisted keys and values, [T][B][r][256]
        each (frame t's [B][r][256] slab contiguous): 157 MB per tensor at B = 64, T = 300, r = 8, so
        2 x 5 x 157 MB over the five blocks."""
        lib = _lib.load()
        T, B = ms.shape[0], ms.shape[1]
        dev = ms.device
        att, kvs = self._hoist(fb, mp)
        msc = ms.reshape(T, B, self.fm).contiguous()
        # the kernel reads one byte per frame (a device bool tensor as it is: refreshed per graph replay)
        mask_u8 = mask if (mask.device == dev and mask.dtype in (torch.bool, torch.uint8)) \
            else mask.to(device=dev, dtype=torch.uint8)
        pred = torch.empty(B, T, self.fm, device=dev, dtype=F32)
        st = _stream()
        # (the persistent loop hoists both integrators' outputs: a ratio-1 path, LSTM main chain only)
        if self.ratio == 1 and self.loop_form and _LOOP[0] \
                and lib.mrg_gen_loop_fits(B, _lib.cu_count(dev.index or 0)) == 1:
            return self._generate_loop(lib, B, T, att, msc, mask_u8, pred, st)
        first, later, moves, _keep = self._launches(lib, B, T, att, kvs, msc, mask_u8, pred, st)
        for t in range(T):
            for holder, i, base, step in moves:
                holder[i] = base + t * step
            for fn, flops, what, args, kw in (later if t else first):
                with _probe("gen", flops):
                    _lib.check(fn(*args, **kw), what)
        return pred

    def _launches(self, lib, B, T, att, kvs, msc, mask_u8, pred, st):
        """-> first, later, moves, keep.  The launches of one frame in order, for frame 0 and for every later
        frame (they differ in the first entry: block 0 reads msc[0], then the sampling select's ms_in).
        moves: (holder, index, base, step), the slots that follow the frame, holder[index] = base + t * step
        before frame t's launches (device addresses in bytes; the output FeedForward's t itself).  keep: the
        frame buffers the entries point into.  Ratio 1 and ratio > 1 differ in which entries there are."""
        E, eps, r, fm, dev = E_GEN, self.eps, self.ratio, self.fm, msc.device
        new = lambda n: torch.empty(B, n, device=dev, dtype=F32)
        ms_in = new(fm)
        xb, hh, y, z, m3, zf = (new(E) for _ in range(6))
        y01, z01 = new(2 * E), new(2 * E)
        qb, cx, a0 = (new(E) for _ in range(3)) if r > 1 else (None,) * 3
        fe0, out = self.fe[0], self.out
        row = 4 * B * E   # bytes of one frame's [B][256] rows
        launches, moves = [], []
        for bi, blk in enumerate(self.blocks):
            mix, (i0, i1), ffn = blk.mix, blk.integ, blk.ffn
            # the recurrent mixer's launch: the two entries take the same arguments
            cell = lib.mrg_gen_lstm if blk.kind == "lstm" else lib.mrg_gen_gru
            f_cell = 2.0 * B * (4 if blk.kind == "lstm" else 3) * E * E
            tail = [eps, _ptr(xb), _ptr(mix.w_ih), _ptr(mix.b_ih), _ptr(mix.b_hh), _ptr(hh), st]
            if bi == 0:
                embed = lambda src: Launch(cell, f_cell + 2.0 * B * E * fm, "gen mixer cell",
                                           [B, fm, _ptr(src), _ptr(fe0.weight), _ptr(fe0.bias), None, None, None, None,
                                            *tail])
                launches.append(embed(ms_in))
                frame0 = embed(msc[0])
            else:
                prev = self.blocks[bi - 1].ffn.ln
                launches.append(Launch(cell, f_cell, "gen mixer cell",
                                       [B, fm, None, None, None, _ptr(zf), _ptr(m3), _ptr(prev.weight), _ptr(prev.bias),
                                        *tail]))
            launches.append(Launch(lib.mrg_gen_linear, 2.0 * B * E * E, "gen mixer linear",
                                   [0, B, _arr(hh), _arr(xb), _arr(mix.ln1_w), _arr(mix.ln1_b), E, None, None, None,
                                    eps, _ptr(y), E, _arr(mix.ff_w), _arr(mix.ff_b), _ptr(z), E, st]))
            # M = LN(Z + Y), the prologue of the query projection and of the two-integrator launch
            ln2 = [_arr(z), _arr(y), _arr(mix.ln2_w), _arr(mix.ln2_b), E]
            a2 = _arr(a0 if r > 1 else att[bi][0], att[bi][1])
            if r == 1:
                moves.append((a2, 0, att[bi][0].data_ptr(), row))
            else:
                # Q = M W_q^T + b_q (in_w's first E rows; M's rows are not kept), the attention over frame
                # t's r keys, a_0 = ctx W_o^T + b_o
                launches.append(Launch(lib.mrg_gen_linear, 2.0 * B * E * E, "gen query linear",
                                       [0, B, *ln2, None, None, None, eps, None, 0, _arr(i0.in_w), _arr(i0.in_b),
                                        _ptr(qb), E, st]))
                kt, vt = kvs[bi]
                args = [B, r, blk.heads, _ptr(qb), _ptr(kt), _ptr(vt), _ptr(cx), st]
                moves += [(args, 4, kt.data_ptr(), r * row), (args, 5, vt.data_ptr(), r * row)]
                # q . k and p v over the frame's r keys, all heads
                launches.append(Launch(lib.mrg_gen_attention, 2.0 * B * r * 2 * E, "gen attention", args))
                launches.append(Launch(_few_row_gemm, 2.0 * B * E * E, "gen attention out_proj",
                                       [B, E, E, _ptr(cx), 0, E, _ptr(i0.out_w), 1, E, _ptr(a0), E],
                                       dict(bias=_ptr(i0.out_b), device=dev)))
            moves.append((a2, 1, att[bi][1].data_ptr(), row))
            launches.append(Launch(lib.mrg_gen_linear, 2.0 * B * 2 * E * E, "gen integrators",
                                   [1, B, *ln2, a2, _arr(i0.ln1_w, i1.ln1_w), _arr(i0.ln1_b, i1.ln1_b), eps, _ptr(y01),
                                    2 * E, _arr(i0.ff_w, i1.ff_w), _arr(i0.ff_b, i1.ff_b), _ptr(z01), 2 * E, st]))
            launches.append(Launch(lib.mrg_gen_linear, 2.0 * B * E * 2 * E, "gen cat_linear",
                                   [2, B, _arr(_ptr(z01), _ptr(z01, E)), _arr(_ptr(y01), _ptr(y01, E)),
                                    _arr(i0.ln2_w, i1.ln2_w), _arr(i0.ln2_b, i1.ln2_b), 2 * E, None, None, None, eps,
                                    None, 0, _arr(blk.cat_w), _arr(blk.cat_b), _ptr(m3), E, st]))
            launches.append(Launch(lib.mrg_gen_ffn, 2.0 * B * HB_GEN * (E + E), "gen ffn",
                                   [B, E, _ptr(m3), None, None, None, eps, _ptr(ffn.w1), _ptr(ffn.b1), _ptr(ffn.w2),
                                    _ptr(ffn.b2), _ptr(zf), None, 0, None, None, None, 0, st]))
        lastln = self.blocks[-1].ffn.ln
        args = [B, fm, _ptr(zf), _ptr(m3), _ptr(lastln.weight), _ptr(lastln.bias), eps, _ptr(out.w1), _ptr(out.b1),
                _ptr(out.w2), _ptr(out.b2), None, _ptr(pred), T * fm, _ptr(ms_in), _ptr(msc), _ptr(mask_u8), 0, st]
        moves += [(args, 15, msc.data_ptr(), 4 * B * fm), (args, 17, 0, 1)]
        launches.append(Launch(lib.mrg_gen_ffn, 2.0 * B * HB_GEN * (E + fm), "gen output", args))
        keep = (ms_in, xb, hh, y, z, m3, zf, y01, z01, qb, cx, a0)
        return [frame0] + launches[1:], launches, moves, keep

    def _generate_loop(self, lib, B, T, att, msc, mask_u8, pred, st):
        """The frame loop in one persistent launch (mrg_gen_loop; pointer table order in include/mrg.h)."""
        ptrs = []
        for bi, blk in enumerate(self.blocks):
            mix, ffn = blk.mix, blk.ffn
            ptrs += [mix.w_ih, mix.b_ih, mix.b_hh, mix.ln1_w, mix.ln1_b, mix.ff_w, mix.ff_b, mix.ln2_w, mix.ln2_b]
            for ip in blk.integ:
                ptrs += [ip.ln1_w, ip.ln1_b, ip.ff_w, ip.ff_b, ip.ln2_w, ip.ln2_b]
            ptrs += [blk.cat_w, blk.cat_b, ffn.w1, ffn.b1, ffn.w2, ffn.b2, ffn.ln.weight, ffn.ln.bias, att[bi][0],
                     att[bi][1]]
        fe0, out = self.fe[0], self.out
        ptrs += [fe0.weight, fe0.bias, out.w1, out.b1, out.w2, out.b2]
        ring = zeros(max(1, lib.mrg_gen_loop_ring_bytes(B) // 8), dtype=torch.int64, device=msc.device)
        E = E_GEN
        flop = T * (len(self.blocks) * 2.0 * B * (4 * E * E + E * E + 2 * E * E + 2 * E * E + 2 * HB_GEN * E)
                    + 2.0 * B * HB_GEN * (E + self.fm))
        with _probe("gen", flop):
            _lib.check(lib.mrg_gen_loop(B, T, self.fm, len(self.blocks), self.eps, _arr(*ptrs), len(ptrs), _ptr(msc),
                                        _ptr(mask_u8), _ptr(pred), _ptr(ring), _ptr(_err_flag(msc.device)), st),
                       "gen loop")
        return pred


_PLANS = {}


def _dropout_active(module) -> bool:
    """A submodule in training mode would drop: an MHA with p > 0, or a multi-layer LSTM / GRU with p > 0."""
    from .model.layers import GRU, LSTM, MultiheadAttention
    for m in module.modules():
        if not (m.training and getattr(m, "dropout", 0.0)):
            continue
        if isinstance(m, MultiheadAttention) or (isinstance(m, (LSTM, GRU)) and m.num_layers > 1):
            return True
    return False


def _records_attention(module) -> bool:
    """An attention of the module keeps its weights (MultiheadAttention.record_weights): the fused
    frames would bypass it."""
    from .model.layers import MultiheadAttention
    return any(isinstance(m, MultiheadAttention) and m.record_weights is not None for m in module.modules())


def plan_for(model) -> Optional[GenPlan]:
    """The model's GenPlan (cached per module identity and parameter storage), or None outside it.
    Eligibility is cached, so what changes after construction is re-checked on every call: with an
    active dropout (model.train() / eval()) the frames take the module path, as the reference's would,
    and so they do while an attention records its weights (the switch is never part of the plan)."""
    mf = model.metaformer
    if _dropout_active(mf) or _records_attention(mf):
        return None
    key = (id(mf), mf.feature_embedding[0].weight.data_ptr(), model.ratio)
    p = _PLANS.get(key)
    if p is None:
        p = GenPlan(mf, model.ratio)
        _PLANS.clear()
        _PLANS[key] = p
    return p if p.ok else None
