"""The recurrent autograd Functions: the persistent LSTM launch, the one-step LSTM cell and the GRU."""
import ctypes
import os
from typing import Sequence

import torch
from torch.autograd import Function

from . import _lib, gemm_ops
from .dense import _resln_bwd, _resln_fwd, residual_add, residual_layernorm
from .gemm_ops import _dx_gemm, _fwd_gemm, _wgrad, _wt_note, colsum, gemm
from .launch import _ARITH, _err_flag, _gbuf, _keeps_precision, _probe, _ptr, _stream, zeros
from .wgrad_streams import beside_recurrence


def _arr(ctype, vals):
    return (ctype * len(vals))(*vals)


def _bias_pair(b_ih, b_hh):
    """(gb, gb2) for the input product's fused bias sums: both biases take the same column sums of
    dG, so they share one launch; the first existing buffer leads."""
    gbi, gbh = _gbuf(b_ih), _gbuf(b_hh)
    return (gbi, gbh) if gbi is not None else (gbh, None)


def _rec_wgrad(gw, dG, G, y, y_bs, y_ts, yoff, h0, B, T, H, reverse, dev):
    """gw[G, H] += sum_t dG_t^T h_prev(t), the recurrent weight gradient of one direction; G = 4H
    (LSTM) or 3H (GRU) is dG's gate width, dG [B, T, G] contiguous.  h_t is read from y at element
    offset yoff with batch / time strides y_bs / y_ts: one shifted-pair product over the T - 1 steps
    whose predecessor is in y (forward pairs (dG[t], y[t-1]), reverse (dG[t], y[t+1])), plus the h0
    term of the first step."""
    if gw is None:
        return
    if T > 1:
        a_off = 0 if reverse else G
        b_off = yoff + (y_ts if reverse else 0)
        _wgrad(_ptr(dG, a_off), G, _ptr(y, b_off), y_ts, B * (T - 1), G, H, gw, dev,
               dy_hi=T * G, dy_div=T - 1, x_hi=y_bs, x_div=T - 1, keep=(dG, y))
    if h0 is not None:
        t0 = T - 1 if reverse else 0
        gemm_ops._on_side(dev, B * T, (dG, h0),
                          lambda: gemm(G, H, B, _ptr(dG, t0 * G), 1, T * G, _ptr(h0), 0, H, _ptr(gw), H, beta=1.0,
                                       device=dev), writes=(gw,))


# ------------------------------------------------------------------ LSTM
class _LSTMFn(Function):
    """``nprob`` same-shape single-layer LSTM directions in one persistent launch.

    tensors = [x, w_ih, w_hh, b_ih, b_hh, h0, c0] * nprob (h0/c0 may be None).
    concat: True = all problems share x and write one [B, T, nprob*H] output (bidirectional layer:
    forward then reverse, like nn.LSTM); an int g = consecutive groups of g problems, each group
    sharing its x and writing one [B, T, g*H] output (several bidirectional layers on different
    inputs in one launch: g = 2); False = one output per problem.
    Outputs: (y...) then (hT_i, cT_i) per problem.
    """

    @staticmethod
    @_keeps_precision
    def forward(ctx, spec, *tensors):
        nprob, concat, reverse, force_bs, eps = spec
        # unused outputs (hT, cT of the stateless mixers) get no gradient: None, not a
        # zero-filled tensor (the recurrence takes null dhT / dcT as zero)
        ctx.set_materialize_grads(False)
        resln = eps is not None  # per problem LN(y + x) (ResidualConnection around LSTMMixer)
        K = 9 if resln else 7
        probs = [tensors[K * i:K * i + K] for i in range(nprob)]
        x0 = probs[0][0]
        _lib.require_device(x0)
        dev = x0.device
        B, T, In = x0.shape
        H = probs[0][2].shape[1]
        lib = _lib.load()
        if not lib.mrg_lstm_supported_hidden(H):
            raise RuntimeError(f"LSTM hidden size {H} not supported by libmrg (16/32/64/128/256)")
        xs = [p[0].contiguous() for p in probs]
        gs = nprob if concat is True else (1 if concat is False else int(concat))   # problems per output
        if nprob % gs or (resln and gs > 1):
            raise ValueError(f"lstm: {nprob} problems do not form groups of {gs}")
        gxs, y_ptrs = [], []
        yout = [torch.empty(B, T, gs * H, device=dev, dtype=torch.float32) for _ in range(nprob // gs)]
        y_bs, y_ts = [T * gs * H] * nprob, [gs * H] * nprob
        for i, p in enumerate(probs):
            x, w_ih, b_ih = xs[i], p[1], p[3]
            In_i = x.shape[2]
            gx = torch.empty(B, T, 4 * H, device=dev, dtype=torch.float32)
            _fwd_gemm(B * T, 4 * H, In_i, _ptr(x), In_i, w_ih, _ptr(gx), 4 * H, bias=_ptr(b_ih), device=dev)
            _wt_note(w_ih, B * T, ctx.needs_input_grad[1 + K * i])
            gxs.append(gx)
            y_ptrs.append(_ptr(yout[i // gs], (i % gs) * H))
        gates = [torch.empty(B, T, 4 * H, device=dev, dtype=torch.float32) for _ in range(nprob)]
        cs = [torch.empty(B, T, H, device=dev, dtype=torch.float32) for _ in range(nprob)]
        hT = [torch.empty(B, H, device=dev, dtype=torch.float32) for _ in range(nprob)]
        cT = [torch.empty(B, H, device=dev, dtype=torch.float32) for _ in range(nprob)]
        xb_elems = lib.mrg_lstm_fwd_xbuf_bytes(B, H) // 8
        xbuf = zeros(nprob, xb_elems, dtype=torch.int64, device=dev)
        h0 = [None if p[5] is None else p[5].contiguous() for p in probs]
        c0 = [None if p[6] is None else p[6].contiguous() for p in probs]
        arr, VP = _arr, ctypes.c_void_p
        with _probe("lstm_fwd", 8.0 * H * H * B * T * nprob):  # recurrent h W_hh^T FLOPs
            rc = lib.mrg_lstm_fwd(
                nprob, B, T, H,
                arr(VP, [_ptr(g) for g in gxs]), arr(ctypes.c_long, [T * 4 * H] * nprob),
                arr(ctypes.c_long, [4 * H] * nprob),
                arr(VP, [_ptr(p[2]) for p in probs]), arr(VP, [_ptr(p[4]) for p in probs]),
                arr(VP, [_ptr(h) for h in h0]), arr(VP, [_ptr(c) for c in c0]),
                arr(VP, y_ptrs), arr(ctypes.c_long, y_bs), arr(ctypes.c_long, y_ts),
                arr(VP, [_ptr(g) for g in gates]), arr(VP, [_ptr(c) for c in cs]),
                arr(VP, [_ptr(h) for h in hT]), arr(VP, [_ptr(c) for c in cT]),
                arr(ctypes.c_int, [int(r) for r in reverse]),
                arr(VP, [_ptr(xbuf[i]) for i in range(nprob)]), None, _ptr(_err_flag(dev)),
                _lib.cu_count(dev.index or 0), force_bs, _stream())
        _lib.check(rc, "lstm fwd")
        ctx.spec = (nprob, gs, tuple(reverse), force_bs, B, T, H, resln)
        save, uout = [], []
        for i, p in enumerate(probs):
            save += [xs[i], p[1], p[2], p[3], p[4], gates[i], cs[i], h0[i], c0[i]]
            if resln:
                u, mean, rstd = _resln_fwd(yout[i].view(B * T, H), xs[i].view(B * T, H), p[7], p[8], eps)
                uout.append(u.view(B, T, H))
                save += [p[7], p[8], mean, rstd]
        save += yout
        ctx.save_for_backward(*save)
        # each problem's x owner: the first problem holding the same tensor (its dx collects theirs)
        ctx.x_owner = [next(k for k in range(i + 1) if probs[k][0] is probs[i][0]) for i in range(nprob)]
        outs = list(uout if resln else yout)
        for i in range(nprob):
            outs += [hT[i], cT[i]]
        return tuple(outs)

    @staticmethod
    @_keeps_precision
    def backward(ctx, *grads):
        nprob, gs, reverse, force_bs, B, T, H, resln = ctx.spec
        saved = ctx.saved_tensors
        S = 13 if resln else 9
        per = [saved[S * i:S * i + S] for i in range(nprob)]
        yout = saved[S * nprob:]
        dev = yout[0].device
        lib = _lib.load()
        ny = nprob // gs
        gy = list(grads[:ny])
        gstate = grads[ny:]
        res = [None] * nprob  # residual-branch gradient g_i of LN(y_i + x_i), added by the dX GEMM
        if resln:
            for i in range(nprob):
                if gy[i] is None:
                    continue
                gamma, beta, mean, rstd = per[i][9:13]
                res[i] = _resln_bwd(gy[i].reshape(B * T, H).contiguous(), yout[i].view(B * T, H),
                                    per[i][0].view(B * T, H), gamma, beta, mean, rstd)
                gy[i] = res[i].view(B, T, H)
        y_bs, y_ts = [T * gs * H] * nprob, [gs * H] * nprob
        dy_ptr, dy_bs, dy_ts = [], [], []
        for i in range(nprob):
            g = gy[i // gs]
            if g is not None:
                gy[i // gs] = g = g.contiguous()
            dy_ptr.append(_ptr(g, (i % gs) * H))
            dy_bs.append(0 if g is None else y_bs[i])
            dy_ts.append(0 if g is None else y_ts[i])
        dhT = [None if gstate[2 * i] is None else gstate[2 * i].contiguous() for i in range(nprob)]
        dcT = [None if gstate[2 * i + 1] is None else gstate[2 * i + 1].contiguous() for i in range(nprob)]
        dG = [torch.empty(B, T, 4 * H, device=dev, dtype=torch.float32) for _ in range(nprob)]
        need = ctx.needs_input_grad  # index 0 is spec
        K = 9 if resln else 7
        dh0 = [torch.empty(B, H, device=dev, dtype=torch.float32)
               if per[i][7] is not None and need[1 + K * i + 5] else None for i in range(nprob)]
        dc0 = [torch.empty(B, H, device=dev, dtype=torch.float32)
               if per[i][8] is not None and need[1 + K * i + 6] else None for i in range(nprob)]
        xb_elems = lib.mrg_lstm_bwd_xbuf_bytes(B, H) // 8
        xbuf = zeros(nprob, xb_elems, dtype=torch.int64, device=dev)
        arr, VP = _arr, ctypes.c_void_p
        with beside_recurrence(dev) as cap:
            lib.mrg_lstm_set_blocks_per_cu(cap)
            with _probe("lstm_bwd", 8.0 * H * H * B * T * nprob):  # dG W_hh FLOPs
                rc = lib.mrg_lstm_bwd(
                    nprob, B, T, H,
                    arr(VP, [_ptr(p[2]) for p in per]), arr(VP, [_ptr(p[5]) for p in per]),
                    arr(VP, [_ptr(p[6]) for p in per]), arr(VP, [_ptr(p[8]) for p in per]),
                    arr(VP, dy_ptr), arr(ctypes.c_long, dy_bs), arr(ctypes.c_long, dy_ts),
                    arr(VP, [_ptr(t) for t in dhT]), arr(VP, [_ptr(t) for t in dcT]),
                    arr(VP, [_ptr(t) for t in dG]), arr(VP, [_ptr(t) for t in dh0]),
                    arr(VP, [_ptr(t) for t in dc0]), arr(ctypes.c_int, [int(r) for r in reverse]),
                    arr(VP, [_ptr(xbuf[i]) for i in range(nprob)]), None, _ptr(_err_flag(dev)),
                    _lib.cu_count(dev.index or 0), force_bs, _stream())
            _lib.check(rc, "lstm bwd")

        out = [None]
        dx_of = {}   # first problem of each shared x -> its dx (the others add into it)
        for i in range(nprob):
            x, w_ih, w_hh, b_ih, b_hh, _g, _c, h0, _c0 = per[i][:9]
            In = x.shape[2]
            g = dG[i]
            rows = B * T
            _rec_wgrad(_gbuf(w_hh), g, 4 * H, yout[i // gs], y_bs[i], y_ts[i], (i % gs) * H, h0, B, T, H,
                       reverse[i], dev)
            first, second = _bias_pair(b_ih, b_hh)
            _wgrad(_ptr(g), 4 * H, _ptr(x), In, rows, 4 * H, In, _gbuf(w_ih), dev, gb=first, gb2=second,
                   keep=(g, x))
            dx = None
            if need[1 + K * i]:
                owner = ctx.x_owner[i]
                if owner != i and owner in dx_of:
                    _dx_gemm(rows, In, 4 * H, _ptr(g), 4 * H, w_ih, _ptr(dx_of[owner]), In, beta=1.0, device=dev)
                else:
                    dx = torch.empty(B, T, In, device=dev, dtype=torch.float32)
                    # with LN(y + x): dx = dG W_ih + g (residual branch in the epilogue)
                    kw = {} if res[i] is None else dict(epi=3, aux=_ptr(res[i]), ldaux=In)
                    _dx_gemm(rows, In, 4 * H, _ptr(g), 4 * H, w_ih, _ptr(dx), In, device=dev, **kw)
                    dx_of[i] = dx
            out += [dx, None, None, None, None, dh0[i], dc0[i]] + ([None, None] if resln else [])
        return tuple(out)


class _LSTMCellFn(Function):
    """One time step (T = 1) of one nn.LSTM direction: gate pre-activations by the GEMMs
    (x W_ih^T + b_ih, + h0 W_hh^T with a state) and the element-wise cell kernels.  The per-frame
    decode of lstm_with_sampling's scheduled sampling (lstm_with_sample.py:410-433) runs 300 of
    these per training step; a persistent recurrence launch per frame would be pure overhead."""

    @staticmethod
    @_keeps_precision
    def forward(ctx, x, w_ih, w_hh, b_ih, b_hh, h0, c0):
        _lib.require_device(x)
        dev = x.device
        B, _, In = x.shape
        H = w_hh.shape[1]
        lib = _lib.load()
        x2 = x.reshape(B, In).contiguous()
        h0c = None if h0 is None else h0.contiguous()
        c0c = None if c0 is None else c0.contiguous()
        gates = torch.empty(B, 4 * H, device=dev, dtype=torch.float32)
        c = torch.empty(B, H, device=dev, dtype=torch.float32)
        y = torch.empty(B, 1, H, device=dev, dtype=torch.float32)
        hT = torch.empty(B, H, device=dev, dtype=torch.float32)
        if _ARITH[0] is None and In % 4 == 0 and H % 4 == 0 and In + H <= 512:
            # gates GEMMs + cell in one launch (decode.hip lstm_step_fwd_kernel)
            _lib.check(lib.mrg_lstm_step_fwd(B, H, In, _ptr(x2), _ptr(h0c), _ptr(c0c), _ptr(w_ih), _ptr(w_hh),
                                             _ptr(b_ih), _ptr(b_hh), _ptr(gates), _ptr(c), _ptr(y), H, _ptr(hT),
                                             _stream()), "lstm step fwd")
        else:
            pre = torch.empty(B, 4 * H, device=dev, dtype=torch.float32)
            gemm(B, 4 * H, In, _ptr(x2), 0, In, _ptr(w_ih), 1, In, _ptr(pre), 4 * H, bias=_ptr(b_ih), device=dev)
            if h0c is not None:
                gemm(B, 4 * H, H, _ptr(h0c), 0, H, _ptr(w_hh), 1, H, _ptr(pre), 4 * H, beta=1.0, device=dev)
            _lib.check(lib.mrg_lstm_cell_fwd(B, H, _ptr(pre), 4 * H, _ptr(b_hh), _ptr(c0c), _ptr(gates), _ptr(c),
                                             _ptr(y), H, _ptr(hT), _stream()), "lstm cell fwd")
        ctx.save_for_backward(x2, w_ih, w_hh, b_ih, b_hh, h0c, c0c, gates, c)
        ctx.set_materialize_grads(False)  # an unused final state costs no zero-filled gradient
        return y, hT, c

    @staticmethod
    @_keeps_precision
    def backward(ctx, dy, dhT, dcT):
        x2, w_ih, w_hh, b_ih, b_hh, h0c, c0c, gates, c = ctx.saved_tensors
        B, In = x2.shape
        H = w_hh.shape[1]
        dev = x2.device
        lib = _lib.load()
        dy = None if dy is None else dy.contiguous()
        dhT = None if dhT is None else dhT.contiguous()
        dcT = None if dcT is None else dcT.contiguous()
        dG = torch.empty(B, 4 * H, device=dev, dtype=torch.float32)
        need = ctx.needs_input_grad
        dc0 = torch.empty(B, H, device=dev, dtype=torch.float32) if (c0c is not None and need[6]) else None
        _lib.check(lib.mrg_lstm_cell_bwd(B, H, _ptr(gates), _ptr(c), _ptr(c0c), _ptr(dy), H, _ptr(dhT), _ptr(dcT),
                                         _ptr(dG), _ptr(dc0), _stream()), "lstm cell bwd")
        first, second = _bias_pair(b_ih, b_hh)
        _wgrad(_ptr(dG), 4 * H, _ptr(x2), In, B, 4 * H, In, _gbuf(w_ih), dev, gb=first, gb2=second, keep=(dG, x2))
        gw = _gbuf(w_hh)  # zero state: dW_hh = dG^T h0 = 0 (the buffer still exists, as with nn.LSTM)
        if gw is not None and h0c is not None:
            _wgrad(_ptr(dG), 4 * H, _ptr(h0c), H, B, 4 * H, H, gw, dev, keep=(dG, h0c))
        dx = dh0 = None
        if need[0]:
            dx = torch.empty(B, 1, In, device=dev, dtype=torch.float32)
            gemm(B, In, 4 * H, _ptr(dG), 0, 4 * H, _ptr(w_ih), 0, In, _ptr(dx), In, device=dev)
        if h0c is not None and need[5]:
            dh0 = torch.empty(B, H, device=dev, dtype=torch.float32)
            gemm(B, H, 4 * H, _ptr(dG), 0, 4 * H, _ptr(w_hh), 0, H, _ptr(dh0), H, device=dev)
        return dx, None, None, None, None, dh0, dc0


def lstm_layer(x, w_ih, w_hh, b_ih, b_hh, h0=None, c0=None, reverse=False, force_bs=0):
    """One direction of one nn.LSTM layer (batch_first).  Returns (y, hT, cT)."""
    if x.shape[1] == 1 and force_bs == 0:
        return _LSTMCellFn.apply(x, w_ih, w_hh, b_ih, b_hh, h0, c0)
    return _LSTMFn.apply((1, False, (reverse,), force_bs, None), x, w_ih, w_hh, b_ih, b_hh, h0, c0)


def lstm_residual_layernorm(x, w_ih, w_hh, b_ih, b_hh, gamma, beta, eps=1e-5, h0=None, c0=None,
                            force_bs=0):
    """LN(LSTM(x) + x) for one unidirectional layer (ResidualConnection(LSTMMixer), mixer_block.py:
    479-507); the LSTM's dX GEMM takes the residual gradient in its epilogue.  Returns (u, hT, cT)."""
    if x.shape[1] == 1 and force_bs == 0:
        y, hT, cT = _LSTMCellFn.apply(x, w_ih, w_hh, b_ih, b_hh, h0, c0)
        return residual_layernorm(y, x, gamma, beta, eps), hT, cT
    return _LSTMFn.apply((1, False, (False,), force_bs, float(eps)), x, w_ih, w_hh, b_ih, b_hh, h0, c0, gamma, beta)


def lstm_residual(x, w_ih, w_hh, b_ih, b_hh, h0=None, c0=None, force_bs=0):
    """LSTM(x) + x for one unidirectional layer (In == H): ResidualConnection(LSTMMixer) without a
    LayerNorm.  No GEMM feeds the sum (the recurrence writes y), so the add is one launch, over the
    layer output where autograd does not keep it (residual_add).  Returns (y + x, hT, cT)."""
    if x.shape[-1] != w_hh.shape[1]:
        raise ValueError(f"lstm_residual: input size {x.shape[-1]} is not the hidden size {w_hh.shape[1]}")
    y, hT, cT = lstm_layer(x, w_ih, w_hh, b_ih, b_hh, h0, c0, force_bs=force_bs)
    return residual_add(y, x, inplace=True), hT, cT


def lstm_bidirectional_residual(x, fw, bw, h0=None, c0=None, force_bs=0):
    """The same around one bidirectional layer (In == 2H); arguments and states as
    lstm_bidirectional_layer."""
    if x.shape[-1] != 2 * fw[1].shape[1]:
        raise ValueError(f"lstm_bidirectional_residual: input size {x.shape[-1]} is not 2 x {fw[1].shape[1]}")
    y, hT, cT = lstm_bidirectional_layer(x, fw, bw, h0, c0, force_bs=force_bs)
    return residual_add(y, x, inplace=True), hT, cT


def lstm_layers_batched(problems: Sequence[Sequence], force_bs=0):
    """Several independent same-shape unidirectional layers in ONE persistent launch.

    problems: [(x, w_ih, w_hh, b_ih, b_hh)] -> [y_i]; zero initial state.
    """
    flat = []
    eps = None
    for p in problems:
        x, w_ih, w_hh, b_ih, b_hh = p[:5]
        flat += [x, w_ih, w_hh, b_ih, b_hh, None, None]
        if len(p) > 5:  # (.., gamma, beta, eps): LN(LSTM(x) + x) per problem
            flat += [p[5], p[6]]
            eps = float(p[7])
    if eps is not None and any(len(p) <= 5 for p in problems):
        raise ValueError("lstm_layers_batched: residual LayerNorm must be given for every problem or none")
    n = len(problems)
    if problems[0][0].shape[1] == 1 and force_bs == 0:
        return [lstm_layer(*p[:5])[0] if len(p) <= 5 else lstm_residual_layernorm(*p[:5], p[5], p[6], p[7])[0]
                for p in problems]
    outs = _LSTMFn.apply((n, False, (False,) * n, force_bs, eps), *flat)
    return list(outs[:n])


def lstm_bidirectional_layers(layers, force_bs=0):
    """Several independent bidirectional nn.LSTM layers (zero initial state) in ONE persistent launch:
    layers = [(x [B, T, In_i], fw, bw)] with fw / bw = (w_ih, w_hh, b_ih, b_hh), the same B, T and
    hidden size.  Returns [(y [B, T, 2H], hT [2, B, H], cT [2, B, H])] per layer."""
    flat, rev = [], []
    for x, fw, bw in layers:
        flat += [x, *fw, None, None, x, *bw, None, None]
        rev += [False, True]
    n = len(layers)
    outs = _LSTMFn.apply((2 * n, 2, tuple(rev), force_bs, None), *flat)
    ys, st = outs[:n], outs[n:]
    return [(ys[k], torch.stack([st[4 * k], st[4 * k + 2]]), torch.stack([st[4 * k + 1], st[4 * k + 3]]))
            for k in range(n)]


def lstm_bidirectional_layer(x, fw, bw, h0=None, c0=None, force_bs=0):
    """One bidirectional nn.LSTM layer: fw/bw = (w_ih, w_hh, b_ih, b_hh); returns (y[B,T,2H], hT[2,B,H], cT)."""
    h0f, h0b = (None, None) if h0 is None else (h0[0], h0[1])
    c0f, c0b = (None, None) if c0 is None else (c0[0], c0[1])
    y, hTf, cTf, hTb, cTb = _LSTMFn.apply((2, True, (False, True), force_bs, None), x, *fw, h0f, c0f, x, *bw, h0b, c0b)
    return y, torch.stack([hTf, hTb]), torch.stack([cTf, cTb])


# ------------------------------------------------------------------ GRU
# persistent GRU recurrences (gru_rec.hip); MRG_GRU_PERSIST=0 runs the per-step products + cells
_GRU_PERSIST = [os.environ.get("MRG_GRU_PERSIST", "1") == "1"]


class _GRUFn(Function):
    """One direction of one torch.nn.GRU layer (gate order r, z, n; mixer_block.py:169-208), batch
    first: the input GEMM for all steps, then per step the few-row recurrent GEMM h W_hh^T and the
    fused cell (gru.hip); backward runs the cell derivative and dh_{t-1} += dGH_t W_hh per step, then
    the weight / bias / input gradients as GEMMs over all steps.  Returns (y [B, T, H], hT [B, H])."""

    @staticmethod
    @_keeps_precision
    def forward(ctx, reverse, x, w_ih, w_hh, b_ih, b_hh, h0):
        _lib.require_device(x)
        dev = x.device
        B, T, In = x.shape
        H = w_hh.shape[1]
        H3 = 3 * H
        lib = _lib.load()
        x = x.contiguous()
        gx = torch.empty(B, T, H3, device=dev, dtype=torch.float32)
        gemm(B * T, H3, In, _ptr(x), 0, In, _ptr(w_ih), 1, In, _ptr(gx), H3, bias=_ptr(b_ih), device=dev)
        y = torch.empty(B, T, H, device=dev, dtype=torch.float32)
        gates = torch.empty(B, T, H3, device=dev, dtype=torch.float32)
        ghn = torch.empty(B, T, H, device=dev, dtype=torch.float32)
        h0c = None if h0 is None else h0.contiguous()
        ctx.persist = _GRU_PERSIST[0] and T > 1 and bool(lib.mrg_gru_supported_hidden(H))
        if ctx.persist:   # one persistent launch for all steps (gru_rec.hip)
            xb = zeros(max(1, lib.mrg_gru_xbuf_bytes(B, H) // 8), dtype=torch.int64, device=dev)
            with _probe("gru_fwd", 6.0 * H * H * B * T):
                rc = lib.mrg_gru_fwd(B, T, H, _ptr(gx), T * H3, H3, _ptr(w_hh), _ptr(b_hh), _ptr(h0c), _ptr(y), T * H,
                                     H, _ptr(gates), T * H3, H3, _ptr(ghn), T * H, H, int(bool(reverse)), _ptr(xb),
                                     _ptr(_err_flag(dev)), _lib.cu_count(dev.index or 0), _stream())
            _lib.check(rc, "gru fwd")
        else:
            gh = torch.empty(B, H3, device=dev, dtype=torch.float32)
            zero = torch.zeros(B, H3, device=dev, dtype=torch.float32) if h0 is None else None
            prev = None
            for t in (range(T - 1, -1, -1) if reverse else range(T)):
                if prev is None:
                    hp, hp_ld = _ptr(h0c), H
                else:
                    hp, hp_ld = _ptr(y, prev * H), T * H
                if hp is not None:
                    gemm(B, H3, H, hp, 0, hp_ld, _ptr(w_hh), 1, H, _ptr(gh), H3, device=dev)
                _lib.check(lib.mrg_gru_cell_fwd(B, H, _ptr(gx, t * H3), T * H3, _ptr(gh if hp is not None else zero),
                                                _ptr(b_hh), hp, hp_ld, _ptr(y, t * H), T * H, _ptr(gates, t * H3),
                                                T * H3, _ptr(ghn, t * H), T * H, _stream()), "gru cell fwd")
                prev = t
        h_last = y[:, 0 if reverse else T - 1] if T > 0 else (torch.zeros(B, H, device=dev) if h0c is None else h0c)
        hT = h_last.clone()
        ctx.reverse = bool(reverse)
        ctx.save_for_backward(x, w_ih, w_hh, b_ih, b_hh, h0c, y, gates, ghn)
        ctx.set_materialize_grads(False)
        return y, hT

    @staticmethod
    @_keeps_precision
    def backward(ctx, dy, dhT):
        x, w_ih, w_hh, b_ih, b_hh, h0c, y, gates, ghn = ctx.saved_tensors
        reverse = ctx.reverse
        dev = x.device
        B, T, In = x.shape
        H = w_hh.shape[1]
        H3 = 3 * H
        lib = _lib.load()
        dy = None if dy is None else dy.contiguous()
        dGX = torch.empty(B, T, H3, device=dev, dtype=torch.float32)
        dGH = torch.empty(B, T, H3, device=dev, dtype=torch.float32)
        dh_next = None if dhT is None else dhT.contiguous()
        need = ctx.needs_input_grad
        if ctx.persist:
            xb = zeros(max(1, lib.mrg_gru_xbuf_bytes(B, H) // 8), dtype=torch.int64, device=dev)
            dh_next = torch.empty(B, H, device=dev, dtype=torch.float32) if (h0c is not None and need[6]) else None
            # deferred weight gradients (wgrad_streams._DEFER) run beside this recurrence, as beside the LSTM's
            with beside_recurrence(dev):
                with _probe("gru_bwd", 6.0 * H * H * B * T):
                    rc = lib.mrg_gru_bwd(B, T, H, _ptr(w_hh), _ptr(gates), T * H3, H3, _ptr(ghn), T * H, H, _ptr(y), T * H,
                                         H, _ptr(h0c), _ptr(dy), T * H, H, _ptr(None if dhT is None else dhT.contiguous()),
                                         _ptr(dGX), _ptr(dGH), T * H3, H3, _ptr(dh_next), int(reverse), _ptr(xb),
                                         _ptr(_err_flag(dev)), _lib.cu_count(dev.index or 0), _stream())
                _lib.check(rc, "gru bwd")
        for t in ((range(T) if reverse else range(T - 1, -1, -1)) if not ctx.persist else ()):
            pt = t + 1 if reverse else t - 1
            if 0 <= pt < T:
                hp, hp_ld = _ptr(y, pt * H), T * H
            else:
                hp, hp_ld = _ptr(h0c), H
            dhp = torch.empty(B, H, device=dev, dtype=torch.float32)
            _lib.check(lib.mrg_gru_cell_bwd(B, H, _ptr(gates, t * H3), T * H3, _ptr(ghn, t * H), T * H, hp, hp_ld,
                                            _ptr(dy, t * H) if dy is not None else None, T * H, _ptr(dh_next),
                                            _ptr(dGX, t * H3), _ptr(dGH, t * H3), T * H3, _ptr(dhp), _stream()),
                       "gru cell bwd")
            gemm(B, H, H3, _ptr(dGH, t * H3), 0, T * H3, _ptr(w_hh), 0, H, _ptr(dhp), H, beta=1.0, device=dev)
            dh_next = dhp
        dh0 = dh_next if (h0c is not None and need[6]) else None
        _wgrad(_ptr(dGX), H3, _ptr(x), In, B * T, H3, In, _gbuf(w_ih), dev, gb=_gbuf(b_ih), keep=(dGX, x))
        _rec_wgrad(_gbuf(w_hh), dGH, H3, y, T * H, H, 0, h0c, B, T, H, reverse, dev)
        gbh = _gbuf(b_hh)
        if gbh is not None:
            gemm_ops._on_side(dev, B * T, (dGH,), lambda: colsum(B * T, H3, _ptr(dGH), H3, _ptr(gbh), device=dev),
                              writes=(gbh,))
        dx = None
        if need[1]:
            dx = torch.empty(B, T, In, device=dev, dtype=torch.float32)
            gemm(B * T, In, H3, _ptr(dGX), 0, H3, _ptr(w_ih), 0, In, _ptr(dx), In, device=dev)
        return None, dx, None, None, None, None, dh0


def gru_layer(x, w_ih, w_hh, b_ih, b_hh, h0=None, reverse=False):
    """One direction of one nn.GRU layer (batch_first).  Returns (y, hT)."""
    return _GRUFn.apply(bool(reverse), x, w_ih, w_hh, b_ih, b_hh, h0)


def gru_residual(x, w_ih, w_hh, b_ih, b_hh, h0=None):
    """GRU(x) + x for one forward layer (In == H), as lstm_residual.  Returns (y + x, hT)."""
    if x.shape[-1] != w_hh.shape[1]:
        raise ValueError(f"gru_residual: input size {x.shape[-1]} is not the hidden size {w_hh.shape[1]}")
    y, hT = gru_layer(x, w_ih, w_hh, b_ih, b_hh, h0)
    return residual_add(y, x, inplace=True), hT
