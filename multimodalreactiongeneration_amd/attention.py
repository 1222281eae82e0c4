"""Multi-head attention: the kernel calls (attn_fwd, attn_bwd) and nn.MultiheadAttention's forms on them."""
import math
from contextlib import nullcontext
from types import SimpleNamespace
from typing import NamedTuple, Optional

import torch
from torch.autograd import Function

from . import _lib
from .dense import _resln_bwd, _resln_fwd
from .dropout import _drop_consts, _rng_draw
from .gemm_ops import _dx_gemm, _fwd_gemm, _wgrad, _wt_note, gemm
from .launch import _gbuf, _keeps_precision, _probe, _ptr, _stream, _ws, zeros


class MHASpec(NamedTuple):
    """What an attention Function computes around the kernels (its first argument)."""
    heads: int
    causal: bool
    eps: Optional[float] = None     # not None: return LN(attn + q) (ResidualConnection(MHAMixer))
    p: float = 0.0                  # > 0: dropout on the attention probabilities, one draw
    addq: bool = False              # return attn + q, the residual without a LayerNorm
    zero_attn: bool = False         # add_zero_attn's always-visible zero key
    weights: Optional[str] = None   # need_weights: None, "mean" (over the heads) or "heads"


def _save(ctx, **tensors):
    """save_for_backward under names (None where the form has no such tensor); _saved gives them back."""
    ctx.saved_names = tuple(tensors)
    ctx.save_for_backward(*tensors.values())


def _saved(ctx):
    return SimpleNamespace(**dict(zip(ctx.saved_names, ctx.saved_tensors)))


def visible_pairs(Tq, Tk, causal):
    """(query, key) pairs the block-causal rule admits per (sample, head) (gen_attention_mask rules)."""
    if not causal:
        return Tq * Tk
    if Tk >= Tq:
        r = Tk // Tq
        return sum(min((i + 1) * r, Tk) for i in range(Tq))
    r = Tq // Tk
    return sum(min(i // r + 1, Tk) for i in range(Tq))


def _attn_args(heads, Q, KV, O, lse, qpad, kpad, causal, scale, v=None, chunk=()):
    """The leading arguments every attention entry point takes: shapes (then a chunk form's q_off, Tq_full), Q,
    K and V, O, the row log-sum-exps, the padding flags and the mask rule.  KV is [B, Tk, 2E], keys then values
    in a row; Q and O: B * Tq contiguous rows of E under any leading shape; v: the values are its first E columns."""
    B, Tk, E2 = KV.shape
    E = E2 // 2
    Tq = Q.numel() // max(1, B * E)
    return (B, heads, Tq, Tk, E // heads, *chunk, _ptr(Q), Tq * E, E, _ptr(KV), Tk * E2, E2,
            _ptr(KV, E) if v is None else _ptr(v), Tk * E2, E2, _ptr(O), Tq * E, E, _ptr(lse), _ptr(qpad), _ptr(kpad),
            int(causal), scale)


def _bracket(name, probe, flops_per_pair, args, causal):
    """The probe bracket of a launch with these leading arguments (nothing when not probe)."""
    B, heads, Tq, Tk, D = args[:5]
    return _probe(name, flops_per_pair * D * B * heads * visible_pairs(Tq, Tk, causal)) if probe else nullcontext()


def attn_fwd(heads, Q, KV, O, lse, qpad, kpad, causal, scale, *, drop=None, v=None, probe=False,
             what="attention fwd"):
    """One forward launch of the attention kernels into O and lse; every forward call of the package.
    drop = (thr, scale_keep, key): the dropout form (never bracketed); v: see _attn_args (V = K: v=KV);
    probe: bracket the launch as "attn_fwd" for the per-kernel measurements."""
    args = _attn_args(heads, Q, KV, O, lse, qpad, kpad, causal, scale, v)
    lib = _lib.load()
    if drop is not None:
        rc = lib.mrg_attention_fwd_dropout(*args, *drop[:2], _ptr(drop[2]), _stream())
    else:
        with _bracket("attn_fwd", probe, 4.0, args, causal):
            rc = lib.mrg_attention_fwd(*args, _stream())
    _lib.check(rc, what)


def attn_bwd(heads, Q, KV, O, lse, qpad, kpad, causal, scale, dO, dQ, dKV, ws, *, drop=None, chunk=None, passes=3,
             kv_accumulate=0, probe=False, what="attention bwd"):
    """One backward call of the attention kernels into dQ and the two halves of dKV; every backward call of the
    package.  dO: rows like Q's, or one row [E] taken for every query (strides 0); ws: the delta workspace
    (mrg_attention_bwd_workspace_bytes); drop, probe ("attn_bwd") as in attn_fwd; chunk = (q_off, Tq_full): the chunk
    form with its passes and kv_accumulate (include/mrg.h: lse, ws, qpad the whole sequence's; no dropout variant)."""
    args = _attn_args(heads, Q, KV, O, lse, qpad, kpad, causal, scale, chunk=chunk or ())
    Tq, Tk = args[2:4]
    E = KV.shape[2] // 2
    lib = _lib.load()
    args += (_ptr(dO), *((0, 0) if dO.dim() == 1 else (Tq * E, E)), _ptr(dQ), Tq * E, E, _ptr(dKV), Tk * 2 * E, 2 * E,
             _ptr(dKV, E), Tk * 2 * E, 2 * E)
    if chunk is not None:
        rc = lib.mrg_attention_bwd_chunk(*args, passes, kv_accumulate, _ptr(ws), _stream())
    elif drop is not None:
        rc = lib.mrg_attention_bwd_dropout(*args, _ptr(ws), *drop[:2], _ptr(drop[2]), _stream())
    else:
        with _bracket("attn_bwd", probe, 10.0, args, causal):
            rc = lib.mrg_attention_bwd(*args, _ptr(ws), _stream())
    _lib.check(rc, what)


class _MHAFn(Function):
    @staticmethod
    @_keeps_precision
    def forward(ctx, spec, q_in, kv_in, in_w, in_b, out_w, out_b, qpad, kpad, gamma=None, beta=None,
                bias_k=None, bias_v=None):
        # p > 0: one draw, its key saved for the backward; addq: by the output projection's epilogue 3; extra
        # keys (bias_k / bias_v, zero_attn): one merge launch (_extra_fwd); weights: one more launch (_weights)
        heads, causal, eps, p, addq, zero_attn, want = spec
        _lib.require_device(q_in)
        dev = q_in.device
        B, Tq, E = q_in.shape
        Tk = kv_in.shape[1]
        q2 = q_in.contiguous()
        kv2 = kv_in.contiguous()
        Q = torch.empty(B, Tq, E, device=dev, dtype=torch.float32)
        _fwd_gemm(B * Tq, E, E, _ptr(q2), E, in_w[:E], _ptr(Q), E, bias=_ptr(in_b), device=dev)
        KV = torch.empty(B, Tk, 2 * E, device=dev, dtype=torch.float32)
        _fwd_gemm(B * Tk, 2 * E, E, _ptr(kv2), E, in_w[E:], _ptr(KV), 2 * E, bias=_ptr(in_b, E), device=dev)
        O = torch.empty(B, Tq, E, device=dev, dtype=torch.float32)
        lse = torch.empty(B, heads, Tq, device=dev, dtype=torch.float32)
        scale = 1.0 / math.sqrt(E // heads)
        drop = (*_drop_consts(p), _rng_draw(dev)) if p > 0.0 else None
        attn_fwd(heads, Q, KV, O, lse, qpad, kpad, causal, scale, drop=drop, probe=True)
        if bias_k is not None or zero_attn:
            _extra_fwd(heads, Q, bias_k, bias_v, zero_attn, scale, O, lse, Tk, drop)
        out = torch.empty(B, Tq, E, device=dev, dtype=torch.float32)
        kw = dict(epi=3, aux=_ptr(q2), ldaux=E) if addq else {}
        _fwd_gemm(B * Tq, E, E, _ptr(O), E, out_w, _ptr(out), E, bias=_ptr(out_b), device=dev, **kw)
        # dO = dout W_out runs in every backward (the in_proj weight gradient needs dO even when
        # neither input does), so out_w is noted unconditionally (a stale copy is never reused)
        _wt_note(out_w, B * Tq)
        _wt_note(in_w[:E], B * Tq, ctx.needs_input_grad[1])
        _wt_note(in_w[E:], B * Tk, ctx.needs_input_grad[2])
        ln = {}
        res = out
        if eps is not None:
            u, mean, rstd = _resln_fwd(out.view(B * Tq, E), q2.view(B * Tq, E), gamma, beta, eps)
            res = u.view(B, Tq, E)
            ln = dict(out=out, gamma=gamma, beta=beta, mean=mean, rstd=rstd)
        _save(ctx, q2=q2, kv2=kv2, Q=Q, KV=KV, O=O, lse=lse, in_w=in_w, in_b=in_b, out_w=out_w, out_b=out_b,
              qpad=qpad, kpad=kpad, **ln, bias_k=bias_k, bias_v=bias_v)
        ctx.spec = (heads, causal, scale, eps is not None)
        ctx.addq = addq
        ctx.drop = drop
        if want is None:
            return res
        wts = _weights(heads, Q, KV, bias_k, zero_attn, lse, qpad, kpad, causal, scale, want == "mean", drop)
        ctx.mark_non_differentiable(wts)
        return res, wts

    @staticmethod
    @_keeps_precision
    def backward(ctx, dout, _dweights=None):
        s = _saved(ctx)
        q2, kv2, Q, KV, O, lse, in_w, in_b, out_w, out_b, qpad, kpad = (
            s.q2, s.kv2, s.Q, s.KV, s.O, s.lse, s.in_w, s.in_b, s.out_w, s.out_b, s.qpad, s.kpad)
        heads, causal, scale, resln = ctx.spec
        B, Tq, E = q2.shape
        Tk = kv2.shape[1]
        dev = dout.device
        g = None  # residual-branch gradient of LN(attn + q), added by the dq GEMM's epilogue
        if resln:
            g = _resln_bwd(dout.reshape(B * Tq, E).contiguous(), s.out.view(B * Tq, E), q2.view(B * Tq, E),
                           s.gamma, s.beta, s.mean, s.rstd)
            do2 = g.view(B, Tq, E)
        else:
            do2 = dout.contiguous()
            if ctx.addq:   # attn + q: dq = dQ W_q + dout, by the same epilogue
                g = do2.view(B * Tq, E)
        dO = torch.empty(B, Tq, E, device=dev, dtype=torch.float32)
        _dx_gemm(B * Tq, E, E, _ptr(do2), E, out_w, _ptr(dO), E, device=dev)
        _wgrad(_ptr(do2), E, _ptr(O), E, B * Tq, E, E, _gbuf(out_w), dev, gb=_gbuf(out_b), keep=(do2, O))
        dQ = torch.empty(B, Tq, E, device=dev, dtype=torch.float32)
        dKV = torch.empty(B, Tk, 2 * E, device=dev, dtype=torch.float32)
        ws = _ws(_lib.load().mrg_attention_bwd_workspace_bytes(B, heads, Tq), dev)
        attn_bwd(heads, Q, KV, O, lse, qpad, kpad, causal, scale, dO, dQ, dKV, ws, drop=ctx.drop, probe=True)
        if s.bias_k is not None:   # the zero key alone has no gradient: the merged O / lse did it all
            _extra_bwd(heads, Q, KV, O, lse, qpad, kpad, causal, scale, (s.bias_k, s.bias_v), dO, dQ, dKV, ctx.drop)
        gw, gb = _gbuf(in_w), _gbuf(in_b)
        _wgrad(_ptr(dQ), E, _ptr(q2), E, B * Tq, E, E, None if gw is None else gw[:E], dev,
               gb=None if gb is None else gb[:E], keep=(dQ, q2))
        _wgrad(_ptr(dKV), 2 * E, _ptr(kv2), E, B * Tk, 2 * E, E, None if gw is None else gw[E:], dev,
               gb=None if gb is None else gb[E:], keep=(dKV, kv2))
        dq_in = dkv_in = None
        if ctx.needs_input_grad[1]:
            dq_in = torch.empty(B, Tq, E, device=dev, dtype=torch.float32)
            kw = {} if g is None else dict(epi=3, aux=_ptr(g), ldaux=E)
            _dx_gemm(B * Tq, E, E, _ptr(dQ), E, in_w[:E], _ptr(dq_in), E, device=dev, **kw)
        if ctx.needs_input_grad[2]:
            dkv_in = torch.empty(B, Tk, E, device=dev, dtype=torch.float32)
            _dx_gemm(B * Tk, E, 2 * E, _ptr(dKV), 2 * E, in_w[E:], _ptr(dkv_in), E, device=dev)
        return None, dq_in, dkv_in, None, None, None, None, None, None, None, None, None, None


def _extra_fwd(heads, Q, bias_k, bias_v, zero_attn, scale, O, lse, Tk, drop):
    """Merge the extra keys into the attention kernel's O / lse in place (mrg_attention_extra_fwd)."""
    B, Tq, E = Q.shape
    thr, sk, key = drop if drop is not None else (0, 1.0, None)
    _lib.check(_lib.load().mrg_attention_extra_fwd(
        B, heads, Tq, E // heads, _ptr(Q), Tq * E, E, _ptr(bias_k), _ptr(bias_v), int(zero_attn), scale,
        _ptr(O), Tq * E, E, _ptr(lse), Tk, thr, sk, _ptr(key), _stream()), "attention extra keys fwd")


def _weights(heads, Q, KV, bias_k, zero_attn, lse, qpad, kpad, causal, scale, average, drop):
    """The attention probabilities of an op that holds the projected Q / KV, the (merged) lse and, with
    dropout, the draw's key: [B, Tq, Tk + n] averaged over the heads or [B, heads, Tq, Tk + n], columns in
    torch's order [real keys, bias key, zero key] (mrg_attention_weights: one launch, its throughput
    not measured).  With dropout they are the dropped, rescaled ones O was built from, as torch's are."""
    B, Tq, E = Q.shape
    Tk = KV.shape[1]
    W = Tk + (bias_k is not None) + bool(zero_attn)
    shape = (B, Tq, W) if average else (B, heads, Tq, W)
    out = torch.empty(*shape, device=Q.device, dtype=torch.float32)
    thr, sk, key = drop if drop is not None else (0, 1.0, None)
    _lib.check(_lib.load().mrg_attention_weights(
        B, heads, Tq, Tk, E // heads, _ptr(Q), Tq * E, E, _ptr(KV), Tk * 2 * E, 2 * E, _ptr(bias_k),
        int(bool(zero_attn)), _ptr(lse), _ptr(qpad), _ptr(kpad), int(causal), scale, int(bool(average)), thr, sk,
        _ptr(key), _ptr(out), _stream()), "attention weights")
    return out


def _one_key_weights(q, heads, qpad, kpad, average):
    """Weights of the one-key form: the softmax over a single visible key is 1, and NaN where the
    pair is hidden (query AND key padding); there is no softmax to rebuild, so no kernel."""
    B = q.shape[0]
    shape = (B, 1, 1) if average else (B, heads, 1, 1)
    w = torch.ones(*shape, device=q.device, dtype=torch.float32)
    if qpad is not None and kpad is not None:
        hide = (qpad.reshape(B, 1) & kpad.reshape(B, 1)).bool().view(B, *([1] * (len(shape) - 1)))
        w = torch.where(hide, torch.full_like(w, float("nan")), w)
    return w


def _extra_bwd(heads, Q, KV, O, lse, qpad, kpad, causal, scale, bias_kv, dO, dQ, dKV, drop):
    """The bias key's share of the gradients, after the attention backward on the merged O / lse: dQ
    gets its term in place, bias_k.grad / bias_v.grad theirs (mrg_attention_extra_bwd).  The dropout
    backward forms delta from the main keys' own terms, so there the bias key's term c is missing
    from dQ and dK: a forward call with V = K gives sum_k P_k K_k for the dQ term, and the dK / dV
    pass alone (dO = 0, c in the delta rows, accumulating) subtracts the dK term (include/mrg.h)."""
    bias_k, bias_v = bias_kv
    B, Tq, E = Q.shape
    Tk = KV.shape[1]
    D = E // heads
    dev = Q.device
    lib = _lib.load()
    gk, gv = _gbuf(bias_k), _gbuf(bias_v)
    acc = 1
    if gk is None or gv is None:   # frozen: the kernel still needs somewhere to write
        gk, gv, acc = torch.empty(E, device=dev), torch.empty(E, device=dev), 0
    ws = _ws(lib.mrg_attention_extra_bwd_workspace_bytes(B, heads, Tq, D), dev)
    thr, sk, key = drop if drop is not None else (0, 1.0, None)
    pk = lse_main = cbuf = None
    if drop is not None and Tk > 0:
        pk = torch.empty(B, Tq, E, device=dev, dtype=torch.float32)
        lse_main = torch.empty(B, heads, Tq, device=dev, dtype=torch.float32)
        cbuf = torch.empty(B, heads, Tq, device=dev, dtype=torch.float32)
        attn_fwd(heads, Q, KV, pk, lse_main, qpad, kpad, causal, scale, v=KV, what="attention extra keys: P K")
    _lib.check(lib.mrg_attention_extra_bwd(
        B, heads, Tq, D, _ptr(Q), Tq * E, E, _ptr(bias_k), _ptr(bias_v), scale, _ptr(O), Tq * E, E, _ptr(lse),
        _ptr(dO), Tq * E, E, _ptr(dQ), Tq * E, E, _ptr(gk), _ptr(gv), acc, Tk, thr, sk, _ptr(key),
        _ptr(pk), Tq * E, E, _ptr(lse_main), _ptr(cbuf), _ptr(ws), _stream()), "attention extra keys bwd")
    if cbuf is not None:
        z = zeros(E, device=dev)   # dO = 0 for every query: one row, strides 0
        attn_bwd(heads, Q, KV, O, lse, qpad, kpad, causal, scale, z, dQ, dKV, cbuf, chunk=(0, Tq), passes=2,
                 kv_accumulate=1, what="attention extra keys: dK delta term")


class _MHAOneKeyFn(Function):
    """nn.MultiheadAttention when every query sees exactly one key (Tq = Tk = 1: a frame of the
    generation loops attending to one partner / audio frame, lstmformer.py:498-521).  Softmax over a
    single visible key is exactly 1, so the attention output IS the value projection (bitwise the
    SDPA result: P = exp(s - s) / 1 = 1, O = 1 * V); the query / key projections and the attention
    kernel are skipped.  A row the mask rules hide entirely (query AND key padding) is NaN, as the
    softmax over an all -inf row is.  Gradients: dV = dO; the query and key projections get none
    (the reference's dS = P (dP - rowsum(dO O)) is 0 up to rounding there)."""

    @staticmethod
    @_keeps_precision
    def forward(ctx, spec, q_in, kv_in, in_w, in_b, out_w, out_b, qpad, kpad, gamma=None, beta=None):
        eps, addq = spec.eps, spec.addq   # addq: q added by the output projection's epilogue 3
        _lib.require_device(q_in)
        dev = q_in.device
        B, _, E = q_in.shape
        q2 = q_in.reshape(B, E).contiguous()
        kv2 = kv_in.reshape(B, E).contiguous()
        V = torch.empty(B, E, device=dev, dtype=torch.float32)
        gemm(B, E, E, _ptr(kv2), 0, E, _ptr(in_w, 2 * E * E), 1, E, _ptr(V), E, bias=_ptr(in_b, 2 * E), device=dev)
        hide = None
        O = V
        if qpad is not None and kpad is not None:
            hide = (qpad.reshape(B, 1) & kpad.reshape(B, 1)).bool()
            O = torch.where(hide, torch.full_like(V, float("nan")), V)
        out = torch.empty(B, E, device=dev, dtype=torch.float32)
        kw = dict(epi=3, aux=_ptr(q2), ldaux=E) if addq else {}
        gemm(B, E, E, _ptr(O), 0, E, _ptr(out_w), 1, E, _ptr(out), E, bias=_ptr(out_b), device=dev, **kw)
        res = out
        ln = {}
        if eps is not None:
            u, mean, rstd = _resln_fwd(out, q2, gamma, beta, eps)
            res = u
            ln = dict(out=out, gamma=gamma, beta=beta, mean=mean, rstd=rstd)
        _save(ctx, q2=q2, kv2=kv2, O=O, in_w=in_w, in_b=in_b, out_w=out_w, out_b=out_b, **ln)
        ctx.hide = hide
        ctx.resln = eps is not None
        ctx.addq = addq
        return res.view(B, 1, E)

    @staticmethod
    @_keeps_precision
    def backward(ctx, dout):
        s = _saved(ctx)
        q2, kv2, O, in_w, in_b, out_w, out_b = s.q2, s.kv2, s.O, s.in_w, s.in_b, s.out_w, s.out_b
        B, E = q2.shape
        dev = dout.device
        g = None
        if ctx.resln:
            g = _resln_bwd(dout.reshape(B, E).contiguous(), s.out, q2, s.gamma, s.beta, s.mean, s.rstd)
            do2 = g
        else:
            do2 = dout.reshape(B, E).contiguous()
            if ctx.addq:
                g = do2
        dO = torch.empty(B, E, device=dev, dtype=torch.float32)
        gemm(B, E, E, _ptr(do2), 0, E, _ptr(out_w), 0, E, _ptr(dO), E, device=dev)
        _wgrad(_ptr(do2), E, _ptr(O), E, B, E, E, _gbuf(out_w), dev, gb=_gbuf(out_b), keep=(do2, O))
        if ctx.hide is not None:  # hidden rows: O is the constant NaN, nothing flows to V
            dO = torch.where(ctx.hide, torch.zeros_like(dO), dO)
        gw, gb = _gbuf(in_w), _gbuf(in_b)
        _wgrad(_ptr(dO), E, _ptr(kv2), E, B, E, E, None if gw is None else gw[2 * E:], dev,
               gb=None if gb is None else gb[2 * E:], keep=(dO, kv2))
        dkv = None
        if ctx.needs_input_grad[2]:
            dkv = torch.empty(B, 1, E, device=dev, dtype=torch.float32)
            gemm(B, E, E, _ptr(dO), 0, E, _ptr(in_w, 2 * E * E), 0, E, _ptr(dkv), E, device=dev)
        dq = g.view(B, 1, E) if (g is not None and ctx.needs_input_grad[1]) else None
        return None, dq, dkv, None, None, None, None, None, None, None, None


def _one_key(q, kv):
    return q.dim() == 3 and q.shape[1] == 1 and kv.shape[1] == 1 and kv.shape[-1] == q.shape[-1]


def _mha(q, kv, in_proj_weight, in_proj_bias, out_weight, out_bias, heads, causal, qpad, kpad, dropout_p,
         eps, ln, addq, *, bias_k=None, bias_v=None, add_zero_attn=False, need_weights=False,
         average_attn_weights=True):
    """The attention Function for these shapes; eps not None: LN(. + q) with ln = (gamma, beta); addq:
    . + q without a LayerNorm.  The keywords (the three public forms pass theirs on): bias_k / bias_v
    ([1, 1, E] or [E]; both or neither) and add_zero_attn: nn.MultiheadAttention's extra keys, visible to
    every query whatever the mask rules say.  With one the
    call is always the unchunked _MHAFn: the one-key form does not apply (there is more than one key),
    and the query-chunked schedules (encoder_stack, integrate) never see such a module
    (forms.integrator_form declines it), so the merge has no chunk form.
    need_weights: return (out, weights), weights [B, Tq, Tk + n] (average_attn_weights) or
    [B, heads, Tq, Tk + n] as nn.MultiheadAttention returns them, rebuilt by one more launch from what the
    op holds (_weights).  They carry no gradient (requires_grad False: unlike torch, nothing trains through
    them); out and its backward are the op's without them, launch for launch and draw for draw."""
    if in_proj_weight.shape[0] != 3 * q.shape[-1]:
        raise ValueError("in_proj_weight must be [3E, E]")
    p = float(dropout_p)
    _drop_consts(p)
    want = ("mean" if average_attn_weights else "heads") if need_weights else None
    if (bias_k is None) != (bias_v is None):
        raise ValueError("mha: bias_k and bias_v come together")
    for t in (bias_k, bias_v):
        if t is not None and (t.numel() != q.shape[-1] or t.dtype != torch.float32 or not t.is_contiguous()
                              or t.device != q.device):
            raise ValueError("mha: bias_k / bias_v must be contiguous float32 [1, 1, E] on the query's device")
    extra = bias_k is not None or add_zero_attn
    spec = MHASpec(heads, bool(causal), eps, p, bool(addq), bool(add_zero_attn), want)
    args = (spec, q, kv, in_proj_weight, in_proj_bias, out_weight, out_bias, qpad, kpad, *ln)
    if not extra and p == 0.0 and _one_key(q, kv):   # with dropout the single probability 1 is still dropped: _MHAFn
        out = _MHAOneKeyFn.apply(*args)
        return (out, _one_key_weights(q, heads, qpad, kpad, want == "mean")) if want else out
    return _MHAFn.apply(*args, bias_k, bias_v)


def mha(q, kv, in_proj_weight, in_proj_bias, out_weight, out_bias, heads, causal=False,
        qpad=None, kpad=None, dropout_p=0.0, **kw):
    """nn.MultiheadAttention(batch_first, kdim=vdim=E)(q, kv, kv) with the reference mask rules.
    dropout_p > 0: dropout on the attention probabilities (the module's training mode).
    Keywords (_mha's): bias_k / bias_v, add_zero_attn: the module's add_bias_kv / add_zero_attn keys;
    need_weights, average_attn_weights: (out, weights), the attention probabilities without a gradient."""
    return _mha(q, kv, in_proj_weight, in_proj_bias, out_weight, out_bias, heads, causal, qpad, kpad, dropout_p,
                None, (None, None), False, **kw)


def mha_residual_layernorm(q, kv, in_proj_weight, in_proj_bias, out_weight, out_bias, heads, gamma, beta,
                           eps=1e-5, causal=False, qpad=None, kpad=None, dropout_p=0.0, **kw):
    """LN(MHA(q, kv, kv) + q): ResidualConnection(MHAMixer) (mixer_block.py:567-603); the query
    projection's input-gradient GEMM takes the residual gradient in its epilogue.  Keywords as mha's."""
    return _mha(q, kv, in_proj_weight, in_proj_bias, out_weight, out_bias, heads, causal, qpad, kpad, dropout_p,
                float(eps), (gamma, beta), False, **kw)


def mha_residual(q, kv, in_proj_weight, in_proj_bias, out_weight, out_bias, heads, causal=False,
                 qpad=None, kpad=None, dropout_p=0.0, **kw):
    """MHA(q, kv, kv) + q: ResidualConnection(MHAMixer) without a LayerNorm.  q is added by the output
    projection's GEMM (epilogue 3) in both forms of mha, and the gradient of the sum by the query
    projection's input-gradient GEMM (the one-key form has no query projection: there dq is the
    gradient itself).  Keywords as mha's."""
    return _mha(q, kv, in_proj_weight, in_proj_bias, out_weight, out_bias, heads, causal, qpad, kpad, dropout_p,
                None, (None, None), True, **kw)


