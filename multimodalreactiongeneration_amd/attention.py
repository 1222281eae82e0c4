"""The device dropout RNG, dropout, and multi-head attention."""
import math

import torch
from torch.autograd import Function

from . import _lib
from .dense import _resln_bwd, _resln_fwd
from .gemm_ops import _dx_gemm, _fwd_gemm, _wgrad, _wt_note, gemm
from .launch import _flush_touched, _gbuf, _keeps_precision, _probe, _ptr, _stream, _ws, zeros

# --- dropout RNG (csrc/rng.h, rng.py): a per-device {seed, draw} state in device memory.  An op that
# drops takes one draw with a one-thread kernel (a graph node: a replayed step takes fresh draws) and
# keeps the 16-byte key tensor for its backward.  All DDP ranks share the default seed unless the
# caller seeds per rank (manual_seed(base + rank)).
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


# ------------------------------------------------------------------ multi-head attention
def visible_pairs(Tq, Tk, causal):
    """(query, key) pairs the block-causal rule admits per (sample, head) (gen_attention_mask rules)."""
    if not causal:
        return Tq * Tk
    if Tk >= Tq:
        r = Tk // Tq
        return sum(min((i + 1) * r, Tk) for i in range(Tq))
    r = Tq // Tk
    return sum(min(i // r + 1, Tk) for i in range(Tq))


def _attn_args(heads, Q, KV, O, lse, qpad, kpad, causal, scale):
    """The leading arguments every attention entry point takes: shapes, Q, K and V (the two halves of
    KV), O, the row log-sum-exps, the padding flags and the mask rule."""
    B, Tq, E = Q.shape
    Tk = KV.shape[1]
    return (B, heads, Tq, Tk, E // heads, _ptr(Q), Tq * E, E, _ptr(KV), Tk * 2 * E, 2 * E, _ptr(KV, E), Tk * 2 * E,
            2 * E, _ptr(O), Tq * E, E, _ptr(lse), _ptr(qpad), _ptr(kpad), int(causal), scale)


class _MHAFn(Function):
    @staticmethod
    @_keeps_precision
    def forward(ctx, spec, q_in, kv_in, in_w, in_b, out_w, out_b, qpad, kpad, gamma=None, beta=None,
                bias_k=None, bias_v=None):
        # eps not None: return LN(attn + q) (ResidualConnection(MHAMixer)); p > 0: dropout on the
        # attention probabilities with one draw, the key saved for the backward
        # addq: return attn + q (the residual without a LayerNorm), q added by the output projection's
        # epilogue 3
        heads, causal, eps, *rest = spec
        p = rest[0] if rest else 0.0
        addq = bool(rest[1]) if len(rest) > 1 else False
        # extra always-visible keys (add_bias_kv: bias_k / bias_v; add_zero_attn: rest[2]): one merge launch
        # after the attention kernel (_extra_fwd)
        zero_attn = bool(rest[2]) if len(rest) > 2 else False
        # need_weights (rest[3]: None, "mean" or "heads"): a second, non-differentiable output, the attention
        # probabilities rebuilt from Q, K and lse by one more launch (_weights)
        want = rest[3] if len(rest) > 3 else None
        _lib.require_device(q_in)
        dev = q_in.device
        B, Tq, E = q_in.shape
        Tk = kv_in.shape[1]
        D = E // heads
        q2 = q_in.contiguous()
        kv2 = kv_in.contiguous()
        Q = torch.empty(B, Tq, E, device=dev, dtype=torch.float32)
        _fwd_gemm(B * Tq, E, E, _ptr(q2), E, in_w[:E], _ptr(Q), E, bias=_ptr(in_b), device=dev)
        KV = torch.empty(B, Tk, 2 * E, device=dev, dtype=torch.float32)
        _fwd_gemm(B * Tk, 2 * E, E, _ptr(kv2), E, in_w[E:], _ptr(KV), 2 * E, bias=_ptr(in_b, E), device=dev)
        O = torch.empty(B, Tq, E, device=dev, dtype=torch.float32)
        lse = torch.empty(B, heads, Tq, device=dev, dtype=torch.float32)
        scale = 1.0 / math.sqrt(D)
        lib = _lib.load()
        args = _attn_args(heads, Q, KV, O, lse, qpad, kpad, causal, scale)
        drop = None
        if p > 0.0:
            thr, sk = _drop_consts(p)
            drop = (thr, sk, _rng_draw(dev))
            rc = lib.mrg_attention_fwd_dropout(*args, thr, sk, _ptr(drop[2]), _stream())
        else:
            with _probe("attn_fwd", 4.0 * D * B * heads * visible_pairs(Tq, Tk, causal)):
                rc = lib.mrg_attention_fwd(*args, _stream())
        _lib.check(rc, "attention fwd")
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
        extra = []
        res = out
        if eps is not None:
            u, mean, rstd = _resln_fwd(out.view(B * Tq, E), q2.view(B * Tq, E), gamma, beta, eps)
            res = u.view(B, Tq, E)
            extra = [out, gamma, beta, mean, rstd]
        if bias_k is not None:
            extra = extra + [bias_k, bias_v]
        ctx.save_for_backward(q2, kv2, Q, KV, O, lse, in_w, in_b, out_w, out_b, qpad, kpad, *extra)
        ctx.has_bias_kv = bias_k is not None
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
        saved = ctx.saved_tensors
        q2, kv2, Q, KV, O, lse, in_w, in_b, out_w, out_b, qpad, kpad = saved[:12]
        heads, causal, scale, resln = ctx.spec
        B, Tq, E = q2.shape
        Tk = kv2.shape[1]
        D = E // heads
        dev = dout.device
        lib = _lib.load()
        g = None  # residual-branch gradient of LN(attn + q), added by the dq GEMM's epilogue
        if resln:
            out, gamma, beta, mean, rstd = saved[12:17]
            g = _resln_bwd(dout.reshape(B * Tq, E).contiguous(), out.view(B * Tq, E), q2.view(B * Tq, E),
                           gamma, beta, mean, rstd)
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
        ws = _ws(lib.mrg_attention_bwd_workspace_bytes(B, heads, Tq), dev)
        args = _attn_args(heads, Q, KV, O, lse, qpad, kpad, causal, scale) + (
            _ptr(dO), Tq * E, E, _ptr(dQ), Tq * E, E, _ptr(dKV), Tk * 2 * E, 2 * E, _ptr(dKV, E), Tk * 2 * E, 2 * E,
            _ptr(ws))
        if ctx.drop is not None:
            thr, sk, key = ctx.drop
            rc = lib.mrg_attention_bwd_dropout(*args, thr, sk, _ptr(key), _stream())
        else:
            with _probe("attn_bwd", 10.0 * D * B * heads * visible_pairs(Tq, Tk, causal)):
                rc = lib.mrg_attention_bwd(*args, _stream())
        _lib.check(rc, "attention bwd")
        if ctx.has_bias_kv:   # the zero key alone has no gradient: the merged O / lse did it all
            _extra_bwd(heads, Q, KV, O, lse, qpad, kpad, causal, scale, saved[-2:], dO, dQ, dKV, ctx.drop)
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
        _lib.check(lib.mrg_attention_fwd(B, heads, Tq, Tk, D, _ptr(Q), Tq * E, E, _ptr(KV), Tk * 2 * E, 2 * E,
                                         _ptr(KV), Tk * 2 * E, 2 * E, _ptr(pk), Tq * E, E, _ptr(lse_main),
                                         _ptr(qpad), _ptr(kpad), int(causal), scale, _stream()),
                   "attention extra keys: P K")
    _lib.check(lib.mrg_attention_extra_bwd(
        B, heads, Tq, D, _ptr(Q), Tq * E, E, _ptr(bias_k), _ptr(bias_v), scale, _ptr(O), Tq * E, E, _ptr(lse),
        _ptr(dO), Tq * E, E, _ptr(dQ), Tq * E, E, _ptr(gk), _ptr(gv), acc, Tk, thr, sk, _ptr(key),
        _ptr(pk), Tq * E, E, _ptr(lse_main), _ptr(cbuf), _ptr(ws), _stream()), "attention extra keys bwd")
    if cbuf is not None:
        z = zeros(E, device=dev)   # dO = 0 for every query: one row, strides 0
        _lib.check(lib.mrg_attention_bwd_chunk(
            B, heads, Tq, Tk, D, 0, Tq, _ptr(Q), Tq * E, E, _ptr(KV), Tk * 2 * E, 2 * E, _ptr(KV, E), Tk * 2 * E,
            2 * E, _ptr(O), Tq * E, E, _ptr(lse), _ptr(qpad), _ptr(kpad), int(causal), scale, _ptr(z), 0, 0,
            _ptr(dQ), Tq * E, E, _ptr(dKV), Tk * 2 * E, 2 * E, _ptr(dKV, E), Tk * 2 * E, 2 * E, 2, 1, _ptr(cbuf),
            _stream()), "attention extra keys: dK delta term")


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
    def forward(ctx, eps, q_in, kv_in, in_w, in_b, out_w, out_b, qpad, kpad, gamma=None, beta=None):
        addq = eps == "add"   # attn + q without a LayerNorm: q added by the output projection's epilogue 3
        eps = None if addq else eps
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
        extra = []
        if eps is not None:
            u, mean, rstd = _resln_fwd(out, q2, gamma, beta, eps)
            res = u
            extra = [out, gamma, beta, mean, rstd]
        ctx.save_for_backward(q2, kv2, O, in_w, in_b, out_w, out_b, *extra)
        ctx.hide = hide
        ctx.resln = eps is not None
        ctx.addq = addq
        return res.view(B, 1, E)

    @staticmethod
    @_keeps_precision
    def backward(ctx, dout):
        saved = ctx.saved_tensors
        q2, kv2, O, in_w, in_b, out_w, out_b = saved[:7]
        B, E = q2.shape
        dev = dout.device
        g = None
        if ctx.resln:
            out, gamma, beta, mean, rstd = saved[7:]
            g = _resln_bwd(dout.reshape(B, E).contiguous(), out, q2, gamma, beta, mean, rstd)
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
         eps=None, ln=(), addq=False, bias_k=None, bias_v=None, add_zero_attn=False, need_weights=False,
         average_attn_weights=True):
    """The attention Function for these shapes; eps not None: LN(. + q) with ln = (gamma, beta); addq:
    . + q without a LayerNorm.  bias_k / bias_v ([1, 1, E] or [E]; both or neither) and add_zero_attn:
    nn.MultiheadAttention's extra keys, visible to every query whatever the mask rules say.  With one the
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
    if bias_k is not None or add_zero_attn:
        E = q.shape[-1]
        for t in (bias_k, bias_v):
            if t is not None and (t.numel() != E or t.dtype != torch.float32 or not t.is_contiguous()
                                  or t.device != q.device):
                raise ValueError("mha: bias_k / bias_v must be contiguous float32 [1, 1, E] on the query's device")
        lnp = ln if ln else (None, None)
        spec = (heads, bool(causal), eps, p, bool(addq), bool(add_zero_attn)) + ((want,) if want else ())
        return _MHAFn.apply(spec, q, kv, in_proj_weight, in_proj_bias, out_weight, out_bias, qpad, kpad, *lnp,
                            bias_k, bias_v)
    if p == 0.0 and _one_key(q, kv):   # with dropout the single probability 1 is still dropped: _MHAFn
        out = _MHAOneKeyFn.apply("add" if addq else eps, q, kv, in_proj_weight, in_proj_bias, out_weight, out_bias,
                                 qpad, kpad, *ln)
        return (out, _one_key_weights(q, heads, qpad, kpad, want == "mean")) if want else out
    spec = (heads, bool(causal), eps, p, bool(addq)) + ((False, want) if want else ())
    return _MHAFn.apply(spec, q, kv, in_proj_weight, in_proj_bias, out_weight, out_bias, qpad, kpad, *ln)


def mha(q, kv, in_proj_weight, in_proj_bias, out_weight, out_bias, heads, causal=False,
        qpad=None, kpad=None, dropout_p=0.0, bias_k=None, bias_v=None, add_zero_attn=False,
        need_weights=False, average_attn_weights=True):
    """nn.MultiheadAttention(batch_first, kdim=vdim=E)(q, kv, kv) with the reference mask rules.
    dropout_p > 0: dropout on the attention probabilities (the module's training mode).
    bias_k / bias_v, add_zero_attn: the module's add_bias_kv / add_zero_attn keys (see _mha).
    need_weights: (out, weights) with the attention probabilities, no gradient through them (see _mha)."""
    return _mha(q, kv, in_proj_weight, in_proj_bias, out_weight, out_bias, heads, causal, qpad, kpad, dropout_p,
                bias_k=bias_k, bias_v=bias_v, add_zero_attn=add_zero_attn, need_weights=need_weights,
                average_attn_weights=average_attn_weights)


def mha_residual_layernorm(q, kv, in_proj_weight, in_proj_bias, out_weight, out_bias, heads, gamma, beta,
                           eps=1e-5, causal=False, qpad=None, kpad=None, dropout_p=0.0, bias_k=None, bias_v=None,
                           add_zero_attn=False, need_weights=False, average_attn_weights=True):
    """LN(MHA(q, kv, kv) + q): ResidualConnection(MHAMixer) (mixer_block.py:567-603); the query
    projection's input-gradient GEMM takes the residual gradient in its epilogue."""
    return _mha(q, kv, in_proj_weight, in_proj_bias, out_weight, out_bias, heads, causal, qpad, kpad, dropout_p,
                float(eps), (gamma, beta), bias_k=bias_k, bias_v=bias_v, add_zero_attn=add_zero_attn,
                need_weights=need_weights, average_attn_weights=average_attn_weights)


def mha_residual(q, kv, in_proj_weight, in_proj_bias, out_weight, out_bias, heads, causal=False,
                 qpad=None, kpad=None, dropout_p=0.0, bias_k=None, bias_v=None, add_zero_attn=False,
                 need_weights=False, average_attn_weights=True):
    """MHA(q, kv, kv) + q: ResidualConnection(MHAMixer) without a LayerNorm.  q is added by the output
    projection's GEMM (epilogue 3) in both forms of mha, and the gradient of the sum by the query
    projection's input-gradient GEMM (the one-key form has no query projection: there dq is the
    gradient itself)."""
    return _mha(q, kv, in_proj_weight, in_proj_bias, out_weight, out_bias, heads, causal, qpad, kpad, dropout_p,
                addq=True, bias_k=bias_k, bias_v=bias_v, add_zero_attn=add_zero_attn, need_weights=need_weights,
                average_attn_weights=average_attn_weights)
