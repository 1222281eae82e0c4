"""float64 references of nn.MultiheadAttention with add_bias_kv / add_zero_attn under the reference mask
rules: torch.nn.functional.multi_head_attention_forward itself, handed the dense mask of
dropout_ref.visible (torch pads it with visible columns for the extra keys), and a restatement of the
softmax over [real keys, bias key, zero key] that also takes an explicit keep mask of width Tk + n_extra,
for the dropout cases (tests/test_cpu_attention_extra.py proves it against torch at p = 0).  The shapes,
padding patterns and inputs of tests/test_gpu_attention_extra.py live here too.  A plain helper."""
import functools
import math

import torch

from tests.dropout_ref import keep_scale, visible

COMBOS = {"bias": (True, False), "zero": (False, True), "both": (True, True)}
# (Tq, Tk, causal): one key (never the one-key shortcut), both causal ratios, a 64-query block crossed
SHAPES = [(1, 1, False), (5, 10, True), (10, 5, True), (70, 70, False)]
B = 3


def n_extra(combo):
    return sum(COMBOS[combo])


def pads(Tq, Tk, causal):
    """(qpad, kpad) uint8 [3, Tq] / [3, Tk].  Sample 0: every key flagged and query min(2, Tq - 1) flagged:
    that query's real keys are all hidden, the sample's other queries see theirs.  Sample 1: every third
    key and every other query.  Sample 2: no flags."""
    qpad, kpad = torch.zeros(B, Tq, dtype=torch.uint8), torch.zeros(B, Tk, dtype=torch.uint8)
    kpad[0, :] = 1
    qpad[0, min(2, Tq - 1)] = 1
    kpad[1, 1::3] = 1
    qpad[1, ::2] = 1
    return qpad, kpad


def hidden_rows(Tq, Tk, causal):
    """bool [3, Tq]: queries whose real keys are all hidden"""
    qpad, kpad = pads(Tq, Tk, causal)
    return ~visible(Tq, Tk, causal, qpad, kpad, B).any(-1)


def core(q, k, v, heads, scale, vis, bias_k, bias_v, zero, keep=None, p=0.0):
    """The attention core with the extra keys, in the dtype of its inputs.  q [B, Tq, E], k / v [B, Tk, E],
    vis bool [B, Tq, Tk], bias_k / bias_v [E] or None, zero: the all-zero key; keep bool
    [B, heads, Tq, Tk + n_extra] or None.  Returns O [B, Tq, E] and lse [B, heads, Tq] over every key."""
    Bq, Tq, E = q.shape
    Tk, D = k.shape[1], E // heads
    Q = q.view(Bq, Tq, heads, D).transpose(1, 2)
    K = k.view(Bq, Tk, heads, D).transpose(1, 2)
    V = v.view(Bq, Tk, heads, D).transpose(1, 2)
    S = (Q @ K.transpose(-1, -2) * scale).masked_fill(~vis.unsqueeze(1), float("-inf"))
    cols, vals = [S], [V]
    if bias_k is not None:
        bk, bv = bias_k.view(1, heads, 1, D), bias_v.view(1, heads, 1, D)
        cols.append((Q * bk).sum(-1, keepdim=True) * scale)
        vals.append(bv.expand(Bq, heads, 1, D))
    if zero:
        cols.append(torch.zeros(Bq, heads, Tq, 1, dtype=q.dtype))
        vals.append(torch.zeros(Bq, heads, 1, D, dtype=q.dtype))
    S, V = torch.cat(cols, -1), torch.cat(vals, 2)
    P = torch.softmax(S, dim=-1)
    if keep is not None:
        P = P * (keep.to(P.dtype) * keep_scale(p))
    return (P @ V).transpose(1, 2).reshape(Bq, Tq, E), torch.logsumexp(S, dim=-1)


def mha(q, kv, w, heads, causal=False, qpad=None, kpad=None, zero=False, keep=None, p=0.0):
    """The restatement: projections, core, output projection.  w: in_w, in_b, out_w, out_b and, with a bias
    key, bias_k / bias_v [1, 1, E]."""
    Bq, Tq, E = q.shape
    x = kv @ w["in_w"][E:].T + w["in_b"][E:]
    vis = visible(Tq, kv.shape[1], causal, qpad, kpad, Bq)
    bk = w["bias_k"].reshape(E) if "bias_k" in w else None
    bv = w["bias_v"].reshape(E) if "bias_v" in w else None
    O, _ = core(q @ w["in_w"][:E].T + w["in_b"][:E], x[..., :E], x[..., E:], heads, 1.0 / math.sqrt(E // heads), vis,
                bk, bv, zero, keep, p)
    return O @ w["out_w"].T + w["out_b"]


def torch_mha(q, kv, w, heads, causal=False, qpad=None, kpad=None, zero=False):
    """torch.nn.functional.multi_head_attention_forward on the same arguments (no dropout), the dense
    attn_mask [B * heads, Tq, Tk] (True: hidden) materialised from the mask rules."""
    Bq, Tq, E = q.shape
    Tk = kv.shape[1]
    mask = None
    if causal or (qpad is not None and kpad is not None):
        vis = visible(Tq, Tk, causal, qpad, kpad, Bq)
        mask = (~vis).unsqueeze(1).expand(Bq, heads, Tq, Tk).reshape(Bq * heads, Tq, Tk)
    out, _ = torch.nn.functional.multi_head_attention_forward(
        q.transpose(0, 1), kv.transpose(0, 1), kv.transpose(0, 1), E, heads, w["in_w"], w["in_b"],
        w.get("bias_k"), w.get("bias_v"), zero, 0.0, w["out_w"], w["out_b"], training=False,
        need_weights=False, attn_mask=mask)
    return out.transpose(0, 1)


@functools.lru_cache(maxsize=None)
def weights(E, combo, seed=0):
    """float32 CPU weights of one module; not to be modified."""
    g = torch.Generator().manual_seed(977 * E + seed)
    w = {"in_w": torch.randn(3 * E, E, generator=g) / math.sqrt(E), "in_b": torch.randn(3 * E, generator=g) * 0.1,
         "out_w": torch.randn(E, E, generator=g) / math.sqrt(E), "out_b": torch.randn(E, generator=g) * 0.1}
    if COMBOS[combo][0]:
        w["bias_k"] = torch.randn(1, 1, E, generator=g)
        w["bias_v"] = torch.randn(1, 1, E, generator=g)
    return w


@functools.lru_cache(maxsize=None)
def inputs(Tq, Tk, E, seed=0):
    """float32 CPU q [3, Tq, E], kv / k / v [3, Tk, E], dout [3, Tq, E]; not to be modified."""
    g = torch.Generator().manual_seed(31 * Tq + 7 * Tk + E + seed)
    return {n: torch.randn(B, T, E, generator=g) for n, T in (("q", Tq), ("kv", Tk), ("k", Tk), ("v", Tk), ("dout", Tq))}


def grads(fn, q, kv, w, dout):
    """(out, dq, dkv, {name: dweight}) of fn(q, kv, w) in double by autograd"""
    q, kv = (t.double().requires_grad_(True) for t in (q, kv))
    w = {n: t.double().requires_grad_(True) for n, t in w.items()}
    out = fn(q, kv, w)
    out.backward(dout.double())
    return out.detach(), q.grad, kv.grad, {n: t.grad for n, t in w.items()}
