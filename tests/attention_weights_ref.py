"""float64 references of nn.MultiheadAttention(need_weights=True) under the reference mask rules: the
restatement of tests/attention_extra_ref.core that also RETURNS the probabilities (an explicit keep mask
of width Tk + n_extra, the extra keys, the head-average switch), and
torch.nn.functional.multi_head_attention_forward itself asked for its weights
(tests/test_cpu_attention_weights.py proves the first against the second).  The kernel cases of
tests/test_gpu_attention_weights.py and the row-sum bound live here too.  A plain helper."""
import functools
import math
from collections import namedtuple

import torch

from tests.dropout_ref import keep_scale, visible

# (Tq, Tk, E, heads, causal, ragged): D = 64 across the 64-tile edge; D = 32 with Tk = 2 Tq and padding;
# Tq = 2 Tk; D = 8 with odd widths; D = 16; one key
Case = namedtuple("Case", "Tq Tk E heads causal ragged")
CASES = [Case(70, 70, 128, 2, False, False), Case(37, 74, 64, 2, True, True), Case(40, 20, 128, 4, True, False),
         Case(33, 33, 32, 4, False, False), Case(20, 20, 64, 4, True, False), Case(1, 1, 64, 2, False, False)]
B = 2


def probs(Q, K, heads, scale, vis, bias_k=None, zero=False, keep=None, p=0.0, average=False):
    """The attention probabilities of projected Q [B, Tq, E] and K [B, Tk, E], in their dtype: softmax over
    [real keys where vis [B, Tq, Tk] admits them, bias key, zero key], then o keep / (1 - p) with keep bool
    [B, heads, Tq, Tk + n] if given.  Returns (P [B, heads, Tq, Tk + n], or its mean over the heads
    [B, Tq, Tk + n] with ``average``, and lse [B, heads, Tq]).  A fully hidden row with no extra key is NaN."""
    Bq, Tq, E = Q.shape
    Tk, D = K.shape[1], E // heads
    Qh = Q.view(Bq, Tq, heads, D).transpose(1, 2)
    Kh = K.view(Bq, Tk, heads, D).transpose(1, 2)
    S = (Qh @ Kh.transpose(-1, -2) * scale).masked_fill(~vis.unsqueeze(1), float("-inf"))
    cols = [S]
    if bias_k is not None:
        cols.append((Qh * bias_k.reshape(1, heads, 1, D)).sum(-1, keepdim=True) * scale)
    if zero:
        cols.append(torch.zeros(Bq, heads, Tq, 1, dtype=Q.dtype))
    S = torch.cat(cols, -1)
    P = torch.softmax(S, dim=-1)
    if keep is not None:
        P = P * (keep.to(P.dtype) * keep_scale(p))
    return (P.mean(dim=1) if average else P), torch.logsumexp(S, dim=-1)


def mha(q, kv, w, heads, causal=False, qpad=None, kpad=None, zero=False, keep=None, p=0.0, average=True):
    """(out, weights) of the module: projections, the core with its probabilities, output projection.
    w: in_w, in_b, out_w, out_b and, with a bias key, bias_k / bias_v [1, 1, E]."""
    Bq, Tq, E = q.shape
    D = E // heads
    Tk = kv.shape[1]
    x = kv @ w["in_w"][E:].T + w["in_b"][E:]
    Q = q @ w["in_w"][:E].T + w["in_b"][:E]
    vis = visible(Tq, Tk, causal, qpad, kpad, Bq)
    bk = w["bias_k"].reshape(E) if "bias_k" in w else None
    P, _ = probs(Q, x[..., :E], heads, 1.0 / math.sqrt(D), vis, bk, zero, keep, p)
    vals = [x[..., E:].view(Bq, Tk, heads, D).transpose(1, 2)]
    if bk is not None:
        vals.append(w["bias_v"].reshape(1, heads, 1, D).expand(Bq, heads, 1, D))
    if zero:
        vals.append(torch.zeros(Bq, heads, 1, D, dtype=q.dtype))
    O = (P @ torch.cat(vals, 2)).transpose(1, 2).reshape(Bq, Tq, E)
    return O @ w["out_w"].T + w["out_b"], (P.mean(dim=1) if average else P)


def torch_mha(q, kv, w, heads, causal=False, qpad=None, kpad=None, zero=False, average=True):
    """(out, weights) of torch.nn.functional.multi_head_attention_forward(need_weights=True) on the same
    arguments (no dropout), the dense bool attn_mask [B * heads, Tq, Tk] (True: hidden) built from
    dropout_ref.visible."""
    Bq, Tq, E = q.shape
    Tk = kv.shape[1]
    mask = None
    if causal or (qpad is not None and kpad is not None):
        vis = visible(Tq, Tk, causal, qpad, kpad, Bq)
        mask = (~vis).unsqueeze(1).expand(Bq, heads, Tq, Tk).reshape(Bq * heads, Tq, Tk)
    out, wts = torch.nn.functional.multi_head_attention_forward(
        q.transpose(0, 1), kv.transpose(0, 1), kv.transpose(0, 1), E, heads, w["in_w"], w["in_b"],
        w.get("bias_k"), w.get("bias_v"), zero, 0.0, w["out_w"], w["out_b"], training=False,
        need_weights=True, attn_mask=mask, average_attn_weights=average)
    return out.transpose(0, 1), wts


def pads(c, batch=B):
    """(qpad, kpad) uint8 of a ragged case: sample 0 ends in padded queries and keys (so its late queries
    lose their late keys), sample 1 has scattered flags; None, None otherwise."""
    if not c.ragged:
        return None, None
    qpad, kpad = torch.zeros(batch, c.Tq, dtype=torch.uint8), torch.zeros(batch, c.Tk, dtype=torch.uint8)
    qpad[0, c.Tq - max(1, c.Tq // 4):] = 1
    kpad[0, c.Tk - max(1, c.Tk // 3):] = 1
    qpad[1, ::2] = 1
    kpad[1, 1::3] = 1
    return qpad, kpad


@functools.lru_cache(maxsize=None)
def projected(c, seed=0, batch=B):
    """float32 CPU projected Q [B, Tq, E] and KV [B, Tk, 2E] (K | V) of a case; not to be modified."""
    g = torch.Generator().manual_seed(1009 * c.Tq + 31 * c.Tk + c.E + seed)
    return torch.randn(batch, c.Tq, c.E, generator=g), torch.randn(batch, c.Tk, 2 * c.E, generator=g)


def row_sum_dev(P):
    """largest |sum over the last axis - 1| over the finite rows"""
    s = P.double().sum(-1)
    s = s[torch.isfinite(s)]
    return (s - 1).abs().max().item() if s.numel() else 0.0


def row_sum_bound(P64):
    """The row-sum bound of a result whose float64 reference is P64: the largest deviation from 1 the
    reference rounded to float32 shows on these inputs, times 4 (allowance for the fp32 exp and the
    summation order, which the rounded reference does not exercise)."""
    return 4.0 * row_sum_dev(P64.float())
