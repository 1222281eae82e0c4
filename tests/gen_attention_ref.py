"""Float64 restatement of mrg_gen_attention (csrc/gen.hip): one query row per sample over the r keys
of a generated frame, no mask (MultiModalAttentionBlockSequential at Tq = 1, multi_modal_att.py:22-31)."""
import math

import torch

E = 256


def gen_attention_ref(q, k, v, heads):
    """q [B, 256] (projected, bias added), k / v [B, r, 256] (projected), heads -> ctx [B, 256] float64:
    per head h of width D = 256 / heads, softmax_j(q_h . k_hj / sqrt(D)) over the r keys weighs v_hj; the
    heads are concatenated (the context before out_proj)."""
    B, r, _ = k.shape
    D = E // heads
    qh = q.double().reshape(B, heads, 1, D)
    kh = k.double().reshape(B, r, heads, D).transpose(1, 2)
    vh = v.double().reshape(B, r, heads, D).transpose(1, 2)
    p = torch.softmax(qh @ kh.transpose(-1, -2) / math.sqrt(D), dim=-1)   # [B, heads, 1, r]
    return (p @ vh).reshape(B, E)
