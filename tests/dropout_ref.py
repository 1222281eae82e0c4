"""float64 torch restatements of the ops that drop, taking an EXPLICIT keep mask (so the tests can hand
them the mask the kernels used): nn.MultiheadAttention with the reference mask rules and dropout on the
attention probabilities, and stacked nn.LSTM / nn.GRU with inter-layer dropout built from single-layer
torch modules in double."""
import math

import numpy as np
import torch


def keep_scale(p):
    """The factor the kernels multiply kept values by: 1 / (1 - p) rounded to float32."""
    return float(np.float32(1.0 / (1.0 - p)))


def visible(Tq, Tk, causal, qpad=None, kpad=None, B=1):
    """bool [B, Tq, Tk]: query i may see key j (gen_attention_mask: the block-causal rule over the length
    ratio, and padding hides a pair only when BOTH the query and the key are padding)."""
    i = torch.arange(Tq).view(Tq, 1)
    j = torch.arange(Tk).view(1, Tk)
    if not causal:
        vis = torch.ones(Tq, Tk, dtype=torch.bool)
    elif Tk >= Tq:
        vis = j < (i + 1) * (Tk // Tq)
    else:
        vis = j <= i // (Tq // Tk)
    vis = vis.unsqueeze(0).expand(B, Tq, Tk).clone()
    if qpad is not None and kpad is not None:
        vis &= ~(qpad.bool().view(B, Tq, 1) & kpad.bool().view(B, 1, Tk))
    return vis


def mha(q, kv, in_w, in_b, out_w, out_b, heads, causal=False, qpad=None, kpad=None, keep=None, p=0.0):
    """q [B, Tq, E], kv [B, Tk, E] (double); keep: bool [B, heads, Tq, Tk] or None.  The softmax is over the
    undropped scores; the probabilities are then multiplied by keep / (1 - p).  A fully hidden row is NaN."""
    B, Tq, E = q.shape
    Tk = kv.shape[1]
    D = E // heads
    Q = (q @ in_w[:E].T + in_b[:E]).view(B, Tq, heads, D).transpose(1, 2)
    K = (kv @ in_w[E:2 * E].T + in_b[E:2 * E]).view(B, Tk, heads, D).transpose(1, 2)
    V = (kv @ in_w[2 * E:].T + in_b[2 * E:]).view(B, Tk, heads, D).transpose(1, 2)
    S = Q @ K.transpose(-1, -2) / math.sqrt(D)
    vis = visible(Tq, Tk, causal, qpad, kpad, B).unsqueeze(1)
    S = S.masked_fill(~vis, float("-inf"))
    P = torch.softmax(S, dim=-1)
    if keep is not None:
        P = P * (keep.to(P.dtype) * keep_scale(p))
    O = (P @ V).transpose(1, 2).reshape(B, Tq, E)
    return O @ out_w.T + out_b


def stacked_rnn(kind, module, x, keeps=None, p=0.0):
    """The stack of ``module`` (layers.LSTM / layers.GRU: its parameters, sizes and directions) over x in
    double, each layer one single-layer torch.nn.LSTM / nn.GRU; keeps[l] (bool, the shape of layer l's
    output) is applied to the output of layer l, for every layer but the last.
    Returns (y, final states as nn.LSTM / nn.GRU stack them, the torch layers)."""
    cls = torch.nn.LSTM if kind == "lstm" else torch.nn.GRU
    D = 2 if module.bidirectional else 1
    layers, hs, cs = [], [], []
    for l in range(module.num_layers):
        in_sz = module.input_size if l == 0 else module.hidden_size * D
        rnn = cls(in_sz, module.hidden_size, 1, batch_first=True, bidirectional=module.bidirectional).double()
        with torch.no_grad():
            for d in range(D):
                src, dst = f"l{l}" + ("_reverse" if d else ""), "l0" + ("_reverse" if d else "")
                for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                    getattr(rnn, f"{n}_{dst}").copy_(getattr(module, f"{n}_{src}").detach().double().cpu())
        layers.append(rnn)
        if l and keeps is not None:
            x = x * (keeps[l - 1].to(x.dtype) * keep_scale(p))
        x, st = rnn(x)
        if kind == "lstm":
            hs.append(st[0])
            cs.append(st[1])
        else:
            hs.append(st)
    state = (torch.cat(hs), torch.cat(cs)) if kind == "lstm" else torch.cat(hs)
    return x, state, layers
