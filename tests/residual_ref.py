"""float64 torch restatements of the residual connection WITHOUT a LayerNorm around the ops that carry
it, taking explicit parameters: x + linear(x), x + ffn(x), q + mha(q, kv) (tests/dropout_ref.mha, so an
explicit keep mask too) and x + rnn(x) (one layer built by tests/dropout_ref.stacked_rnn)."""
import torch

from tests import dropout_ref

ACTS = {"relu": torch.relu, "tanh": torch.tanh, "silu": torch.nn.functional.silu}


def linear_residual(x, w, b):
    return x + x @ w.T + b


def ffn_residual(x, w1, b1, w2, b2, act):
    return x + ACTS[act](x @ w1.T + b1) @ w2.T + b2


def mha_residual(q, kv, in_w, in_b, out_w, out_b, heads, causal=False, qpad=None, kpad=None, keep=None, p=0.0):
    return q + dropout_ref.mha(q, kv, in_w, in_b, out_w, out_b, heads, causal, qpad, kpad, keep, p)


def rnn_residual(kind, module, x, state=None):
    """x + rnn(x) over the ONE layer of ``module`` (layers.LSTM / layers.GRU, either direction count) in
    double; state: the initial state as nn.LSTM / nn.GRU take it, or None.  Returns (y, final state, the
    torch layer): the layer's parameters carry the gradients."""
    assert module.num_layers == 1
    _, _, layers = dropout_ref.stacked_rnn(kind, module, x.detach())
    rnn = layers[0]
    y, st = rnn(x) if state is None else rnn(x, state)
    return x + y, st, rnn
