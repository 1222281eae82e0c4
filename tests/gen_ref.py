"""Float64 restatements of the per-launch generation kernels' entry points (csrc/gen.hip): mrg_gen_lstm,
mrg_gen_gru, mrg_gen_linear, mrg_gen_ffn and mrg_gen_attention.  Inputs of any float dtype, results float64."""
import math

import torch

E = 256


def _d(t):
    return t.double()


def _ln(x, ga, be, eps):
    """torch.layer_norm over the last axis: biased variance, eps inside the root."""
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * _d(ga) + _d(be)


def _mixer_x(ms, fe_w, fe_b, a, r, ga, be, eps):
    """The recurrent mixers' input rows: X = ms fe_w^T + fe_b (ms [B, fm]) when ms is given, else LN(a + r)."""
    if ms is not None:
        return _d(ms) @ _d(fe_w).t() + _d(fe_b)
    return _ln(_d(a) + _d(r), ga, be, eps)


def gen_lstm_ref(w_ih, b_ih, b_hh, ms=None, fe_w=None, fe_b=None, a=None, r=None, ga=None, be=None, eps=1e-5):
    """-> (X [B, 256], h [B, 256]).  The zero-state step of torch.nn.LSTM (LSTMMixer at T = 1,
    mixer_block.py:237-252; gate order i, f, g, o): G = X w_ih^T + b_ih + b_hh (w_ih [1024, 256]),
    c = s(G_i) tanh(G_g), h = s(G_o) tanh(c): h_0 = c_0 = 0, so W_hh and the forget gate appear nowhere."""
    x = _mixer_x(ms, fe_w, fe_b, a, r, ga, be, eps)
    g = x @ _d(w_ih).t() + _d(b_ih) + _d(b_hh)
    c = torch.sigmoid(g[:, :E]) * torch.tanh(g[:, 2 * E:3 * E])
    return x, torch.sigmoid(g[:, 3 * E:]) * torch.tanh(c)


def gen_gru_ref(w_ih, b_ih, b_hh, ms=None, fe_w=None, fe_b=None, a=None, r=None, ga=None, be=None, eps=1e-5):
    """-> (X [B, 256], h [B, 256]).  The zero-state step of torch.nn.GRU (GRUMixer at T = 1 from h_0 = 0,
    mixer_block.py:193-208; gate order r, z, n): G = X w_ih^T + b_ih (w_ih [768, 256]),
    r_g = s(G_r + b_hr), z_g = s(G_z + b_hz), n_g = tanh(G_n + r_g b_hn), h = (1 - z_g) n_g: h_0 = 0, so
    W_hh appears nowhere."""
    x = _mixer_x(ms, fe_w, fe_b, a, r, ga, be, eps)
    g = x @ _d(w_ih).t() + _d(b_ih)
    bh = _d(b_hh)
    rg = torch.sigmoid(g[:, :E] + bh[:E])
    zg = torch.sigmoid(g[:, E:2 * E] + bh[E:2 * E])
    ng = torch.tanh(g[:, 2 * E:] + rg * bh[2 * E:])
    return x, (1.0 - zg) * ng


def gen_linear_ref(mode, a, r, ga, be, w, bias, a2=None, ga2=None, be2=None, eps=1e-5):
    """-> (xw, out), the three modes of mrg_gen_linear.
    mode 0: xw = LN(a + r) [B, 256], out = xw w^T + bias.
    mode 1 (the two integrators; a2, ga2, be2, w, bias pairs): M = LN(a + r), Y_i = LN(a2[i] + M) with
            ga2[i] / be2[i], xw = [Y_0 | Y_1] [B, 512], out = [Y_0 w[0]^T + bias[0] | Y_1 w[1]^T + bias[1]].
    mode 2 (a, r, ga, be pairs; w [256, 512]): xw = [LN(a[0] + r[0]) | LN(a[1] + r[1])] (the kernel keeps
            no rows in this mode), out = xw w^T + bias."""
    if mode == 0:
        xw = _ln(_d(a) + _d(r), ga, be, eps)
        return xw, xw @ _d(w).t() + _d(bias)
    if mode == 1:
        m = _ln(_d(a) + _d(r), ga, be, eps)
        ys = [_ln(_d(a2[i]) + m, ga2[i], be2[i], eps) for i in range(2)]
        return torch.cat(ys, -1), torch.cat([ys[i] @ _d(w[i]).t() + _d(bias[i]) for i in range(2)], -1)
    xw = torch.cat([_ln(_d(a[i]) + _d(r[i]), ga[i], be[i], eps) for i in range(2)], -1)
    return xw, xw @ _d(w).t() + _d(bias)


def gen_ffn_ref(a, w1, b1, w2, b2, r=None, ga=None, be=None, eps=1e-5, ms_src=None, mask_t=None):
    """FeedForward of X = a (r None) or X = LN(a + r): out = relu(X w1^T + b1) w2^T + b2 [B, N].  With
    ms_src [B, N] and mask_t (the mask's value at the frame) -> (out, ms_next): out is pred[:, t] and
    ms_next = out where mask_t else ms_src (the sampling select, lstmformer.py:487-492)."""
    x = _d(a) if r is None else _ln(_d(a) + _d(r), ga, be, eps)
    out = torch.relu(x @ _d(w1).t() + _d(b1)) @ _d(w2).t() + _d(b2)
    if ms_src is None:
        return out
    return out, (out if mask_t else _d(ms_src))


def gen_attention_ref(q, k, v, heads):
    """One query row per sample over the r keys of a generated frame, no mask
    (MultiModalAttentionBlockSequential at Tq = 1, multi_modal_att.py:22-31).  q [B, 256] (projected, bias
    added), k / v [B, r, 256] (projected), heads -> ctx [B, 256]: per head h of width D = 256 / heads,
    softmax_j(q_h . k_hj / sqrt(D)) over the r keys weighs v_hj; the heads are concatenated (the context
    before out_proj)."""
    B, r, _ = k.shape
    D = E // heads
    qh = _d(q).reshape(B, heads, 1, D)
    kh = _d(k).reshape(B, r, heads, D).transpose(1, 2)
    vh = _d(v).reshape(B, r, heads, D).transpose(1, 2)
    p = torch.softmax(qh @ kh.transpose(-1, -2) / math.sqrt(D), dim=-1)   # [B, heads, 1, r]
    return (p @ vh).reshape(B, E)
