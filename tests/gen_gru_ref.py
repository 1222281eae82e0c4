"""Float64 restatement of mrg_gen_gru (csrc/gen.hip): one of the two prologues, then the zero-state step
of torch.nn.GRU (GRUMixer at T = 1 from h_0 = 0, mixer_block.py:193-208; gate order r, z, n)."""
import torch

E = 256


def gen_gru_ref(w_ih, b_ih, b_hh, ms=None, fe_w=None, fe_b=None, a=None, r=None, ga=None, be=None, eps=1e-5):
    """-> (X [B, 256], h [B, 256]) float64.  Prologue: X = ms fe_w^T + fe_b (ms [B, fm]) when ms is given,
    else X = LN(a + r) with ga / be / eps.  Step: G = X w_ih^T + b_ih (w_ih [768, 256]),
    r_g = s(G_r + b_hr), z_g = s(G_z + b_hz), n_g = tanh(G_n + r_g b_hn), h = (1 - z_g) n_g: h_0 = 0, so
    W_hh appears nowhere."""
    d = lambda t: t.double()
    if ms is not None:
        x = d(ms) @ d(fe_w).t() + d(fe_b)
    else:
        s = d(a) + d(r)
        mu = s.mean(-1, keepdim=True)
        var = ((s - mu) ** 2).mean(-1, keepdim=True)
        x = (s - mu) / torch.sqrt(var + eps) * d(ga) + d(be)
    g = x @ d(w_ih).t() + d(b_ih)
    bh = d(b_hh)
    rg = torch.sigmoid(g[:, :E] + bh[:E])
    zg = torch.sigmoid(g[:, E:2 * E] + bh[E:2 * E])
    ng = torch.tanh(g[:, 2 * E:] + rg * bh[2 * E:])
    return x, (1.0 - zg) * ng
