"""The float64 restatements of mrg_gen_lstm, mrg_gen_linear and mrg_gen_ffn (tests/gen_ref.py) are the
torch modules' arithmetic: nn.LSTM at T = 1 from zero state, F.layer_norm + nn.Linear compositions and
Linear-ReLU-Linear.  CPU only, double precision, no kernel runs; the entries' argument checks answer
before any launch, so they are asked here too."""
import copy

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from tests.gen_ref import gen_ffn_ref, gen_linear_ref, gen_lstm_ref

E, HB, B = 256, 64, 5
F64 = torch.float64
ATOL = 1e-12


def _rn(*shape):
    return torch.randn(*shape, dtype=F64)


def _lnp():
    return 1.0 + 0.2 * _rn(E), 0.2 * _rn(E)


def _layer_norm(x, ga, be):
    return F.layer_norm(x, (E,), ga, be, 1e-5)


@pytest.fixture(scope="module")
def lstm_case():
    torch.manual_seed(12)
    lstm = nn.LSTM(E, E, batch_first=True).double()
    ga, be = _lnp()
    return lstm, dict(a=_rn(B, E), r=_rn(B, E), ga=ga, be=be), dict(ms=_rn(B, 6), fe_w=_rn(E, 6), fe_b=_rn(E))


def _through_lstm(lstm, x):
    z = torch.zeros(1, x.shape[0], E, dtype=F64)
    with torch.no_grad():
        y, _ = lstm(x.unsqueeze(1), (z, z))
    return y[:, 0]


def _weights(lstm):
    return lstm.weight_ih_l0.detach(), lstm.bias_ih_l0.detach(), lstm.bias_hh_l0.detach()


@pytest.mark.parametrize("prologue", ["layernorm", "embedding"])
def test_lstm_restatement_is_the_zero_state_step_of_nn_lstm(lstm_case, prologue):
    lstm, ln, emb = lstm_case
    x, h = gen_lstm_ref(*_weights(lstm), **(ln if prologue == "layernorm" else emb))
    if prologue == "layernorm":
        want_x = _layer_norm(ln["a"] + ln["r"], ln["ga"], ln["be"])
    else:
        want_x = emb["ms"] @ emb["fe_w"].t() + emb["fe_b"]
    assert torch.allclose(x, want_x, rtol=0, atol=ATOL)
    assert torch.allclose(h, _through_lstm(lstm, x), rtol=0, atol=ATOL)


def test_lstm_weight_hh_plays_no_part(lstm_case):
    lstm, ln, _ = lstm_case
    l2 = copy.deepcopy(lstm)
    x, h = gen_lstm_ref(*_weights(lstm), **ln)
    before = _through_lstm(l2, x)
    with torch.no_grad():
        l2.weight_hh_l0.copy_(torch.randn_like(l2.weight_hh_l0))
    after = _through_lstm(l2, x)
    assert torch.equal(before, after)
    assert torch.allclose(h, after, rtol=0, atol=ATOL)


def test_linear_restatement_is_layer_norm_then_linear():
    """mode 0: the mixer's LN1 + Linear (mixer_block.py:479-507); mode 1: LN2, then per integrator the
    attention residual's LayerNorm and its Linear (:567-603); mode 2: the integrators' second LayerNorms
    side by side into cat_linear (multi_modal_metaformer.py:128-217)."""
    torch.manual_seed(13)
    a, r = _rn(B, E), _rn(B, E)
    ga, be = _lnp()
    lin = nn.Linear(E, E).double()
    with torch.no_grad():
        xw, out = gen_linear_ref(0, a, r, ga, be, lin.weight, lin.bias)
        want = _layer_norm(a + r, ga, be)
        assert torch.allclose(xw, want, rtol=0, atol=ATOL) and torch.allclose(out, lin(want), rtol=0, atol=ATOL)

        lins = [nn.Linear(E, E).double() for _ in range(2)]
        a2, p2 = [_rn(B, E) for _ in range(2)], [_lnp() for _ in range(2)]
        xw, out = gen_linear_ref(1, a, r, ga, be, [l.weight for l in lins], [l.bias for l in lins], a2,
                                 [p[0] for p in p2], [p[1] for p in p2])
        m = _layer_norm(a + r, ga, be)
        ys = [_layer_norm(a2[i] + m, *p2[i]) for i in range(2)]
        assert xw.shape == out.shape == (B, 2 * E)
        assert torch.allclose(xw, torch.cat(ys, -1), rtol=0, atol=ATOL)
        assert torch.allclose(out, torch.cat([l(y) for l, y in zip(lins, ys)], -1), rtol=0, atol=ATOL)

        cat = nn.Linear(2 * E, E).double()
        aa, rr = [_rn(B, E) for _ in range(2)], [_rn(B, E) for _ in range(2)]
        xw, out = gen_linear_ref(2, aa, rr, [p[0] for p in p2], [p[1] for p in p2], cat.weight, cat.bias)
        want = torch.cat([_layer_norm(aa[i] + rr[i], *p2[i]) for i in range(2)], -1)
        assert torch.allclose(xw, want, rtol=0, atol=ATOL) and torch.allclose(out, cat(want), rtol=0, atol=ATOL)


@pytest.mark.parametrize("N", [E, 6])
@pytest.mark.parametrize("prologue", [False, True])
def test_ffn_restatement_is_linear_relu_linear(N, prologue):
    torch.manual_seed(14 + N)
    ff = nn.Sequential(nn.Linear(E, HB), nn.ReLU(), nn.Linear(HB, N)).double()
    a, r = _rn(B, E), _rn(B, E)
    ga, be = _lnp()
    kw = dict(r=r, ga=ga, be=be) if prologue else {}
    w = (ff[0].weight, ff[0].bias, ff[2].weight, ff[2].bias)
    with torch.no_grad():
        x = _layer_norm(a + r, ga, be) if prologue else a
        want = ff(x)
        assert (ff[0](x) < 0).any() and (ff[0](x) > 0).any()   # both sides of the ReLU
        assert torch.allclose(gen_ffn_ref(a, *w, **kw), want, rtol=0, atol=ATOL)
        src = _rn(B, N)
        for mask_t in (True, False):
            out, nxt = gen_ffn_ref(a, *w, ms_src=src, mask_t=mask_t, **kw)
            assert torch.allclose(out, want, rtol=0, atol=ATOL)
            assert torch.equal(nxt, out if mask_t else src)


def test_entries_refuse_before_any_launch():
    """What the three entries' argument checks refuse returns non-zero without a device; B = 0 returns 0.
    mrg_gen_lstm shares its launcher with mrg_gen_gru since library version 106: null xw / w_ih / b_ih /
    b_hh / h and both prologues at once are refused instead of launched."""
    from multimodalreactiongeneration_amd import _lib
    lib = _lib.load()
    assert lib.mrg_version() >= 106
    one = 1   # a non-null address that a refused call never reads
    arr = (_lib.ctypes.c_void_p * 2)(one, one)

    def lstm(fm, ms, ln, xw=one, w_ih=one, b_ih=one, b_hh=one, h=one, B_=2):
        return lib.mrg_gen_lstm(B_, fm, ms, ms, ms, ln, ln, ln, ln, 1e-5, xw, w_ih, b_ih, b_hh, h, None)
    bad = [lstm(17, one, None), lstm(0, one, None), lstm(6, None, None), lstm(6, one, one)]
    bad += [lstm(6, one, None, **{k: None}) for k in ("xw", "w_ih", "b_ih", "b_hh", "h")]

    def linear(mode, a=arr, a2=arr, w=arr, out=one, B_=2):
        return lib.mrg_gen_linear(mode, B_, a, arr, arr, arr, E, a2, a2, a2, 1e-5, None, E, w, arr, out, E, None)
    bad += [linear(3), linear(-1), linear(0, a=None), linear(0, w=None), linear(2, out=None), linear(1, a2=None)]

    def ffn(N, out=None, pred=None, a=one, r=None, ga=None, src=None, B_=2):
        return lib.mrg_gen_ffn(B_, N, a, r, ga, ga, 1e-5, one, one, one, one, out, pred, 0, src, src, src, 0, None)
    bad += [ffn(E), ffn(6, out=one), ffn(17, pred=one, src=one), ffn(0, pred=one, src=one), ffn(6, pred=one),
            ffn(E, out=one, a=None), ffn(E, out=one, r=one)]
    for i, rc in enumerate(bad):
        assert rc != 0, i
    assert lib.mrg_last_error()
    assert lstm(6, one, None, B_=0) == 0 and linear(0, B_=0) == 0 and ffn(E, out=one, B_=0) == 0
