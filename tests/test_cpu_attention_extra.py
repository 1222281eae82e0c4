"""nn.MultiheadAttention's add_bias_kv / add_zero_attn on the host side: the module's parameters and
state-dict keys, the lstmformer built with both flags on, the fused schedules declining such a module,
and the float64 restatement of tests/attention_extra_ref.py against
torch.nn.functional.multi_head_attention_forward on every shape, padding pattern and key combination the
GPU tests use."""
import pytest
import torch

from tests import attention_extra_ref as X


def _layers():
    from multimodalreactiongeneration_amd.model import layers
    return layers


def test_add_bias_kv_creates_torch_named_parameters():
    E, h = 32, 4
    m = _layers().MultiheadAttention(E, h, add_bias_kv=True, batch_first=True)
    sd = m.state_dict()
    assert tuple(sd["bias_k"].shape) == (1, 1, E) and tuple(sd["bias_v"].shape) == (1, 1, E)
    assert isinstance(m.bias_k, torch.nn.Parameter) and isinstance(m.bias_v, torch.nn.Parameter)
    assert m.bias_k.abs().max() > 0 and m.bias_v.abs().max() > 0          # xavier_normal_, not zeros
    assert not m.add_zero_attn
    ref = torch.nn.MultiheadAttention(E, h, add_bias_kv=True, batch_first=True)
    assert set(sd) == set(ref.state_dict())
    m.load_state_dict(ref.state_dict(), strict=True)
    for k, v in ref.state_dict().items():
        assert torch.equal(m.state_dict()[k], v), k


def test_add_zero_attn_alone_adds_no_keys():
    E, h = 32, 4
    m = _layers().MultiheadAttention(E, h, add_zero_attn=True, batch_first=True)
    plain = _layers().MultiheadAttention(E, h, batch_first=True)
    assert set(m.state_dict()) == set(plain.state_dict())
    assert m.bias_k is None and m.bias_v is None and m.add_zero_attn and not plain.add_zero_attn
    m.load_state_dict(torch.nn.MultiheadAttention(E, h, add_zero_attn=True, batch_first=True).state_dict(), strict=True)


def test_other_refusals_stay():
    L = _layers()
    with pytest.raises(NotImplementedError):
        L.MultiheadAttention(32, 4, kdim=16)
    with pytest.raises(NotImplementedError):
        L.MultiheadAttention(32, 4, bias=False)


def _metaformer(**flags):
    from multimodalreactiongeneration_amd import configs as C
    from multimodalreactiongeneration_amd.model import Metaformer
    torch.manual_seed(0)
    mc, oc, me = C.lstmformer_config(hidden=32, num_block=2, encoder_num_layer=1, bottleneck=8, num_heads=4,
                                     emb_mixers=("mha", "lstm", "lstm"))
    mc.update(flags)
    return Metaformer(mc, oc, me)


def test_metaformer_with_both_flags_has_the_bias_keys_of_every_attention():
    plain = set(_metaformer().state_dict())
    both = set(_metaformer(add_bias_kv=True, add_zero_attn=True).state_dict())
    stems = [k[:-len("in_proj_weight")] for k in plain if k.endswith("in_proj_weight")]
    assert len(stems) > 2                   # the "mha" embedding mixers and the integrators' cross-attention
    assert both == plain | {s + n for s in stems for n in ("bias_k", "bias_v")}
    assert set(_metaformer(add_zero_attn=True).state_dict()) == plain


def _integrate_blocks(model):
    return [m for m in model.modules() if hasattr(m, "integrators") and hasattr(m, "cat_linear")]


@pytest.mark.parametrize("flags", [dict(add_zero_attn=True), dict(add_bias_kv=True),
                                   dict(add_bias_kv=True, add_zero_attn=True)])
def test_integrator_form_declines_extra_keys(flags):
    from multimodalreactiongeneration_amd.model import forms
    plain = _integrate_blocks(_metaformer())
    assert plain and all(forms.integrator_form(b) is not None for b in plain)
    blocks = _integrate_blocks(_metaformer(**flags))
    assert blocks and all(forms.integrator_form(b) is None for b in blocks)


@pytest.mark.parametrize("combo", list(X.COMBOS))
@pytest.mark.parametrize("Tq,Tk,causal", X.SHAPES)
def test_restatement_equals_torch_in_float64(Tq, Tk, causal, combo):
    """Output and every gradient, on the GPU tests' padding pattern (a row with every real key hidden
    included: finite in both) and without flags."""
    heads, E = 3, 24
    x, w = X.inputs(Tq, Tk, E), dict(X.weights(E, combo))
    zero = X.COMBOS[combo][1]
    for qpad, kpad in (X.pads(Tq, Tk, causal), (None, None)):
        a = X.grads(lambda q, kv, ww: X.mha(q, kv, ww, heads, causal, qpad, kpad, zero), x["q"], x["kv"], w, x["dout"])
        b = X.grads(lambda q, kv, ww: X.torch_mha(q, kv, ww, heads, causal, qpad, kpad, zero), x["q"], x["kv"], w,
                    x["dout"])
        assert torch.isfinite(b[0]).all()
        for got, ref in zip(a[:3], b[:3]):
            assert torch.allclose(got, ref, rtol=1e-11, atol=1e-12)
        for n in w:
            assert torch.allclose(a[3][n], b[3][n], rtol=1e-11, atol=1e-12), n


def test_hidden_row_of_the_restatement_is_the_bias_value_or_zero():
    """Only the bias key seen: the row is bias_v; only the zero key: exactly 0."""
    Tq, Tk, heads, E = 5, 10, 3, 24
    x = X.inputs(Tq, Tk, E)
    vis = torch.zeros(X.B, Tq, Tk, dtype=torch.bool)
    q, k, v = (x[n].double() for n in ("q", "k", "v"))
    bk, bv = torch.randn(E, dtype=torch.float64), torch.randn(E, dtype=torch.float64)
    O, lse = X.core(q, k, v, heads, 0.5, vis, bk, bv, False)
    assert torch.allclose(O, bv.expand_as(O), rtol=0, atol=1e-15) and torch.isfinite(lse).all()
    O, lse = X.core(q, k, v, heads, 0.5, vis, None, None, True)
    assert bool((O == 0).all()) and bool((lse == 0).all())
