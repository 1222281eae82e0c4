"""need_weights on the host side: mrg_attention_weights declared, bound and exported; the float64
restatement of tests/attention_weights_ref.py against torch.nn.functional.multi_head_attention_forward
asked for its weights (both average switches, the dense mask of the reference rules, the extra keys, a
fully hidden row); the refusals that stay; and the fused schedules declining a model whose attention
records its weights."""
import ctypes
import os

import pytest
import torch

from tests import attention_extra_ref as X
from tests import attention_weights_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _layers():
    from multimodalreactiongeneration_amd.model import layers
    return layers


def test_entry_is_declared_bound_and_exported():
    from multimodalreactiongeneration_amd import _lib
    with open(os.path.join(ROOT, "include", "mrg.h")) as f:
        assert "int mrg_attention_weights(" in f.read()
    res, args = _lib.SIGNATURES["mrg_attention_weights"]
    assert res is ctypes.c_int and len(args) == 24
    lib = ctypes.CDLL(os.path.join(ROOT, "multimodalreactiongeneration_amd", "libmrg.so"))
    assert hasattr(lib, "mrg_attention_weights")


@pytest.mark.parametrize("average", [True, False])
@pytest.mark.parametrize("combo", [None] + list(X.COMBOS))
@pytest.mark.parametrize("Tq,Tk,causal", X.SHAPES)
def test_restatement_equals_torch_in_float64(Tq, Tk, causal, combo, average):
    """Output and weights, with the padding pattern of the extra-key tests (finite everywhere once an extra
    key is there) and without flags."""
    heads, E = 3, 24
    x = X.inputs(Tq, Tk, E)
    w = {n: t.double() for n, t in X.weights(E, combo or "zero").items()}
    zero = bool(combo) and X.COMBOS[combo][1]
    q, kv = x["q"].double(), x["kv"].double()
    for qpad, kpad in (X.pads(Tq, Tk, causal), (None, None)):
        if combo is None and qpad is not None and bool(X.hidden_rows(Tq, Tk, causal).any()):
            continue   # NaN rows: test_fully_hidden_row_is_nan_in_both
        out, wts = W.mha(q, kv, w, heads, causal, qpad, kpad, zero, average=average)
        ro, rw = W.torch_mha(q, kv, w, heads, causal, qpad, kpad, zero, average=average)
        n = Tk + (X.n_extra(combo) if combo else 0)
        assert tuple(wts.shape) == tuple(rw.shape) == ((X.B, Tq, n) if average else (X.B, heads, Tq, n))
        assert torch.isfinite(rw).all()
        assert torch.allclose(out, ro, rtol=1e-11, atol=1e-12)
        assert torch.allclose(wts, rw, rtol=1e-11, atol=1e-13)
        vis = W.visible(Tq, Tk, causal, qpad, kpad, X.B)
        hidden = ~(vis if average else vis.unsqueeze(1).expand(X.B, heads, Tq, Tk))
        assert bool((wts[..., :Tk][hidden] == 0).all())


@pytest.mark.parametrize("average", [True, False])
def test_fully_hidden_row_is_nan_in_both(average):
    """Sample 0's query 2 loses every key to the padding rule: its weights are NaN across the row in torch
    and in the restatement; the other rows agree."""
    Tq, Tk, causal, heads, E = 5, 10, True, 3, 24
    x = X.inputs(Tq, Tk, E)
    w = {n: t.double() for n, t in X.weights(E, "zero").items()}
    qpad, kpad = X.pads(Tq, Tk, causal)
    dead = X.hidden_rows(Tq, Tk, causal)
    assert bool(dead[0, 2]) and int(dead.sum()) == 1
    _, wts = W.mha(x["q"].double(), x["kv"].double(), w, heads, causal, qpad, kpad, average=average)
    _, rw = W.torch_mha(x["q"].double(), x["kv"].double(), w, heads, causal, qpad, kpad, average=average)
    row = (0, 2) if average else (0, slice(None), 2)
    assert torch.isnan(wts[row]).all() and torch.isnan(rw[row]).all()
    live = ~torch.isnan(rw)
    assert bool((live == ~torch.isnan(wts)).all())
    assert torch.allclose(wts[live], rw[live], rtol=1e-11, atol=1e-13)


def test_probs_takes_an_explicit_keep_mask():
    c = W.CASES[3]
    Q, KV = W.projected(c)
    vis = W.visible(c.Tq, c.Tk, c.causal, None, None, W.B)
    keep = torch.rand(W.B, c.heads, c.Tq, c.Tk + 1, generator=torch.Generator().manual_seed(3)) > 0.25
    P, _ = W.probs(Q.double(), KV[..., :c.E].double(), c.heads, 0.5, vis, None, True)
    Pk, _ = W.probs(Q.double(), KV[..., :c.E].double(), c.heads, 0.5, vis, None, True, keep, 0.25)
    assert bool((Pk[~keep] == 0).all())
    assert torch.equal(Pk[keep], (P * W.keep_scale(0.25))[keep])
    Pa, _ = W.probs(Q.double(), KV[..., :c.E].double(), c.heads, 0.5, vis, None, True, keep, 0.25, average=True)
    assert torch.allclose(Pa, Pk.mean(1), rtol=0, atol=1e-15)


def test_refusals():
    L = _layers()
    m = L.MultiheadAttention(32, 4, batch_first=True)
    x = torch.randn(2, 5, 32)
    with pytest.raises(NotImplementedError, match="key_padding_mask"):
        m(x, x, x, key_padding_mask=torch.zeros(2, 5, dtype=torch.bool))
    # need_weights is no refusal any more: a CPU tensor gets as far as the device check
    with pytest.raises(Exception) as e:
        m(x, x, x, need_weights=True)
    assert not isinstance(e.value, NotImplementedError) and "need_weights" not in str(e.value)
    with pytest.raises(Exception) as e0:
        m(x, x, x)
    assert type(e.value) is type(e0.value) and str(e.value) == str(e0.value)
    for bad in ("sum", True, 1, "Mean"):
        with pytest.raises(ValueError):
            m.record_weights = bad
    for ok in ("mean", "heads", None):
        m.record_weights = ok
        assert m.record_weights == ok


def test_switch_and_weights_stay_out_of_the_state_dict():
    m = _layers().MultiheadAttention(32, 4, batch_first=True)
    keys = set(m.state_dict())
    m.record_weights = "heads"
    m.last_weights = torch.zeros(1, 4, 2, 2)
    assert set(m.state_dict()) == keys == set(torch.nn.MultiheadAttention(32, 4, batch_first=True).state_dict())
    assert m.last_weights is not None and not list(m.buffers())


def test_sequential_wrapper_keeps_need_weights_off():
    seen = {}
    L = _layers()
    wrap = L.MHAforSequentail(32, 4, batch_first=True)
    wrap.mha.forward = lambda *a: seen.setdefault("args", a) and (a[0], None)
    x = torch.randn(2, 5, 32)
    wrap((x, x, x, None, True, None, True, False))
    assert seen["args"][4] is False and seen["args"][6] is False


def _metaformer():
    from multimodalreactiongeneration_amd import configs as C
    from multimodalreactiongeneration_amd.model import Metaformer
    torch.manual_seed(0)
    mc, oc, me = C.lstmformer_config(hidden=32, num_block=2, encoder_num_layer=1, bottleneck=8, num_heads=4)
    return Metaformer(mc, oc, me)


def test_integrator_form_declines_a_recording_attention_until_cleared():
    from multimodalreactiongeneration_amd.model import forms
    model = _metaformer()
    blocks = [m for m in model.modules() if hasattr(m, "integrators") and hasattr(m, "cat_linear")]
    atts = [m for m in model.modules() if isinstance(m, _layers().MultiheadAttention)]
    assert blocks and atts and all(forms.integrator_form(b) is not None for b in blocks)
    atts[-1].record_weights = "mean"
    assert forms.integrator_form(blocks[-1]) is None
    assert all(forms.integrator_form(b) is not None for b in blocks[:-1])
    atts[-1].record_weights = None
    assert all(forms.integrator_form(b) is not None for b in blocks)


def test_generation_plan_declines_a_recording_attention_until_cleared(monkeypatch):
    """plan_for re-reads the switch on every call: a cached plan is not handed out while an attention
    records, and is again once the switch is cleared."""
    from multimodalreactiongeneration_amd import generate
    model = _metaformer()

    class Plan:
        ok = True
    monkeypatch.setattr(generate, "GenPlan", lambda mf, ratio: Plan())
    monkeypatch.setattr(generate, "_PLANS", {})
    first = generate.plan_for(model)
    assert isinstance(first, Plan)
    att = next(m for m in model.modules() if isinstance(m, _layers().MultiheadAttention))
    att.record_weights = "heads"
    assert generate.plan_for(model) is None
    att.record_weights = None
    assert generate.plan_for(model) is first
