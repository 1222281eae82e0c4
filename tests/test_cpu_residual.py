"""CPU-only checks of the residual connection without a LayerNorm: the three no-LN models construct
with the reference's state_dict layout (tests/golden/residual_noln.npz), every fused schedule declines
them, and mrg_residual_add is declared, bound and exported."""
import ctypes
import os
import re

import pytest

from tests.residual_cases import CASES, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", CASES)
def test_state_dict_matches_reference(case):
    m, d, _ = build(case)   # load_state_dict(strict=True): the same key set
    ref = {k[len("param/"):]: list(d[k].shape) for k in d.files if k.startswith("param/")}
    got = {k: list(v.shape) for k, v in m.state_dict().items()}
    assert list(got) == list(ref)
    assert got == ref
    assert not any("layer_norm" in k for k in got)


def _residual_connections(m):
    from multimodalreactiongeneration_amd.model.layers import ResidualConnection
    return [r for r in m.modules() if isinstance(r, ResidualConnection)]


@pytest.mark.parametrize("case", CASES)
def test_every_residual_connection_is_without_layernorm(case):
    m, _, _ = build(case)
    rcs = _residual_connections(m)
    assert rcs and all(r.layer_norm is None for r in rcs)


def test_lstm_with_sample_takes_the_per_frame_path():
    from multimodalreactiongeneration_amd.model import forms
    m, _, _ = build("sample")
    assert forms.decode_form(m) is None
    assert m._fused_params() is None


def test_metaformer_fused_schedules_decline():
    from multimodalreactiongeneration_amd.generate import GenPlan
    from multimodalreactiongeneration_amd.model import forms
    from multimodalreactiongeneration_amd.model.mixers import MixerBlock
    m, _, _ = build("meta")
    mf = m.metaformer
    blocks = [b for b in mf.modules() if isinstance(b, MixerBlock)]
    kinds = {type(b).__name__ for b in blocks}
    assert {"LSTMMixerBlock", "GRUMixerBlock", "MHAMixerBlock"} <= kinds
    for b in blocks:
        assert forms.residual_lstm(b) is None
        assert forms.residual_gru(b) is None
        assert forms._linear_residual_ln(b.feed_forward) is None
    for blk in mf.metaformer_blocks:
        blk = blk.module   # interlayer_residual: a ResidualConnection around the block
        assert forms.integrator_form(blk.integrator) is None
        assert forms.relu_ffn_form(blk.feedforward, True) is None
        assert forms.embedding_stack_form(blk) is None
    assert mf._fast_eligible() is False
    assert GenPlan(mf, 1).ok is False


def test_simple_lstm_blocks_keep_their_lstm_for_the_paired_launch():
    """paired_lstm_layerd reaches each block's LSTM through the ResidualConnection whatever its norm."""
    from multimodalreactiongeneration_amd.model.layers import LSTM, LSTMLayerd, _block_lstm
    m, _, _ = build("simple")
    stacks = [s for s in m.modules() if isinstance(s, LSTMLayerd)]
    assert stacks
    for s in stacks:
        assert all(isinstance(_block_lstm(b), LSTM) for b in s.lstm_layered)


def test_symbol_declared_bound_and_exported():
    from multimodalreactiongeneration_amd import _lib
    h = open(os.path.join(ROOT, "include", "mrg.h")).read()
    name = "mrg_residual_add"
    assert re.search(r"^int\s+" + name + r"\s*\(long n, const float\* a, const float\* b, float\* y,\s*"
                     r"hipStream_t stream\);", h, re.M)
    res, args = _lib.SIGNATURES[name]
    assert res is ctypes.c_int and len(args) == 5 and args[0] is ctypes.c_long
    assert isinstance(getattr(_lib.load(), name), ctypes._CFuncPtr)


def test_residual_connection_without_num_nodes():
    from torch import nn
    from multimodalreactiongeneration_amd.model.layers import ResidualConnection
    rc = ResidualConnection(nn.Identity(), False)
    assert rc.layer_norm is None and list(rc.state_dict()) == []
    with pytest.raises(ValueError, match="num_nodes"):
        ResidualConnection(nn.Identity(), True)


def test_ops_refuse_a_residual_that_changes_the_width():
    import torch
    from multimodalreactiongeneration_amd import functional as Fn
    x = torch.zeros(2, 8)
    with pytest.raises(ValueError):
        Fn.linear_residual(x, torch.zeros(4, 8), torch.zeros(4))
    with pytest.raises(ValueError):
        Fn.ffn_residual(x, torch.zeros(4, 8), torch.zeros(4), torch.zeros(6, 4), torch.zeros(6), "relu")
    with pytest.raises(ValueError):
        Fn.ffn_residual(x, torch.zeros(4, 8), torch.zeros(4), torch.zeros(8, 4), torch.zeros(8), "gelu")
