"""CPU-only checks of the ratio > 1 generation plan's new entry point: mrg_gen_attention is declared,
exported and bound, refuses bad arguments before any launch, and its float64 restatement
(tests/gen_ref.py) is torch.nn.MultiheadAttention's context at one query over r keys."""
import os
import re

import pytest
import torch

from tests.gen_ref import gen_attention_ref
from tests.golden_util import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gen_attention_is_declared_exported_and_bound():
    from multimodalreactiongeneration_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mrg.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+mrg_gen_attention\s*\(([^;]*)\)\s*;", src)
    assert m, "include/mrg.h does not declare mrg_gen_attention"
    assert "mrg_gen_attention" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["mrg_gen_attention"][1]) == len(m.group(1).split(",")) == 8
    assert hasattr(_lib.load(), "mrg_gen_attention")


def test_gen_attention_refuses_before_any_launch():
    """The argument checks come before the launch, so they answer without a device: r outside 1..16,
    heads outside {4, 8, 16}, B < 0 and a null buffer return non-zero; B = 0 returns 0."""
    from multimodalreactiongeneration_amd import _lib
    lib = _lib.load()
    one = 1   # a non-null address that a refused call never reads
    for B, r, heads, q in ((2, 0, 4, one), (2, 17, 4, one), (2, 8, 2, one), (2, 8, 3, one), (-1, 8, 4, one),
                           (2, 8, 4, None)):
        assert lib.mrg_gen_attention(B, r, heads, q, one, one, one, None) != 0, (B, r, heads, q)
        assert lib.mrg_last_error()
    assert lib.mrg_gen_attention(0, 8, 4, one, one, one, one, None) == 0


@pytest.mark.parametrize("r", [1, 8])
def test_gen_attention_ref_is_multihead_attention(r):
    """The restatement against torch.nn.MultiheadAttention in double (embed_dim 256, 4 heads, batch_first,
    one query, r keys): the module's own projected q / k / v go through gen_attention_ref, and
    out_proj of that context is the module's output."""
    heads, B, E = 4, 5, 256
    torch.manual_seed(r)
    mha = torch.nn.MultiheadAttention(E, heads, batch_first=True).double()
    with torch.no_grad():
        mha.in_proj_bias.normal_(std=0.1)
        mha.out_proj.bias.normal_(std=0.1)
    x, kv = torch.randn(B, 1, E).double(), torch.randn(B, r, E).double()
    w, b = mha.in_proj_weight, mha.in_proj_bias
    with torch.no_grad():
        q = x[:, 0] @ w[:E].T + b[:E]
        k = kv @ w[E:2 * E].T + b[E:2 * E]
        v = kv @ w[2 * E:].T + b[2 * E:]
        ctx = gen_attention_ref(q, k, v, heads)
        assert ctx.shape == (B, E) and ctx.dtype == torch.float64
        want, _ = mha(x, kv, kv, need_weights=False)
        assert rel_err(mha.out_proj(ctx), want[:, 0]) < 1e-12
        if r == 1:
            assert torch.equal(ctx, v[:, 0])   # one key: weight exactly 1
