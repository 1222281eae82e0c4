"""CPU-only checks of the dropout RNG's host restatement (multimodalreactiongeneration_amd/rng.py, the
specification the kernels are tested against) and of the new C-ABI symbols."""
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20240607   # the keep-rate and distinct-mask checks below are deterministic for this seed

NEW_SYMBOLS = ("mrg_rng_draw", "mrg_dropout", "mrg_dropout_keep_mask", "mrg_attention_keep_mask",
               "mrg_attention_fwd_dropout", "mrg_attention_bwd_dropout")


@pytest.mark.parametrize("counter,key,expect", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     "d16cfe09 94fdcceb 5001e420 24126ea1")])
def test_philox4x32_10_known_answers(counter, key, expect):
    from multimodalreactiongeneration_amd.rng import philox4x32_10
    out = philox4x32_10(counter, key)
    assert " ".join(f"{int(w):08x}" for w in out) == expect


def test_philox_is_elementwise_over_arrays():
    from multimodalreactiongeneration_amd.rng import philox4x32_10
    c0 = np.array([0, 0x243F6A88], dtype=np.uint32)
    a = philox4x32_10((c0, 7, 9, 11), (3, 5))
    for i in range(2):
        b = philox4x32_10((int(c0[i]), 7, 9, 11), (3, 5))
        assert [int(w[i]) for w in a] == [int(w) for w in b]


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_rate_and_draws(p):
    from multimodalreactiongeneration_amd.rng import keep_mask
    n = 1 << 20
    m0 = keep_mask(SEED, 0, n, p)
    assert m0.dtype == np.bool_ and m0.shape == (n,)
    rate = float(m0.mean())
    print(f"p={p} keep rate {rate:.6f} bound {5 * math.sqrt(p * (1 - p) / n):.6f}")
    assert abs(rate - (1 - p)) <= 5 * math.sqrt(p * (1 - p) / n)
    assert np.array_equal(m0, keep_mask(SEED, 0, n, p))          # same (seed, draw): same mask
    m1 = keep_mask(SEED, 1, n, p)
    assert not np.array_equal(m0, m1)                            # another draw: another mask
    assert not np.array_equal(m0, keep_mask(SEED + 1, 0, n, p))  # another seed
    # a draw past 2^32 changes the key's high word, not only the counter
    assert not np.array_equal(keep_mask(SEED, 5, 4096, p), keep_mask(SEED, 5 + (1 << 32), 4096, p))
    # a prefix of a longer mask is the shorter mask (the flat index alone addresses an element)
    assert np.array_equal(m0[:4099], keep_mask(SEED, 0, 4099, p))


def test_attention_keep_mask_shape_and_rate():
    from multimodalreactiongeneration_amd.rng import attention_keep_mask
    B, H, Tq, Tk, p = 2, 3, 70, 75, 0.25
    m = attention_keep_mask(SEED, 3, B, H, Tq, Tk, p)
    assert m.shape == (B, H, Tq, Tk) and m.dtype == np.bool_
    n = m.size
    assert abs(float(m.mean()) - (1 - p)) <= 5 * math.sqrt(p * (1 - p) / n)
    # rows, heads and samples are independent streams
    assert not np.array_equal(m[0, 0, 0], m[0, 0, 1]) and not np.array_equal(m[0, 0], m[0, 1])
    assert not np.array_equal(m[0], m[1])
    # a narrower key range is a prefix: the map depends on (b, head, q, k), not on Tk
    assert np.array_equal(m[..., :33], attention_keep_mask(SEED, 3, B, H, Tq, 33, p))


def test_threshold_edge_cases():
    from multimodalreactiongeneration_amd.rng import attention_keep_mask, keep_mask, threshold
    assert threshold(0.0) == 0 and threshold(0.5) == 1 << 31 and threshold(0.25) == 1 << 30
    assert threshold(1.0 - 2.0 ** -33) == (1 << 32) - 1        # floor, never 2^32
    assert keep_mask(SEED, 0, 1000, 0.0).all()                  # p = 0 keeps everything
    assert attention_keep_mask(SEED, 0, 1, 2, 5, 7, 0.0).all()
    for bad in (1.0, 1.5, -0.1, float("nan")):
        with pytest.raises(ValueError):
            threshold(bad)
        with pytest.raises(ValueError):
            keep_mask(SEED, 0, 8, bad)
        with pytest.raises(ValueError):
            attention_keep_mask(SEED, 0, 1, 1, 2, 2, bad)


def test_functional_rejects_bad_probability_before_any_launch():
    import torch
    from multimodalreactiongeneration_amd import functional as Fn
    x = torch.zeros(4)
    for bad in (1.0, -0.5):
        with pytest.raises(ValueError):
            Fn.dropout(x, bad)
    w = torch.zeros(12, 4)
    with pytest.raises(ValueError):
        Fn.mha(torch.zeros(1, 2, 4), torch.zeros(1, 2, 4), w, torch.zeros(12), torch.zeros(4, 4), torch.zeros(4), 2,
               dropout_p=1.0)


def test_new_symbols_declared_exported_and_bound():
    from multimodalreactiongeneration_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mrg.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mrg_[a-z0-9_]+)\s*\(", src))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert lib.mrg_version() >= 101


def test_dropout_no_longer_refused_where_the_headline_model_uses_it():
    """layers.MultiheadAttention / LSTM / GRU accept train() with dropout > 0 up to the device check (the
    refusal was a NotImplementedError); ResidualConnection(dropout > 0) stays refused."""
    import torch
    from multimodalreactiongeneration_amd.model import layers as L
    x = torch.zeros(2, 3, 8)
    for m, args in ((L.MultiheadAttention(8, 2, dropout=0.1, batch_first=True), (x, x, x)),
                    (L.LSTM(8, 8, num_layers=2, dropout=0.1), (x,)),
                    (L.GRU(8, 8, num_layers=2, dropout=0.1), (x,))):
        m.train()
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m(*args)
    with pytest.raises(NotImplementedError):
        L.ResidualConnection(torch.nn.Identity(), True, 8, dropout=0.1)
