"""attention.attn_fwd / attn_bwd make every attention kernel call of the package.  Driven here through CPU
tensors against a recording stand-in for the library: for each form product code uses, the entry point, the
argument count of its ctypes signature and the whole argument tuple, written out as the call sites had it
before the helpers existed (pointers as data_ptr() + byte offset)."""
import ctypes

import pytest
import torch

from multimodalreactiongeneration_amd import _lib, attention

B, H, TQ, TK, E = 2, 2, 3, 6, 16      # D = 8; Tq * E = 48, Tk * 2E = 192, 2E = 32; V starts 64 bytes into a KV row
SCALE, STREAM = 0.25, 4242
THR, SK = 123456789, 1.25


class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, tuple(a.value if isinstance(a, ctypes.c_void_p) else a for a in args)))
            return 0
        return call


class _Probe:
    seen = []

    def __init__(self, name, work=0.0):
        _Probe.seen.append((name, work))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


@pytest.fixture()
def lib(monkeypatch):
    rec = _Recorder()
    _Probe.seen = []
    monkeypatch.setattr(_lib, "load", lambda: rec)
    monkeypatch.setattr(attention, "_stream", lambda: STREAM)
    monkeypatch.setattr(attention, "_probe", _Probe)
    return rec


def _tensors():
    f = torch.zeros
    return dict(Q=f(B, TQ, E), KV=f(B, TK, 2 * E), O=f(B, TQ, E), lse=f(B, H, TQ), dO=f(B, TQ, E), dQ=f(B, TQ, E),
                dKV=f(B, TK, 2 * E), ws=f(B * H * TQ), qpad=f(B, TQ, dtype=torch.uint8), kpad=f(B, TK, dtype=torch.uint8),
                key=f(2, dtype=torch.int64))


def _p(t, byte_off=0):
    return t.data_ptr() + byte_off


def _one(lib, name, expected):
    assert len(lib.calls) == 1
    got_name, got = lib.calls[0]
    assert got_name == name
    assert len(got) == len(_lib.SIGNATURES[name][1])
    assert got == expected


def test_plain_forward_and_backward(lib):
    t = _tensors()
    attention.attn_fwd(H, t["Q"], t["KV"], t["O"], t["lse"], t["qpad"], t["kpad"], True, SCALE, drop=None, probe=True)
    head = (2, 2, 3, 6, 8, _p(t["Q"]), 48, 16, _p(t["KV"]), 192, 32, _p(t["KV"], 64), 192, 32, _p(t["O"]), 48, 16,
            _p(t["lse"]), _p(t["qpad"]), _p(t["kpad"]), 1, 0.25)
    _one(lib, "mrg_attention_fwd", head + (4242,))
    lib.calls.clear()
    attention.attn_bwd(H, t["Q"], t["KV"], t["O"], t["lse"], t["qpad"], t["kpad"], True, SCALE, t["dO"], t["dQ"],
                       t["dKV"], t["ws"], drop=None, probe=True)
    _one(lib, "mrg_attention_bwd", head + (_p(t["dO"]), 48, 16, _p(t["dQ"]), 48, 16, _p(t["dKV"]), 192, 32,
                                           _p(t["dKV"], 64), 192, 32, _p(t["ws"]), 4242))
    # causal, Tk = 2 Tq: query i sees 2 (i + 1) keys, 2 + 4 + 6 = 12 pairs per (sample, head)
    assert _Probe.seen == [("attn_fwd", 4.0 * 8 * 2 * 2 * 12), ("attn_bwd", 10.0 * 8 * 2 * 2 * 12)]


def test_dropout_forward_and_backward_are_not_bracketed(lib):
    t = _tensors()
    drop = (THR, SK, t["key"])
    attention.attn_fwd(H, t["Q"], t["KV"], t["O"], t["lse"], None, t["kpad"], False, SCALE, drop=drop, probe=True)
    head = (2, 2, 3, 6, 8, _p(t["Q"]), 48, 16, _p(t["KV"]), 192, 32, _p(t["KV"], 64), 192, 32, _p(t["O"]), 48, 16,
            _p(t["lse"]), None, _p(t["kpad"]), 0, 0.25)
    _one(lib, "mrg_attention_fwd_dropout", head + (123456789, 1.25, _p(t["key"]), 4242))
    lib.calls.clear()
    attention.attn_bwd(H, t["Q"], t["KV"], t["O"], t["lse"], None, t["kpad"], False, SCALE, t["dO"], t["dQ"], t["dKV"],
                       t["ws"], drop=drop, probe=True)
    _one(lib, "mrg_attention_bwd_dropout",
         head + (_p(t["dO"]), 48, 16, _p(t["dQ"]), 48, 16, _p(t["dKV"]), 192, 32, _p(t["dKV"], 64), 192, 32, _p(t["ws"]),
                 123456789, 1.25, _p(t["key"]), 4242))
    assert _Probe.seen == []


def test_extra_key_corrections_v_is_k_forward_and_dkv_only_chunk_backward(lib):
    """The two calls of the bias key's dropout correction: the forward with V = K into its own output and
    statistics, and the accumulating dK / dV pass alone over the whole sequence with a one-row zero dO at
    strides 0 and the c rows as the workspace.  Neither is bracketed."""
    t = _tensors()
    pk, lse_main, cbuf, z = torch.zeros(B, TQ, E), torch.zeros(B, H, TQ), torch.zeros(B, H, TQ), torch.zeros(E)
    attention.attn_fwd(H, t["Q"], t["KV"], pk, lse_main, t["qpad"], t["kpad"], True, SCALE, v=t["KV"],
                       what="attention extra keys: P K")
    _one(lib, "mrg_attention_fwd",
         (2, 2, 3, 6, 8, _p(t["Q"]), 48, 16, _p(t["KV"]), 192, 32, _p(t["KV"]), 192, 32, _p(pk), 48, 16, _p(lse_main),
          _p(t["qpad"]), _p(t["kpad"]), 1, 0.25, 4242))
    lib.calls.clear()
    attention.attn_bwd(H, t["Q"], t["KV"], t["O"], t["lse"], t["qpad"], t["kpad"], True, SCALE, z, t["dQ"], t["dKV"], cbuf,
                       chunk=(0, TQ), passes=2, kv_accumulate=1, what="attention extra keys: dK delta term")
    _one(lib, "mrg_attention_bwd_chunk",
         (2, 2, 3, 6, 8, 0, 3, _p(t["Q"]), 48, 16, _p(t["KV"]), 192, 32, _p(t["KV"], 64), 192, 32, _p(t["O"]), 48, 16,
          _p(t["lse"]), _p(t["qpad"]), _p(t["kpad"]), 1, 0.25, _p(z), 0, 0, _p(t["dQ"]), 48, 16, _p(t["dKV"]), 192, 32,
          _p(t["dKV"], 64), 192, 32, 2, 1, _p(cbuf), 4242))
    assert _Probe.seen == []


def test_integrator_calls_on_slices_of_stacked_buffers(lib):
    """integrate.py hands in integrator i's [N, E] slice of the stacked [n, N, E] buffers (N = B * Tq) and its
    [B, heads, Tq] slice of the stacked statistics; no padding flags here."""
    n, i, N = 2, 1, B * TQ
    Q, O, dO, dQ = (torch.zeros(n, N, E) for _ in range(4))
    lse = torch.zeros(n, B, H, TQ)
    KV, dKV, ws = torch.zeros(B, TK, 2 * E), torch.zeros(B, TK, 2 * E), torch.zeros(B * H * TQ)
    attention.attn_fwd(H, Q[i], KV, O[i], lse[i], None, None, False, SCALE, probe=True, what="attention fwd (integrator)")
    head = (2, 2, 3, 6, 8, _p(Q, 4 * N * E), 48, 16, _p(KV), 192, 32, _p(KV, 64), 192, 32, _p(O, 4 * N * E), 48, 16,
            _p(lse, 4 * B * H * TQ), None, None, 0, 0.25)
    _one(lib, "mrg_attention_fwd", head + (4242,))
    lib.calls.clear()
    attention.attn_bwd(H, Q[i], KV, O[i], lse[i], None, None, False, SCALE, dO[i], dQ[i], dKV, ws, probe=True,
                       what="attention bwd (integrator)")
    _one(lib, "mrg_attention_bwd", head + (_p(dO, 4 * N * E), 48, 16, _p(dQ, 4 * N * E), 48, 16, _p(dKV), 192, 32,
                                           _p(dKV, 64), 192, 32, _p(ws), 4242))
    assert _Probe.seen == [("attn_fwd", 4.0 * 8 * 2 * 2 * 18), ("attn_bwd", 10.0 * 8 * 2 * 2 * 18)]


def test_mha_spec_defaults():
    s = attention.MHASpec(4, True)
    assert (s.heads, s.causal) == (4, True)
    assert (s.eps, s.p, s.addq, s.zero_attn, s.weights) == (None, 0.0, False, False, None)
    assert s._fields == ("heads", "causal", "eps", "p", "addq", "zero_attn", "weights")
