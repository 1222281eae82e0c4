"""The attention kernels (csrc/attention.hip) called through the C ABI, one by one, against the float64
core of tests/attention_ref.py: every head width D in {8, 16, 32, 64} (both lane-to-d maps, the guards of
the partial d tile at D = 8, the half-idle tile loader), the forward output and log-sum-exp, dQ, dK and dV,
both backward forms at D = 64, the scalar row paths of unaligned q / o / dq / dk / dv, leading and scattered
padding flags, large logits, the memory around the written rows, the query-chunk forms and determinism.

Error measure: max |a - ref| / max |ref| per (sample, head) slice, bound TOL = 1e-4 (the fp32 bar of
tests/test_gpu_ops.py).  The one place the measure is undefined, the exactly zero dQ and dK of the single
(query, key) pair, is measured against attention_ref.zero_scales instead.  Every comparison prints its
figure with the error plain fp32 torch ops make on the same inputs beside it (run with -s to see them)."""
from collections import namedtuple

import pytest
import torch

from tests import attention_ref as R

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = "cuda:0"
FILL = 7.0        # what the output rows hold before a call (the sentinel sits between and beyond them)
B, H = R.B, R.HEADS
OUTS = ("O", "lse", "dQ", "dK", "dV")

# how the rows handed to the kernels lie in memory.  q_extra / o_extra: floats between the rows of q /
# of every output (o, dq, dk, dv); lead: floats in front of those buffers; kv "inter": K and V are the
# halves of one [B, Tk, 2E] buffer, "k_inter": K is, V is a [B, Tk, E] buffer of its own (two different
# aligned strides); inter_out: dK and dV are the halves of one buffer
Layout = namedtuple("Layout", "q_extra o_extra lead kv inter_out")
PACKED = Layout(0, 0, 0, "inter", True)      # the [B, T, E] / [B, T, 2E] projections the modules pass
WIDE = Layout(0, 4, 4, "inter", True)        # 16-B rows with gaps: the vector paths next to guard zones
ODD = Layout(1, 1, 3, "k_inter", False)      # odd row strides: qvec = ovec = dkvvec = 0


@pytest.fixture(scope="module")
def lib():
    from multimodalreactiongeneration_amd import _lib as L
    lib = L.load()
    yield lib
    torch.cuda.synchronize()


def _ptr(t):
    from multimodalreactiongeneration_amd.functional import _ptr as p
    return p(t)


def _stream():
    from multimodalreactiongeneration_amd.functional import _stream as s
    return s()


def _rows(t):
    """pointer, batch stride, row stride of a [B, T, E] view"""
    assert t.dim() == 3 and t.stride(2) == 1
    return _ptr(t), t.stride(0), t.stride(1)


def _rows_out(shape, extra, lead):
    """a guarded output: (buffer, [B, T, E] view holding FILL)"""
    return R.strided(torch.full(shape, FILL, dtype=torch.float32, device=DEV), shape[2] + extra, lead)


def _flat_out(n):
    """a guarded flat output of n floats (lse, the workspace): 8 sentinels in front, 2 n behind"""
    buf, view = R.strided(torch.full((1, 1, n), FILL, dtype=torch.float32, device=DEV), n, 8)
    return buf, view.view(n)


def _device_inputs(name, D, lay):
    x = R.inputs(name, D)
    E = H * D
    d = {n: x[n].to(DEV) for n in ("q", "dout")}
    d["qf"] = d["q"] if lay.q_extra == 0 else R.strided(d["q"], E + lay.q_extra, lay.lead)[1]
    kv = torch.cat([x["k"], x["v"]], -1).to(DEV)
    d["k"], d["v"] = kv[:, :, :E], (kv[:, :, E:] if lay.kv == "inter" else x["v"].to(DEV))
    d["qpad"], d["kpad"] = (None if x[n] is None else x[n].to(DEV) for n in ("qpad", "kpad"))
    d["scale"] = x["scale"]
    return d


def _fwd(lib, c, D, d, q, k, v, o, lse):
    return lib.mrg_attention_fwd(B, H, c.Tq, c.Tk, D, *_rows(q), *_rows(k), *_rows(v), *_rows(o), _ptr(lse),
                                 _ptr(d["qpad"]), _ptr(d["kpad"]), int(c.causal), d["scale"], _stream())


def _bwd(lib, c, D, d, q, k, v, o, lse, dout, dq, dk, dv, ws):
    return lib.mrg_attention_bwd(B, H, c.Tq, c.Tk, D, *_rows(q), *_rows(k), *_rows(v), *_rows(o), _ptr(lse),
                                 _ptr(d["qpad"]), _ptr(d["kpad"]), int(c.causal), d["scale"], *_rows(dout),
                                 *_rows(dq), *_rows(dk), *_rows(dv), _ptr(ws), _stream())


def _run(lib, name, D, lay, fused=None, bwd=True):
    """Forward (q in the layout's rows) and backward (q, k, v, dout 16-B rows as the ABI requires; o, dq,
    dk, dv in the layout's rows) of a case; fused: mrg_attention_set_fused for the backward (None: as it
    is, the default 1).  Every output sits in a guarded buffer and the guards are checked here."""
    c = R.BY_NAME[name]
    E = H * D
    d = _device_inputs(name, D, lay)
    guards = []

    def out(shape):
        buf, view = _rows_out(shape, lay.o_extra, lay.lead)
        guards.append((buf, view))
        return view

    def flat(n):
        buf, view = _flat_out(n)
        guards.append((buf, view))
        return view
    r = {"O": out((B, c.Tq, E)), "lse": flat(B * H * c.Tq).view(B, H, c.Tq)}
    assert _fwd(lib, c, D, d, d["qf"], d["k"], d["v"], r["O"], r["lse"]) == 0
    if bwd:
        r["dQ"] = out((B, c.Tq, E))
        if lay.inter_out:
            dkv = out((B, c.Tk, 2 * E))
            r["dK"], r["dV"] = dkv[:, :, :E], dkv[:, :, E:]
        else:
            r["dK"], r["dV"] = out((B, c.Tk, E)), out((B, c.Tk, E))
        r["ws"] = flat(B * H * c.Tq)
        prev = lib.mrg_attention_set_fused(fused) if fused is not None else None
        try:
            assert _bwd(lib, c, D, d, d["q"], d["k"], d["v"], r["O"], r["lse"], d["dout"], r["dQ"], r["dK"], r["dV"],
                        r["ws"]) == 0
        finally:
            if prev is not None:
                lib.mrg_attention_set_fused(prev)
    torch.cuda.synchronize()
    for buf, view in guards:
        assert R.outside_intact(buf, view), f"{name} D={D}: a store outside the rows"
    return r


def _errors(test, name, D, got, outs=OUTS, note=""):
    """{output: [B, H] slice errors against float64}, printed with the fp32 composite's beside them"""
    errs, yard = R.errors(got, name, D, outs), R.yardstick(name, D, len(outs) > 2)
    for n in outs:
        print(f"ATTN {test} {name} D={D}{note} {n} err={errs[n].max().item():.3e} fp32={yard[n].max().item():.3e}")
    return errs


def _assert_close(test, name, D, got, outs=OUTS, note=""):
    errs = _errors(test, name, D, got, outs, note)
    bad = {n: e.max().item() for n, e in errs.items() if not e.max().item() < TOL}
    assert not bad, f"{name} D={D}{note}: {bad}"


# ---------------------------------------------------------------- a. every width against float64
@pytest.mark.parametrize("name,D", R.case_params(lambda c: c.qscale == 1.0 and "fully_masked" not in c.tags))
def test_every_width_matches_float64(lib, name, D):
    """O, lse, dQ, dK, dV of every shape x padding pattern at every head width; at D = 64 the backward
    both as the single pass and as the dQ and dK / dV passes."""
    for fused in ((1, 0) if D == 64 else (None,)):
        got = _run(lib, name, D, PACKED, fused)
        _assert_close("a", name, D, got, note="" if fused is None else f" fused={fused}")


# ---------------------------------------------------------------- b. large logits
@pytest.mark.parametrize("name,D", R.case_params(lambda c: "large_logits" in c.tags))
def test_large_logits(lib, name, D):
    """Scores of standard deviation about 8: a near one-hot softmax whose running maximum moves between the
    32-key updates.  Bound per slice: TOL, or, where the fast exp / log intrinsics do not reach it, 4 x the
    error of the fp32 composite on the same inputs (intrinsics and summation order)."""
    yard = R.yardstick(name, D)
    for fused in ((1, 0) if D == 64 else (None,)):
        note = "" if fused is None else f" fused={fused}"
        errs = _errors("b", name, D, _run(lib, name, D, PACKED, fused), note=note)
        bad = {}
        for n in OUTS:
            fallback = errs[n] >= TOL
            print(f"ATTN b {name} D={D}{note} {n} bound={'4 x fp32' if bool(fallback.any()) else 'TOL'}")
            if bool((fallback & ~(errs[n] <= 4 * yard[n])).any()):
                bad[n] = (errs[n].max().item(), yard[n].max().item())
        assert not bad, f"{name} D={D}{note}: (error, fp32 composite) {bad}"


# ---------------------------------------------------------------- c. scalar row paths
@pytest.mark.parametrize("D", R.WIDTHS)
@pytest.mark.parametrize("name", ["65x129n-tail", "66x33c-none"])
def test_unaligned_rows_take_the_scalar_paths(lib, name, D):
    """Odd row strides of q and o (forward) and of o, dq, dk, dv (backward: the single pass declines):
    float64 parity, bitwise the aligned two-pass call (only loads and stores differ), guards intact
    (checked in _run), and the documented refusals of unaligned K and dO.  Every width: the scalar loads
    index through dmap, whose two branches are D >= 32 and D < 32."""
    got = _run(lib, name, D, ODD)
    _assert_close("c", name, D, got)
    base = _run(lib, name, D, PACKED, fused=0)
    for n in OUTS + ("ws",):   # ws: delta, which only the two-pass form writes
        assert torch.equal(got[n], base[n]), n
    assert not bool((got["ws"] == FILL).any())

    c, E = R.BY_NAME[name], H * D
    d = _device_inputs(name, D, PACKED)
    odd = lambda t: R.strided(t, E + 1, 0)[1]
    o, lse = torch.full((B, c.Tq, E), FILL, device=DEV), torch.full((B, H, c.Tq), FILL, device=DEV)
    assert _fwd(lib, c, D, d, d["q"], odd(d["k"]), d["v"], o, lse) != 0
    assert b"16-B" in lib.mrg_last_error()
    dq, dk, dv = (torch.full((B, T, E), FILL, device=DEV) for T in (c.Tq, c.Tk, c.Tk))
    ws = torch.full((B * H * c.Tq,), FILL, device=DEV)
    assert _bwd(lib, c, D, d, d["q"], d["k"], d["v"], base["O"], base["lse"], odd(d["dout"]), dq, dk, dv, ws) != 0
    assert b"16-B" in lib.mrg_last_error()
    torch.cuda.synchronize()
    assert all(bool((t == FILL).all()) for t in (o, lse, dq, dk, dv, ws))


# ---------------------------------------------------------------- d. guard zones on the aligned paths
@pytest.mark.parametrize("D", [8, 16])
@pytest.mark.parametrize("name", ["17x33n-none", "65x65c-tail"])
def test_narrow_heads_write_only_their_rows(lib, name, D):
    """D = 8 (a partial 16-wide d tile) and D = 16 with four spare floats after every output row: nothing
    outside [:, :T, :E] changes (checked in _run), and the rows are right."""
    _assert_close("d", name, D, _run(lib, name, D, WIDE))


# ---------------------------------------------------------------- e. fully masked row at a tile edge
@pytest.mark.parametrize("D", [8, 64])
def test_fully_masked_row_65_is_nan_and_alone(lib, D):
    """Query 64 (the first of the second workgroup) sees no key: its O and lse are NaN for every head, and
    every other row is untouched by that.  Forward only: such a row has no defined gradients."""
    name = "65x65c-row64"
    got = _run(lib, name, D, PACKED, bwd=False)
    assert bool(torch.isnan(got["O"][:, 64]).all()) and bool(torch.isnan(got["lse"][:, :, 64]).all())
    assert bool(torch.isfinite(got["O"][:, :64]).all()) and bool(torch.isfinite(got["lse"][:, :, :64]).all())
    _assert_close("e", name, D, got, outs=("O", "lse"))   # the reference's non-finite row is left out


# ---------------------------------------------------------------- f. chunk forms
@pytest.mark.parametrize("D", [16, 32])
@pytest.mark.parametrize("name,cuts", [("66x33c-tail", (0, 17, 66)), ("33x132c-tail", (0, 5, 33)),
                                       ("65x129n-tail", (0, 64, 65))])
def test_query_chunks_below_64_and_inside_a_ratio_group(lib, name, cuts, D):
    """mrg_attention_{fwd,bwd}_chunk at D < 64 with a cut inside a ratio group (Tq = 2 Tk cut at 17), next
    to a ratio group (Tk = 4 Tq) and one query from the end: O, lse, dQ bitwise the whole call; dK / dV
    bitwise from one pass-2 call after the chunks' pass-1 calls, within 1e-5 when accumulated chunk by
    chunk (fp32 reordering); everything against float64."""
    c, E = R.BY_NAME[name], H * D
    whole = _run(lib, name, D, PACKED, fused=0)
    d = _device_inputs(name, D, PACKED)
    f = dict(device=DEV, dtype=torch.float32)
    oc, lc = torch.full((B, c.Tq, E), FILL, **f), torch.full((B, H, c.Tq), FILL, **f)
    dqc, dqs = torch.full((B, c.Tq, E), FILL, **f), torch.full((B, c.Tq, E), FILL, **f)
    dkc, dvc = torch.zeros(B, c.Tk, E, **f), torch.zeros(B, c.Tk, E, **f)
    dks, dvs = torch.full((B, c.Tk, E), FILL, **f), torch.full((B, c.Tk, E), FILL, **f)
    wsc, wss = torch.full((B * H * c.Tq,), FILL, **f), torch.full((B * H * c.Tq,), FILL, **f)
    pads = (_ptr(d["qpad"]), _ptr(d["kpad"]), int(c.causal), d["scale"])

    def chunk_bwd(q0, n, dqx, dkx, dvx, passes, acc, wsx):
        return lib.mrg_attention_bwd_chunk(
            B, H, n, c.Tk, D, q0, c.Tq, *_rows(d["q"][:, q0:]), *_rows(d["k"]), *_rows(d["v"]), *_rows(oc[:, q0:]),
            _ptr(lc), *pads, *_rows(d["dout"][:, q0:]), *_rows(dqx[:, q0:]), *_rows(dkx), *_rows(dvx), passes, acc,
            _ptr(wsx), _stream())
    for q0, q1 in zip(cuts[:-1], cuts[1:]):
        n = q1 - q0
        assert lib.mrg_attention_fwd_chunk(B, H, n, c.Tk, D, q0, c.Tq, *_rows(d["q"][:, q0:]), *_rows(d["k"]),
                                           *_rows(d["v"]), *_rows(oc[:, q0:]), _ptr(lc), *pads, _stream()) == 0
        assert chunk_bwd(q0, n, dqc, dkc, dvc, 3, 1, wsc) == 0
        assert chunk_bwd(q0, n, dqs, dks, dvs, 1, 0, wss) == 0
    assert chunk_bwd(0, c.Tq, dqs, dks, dvs, 2, 0, wss) == 0
    torch.cuda.synchronize()
    assert torch.equal(lc, whole["lse"]) and torch.equal(oc, whole["O"])
    assert torch.equal(dqc, whole["dQ"]) and torch.equal(dqs, whole["dQ"])
    assert torch.equal(dks, whole["dK"]) and torch.equal(dvs, whole["dV"])
    assert R.slice_err(dkc, whole["dK"]) < 1e-5 and R.slice_err(dvc, whole["dV"]) < 1e-5
    _assert_close("f", name, D, dict(O=oc, lse=lc, dQ=dqc, dK=dkc, dV=dvc), note=f" cuts={cuts} accumulated")
    _assert_close("f", name, D, whole, note=" whole")


# ---------------------------------------------------------------- g. determinism
@pytest.mark.parametrize("D", R.WIDTHS)
def test_two_runs_are_bitwise_equal(lib, D):
    """"Deterministic (no atomics)": the same forward and backward twice leave the same bits (at D = 64 the
    single-pass backward, and the two-pass form too)."""
    name = "130x130c-scattered"
    for fused in ((1, 0) if D == 64 else (None,)):
        a, b = _run(lib, name, D, PACKED, fused), _run(lib, name, D, PACKED, fused)
        for n in OUTS:
            assert torch.equal(a[n], b[n]), (n, fused)
