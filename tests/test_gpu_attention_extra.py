"""nn.MultiheadAttention's add_bias_kv / add_zero_attn keys on the device: the merge kernels of
csrc/attention_extra.hip through the C ABI after the attention kernels, and Fn.mha / the MHAMixer residual
forms end to end, against float64 (torch.nn.functional.multi_head_attention_forward on the dense mask; with
dropout the restatement of tests/attention_extra_ref.py on the exported keep mask of width Tk + n_extra).

Bounds: TOL = 1e-4, the bar tests/test_gpu_attention.py puts on O, lse, dQ, dK and dV (per (sample, head)
slice at the C ABI) and tests/test_gpu_ops.py on dgamma / dbeta (rel_err), which dbias_k / dbias_v, sums over
the B * Tq rows like those, are held to as well.  Every comparison prints its figure (run with -s)."""
import pytest
import torch

from tests import attention_extra_ref as X
from tests import attention_ref as R
from tests.golden_util import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = "cuda:0"
FILL = 7.0
B, H = X.B, R.HEADS
SEED = 20250311


@pytest.fixture(scope="module")
def lib():
    from multimodalreactiongeneration_amd import _lib as L
    lib = L.load()
    yield lib
    from multimodalreactiongeneration_amd import functional as Fn
    torch.cuda.synchronize()
    Fn.check_errors()


def _ptr(t, off=0):
    from multimodalreactiongeneration_amd.functional import _ptr as p
    return p(t, off)


def _stream():
    from multimodalreactiongeneration_amd.functional import _stream as s
    return s()


def _rows(t):
    assert t.dim() == 3 and t.stride(2) == 1
    return _ptr(t), t.stride(0), t.stride(1)


def _param(t):
    return torch.nn.Parameter(t.clone().to(DEV))


def _key(seed, draw):
    from multimodalreactiongeneration_amd.functional import _i64
    return torch.tensor([_i64(seed), _i64(draw)], dtype=torch.int64, device=DEV)


# ---------------------------------------------------------------- the C ABI
class _Guards(list):
    def rows(self, shape, extra, lead):
        buf, view = R.strided(torch.full(shape, FILL, dtype=torch.float32, device=DEV), shape[2] + extra, lead)
        self.append((buf, view))
        return view

    def flat(self, n, lead=8):
        buf, view = R.strided(torch.full((1, 1, n), FILL, dtype=torch.float32, device=DEV), n, lead)
        self.append((buf, view))
        return view.view(n)

    def check(self, what):
        for buf, view in self:
            assert R.outside_intact(buf, view), f"{what}: a store outside the rows"


def _bias(E, combo, odd):
    """bias_k / bias_v [E] float32 on the CPU and on the device (odd: 4 bytes off a 16-B boundary)"""
    if not X.COMBOS[combo][0]:
        return None, None, None, None
    w = X.weights(E, "bias", seed=5)
    bk, bv = w["bias_k"].reshape(E), w["bias_v"].reshape(E)
    dev = torch.zeros(2 * E + 8, device=DEV)
    o = 1 if odd else 0
    dk_, dv_ = dev[o:o + E], dev[E + 4 + o:2 * E + 4 + o]
    dk_.copy_(bk)
    dv_.copy_(bv)
    return bk, bv, dk_, dv_


def _abi(lib, Tq, Tk, causal, D, combo, heads=H, odd=False, accumulate=None):
    """mrg_attention_fwd, the merge, mrg_attention_bwd, the extras' backward; every output guarded.  odd: o / dq
    rows of stride E + 1 and the biases off alignment (the scalar kernels); else packed rows (float4)."""
    E = heads * D
    x = X.inputs(Tq, Tk, E)
    q, k, v, dout = (x[n].to(DEV) for n in ("q", "k", "v", "dout"))
    qpad, kpad = (t.to(DEV) for t in X.pads(Tq, Tk, causal))
    bk, bv, dbk_, dbv_ = _bias(E, combo, odd)
    zero = int(X.COMBOS[combo][1])
    scale = float(D) ** -0.5
    G = _Guards()
    extra, lead = (1, 3) if odd else (0, 0)
    r = {"O": G.rows((B, Tq, E), extra, lead), "lse": G.flat(B * heads * Tq).view(B, heads, Tq)}
    main = (B, heads, Tq, Tk, D, *_rows(q), *_rows(k), *_rows(v), *_rows(r["O"]), _ptr(r["lse"]), _ptr(qpad), _ptr(kpad),
            int(causal), scale)
    assert lib.mrg_attention_fwd(*main, _stream()) == 0
    assert lib.mrg_attention_extra_fwd(B, heads, Tq, D, *_rows(q), _ptr(dbk_), _ptr(dbv_), zero, scale, *_rows(r["O"]),
                                       _ptr(r["lse"]), Tk, 0, 1.0, None, _stream()) == 0, lib.mrg_last_error()
    r["dQ"] = G.rows((B, Tq, E), extra, lead)
    dkv = G.rows((B, Tk, 2 * E), 0, 0)
    r["dK"], r["dV"] = dkv[:, :, :E], dkv[:, :, E:]
    ws = G.flat(B * heads * Tq)
    assert lib.mrg_attention_bwd(*main, *_rows(dout), *_rows(r["dQ"]), *_rows(r["dK"]), *_rows(r["dV"]), _ptr(ws),
                                 _stream()) == 0
    if bk is not None:
        n = lib.mrg_attention_extra_bwd_workspace_bytes(B, heads, Tq, D) // 4
        assert n > 0
        xws = G.flat(n)
        r["dbk"], r["dbv"] = G.flat(E, 8 + (1 if odd else 0)), G.flat(E, 8 + (1 if odd else 0))
        if accumulate is not None:
            r["dbk"].copy_(accumulate[0])
            r["dbv"].copy_(accumulate[1])
        assert lib.mrg_attention_extra_bwd(B, heads, Tq, D, *_rows(q), _ptr(dbk_), _ptr(dbv_), scale, *_rows(r["O"]),
                                           _ptr(r["lse"]), *_rows(dout), *_rows(r["dQ"]), _ptr(r["dbk"]), _ptr(r["dbv"]),
                                           int(accumulate is not None), Tk, 0, 1.0, None, None, 0, 0, None, None,
                                           _ptr(xws), _stream()) == 0, lib.mrg_last_error()
    torch.cuda.synchronize()
    G.check(f"{Tq}x{Tk} D={D} {combo}")
    return r


def _abi_ref(Tq, Tk, causal, D, combo, heads=H):
    E = heads * D
    x = X.inputs(Tq, Tk, E)
    bk, bv, _, _ = _bias(E, combo, False)
    ts = {n: x[n].double().requires_grad_(True) for n in ("q", "k", "v")}
    if bk is not None:
        ts["bk"], ts["bv"] = bk.double().requires_grad_(True), bv.double().requires_grad_(True)
    vis = X.visible(Tq, Tk, causal, *X.pads(Tq, Tk, causal), B)
    O, lse = X.core(ts["q"], ts["k"], ts["v"], heads, float(D) ** -0.5, vis, ts.get("bk"), ts.get("bv"),
                    X.COMBOS[combo][1])
    O.backward(x["dout"].double())
    ref = {"O": O.detach(), "lse": lse.detach(), "dQ": ts["q"].grad, "dK": ts["k"].grad, "dV": ts["v"].grad}
    if bk is not None:
        ref["dbk"], ref["dbv"] = ts["bk"].grad, ts["bv"].grad
    return ref


def _abi_close(got, ref, heads, note):
    errs = {n: R.slice_err(got[n], ref[n], heads) for n in ("O", "dQ", "dK", "dV")}
    errs["lse"] = rel_err(got["lse"], ref["lse"])
    errs.update({n: rel_err(got[n], ref[n]) for n in ("dbk", "dbv") if n in ref})
    print(f"EXTRA {note} " + " ".join(f"{n}={e:.2e}" for n, e in errs.items()))
    assert all(bool(torch.isfinite(got[n]).all()) for n in ref), note
    bad = {n: e for n, e in errs.items() if not e < TOL}
    assert not bad, f"{note}: {bad}"


@pytest.mark.parametrize("combo", list(X.COMBOS))
@pytest.mark.parametrize("D", R.WIDTHS)
@pytest.mark.parametrize("Tq,Tk,causal", X.SHAPES)
def test_merge_matches_float64_at_every_width(lib, Tq, Tk, causal, D, combo):
    """Both memory forms; the rows whose real keys are all hidden are finite and exact: bias_v when only the
    bias key is seen, 0 with only the zero key, and nothing of them leaks into the other rows' gradients."""
    ref = _abi_ref(Tq, Tk, causal, D, combo)
    hid = X.hidden_rows(Tq, Tk, causal)
    assert hid.any() and not hid.all()
    for odd in (False, True):
        got = _abi(lib, Tq, Tk, causal, D, combo, odd=odd)
        _abi_close(got, ref, H, f"{Tq}x{Tk} D={D} {combo} odd={odd}")
        rows = got["O"].cpu()[hid]
        if combo == "zero":
            assert bool((rows == 0).all())
        elif combo == "bias":
            assert torch.equal(rows, _bias(H * D, combo, False)[1].expand_as(rows))


def test_rows_wider_than_one_wave_step(lib):
    """E = 320: 80 float4 units, a second, partly idle 64-unit step (and five scalar steps)."""
    ref = _abi_ref(70, 70, False, 64, "both", heads=5)
    for odd in (False, True):
        _abi_close(_abi(lib, 70, 70, False, 64, "both", heads=5, odd=odd), ref, 5, f"E=320 odd={odd}")


def test_more_rows_than_the_backward_has_waves(lib):
    """3 x 352 rows: the backward's 256 blocks of four waves take a second row each."""
    ref = _abi_ref(352, 16, False, 8, "both")
    _abi_close(_abi(lib, 352, 16, False, 8, "both"), ref, H, "352x16")


def test_two_runs_are_bitwise_equal_and_accumulate_adds(lib):
    a, b = (_abi(lib, 70, 70, False, 16, "both") for _ in range(2))
    for n in a:
        assert torch.equal(a[n], b[n]), n
    E = H * 16
    pre = torch.randn(2, E, generator=torch.Generator().manual_seed(4)).to(DEV)
    c = _abi(lib, 70, 70, False, 16, "both", accumulate=pre)
    assert torch.equal(c["dbk"], pre[0] + a["dbk"]) and torch.equal(c["dbv"], pre[1] + a["dbv"])
    assert torch.equal(c["dQ"], a["dQ"])


def test_refusals_leave_the_outputs_untouched(lib):
    Tq, Tk, D = 5, 10, 16
    E = H * D
    q = torch.randn(B, Tq, E, device=DEV)
    bias = torch.randn(E, device=DEV)
    o, dq = (torch.full((B, Tq, E), FILL, device=DEV) for _ in range(2))
    lse = torch.full((B, H, Tq), FILL, device=DEV)
    dbk, dbv, ws = (torch.full((4096,), FILL, device=DEV) for _ in range(3))

    def fwd(D_=D, bk=bias, bv=bias, zero=1, o_=o, lse_=lse, q_=q):
        return lib.mrg_attention_extra_fwd(B, H, Tq, D_, _ptr(q_), Tq * E, E, _ptr(bk), _ptr(bv), zero, 0.25, _ptr(o_),
                                           Tq * E, E, _ptr(lse_), Tk, 0, 1.0, None, _stream())

    def bwd(D_=D, bk=bias, bv=bias, dq_=dq, dbk_=dbk, ws_=ws, pk=None):
        return lib.mrg_attention_extra_bwd(B, H, Tq, D_, _ptr(q), Tq * E, E, _ptr(bk), _ptr(bv), 0.25, _ptr(o), Tq * E, E,
                                           _ptr(lse), _ptr(q), Tq * E, E, _ptr(dq_), Tq * E, E, _ptr(dbk_), _ptr(dbv), 0,
                                           Tk, 0, 1.0, None, _ptr(pk), Tq * E, E, None, None, _ptr(ws_), _stream())
    for call, word in ((lambda: fwd(D_=12), b"head dim"), (lambda: fwd(bv=None), b"together"),
                       (lambda: fwd(bk=None, bv=None, zero=0), b"neither"), (lambda: fwd(o_=None), b"required"),
                       (lambda: fwd(lse_=None), b"required"), (lambda: fwd(q_=None), b"required"),
                       (lambda: bwd(D_=24), b"head dim"), (lambda: bwd(bk=None), b"bias_k and bias_v required"),
                       (lambda: bwd(dq_=None), b"null buffer"), (lambda: bwd(dbk_=None), b"null buffer"),
                       (lambda: bwd(ws_=None), b"workspace"), (lambda: bwd(pk=q), b"together")):
        assert call() != 0
        assert word in lib.mrg_last_error(), lib.mrg_last_error()
    torch.cuda.synchronize()
    assert all(bool((t == FILL).all()) for t in (o, dq, lse, dbk, dbv, ws))


# ---------------------------------------------------------------- Fn.mha
def _mha_dev(Tq, Tk, causal, D, combo, p, fn="mha", ln=None):
    """Fn.<fn> forward + backward on the device.  Returns (out, dq, dkv, {name: grad}), the op's key."""
    from multimodalreactiongeneration_amd import functional as Fn
    E = H * D
    x, w = X.inputs(Tq, Tk, E), X.weights(E, combo)
    ps = {n: _param(t) for n, t in w.items()}
    qd, kvd = x["q"].to(DEV).requires_grad_(True), x["kv"].to(DEV).requires_grad_(True)
    qpad, kpad = (t.to(DEV) for t in X.pads(Tq, Tk, causal))
    seed, draw = Fn.get_rng_state(DEV)
    kw = dict(causal=causal, qpad=qpad, kpad=kpad, dropout_p=p, bias_k=ps.get("bias_k"), bias_v=ps.get("bias_v"),
              add_zero_attn=X.COMBOS[combo][1])
    args = (qd, kvd, ps["in_w"], ps["in_b"], ps["out_w"], ps["out_b"], H)
    if fn == "mha_residual_layernorm":
        lnp = [_param(t) for t in ln]
        out = Fn.mha_residual_layernorm(*args, *lnp, 1e-5, **kw)
    else:
        out = getattr(Fn, fn)(*args, **kw)
    out.backward(x["dout"].to(DEV))
    torch.cuda.synchronize()
    assert Fn.get_rng_state(DEV) == (seed, draw + (1 if p else 0))
    return (out.detach(), qd.grad, kvd.grad, {n: t.grad for n, t in ps.items()}), _key(seed, draw)


def _mha_close(got, ref, note):
    errs = {"out": rel_err(got[0], ref[0]), "dq": rel_err(got[1], ref[1]), "dkv": rel_err(got[2], ref[2])}
    errs.update({n: rel_err(got[3][n], ref[3][n]) for n in ref[3]})
    print(f"EXTRA mha {note} " + " ".join(f"{n}={e:.2e}" for n, e in errs.items()))
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in got[3].values()), note
    bad = {n: e for n, e in errs.items() if not e < TOL}
    assert not bad, f"{note}: {bad}"


@pytest.mark.parametrize("combo", list(X.COMBOS))
@pytest.mark.parametrize("D", R.WIDTHS)
@pytest.mark.parametrize("Tq,Tk,causal", X.SHAPES)
def test_mha_matches_torch_float64(lib, Tq, Tk, causal, D, combo):
    """Output, dq, dkv, d in_proj, d out_proj, dbias_k, dbias_v against multi_head_attention_forward itself."""
    x, w = X.inputs(Tq, Tk, H * D), dict(X.weights(H * D, combo))
    qpad, kpad = X.pads(Tq, Tk, causal)
    ref = X.grads(lambda q, kv, ww: X.torch_mha(q, kv, ww, H, causal, qpad, kpad, X.COMBOS[combo][1]),
                  x["q"], x["kv"], w, x["dout"])
    got, _ = _mha_dev(Tq, Tk, causal, D, combo, 0.0)
    _mha_close(got, ref, f"{Tq}x{Tk} D={D} {combo}")


@pytest.mark.parametrize("combo", list(X.COMBOS))
@pytest.mark.parametrize("D", R.WIDTHS)
@pytest.mark.parametrize("Tq,Tk,causal", X.SHAPES)
def test_mha_dropout_matches_the_restatement_on_the_exported_mask(lib, Tq, Tk, causal, D, combo):
    """p = 0.25; the mask has Tk + n_extra columns, the bias key's at Tk.  Two runs with one key are bitwise
    equal."""
    from multimodalreactiongeneration_amd import functional as Fn
    p = 0.25
    x, w = X.inputs(Tq, Tk, H * D), dict(X.weights(H * D, combo))
    qpad, kpad = X.pads(Tq, Tk, causal)
    Fn.manual_seed(SEED + Tq + D, DEV)
    got, key = _mha_dev(Tq, Tk, causal, D, combo, p)
    keep = Fn.attention_keep_mask(key, B, H, Tq, Tk + X.n_extra(combo), p).cpu().bool()
    ref = X.grads(lambda q, kv, ww: X.mha(q, kv, ww, H, causal, qpad, kpad, X.COMBOS[combo][1], keep, p),
                  x["q"], x["kv"], w, x["dout"])
    _mha_close(got, ref, f"{Tq}x{Tk} D={D} {combo} p={p}")
    Fn.manual_seed(SEED + Tq + D, DEV)
    again, key2 = _mha_dev(Tq, Tk, causal, D, combo, p)
    assert torch.equal(key, key2)
    for a, b in zip(got[:3], again[:3]):
        assert torch.equal(a, b)
    for n in got[3]:
        assert torch.equal(got[3][n], again[3][n]), n


def test_graph_replay_takes_a_fresh_draw(lib):
    from multimodalreactiongeneration_amd import functional as Fn
    from multimodalreactiongeneration_amd import graphs
    Tq, Tk, D, p = 10, 5, 16, 0.25
    E = H * D
    x, w = X.inputs(Tq, Tk, E), X.weights(E, "both")
    ps = {n: _param(t) for n, t in w.items()}
    q, kv = x["q"].to(DEV).requires_grad_(True), x["kv"].to(DEV).requires_grad_(True)
    do = x["dout"].to(DEV)
    out = {"o": torch.zeros(B, Tq, E, device=DEV), "gq": torch.zeros(B, Tq, E, device=DEV),
           "gkv": torch.zeros(B, Tk, E, device=DEV), "key": torch.zeros(2, dtype=torch.int64, device=DEV)}

    def step():
        out["key"].copy_(Fn._rng_state(DEV))
        o = Fn.mha(q, kv, ps["in_w"], ps["in_b"], ps["out_w"], ps["out_b"], H, True, None, None, dropout_p=p,
                   bias_k=ps["bias_k"], bias_v=ps["bias_v"], add_zero_attn=True)
        gq, gkv = torch.autograd.grad(o, (q, kv), do)
        out["o"].copy_(o.detach())
        out["gq"].copy_(gq)
        out["gkv"].copy_(gkv)

    Fn.manual_seed(SEED, DEV)
    replay = graphs.capture(step)
    keys, outs = [], []
    for _ in range(3):
        replay()
        torch.cuda.synchronize()
        keep = Fn.attention_keep_mask(out["key"], B, H, Tq, Tk + 2, p).cpu().bool()
        qr, kvr = (t.detach().double().cpu().requires_grad_(True) for t in (q, kv))
        orf = X.mha(qr, kvr, {n: t.double() for n, t in w.items()}, H, True, None, None, True, keep, p)
        gqr, gkvr = torch.autograd.grad(orf, (qr, kvr), do.double().cpu())
        assert rel_err(out["o"], orf) < TOL and rel_err(out["gq"], gqr) < TOL and rel_err(out["gkv"], gkvr) < TOL
        keys.append(out["key"].clone())
        outs.append(out["o"].clone())
    assert keys[1][1] > keys[0][1] and keys[2][1] > keys[1][1]
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2])


def test_flags_off_reach_no_new_entry_point(lib, monkeypatch):
    """Without extra keys every form of Fn.mha issues what it issued before: the new entry points are not
    called and the results are bitwise those of a call that never mentions the arguments.  With a key they
    are called (the probe sees them), the one-key shape included."""
    from multimodalreactiongeneration_amd import functional as Fn
    calls = []
    for name in ("mrg_attention_extra_fwd", "mrg_attention_extra_bwd", "mrg_attention_extra_bwd_workspace_bytes"):
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _r=real, _n=name: (calls.append(_n), _r(*a))[1])
    for Tq, Tk, causal, p in ((1, 1, False, 0.0), (5, 10, True, 0.0), (5, 10, True, 0.25)):
        E = H * 16
        x, w = X.inputs(Tq, Tk, E), X.weights(E, "zero")
        res = []
        for kw in ({}, dict(bias_k=None, bias_v=None, add_zero_attn=False)):
            ps = {n: _param(t) for n, t in w.items()}
            qd, kvd = x["q"].to(DEV).requires_grad_(True), x["kv"].to(DEV).requires_grad_(True)
            Fn.manual_seed(SEED, DEV)
            o = Fn.mha(qd, kvd, ps["in_w"], ps["in_b"], ps["out_w"], ps["out_b"], H, causal, dropout_p=p, **kw)
            o.backward(x["dout"].to(DEV))
            res.append([o.detach(), qd.grad, kvd.grad] + [t.grad for t in ps.values()])
        torch.cuda.synchronize()
        assert calls == []
        # (the one-key form hands the query no gradient: None in both)
        assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(*res))
    got, _ = _mha_dev(1, 1, False, 16, "both", 0.0)
    assert "mrg_attention_extra_fwd" in calls and "mrg_attention_extra_bwd" in calls


@pytest.mark.parametrize("use_ln", [True, False])
@pytest.mark.parametrize("combo", list(X.COMBOS))
def test_mixer_in_a_residual_connection_matches_module_by_module(lib, combo, use_ln):
    """ResidualConnection(MHAMixer) takes the fused residual forms; float64: LN(mha + q) / mha + q with
    torch's attention, module by module."""
    from multimodalreactiongeneration_amd.model.layers import ResidualConnection
    from multimodalreactiongeneration_amd.model.masks import BlockCausalMask
    from multimodalreactiongeneration_amd.model.mixers import MHAMixer
    Tq, Tk, D = 5, 10, 16
    E = H * D
    bias, zero = X.COMBOS[combo]
    torch.manual_seed(3)
    res = ResidualConnection(MHAMixer(E, H, batch_first=True, add_bias_kv=bias, add_zero_attn=zero), use_ln, E).to(DEV)
    mha = res.module.mixer[0].mha
    with torch.no_grad():
        mha.in_proj_bias.normal_(0, 0.1)
        mha.out_proj.bias.normal_(0, 0.1)
        if use_ln:
            res.layer_norm.weight.normal_(1, 0.1)
            res.layer_norm.bias.normal_(0, 0.1)
    x = X.inputs(Tq, Tk, E)
    qpad, kpad = X.pads(Tq, Tk, True)
    qd, kvd = x["q"].to(DEV).requires_grad_(True), x["kv"].to(DEV).requires_grad_(True)
    out = res(qd, kvd, kvd, BlockCausalMask(qpad.to(DEV), kpad.to(DEV), H))
    out.backward(x["dout"].to(DEV))
    torch.cuda.synchronize()
    names = {"in_w": mha.in_proj_weight, "in_b": mha.in_proj_bias, "out_w": mha.out_proj.weight, "out_b": mha.out_proj.bias}
    if bias:
        names.update(bias_k=mha.bias_k, bias_v=mha.bias_v)
    if use_ln:
        names.update(gamma=res.layer_norm.weight, beta=res.layer_norm.bias)

    def ref_fn(q, kv, ww):
        y = X.torch_mha(q, kv, ww, H, True, qpad, kpad, zero) + q
        return torch.nn.functional.layer_norm(y, (E,), ww["gamma"], ww["beta"], res.layer_norm.eps) if use_ln else y
    ref = X.grads(ref_fn, x["q"], x["kv"], {n: t.detach().cpu() for n, t in names.items()}, x["dout"])
    _mha_close((out.detach(), qd.grad, kvd.grad, {n: t.grad for n, t in names.items()}), ref, f"mixer {combo} ln={use_ln}")


def test_a_model_with_both_flags_trains_a_step_and_generates(lib):
    from multimodalreactiongeneration_amd import configs as C
    from multimodalreactiongeneration_amd.model import Metaformer
    from multimodalreactiongeneration_amd.synthetic import clone_batch, make_batch
    torch.manual_seed(0)
    mc, oc, me = C.lstmformer_config(hidden=64, num_block=2, encoder_num_layer=1, bottleneck=16, lr=1e-3,
                                     emb_mixers=("mha", "lstm", "lstm"))
    mc.update(add_bias_kv=True, add_zero_attn=True)
    model = Metaformer(mc, oc, me).to(DEV)
    batch = clone_batch(make_batch(B=2, T=12, lead=3, seed=7), DEV)
    opt = model.configure_optimizers()["optimizer"]
    loss = model.training_step(batch)["loss"]
    loss.backward()
    biases = [(n, p) for n, p in model.named_parameters() if n.endswith(("bias_k", "bias_v"))]
    assert biases and all(p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0
                          for _, p in biases)
    before = [p.detach().clone() for _, p in biases]
    opt.step()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss)) and all(not torch.equal(b, p) for b, (_, p) in zip(before, biases))
    model.eval()
    with torch.no_grad():
        gen = model.validation_step(batch)
    torch.cuda.synchronize()
    vals = [v for v in (gen.values() if isinstance(gen, dict) else [gen]) if isinstance(v, torch.Tensor)]
    assert all(bool(torch.isfinite(v).all()) for v in vals)
