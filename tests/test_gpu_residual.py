"""Residual connections without a LayerNorm on the MI355X path: mrg_residual_add through the C ABI
(bitwise against numpy), the functional ops against the float64 restatements of tests/residual_ref.py
(bar: rel_err <= 1e-4, tests.golden_util), the three no-LN models against the reference's golden
(tests/golden/residual_noln.npz), graph replay, and the LayerNorm paths left as they were."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import residual_ref as R
from tests.golden_util import batch_from, rel_err
from tests.residual_cases import build

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = "cuda:0"
GUARD = 4   # sentinel floats on either side of y (16 bytes: the aligned case stays aligned)


@pytest.fixture(scope="module", autouse=True)
def _done():
    from multimodalreactiongeneration_amd import _lib as L
    L.load()
    yield
    from multimodalreactiongeneration_amd import functional as Fn
    torch.cuda.synchronize()
    Fn.check_errors()


def _p(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + 4 * off)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _param(t):
    return torch.nn.Parameter(t.clone().to(DEV))


def _within(errs):
    print({k: f"{e:.2e}" for k, e in errs.items()})
    for k, e in errs.items():
        assert e <= TOL, (k, e)


# ------------------------------------------------------------------ 1. the kernel through the C ABI
@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 1023, 1025, 4099])
def test_residual_add_bitwise(n, off, inplace):
    """off = 1 moves a, b and y one float past a 16-byte boundary (the scalar form); inplace: y is a."""
    from multimodalreactiongeneration_amd import _lib as L
    rs = np.random.RandomState(n + off)
    a, b = rs.standard_normal(n).astype(np.float32), rs.standard_normal(n).astype(np.float32)
    sent = np.float32(-777.0)
    hold = np.full(n + 2 * GUARD + off, sent, dtype=np.float32)
    if inplace:
        hold[GUARD + off:GUARD + off + n] = a
    y = torch.from_numpy(hold).to(DEV)
    bd = torch.from_numpy(np.concatenate([np.zeros(off, np.float32), b])).to(DEV)
    ad = torch.from_numpy(np.concatenate([np.zeros(off, np.float32), a])).to(DEV)
    assert y.data_ptr() % 16 == 0 and ad.data_ptr() % 16 == 0 and bd.data_ptr() % 16 == 0
    pa = _p(y, GUARD + off) if inplace else _p(ad, off)
    assert L.load().mrg_residual_add(n, pa, _p(bd, off), _p(y, GUARD + off), _stream()) == 0
    torch.cuda.synchronize()
    got = y.cpu().numpy()
    assert np.array_equal(got[GUARD + off:GUARD + off + n], a + b)
    assert (got[:GUARD + off] == sent).all() and (got[GUARD + off + n:] == sent).all(), "a sentinel was overwritten"


def test_residual_add_empty_and_refused():
    from multimodalreactiongeneration_amd import _lib as L
    lib = L.load()
    a = torch.ones(8, device=DEV)
    y = torch.full((8,), 5.0, device=DEV)
    assert lib.mrg_residual_add(0, _p(a), _p(a), _p(y), _stream()) == 0
    assert lib.mrg_residual_add(0, None, None, None, _stream()) == 0
    torch.cuda.synchronize()
    assert (y == 5.0).all()
    for args in ((8, None, _p(a), _p(y)), (8, _p(a), None, _p(y)), (8, _p(a), _p(a), None), (-1, _p(a), _p(a), _p(y))):
        assert lib.mrg_residual_add(*args, _stream()) != 0
    torch.cuda.synchronize()
    assert (y == 5.0).all()


def test_residual_add_function():
    """y + x with the gradient handed to both operands as it is; in place only outside autograd."""
    from multimodalreactiongeneration_amd import functional as Fn
    g = torch.Generator().manual_seed(3)
    y, x, do = (torch.randn(3, 5, 7, generator=g) for _ in range(3))
    yd, xd = y.to(DEV).requires_grad_(True), x.to(DEV).requires_grad_(True)
    out = Fn.residual_add(yd, xd, inplace=True)
    assert out.data_ptr() != yd.data_ptr()
    out.backward(do.to(DEV))
    assert torch.equal(out.detach().cpu(), y + x)
    assert torch.equal(yd.grad.cpu(), do) and torch.equal(xd.grad.cpu(), do)
    with torch.no_grad():
        buf = y.to(DEV)
        out = Fn.residual_add(buf, x.to(DEV), inplace=True)
        assert out.data_ptr() == buf.data_ptr() and torch.equal(out.cpu(), y + x)
    with pytest.raises(ValueError):
        Fn.residual_add(yd, xd[:, :4])


# ------------------------------------------------------------------ 2. Linear and FFN under the residual
ROWS_E = [(rows, E) for rows in (1, 5, 70, 257) for E in (8, 64, 256)]


def _grads(out, do, tensors):
    out.backward(do)
    return [t.grad for t in tensors]


@pytest.mark.parametrize("rows,E", ROWS_E)
def test_linear_residual_vs_float64(rows, E):
    from multimodalreactiongeneration_amd import functional as Fn
    g = torch.Generator().manual_seed(rows * 7 + E)
    x, do = torch.randn(rows, E, generator=g), torch.randn(rows, E, generator=g)
    w, b = torch.randn(E, E, generator=g) / math.sqrt(E), torch.randn(E, generator=g) * 0.1
    ref_t = [t.double().requires_grad_(True) for t in (x, w, b)]
    ref_o = R.linear_residual(*ref_t)
    ref_g = _grads(ref_o, do.double(), ref_t)
    names = ("dx", "dW", "db")

    def run(fused):
        xd, wd, bd = x.to(DEV).requires_grad_(True), _param(w), _param(b)
        o = Fn.linear_residual(xd, wd, bd) if fused else Fn.residual_add(Fn.linear(xd, wd, bd), xd)
        return o.detach(), _grads(o, do.to(DEV), (xd, wd, bd))
    (o, gs), (o2, gs2) = run(True), run(False)
    errs = {"out": rel_err(o, ref_o), **{n: rel_err(a, r) for n, a, r in zip(names, gs, ref_g)}}
    errs.update({"unfused out": rel_err(o2, ref_o), **{f"unfused {n}": rel_err(a, r) for n, a, r in zip(names, gs2, ref_g)}})
    errs.update({"fused vs unfused out": rel_err(o, o2),
                 **{f"fused vs unfused {n}": rel_err(a, r) for n, a, r in zip(names, gs, gs2)}})
    _within(errs)
    # the epilogue forms v = alpha acc + bias, then v + aux (gemm_common.h, alpha = 1):
    # the value the unfused GEMM stores, then the add residual_add makes, in the same order
    assert torch.equal(o, o2)


@pytest.mark.parametrize("act", ["relu", "tanh", "silu"])
@pytest.mark.parametrize("rows,E", ROWS_E)
def test_ffn_residual_vs_float64(rows, E, act):
    """Bottleneck E / 4 (at least 8).  relu: the float64 reference's own kinks are used; a pre-activation
    within float32 rounding of zero could flip one, which random data at these sizes does not produce."""
    from multimodalreactiongeneration_amd import functional as Fn
    Hb = max(8, E // 4)
    g = torch.Generator().manual_seed(rows * 11 + E)
    x, do = torch.randn(rows, E, generator=g), torch.randn(rows, E, generator=g)
    ps = (torch.randn(Hb, E, generator=g) / math.sqrt(E), torch.randn(Hb, generator=g) * 0.1,
          torch.randn(E, Hb, generator=g) / math.sqrt(Hb), torch.randn(E, generator=g) * 0.1)
    ref_t = [t.double().requires_grad_(True) for t in (x, *ps)]
    ref_o = R.ffn_residual(*ref_t, act)
    ref_g = _grads(ref_o, do.double(), ref_t)
    names = ("dx", "dW1", "db1", "dW2", "db2")

    def run(fused):
        xd, pd = x.to(DEV).requires_grad_(True), [_param(t) for t in ps]
        o = Fn.ffn_residual(xd, *pd, act) if fused else Fn.residual_add(Fn.ffn(xd, *pd, act), xd)
        return o.detach(), _grads(o, do.to(DEV), (xd, *pd))
    (o, gs), (o2, gs2) = run(True), run(False)
    errs = {"out": rel_err(o, ref_o), **{n: rel_err(a, r) for n, a, r in zip(names, gs, ref_g)}}
    errs.update({"fused vs unfused out": rel_err(o, o2),
                 **{f"fused vs unfused {n}": rel_err(a, r) for n, a, r in zip(names, gs, gs2)}})
    _within(errs)
    # the epilogue forms v = alpha acc + bias, then v + aux (gemm_common.h, alpha = 1):
    # the value the unfused GEMM stores, then the add residual_add makes, in the same order
    assert torch.equal(o, o2)


def test_linear_add_vs_float64():
    """linear(h) + r with r another tensor (LSTMModule's mixing Linear, the attention block's projection)."""
    from multimodalreactiongeneration_amd import functional as Fn
    g = torch.Generator().manual_seed(5)
    h, r, do = torch.randn(3, 23, 24, generator=g), torch.randn(3, 23, 40, generator=g), torch.randn(3, 23, 40, generator=g)
    w, b = torch.randn(40, 24, generator=g) / 5, torch.randn(40, generator=g) * 0.1
    ref_t = [t.double().requires_grad_(True) for t in (h, w, b, r)]
    ref_o = ref_t[0] @ ref_t[1].T + ref_t[2] + ref_t[3]
    ref_g = _grads(ref_o, do.double(), ref_t)
    dev_t = [h.to(DEV).requires_grad_(True), _param(w), _param(b), r.to(DEV).requires_grad_(True)]
    o = Fn.linear_add(*dev_t)
    gs = _grads(o, do.to(DEV), dev_t)
    _within({"out": rel_err(o, ref_o), **{n: rel_err(a, r_) for n, a, r_ in zip(("dh", "dW", "db", "dr"), gs, ref_g)}})


# ------------------------------------------------------------------ 3. attention under the residual
def _mha_weights(E, g):
    return {"in_w": torch.randn(3 * E, E, generator=g) / math.sqrt(E), "in_b": torch.randn(3 * E, generator=g) * 0.1,
            "out_w": torch.randn(E, E, generator=g) / math.sqrt(E), "out_b": torch.randn(E, generator=g) * 0.1}


def _mha_case(Tq, Tk, E, heads, causal, ragged, p):
    from multimodalreactiongeneration_amd import functional as Fn
    B = 2
    g = torch.Generator().manual_seed(Tq * 5 + Tk + E)
    q, kv = torch.randn(B, Tq, E, generator=g), torch.randn(B, Tk, E, generator=g)
    qpad = kpad = None
    if ragged:
        q[1, Tq * 2 // 3:] = -100.0
        kv[1, Tk // 2:] = -100.0
    if causal:
        qpad, kpad = Fn.padding_flags(q.to(DEV)), Fn.padding_flags(kv.to(DEV))
    w = _mha_weights(E, g)
    do = torch.randn(B, Tq, E, generator=g)
    ps = {k: _param(v) for k, v in w.items()}
    qd, kvd = q.to(DEV).requires_grad_(True), kv.to(DEV).requires_grad_(True)
    keep = None
    if p:
        Fn.manual_seed(20240607 + Tq, DEV)
        seed, draw = Fn.get_rng_state(DEV)
    o = Fn.mha_residual(qd, kvd, ps["in_w"], ps["in_b"], ps["out_w"], ps["out_b"], heads, causal, qpad, kpad,
                        dropout_p=p)
    o.backward(do.to(DEV))
    if p:
        assert Fn.get_rng_state(DEV) == (seed, draw + 1)
        key = torch.tensor([Fn._i64(seed), Fn._i64(draw)], dtype=torch.int64, device=DEV)
        keep = Fn.attention_keep_mask(key, B, heads, Tq, Tk, p).cpu().bool()
        assert keep.any() and not keep.all()
    rs = {k: v.double().requires_grad_(True) for k, v in w.items()}
    qr, kvr = q.double().requires_grad_(True), kv.double().requires_grad_(True)
    orf = R.mha_residual(qr, kvr, rs["in_w"], rs["in_b"], rs["out_w"], rs["out_b"], heads, causal,
                         None if qpad is None else qpad.cpu(), None if kpad is None else kpad.cpu(), keep, p)
    orf.backward(do.double())
    assert not torch.isnan(orf).any()
    errs = {"out": rel_err(o, orf), "dq": rel_err(qd.grad, qr.grad), "dkv": rel_err(kvd.grad, kvr.grad)}
    errs.update({k: rel_err(ps[k].grad, rs[k].grad) for k in w})
    _within(errs)


@pytest.mark.parametrize("Tq,Tk,E,heads,causal,ragged,p", [
    (1, 1, 64, 2, False, False, 0.0),      # the one-key form
    (37, 74, 64, 2, True, False, 0.0),
    (70, 70, 128, 2, False, False, 0.0),
    (37, 74, 64, 2, True, True, 0.0),      # ragged padding
    (37, 74, 64, 2, True, False, 0.3)])    # attention dropout, against the op's own keep mask
def test_mha_residual_vs_float64(Tq, Tk, E, heads, causal, ragged, p):
    _mha_case(Tq, Tk, E, heads, causal, ragged, p)


# ------------------------------------------------------------------ 4. recurrences under the residual
@pytest.mark.parametrize("state", [False, True])
@pytest.mark.parametrize("T", [1, 2, 7])
@pytest.mark.parametrize("kind", ["lstm", "bilstm", "gru"])
def test_rnn_residual_vs_float64(kind, T, state):
    from multimodalreactiongeneration_amd import functional as Fn
    from multimodalreactiongeneration_amd.model.layers import GRU, LSTM
    B, H = 3, 16
    bi = kind == "bilstm"
    In = 2 * H if bi else H
    torch.manual_seed(T * 3 + len(kind))
    mod = (GRU(In, H) if kind == "gru" else LSTM(In, H, bidirectional=bi)).to(DEV)
    g = torch.Generator().manual_seed(T + 17)
    D = 2 if bi else 1
    x, do = torch.randn(B, T, In, generator=g), torch.randn(B, T, In, generator=g)
    h0, c0 = torch.randn(D, B, H, generator=g) * 0.5, torch.randn(D, B, H, generator=g) * 0.5
    xr = x.double().requires_grad_(True)
    st_r = None
    if state:
        h0r, c0r = h0.double().requires_grad_(True), c0.double().requires_grad_(True)
        st_r = h0r if kind == "gru" else (h0r, c0r)
    yr, _, rnn = R.rnn_residual("gru" if kind == "gru" else "lstm", mod, xr, st_r)
    yr.backward(do.double())
    xd = x.to(DEV).requires_grad_(True)
    h0d = h0.to(DEV).requires_grad_(True) if state else None
    c0d = c0.to(DEV).requires_grad_(True) if state else None
    if kind == "gru":
        y, _ = Fn.gru_residual(xd, *mod.direction_params(0), None if h0d is None else h0d[0])
    elif bi:
        y, _, _ = Fn.lstm_bidirectional_residual(xd, mod.direction_params(0, False), mod.direction_params(0, True),
                                                 h0d, c0d)
    else:
        y, _, _ = Fn.lstm_residual(xd, *mod.direction_params(0), None if h0d is None else h0d[0],
                                   None if c0d is None else c0d[0])
    y.backward(do.to(DEV))
    torch.cuda.synchronize()
    errs = {"y": rel_err(y, yr), "dx": rel_err(xd.grad, xr.grad)}
    for k, p in mod.named_parameters():
        if not state and T == 1 and k.startswith("weight_hh"):
            assert rnn.get_parameter(k).grad.abs().max() == 0   # no previous state: nothing reaches W_hh
            assert p.grad is None or p.grad.abs().max() == 0
            continue
        errs[k] = rel_err(p.grad, rnn.get_parameter(k).grad)
    if state:
        errs["dh0"] = rel_err(h0d.grad, h0r.grad)
        if kind != "gru":
            errs["dc0"] = rel_err(c0d.grad, c0r.grad)
    _within(errs)
    with torch.no_grad():   # outside autograd the add runs over the layer output: the same values
        if kind == "gru":
            y2 = Fn.gru_residual(xd, *mod.direction_params(0), None if h0d is None else h0d[0])[0]
        elif bi:
            y2 = Fn.lstm_bidirectional_residual(xd, mod.direction_params(0, False), mod.direction_params(0, True),
                                                h0d, c0d)[0]
        else:
            y2 = Fn.lstm_residual(xd, *mod.direction_params(0), None if h0d is None else h0d[0],
                                  None if c0d is None else c0d[0])[0]
        assert torch.equal(y2, y.detach())


# ------------------------------------------------------------------ 5. the three no-LN models
def _simple_inputs(d):
    return tuple(torch.from_numpy(d[k]).to(DEV) for k in ("in/audio", "in/motion", "in/target"))


def _check_golden(d, m, loss):
    errs = {"loss": abs(loss.item() - float(d["loss"])) / abs(float(d["loss"]))}
    stored = [k[len("grad/"):] for k in d.files if k.startswith("grad/")]
    named = dict(m.named_parameters())
    assert len(stored) == 2 and stored[0] == next(iter(named)) and stored[1] == list(named)[-1]
    for k in stored:
        errs[k] = rel_err(named[k].grad, d[f"grad/{k}"])
    print({k: f"{e:.2e}" for k, e in errs.items()})
    for k, e in errs.items():
        assert e < TOL, (k, e)


def _step_and_check(d, m, batch):
    from multimodalreactiongeneration_amd import functional as Fn
    opt = m.configure_optimizers()["optimizer"]
    loss = m.training_step(batch)["loss"]
    loss.backward()
    torch.cuda.synchronize()
    _check_golden(d, m, loss)
    before = opt.flat.clone()
    opt.step()
    torch.cuda.synchronize()
    Fn.check_errors()
    assert torch.isfinite(opt.flat).all() and not torch.equal(opt.flat, before)


def test_simple_lstm_without_layernorm_vs_golden():
    m, d, _ = build("simple", DEV)
    a, mo, t = _simple_inputs(d)
    with torch.no_grad():
        e = rel_err(m.forward(a, mo), d["y"])
        print(f"y {e:.2e}")
        assert e < TOL
    _step_and_check(d, m, (a, mo, t))


def test_lstm_with_sample_without_layernorm_vs_golden():
    m, d, _ = build("sample", DEV)
    m.current_epoch = 30
    batch = batch_from(d, DEV)
    with torch.no_grad():
        e = rel_err(m.forward(*batch[:-1])[0], d["y"])
        print(f"y {e:.2e}")
        assert e < TOL
    _step_and_check(d, m, [(x.clone(), n) for x, n in batch])
    m.eval()
    with torch.no_grad():
        g1 = m.prediction([(x.clone(), n) for x, n in batch], full_generation=True)[0]
        g2 = m.prediction([(x.clone(), n) for x, n in batch], full_generation=True)[0]
    assert torch.isfinite(g1).all() and torch.equal(g1, g2)


def test_metaformer_without_layernorm_vs_golden():
    m, d, _ = build("meta", DEV)
    batch = batch_from(d, DEV)
    with torch.no_grad():
        b2 = [(x.clone(), n) for x, n in batch]
        b2[2] = (b2[2][0] * (b2[2][0] != -100).float(), b2[2][1])
        e = rel_err(m.forward(*b2[:-1])[0], d["y"])
        print(f"y {e:.2e}")
        assert e < TOL
    _step_and_check(d, m, [(x.clone(), n) for x, n in batch])
    m.current_epoch = 30
    m.eval()
    with torch.no_grad():
        g1 = m.prediction([(x.clone(), n) for x, n in batch], full_generation=True)[0]
        g2 = m.prediction([(x.clone(), n) for x, n in batch], full_generation=True)[0]
    assert torch.isfinite(g1).all() and torch.equal(g1, g2)


@pytest.mark.parametrize("mask", [[True, False, True, True, False, True], [False] * 6, [True] * 6],
                         ids=["mixed", "teacher", "sampled"])
def test_metaformer_without_layernorm_level_schedule_equals_frame_loop(mask):
    """The scheduled-sampling step of the no-LN golden model: the level schedule (ss_levels.py) against
    the per-frame loop, loss and every gradient at the bar tests/test_gpu_ss_levels.py uses (1e-4)."""
    from multimodalreactiongeneration_amd import functional as Fn
    from tests.residual_cases import load_case, model_class
    from tests.golden_util import config, prefixed
    d = load_case("meta")
    cfg = config(d)
    cfg["model"]["use_scheduled_sampling"] = True
    m = model_class("meta")(cfg["model"], cfg["optim"], cfg["metrics"])
    m.load_state_dict(prefixed(d, "param/"), strict=True)
    m = m.to(DEV)
    m.current_epoch = 30
    batch = batch_from(d, DEV)
    mask = torch.tensor(mask)

    def step(levels_on):
        for p in m.parameters():
            p.grad = None
        m.configure_optimizers()
        m.use_level_schedule = levels_on
        try:
            loss = m.training_step([(x.clone(), n) for x, n in batch], sampling_mask=mask)["loss"]
            loss.backward()
            torch.cuda.synchronize()
            Fn.check_errors()
        finally:
            del m.use_level_schedule
        return loss.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters()}
    loss1, g1 = step(True)
    loss0, g0 = step(False)
    err = abs(loss1.item() - loss0.item()) / abs(loss0.item())
    worst = max((rel_err(g1[k], g0[k]), k) for k in g0)
    print(f"loss rel err {err:.2e}; worst gradient {worst[0]:.2e} ({worst[1]})")
    assert err < TOL and worst[0] < TOL, (err, worst)


# ------------------------------------------------------------------ 6. graph capture
def test_simple_lstm_without_layernorm_graph_replay_bitwise():
    """One training step (forward, backward, AdamW) captured and replayed twice: after each replay the
    parameters are bitwise those of the same number of eager steps (the add launch and the epilogue
    forms read no host state)."""
    from multimodalreactiongeneration_amd import functional as Fn
    from multimodalreactiongeneration_amd.graphs import capture
    eager, d, _ = build("simple", DEV)
    graphed, _, _ = build("simple", DEV)
    batch = _simple_inputs(d)

    def stepper(m):
        opt = m.configure_optimizers()["optimizer"]

        def step():
            opt.zero_grad()
            m.training_step(batch)["loss"].backward()
            opt.step()
        return opt, step
    opt_e, step_e = stepper(eager)
    opt_g, step_g = stepper(graphed)
    replay = capture(step_g, 1, preserve=opt_g.state_tensors())
    assert torch.equal(opt_g.flat, opt_e.flat)
    for _ in range(2):
        step_e()
        replay()
        torch.cuda.synchronize()
        Fn.check_errors()
        assert torch.equal(opt_g.flat, opt_e.flat)


# ------------------------------------------------------------------ 7. LayerNorm paths are as they were
def test_layernorm_models_never_call_the_new_ops(monkeypatch):
    from multimodalreactiongeneration_amd import configs as C
    from multimodalreactiongeneration_amd import functional as Fn
    from multimodalreactiongeneration_amd.model import Metaformer, SimpleLSTM
    from multimodalreactiongeneration_amd.synthetic import make_batch, make_simple_batch
    calls = []
    new_ops = ("residual_add", "linear_residual", "ffn_residual", "linear_add", "mha_residual", "lstm_residual",
               "lstm_bidirectional_residual", "gru_residual")
    for name in new_ops:
        monkeypatch.setattr(Fn, name, lambda *a, _n=name, **k: calls.append(_n))
    torch.manual_seed(0)
    m = Metaformer(*C.lstmformer_config(hidden=32, num_block=1, encoder_num_layer=1, num_heads=2, bottleneck=16,
                                        emb_mixers=("mha", "gru", "lstm"))).to(DEV)
    m.training_step(make_batch(B=2, T=6, lead=2, seed=3, device=DEV))["loss"].backward()
    s = SimpleLSTM(*C.simple_lstm_config(hidden=32, lstm=16, bottleneck=8, att_heads=2, att_layers=1, enc_layers=1,
                                         dec_layers=1, mapping=8)).to(DEV)
    s.training_step(make_simple_batch(B=2, T=6, device=DEV))["loss"].backward()
    torch.cuda.synchronize()
    assert calls == []
    # and a no-LN connection does reach them (the patch is in the way: the count is the check)
    from multimodalreactiongeneration_amd.model.layers import ResidualConnection
    ResidualConnection(torch.nn.Identity(), False)(torch.zeros(2, 4, device=DEV))
    assert calls == ["residual_add"]
