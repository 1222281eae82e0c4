"""need_weights on the device: mrg_attention_weights through the C ABI against the float64 restatement of
tests/attention_weights_ref.py (every head width, both causal ratios, padding, the tile edge, one key; per
head and head-averaged; the scalar store form; the memory around the output; hidden positions exactly 0;
row sums; the extra keys; fully hidden rows; dropout with the op's own keep mask), then functional.mha,
layers.MultiheadAttention, Metaformer.attention_maps and SimpleLSTM.attention_maps.

Error measure: tests.golden_util.rel_err (max |a - ref| / max |ref|), bound TOL = 1e-4 as the neighbouring
attention tests.  Row sums: attention_weights_ref.row_sum_bound.  Every comparison prints its figure (-s)."""
import math

import pytest
import torch

from tests import attention_extra_ref as X
from tests import attention_weights_ref as W
from tests.golden_util import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = "cuda:0"
SEED = 20240917


def _fn():
    from multimodalreactiongeneration_amd import functional as Fn
    return Fn


@pytest.fixture(scope="module")
def lib():
    from multimodalreactiongeneration_amd import _lib as L
    lib = L.load()
    yield lib
    torch.cuda.synchronize()


def _ptr(t, off=0):
    from multimodalreactiongeneration_amd.functional import _ptr as p
    return p(t) if off == 0 else p(t, off)


def _stream():
    from multimodalreactiongeneration_amd.functional import _stream as s
    return s()


def _forward(lib, c, Q, KV, qpad, kpad, bias=None, zero=False, batch=W.B):
    """mrg_attention_fwd (+ the extra-key merge) on device Q / KV: the lse the weights kernel takes"""
    E, D = c.E, c.E // c.heads
    O = torch.empty(batch, c.Tq, E, device=DEV)
    lse = torch.empty(batch, c.heads, c.Tq, device=DEV)
    scale = 1.0 / math.sqrt(D)
    assert lib.mrg_attention_fwd(batch, c.heads, c.Tq, c.Tk, D, _ptr(Q), c.Tq * E, E, _ptr(KV), c.Tk * 2 * E, 2 * E,
                                 _ptr(KV, E), c.Tk * 2 * E, 2 * E, _ptr(O), c.Tq * E, E, _ptr(lse), _ptr(qpad),
                                 _ptr(kpad), int(c.causal), scale, _stream()) == 0
    if bias is not None or zero:
        bk, bv = (None, None) if bias is None else bias
        assert lib.mrg_attention_extra_fwd(batch, c.heads, c.Tq, D, _ptr(Q), c.Tq * E, E, _ptr(bk), _ptr(bv), int(zero),
                                           scale, _ptr(O), c.Tq * E, E, _ptr(lse), c.Tk, 0, 1.0, None, _stream()) == 0
    return lse, scale


def _weights(lib, c, Q, KV, lse, qpad, kpad, scale, average, out, bias_k=None, zero=False, batch=W.B):
    E = c.E
    return lib.mrg_attention_weights(batch, c.heads, c.Tq, c.Tk, E // c.heads, _ptr(Q), c.Tq * E, E, _ptr(KV),
                                     c.Tk * 2 * E, 2 * E, _ptr(bias_k), int(zero), _ptr(lse), _ptr(qpad), _ptr(kpad),
                                     int(c.causal), scale, int(average), 0, 1.0, None, _ptr(out), _stream())


def _guarded(shape, lead):
    """(buffer of NaN, view of ``shape`` starting ``lead`` floats in, 64 more NaN floats behind it)"""
    n = math.prod(shape)
    buf = torch.full((lead + n + 64,), float("nan"), device=DEV)
    return buf, buf[lead:lead + n].view(shape)


_REF = {}


def _reference(c):
    """float64 P [B, heads, Tq, Tk] of a case (computed once, not to be modified) and its bool hidden mask"""
    if c not in _REF:
        Q, KV = W.projected(c)
        qpad, kpad = W.pads(c)
        vis = W.visible(c.Tq, c.Tk, c.causal, qpad, kpad, W.B)
        P, _ = W.probs(Q.double(), KV[..., :c.E].double(), c.heads, 1.0 / math.sqrt(c.E // c.heads), vis)
        _REF[c] = (P, ~vis)
    return _REF[c]


@pytest.mark.parametrize("lead", [0, 1], ids=["aligned", "offset4B"])
@pytest.mark.parametrize("average", [False, True], ids=["heads", "mean"])
@pytest.mark.parametrize("c", W.CASES, ids=lambda c: f"{c.Tq}x{c.Tk}E{c.E}h{c.heads}")
def test_kernel_against_float64(lib, c, average, lead):
    """lead = 1: the output starts 4 bytes past a 16-byte boundary, so every row whose start is not
    aligned takes the scalar stores.  The NaN floats in front of and behind the output must survive."""
    Q, KV = (t.to(DEV) for t in W.projected(c))
    qpad, kpad = (None if t is None else t.to(DEV) for t in W.pads(c))
    lse, scale = _forward(lib, c, Q, KV, qpad, kpad)
    shape = (W.B, c.Tq, c.Tk) if average else (W.B, c.heads, c.Tq, c.Tk)
    buf, out = _guarded(shape, 4 + lead)
    assert out.data_ptr() % 16 == (4 * lead) % 16
    assert _weights(lib, c, Q, KV, lse, qpad, kpad, scale, average, out) == 0
    torch.cuda.synchronize()
    P, hid = _reference(c)
    ref = P.mean(1) if average else P
    got = out.cpu()
    assert torch.isfinite(ref).all() and torch.isfinite(got).all()
    err = rel_err(got, ref)
    print(f"weights {c} average={average} lead={lead}: rel_err {err:.2e}")
    assert err < TOL
    hidden = hid if average else hid.unsqueeze(1).expand_as(got)
    assert bool((got[hidden] == 0).all())
    assert torch.isnan(buf[:4 + lead]).all() and torch.isnan(buf[4 + lead + out.numel():]).all()


@pytest.mark.parametrize("average", [False, True], ids=["heads", "mean"])
@pytest.mark.parametrize("c", W.CASES, ids=lambda c: f"{c.Tq}x{c.Tk}E{c.E}h{c.heads}")
def test_row_sums(lib, c, average):
    """Without dropout every finite row sums to 1, within 4x the largest deviation the float64 reference
    rounded to float32 shows on the same inputs (attention_weights_ref.row_sum_bound).

    The bound is 4e-8 to 1.6e-7 here, mostly below one float32 ulp of 1.0.  exp(s - lse) alone misses it
    (measured 1.7e-7 to 6.2e-7: lse is ONE float32 per row and its rounding, up to 2.4e-7 at lse near 4.8,
    scales the whole row), which is why the kernel divides each row by the double sum of its own terms."""
    Q, KV = (t.to(DEV) for t in W.projected(c))
    qpad, kpad = (None if t is None else t.to(DEV) for t in W.pads(c))
    lse, scale = _forward(lib, c, Q, KV, qpad, kpad)
    out = torch.empty((W.B, c.Tq, c.Tk) if average else (W.B, c.heads, c.Tq, c.Tk), device=DEV)
    assert _weights(lib, c, Q, KV, lse, qpad, kpad, scale, average, out) == 0
    P, _ = _reference(c)
    dev, bound = W.row_sum_dev(out.cpu()), W.row_sum_bound(P.mean(1) if average else P)
    print(f"row sums {c} average={average}: off by {dev:.2e}, bound {bound:.2e}")
    assert dev <= bound


@pytest.mark.parametrize("average", [False, True], ids=["heads", "mean"])
@pytest.mark.parametrize("combo", list(X.COMBOS))
def test_extra_keys(lib, combo, average):
    c = W.CASES[1]   # causal, ragged, Tk = 2 Tq: widths 75 and 76
    Q, KV = (t.to(DEV) for t in W.projected(c))
    qpad, kpad = W.pads(c)
    has_b, zero = X.COMBOS[combo]
    g = torch.Generator().manual_seed(5)
    bk, bv = (torch.randn(c.E, generator=g), torch.randn(c.E, generator=g)) if has_b else (None, None)
    bias = (bk.to(DEV), bv.to(DEV)) if has_b else None
    lse, scale = _forward(lib, c, Q, KV, qpad.to(DEV), kpad.to(DEV), bias, zero)
    n = c.Tk + X.n_extra(combo)
    buf, out = _guarded((W.B, c.Tq, n) if average else (W.B, c.heads, c.Tq, n), 4)
    assert _weights(lib, c, Q, KV, lse, qpad.to(DEV), kpad.to(DEV), scale, average, out,
                    None if bias is None else bias[0], zero) == 0
    vis = W.visible(c.Tq, c.Tk, c.causal, qpad, kpad, W.B)
    Qc, KVc = W.projected(c)
    ref, _ = W.probs(Qc.double(), KVc[..., :c.E].double(), c.heads, scale, vis, None if bk is None else bk.double(),
                     zero, average=average)
    got = out.cpu()
    err = rel_err(got, ref)
    print(f"extra keys {combo} average={average}: width {n}, rel_err {err:.2e}")
    assert tuple(got.shape)[-1] == n and err < TOL
    assert bool((got[..., c.Tk:] > 0).all())
    assert torch.isnan(buf[:4]).all() and torch.isnan(buf[4 + out.numel():]).all()


def _hidden_row_case():
    """the inputs of test_attention_dropout_fully_masked_row_stays_nan: query 0 sees only key 0, both padded"""
    g = torch.Generator().manual_seed(17)
    q, kv = torch.randn(1, 4, 16, generator=g), torch.randn(1, 4, 16, generator=g)
    q[0, 0] = -100
    kv[0, 0] = -100
    return q, kv, X.weights(16, "bias", seed=17)


@pytest.mark.parametrize("average", [False, True], ids=["heads", "mean"])
def test_fully_hidden_row_is_nan_and_finite_with_a_bias_key(average):
    Fn = _fn()
    heads = 2
    q, kv, w = _hidden_row_case()
    qpad, kpad = Fn.padding_flags(q.to(DEV)), Fn.padding_flags(kv.to(DEV))
    wd = {n: t.to(DEV) for n, t in w.items()}
    _, got = Fn.mha(q.to(DEV), kv.to(DEV), wd["in_w"], wd["in_b"], wd["out_w"], wd["out_b"], heads, True, qpad, kpad,
                    need_weights=True, average_attn_weights=average)
    plain = {n: t.double() for n, t in w.items() if not n.startswith("bias_")}
    _, ref = W.mha(q.double(), kv.double(), plain, heads, True, qpad.cpu(), kpad.cpu(), average=average)
    got = got.cpu()
    row = (0, 0) if average else (0, slice(None), 0)
    assert torch.isnan(ref[row]).all() and torch.isnan(got[row]).all()
    live = ~torch.isnan(ref)
    assert bool((live == ~torch.isnan(got)).all())
    err = rel_err(got[live], ref[live])
    print(f"hidden row average={average}: other rows rel_err {err:.2e}")
    assert err < TOL
    # with a bias key the row is finite and all its weight sits on the extra column
    _, got = Fn.mha(q.to(DEV), kv.to(DEV), wd["in_w"], wd["in_b"], wd["out_w"], wd["out_b"], heads, True, qpad, kpad,
                    bias_k=wd["bias_k"], bias_v=wd["bias_v"], need_weights=True, average_attn_weights=average)
    _, ref = W.mha(q.double(), kv.double(), {n: t.double() for n, t in w.items()}, heads, True, qpad.cpu(), kpad.cpu(),
                   average=average)
    got = got.cpu()
    assert torch.isfinite(got).all() and got.shape[-1] == 5
    # (the extra column is exp(s1 - lse) with |lse| in the hundreds here: within the bar of 1, not bitwise)
    assert bool((got[row][..., :4] == 0).all()) and bool(((got[row][..., 4] - 1).abs() < TOL).all())
    err = rel_err(got, ref)
    print(f"hidden row with a bias key average={average}: rel_err {err:.2e}")
    assert err < TOL


def _module_inputs(c, seed=3):
    g = torch.Generator().manual_seed(seed + c.Tq)
    return torch.randn(W.B, c.Tq, c.E, generator=g), torch.randn(W.B, c.Tk, c.E, generator=g)


@pytest.mark.parametrize("combo", [None, "both"])
@pytest.mark.parametrize("average", [False, True], ids=["heads", "mean"])
def test_dropout_weights_are_the_dropped_ones(combo, average):
    Fn = _fn()
    c, p = W.CASES[1], 0.25
    q, kv = _module_inputs(c)
    w = X.weights(c.E, combo or "zero")
    zero = bool(combo)
    qpad, kpad = W.pads(c)
    wd = {n: t.to(DEV) for n, t in w.items()}
    Fn.manual_seed(SEED, DEV)
    before = Fn.get_rng_state(DEV)
    out, got = Fn.mha(q.to(DEV), kv.to(DEV), wd["in_w"], wd["in_b"], wd["out_w"], wd["out_b"], c.heads, c.causal,
                      qpad.to(DEV), kpad.to(DEV), dropout_p=p, bias_k=wd.get("bias_k"), bias_v=wd.get("bias_v"),
                      add_zero_attn=zero, need_weights=True, average_attn_weights=average)
    after = Fn.get_rng_state(DEV)
    assert after == (before[0], before[1] + 1)   # one draw, not two
    n = c.Tk + (2 if combo else 0)
    key = torch.tensor([Fn._i64(before[0]), Fn._i64(before[1])], dtype=torch.int64, device=DEV)
    keep = Fn.attention_keep_mask(key, W.B, c.heads, c.Tq, n, p).bool().cpu()
    ro, ref = W.mha(q.double(), kv.double(), {k: t.double() for k, t in w.items()}, c.heads, c.causal, qpad, kpad, zero,
                    keep, p, average=False)
    gh = got.cpu()
    if not average:
        assert bool((gh[~keep] == 0).all())
    else:
        ref = ref.mean(1)
        assert bool((gh[~keep.any(1)] == 0).all())
    err, eo = rel_err(gh, ref), rel_err(out, ro)
    print(f"dropout weights combo={combo} average={average}: rel_err {err:.2e} (out {eo:.2e})")
    assert err < TOL and eo < TOL


@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("c", [W.CASES[0], W.CASES[1], W.CASES[5]], ids=lambda c: f"{c.Tq}x{c.Tk}")
def test_need_weights_leaves_out_and_gradients_bitwise(c, p):
    Fn = _fn()
    q, kv = _module_inputs(c)
    w = X.weights(c.E, "zero")
    qpad, kpad = (None if t is None else t.to(DEV) for t in W.pads(c))
    do = torch.randn(W.B, c.Tq, c.E, generator=torch.Generator().manual_seed(9)).to(DEV)
    res = []
    for need in (False, True):
        ps = {n: torch.nn.Parameter(t.clone().to(DEV)) for n, t in w.items()}
        qd, kvd = q.to(DEV).requires_grad_(True), kv.to(DEV).requires_grad_(True)
        Fn.manual_seed(SEED, DEV)
        before = Fn.get_rng_state(DEV)
        r = Fn.mha(qd, kvd, ps["in_w"], ps["in_b"], ps["out_w"], ps["out_b"], c.heads, c.causal, qpad, kpad,
                   dropout_p=p, need_weights=need)
        assert Fn.get_rng_state(DEV) == (before[0], before[1] + (1 if p else 0))   # no extra draw either way
        if need:
            out, wts = r
            assert not wts.requires_grad and wts.grad_fn is None
            assert tuple(wts.shape) == (W.B, c.Tq, c.Tk)
        else:
            assert isinstance(r, torch.Tensor)
            out = r
        out.backward(do)
        res.append([out.detach()] + [t.grad for t in (qd, kvd, *ps.values())])
    for a, b in zip(*res):
        assert (a is None) == (b is None)
        if a is not None:
            assert torch.equal(a, b)


def test_one_key_form_builds_its_weights_without_the_kernel():
    Fn = _fn()
    c = W.CASES[5]
    q, kv = _module_inputs(c)
    wd = {n: t.to(DEV) for n, t in X.weights(c.E, "zero").items()}
    qpad = torch.tensor([[1], [0]], dtype=torch.uint8, device=DEV)
    kpad = torch.tensor([[1], [1]], dtype=torch.uint8, device=DEV)
    for average, shape in ((True, (2, 1, 1)), (False, (2, c.heads, 1, 1))):
        out, wts = Fn.mha(q.to(DEV), kv.to(DEV), wd["in_w"], wd["in_b"], wd["out_w"], wd["out_b"], c.heads, True, qpad,
                          kpad, need_weights=True, average_attn_weights=average)
        assert tuple(wts.shape) == shape and not wts.requires_grad
        assert torch.isnan(wts[0]).all() and bool((wts[1] == 1).all())
        assert torch.isnan(out[0]).all() and torch.isfinite(out[1]).all()


@pytest.mark.parametrize("batch_first", [True, False])
def test_layer_returns_torch_shapes_and_records(batch_first):
    from multimodalreactiongeneration_amd.model import layers
    torch.manual_seed(1)
    E, heads, Tq, Tk = 32, 4, 6, 9
    m = layers.MultiheadAttention(E, heads, batch_first=batch_first).to(DEV)
    ref = torch.nn.MultiheadAttention(E, heads, batch_first=batch_first).double()
    ref.load_state_dict({k: v.double().cpu() for k, v in m.state_dict().items()})
    q, kv = torch.randn(W.B, Tq, E), torch.randn(W.B, Tk, E)
    if not batch_first:
        q, kv = q.transpose(0, 1).contiguous(), kv.transpose(0, 1).contiguous()
    qd, kvd = q.to(DEV), kv.to(DEV)
    for average in (True, False):
        out, wts = m(qd, kvd, kvd, need_weights=True, average_attn_weights=average)
        ro, rw = ref(q.double(), kv.double(), kv.double(), need_weights=True, average_attn_weights=average)
        assert tuple(out.shape) == tuple(ro.shape) and tuple(wts.shape) == tuple(rw.shape)
        assert rel_err(out, ro) < TOL and rel_err(wts, rw) < TOL
    out, none = m(qd, kvd, kvd)
    assert none is None and m.last_weights is None
    m.record_weights = "heads"
    out2, none = m(qd, kvd, kvd)
    assert none is None and torch.equal(out, out2)
    assert tuple(m.last_weights.shape) == (W.B, heads, Tq, Tk) and not m.last_weights.requires_grad
    assert rel_err(m.last_weights, rw) < TOL


def test_averaged_form_is_deterministic(lib):
    c = W.CASES[2]
    Q, KV = (t.to(DEV) for t in W.projected(c))
    lse, scale = _forward(lib, c, Q, KV, None, None)
    outs = []
    for _ in range(2):
        out = torch.full((W.B, c.Tq, c.Tk), float("nan"), device=DEV)
        assert _weights(lib, c, Q, KV, lse, None, None, scale, True, out) == 0
        outs.append(out)
    assert torch.equal(*outs)


def test_refusals_and_empty_sizes(lib):
    c = W.CASES[4]
    Q, KV = (t.to(DEV) for t in W.projected(c))
    lse, scale = _forward(lib, c, Q, KV, None, None)
    out = torch.full((W.B, c.heads, c.Tq, c.Tk), 7.0, device=DEV)
    args = lambda **kw: [kw.get("B", W.B), c.heads, kw.get("Tq", c.Tq), kw.get("Tk", c.Tk), kw.get("D", 16), _ptr(Q),
                         c.Tq * c.E, c.E, _ptr(KV), c.Tk * 2 * c.E, 2 * c.E, None, 0, kw.get("lse", _ptr(lse)), None, None,
                         1, scale, 0, 0, 1.0, None, kw.get("out", _ptr(out)), _stream()]
    for bad in (dict(D=12), dict(Tq=-1), dict(Tq=70000), dict(lse=None), dict(out=None), dict(Tq=3, Tk=20)):
        assert lib.mrg_attention_weights(*args(**bad)) != 0, bad
    for empty in (dict(B=0), dict(Tq=0), dict(Tk=0)):
        assert lib.mrg_attention_weights(*args(**empty)) == 0, empty
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def _metaformer(ratio):
    from multimodalreactiongeneration_amd import configs as C
    from multimodalreactiongeneration_amd.model import Metaformer
    from multimodalreactiongeneration_amd.synthetic import clone_batch, make_batch
    torch.manual_seed(0)
    mc, oc, me = C.lstmformer_config(hidden=32, num_block=1, encoder_num_layer=1, bottleneck=8, num_heads=2, ratio=ratio)
    model = Metaformer(mc, oc, me).to(DEV)
    batch = clone_batch(make_batch(B=2, T=16, lead=3, ratio=ratio, seed=11, lengths=[16, 11]), DEV)
    return model, batch


@pytest.mark.parametrize("average", [True, False], ids=["mean", "heads"])
@pytest.mark.parametrize("ratio", [1, 2])
def test_metaformer_attention_maps(ratio, average):
    from multimodalreactiongeneration_amd.model import layers, mixers
    Fn = _fn()
    model, batch = _metaformer(ratio)
    atts = {n: m for n, m in model.named_modules() if isinstance(m, layers.MultiheadAttention)}
    assert len(atts) == 2
    model.train()
    captured = {}
    hooks = []
    for n, blk in model.named_modules():
        if isinstance(blk, mixers.MHAMixerBlock):
            name = next(k for k, m in atts.items() if m is blk.mha_module())
            hooks.append(blk.register_forward_pre_hook(lambda mod, a, name=name: captured.__setitem__(name, a)))
    y, maps = model.attention_maps(*batch[:-1], average_heads=average)
    for h in hooks:
        h.remove()
    assert model.training and all(m.training for m in model.modules())
    assert all(m.record_weights is None and m.last_weights is None for m in atts.values())
    assert list(maps) == list(atts) and set(captured) == set(atts)
    model.eval()
    with torch.no_grad():
        y0, _ = model(*batch[:-1])
    print(f"attention_maps ratio={ratio}: y against the eval forward, max |diff| {(y - y0).abs().max().item():.3e}")
    assert torch.equal(y, y0)
    T = 16 + 3
    for n, m in atts.items():
        q, k, v, mask = captured[n][:4]
        Tk = k.shape[1]
        assert Tk in (T, T * ratio)
        assert tuple(maps[n].shape) == ((2, T, Tk) if average else (2, 2, T, Tk))
        with torch.no_grad():
            _, ref = Fn.mha(q, k, m.in_proj_weight, m.in_proj_bias, m.out_proj.weight, m.out_proj.bias, m.num_heads,
                            True, mask.main_pad, mask.other_pad, need_weights=True, average_attn_weights=average)
        assert torch.equal(maps[n], ref)
        hid = ~W.visible(T, Tk, True, None, None, 2)
        hid = hid if average else hid.unsqueeze(1).expand(2, 2, T, Tk)
        assert bool((maps[n].cpu()[hid] == 0).all())
        assert torch.isfinite(maps[n]).all()
    assert {k.shape[1] for _, k, *_ in captured.values()} == {T, T * ratio}


def test_attention_maps_restores_on_an_exception():
    model, batch = _metaformer(1)
    atts = [m for m in model.modules() if hasattr(m, "record_weights")]
    atts[0].record_weights = "heads"
    model.train()
    with pytest.raises(Exception):
        model.attention_maps(*batch[:2])   # too few inputs: the forward raises
    assert model.training and atts[0].record_weights == "heads" and all(m.record_weights is None for m in atts[1:])


_SIMPLE = {}


def _simple_lstm_maps():
    """{module path: (map on the host, its float64 reference on the inputs the layer saw)}, run once"""
    if _SIMPLE:
        return _SIMPLE
    from multimodalreactiongeneration_amd import configs as C
    from multimodalreactiongeneration_amd.model import SimpleLSTM, layers
    from multimodalreactiongeneration_amd.synthetic import make_simple_batch
    torch.manual_seed(0)
    cfg, oc, me = C.simple_lstm_config(hidden=32, lstm=16, bottleneck=8, att_heads=4, att_layers=2, enc_layers=1,
                                       dec_layers=1, mapping=16)
    model = SimpleLSTM(cfg, oc, me).to(DEV)
    a, m, _ = make_simple_batch(B=2, T=12, device=DEV)
    a = torch.cat([a, a.flip(1)], 1)[:, :20].contiguous()   # Ta = 20, Tm = 12
    model.eval()
    with torch.no_grad():
        y0 = model(a, m)
    atts = {n: mod for n, mod in model.named_modules() if isinstance(mod, layers.MultiheadAttention)}
    captured = {}
    hooks = [mod.register_forward_pre_hook(lambda _m, args, n=n: captured.__setitem__(n, args)) for n, mod in atts.items()]
    y, maps = model.attention_maps(a, m)
    for h in hooks:
        h.remove()
    assert list(maps) == list(atts) and len(atts) == 2 and torch.equal(y, y0)
    for n, mod in atts.items():
        got = maps[n].cpu()
        assert tuple(got.shape) == (2, 12, 20)
        # the float64 weights of this layer on the inputs it saw: the row-sum bound's reference
        q, kv = (t.double().cpu() for t in captured[n][:2])
        w = {"in_w": mod.in_proj_weight, "in_b": mod.in_proj_bias, "out_w": mod.out_proj.weight, "out_b": mod.out_proj.bias}
        _, ref = W.mha(q, kv, {k: t.detach().double().cpu() for k, t in w.items()}, mod.num_heads)
        _SIMPLE[n] = (got, ref)
    return _SIMPLE


def test_simple_lstm_attention_maps():
    """one map [B, Tm, Ta] per cross-attention layer (and y is the eval forward's, checked in the helper)"""
    got = _simple_lstm_maps()
    assert len(got) == 2
    for n, (w, ref) in got.items():
        err = rel_err(w, ref)
        print(f"simple_lstm {n}: rel_err {err:.2e}")
        assert tuple(w.shape) == (2, 12, 20) and err < TOL


def test_simple_lstm_rows_sum_to_one():
    """The row-sum bound of test_row_sums on each layer's map."""
    for n, (w, ref) in _simple_lstm_maps().items():
        dev, bound = W.row_sum_dev(w), W.row_sum_bound(ref)
        print(f"simple_lstm {n}: row sums off by {dev:.2e}, bound {bound:.2e}")
        assert dev <= bound
