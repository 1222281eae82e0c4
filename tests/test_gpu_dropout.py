"""Dropout on the MI355X path: the counter-based RNG's kernels against the host restatement (rng.py),
functional.dropout, attention-probability dropout and the stacked LSTM / GRU against float64 references
that are handed the very mask the kernels used (tests/dropout_ref.py), the lstmformer end to end, graph
replay and the generation plan's train / eval switch.  Bar: rel_err < 1e-4 (tests.golden_util)."""
import math

import numpy as np
import pytest
import torch

from tests import dropout_ref as R
from tests.golden_util import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = "cuda:0"
SEED = 20240607


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from multimodalreactiongeneration_amd import _lib as L
    L.load()
    yield
    from multimodalreactiongeneration_amd import functional as Fn
    torch.cuda.synchronize()
    Fn.check_errors()


def _param(t):
    return torch.nn.Parameter(t.clone().to(DEV))


def _key(seed, draw):
    from multimodalreactiongeneration_amd.functional import _i64
    return torch.tensor([_i64(seed), _i64(draw)], dtype=torch.int64, device=DEV)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_flat_keep_mask_is_bit_identical_to_host(p):
    from multimodalreactiongeneration_amd import functional as Fn
    from multimodalreactiongeneration_amd import rng
    n = 4099
    for seed, draw in ((SEED, 0), (SEED, 7), ((1 << 63) + 12345, (1 << 32) + 3)):
        got = Fn.dropout_keep_mask(_key(seed, draw), n, p).cpu().numpy().astype(bool)
        assert np.array_equal(got, rng.keep_mask(seed, draw, n, p)), (seed, draw)


def test_attention_keep_mask_is_bit_identical_to_host():
    from multimodalreactiongeneration_amd import functional as Fn
    from multimodalreactiongeneration_amd import rng
    B, H, Tq, Tk = 2, 2, 70, 75
    for p in (0.1, 0.5):
        for seed, draw in ((SEED, 2), ((1 << 63) + 12345, (1 << 32) + 3)):
            got = Fn.attention_keep_mask(_key(seed, draw), B, H, Tq, Tk, p).cpu().numpy().astype(bool)
            assert np.array_equal(got, rng.attention_keep_mask(seed, draw, B, H, Tq, Tk, p)), (p, seed, draw)


def test_rng_state_api_and_draw_counter():
    from multimodalreactiongeneration_amd import functional as Fn
    Fn.manual_seed(SEED, DEV)
    assert Fn.get_rng_state(DEV) == (SEED, 0)
    x = torch.ones(5, device=DEV)
    Fn.dropout(x, 0.5)
    Fn.dropout(x, 0.5)
    assert Fn.get_rng_state(DEV) == (SEED, 2)           # one draw per op
    Fn.dropout(x, 0.0)
    assert Fn.get_rng_state(DEV) == (SEED, 2)           # p = 0 takes none
    Fn.set_rng_state(DEV, ((1 << 64) - 1, 41))
    assert Fn.get_rng_state(DEV) == ((1 << 64) - 1, 41)
    Fn.manual_seed(SEED)                                # device None: the current device
    assert Fn.get_rng_state(DEV) == (SEED, 0)


@pytest.mark.parametrize("p,shape", [(0.1, (4099,)), (0.5, (3, 9, 32)), (0.3, (7, 5))])
def test_functional_dropout(p, shape):
    from multimodalreactiongeneration_amd import functional as Fn
    from multimodalreactiongeneration_amd import rng
    g = torch.Generator().manual_seed(5)
    x = torch.randn(*shape, generator=g)
    dy = torch.randn(*shape, generator=g)
    n = x.numel()
    scale = torch.tensor(np.float32(1.0 / (1.0 - p)))
    Fn.manual_seed(SEED, DEV)
    xd = x.to(DEV).requires_grad_(True)
    y = Fn.dropout(xd, p)
    y.backward(dy.to(DEV))
    keep = torch.from_numpy(rng.keep_mask(SEED, 0, n, p)).view(*shape)
    assert torch.equal(y.detach().cpu(), torch.where(keep, x * scale, torch.zeros(())))
    assert torch.equal(xd.grad.cpu(), torch.where(keep, dy * scale, torch.zeros(())))
    y2 = Fn.dropout(xd, p)                               # the next draw: another mask
    assert not torch.equal(y2, y)
    assert torch.equal((y2 != 0).cpu().view(-1), torch.from_numpy(rng.keep_mask(SEED, 1, n, p)) & (x.view(-1) != 0))
    Fn.manual_seed(SEED, DEV)                            # the seed reproduces
    assert torch.equal(Fn.dropout(xd, p), y)
    y0 = Fn.dropout(xd, 0.0)                             # p = 0: the input's values, bitwise
    assert torch.equal(y0, xd)
    # an unaligned view takes the element-wise path
    if len(shape) == 1:
        Fn.manual_seed(SEED, DEV)
        xo = x.to(DEV)[1:]
        keep1 = torch.from_numpy(rng.keep_mask(SEED, 0, n - 1, p))
        assert torch.equal(Fn.dropout(xo, p).cpu(), torch.where(keep1, x[1:] * scale, torch.zeros(())))


def _mha_weights(E, g):
    return {"in_w": torch.randn(3 * E, E, generator=g) / math.sqrt(E), "in_b": torch.randn(3 * E, generator=g) * 0.1,
            "out_w": torch.randn(E, E, generator=g) / math.sqrt(E), "out_b": torch.randn(E, generator=g) * 0.1}


def _run_mha_dropout(q, kv, w, heads, causal, qpad, kpad, p, do):
    """Fn.mha with dropout_p = p on the device and the float64 reference with the mask of the draw the op
    took (read from the state before the call).  Returns (device out, q, kv, params), (reference ...)."""
    from multimodalreactiongeneration_amd import functional as Fn
    B, Tq, _ = q.shape
    Tk = kv.shape[1]
    ps = {k: _param(v) for k, v in w.items()}
    qd, kvd = q.to(DEV).requires_grad_(True), kv.to(DEV).requires_grad_(True)
    seed, draw = Fn.get_rng_state(DEV)
    o = Fn.mha(qd, kvd, ps["in_w"], ps["in_b"], ps["out_w"], ps["out_b"], heads, causal, qpad, kpad, dropout_p=p)
    if do is not None:
        o.backward(do.to(DEV))
    assert Fn.get_rng_state(DEV) == (seed, draw + 1)
    keep = Fn.attention_keep_mask(_key(seed, draw), B, heads, Tq, Tk, p).cpu().bool()
    rs = {k: v.double().requires_grad_(True) for k, v in w.items()}
    qr, kvr = q.double().requires_grad_(True), kv.double().requires_grad_(True)
    orf = R.mha(qr, kvr, rs["in_w"], rs["in_b"], rs["out_w"], rs["out_b"], heads, causal,
                None if qpad is None else qpad.cpu(), None if kpad is None else kpad.cpu(), keep, p)
    if do is not None:
        orf.backward(do.double())
    return (o, qd, kvd, ps), (orf, qr, kvr, rs), keep


@pytest.mark.parametrize("Tq,Tk,E,heads,causal,ragged", [
    (70, 70, 128, 2, False, False),   # D = 64 across the 64-tile edge; p = 0 here takes the single-pass backward
    (37, 74, 64, 2, True, True),
    (40, 20, 128, 4, True, False),
    (33, 33, 32, 4, False, False),    # D = 8
    (20, 20, 64, 4, True, False),     # D = 16
    (1, 1, 64, 2, False, False)])     # one key: the probability 1 is still dropped
def test_attention_dropout_vs_float64(Tq, Tk, E, heads, causal, ragged):
    """Output, dq, dkv and the four parameter gradients against float64 with the op's own mask, each at
    rel_err < 1e-4.  With one key the float64 query gradient is exactly zero, so rel_err divides by its
    1e-6 floor: the case holds because the dQ kernel forms delta from the terms it is subtracted from
    (attention.hip), which makes the one-key dS cancel exactly (dq = 0.0 measured)."""
    from multimodalreactiongeneration_amd import functional as Fn
    B, p = 2, 0.25
    g = torch.Generator().manual_seed(Tq * 5 + Tk)
    q, kv = torch.randn(B, Tq, E, generator=g), torch.randn(B, Tk, E, generator=g)
    qpad = kpad = None
    if ragged:
        q[1, Tq * 2 // 3:] = -100.0
        kv[1, Tk // 2:] = -100.0
    if causal:
        qpad, kpad = Fn.padding_flags(q.to(DEV)), Fn.padding_flags(kv.to(DEV))
    w = _mha_weights(E, g)
    do = torch.randn(B, Tq, E, generator=g)
    Fn.manual_seed(SEED + Tq, DEV)
    (o, qd, kvd, ps), (orf, qr, kvr, rs), keep = _run_mha_dropout(q, kv, w, heads, causal, qpad, kpad, p, do)
    assert not torch.isnan(orf).any()
    assert not keep.all() and keep.any()
    errs = {"out": rel_err(o, orf), "dq": rel_err(qd.grad, qr.grad), "dkv": rel_err(kvd.grad, kvr.grad)}
    errs.update({k: rel_err(ps[k].grad, rs[k].grad) for k in w})
    print(errs)
    for k, e in errs.items():
        assert e < TOL, (k, e)


def test_attention_dropout_one_key_rows_are_dropped_or_scaled():
    """Tq = Tk = 1 with dropout goes through the attention kernel, not the one-key shortcut: a dropped
    (sample, head) contributes zero, a kept one V / (1 - p)."""
    from multimodalreactiongeneration_amd import functional as Fn
    B, E, heads, p = 16, 64, 2, 0.5
    g = torch.Generator().manual_seed(3)
    q, kv = torch.randn(B, 1, E, generator=g), torch.randn(B, 1, E, generator=g)
    Fn.manual_seed(SEED, DEV)
    (o, *_), (orf, *_), keep = _run_mha_dropout(q, kv, _mha_weights(E, g), heads, False, None, None, p, None)
    assert keep.any() and not keep.all()
    assert rel_err(o, orf) < TOL


def test_attention_dropout_fully_masked_row_stays_nan():
    """A query row the mask rules hide entirely is NaN with dropout too (the softmax over an all -inf
    row), and the other rows match the float64 reference."""
    from multimodalreactiongeneration_amd import functional as Fn
    B, T, E, heads, p = 1, 4, 16, 2, 0.25
    g = torch.Generator().manual_seed(17)
    q, kv = torch.randn(B, T, E, generator=g), torch.randn(B, T, E, generator=g)
    q[0, 0] = -100
    kv[0, 0] = -100   # query 0 sees only key 0, both padded -> masked
    Fn.manual_seed(SEED, DEV)
    (o, *_), (orf, *_), _ = _run_mha_dropout(q, kv, _mha_weights(E, g), heads, True, Fn.padding_flags(q.to(DEV)),
                                             Fn.padding_flags(kv.to(DEV)), p, None)
    assert torch.isnan(orf[0, 0]).all() and torch.isnan(o[0, 0].cpu()).all()
    assert rel_err(o[0, 1:], orf[0, 1:]) < TOL


@pytest.mark.parametrize("Tq,Tk,E,heads,causal", [(70, 70, 128, 2, False), (37, 74, 64, 2, True), (1, 1, 64, 2, False)])
def test_mha_dropout_p_zero_is_the_old_path(Tq, Tk, E, heads, causal):
    from multimodalreactiongeneration_amd import functional as Fn
    B = 2
    g = torch.Generator().manual_seed(Tq + 3 * Tk)
    q, kv = torch.randn(B, Tq, E, generator=g), torch.randn(B, Tk, E, generator=g)
    w = _mha_weights(E, g)
    do = torch.randn(B, Tq, E, generator=g).to(DEV)
    qpad = torch.zeros(B, Tq, dtype=torch.uint8, device=DEV) if causal else None
    kpad = torch.zeros(B, Tk, dtype=torch.uint8, device=DEV) if causal else None
    before = Fn.get_rng_state(DEV)
    res = []
    for kw in ({}, {"dropout_p": 0.0}):
        ps = {k: _param(v) for k, v in w.items()}
        qd, kvd = q.to(DEV).requires_grad_(True), kv.to(DEV).requires_grad_(True)
        o = Fn.mha(qd, kvd, ps["in_w"], ps["in_b"], ps["out_w"], ps["out_b"], heads, causal, qpad, kpad, **kw)
        o.backward(do)
        res.append([o.detach(), qd.grad, kvd.grad] + [ps[k].grad for k in w])
    assert Fn.get_rng_state(DEV) == before                # no draw
    for a, b in zip(*res):
        if a is None or b is None:
            assert a is None and b is None
        else:
            assert torch.equal(a, b)


@pytest.mark.parametrize("kind,layers,bidir", [("lstm", 3, False), ("lstm", 3, True), ("gru", 2, False)])
def test_stacked_rnn_dropout_vs_float64(kind, layers, bidir):
    from multimodalreactiongeneration_amd import functional as Fn
    from multimodalreactiongeneration_amd import rng
    from multimodalreactiongeneration_amd.model import layers as L
    In, H, B, T, p = 16, 32, 3, 9, 0.3
    cls = L.LSTM if kind == "lstm" else L.GRU
    torch.manual_seed(layers * 10 + bidir)
    m = cls(In, H, num_layers=layers, dropout=p, bidirectional=bidir).to(DEV).train()
    g = torch.Generator().manual_seed(23)
    x = torch.randn(B, T, In, generator=g)
    HD = H * (2 if bidir else 1)
    dy = torch.randn(B, T, HD, generator=g)
    nst = layers * (2 if bidir else 1)
    dst = [torch.randn(nst, B, H, generator=g) for _ in range(2 if kind == "lstm" else 1)]
    Fn.manual_seed(SEED, DEV)
    seed, draw0 = Fn.get_rng_state(DEV)
    xd = x.to(DEV).requires_grad_(True)
    y, st = m(xd)
    sts = list(st) if kind == "lstm" else [st]
    (y * dy.to(DEV)).sum().add(sum((s * d.to(DEV)).sum() for s, d in zip(sts, dst))).backward()
    assert Fn.get_rng_state(DEV) == (seed, draw0 + layers - 1)   # one draw per layer but the last
    keeps = [torch.from_numpy(rng.keep_mask(seed, draw0 + l, B * T * HD, p)).view(B, T, HD) for l in range(layers - 1)]
    xr = x.double().requires_grad_(True)
    yr, str_, ref_layers = R.stacked_rnn(kind, m, xr, keeps, p)
    strs = list(str_) if kind == "lstm" else [str_]
    (yr * dy.double()).sum().add(sum((s * d.double()).sum() for s, d in zip(strs, dst))).backward()
    errs = {"y": rel_err(y, yr), "dx": rel_err(xd.grad, xr.grad)}
    for i, (s, sr) in enumerate(zip(sts, strs)):
        errs[f"state{i}"] = rel_err(s, sr)
    for l, rl in enumerate(ref_layers):
        for d in range(2 if bidir else 1):
            for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                sfx = "_reverse" if d else ""
                errs[f"{n}_l{l}{sfx}"] = rel_err(getattr(m, f"{n}_l{l}{sfx}").grad, getattr(rl, f"{n}_l0{sfx}").grad)
    print(errs)
    for k, e in errs.items():
        assert e < TOL, (k, e)
    # eval(): bitwise the same module built with dropout = 0 and the same weights, and no draw
    m0 = cls(In, H, num_layers=layers, dropout=0.0, bidirectional=bidir).to(DEV)
    m0.load_state_dict(m.state_dict())
    before = Fn.get_rng_state(DEV)
    with torch.no_grad():
        ye, _ = m.eval()(x.to(DEV))
        y0, _ = m0.eval()(x.to(DEV))
    assert torch.equal(ye, y0)
    assert Fn.get_rng_state(DEV) == before


def _tiny_metaformer(dropout, hidden=32, num_internal_layer=2, bottleneck=16):
    from multimodalreactiongeneration_amd import configs as C
    from multimodalreactiongeneration_amd.model import Metaformer
    mc, oc, me = C.lstmformer_config(hidden=hidden, num_block=1, encoder_num_layer=1, num_heads=2, bottleneck=bottleneck)
    mc["dropout"] = dropout
    m = Metaformer(mc, oc, me)
    if num_internal_layer > 1:
        # model.num_internal_layer also reaches the integrators' MHAMixer, where more than one layer is
        # refused (the reference feeds a tuple into its layer 2; tests/test_cpu_nonlin.py pins that).  So
        # the LSTM mixer stacks are rebuilt with it and the integrators keep their one attention layer.
        from multimodalreactiongeneration_amd.model.metaformer import MultiModalMetaformer
        m.main_mixer_configs = dict(m.main_mixer_configs, num_internal_layer=num_internal_layer)
        m.other_mixer_configs = [dict(c, num_internal_layer=num_internal_layer) for c in m.other_mixer_configs]
        m.metaformer = MultiModalMetaformer(
            modal_num=m.modal_num, hidden_dim=m.hidden_dim, num_layer=m.num_block,
            main_modal_feature_dim=m.motion_input_size, main_mixer_type=m.main_mixer_type,
            main_mixer_configs=m.main_mixer_configs, integrate_mixer_configs=m.integrate_mixer_configs,
            feedforward_configs=m.feedforward_configs, output_feedforward_configs=m.output_feedforward_configs,
            other_modal_feature_dim=[m.acoustic_input_size, m.motion_input_size],
            other_mixer_type=m.other_mixer_type, other_mixer_configs=m.other_mixer_configs,
            repeat_with_encoder=m.repeat_with_encoder, interlayer_residual=m.interlayer_residual,
            interlayer_residual_norm=m.interlayer_residual_norm)
        lstms = [x for x in m.modules() if type(x).__name__ == "LSTM"]
        assert lstms and all(x.num_layers == num_internal_layer and x.dropout == dropout for x in lstms)
    return m


def test_metaformer_trains_with_dropout():
    from multimodalreactiongeneration_amd import functional as Fn
    from multimodalreactiongeneration_amd.synthetic import clone_batch, make_batch
    torch.manual_seed(0)
    model = _tiny_metaformer(0.2).to(DEV).train()
    ref = _tiny_metaformer(0.0)
    assert list(ref.state_dict().keys()) == list(model.state_dict().keys())
    ref.load_state_dict(model.state_dict())
    ref = ref.to(DEV)
    batch = make_batch(B=2, T=16, lead=3, seed=7)
    Fn.manual_seed(SEED, DEV)
    loss = model.training_step(clone_batch(batch, DEV))["loss"]
    loss.backward()
    torch.cuda.synchronize()
    assert Fn.get_rng_state(DEV)[1] > 0                  # the step did drop
    assert torch.isfinite(loss).item()
    for k, prm in model.named_parameters():
        assert prm.grad is not None and torch.isfinite(prm.grad).all(), k
    with torch.no_grad():
        y1, _ = model(*clone_batch(batch, DEV)[:-1])
        y2, _ = model(*clone_batch(batch, DEV)[:-1])
        assert not torch.equal(y1, y2)                   # two forwards, two sets of draws
        Fn.manual_seed(SEED, DEV)
        ya, _ = model(*clone_batch(batch, DEV)[:-1])
        Fn.manual_seed(SEED, DEV)
        yb, _ = model(*clone_batch(batch, DEV)[:-1])
        assert torch.equal(ya, yb)                       # the seed reproduces them bitwise
        before = Fn.get_rng_state(DEV)
        ye, _ = model.eval()(*clone_batch(batch, DEV)[:-1])
        y0, _ = ref.eval()(*clone_batch(batch, DEV)[:-1])
        assert torch.equal(ye, y0)                       # eval(): the dropout = 0 model, bitwise
        assert Fn.get_rng_state(DEV) == before


def test_graph_replay_takes_fresh_draws():
    """A captured step with Fn.dropout and a dropout-MHA forward + backward on static buffers: every replay
    draws new masks, each replay's backward uses its own forward's mask, and the state's draw advances by
    replays x draws-per-step."""
    from multimodalreactiongeneration_amd import functional as Fn
    from multimodalreactiongeneration_amd import graphs
    p, n = 0.5, 4096
    B, T, E, heads = 2, 20, 64, 4
    g = torch.Generator().manual_seed(1)
    x = (torch.rand(n, generator=g) + 0.5).to(DEV).requires_grad_(True)      # all non-zero
    q = torch.randn(B, T, E, generator=g).to(DEV).requires_grad_(True)
    kv = torch.randn(B, T, E, generator=g).to(DEV).requires_grad_(True)
    w = {k: _param(v) for k, v in _mha_weights(E, g).items()}
    do = torch.randn(B, T, E, generator=g).to(DEV)
    out = {"y": torch.zeros(n, device=DEV), "gx": torch.zeros(n, device=DEV), "o": torch.zeros(B, T, E, device=DEV),
           "gq": torch.zeros(B, T, E, device=DEV), "key": torch.zeros(2, dtype=torch.int64, device=DEV)}

    def step():
        y = Fn.dropout(x, p)
        (gx,) = torch.autograd.grad(y.sum(), x)
        out["y"].copy_(y.detach())
        out["gx"].copy_(gx)
        out["key"].copy_(Fn._rng_state(DEV))           # {seed, draw} right before the attention's draw
        o = Fn.mha(q, kv, w["in_w"], w["in_b"], w["out_w"], w["out_b"], heads, False, None, None, dropout_p=0.25)
        (gq,) = torch.autograd.grad(o, q, do)
        out["o"].copy_(o.detach())
        out["gq"].copy_(gq)

    Fn.manual_seed(SEED, DEV)
    replay = graphs.capture(step)
    draw0 = Fn.get_rng_state(DEV)[1]
    scale = float(np.float32(1.0 / (1.0 - p)))
    masks, outs = [], []
    rs = {k: v.detach().double().cpu() for k, v in w.items()}
    for i in range(3):
        replay()
        torch.cuda.synchronize()
        keep = out["y"] != 0
        assert torch.equal(out["gx"], keep.float() * scale)                  # this replay's own mask
        assert torch.equal(out["y"], torch.where(keep, x.detach() * scale, torch.zeros((), device=DEV)))
        masks.append(keep.clone())
        # the attention of this replay against float64 with the mask of the draw it took
        seed, d = out["key"].tolist()
        assert d == draw0 + 2 * i + 1
        akeep = Fn.attention_keep_mask(out["key"], B, heads, T, T, 0.25).cpu().bool()
        qr = q.detach().double().cpu().requires_grad_(True)
        orf = R.mha(qr, kv.detach().double().cpu(), rs["in_w"], rs["in_b"], rs["out_w"], rs["out_b"], heads,
                    keep=akeep, p=0.25)
        (gqr,) = torch.autograd.grad(orf, qr, do.double().cpu())
        assert rel_err(out["o"], orf) < TOL and rel_err(out["gq"], gqr) < TOL
        outs.append(out["o"].clone())
    assert not torch.equal(masks[0], masks[1]) and not torch.equal(masks[1], masks[2])
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2])
    assert Fn.get_rng_state(DEV)[1] == draw0 + 3 * 2                         # replays x draws per step


def test_generation_plan_follows_train_and_eval():
    from multimodalreactiongeneration_amd.generate import plan_for
    torch.manual_seed(0)
    plain = _tiny_metaformer(0.0, hidden=256, num_internal_layer=1, bottleneck=64).to(DEV)
    assert plan_for(plain.train()) is not None           # no dropout: the mode does not matter
    model = _tiny_metaformer(0.2, hidden=256, num_internal_layer=1, bottleneck=64).to(DEV)
    assert plan_for(model.eval()) is not None
    assert plan_for(model.train()) is None               # an MHA would drop: the module path
    assert plan_for(model.eval()) is not None
    fresh = _tiny_metaformer(0.2, hidden=256, num_internal_layer=1, bottleneck=64).to(DEV)
    assert plan_for(fresh.train()) is None               # asked first in train(): nothing stale is cached
    assert plan_for(fresh.eval()) is not None
