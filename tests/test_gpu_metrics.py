"""Per-target MSE metrics on the MI355X (csrc/metrics.hip, metrics.MultiTargetMetrics) against a float64 torch
restatement of the reference's SeparateMeanSquaredError (multi_modal_metrics.py:18-33):
``((p - t) ** 2)[..., s:e].sum() / numel`` on the tensors the reference's steps hand to the collection.
Bar: rel_err < 1e-4 per value."""
import math

import pytest
import torch

from tests.golden_util import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = "cuda:0"
PAD = -100.0


@pytest.fixture(scope="module", autouse=True)
def _done():
    yield
    from multimodalreactiongeneration_amd import functional as Fn
    torch.cuda.synchronize()
    Fn.check_errors()


# ---------------------------------------------------------------- the float64 restatement
def _mse64(p, t, ranges):
    """One value per (start, end): SeparateMeanSquaredError.update + MeanSquaredError.compute in float64."""
    assert p.dtype == t.dtype == torch.float64 and p.shape == t.shape
    out = []
    for s, e in ranges:
        e = p.shape[-1] if e == -1 else e
        d = ((p - t) ** 2)[..., s:e]
        out.append(d.sum() / d.numel())
    return torch.stack(out)


def _masked64(y, target, lead=0, mask_padding=True, delta_order=0, scale=1.0):
    """(y * scaler, target * scaler) of training_step (lstmformer.py:369-383) in float64."""
    y, t = y.detach().double().cpu()[:, lead:], target.detach().double().cpu()
    if mask_padding:
        m = (t != PAD).double()
        y, t = y * m, t * m
    s = torch.ones_like(y)
    s[:, :, y.shape[2] // (delta_order + 1):] = math.sqrt(scale)
    return y * s, t * s


def _bcast64(pred, target, ms, scaler=True, delta_order=0, scale=1.0):
    """The literally materialised [Tm, B, T, F] tensors of prediction + generation_step / training_step
    (lstmformer.py:434-435, 372-383, 413-421) in float64."""
    pred, target, ms = (x.detach().double().cpu() for x in (pred, target, ms))
    mask = (ms.transpose(0, 1).unsqueeze(2) != PAD).double()      # [Tm, B, 1, F]
    t = target * mask                                             # [Tm, B, T, F]
    lm = (t != PAD).double()
    p, t = pred * lm, t * lm
    if scaler:
        s = torch.ones_like(p)
        s[:, :, p.shape[2] // (delta_order + 1):] = math.sqrt(scale)
        p, t = p * s, t * s
    return p, t


def _close(got, ref):
    got = torch.stack([v.detach() for v in got.values()]) if isinstance(got, dict) else got
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape
    errs = [rel_err(g, r) for g, r in zip(got, ref)]
    assert max(errs) < TOL, (errs, got.tolist(), ref.tolist())


def _ranges(F):
    """gen_target_dict's slices for the width, plus an (0, -1) range and one that overlaps two of them."""
    from multimodalreactiongeneration_amd.configs import AttrDict
    from multimodalreactiongeneration_amd.model import gen_target_dict
    d = gen_target_dict(AttrDict(use_centroid=True, use_angle=True, delta_order=F // 6 - 1))
    assert len(d) == F // 3
    d["all"] = (0, -1)
    d["overlap"] = (2, F - 1)
    return d


def _metrics(F, **kw):
    from multimodalreactiongeneration_amd.metrics import MultiTargetMetrics
    return MultiTargetMetrics(_ranges(F), **kw).to(DEV)


def _pair(B, T, F, lead, seed):
    """y [B, lead + T, F], target [B, T, F] with about 20 % of its rows padded."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(B, lead + T, F, generator=g)
    t = torch.randn(B, T, F, generator=g)
    rows = torch.rand(B, T, generator=g) < 0.2
    rows[0, -1] = True
    t[rows] = PAD
    return y, t


# ---------------------------------------------------------------- plain form
@pytest.mark.parametrize("scale", [1.0, 4.0])
@pytest.mark.parametrize("mask_padding", [True, False])
@pytest.mark.parametrize("B,T,F,lead", [(3, 7, 18, 0), (2, 5, 6, 3), (5, 301, 18, 2)])
def test_plain_form(B, T, F, lead, mask_padding, scale):
    y, t = _pair(B, T, F, lead, seed=B * T)
    m = _metrics(F, prefix="train_")
    order = F // 6 - 1
    m.update_masked(y.to(DEV), t.to(DEV), lead, mask_padding, order, scale)
    ref = _mse64(*_masked64(y, t, lead, mask_padding, order, scale), list(_ranges(F).values()))
    out = m.compute()
    assert list(out) == ["train_" + k for k in _ranges(F)]
    assert all(v.dim() == 0 and v.dtype == torch.float32 and v.is_cuda for v in out.values())
    _close(out, ref)
    _close(m._batch, ref)
    counts = torch.tensor([B * T * ((F if e == -1 else e) - s) for s, e in _ranges(F).values()], dtype=torch.float64)
    assert torch.equal(m.state[:, 1].cpu(), counts)


def test_generic_update_any_leading_dimensions():
    g = torch.Generator().manual_seed(5)
    p, t = torch.randn(2, 3, 5, 6, generator=g), torch.randn(2, 3, 5, 6, generator=g)
    t[0, 1, 2] = PAD                                   # a plain update does not mask
    m = _metrics(6)
    m.update(p.to(DEV), t.to(DEV))
    _close(m.compute(), _mse64(p.double(), t.double(), list(_ranges(6).values())))
    with pytest.raises(RuntimeError):
        m.update(p.to(DEV), t[:1].to(DEV))


def test_accumulation_reset_and_forward():
    F, order, scale = 18, 2, 4.0
    rng = list(_ranges(F).values())
    batches = [_pair(B, T, F, lead, seed) for B, T, lead, seed in ((3, 7, 0, 1), (2, 40, 2, 2), (5, 11, 1, 3))]
    m = _metrics(F)
    rows = []
    for y, t in batches:
        lead = y.shape[1] - t.shape[1]
        m.update_masked(y.to(DEV), t.to(DEV), lead, True, order, scale)
        rows.append([x.reshape(-1, F) for x in _masked64(y, t, lead, True, order, scale)])
    _close(m.compute(), _mse64(torch.cat([r[0] for r in rows]), torch.cat([r[1] for r in rows]), rng))
    m.reset()
    assert torch.equal(m.state.cpu(), torch.zeros(len(rng), 2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="before any update"):
        m.compute()
    y, t = batches[1]
    m.update_masked(y.to(DEV), t.to(DEV), 2, True, order, scale)
    _close(m.compute(), _mse64(*rows[1], rng))
    # forward: accumulates, returns the batch alone
    p, q = torch.randn(4, 9, F, generator=torch.Generator().manual_seed(9)), batches[0][1][:, :1].expand(3, 9, F)
    p, q = p[:3].contiguous(), q.contiguous()
    before = m.state.clone()
    got = m(p.to(DEV), q.to(DEV))
    assert list(got) == m.keys()
    _close(got, _mse64(p.double(), q.double(), rng))
    assert torch.equal(m.state[:, 1], before[:, 1] + torch.tensor(
        [3 * 9 * ((F if e == -1 else e) - s) for s, e in rng], dtype=torch.float64, device=DEV))
    both = (torch.cat([rows[1][0], p.double().reshape(-1, F)]), torch.cat([rows[1][1], q.double().reshape(-1, F)]))
    _close(m.compute(), _mse64(*both, rng))


def test_identical_runs_leave_bitwise_equal_state():
    F = 18
    batches = [_pair(B, T, F, lead, seed) for B, T, lead, seed in ((3, 7, 0, 1), (5, 301, 2, 2), (2, 40, 1, 3))]
    dev = [(y.to(DEV), t.to(DEV)) for y, t in batches]
    m = _metrics(F)
    states = []
    for _ in range(2):
        m.reset()
        for y, t in dev:
            m.update_masked(y, t, y.shape[1] - t.shape[1], True, 2, 4.0)
        states.append(m.state.clone())
    assert (states[0][:, 0] > 0).all()
    assert torch.equal(states[0].view(torch.int64), states[1].view(torch.int64))


# ---------------------------------------------------------------- broadcast form
@pytest.mark.parametrize("scaler", [True, False])
@pytest.mark.parametrize("B,T,Tm,F", [(2, 9, 9, 18), (3, 12, 12, 6)])
def test_broadcast_form(B, T, Tm, F, scaler):
    g = torch.Generator().manual_seed(T)
    pred, target, ms = (torch.randn(B, n, F, generator=g) for n in (T, T, Tm))
    for b in range(B):                                 # ragged padding, different in the two tensors
        ms[b, Tm - 1 - 2 * b:] = PAD
        target[b, T - 2 - b:] = PAD
    ms[0, 1, 2] = PAD                                  # counts are per (b, f)
    ms[B - 1, 0, F - 1] = PAD
    order, scale = F // 6 - 1, 4.0
    m = _metrics(F, prefix="genrt_")
    m.update_broadcast(pred.to(DEV), target.to(DEV), ms.to(DEV), scaler, order, scale)
    ref = _mse64(*_bcast64(pred, target, ms, scaler, order, scale), list(_ranges(F).values()))
    _close(m.compute(), ref)
    counts = torch.tensor([Tm * B * T * ((F if e == -1 else e) - s) for s, e in _ranges(F).values()],
                          dtype=torch.float64)
    assert torch.equal(m.state[:, 1].cpu(), counts)


# ---------------------------------------------------------------- models
def _tiny(name, **kw):
    from multimodalreactiongeneration_amd import configs as C
    from multimodalreactiongeneration_amd import model as M
    if name == "Metaformer":
        mc, oc, me = C.lstmformer_config(hidden=32, num_block=1, encoder_num_layer=1, num_heads=2, bottleneck=16,
                                         delta_order=1, delta_loss_scale=4.0, **kw)
    elif name == "LSTMwithSample":
        mc, oc, me = C.lstm_with_sampling_config(hidden=32, sampler_hidden=16, bottleneck=16, delta_order=1, **kw)
        mc["delta_loss_scale"] = 4.0
    else:
        mc, oc, me = C.simple_lstm_config(hidden=32, lstm=16, bottleneck=8, att_heads=4, att_layers=2, enc_layers=2,
                                          dec_layers=2, mapping=8)
        mc["delta_loss_scale"] = 4.0
    torch.manual_seed(3)
    return getattr(M, name)(mc, oc, me)


def _batch(name):
    from multimodalreactiongeneration_amd.synthetic import make_batch, make_simple_batch
    if name == "SimpleLSTM":
        return make_simple_batch(B=3, T=9, seed=4, device=DEV)
    return make_batch(B=3, T=10, lead=2, feat_audio=80, feat_motion=12, seed=4, lengths=[10, 7, 4], device=DEV)


def _copy(name, batch):
    from multimodalreactiongeneration_amd.synthetic import clone_batch
    return tuple(x.clone() for x in batch) if name == "SimpleLSTM" else clone_batch(batch, DEV)


def _vals(m, p, t):
    return _mse64(p, t, list(m.target_dict.values()))


def test_metaformer_steps_update_the_metrics():
    m = _tiny("Metaformer").to(DEV)
    batch = _batch("Metaformer")
    lead, target, ms = 2, batch[-1][0], batch[2][0]
    assert m.train_metrics.keys() == ["train_centroid", "train_angle", "train_delta1-centroid", "train_delta1-angle"]
    m.training_step(_copy("Metaformer", batch))
    b2 = _copy("Metaformer", batch)
    b2[2] = (ms * (ms != PAD).float(), b2[2][1])
    with torch.no_grad():
        y, _ = m.forward(*b2[:-1])
    _close(m.train_metrics.compute(), _vals(m, *_masked64(y, target, lead, True, 1, 4.0)))
    with torch.no_grad():
        m.validation_step(_copy("Metaformer", batch))
        y, _ = m.forward(*_copy("Metaformer", batch)[:-1])
        pred = m._generate(_copy("Metaformer", batch))
    assert m.valid_metrics.keys()[0] == "valid_centroid" and m.genrt_metrics.keys()[0] == "genrt_centroid"
    _close(m.valid_metrics.compute(), _vals(m, *_masked64(y, target, lead, True)))
    _close(m.genrt_metrics.compute(), _vals(m, *_bcast64(pred, target, ms, scaler=False)))


def test_metaformer_scheduled_sampling_step_uses_the_broadcast_form():
    m = _tiny("Metaformer", use_scheduled_sampling=True).to(DEV)
    batch = _batch("Metaformer")
    mask = torch.tensor([i % 3 == 0 for i in range(10)])
    m.training_step(_copy("Metaformer", batch), sampling_mask=mask)
    pred = m._generate(_copy("Metaformer", batch), True, False, mask).detach()
    _close(m.train_metrics.compute(), _vals(m, *_bcast64(pred, batch[-1][0], batch[2][0], True, 1, 4.0)))


def test_lstm_with_sample_steps_update_the_metrics():
    m = _tiny("LSTMwithSample").to(DEV)
    batch = _batch("LSTMwithSample")
    target = batch[-1][0]
    m.training_step(_copy("LSTMwithSample", batch))
    with torch.no_grad():
        y, (lead, _, _), _ = m.forward(*_copy("LSTMwithSample", batch)[:-1])
    assert lead == 2
    _close(m.train_metrics.compute(), _vals(m, *_masked64(y, target, lead, True, 1, 4.0)))
    with torch.no_grad():
        m.validation_step(_copy("LSTMwithSample", batch))
        pred, tgt = m.prediction(_copy("LSTMwithSample", batch))
    _close(m.valid_metrics.compute(), _vals(m, *_masked64(y, target, lead, True)))
    _close(m.genrt_metrics.compute(), _vals(m, *_masked64(pred, tgt, 0, True)))


def test_simple_lstm_steps_update_the_metrics():
    m = _tiny("SimpleLSTM").to(DEV)
    a, mo, t = _batch("SimpleLSTM")
    assert not hasattr(m, "genrt_metrics")
    m.training_step((a, mo, t))
    with torch.no_grad():
        m.validation_step((a, mo, t))
        y = m.split_and_form(mo, m.forward(a, mo))
    # SimpleLSTM never masks (simple_lstm.py:246-253); delta_order 0: the scaler starts past the last feature
    _close(m.train_metrics.compute(), _vals(m, *_masked64(y, t, 0, False, 0, 4.0)))
    _close(m.valid_metrics.compute(), _vals(m, *_masked64(y, t, 0, False)))


@pytest.mark.parametrize("name", ["Metaformer", "LSTMwithSample", "SimpleLSTM"])
def test_metrics_do_not_touch_loss_or_gradients(name):
    on, off = _tiny(name), _tiny(name)
    off.load_state_dict(on.state_dict())
    on, off = on.to(DEV), off.to(DEV)
    off.metrics_enabled = False
    batch = _batch(name)
    out = []
    for m in (on, off):
        loss = m.training_step(_copy(name, batch))["loss"]
        loss.backward()
        with torch.no_grad():
            m.validation_step(_copy(name, batch))
        out.append(loss.detach())
    torch.cuda.synchronize()
    assert torch.equal(out[0], out[1])
    for (k, p), (_, q) in zip(on.named_parameters(), off.named_parameters()):
        assert p.grad is not None and torch.equal(p.grad, q.grad), k
    assert (on.train_metrics.state[:, 1] > 0).all() and (on.valid_metrics.state[:, 1] > 0).all()
    for mt in (off.train_metrics, off.valid_metrics):      # off: no update at all
        assert torch.equal(mt.state.cpu(), torch.zeros_like(mt.state.cpu()))
        with pytest.raises(RuntimeError, match="before any update"):
            mt.compute()


def test_graph_replay_keeps_accumulating():
    from multimodalreactiongeneration_amd import graphs
    m = _tiny("Metaformer").to(DEV)
    batch = _batch("Metaformer")
    opt = m.configure_optimizers()["optimizer"]

    def step():
        opt.zero_grad()
        m.training_step(batch)["loss"].backward()

    step()
    single = torch.stack(list(m.train_metrics.compute().values())).clone()
    one = m.train_metrics.state.clone()
    replay = graphs.capture(step, 1)
    m.train_metrics.reset()
    for _ in range(3):
        replay()
    torch.cuda.synchronize()
    _close(m.train_metrics.compute(), single)
    assert torch.equal(m.train_metrics.state[:, 1], 3 * one[:, 1])
    # and the replayed value is the float64 one of the model's own output
    b2 = _copy("Metaformer", batch)
    ms = batch[2][0]
    b2[2] = (ms * (ms != PAD).float(), b2[2][1])
    with torch.no_grad():
        y, _ = m.forward(*b2[:-1])
    _close(m.train_metrics.compute(), _vals(m, *_masked64(y, batch[-1][0], 2, True, 1, 4.0)))
