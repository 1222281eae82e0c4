"""GPU checks of the level schedule of scheduled-sampling training (multimodalreactiongeneration_amd/
ss_levels.py, csrc/ss_levels.hip): the three frame-move kernels against numpy, their autograd Functions
against index arithmetic (bitwise: they only move values), and the schedule against the per-frame path
and the CPU oracle."""
import ctypes

import numpy as np
import pytest
import torch

from tests.golden_util import rel_err
from tests.test_cpu_ss_levels import MASKS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4      # the project's bar (tests.golden_util)
T_K = 7         # frames of the kernel tests' time-major tensors
GUARD = 4       # NaN floats on either side of a destination (16 bytes: the aligned case stays aligned)


def _lib():
    from multimodalreactiongeneration_amd import _lib as L
    return L, L.load()


def _p(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + 4 * off)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _placed(values, off):
    """values on the device at `off` floats past a 16-byte aligned address, NaN sentinels around it ->
    (the flat holder, the offset of the first value in it)."""
    v = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32).reshape(-1))
    flat = torch.full((v.numel() + 2 * GUARD + off,), float("nan"))
    flat[GUARD + off:GUARD + off + v.numel()] = v
    return flat.to(DEV), GUARD + off


def _read(flat, start, shape):
    torch.cuda.synchronize()
    h = flat.cpu().numpy()
    n = int(np.prod(shape))
    assert np.isnan(h[:start]).all() and np.isnan(h[start + n:]).all(), "a sentinel was overwritten"
    return h[start:start + n].reshape(shape)


def _idx(values):
    return torch.tensor(list(values), dtype=torch.int32, device=DEV)


GATHER_IDX = {1: [4], 5: [6, 0, 3, 3, 1]}          # permuted and repeated
SCATTER_IDX = {1: [2], 5: [5, 0, 6, 2, 3]}         # distinct
PREV = {1: [1], 5: [-1, 2, -1, 0, 3]}              # into M_PREV frames; -1 reads the teacher
TEACH = {1: [3], 5: [0, 1, 5, 6, 2]}
M_PREV = 4
SHAPES = [(W, B, n) for W in (1, 3, 4, 18, 256, 260) for B in (1, 3) for n in (1, 5)]


@pytest.mark.parametrize("off", [0, 1])            # 1: a base one float past alignment, the scalar path
@pytest.mark.parametrize("W,B,n", SHAPES)
def test_frame_gather_vs_numpy(W, B, n, off):
    L, lib = _lib()
    rs = np.random.RandomState(W * 100 + B * 10 + n)
    src = rs.standard_normal((T_K, B, W)).astype(np.float32)
    s_flat, s0 = _placed(src, off)
    d_flat, d0 = _placed(np.full((n, B, W), 7.0), off)
    idx = _idx(GATHER_IDX[n])
    L.check(lib.mrg_frame_gather(n, B, W, _p(s_flat, s0), _p(idx), _p(d_flat, d0), _stream()))
    assert np.array_equal(_read(d_flat, d0, (n, B, W)), src[GATHER_IDX[n]])


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("W,B,n", SHAPES)
def test_frame_scatter_vs_numpy(W, B, n, off):
    L, lib = _lib()
    rs = np.random.RandomState(W * 100 + B * 10 + n + 1)
    src = rs.standard_normal((n, B, W)).astype(np.float32)
    before = rs.standard_normal((T_K, B, W)).astype(np.float32)
    s_flat, s0 = _placed(src, off)
    d_flat, d0 = _placed(before, off)
    idx = _idx(SCATTER_IDX[n])
    L.check(lib.mrg_frame_scatter(n, B, W, _p(s_flat, s0), _p(idx), _p(d_flat, d0), _stream()))
    want = before.copy()
    want[SCATTER_IDX[n]] = src                       # every other frame keeps what it held
    assert np.array_equal(_read(d_flat, d0, (T_K, B, W)), want)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("W,B,n", SHAPES)
def test_level_input_vs_numpy(W, B, n, off):
    L, lib = _lib()
    rs = np.random.RandomState(W * 100 + B * 10 + n + 2)
    y_prev = rs.standard_normal((M_PREV, B, W)).astype(np.float32)
    ms = rs.standard_normal((T_K, B, W)).astype(np.float32)
    prev, teach = np.array(PREV[n]), np.array(TEACH[n])
    y_flat, y0 = _placed(y_prev, off)
    m_flat, m0 = _placed(ms, off)
    want = np.where((prev >= 0)[:, None, None], y_prev[np.maximum(prev, 0)], ms[teach])
    d_flat, d0 = _placed(np.full((n, B, W), 7.0), off)
    prev_d, teach_d, none_d = _idx(prev), _idx(teach), _idx([-1] * n)   # held until the reads below
    L.check(lib.mrg_level_input(n, B, W, _p(y_flat, y0), _p(prev_d), _p(m_flat, m0), _p(teach_d), _p(d_flat, d0),
                                _stream()))
    assert np.array_equal(_read(d_flat, d0, (n, B, W)), want)
    # no ms (the gradient's form): zeros where prev < 0
    d_flat, d0 = _placed(np.full((n, B, W), 7.0), off)
    L.check(lib.mrg_level_input(n, B, W, _p(y_flat, y0), _p(prev_d), None, None, _p(d_flat, d0), _stream()))
    assert np.array_equal(_read(d_flat, d0, (n, B, W)), np.where((prev >= 0)[:, None, None], want, 0.0))
    # no y_prev (depth 0): every frame from ms
    d_flat, d0 = _placed(np.full((n, B, W), 7.0), off)
    L.check(lib.mrg_level_input(n, B, W, None, _p(none_d), _p(m_flat, m0), _p(teach_d), _p(d_flat, d0), _stream()))
    assert np.array_equal(_read(d_flat, d0, (n, B, W)), ms[teach])


def test_empty_calls_launch_nothing_and_bad_calls_are_refused():
    L, lib = _lib()
    x = torch.zeros(8, device=DEV)
    i = _idx([0])
    for fn in (lib.mrg_frame_gather, lib.mrg_frame_scatter):
        assert fn(0, 3, 4, None, None, None, _stream()) == 0
        assert fn(1, 0, 4, None, None, None, _stream()) == 0
        assert fn(-1, 1, 4, _p(x), _p(i), _p(x), _stream()) != 0
        assert fn(1, 1, 4, None, _p(i), _p(x), _stream()) != 0
    assert lib.mrg_level_input(0, 3, 4, None, None, None, None, None, _stream()) == 0
    assert lib.mrg_level_input(1, 1, 4, _p(x), _p(i), _p(x), None, _p(x), _stream()) != 0   # ms without teacher
    torch.cuda.synchronize()


@pytest.mark.parametrize("W,B", [(6, 3), (4, 1), (260, 2)])
def test_function_gradients_are_index_arithmetic(W, B):
    from multimodalreactiongeneration_amd import ss_levels as S
    g = torch.Generator().manual_seed(W + B)
    rnd = lambda *s: torch.randn(*s, generator=g).to(DEV)
    # gather: the gradient is a scatter into zeros
    idx = [5, 0, 6, 2]
    src = rnd(T_K, B, W).requires_grad_(True)
    out = S.gather(src, idx)
    assert torch.equal(out, src.detach()[idx])
    do = rnd(len(idx), B, W)
    out.backward(do)
    want = torch.zeros(T_K, B, W, device=DEV)
    want[idx] = do
    assert torch.equal(src.grad, want)
    with pytest.raises(RuntimeError, match="distinct"):
        S.gather(src, [1, 1]).sum().backward()
    with pytest.raises(IndexError):
        S.gather(src, [T_K])
    # scatter, twice into one buffer: each source takes its frames of the gradient
    a, b = rnd(3, B, W).requires_grad_(True), rnd(2, B, W).requires_grad_(True)
    buf = torch.zeros(T_K, B, W, device=DEV)
    out = S.scatter(S.scatter(buf, a, [4, 1, 6]), b, [0, 5])
    want = torch.zeros(T_K, B, W, device=DEV)
    want[[4, 1, 6]] = a.detach()
    want[[0, 5]] = b.detach()
    assert torch.equal(out, want)
    do = rnd(T_K, B, W)
    out.backward(do)
    assert torch.equal(a.grad, do[[4, 1, 6]]) and torch.equal(b.grad, do[[0, 5]])
    with pytest.raises(ValueError):
        S.scatter(buf.detach(), a.detach(), [1, 1, 2])
    with pytest.raises(IndexError):
        S.scatter(buf.detach(), a.detach(), [1, 2, T_K])
    # level input: block j of the previous level takes the gradient of its one consumer, or zero
    prev, teach = PREV[5], TEACH[5]
    y_prev = rnd(M_PREV, B, W).requires_grad_(True)
    ms = rnd(T_K, B, W)
    out = S.level_input(y_prev, prev, ms, teach)
    want = torch.stack([y_prev.detach()[p] if p >= 0 else ms[t] for p, t in zip(prev, teach)])
    assert torch.equal(out, want)
    do = rnd(len(prev), B, W)
    out.backward(do)
    want = torch.zeros(M_PREV, B, W, device=DEV)
    for i, p in enumerate(prev):
        if p >= 0:
            want[p] = do[i]
    assert torch.equal(y_prev.grad, want)
    assert torch.equal(S.level_input(None, [-1, -1], ms, [3, 0]), ms[[3, 0]])
    with pytest.raises(IndexError):
        S.level_input(y_prev, [M_PREV], ms, [0])
    with pytest.raises(ValueError):
        S.level_input(y_prev, [1, 1], ms, [0, 0])


# ------------------------------------------------------------------ the schedule
B_S, T_S, LEAD = 3, 12, 3
LENGTHS = [12, 9, 5]
SCHEDULE_MASKS = {k: v for k, v in MASKS.items() if len(v) == T_S}
SCHEDULE_MASKS["random_12"] = np.random.RandomState(7).rand(T_S) < 0.5


def _tiny(ratio=1, mixers=("lstm", "lstm", "lstm"), dropout=0.0):
    from multimodalreactiongeneration_amd import configs as C
    from multimodalreactiongeneration_amd.model import Metaformer
    mc, oc, me = C.lstmformer_config(hidden=32, num_block=1, encoder_num_layer=1, num_heads=2, bottleneck=16,
                                     ratio=ratio, emb_mixers=mixers, use_scheduled_sampling=True)
    mc["dropout"] = dropout
    torch.manual_seed(0)
    m = Metaformer(mc, oc, me)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    return m.to(DEV), sd, mc, oc


def _batch(ratio=1):
    from multimodalreactiongeneration_amd.synthetic import make_batch
    return make_batch(B=B_S, T=T_S, lead=LEAD, ratio=ratio, seed=7, lengths=LENGTHS)


def _step(m, batch, mask, levels_on, calls=None):
    """One scheduled-sampling training step's loss and gradients with the switch on or off."""
    from multimodalreactiongeneration_amd import functional as Fn
    from multimodalreactiongeneration_amd.synthetic import clone_batch
    for p in m.parameters():
        p.grad = None
    m.configure_optimizers()
    m.use_level_schedule = levels_on
    hook = m.metaformer.register_forward_hook(lambda *a: calls.append(1)) if calls is not None else None
    try:
        loss = m.training_step(clone_batch(batch, DEV), sampling_mask=mask)["loss"]
        loss.backward()
        torch.cuda.synchronize()
        Fn.check_errors()
    finally:
        del m.use_level_schedule
        if hook is not None:
            hook.remove()
    return loss.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters()}


def _compare(m, batch, mask):
    on, off = [], []
    loss1, g1 = _step(m, batch, mask, True, on)
    loss0, g0 = _step(m, batch, mask, False, off)
    err = abs(loss1.item() - loss0.item()) / abs(loss0.item())
    worst = max((rel_err(g1[k], g0[k]), k) for k in g0)
    print(f"forwards {len(on)} vs {len(off)}; loss rel err {err:.2e}; worst gradient {worst[0]:.2e} ({worst[1]})")
    assert len(off) == T_S + 1                      # T frames and the warm-up
    assert err < TOL and worst[0] < TOL, (err, worst)
    return len(on)


_MODELS = {}


def _model(key, **kw):
    if key not in _MODELS:
        _MODELS[key] = _tiny(**kw)
    return _MODELS[key]


@pytest.mark.parametrize("name", sorted(SCHEDULE_MASKS))
def test_schedule_vs_per_frame_path(name):
    from multimodalreactiongeneration_amd import ss_levels as S
    m = _model("lstm_r1")[0]
    mask = torch.from_numpy(SCHEDULE_MASKS[name])
    planned = len(S.plan_levels(mask))
    forwards = _compare(m, _batch(), mask)
    # one forward per planned level and nothing else; a plan that saves nothing keeps the loop
    assert forwards == (planned if planned < T_S else T_S + 1)


@pytest.mark.parametrize("name", sorted(SCHEDULE_MASKS))
def test_schedule_ratio_2_chunked(name):
    from multimodalreactiongeneration_amd import ss_levels as S
    m = _model("lstm_r2", ratio=2)[0]
    mask = torch.from_numpy(SCHEDULE_MASKS[name])
    S._ROWS_CAP[0] = 2 * B_S
    try:
        planned = S.plan_levels(mask, S.rows_cap_for(m, DEV), B_S)
        assert all(len(lv.frames) <= 2 for lv in planned)
        forwards = _compare(m, _batch(2), mask)
    finally:
        S._ROWS_CAP[0] = None
    assert forwards == (len(planned) if len(planned) < T_S else T_S + 1)
    if name == "none":
        assert len(planned) == T_S // 2             # the one level of 12 frames in chunks of 2


@pytest.mark.parametrize("name", sorted(SCHEDULE_MASKS))
def test_schedule_gru_mixers(name):
    m = _model("gru_r1", mixers=("gru", "gru", "gru"))[0]
    _compare(m, _batch(), torch.from_numpy(SCHEDULE_MASKS[name]))


def test_rows_cap_follows_the_recurrence_limits():
    from multimodalreactiongeneration_amd import _lib as L
    from multimodalreactiongeneration_amd import ss_levels as S
    from multimodalreactiongeneration_amd.generate import _RECURRENCE
    cus = L.cu_count(0)
    assert S.rows_cap_for(_model("lstm_r1")[0], DEV) is None
    assert S.rows_cap_for(_model("lstm_r2", ratio=2)[0], DEV) == _RECURRENCE["lstm"][1] * max(1, cus // 8)


@pytest.mark.parametrize("key,kw,ratio", [("lstm_r1", {}, 1), ("lstm_r2", dict(ratio=2), 2)])
def test_schedule_vs_oracle(key, kw, ratio):
    from multimodalreactiongeneration_amd.synthetic import clone_batch
    from oracle import mrg_oracle as O
    m, sd, mc, oc = _model(key, **kw)
    batch = _batch(ratio)
    mask = torch.from_numpy(SCHEDULE_MASKS["random_12"])
    calls = []
    loss, grads = _step(m, batch, mask, True, calls)
    assert len(calls) < T_S                         # the level path ran
    ref_loss, _, ref, _ = O.run_train_step(O.metaformer_ss_training_loss, sd, oc, mc, clone_batch(batch),
                                           sampling_mask=mask)
    err = abs(loss.item() - ref_loss.item()) / abs(ref_loss.item())
    worst = max((rel_err(grads[k], ref[k]), k) for k in ref)
    print(f"loss rel err {err:.2e}; worst gradient {worst[0]:.2e} ({worst[1]})")
    assert err < TOL and worst[0] < TOL, (err, worst)


def test_fallbacks_keep_one_forward_per_frame():
    from multimodalreactiongeneration_amd import functional as Fn
    from multimodalreactiongeneration_amd.synthetic import clone_batch
    m = _model("lstm_r1")[0]
    batch = _batch()
    some = torch.from_numpy(SCHEDULE_MASKS["random_12"])

    def forwards(model, mask, grad=True):
        calls = []
        hook = model.metaformer.register_forward_hook(lambda *a: calls.append(1))
        try:
            with torch.enable_grad() if grad else torch.no_grad():
                model._generate(clone_batch(batch, DEV), sampling_mask=mask)
            torch.cuda.synchronize()
        finally:
            hook.remove()
        return len(calls)

    assert m.use_level_schedule
    assert forwards(m, some) < T_S                                  # the level path, for contrast
    assert forwards(m, some.to(DEV)) == T_S + 1                     # a device mask
    assert forwards(m, some, grad=False) == T_S + 1                 # no grad
    assert forwards(m, torch.ones(T_S, dtype=torch.bool)) == T_S + 1   # all sampled: nothing to save
    drop = _tiny(dropout=0.2)[0]
    Fn.manual_seed(20240607, DEV)
    assert forwards(drop.train(), some) == T_S + 1                  # an MHA would drop
    assert forwards(drop.eval(), some) < T_S                        # eval(): no dropout is active
