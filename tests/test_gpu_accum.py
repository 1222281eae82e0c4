"""Gradient accumulation on a real MI355X: the accumulating AdamW / SGD steps, the clip launches that go
with them and the device micro-step counter, against the float64 restatement of tests/accum_ref.py.

Sizes: 1 (one thread), 3 (a partial float4), 255 / 256 / 257 (both sides of a 256-thread workgroup edge),
1027 and 4099 (several blocks, ragged tails).  One case builds the flat buffer from parameters of odd
sizes.  Bars: tests.golden_util.rel_err < 1e-4 for parameters and moments against float64, the project's
kernel-vs-float64 bar (the moments always, see _assert_matches); 1e-5 for the norm, the coefficient and the
parameters of a clipped step, the bars of test_gpu_gradclip.py (whose reasoning carries over: the partial sums are the same kernel's, the division by
n is done in double).  Everything that must not change, and an unclipped window against the plain step on
the host-averaged gradient: bitwise."""
import functools
import math

import pytest
import torch

from tests.accum_ref import AccumRef
from tests.golden_util import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [1, 3, 255, 256, 257, 1027, 4099]
ODD_SHAPES = [(3,), (5, 7), (1,)]       # slices at element offsets 0, 3, 38: the last two not 16-byte aligned
LR, WD, MOM = 1e-2, 1e-2, 0.9


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from multimodalreactiongeneration_amd import _lib as L
    L.load()
    yield
    from multimodalreactiongeneration_amd import functional as Fn
    torch.cuda.synchronize()
    Fn.check_errors()


@functools.lru_cache(maxsize=None)
def _data(n_elems, count, seed=0):
    """(initial parameters, `count` micro-batch gradients): CPU float32, computed once, never written to."""
    g = torch.Generator().manual_seed(100 * n_elems + seed)
    return torch.randn(n_elems, generator=g), tuple(torch.randn(n_elems, generator=g) for _ in range(count))


def _fused(which, params, **kw):
    from multimodalreactiongeneration_amd.optim import FusedAdamW, FusedSGD
    if which == "adamw":
        return FusedAdamW(params, lr=LR, weight_decay=WD, **kw)
    return FusedSGD(params, lr=LR, momentum=MOM, weight_decay=WD, **kw)


def _flat_opt(which, p0, **kw):
    return _fused(which, [torch.nn.Parameter(p0.clone().to(DEV))], **kw)


def _ref(which, p0, n, **kw):
    return AccumRef(which, p0, n, LR, WD, momentum=MOM, **kw)


def _moments(opt):
    if hasattr(opt, "exp_avg"):
        return {"exp_avg": opt.exp_avg, "exp_avg_sq": opt.exp_avg_sq}
    return {"momentum_buf": opt.momentum_buf}


def _micro(opt, grad):
    """What a backward pass does to the flat buffer, then the optimizer call that follows it."""
    opt.flat_grad.add_(grad.to(DEV))
    opt.step()


def _assert_matches(opt, ref, bar, what):
    """Parameters within `bar`; the moments within 1e-4 whatever the bar: the kernels form 1 - beta2 as
    1.0f - 0.999f = 9.9998712e-4, 1.29e-5 away from 1e-3 in relative terms before any gradient is seen, so
    exp_avg_sq cannot meet the 1e-5 that the parameters of a clipped step are held to."""
    e = rel_err(opt.flat, ref.p)
    print(f"{what}: params rel err {e:.2e}")
    assert e < bar, what
    for k, buf in _moments(opt).items():
        e = rel_err(buf, ref.moments()[k])
        print(f"{what}: {k} rel err {e:.2e}")
        assert e < 1e-4, (what, k)


# ---------------------------------------------------------------- 1. window parity
def _run_windows(which, n, opt, p0, grads):
    ref = _ref(which, p0, n)
    for w in range(3):
        for k in range(n):
            g = grads[w * n + k]
            _micro(opt, g)
            closed = ref.micro_step(g)
            assert closed == (k == n - 1)
        _assert_matches(opt, ref, 1e-4, f"{which} n={n} window {w + 1}")
        assert float(opt.step_lr[0]) == w + 1 == ref.steps
        assert int(opt.micro_step) == 0
        assert not opt.flat_grad.any()                       # exactly zero
        assert not torch.equal(opt.flat.cpu(), p0)           # the update ran


@pytest.mark.parametrize("n_elems", SIZES)
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("which", ["adamw", "sgd"])
def test_window_parity(which, n, n_elems):
    p0, grads = _data(n_elems, 9)
    _run_windows(which, n, _flat_opt(which, p0, accumulate_grad_batches=n), p0, grads)


@pytest.mark.parametrize("which", ["adamw", "sgd"])
def test_window_parity_odd_parameter_shapes(which):
    n_elems = sum(math.prod(s) for s in ODD_SHAPES)
    p0, grads = _data(n_elems, 9, seed=1)
    params, off = [], 0
    for s in ODD_SHAPES:
        k = math.prod(s)
        params.append(torch.nn.Parameter(p0[off:off + k].clone().view(s).to(DEV)))
        off += k
    opt = _fused(which, params, accumulate_grad_batches=3)
    assert [p.data_ptr() % 16 for p in params] == [0, 12, 8]
    _run_windows(which, 3, opt, p0, grads)
    assert torch.equal(torch.cat([p.detach().reshape(-1) for p in params]), opt.flat)   # still views


# ---------------------------------------------------------------- 2. off-boundary is inert
@pytest.mark.parametrize("n_elems", SIZES)
@pytest.mark.parametrize("which", ["adamw", "sgd"])
def test_off_boundary_calls_change_nothing_but_the_counter(which, n_elems):
    """After one whole window (so that the moments, the step count and clip_state hold something), calls
    1 .. n-1 of the next leave every state tensor and clip_state bitwise alone and flat_grad the running sum."""
    n = 4
    p0, grads = _data(n_elems, 9)
    opt = _flat_opt(which, p0, accumulate_grad_batches=n, gradient_clip_val=0.5)
    for g in grads[:n]:
        _micro(opt, g)
    assert float(opt.step_lr[0]) == 1.0 and float(opt.grad_norm) > 0
    snap = {"flat": opt.flat.clone(), "step_lr": opt.step_lr.clone(), "clip_state": opt.clip_state.clone()}
    snap.update({k: v.clone() for k, v in _moments(opt).items()})
    running = torch.zeros(n_elems, device=DEV)
    for k in range(1, n):
        g = grads[n + k].to(DEV)
        running.add_(g)
        _micro(opt, g)
        assert int(opt.micro_step) == k
        assert torch.equal(opt.flat, snap["flat"])
        assert torch.equal(opt.step_lr, snap["step_lr"])
        assert torch.equal(opt.clip_state, snap["clip_state"])
        for name, buf in _moments(opt).items():
            assert torch.equal(buf, snap[name]), name
        assert torch.equal(opt.flat_grad, running)
    _micro(opt, grads[0])                                     # the boundary: now everything moves
    assert int(opt.micro_step) == 0 and float(opt.step_lr[0]) == 2.0
    assert not torch.equal(opt.flat, snap["flat"]) and not opt.flat_grad.any()


# ---------------------------------------------------------------- 3. the unfused recipe
@pytest.mark.parametrize("n_elems", [257, 4099])
@pytest.mark.parametrize("which", ["adamw", "sgd"])
def test_equals_plain_step_on_host_averaged_gradient(which, n_elems):
    """n = 3 against n = 1 on (g1 + g2 + g3) * (1 / 3) formed on the host in fp32, in the order the device
    sums.  BITWISE holds here, not only rel_err < 1e-6: the accumulating kernel scales before anything else,
    by one rounded fp32 multiplication with 1.0f / 3 (the value torch's `* (1 / 3)` rounds to), and then runs
    the plain kernel's operations in the plain kernel's order."""
    p0, grads = _data(n_elems, 9)
    acc = _flat_opt(which, p0, accumulate_grad_batches=3)
    one = _flat_opt(which, p0)
    for w in range(3):
        g1, g2, g3 = grads[3 * w:3 * w + 3]
        for g in (g1, g2, g3):
            _micro(acc, g)
        one.flat_grad.copy_((((g1 + g2) + g3) * (1 / 3)).to(DEV))
        one.step()
        e = rel_err(acc.flat, one.flat)
        print(f"{which} n_elems={n_elems} window {w + 1}: rel err {e:.2e}, "
              f"bitwise {torch.equal(acc.flat, one.flat)}")
        assert e < 1e-6
        assert torch.equal(acc.flat, one.flat)
        for k, buf in _moments(acc).items():
            assert torch.equal(buf, _moments(one)[k]), k
        assert torch.equal(acc.step_lr, one.step_lr)


# ---------------------------------------------------------------- 4. clipping
def _mean_norm64(gs):
    return float((sum(g.double() for g in gs) / len(gs)).square().sum().sqrt())


@pytest.mark.parametrize("n_elems", [257, 4099])
@pytest.mark.parametrize("mode", ["norm_below", "norm_above", "value"])
@pytest.mark.parametrize("which", ["adamw", "sgd"])
def test_clipping_sees_the_mean_gradient(which, mode, n_elems):
    n = 2
    p0, grads = _data(n_elems, 9)
    norms = [_mean_norm64(grads[n * w:n * w + n]) for w in range(2)]
    algorithm = "value" if mode == "value" else "norm"
    val = {"norm_below": 0.5 * min(norms), "norm_above": 2.0 * max(norms), "value": 0.3}[mode]
    opt = _flat_opt(which, p0, accumulate_grad_batches=n, gradient_clip_val=val, gradient_clip_algorithm=algorithm)
    unclipped = _flat_opt(which, p0, accumulate_grad_batches=n)
    ref = _ref(which, p0, n, clip_val=val, clip_algorithm=algorithm)
    prev_state = None
    for w in range(2):
        for k in range(n):
            g = grads[n * w + k]
            _micro(opt, g)
            _micro(unclipped, g)
            ref.micro_step(g)
            if algorithm == "norm" and k < n - 1 and prev_state is not None:
                assert torch.equal(opt.clip_state, prev_state)        # the previous window's, bitwise
        _assert_matches(opt, ref, 1e-5, f"{which} {mode} window {w + 1}")
        assert float(opt.step_lr[0]) == w + 1 and not opt.flat_grad.any()
        if algorithm == "norm":
            prev_state = opt.clip_state.clone()
            got_norm, got_coef = float(opt.grad_norm), float(opt.grad_clip_coef)
            e = abs(got_norm - norms[w]) / norms[w]
            print(f"{which} {mode} window {w + 1}: norm {got_norm:.9g} float64 {norms[w]:.9g} rel err {e:.2e}, "
                  f"coef {got_coef:.9g} ref {ref.clip_coef:.9g}")
            assert e <= 1e-5
            assert abs(ref.grad_norm - norms[w]) <= 1e-12 * norms[w]
            assert abs(got_coef - ref.clip_coef) < 1e-5
            assert (got_coef == 1.0) == (mode == "norm_above")
        # a window that does not clip is the window without clipping, bitwise; one that clips is not
        assert torch.equal(opt.flat, unclipped.flat) == (mode == "norm_above")


# ---------------------------------------------------------------- 5. error flag at the boundary
@pytest.mark.parametrize("clip", [None, "norm", "value"])
@pytest.mark.parametrize("which", ["adamw", "sgd"])
def test_error_flag_at_boundary_skips_update_and_closes_window(which, clip):
    """The flag is written from the host; no kernel is made to fail.  The window after it starts clean."""
    from multimodalreactiongeneration_amd import launch
    n = 2
    p0, grads = _data(1027, 9)
    kw = {} if clip is None else dict(gradient_clip_val=0.3, gradient_clip_algorithm=clip)
    opt = _flat_opt(which, p0, accumulate_grad_batches=n, **kw)
    for g in grads[:n]:                                       # one good window first
        _micro(opt, g)
    snap = {"flat": opt.flat.clone(), "step_lr": opt.step_lr.clone()}
    snap.update({k: v.clone() for k, v in _moments(opt).items()})
    err = launch._err_flag(DEV)
    _micro(opt, grads[2])
    try:
        err.fill_(1)
        _micro(opt, grads[3])                                 # the boundary, with the flag set
        torch.cuda.synchronize()
    finally:
        err.zero_()
        torch.cuda.synchronize()
    assert torch.equal(opt.flat, snap["flat"])
    for k, buf in _moments(opt).items():
        assert torch.equal(buf, snap[k]), k
    assert torch.equal(opt.step_lr, snap["step_lr"]) and float(opt.step_lr[0]) == 1.0
    assert not opt.flat_grad.any()
    assert int(opt.micro_step) == 0


# ---------------------------------------------------------------- 6. graph replay
@pytest.mark.parametrize("clip", [None, "norm"])
@pytest.mark.parametrize("which", ["adamw", "sgd"])
def test_graph_replay_updates_on_every_nth_replay(which, clip):
    """One captured micro-step (add the gradient buffer, opt.step()) replayed 2 n times with n = 2: the
    parameters move after replays 2 and 4 only and follow the float64 reference.  A host-side `if` around
    step() would have been frozen at capture."""
    from multimodalreactiongeneration_amd.graphs import capture
    n = 2
    p0, grads = _data(4099, 9)
    val = None if clip is None else 0.5 * _mean_norm64(grads[:2])
    opt = _flat_opt(which, p0, accumulate_grad_batches=n, gradient_clip_val=val)
    ref = _ref(which, p0, n, clip_val=val)
    for g in grads[:n]:                                       # one eager warm-up window
        _micro(opt, g)
        ref.micro_step(g)
    gbuf = torch.zeros(4099, device=DEV)

    refused = []

    def micro():
        if torch.cuda.is_current_stream_capturing():          # the setting cannot change under a capture
            try:
                opt.set_accumulation(3)
            except RuntimeError as e:
                refused.append(str(e))
        opt.flat_grad.add_(gbuf)
        opt.step()
    replay = capture(micro, 2, preserve=opt.state_tensors())
    assert len(refused) == 1 and "inside a graph capture" in refused[0] and opt.accumulate_grad_batches == n
    opt.zero_grad()
    torch.cuda.synchronize()
    assert int(opt.micro_step) == 0 and float(opt.step_lr[0]) == 1.0   # the warm-up left nothing behind
    _assert_matches(opt, ref, 1e-4, f"{which} after the capture")
    before = opt.flat.clone()
    for r in range(1, 2 * n + 1):
        g = grads[n + r - 1]
        gbuf.copy_(g.to(DEV))
        replay()
        torch.cuda.synchronize()
        closed = ref.micro_step(g)
        assert closed == (r % n == 0)
        assert int(opt.micro_step) == r % n
        if closed:
            assert not torch.equal(opt.flat, before)
            _assert_matches(opt, ref, 1e-5 if clip else 1e-4, f"{which} replay {r}")
            assert not opt.flat_grad.any()
            before = opt.flat.clone()
        else:
            assert torch.equal(opt.flat, before)
            assert torch.equal(opt.flat_grad, g.to(DEV))
        assert float(opt.step_lr[0]) == 1 + r // n
    with pytest.raises(RuntimeError, match="captured into a graph"):
        opt.closes_window()                                   # the host lost count, and says so


# ---------------------------------------------------------------- 7. n = 1 is the parent
_STEP_ENTRY_POINTS = ("mrg_adamw_step", "mrg_sgd_step", "mrg_grad_clip_norm", "mrg_grad_clip_value",
                      "mrg_adamw_step_accum", "mrg_sgd_step_accum", "mrg_grad_clip_norm_accum",
                      "mrg_grad_clip_value_accum", "mrg_fill_zero")


@pytest.mark.parametrize("clip", [None, "norm", "value"])
@pytest.mark.parametrize("which", ["adamw", "sgd"])
def test_n_equal_one_is_the_plain_optimizer(which, clip, monkeypatch):
    """accumulate_grad_batches=1 against an optimizer constructed without the argument: the same library
    entry points with the same arguments (the pointers apart), none of the accumulation ones, and
    bitwise-equal parameters."""
    from multimodalreactiongeneration_amd import _lib as L
    lib = L.load()
    calls = []

    def spy(name, fn):
        def wrapped(*args):
            calls.append((name,) + tuple(a for a in args if isinstance(a, (int, float))))
            return fn(*args)
        return wrapped
    for name in _STEP_ENTRY_POINTS:
        monkeypatch.setattr(lib, name, spy(name, getattr(lib, name)), raising=False)
    p0, grads = _data(4099, 9)
    kw = {} if clip is None else dict(gradient_clip_val=0.3, gradient_clip_algorithm=clip)
    logs = []
    opts = [_flat_opt(which, p0, accumulate_grad_batches=1, **kw), _flat_opt(which, p0, **kw)]
    for opt in opts:
        assert opt.accumulate_grad_batches == 1 and opt.accum_state is None
        calls.clear()
        for g in grads[:3]:
            opt.zero_grad()
            _micro(opt, g)
        logs.append(list(calls))
    assert logs[0] == logs[1]
    names = [c[0] for c in logs[0]]
    assert not [x for x in names if x.endswith("_accum")]
    per_step = ["mrg_fill_zero"] + ([] if clip is None else [f"mrg_grad_clip_{clip}"]) + \
        ["mrg_adamw_step" if which == "adamw" else "mrg_sgd_step"]
    assert names == per_step * 3
    assert torch.equal(opts[0].flat, opts[1].flat)
    for k, buf in _moments(opts[0]).items():
        assert torch.equal(buf, _moments(opts[1])[k])
    assert not torch.equal(opts[0].flat.cpu(), p0)


# ---------------------------------------------------------------- 8. one model end to end
@pytest.mark.parametrize("use", ["adam", "sgd"])
def test_model_accumulates_two_micro_batches(use):
    """The reduced lstmformer (B = 2, T = 5, one block): training_step + backward on two different
    micro-batches with accumulate_grad_batches = 2, against one plain step on the mean of the two gradients
    taken from two separate backward passes."""
    from multimodalreactiongeneration_amd import configs as C
    from multimodalreactiongeneration_amd import functional as Fn
    from multimodalreactiongeneration_amd.model import Metaformer
    from multimodalreactiongeneration_amd.synthetic import make_batch
    mc, oc, me = C.lstmformer_config(hidden=32, num_block=1, encoder_num_layer=1, num_heads=2, bottleneck=16)
    oc.use_optimizer, oc.momentum, oc.use_lr_sched, oc.lr = use, 0.9, False, 1e-2
    batches = [make_batch(B=2, T=5, lead=3, seed=s, device=DEV) for s in (7, 8)]
    torch.manual_seed(33)
    sd = Metaformer(mc, oc, me).state_dict()

    def model_with(**keys):
        o = oc.copy()
        o.update(keys)
        m = Metaformer(mc, o, me)
        m.load_state_dict(sd)
        m = m.to(DEV)
        return m, m.configure_optimizers()["optimizer"]

    def backward(m, batch):
        m.training_step([(x.clone(), n) for x, n in batch])["loss"].backward()

    m1, acc = model_with(accumulate_grad_batches=2)
    m2, one = model_with()
    assert acc.accumulate_grad_batches == 2 and one.accumulate_grad_batches == 1
    start = acc.flat.clone()
    acc.zero_grad()
    backward(m1, batches[0])
    acc.step()
    assert torch.equal(acc.flat, start) and int(acc.micro_step) == 1
    backward(m1, batches[1])                                  # no zero_grad() inside the window
    acc.step()
    parts = []
    for b in batches:
        one.zero_grad()
        backward(m2, b)
        parts.append(one.flat_grad.clone())
    assert not torch.equal(parts[0], parts[1])
    one.flat_grad.copy_((parts[0] + parts[1]) * 0.5)
    one.step()
    torch.cuda.synchronize()
    Fn.check_errors()
    e = rel_err(acc.flat, one.flat)
    print(f"{use}: accumulated vs averaged-by-hand params rel err {e:.2e}")
    assert e < 1e-4
    assert not torch.equal(acc.flat, start)
    assert float(acc.step_lr[0]) == 1.0 and int(acc.micro_step) == 0 and not acc.flat_grad.any()
