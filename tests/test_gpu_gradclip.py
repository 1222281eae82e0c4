"""Gradient clipping on a real MI355X: mrg_grad_clip_norm against a float64 norm and against
torch.nn.utils.clip_grad_norm_, mrg_grad_clip_value against torch.clamp, inside both fused optimizers
(eager and replayed from a HIP graph) and in a model's training step.

Floating-point bars.  Norm: relative error <= 1e-5 against the float64 sum on the CPU.  Each lane adds at
most a few dozen fp32 squares at the sizes here, about 10 levels of fp32 combination follow (wave
butterfly, four waves), the rest is double; every term is positive, so nothing cancels: the worst case is
about 1.3e-6 on the sum, half of that on the norm.  Clipped buffer: tests.golden_util.rel_err < 1e-5 against
torch's clip on a float64 copy (the coefficient carries the norm's error into every element).  A step that
does not clip, value clipping and everything that runs the same kernel on the same inputs: bitwise."""
import functools
import math

import pytest
import torch

from tests.golden_util import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SWEEP = 1024 * 256 * 4          # elements one sweep of the capped grid covers (float4 per lane)
# sub-wavefront; sub-block; ragged with an n % 4 tail; past the grid cap (the stride loop runs more than
# once); past four sweeps (the four-loads-in-flight loop runs, then the remainder loop for 300 lanes)
SIZES = [1, 63, 4099, 2 * SWEEP + 5, 4 * SWEEP + 4 * 300 + 3]
# (n, offset): offset 1 is a view flat[1:] of the n-element buffer, an unaligned base (scalar path)
CASES = [(n, 0) for n in SIZES] + [(4099, 1)]
IDS = [f"n{n}" + ("_unaligned" if off else "") for n, off in CASES]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from multimodalreactiongeneration_amd import _lib as L
    L.load()
    yield
    from multimodalreactiongeneration_amd import functional as Fn
    torch.cuda.synchronize()
    Fn.check_errors()


@functools.lru_cache(maxsize=None)
def _case(n, off):
    """(gradients on the CPU, float32, the view the case clips; their float64 norm).  Computed once, shared,
    never written to."""
    g = torch.randn(n, generator=torch.Generator().manual_seed(1000 + n))[off:]
    return g, g.double().square().sum().sqrt().item()


def _on_device(g, off):
    """A device copy of g that starts `off` elements into its allocation."""
    buf = torch.empty(g.numel() + off, device=DEV)
    view = buf[off:]
    view.copy_(g)
    assert view.data_ptr() % 16 == (4 * off) % 16
    return view


def _coef(max_norm, norm):
    """torch's coefficient, in float64."""
    return min(1.0, max_norm / (norm + 1e-6))


def _torch_clipped(g, max_norm, dtype):
    p = torch.nn.Parameter(torch.zeros(g.shape, dtype=dtype))
    p.grad = g.to(dtype).clone()
    total = torch.nn.utils.clip_grad_norm_([p], max_norm, error_if_nonfinite=False)
    return p.grad, total


# ---------------------------------------------------------------- 1. norm against float64
@pytest.mark.parametrize("n,off", CASES, ids=IDS)
def test_norm_matches_float64(n, off):
    from multimodalreactiongeneration_amd import functional as Fn
    g, norm = _case(n, off)
    d = _on_device(g, off)
    st = Fn.clip_grad_norm_(d, math.inf)
    got = st.cpu()
    e = abs(float(got[0]) - norm) / norm
    print(f"n={g.numel()} off={off}: norm {float(got[0]):.9g} float64 {norm:.9g} rel err {e:.2e}")
    assert e <= 1e-5
    assert float(got[1]) == 1.0                           # max_norm = inf measures only
    assert torch.equal(d.cpu(), g)


# ---------------------------------------------------------------- 2. clipping against torch
@pytest.mark.parametrize("n,off", CASES, ids=IDS)
def test_clip_matches_torch(n, off):
    from multimodalreactiongeneration_amd import functional as Fn
    g, norm = _case(n, off)
    # a clipping step
    d = _on_device(g, off)
    st = Fn.clip_grad_norm_(d, 0.5 * norm).cpu()
    ref, _ = _torch_clipped(g, 0.5 * norm, torch.float64)
    e = rel_err(d, ref)
    print(f"n={g.numel()} off={off}: clipped rel err {e:.2e}, coef {float(st[1]):.9g}")
    assert e < 1e-5
    assert abs(float(st[0]) - norm) / norm <= 1e-5        # the norm BEFORE clipping
    assert abs(float(st[1]) - _coef(0.5 * norm, norm)) < 1e-5
    # a step that does not clip: untouched, coefficient exactly 1
    d = _on_device(g, off)
    st = Fn.clip_grad_norm_(d, 2.0 * norm).cpu()
    assert float(st[1]) == 1.0
    assert abs(float(st[0]) - norm) / norm <= 1e-5
    assert torch.equal(d.cpu(), g)


def test_all_zero_buffer():
    from multimodalreactiongeneration_amd import functional as Fn
    d = torch.zeros(4099, device=DEV)
    st = Fn.clip_grad_norm_(d, 1.0).cpu()
    assert float(st[0]) == 0.0 and float(st[1]) == 1.0
    out = d.cpu()
    assert not out.isnan().any() and not out.any()


@pytest.mark.parametrize("bad", [math.inf, math.nan], ids=["inf", "nan"])
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "unaligned"])
def test_nonfinite_element_as_torch(bad, off):
    """error_if_nonfinite=False: an inf element makes the norm inf and the coefficient 0 (finite elements
    become 0, the inf itself NaN); a NaN element makes norm and coefficient NaN and poisons everything."""
    from multimodalreactiongeneration_amd import functional as Fn
    g = _case(4099, off)[0].clone()
    g[1234] = bad
    ref, total = _torch_clipped(g, 1.0, torch.float32)
    d = _on_device(g, off)
    st = Fn.clip_grad_norm_(d, 1.0).cpu()
    out = d.cpu()
    assert torch.equal(out.isnan(), ref.isnan())
    assert torch.equal(out[~ref.isnan()], ref[~ref.isnan()])   # the finite and zero positions
    assert ref.isnan().any()
    if math.isnan(bad):
        assert ref.isnan().all() and math.isnan(float(st[0])) and math.isnan(float(st[1]))
    else:
        assert float(st[0]) == math.inf == float(total) and float(st[1]) == 0.0
        assert int(ref.isnan().sum()) == 1 and not ref[~ref.isnan()].any()


def test_clip_state_and_workspace_can_be_passed_in():
    """The optimizer's form: caller-owned clip_state and workspace, returned as given."""
    from multimodalreactiongeneration_amd import functional as Fn
    g, norm = _case(4099, 0)
    d = _on_device(g, 0)
    st = torch.full((2,), -7.0, device=DEV)
    ws = Fn.clip_grad_workspace(d.numel(), DEV)
    assert Fn.clip_grad_norm_(d, 0.5 * norm, st, ws) is st
    assert abs(float(st[0]) - norm) / norm <= 1e-5 and abs(float(st[1]) - _coef(0.5 * norm, norm)) < 1e-5


def test_refusals():
    from multimodalreactiongeneration_amd import functional as Fn
    d = torch.ones(64, device=DEV)
    for fn in (Fn.clip_grad_norm_, Fn.clip_grad_value_):
        with pytest.raises(ValueError, match="float32"):
            fn(d.double(), 1.0)
        with pytest.raises(ValueError, match="contiguous"):
            fn(d[::2], 1.0)
        for bad in (-1.0, math.nan):
            with pytest.raises(RuntimeError, match="must be >= 0"):
                fn(d, bad)
    torch.cuda.synchronize()
    assert torch.equal(d.cpu(), torch.ones(64))
    e = torch.empty(0, device=DEV)                        # n == 0 launches nothing
    Fn.clip_grad_norm_(e, 1.0)
    Fn.clip_grad_value_(e, 1.0)


# ---------------------------------------------------------------- 3. value clipping
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "unaligned"])
def test_value_clipping_is_torch_clamp_bitwise(off):
    from multimodalreactiongeneration_amd import functional as Fn
    g = _case(4099, off)[0].clone()
    g[77] = math.nan
    g[78] = math.inf
    g[79] = -math.inf
    d = _on_device(g, off)
    Fn.clip_grad_value_(d, 0.3)
    ref = torch.clamp(g, -0.3, 0.3)
    out = d.cpu()
    assert math.isnan(float(out[77])) and float(out[78]) == float(ref[78]) and float(out[79]) == float(ref[79])
    assert torch.equal(out.view(torch.int32), ref.view(torch.int32))   # bitwise, the NaN included
    assert int((ref.abs() == torch.tensor(0.3)).sum()) > 1000             # N(0, 1) data: most of it is clipped


# ---------------------------------------------------------------- 4. determinism
@pytest.mark.parametrize("n,off", [(2 * SWEEP + 5, 0), (4099, 1)], ids=["past_grid_cap", "unaligned"])
def test_two_calls_are_bitwise_equal(n, off):
    from multimodalreactiongeneration_amd import functional as Fn
    g, norm = _case(n, off)
    a, b = _on_device(g, off), _on_device(g, off)
    sa = Fn.clip_grad_norm_(a, 0.5 * norm)
    sb = Fn.clip_grad_norm_(b, 0.5 * norm)
    assert torch.equal(sa, sb) and torch.equal(a, b)
    assert not torch.equal(a.cpu(), g)


# ---------------------------------------------------------------- 5. the optimizers, eager
SHAPES = [(300, 7), (1000,), (5, 3)]                     # 3115 elements, ragged, n % 4 == 3


def _fused(which, params, **kw):
    from multimodalreactiongeneration_amd.optim import FusedAdamW, FusedSGD
    if which == "adamw":
        return FusedAdamW(params, lr=1e-2, weight_decay=1e-2, **kw)
    return FusedSGD(params, lr=1e-2, momentum=0.9, weight_decay=1e-2, **kw)


def _torch_opt(which, params):
    if which == "adamw":
        return torch.optim.AdamW(params, lr=1e-2, weight_decay=1e-2)
    return torch.optim.SGD(params, lr=1e-2, momentum=0.9, weight_decay=1e-2)


def _dev_params(p0):
    return [torch.nn.Parameter(t.clone().to(DEV)) for t in p0]


def _set_grads(params, grads):
    for p, gr in zip(params, grads):
        p.grad.copy_(gr.to(DEV))


def _norm64(grads):
    return math.sqrt(sum(float(t.double().square().sum()) for t in grads))


@pytest.mark.parametrize("algorithm", ["norm", "value"])
@pytest.mark.parametrize("which", ["adamw", "sgd"])
def test_optimizer_clips_before_the_update(which, algorithm):
    """Three steps with fresh gradients: the parameters follow torch's optimizer preceded by torch's
    clipping (1e-5: test_gpu_optim.py's 1e-6 widened by the norm's error, which the coefficient carries into
    every element), grad_norm is the float64 norm, and the same optimizer without clipping ends elsewhere."""
    g = torch.Generator().manual_seed(12)
    p0 = [torch.randn(s, generator=g) for s in SHAPES]
    steps = [[torch.randn(s, generator=g) for s in SHAPES] for _ in range(3)]
    val = 0.5 * _norm64(steps[0]) if algorithm == "norm" else 0.3
    params, plain = _dev_params(p0), _dev_params(p0)
    opt = _fused(which, params, gradient_clip_val=val, gradient_clip_algorithm=algorithm)
    off = _fused(which, plain)
    ref = [torch.nn.Parameter(t.clone()) for t in p0]
    ropt = _torch_opt(which, ref)
    for i, grads in enumerate(steps):
        _set_grads(params, grads)
        _set_grads(plain, grads)
        for r, gr in zip(ref, grads):
            r.grad = gr.clone()
        if algorithm == "norm":
            torch.nn.utils.clip_grad_norm_(ref, val)
        else:
            torch.nn.utils.clip_grad_value_(ref, val)
        opt.step()
        off.step()
        ropt.step()
        for p, r in zip(params, ref):
            e = rel_err(p.detach(), r.detach())
            print(f"{which} {algorithm} step {i + 1} params rel err {e:.2e}")
            assert e < 1e-5, i
        if algorithm == "norm":
            n64 = _norm64(grads)
            assert abs(float(opt.grad_norm) - n64) / n64 <= 1e-5
            assert abs(float(opt.grad_clip_coef) - _coef(val, n64)) < 1e-5
            assert float(opt.grad_clip_coef) < 0.6        # every step here clips
    if algorithm == "value":
        with pytest.raises(RuntimeError, match="norm clipping is off"):
            opt.grad_norm
    assert float(opt.step_lr[0]) == 3.0
    assert not torch.equal(opt.flat, off.flat)            # the feature ran


# ---------------------------------------------------------------- 6. graph replay follows the data
@pytest.mark.parametrize("which", ["adamw", "sgd"])
def test_graph_replay_clips_by_the_replayed_gradients(which):
    """One captured opt.step(); between replays flat_grad is rewritten in place with gradients of norm
    4 x, then 0.25 x max_norm.  Replay 1 clips (coefficient ~0.25), replay 2 does not (exactly 1), and the
    parameters equal an eager optimizer's on the same gradients bitwise: nothing about the norm is baked
    in at capture, and the step allocates nothing while it is recorded."""
    from multimodalreactiongeneration_amd.graphs import capture
    g = torch.Generator().manual_seed(5)
    p0 = [torch.randn(s, generator=g) for s in SHAPES]
    n = sum(t.numel() for t in p0)
    flats = []
    for scale in (4.0, 0.25):
        f = torch.randn(n, generator=g)
        flats.append((f * (scale / f.double().norm().item())).to(DEV))
    opt = _fused(which, _dev_params(p0), gradient_clip_val=1.0)
    eager = _fused(which, _dev_params(p0), gradient_clip_val=1.0)
    opt.flat_grad.copy_(flats[0])
    refused = []

    def step():
        if torch.cuda.is_current_stream_capturing():      # the setting cannot change under a capture
            try:
                opt.set_gradient_clipping(2.0)
            except RuntimeError as e:
                refused.append(str(e))
        opt.step()
    replay = capture(step, 2, preserve=opt.state_tensors())
    assert len(refused) == 1 and "inside a graph capture" in refused[0] and opt.gradient_clip_val == 1.0
    assert torch.equal(opt.flat, eager.flat)              # the warm-up left no update behind
    coefs = []
    for f in flats:
        opt.flat_grad.copy_(f)
        eager.flat_grad.copy_(f)
        replay()
        eager.step()
        torch.cuda.synchronize()
        coefs.append(float(opt.grad_clip_coef))
        assert torch.equal(opt.clip_state, eager.clip_state)
        assert torch.equal(opt.flat, eager.flat)
        assert torch.equal(opt.flat_grad, eager.flat_grad)
    print(f"{which}: replayed coefficients {coefs}")
    assert abs(coefs[0] - _coef(1.0, 4.0)) < 1e-5 and coefs[1] == 1.0
    assert torch.equal(opt.flat_grad, flats[1])           # the second replay left the gradients alone
    assert float(opt.step_lr[0]) == 2.0


# ---------------------------------------------------------------- 7. end to end
def test_metaformer_trains_with_clipping():
    """Two training steps of the reduced-width Metaformer under SGD (its update is linear in the gradient,
    so a clipped step moves the parameters half as far; AdamW's g / sqrt(v) is all but invariant under a
    common scale).  The clip value is half the first step's norm, read from a measuring-only run."""
    from multimodalreactiongeneration_amd import configs as C
    from multimodalreactiongeneration_amd import functional as Fn
    from multimodalreactiongeneration_amd.model import Metaformer
    from multimodalreactiongeneration_amd.synthetic import make_batch
    mc, oc, me = C.lstmformer_config(hidden=32, num_block=1, encoder_num_layer=1, num_heads=2, bottleneck=16)
    oc.use_optimizer, oc.momentum, oc.use_lr_sched, oc.lr = "sgd", 0.9, False, 1e-2
    batch = make_batch(B=2, T=16, lead=3, seed=7, device=DEV)
    torch.manual_seed(33)
    sd = Metaformer(mc, oc, me).state_dict()

    def model_with(**keys):
        o = oc.copy()
        o.update(keys)
        m = Metaformer(mc, o, me)
        m.load_state_dict(sd)
        m = m.to(DEV)
        return m, m.configure_optimizers()["optimizer"]

    def backward(m, opt):
        opt.zero_grad()
        loss = m.training_step([(x.clone(), n) for x, n in batch])["loss"]
        loss.backward()
        return loss.detach()

    m0, opt0 = model_with(gradient_clip_val=math.inf)     # measures only
    backward(m0, opt0)
    opt0.step()
    n0 = float(opt0.grad_norm)
    assert float(opt0.grad_clip_coef) == 1.0 and n0 > 0 and math.isfinite(n0)
    val = 0.5 * n0
    m1, opt1 = model_with(gradient_clip_val=val)
    m2, opt2 = model_with()
    assert opt2.gradient_clip_val is None and opt2.clip_state is None
    for i in range(2):
        loss = backward(m1, opt1)
        backward(m2, opt2)
        pre = float(opt1.flat_grad.double().norm())
        opt1.step()
        opt2.step()
        torch.cuda.synchronize()
        Fn.check_errors()
        assert math.isfinite(float(loss))
        post = float(opt1.flat_grad.double().norm())
        print(f"step {i + 1}: loss {float(loss):.6f} norm {pre:.6g} -> {post:.6g} (clip {val:.6g}), "
              f"grad_norm {float(opt1.grad_norm):.6g} coef {float(opt1.grad_clip_coef):.6g}")
        assert abs(float(opt1.grad_norm) - pre) / pre <= 1e-5
        assert post <= val * (1 + 1e-5)
        if i == 0:
            assert abs(pre - n0) / n0 <= 1e-5             # the same first step as the measuring run
            assert torch.equal(opt0.flat, opt2.flat)      # measuring only == clipping off, bitwise
    assert not torch.equal(opt1.flat, opt2.flat)
