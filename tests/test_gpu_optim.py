"""The fused optimizers on a real MI355X: mrg_sgd_step against torch.optim.SGD (every path of the launch,
the first-step branch on the device counter), inside a replayed HIP graph with an LR scheduler, under the
persistent-recurrence error flag, resumed from a state_dict, and as the optimizer of a model's training step.

Floating-point bar: max|a-b| / max|b| < 1e-6 against torch.optim.SGD in float32 on the CPU (the bar of
test_adamw_matches_oracle_over_three_steps; SGD's arithmetic is a subset of AdamW's); bitwise where the
same kernel runs on the same inputs."""
import pytest
import torch

from tests.golden_util import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from multimodalreactiongeneration_amd import _lib as L
    L.load()
    yield
    from multimodalreactiongeneration_amd import functional as Fn
    torch.cuda.synchronize()
    Fn.check_errors()


def _dev_params(p0):
    return [torch.nn.Parameter(t.clone().to(DEV)) for t in p0]


def _set_grads(params, grads):
    for p, gr in zip(params, grads):
        p.grad.copy_(gr.to(DEV))


# ragged tail (3100 = 12 * 256 + 28); less than one wavefront; past the 4096 x 256 grid cap (the stride
# loop runs twice for the first 257 threads)
@pytest.mark.parametrize("shapes", [[(300, 7), (1000,)], [(3,)], [(1_048_576 + 257,)]],
                         ids=["ragged", "sub_wave", "past_grid_cap"])
@pytest.mark.parametrize("momentum,wd", [(0.9, 1e-2), (0.9, 0.0), (0.0, 1e-2)])
def test_sgd_matches_torch_over_five_steps(shapes, momentum, wd):
    """Five steps from step 1 on.  The first step seeds the buffer with g (weight decay folded in) whatever
    it held: the buffer starts out non-zero here, so a missing first-step branch (momentum * buf + g) or one
    taken every step shows in the parameters from step 1 or 2 on."""
    from multimodalreactiongeneration_amd.optim import FusedSGD
    g = torch.Generator().manual_seed(9)
    p0 = [torch.randn(s, generator=g) for s in shapes]
    params = _dev_params(p0)
    opt = FusedSGD(params, lr=1e-2, momentum=momentum, weight_decay=wd)
    if momentum:
        opt.momentum_buf.fill_(7.0)
    ref = [torch.nn.Parameter(t.clone()) for t in p0]
    ropt = torch.optim.SGD(ref, lr=1e-2, momentum=momentum, weight_decay=wd)
    for step in range(5):
        grads = [torch.randn(t.shape, generator=g) for t in p0]
        _set_grads(params, grads)
        for r, gr in zip(ref, grads):
            r.grad = gr
        opt.step()
        ropt.step()
        for p, r in zip(params, ref):
            e = rel_err(p.detach(), r.detach())
            print(f"step {step + 1} params rel err {e:.2e}")
            assert e < 1e-6, step
    assert float(opt.step_lr[0]) == 5.0
    if momentum:
        off = 0
        for r in ref:
            e = rel_err(opt.momentum_buf[off:off + r.numel()], ropt.state[r]["momentum_buffer"].reshape(-1))
            print(f"momentum buffer rel err {e:.2e}")
            assert e < 1e-6
            off += r.numel()
    else:
        assert opt.momentum_buf is None


def test_sgd_graph_replay_follows_lr_scheduler():
    """A replayed graph holding opt.step() uses the LR CosineAnnealingLR sets between replays, takes the
    first-step branch on the device counter in the first replay only, and capture(preserve=...) leaves no
    warm-up update behind: three replays == three torch.optim.SGD steps."""
    from multimodalreactiongeneration_amd.graphs import capture
    from multimodalreactiongeneration_amd.optim import FusedSGD
    g = torch.Generator().manual_seed(4)
    p0 = [torch.randn(64, 33, generator=g), torch.randn(517, generator=g)]
    grads = [torch.randn(t.shape, generator=g) for t in p0]
    params = _dev_params(p0)
    opt = FusedSGD(params, lr=1e-2, momentum=0.9, weight_decay=1e-2)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=4)
    _set_grads(params, grads)
    replay = capture(opt.step, 2, preserve=opt.state_tensors())
    ref = [torch.nn.Parameter(t.clone()) for t in p0]
    ropt = torch.optim.SGD(ref, lr=1e-2, momentum=0.9, weight_decay=1e-2)
    rsched = torch.optim.lr_scheduler.CosineAnnealingLR(ropt, T_max=4)
    for _ in range(3):
        replay()
        for p, gr in zip(ref, grads):
            p.grad = gr.clone()
        ropt.step()
        sched.step()
        rsched.step()
    torch.cuda.synchronize()
    for p, r in zip(params, ref):
        assert rel_err(p.detach(), r.detach()) < 1e-6
    assert float(opt.step_lr[0]) == 3.0


def test_sgd_skips_the_update_under_the_error_flag_and_raises():
    """With the persistent-recurrence error flag set the kernel leaves parameters, momentum buffer and step
    count alone; the next step raises and clears the flag; a step after that trains again."""
    from multimodalreactiongeneration_amd import functional as Fn
    from multimodalreactiongeneration_amd.optim import FusedSGD
    g = torch.Generator().manual_seed(3)
    p0 = [torch.randn(40, 9, generator=g), torch.randn(77, generator=g)]
    params = _dev_params(p0)
    opt = FusedSGD(params, lr=1e-2, momentum=0.9, weight_decay=1e-2)
    _set_grads(params, [torch.randn(t.shape, generator=g) for t in p0])
    opt.step()                                            # a clean step first: a seeded buffer, count 1
    torch.cuda.synchronize()
    before = [t.clone() for t in opt.state_tensors()]
    flag = Fn._err_flag(DEV)
    try:
        flag.fill_(1)
        opt.step()
        torch.cuda.synchronize()
        for t, b in zip(opt.state_tensors(), before):     # flat, momentum_buf, step_lr: bit-identical
            assert torch.equal(t, b)
        with pytest.raises(RuntimeError, match="timed out"):
            opt.step()                                    # the next host-visible point raises
        Fn.check_errors()                                 # flag cleared by the raise above
    finally:
        flag.zero_()
    opt.step()
    torch.cuda.synchronize()
    assert not torch.equal(opt.flat, before[0])
    assert float(opt.step_lr[0]) == 2.0


@pytest.mark.parametrize("which", ["adamw", "sgd"])
def test_resume_from_state_dict_equals_continuing(which):
    """Two steps, state_dict() + the parameters, two more steps == a fresh optimizer over the saved
    parameters, load_state_dict(), the same two further steps: bitwise (same kernel, same inputs)."""
    from multimodalreactiongeneration_amd.optim import FusedAdamW, FusedSGD

    def make(ps):
        if which == "adamw":
            return FusedAdamW(ps, lr=1e-2, weight_decay=1e-2)
        return FusedSGD(ps, lr=1e-2, momentum=0.9, weight_decay=1e-2)
    g = torch.Generator().manual_seed(6)
    p0 = [torch.randn(300, 7, generator=g), torch.randn(5, generator=g), torch.randn(1000, generator=g)]
    grads = [[torch.randn(t.shape, generator=g) for t in (p0[0], p0[2])] for _ in range(4)]

    def frozen_middle(ps):
        ps[1].requires_grad_(False)                       # a frozen parameter shifts torch's indices
        return ps
    pa = frozen_middle(_dev_params(p0))
    a = make(pa)
    for gr in grads[:2]:
        _set_grads(a.plist, gr)
        a.step()
    sd = a.state_dict()
    saved = [p.detach().clone() for p in pa]
    for gr in grads[2:]:
        _set_grads(a.plist, gr)
        a.step()
    pb = frozen_middle([torch.nn.Parameter(t) for t in saved])
    b = make(pb)
    b.load_state_dict(sd)
    for gr in grads[2:]:
        _set_grads(b.plist, gr)
        b.step()
    torch.cuda.synchronize()
    assert torch.equal(a.flat, b.flat)
    assert not torch.equal(a.flat, torch.cat([saved[0].reshape(-1), saved[2]]))


def test_metaformer_trains_with_fused_sgd_eagerly_and_from_a_graph():
    """Three SGD training steps of the reduced-width Metaformer: every step's update equals torch.optim.SGD
    applied to the previous parameters with that step's flat gradient, and the same three steps replayed
    from one captured graph on an identically initialised model end bit-identical (the step count and the
    momentum buffer live on the device; stale weight planes after step 1 would break both)."""
    from multimodalreactiongeneration_amd import configs as C
    from multimodalreactiongeneration_amd import functional as Fn
    from multimodalreactiongeneration_amd.graphs import capture
    from multimodalreactiongeneration_amd.model import Metaformer
    from multimodalreactiongeneration_amd.optim import FusedSGD
    from multimodalreactiongeneration_amd.synthetic import make_batch
    mc, oc, me = C.lstmformer_config(hidden=32, num_block=2, encoder_num_layer=2, bottleneck=16, lr=1e-2)
    oc.use_optimizer, oc.momentum, oc.use_lr_sched = "sgd", 0.9, False
    torch.manual_seed(21)
    m1 = Metaformer(mc, oc, me)
    m2 = Metaformer(mc, oc, me)
    m2.load_state_dict(m1.state_dict())
    m1, m2 = m1.to(DEV), m2.to(DEV)
    batch = make_batch(B=3, T=5, lead=2, seed=7, device=DEV)

    def step_of(m, opt):
        def step():
            opt.zero_grad()
            m.training_step([(x.clone(), n) for x, n in batch])["loss"].backward()
            opt.step()
        return step
    opt1 = m1.configure_optimizers()["optimizer"]
    assert type(opt1) is FusedSGD
    ref = torch.nn.Parameter(opt1.flat.detach().cpu().clone())
    ropt = torch.optim.SGD([ref], lr=oc.lr, momentum=0.9, weight_decay=oc.weight_decay)
    step1 = step_of(m1, opt1)
    for i in range(3):
        prev = opt1.flat.detach().cpu().clone()
        step1()
        torch.cuda.synchronize()
        Fn.check_errors()
        assert float(opt1.flat_grad.abs().max()) > 0
        with torch.no_grad():
            ref.copy_(prev)                               # torch's update of THIS step from the previous parameters
        ref.grad = opt1.flat_grad.detach().cpu().clone()
        ropt.step()
        e = rel_err(opt1.flat, ref.detach())
        print(f"step {i + 1} params rel err {e:.2e}")
        assert e < 1e-6, i
        assert not torch.equal(opt1.flat.cpu(), prev)
    opt2 = m2.configure_optimizers()["optimizer"]
    replay = capture(step_of(m2, opt2), 2, preserve=opt2.state_tensors())
    for _ in range(3):
        replay()
    torch.cuda.synchronize()
    Fn.check_errors()
    assert float(opt2.step_lr[0]) == 3.0
    assert torch.equal(opt2.flat, opt1.flat)
    assert torch.equal(opt2.momentum_buf, opt1.momentum_buf)
