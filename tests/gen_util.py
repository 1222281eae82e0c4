"""What the GPU generation tests share: the C ABI's plumbing, NaN guard zones and NaN rows around a
kernel's buffers, the seeded model / batch / mask case with the module path's prediction, and the plan run
with the persistent loop on and off."""
import functools

import numpy as np
import pytest
import torch

DEV = "cuda:0"
E = 256
GUARD = 512   # NaN floats on either side of an output
LSTM3 = ("lstm",) * 3


@pytest.fixture(scope="module", autouse=True)
def _done():
    """Import into a test module: after its last test, no asynchronous kernel error is pending."""
    yield
    from multimodalreactiongeneration_amd import functional as Fn
    torch.cuda.synchronize()
    Fn.check_errors()


def _lib():
    from multimodalreactiongeneration_amd import _lib as L
    return L.load()


def _ptr(t, off=0):
    from multimodalreactiongeneration_amd.functional import _ptr as p
    return None if t is None else p(t, off)


def _stream():
    from multimodalreactiongeneration_amd.functional import _stream as s
    return s()


def _poisoned(t):
    """t on the device, followed by one more NaN-filled row (a read past row B - 1 poisons the result)."""
    return torch.cat([t, torch.full_like(t[:1], float("nan"))]).to(DEV).contiguous()


def _guarded(n):
    """n output floats between two NaN guard zones, all NaN; the output starts at element GUARD."""
    return torch.full((2 * GUARD + n,), float("nan"), device=DEV)


def _inside(buf, *shape):
    """The output of a _guarded buffer on the host, after checking that both guard zones are still NaN."""
    n = buf.numel() - 2 * GUARD
    assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all())
    return buf[GUARD:GUARD + n].view(*shape).cpu()


def _model(**kw):
    from multimodalreactiongeneration_amd import configs as C
    from multimodalreactiongeneration_amd.model import Metaformer
    return Metaformer(*C.lstmformer_config(**kw)).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(mixers, r, B, T):
    """Model, ragged batch and scheduled-sampling mask of one case, and the module path's prediction."""
    from multimodalreactiongeneration_amd.synthetic import make_batch
    torch.manual_seed(3)
    m = _model(emb_mixers=mixers, ratio=r, num_block=2, encoder_num_layer=2).eval()
    lengths = [T] * B
    lengths[1] = T - 4
    batch = make_batch(B=B, T=T, ratio=r, lead=12, seed=5, lengths=lengths, device=DEV)
    mask = torch.from_numpy(np.random.RandomState(9).rand(T) < 0.5).to(DEV)
    with torch.enable_grad():
        slow = m._generate(batch, sampling_mask=mask).detach()
    torch.cuda.synchronize()
    return m, batch, mask, slow


def _fast_both_ways(m, batch, mask):
    """The plan's prediction with the persistent loop allowed and not, {allowed: prediction}, and how often
    each run took GenPlan._generate_loop, {allowed: count}."""
    from multimodalreactiongeneration_amd import functional as Fn
    from multimodalreactiongeneration_amd import generate as G
    plan = G.plan_for(m)
    assert plan is not None
    fast, loops = {}, {}
    inner = plan._generate_loop
    prev = G._LOOP[0]
    try:
        for loop in (True, False):
            G._LOOP[0] = loop
            calls = []
            plan._generate_loop = lambda *a, **k: (calls.append(1), inner(*a, **k))[1]
            with torch.no_grad():
                fast[loop] = m._generate(batch, sampling_mask=mask)
            loops[loop] = len(calls)
    finally:
        G._LOOP[0] = prev
        del plan._generate_loop
    torch.cuda.synchronize()
    Fn.check_errors()
    return fast, loops


def _graph_replay_is_eager(m, batch, mask0, B, T):
    """m._generate captured once as a HIP graph with the mask in a device buffer, replayed for two masks:
    each replay is the eager fast path's result for its mask, bit for bit."""
    from multimodalreactiongeneration_amd.graphs import capture
    masks = [mask0, ~mask0]
    eager = []
    with torch.no_grad():
        for mk in masks:
            eager.append(m._generate(batch, sampling_mask=mk).clone())
    assert not torch.equal(eager[0], eager[1])
    mask = torch.zeros(T, dtype=torch.bool, device=DEV)
    out = torch.zeros(B, T, 6, device=DEV)

    def gen():
        with torch.no_grad():
            out.copy_(m._generate(batch, sampling_mask=mask))
    replay = capture(gen, 1)
    for mk, want in zip(masks, eager):
        mask.copy_(mk)
        replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)
