"""World-2 gloo check of gradient accumulation under data parallelism: ``ddp.GradReducer(optimizer=opt)``
issues one all-reduce per window of ``accumulate_grad_batches`` backward passes (Lightning's ``no_sync`` on
the others), and what it then averages is the window's sum.  CPU processes: the fused update itself needs a
device, so the worker stands in for ``step()`` with its host half (``_accum_begin``, which advances the
optimizer's count of the window) and zeroes the buffer where the boundary kernel would."""
import os

import numpy as np
import torch
import torch.distributed as dist

from tests.test_ddp_gloo import _init, _spawn

N, WINDOWS, ELEMS = 3, 2, 37


def _grads(rank):
    g = torch.Generator().manual_seed(50 + rank)
    return [torch.randn(ELEMS, generator=g) for _ in range(N * WINDOWS)]


def _worker(rank, world, port, out_dir):
    torch.set_num_threads(1)
    _init(rank, world, port)
    from multimodalreactiongeneration_amd.ddp import GradReducer
    from multimodalreactiongeneration_amd.optim import FusedSGD
    opt = FusedSGD([torch.nn.Parameter(torch.zeros(ELEMS))], lr=1e-2, accumulate_grad_batches=N)
    red = GradReducer(opt.flat_grad, optimizer=opt)
    calls, real = [], dist.all_reduce

    def counted(t, *a, **kw):
        calls.append(t.numel())
        return real(t, *a, **kw)
    dist.all_reduce = counted
    closed, seen = [], []
    for g in _grads(rank):
        opt.flat_grad.add_(g)                                 # a backward pass: the gradients sum
        red.allreduce()
        seen.append(len([c for c in calls if c == ELEMS]))    # (the error-flag agreement is a 1-element call)
        if opt.closes_window():
            closed.append(opt.flat_grad.clone())
            opt.flat_grad.zero_()                             # what the boundary step does on the device
        opt._accum_begin()
    dist.all_reduce = real
    assert seen == [0, 0, 1, 1, 1, 2] and red.exchanges == WINDOWS, (seen, red.exchanges)
    np.save(os.path.join(out_dir, f"closed{rank}.npy"), torch.stack(closed).numpy())
    dist.destroy_process_group()


def test_one_all_reduce_per_window_of_the_summed_gradients():
    out = _spawn(_worker)
    c0, c1 = (np.load(os.path.join(out, f"closed{r}.npy")) for r in (0, 1))
    assert np.array_equal(c0, c1), "ranks disagree after the all-reduce"
    g0, g1 = _grads(0), _grads(1)
    for w in range(WINDOWS):
        s0 = s1 = torch.zeros(ELEMS)
        for k in range(N):
            s0, s1 = s0 + g0[N * w + k], s1 + g1[N * w + k]
        want = ((s0.double() + s1.double()) / 2).numpy()     # the rank mean of the window's sums
        assert np.abs(c0[w] - want).max() <= 4e-7 * np.abs(want).max()   # two fp32 roundings: the sum, the scale
