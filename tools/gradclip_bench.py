"""Cost of gradient clipping on the flat gradient buffer of the headline model (13,052,678 elements),
measured as DESIGN.md 6e measured the optimizer updates: one process, HIP events around each call,
10 warm-up + 50 timed calls, median.

    python tools/gradclip_bench.py [n]      (on a GPU box; MRG_LIB_PATH picks the library)

Cases: the norm pass on a step that does not clip (partial + final, the scale launch returns at once:
4 B/element), the norm pass on a step that clips (12 B/element: read, read, write), value clipping
(8 B/element), and FusedAdamW.step() with clipping off (28 B/element) as the yardstick.  The gradients
are restored before every call, outside the timed interval, so every call sees the same data.
Prints one line per case and one JSON line with all of them.
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # repo root
from multimodalreactiongeneration_amd import _lib  # noqa: E402
from multimodalreactiongeneration_amd import functional as Fn  # noqa: E402
from multimodalreactiongeneration_amd.optim import FusedAdamW  # noqa: E402

WARMUP, TIMED = 10, 50


def median_us(call, before=None):
    us = []
    for i in range(WARMUP + TIMED):
        if before is not None:
            before()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        call()
        ev[1].record()
        ev[1].synchronize()
        if i >= WARMUP:
            us.append(ev[0].elapsed_time(ev[1]) * 1e3)
    return statistics.median(us), min(us), max(us)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 13_052_678
    _lib.load()
    dev = "cuda:0"
    g0 = torch.randn(n, generator=torch.Generator().manual_seed(0)).to(dev)
    norm = float(g0.double().norm())
    g = g0.clone()
    state = torch.zeros(2, device=dev)
    ws = Fn.clip_grad_workspace(n, dev)
    p = torch.nn.Parameter(torch.randn(n, generator=torch.Generator().manual_seed(1)).to(dev))
    opt = FusedAdamW([p], lr=1e-3)
    opt.flat_grad.copy_(g0)

    def restore():
        g.copy_(g0)

    cases = [("norm, not clipping", 4, lambda: Fn.clip_grad_norm_(g, 2.0 * norm, state, ws), restore),
             ("norm, clipping", 12, lambda: Fn.clip_grad_norm_(g, 0.5 * norm, state, ws), restore),
             ("value", 8, lambda: Fn.clip_grad_value_(g, 0.3), restore),
             ("FusedAdamW.step()", 28, opt.step, None)]
    out = {"n": n}
    for name, bpe, call, before in cases:
        med, lo, hi = median_us(call, before)
        if name.startswith("norm"):
            want = 1.0 if "not" in name else 0.5
            assert abs(float(state[1]) - want) < 1e-4, (name, state)
        tbs = n * bpe / (med * 1e-6) / 1e12
        out[name] = {"median_us": round(med, 2), "min_us": round(lo, 2), "max_us": round(hi, 2),
                     "bytes_per_element": bpe, "TB_per_s": round(tbs, 3)}
        print(f"{name:22s} median {med:7.1f} us (min {lo:.1f}, max {hi:.1f})  "
              f"{tbs:.2f} TB/s at {bpe} B/element", flush=True)
    torch.cuda.synchronize()
    Fn.check_errors()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
