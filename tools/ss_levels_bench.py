"""Scheduled-sampling training step of the lstmformer: the level schedule (ss_levels.py) beside the per-frame
loop.  Benchmark architecture, B = 64 x T = 300 frames of synthetic input, lead 12, at 1 and 8 audio frames
per prediction frame, sampling masks of rate 0.0 / 0.25 / 0.5 / 0.9 drawn from a fixed seed.

One full step (forward + loss + backward + AdamW) per path.  For every mask the two paths alternate, the
switch off first (one forward per frame, what the step was before the schedule) and then on, ROUNDS times:
the spread between two runs of one path can be read beside the difference between the paths.  Each run is
one warm-up step and STEPS timed steps on a host clock between two device synchronisations.

Usage: python tools/ss_levels_bench.py [--ratios 1,8] [--rates 0.0,0.25,0.5,0.9] [--steps 3] [--rounds 2]
       [--batch 64] [--frames 300] [--out FILE]
Prints one line per run: ratio, rate, path, levels of the plan, model forwards per step, ms per step; then per
(ratio, rate) the best run of each path and their quotient."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ratios", default="1,8")
    ap.add_argument("--rates", default="0.0,0.25,0.5,0.9")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()

    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from multimodalreactiongeneration_amd import configs as C
    from multimodalreactiongeneration_amd import functional as Fn
    from multimodalreactiongeneration_amd import ss_levels as S
    from multimodalreactiongeneration_amd.model import Metaformer
    from multimodalreactiongeneration_amd.synthetic import clone_batch, make_batch

    if not torch.cuda.is_available():
        raise SystemExit("ss_levels_bench: needs a HIP device")
    dev = torch.device("cuda", 0)
    B, T = a.batch, a.frames
    sink = open(a.out, "a") if a.out else None

    def say(line):
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    say(f"# scheduled-sampling training step, B={B} T={T} lead=12, {a.steps} timed steps per run after 1 warm-up, "
        f"{a.rounds} runs per path, {torch.cuda.get_device_name(0)}")
    for ratio in [int(r) for r in a.ratios.split(",")]:
        torch.manual_seed(0)
        model = Metaformer(*C.lstmformer_config(ratio=ratio, use_scheduled_sampling=True)).to(dev)
        opt = model.configure_optimizers()["optimizer"]
        batch = make_batch(B=B, T=T, ratio=ratio, lead=12, seed=1234, device=dev)
        calls = []
        model.metaformer.register_forward_hook(lambda *_: calls.append(1))

        def step(mask):
            opt.zero_grad()
            loss = model.training_step(clone_batch(batch), sampling_mask=mask)["loss"]
            loss.backward()
            opt.step()
            return loss

        for rate in [float(r) for r in a.rates.split(",")]:
            mask = torch.from_numpy(np.random.RandomState(a.seed).rand(T) < rate)
            levels = S.plan_levels(mask, S.rows_cap_for(model, dev), B)
            best = {}
            for _ in range(a.rounds):
                for on in (False, True):
                    model.use_level_schedule = on
                    step(mask)                       # warm-up: code objects, allocator, workspaces
                    torch.cuda.synchronize()
                    del calls[:]
                    t0 = time.perf_counter()
                    for _ in range(a.steps):
                        loss = step(mask)
                    torch.cuda.synchronize()
                    ms = (time.perf_counter() - t0) / a.steps * 1e3
                    Fn.check_errors()
                    path = "levels" if on else "frames"
                    best[path] = min(ms, best.get(path, ms))
                    say(f"ratio {ratio} rate {rate:.2f} path {path:6s} plan {len(levels):3d} levels "
                        f"(depth {levels[-1].depth + 1:3d})  forwards/step {len(calls) // a.steps:3d}  "
                        f"{ms:9.2f} ms/step  loss {loss.item():.6f}")
            say(f"ratio {ratio} rate {rate:.2f} best: frames {best['frames']:.2f} ms, levels {best['levels']:.2f} ms, "
                f"frames / levels = {best['frames'] / best['levels']:.2f}")
        del model, opt, batch
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
