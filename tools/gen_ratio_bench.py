"""lstmformer generation at r audio frames per prediction frame (default r = 8, the reference's own rates:
100 Hz audio, 12.5 predictions/s), B = 64 x T = 300 frames of synthetic input, full generation, eval, no
grad, measured as bench.py measures its ratio-1 generation line: captured once as a HIP graph after a
warm-up run, replayed REPS times, ms per 64-clip batch.  One eager run (host clock around a
synchronise) is printed beside it.

  plan    the fused plan (generate.py: 8 launches per block + 1 per frame at r > 1)
  module  the per-frame module forward, generate.plan_for patched to return None for the run
  both    (default) each of the two in a fresh child process under its own time limit; stops at the
          first child that fails.  --rounds N repeats the pair N times, interleaved (plan, module, plan,
          ...), so the spread between two runs of one path can be read beside the difference

--mixers names the embedding mixers: one name for all three modalities (lstm, the default, or gru, the
config_gru.yaml model) or three, comma separated, by modality (audio, partner motion, self motion).

Usage: python tools/gen_ratio_bench.py [--path plan|module|both] [--ratio 8] [--mixers lstm] [--frames 300]
       [--batch 64] [--reps 5] [--rounds 1] [--limit 240]
Prints one JSON line per path and round."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def measure(path, ratio, T, B, reps, mixers):
    import torch
    sys.path.insert(0, ROOT)
    from multimodalreactiongeneration_amd import configs as C
    from multimodalreactiongeneration_amd import functional as Fn
    from multimodalreactiongeneration_amd import generate as G
    from multimodalreactiongeneration_amd.graphs import capture
    from multimodalreactiongeneration_amd.model import Metaformer
    from multimodalreactiongeneration_amd.synthetic import make_batch

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    m = Metaformer(*C.lstmformer_config(ratio=ratio, emb_mixers=mixers)).to(dev).eval()
    batch = make_batch(B=B, T=T, ratio=ratio, lead=12, seed=1234, device=dev)
    mask = torch.ones(T, dtype=torch.bool, device=dev)
    planned = G.plan_for(m) is not None
    if path == "plan" and not planned:
        raise SystemExit(f"no GenPlan at ratio {ratio} for mixers {mixers}")
    if path == "module":
        G.plan_for = lambda model: None   # Metaformer._generate imports it per call
    out = [None]

    def gen():
        with torch.no_grad():
            out[0] = m._generate(batch, sampling_mask=mask)

    gen()   # warm-up: code objects, allocator, lazily made workspaces
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    gen()
    torch.cuda.synchronize()
    eager_ms = (time.perf_counter() - t0) * 1e3
    Fn.check_errors()
    checksum = float(out[0].double().abs().sum())
    replay = capture(gen, 1)
    replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        replay()
    torch.cuda.synchronize()
    graph_ms = (time.perf_counter() - t0) / reps * 1e3
    Fn.check_errors()
    print(json.dumps(dict(path=path, mixers=",".join(mixers), ratio=ratio, B=B, T=T, reps=reps, graph_ms_per_batch=round(graph_ms, 3),
                          eager_ms_per_batch=round(eager_ms, 3), us_per_frame=round(graph_ms * 1e3 / T, 2),
                          abs_sum=checksum, peak_alloc_mb=round(torch.cuda.max_memory_allocated() / 2 ** 20))),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--path", choices=("plan", "module", "both"), default="both")
    ap.add_argument("--ratio", type=int, default=8)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mixers", default="lstm", help="one mixer name, or three by modality: gru,lstm,lstm")
    ap.add_argument("--rounds", type=int, default=1, help="with --path both: interleaved repeats of the pair")
    ap.add_argument("--limit", type=int, default=240, help="seconds per child process")
    a = ap.parse_args()
    mixers = tuple(a.mixers.split(","))
    mixers = mixers * 3 if len(mixers) == 1 else mixers
    if len(mixers) != 3 or any(k not in ("lstm", "gru") for k in mixers):
        ap.error("--mixers: lstm or gru, once or three times")
    if a.path != "both":
        measure(a.path, a.ratio, a.frames, a.batch, a.reps, mixers)
        return 0
    for path in ("plan", "module") * a.rounds:
        cmd = [sys.executable, os.path.abspath(__file__), "--path", path, "--ratio", str(a.ratio), "--frames",
               str(a.frames), "--batch", str(a.batch), "--reps", str(a.reps), "--mixers", ",".join(mixers)]
        try:
            rc = subprocess.run(cmd, timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            print(f"{path}: no result within {a.limit} s", flush=True)
            return 124
        if rc != 0:
            print(f"{path}: exit status {rc}", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
