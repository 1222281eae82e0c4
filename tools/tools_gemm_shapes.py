"""Per-shape census of the GEMMs of one eager lstmformer training step (bench.py's workload):
every functional.gemm call is bracketed with HIP events on its launch stream (weight gradients on
the current stream, so launches are uncontended) and grouped by (M, N, K, transA, transB, splits).

    python tools/tools_gemm_shapes.py            (on a GPU box)
"""
import collections
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # repo root
from multimodalreactiongeneration_amd import configs as C  # noqa: E402
from multimodalreactiongeneration_amd import functional as Fn  # noqa: E402
from multimodalreactiongeneration_amd.model import Metaformer  # noqa: E402
from multimodalreactiongeneration_amd.synthetic import make_batch  # noqa: E402


def main():
    dev = torch.device("cuda", 0)
    mc, oc, me = C.lstmformer_config(ratio=1)
    Fn.set_wgrad_stream(False)
    torch.manual_seed(0)
    model = Metaformer(mc, oc, me).to(dev)
    opt = model.configure_optimizers()["optimizer"]
    batch = make_batch(B=64, T=300, ratio=1, seed=1234, device=dev)

    def step():
        opt.zero_grad()
        loss = model.training_step(list(batch))["loss"]
        loss.backward()
        opt.step()

    census(step)


def census(step):
    for _ in range(2):
        step()
    torch.cuda.synchronize()
    rec = []
    orig = Fn.gemm

    def timed_gemm(M, N, K, A, transA, lda, B, transB, ldb, C_, ldc, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        orig(M, N, K, A, transA, lda, B, transB, ldb, C_, ldc, **kw)
        e1.record()
        rec.append(((M, N, K, transA, transB, kw.get("splits", 1), kw.get("asum_out") is not None), e0, e1))

    # every module of the package that imported gemm by name resolves it in its own namespace
    holders = [m for n, m in list(sys.modules.items())
               if n.startswith("multimodalreactiongeneration_amd") and getattr(m, "gemm", None) is orig]
    for m in holders:
        m.gemm = timed_gemm
    step()
    torch.cuda.synchronize()
    for m in holders:
        m.gemm = orig
    agg = collections.defaultdict(lambda: [0, 0.0])
    for key, e0, e1 in rec:
        a = agg[key]
        a[0] += 1
        a[1] += e0.elapsed_time(e1)
    tot = sum(v[1] for v in agg.values())
    flop = sum(2.0 * k[0] * k[1] * k[2] * v[0] for k, v in agg.items())
    print(f"{len(rec)} gemm calls, {tot:.3f} ms, {flop / tot / 1e9:.1f} TF/s")
    print(f"{'M':>7} {'N':>6} {'K':>6} ta tb spl asum {'n':>4} {'ms':>8} {'us/call':>8} {'TF/s':>7}")
    for k, (n, ms) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
        tf = 2.0 * k[0] * k[1] * k[2] * n / ms / 1e9
        print(f"{k[0]:7d} {k[1]:6d} {k[2]:6d} {k[3]:2d} {k[4]:2d} {k[5]:3d} {int(k[6]):4d} {n:4d} {ms:8.3f} "
              f"{1e3 * ms / n:8.1f} {tf:7.1f}")


if __name__ == "__main__":
    main()
