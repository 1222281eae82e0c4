"""Cost of attention-probability dropout at the lstmformer step shape (B=64, 4 heads, D=64, Tq=Tk=300,
block-causal, padded batch as in training): forward + two-pass backward with p = 0.1
(mrg_attention_fwd_dropout / _bwd_dropout) against p = 0 on the same two-pass form
(mrg_attention_set_fused(0)) of the same library.

    python tools/attn_dropout_bench.py [repeats]      (on a GPU box; MRG_LIB_PATH picks the library)

Prints, per repeat, the µs per call of each kernel group and the dropout / plain ratios (30 calls per
timing after 3 warm-up calls, HIP events on the launch stream, as tools_attn_bench.py).
"""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # repo root
from multimodalreactiongeneration_amd import _lib  # noqa: E402
from multimodalreactiongeneration_amd import functional as Fn  # noqa: E402

B, H, T, D = 64, 4, 300, 64
E = H * D
P = 0.1


def ptr(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + 4 * off) if t is not None else None


def main():
    lib = _lib.load()
    dev = "cuda:0"
    g = torch.Generator(device="cpu").manual_seed(0)
    Q = torch.randn(B, T, E, generator=g).to(dev)
    KV = torch.randn(B, T, 2 * E, generator=g).to(dev)
    dO = torch.randn(B, T, E, generator=g).to(dev)
    lens = torch.randint(T // 2, T + 1, (B,), generator=g)
    lens[0] = T
    pad = (torch.arange(T)[None, :] >= lens[:, None]).to(torch.uint8).to(dev)
    O = torch.empty(B, T, E, device=dev)
    lse = torch.empty(B, H, T, device=dev)
    dQ = torch.empty(B, T, E, device=dev)
    dKV = torch.empty(B, T, 2 * E, device=dev)
    ws = torch.empty(B * H * T, device=dev)
    scale = ctypes.c_float(D ** -0.5)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    thr, sk = Fn._drop_consts(P)
    key = Fn._rng_draw(dev)
    head = (B, H, T, T, D, ptr(Q), T * E, E, ptr(KV), T * 2 * E, 2 * E, ptr(KV, E), T * 2 * E, 2 * E, ptr(O), T * E, E,
            ptr(lse), ptr(pad), ptr(pad), 1, scale)
    grads = (ptr(dO), T * E, E, ptr(dQ), T * E, E, ptr(dKV), T * 2 * E, 2 * E, ptr(dKV, E), T * 2 * E, 2 * E, ptr(ws))

    def run(fn, *args):
        assert fn(*args) == 0, lib.mrg_last_error()

    calls = {"fwd p=0": lambda: run(lib.mrg_attention_fwd, *head, stream),
             "bwd p=0": lambda: run(lib.mrg_attention_bwd, *head, *grads, stream),
             f"fwd p={P}": lambda: run(lib.mrg_attention_fwd_dropout, *head, thr, sk, ptr(key), stream),
             f"bwd p={P}": lambda: run(lib.mrg_attention_bwd_dropout, *head, *grads, thr, sk, ptr(key), stream)}
    prev = lib.mrg_attention_set_fused(0)   # p = 0 on the two-pass form: like with like
    try:
        for rep in range(int(sys.argv[1]) if len(sys.argv) > 1 else 3):
            us = {}
            for name, fn in calls.items():
                for _ in range(3):
                    fn()
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ev[0].record()
                for _ in range(30):
                    fn()
                ev[1].record()
                torch.cuda.synchronize()
                us[name] = ev[0].elapsed_time(ev[1]) / 30 * 1e3
            f0, b0, f1, b1 = us.values()
            print(f"repeat {rep}: " + "  ".join(f"{k} {v:.1f} us" for k, v in us.items())
                  + f"  ratio fwd {f1 / f0:.3f} bwd {b1 / b0:.3f} fwd+bwd {(f1 + b1) / (f0 + b0):.3f}", flush=True)
    finally:
        lib.mrg_attention_set_fused(prev)


if __name__ == "__main__":
    main()
