"""Is the split-fork wrong-gradient replay a missing dependency in the program, or
capture-specific?  B=64 lstmformer backward with one side-stream fork per weight-gradient product
(encoder_stack.SPLIT_FORKS) and no deferral, gradients compared bitwise with the same backward issued
on one stream:
  side        eager, side stream
  side_delay  eager, side stream, a 300 us busy kernel at the head of every fork (the side runs late)
  replay      graph replay
  replay_delay graph replay with the busy kernels captured

    python tools/tools_fork_race.py          (GPU box)
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multimodalreactiongeneration_amd import _lib  # noqa: E402
from multimodalreactiongeneration_amd import configs as C  # noqa: E402
from multimodalreactiongeneration_amd import encoder_stack as ES  # noqa: E402
from multimodalreactiongeneration_amd import functional as Fn  # noqa: E402
from multimodalreactiongeneration_amd import wgrad_streams as WS  # noqa: E402
from multimodalreactiongeneration_amd.graphs import capture  # noqa: E402
from multimodalreactiongeneration_amd.model import Metaformer  # noqa: E402
from multimodalreactiongeneration_amd.synthetic import make_batch  # noqa: E402

_orig_enter = WS.side.__enter__
DELAY = [0.0]


def _enter(self):
    r = _orig_enter(self)
    if self.ctx is not None and DELAY[0] > 0:
        _lib.check(_lib.load().mrg_debug_busy(1, 64, 256, DELAY[0], torch.cuda.current_stream().cuda_stream), "busy")
    return r


WS.side.__enter__ = _enter
_orig_exit = WS.side.__exit__
MAIN_DELAY = [0.0]


def _exit(self, *exc):
    on_side = self.ctx is not None
    r = _orig_exit(self, *exc)
    if on_side and MAIN_DELAY[0] > 0:   # the main stream runs late: the side stream gets ahead of it
        _lib.check(_lib.load().mrg_debug_busy(1, 64, 256, MAIN_DELAY[0], torch.cuda.current_stream().cuda_stream),
                   "busy")
    return r


WS.side.__exit__ = _exit


def grads(m, opt, batch, mode):
    def step():
        opt.zero_grad()
        m.training_step(list(batch))["loss"].backward()
    DELAY[0] = 300.0 if mode.endswith("_delay") else 0.0
    MAIN_DELAY[0] = 300.0 if mode.endswith("_maindelay") else 0.0
    Fn.set_wgrad_stream(mode != "noside")
    if mode.startswith("replay"):
        step()
        torch.cuda.synchronize()
        replay = capture(step, 1)
        opt.flat_grad.fill_(-1.0)
        replay()
    else:
        step()
    torch.cuda.synchronize()
    DELAY[0] = MAIN_DELAY[0] = 0.0
    return {k: p.grad.clone() for k, p in m.named_parameters()}


def main():
    Fn.set_wgrad_defer(False)
    for split in (True, False):
        ES.SPLIT_FORKS = split
        mc, oc, me = C.lstmformer_config(ratio=1)
        torch.manual_seed(0)
        m = Metaformer(mc, oc, me).to("cuda:0")
        opt = m.configure_optimizers()["optimizer"]
        batch = make_batch(B=64, T=300, ratio=1, seed=5, device="cuda:0")
        ref = grads(m, opt, batch, "noside")
        for mode in ("side", "side_delay", "side_maindelay", "replay", "replay_delay", "replay_maindelay"):
            g = grads(m, opt, batch, mode)
            bad = [k for k in ref if not torch.equal(g[k], ref[k])]
            print(f"split_forks={int(split)} {mode:13s}: {len(bad)} params differ from the one-stream backward",
                  flush=True)
            if bad and mode == "side_maindelay":
                for k in bad:
                    d = (g[k] - ref[k]).abs().max().item()
                    print(f"    {k}: max|diff| {d:.3e} max|ref| {ref[k].abs().max().item():.3e} "
                          f"replay all -1: {bool((g[k] == -1).all())}", flush=True)
        del m, opt
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
