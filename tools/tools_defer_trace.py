"""Where the deferred weight-gradient queue is issued during one eager backward of the headline
step: prints, per recurrence fork and per end-of-backward join, how many queued products it issues.

    python tools/tools_defer_trace.py         (on a GPU box)
"""
import os
import sys
import traceback

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # repo root
from multimodalreactiongeneration_amd import configs as C, gemm_ops, wgrad_streams as WS  # noqa: E402
from multimodalreactiongeneration_amd.model import Metaformer  # noqa: E402
from multimodalreactiongeneration_amd.synthetic import make_batch  # noqa: E402


def where():
    for fr in reversed(traceback.extract_stack()[:-2]):
        if ("multimodalreactiongeneration_amd" in fr.filename
                and os.path.basename(fr.filename) not in ("functional.py", "wgrad_streams.py")):
            return f"{os.path.basename(fr.filename)}:{fr.lineno} {fr.name}"
    fr = traceback.extract_stack()[-3]
    return f"{os.path.basename(fr.filename)}:{fr.lineno} {fr.name}"


def main():
    dev = torch.device("cuda", 0)
    mc, oc, me = C.lstmformer_config()
    torch.manual_seed(0)
    model = Metaformer(mc, oc, me).to(dev)
    batch = make_batch(B=64, T=300, seed=1234, device=dev)
    log = []
    orig_on_side, orig_flush, orig_bracket = gemm_ops._on_side, WS._flush_deferred, WS.beside_recurrence

    def on_side(device, rows, keep, fn, writes=None):
        log.append(f"queue  rows={rows} defer={WS._defers(device, rows)} from {where()}")
        return orig_on_side(device, rows, keep, fn, writes=writes)

    def flush(key, device, cap=0, after=None):
        n = len(WS._STATES[key].pending)
        log.append(f"FLUSH  {n} products cap={cap} beside={'yes' if after is not None else 'no'} from {where()}")
        return orig_flush(key, device, cap, after)

    def bracket(device):
        log.append(f"recurrence pending={len(WS._STATES[torch.device(device).index or 0].pending)} from {where()}")
        return orig_bracket(device)
    gemm_ops._on_side, WS._flush_deferred = on_side, flush   # every caller resolves _on_side in gemm_ops
    from multimodalreactiongeneration_amd import encoder_stack, recurrent
    for mod in (recurrent, encoder_stack):
        mod.beside_recurrence = bracket
    for it in range(2):
        log.clear()
        loss = model.training_step(list(batch))["loss"]
        loss.backward()
        torch.cuda.synchronize()
    print("\n".join(log))


if __name__ == "__main__":
    main()
