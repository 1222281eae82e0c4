"""CPU-only checks of the per-target MSE metrics (multimodalreactiongeneration_amd/metrics.py): the C-ABI
symbols, the keys of gen_target_dict, that no metric state reaches state_dict(), compute() / reset()
arithmetic on hand-set state, the pooled compute() of two gloo ranks, and the refusal of CPU tensors."""
import os
import re
import socket
import tempfile

import numpy as np
import pytest
import torch

from tests.model_shapes import keys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("mrg_target_metrics_update", "mrg_target_metrics_update_broadcast",
               "mrg_target_metrics_workspace_bytes")


def _cfg(**kw):
    from multimodalreactiongeneration_amd.configs import AttrDict
    return AttrDict(**kw)


def test_new_symbols_declared_exported_and_bound():
    from multimodalreactiongeneration_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mrg.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mrg_[a-z0-9_]+)\s*\(", src))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert lib.mrg_version() >= 102
    # the broadcast form's B * F counts, then one row of 8 partials per block (at most 1024 blocks)
    assert lib.mrg_target_metrics_workspace_bytes(3, 7, 18) == (3 * 18 + 2 * 8) * 4
    assert lib.mrg_target_metrics_workspace_bytes(64, 300, 18) == (64 * 18 + 1024 * 8) * 4


def test_keys_and_prefixes():
    from multimodalreactiongeneration_amd.metrics import MultiTargetMetrics
    from multimodalreactiongeneration_amd.model import gen_target_dict
    d0 = gen_target_dict(_cfg(use_centroid=True, use_angle=True, delta_order=0))
    assert MultiTargetMetrics(d0, prefix="train_").keys() == ["train_centroid", "train_angle"]
    d2 = gen_target_dict(_cfg(use_centroid=True, use_angle=True, delta_order=2))
    m = MultiTargetMetrics(d2, prefix="valid_", postfix="_mse")
    assert m.keys() == [f"valid_{n}_mse" for n in ("centroid", "angle", "delta1-centroid", "delta1-angle",
                                                    "delta2-centroid", "delta2-angle")]
    assert list(m.target_range.values()) == [(0, 3), (3, 6), (6, 9), (9, 12), (12, 15), (15, 18)]
    da = gen_target_dict(_cfg(use_centroid=False, use_angle=True, delta_order=2))
    assert da == {"angle": (0, 3), "delta1-angle": (3, 6), "delta2-angle": (6, 9)}
    assert MultiTargetMetrics(da).keys() == ["angle", "delta1-angle", "delta2-angle"]
    with pytest.raises(ValueError):
        MultiTargetMetrics({str(i): (0, 1) for i in range(9)})
    with pytest.raises(ValueError):
        MultiTargetMetrics({})


@pytest.mark.parametrize("name,builder,genrt", [("Metaformer", "lstmformer_config", True),
                                                ("LSTMwithSample", "lstm_with_sampling_config", True),
                                                ("SimpleLSTM", "simple_lstm_config", False)])
def test_models_carry_metrics_outside_the_state_dict(name, builder, genrt):
    from multimodalreactiongeneration_amd import configs as C
    from multimodalreactiongeneration_amd import model as M
    from multimodalreactiongeneration_amd.metrics import MultiTargetMetrics
    cls = getattr(M, name)
    m = cls(*getattr(C, builder)())
    assert cls.metrics_enabled is True
    off = cls(*getattr(C, builder)())
    off.metrics_enabled = False
    ref = keys(name)                        # the reference's keys = the parent commit's
    for model in (m, off):
        assert list(model.state_dict()) == list(ref)
        assert not any("metrics" in k or "_state" in k or "_batch" in k for k in model.state_dict())
    names = ["train", "valid"] + (["genrt"] if genrt else [])
    for n in names:
        mt = getattr(m, n + "_metrics")
        assert isinstance(mt, MultiTargetMetrics)
        assert mt.keys() == [f"{n}_{k}" for k in M.gen_target_dict(m.metrics)]
    assert hasattr(m, "genrt_metrics") == genrt
    # the state follows the module and a model-wide dtype cast leaves the accumulators float64
    m.train_metrics.state[0, 0] = 1.0 + 2.0 ** -40
    m.float()
    assert m.train_metrics.state.dtype == torch.float64 and m.train_metrics.state[0, 0].item() == 1.0 + 2.0 ** -40
    m.load_state_dict(off.state_dict())     # strict: no missing and no unexpected metric keys


def test_compute_on_fresh_metrics_raises():
    from multimodalreactiongeneration_amd.metrics import MultiTargetMetrics
    m = MultiTargetMetrics({"a": (0, 3), "b": (3, -1)}, prefix="train_")
    with pytest.raises(RuntimeError, match="before any update"):
        m.compute()
    with pytest.raises(RuntimeError, match="before any update"):
        dict(m.items())


def test_compute_and_reset_arithmetic_on_hand_set_state():
    from multimodalreactiongeneration_amd.metrics import MultiTargetMetrics
    m = MultiTargetMetrics({"a": (0, 3), "b": (3, -1), "all": (0, -1)}, prefix="p_", postfix="_q")
    assert m.state.shape == (3, 2) and m.state.dtype == torch.float64
    m.state.copy_(torch.tensor([[6.0, 12.0], [1.0, 8.0], [7.0, 20.0]], dtype=torch.float64))
    out = m.compute()
    assert list(out) == ["p_a_q", "p_b_q", "p_all_q"]
    for v, want in zip(out.values(), (0.5, 0.125, 0.35)):
        assert v.dim() == 0 and v.dtype == torch.float32 and v.item() == np.float32(want)
    assert dict(m.items()).keys() == out.keys()
    # sums beyond float32's integers stay exact in the float64 state
    m.state.copy_(torch.tensor([[2.0 ** 40 + 1, 1.0], [0.0, 1.0], [3.0, 2.0 ** 33]], dtype=torch.float64))
    assert m.state[0, 0].item() == 2.0 ** 40 + 1
    assert m.compute()["p_all_q"].item() == np.float32(3.0 / 2.0 ** 33)
    m.reset()
    assert torch.equal(m.state, torch.zeros(3, 2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="before any update"):
        m.compute()


def test_update_on_cpu_tensors_has_no_cpu_fallback():
    from multimodalreactiongeneration_amd.metrics import MultiTargetMetrics
    m = MultiTargetMetrics({"a": (0, 3), "b": (3, 6)})
    p, t = torch.randn(2, 5, 6), torch.randn(2, 5, 6)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.update(p, t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(p, t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.update_masked(p, t, 0, True, 0, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.update_broadcast(p, t, t, True, 0, 1.0)
    with pytest.raises(RuntimeError, match="before any update"):   # a refused update accumulated nothing
        m.compute()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker_pooled(rank, world, port, out_dir):
    torch.set_num_threads(1)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    import torch.distributed as dist
    from multimodalreactiongeneration_amd.ddp import init_from_env
    from multimodalreactiongeneration_amd.metrics import MultiTargetMetrics
    init_from_env(backend="gloo")
    m = MultiTargetMetrics({"a": (0, 3), "b": (3, 6)}, prefix="valid_")
    mine = torch.tensor([[3.0, 30.0], [1.0, 30.0]] if rank == 0 else [[9.0, 60.0], [0.5, 60.0]], dtype=torch.float64)
    m.state.copy_(mine)
    out = m.compute()
    assert torch.equal(m.state, mine)       # the all-reduce ran on a copy
    np.save(os.path.join(out_dir, f"m{rank}.npy"), np.array([out["valid_a"].item(), out["valid_b"].item()]))
    dist.destroy_process_group()


def test_two_gloo_ranks_compute_the_pooled_value():
    import torch.multiprocessing as mp
    out = tempfile.mkdtemp(prefix="mrg_metrics_")
    mp.spawn(_worker_pooled, args=(2, _free_port(), out), nprocs=2, join=True)
    v0, v1 = np.load(os.path.join(out, "m0.npy")), np.load(os.path.join(out, "m1.npy"))
    want = np.array([np.float32(12.0 / 90.0), np.float32(1.5 / 90.0)], dtype=np.float64)
    assert np.array_equal(v0, want) and np.array_equal(v1, want)
