"""bench.py's multi-GPU launch logic on the CPU (no GPU): ``--gpus N`` means N ranks.

Reference: Lightning DDP over every listed GPU (mr_gen/model/lstmformer/config.yaml:121,127).
* without torch.distributed.run, ``--gpus 2 --dry-run 1`` launches two gloo ranks that rendezvous on
  127.0.0.1, run the barrier + max-over-ranks timing and print ONE JSON line with ranks_seen = 2;
* ``--gpus 2`` on a host with fewer visible GPUs exits 2 instead of timing one GPU;
* under torch.distributed.run, a WORLD_SIZE different from --gpus exits 2 before any rendezvous.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(OMP_NUM_THREADS="2", MASTER_ADDR="127.0.0.1", **kw)
    return env


def _run(args, env, timeout=240):
    return subprocess.run([sys.executable, BENCH] + args, env=env, capture_output=True, text=True, timeout=timeout)


def test_dry_run_launches_two_gloo_ranks():
    r = _run(["--gpus", "2", "--dry-run", "1", "--steps", "2", "--warmup", "1"], _env())
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout            # rank 0 only
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 2 and out["warmup"] == 1
    assert out["ranks_seen"]["world_size"] == 2 and out["ranks_seen"]["backend"] == "gloo"
    assert sorted(r_["rank"] for r_ in out["ranks_seen"]["ranks"]) == [0, 1]
    assert out["allreduce_mean_ok"] is True
    assert out["ms_per_step"] > 0
    assert out["exchange"]["allreduce_ms"] > 0 and out["exchange"]["allreduce_bytes"] == 13_052_678 * 4


def test_dry_run_single_rank_needs_no_launcher():
    r = _run(["--dry-run", "1", "--steps", "1", "--warmup", "0"], _env())
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["n_gpus"] == 1 and out["ranks_seen"]["world_size"] == 1


def test_headline_is_the_last_line_and_small():
    """a 20.7 KB line holding the secondary block was not parsed by the driver.  The
    secondary configs print as their own lines first; the headline, with full-size synthetic kernels,
    roofline (traffic included), CPU baseline and secondary summary, is the LAST stdout line, parses,
    and fits HEADLINE_MAX_BYTES (8,000) with room to spare."""
    r = _run(["--dry-run", "1", "--steps", "1", "--warmup", "0"], _env())
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.rstrip("\n").split("\n")
    assert all(ln.startswith("{") for ln in lines), r.stdout[:500]
    *sec, last = lines
    assert len(last.encode()) <= 6000, len(last)
    out = json.loads(last)
    assert "secondary" not in out or all(isinstance(v, dict) and "ms_per_step" in v for v in out["secondary"].values())
    assert out["roofline"]["family"] == "gemm" and "traffic" in out["roofline"]
    assert out["roofline"]["frac"] > 0 and out["cpu_baseline"]["cores"] == 16
    assert len(sec) == 6 and len(out["secondary"]) == 6
    for ln in sec:
        s = json.loads(ln)
        assert s["secondary"] in out["secondary"] and "cpu_baseline" in s and "whole_step_roofline" in s


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("mrg_bench_under_test", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plain_run_is_lean_and_full_restores_every_leg():
    """Without --full the secondary configs and the CPU baselines are off whatever their own switches
    say (the probe steps key on args.full itself); --full runs them as before, each leg still
    switchable; --steps is the number of timed steps and must be at least 1."""
    import pytest
    b = _bench_module()
    a = b.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.full, a.secondary, a.cpu_baseline, a.steps, a.warmup, a.dump_outputs) == (False, 0, 0, 7, 2, None)
    a = b.parse(["--secondary", "1", "--cpu-baseline", "1"])
    assert (a.full, a.secondary, a.cpu_baseline) == (False, 0, 0)
    a = b.parse(["--full"])
    assert (a.full, a.secondary, a.cpu_baseline) == (True, 1, 1)
    a = b.parse(["--full", "--secondary", "0", "--dump-outputs", "d"])
    assert (a.full, a.secondary, a.cpu_baseline, a.dump_outputs) == (True, 0, 1, "d")
    with pytest.raises(SystemExit):
        b.parse(["--steps", "0"])


def test_write_outputs_dtypes_budget_and_fixed_sample(tmp_path, monkeypatch):
    """--dump-outputs: float32 files (float64 stays float64), every file together inside the budget, a
    tensor over its share written as the same seeded sample in every run and for every tensor of that
    size, smaller tensors whole."""
    import numpy as np
    import torch
    b = _bench_module()
    monkeypatch.setattr(b, "DUMP_MAX_BYTES", 1600)          # four files: 400 bytes of data each
    big = torch.arange(1000, dtype=torch.float32).reshape(10, 100)
    arrays = {"loss": torch.tensor(0.25), "params": big, "grads": -big.to(torch.bfloat16),
              "wide": torch.arange(1000, dtype=torch.float64)}
    for run in ("a", "b"):
        n = b.write_outputs(str(tmp_path / run), arrays)
        assert n == {"loss": 1, "params": 100, "grads": 100, "wide": 50}
    got = {k: np.load(tmp_path / "a" / (k + ".npy")) for k in arrays}
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == ["grads.npy", "loss.npy", "params.npy", "wide.npy"]
    assert {k: str(v.dtype) for k, v in got.items()} == {"loss": "float32", "params": "float32", "grads": "float32",
                                                         "wide": "float64"}
    assert sum(v.nbytes for v in got.values()) <= 1600
    idx = np.sort(np.random.RandomState(b.DUMP_SEED).choice(1000, 100, replace=False))
    assert got["loss"].tolist() == [0.25]
    assert np.array_equal(got["params"], idx.astype(np.float32))
    assert np.array_equal(got["grads"], -big.to(torch.bfloat16).float().reshape(-1).numpy()[idx])
    assert len(np.unique(got["wide"])) == 50 and np.all(np.diff(got["wide"]) > 0)
    for k in arrays:
        assert np.array_equal(got[k], np.load(tmp_path / "b" / (k + ".npy")))


def test_more_gpus_than_visible_fails_loudly():
    env = _env(HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    r = _run(["--gpus", "2", "--steps", "1"], env, timeout=120)
    assert r.returncode == 2
    assert "visible" in r.stderr and "n_gpus" not in r.stdout


def test_world_size_mismatch_fails_before_rendezvous():
    env = _env(WORLD_SIZE="3", RANK="0", LOCAL_RANK="0", MASTER_PORT="1")
    r = _run(["--gpus", "2", "--steps", "1"], env, timeout=120)
    assert r.returncode == 2
    assert "WORLD_SIZE=3" in r.stderr
