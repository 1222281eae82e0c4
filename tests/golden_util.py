"""Load committed golden fixtures (produced by tests/golden/make_golden.py from the reference)."""
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


PART_BYTES = 900_000   # no committed file over 1 MiB: a larger fixture is name.npz, name.1.npz, ...


class _Parts:
    """The arrays of a fixture stored in several .npz files, read as one (``d[key]``, ``d.files``)."""

    def __init__(self, parts):
        self._where = {k: p for p in parts for k in p.files}
        self.files = list(self._where)

    def __getitem__(self, key):
        return self._where[key][key]

    def __contains__(self, key):
        return key in self._where


def _part_path(name, i):
    return os.path.join(GOLDEN, name + (f".{i}.npz" if i else ".npz"))


def load(name):
    parts = [np.load(_part_path(name, 0), allow_pickle=False)]
    while os.path.exists(_part_path(name, len(parts))):
        parts.append(np.load(_part_path(name, len(parts)), allow_pickle=False))
    return parts[0] if len(parts) == 1 else _Parts(parts)


def save(name, arrays):
    """Write a fixture (the generators' np.savez_compressed), in key order, starting a new part
    whenever the arrays, their .npy headers and zip entries would pass PART_BYTES.  Returns the paths."""
    groups, size = [{}], 0
    for k, v in arrays.items():
        n = np.asarray(v).nbytes + 2 * len(k) + 256
        if groups[-1] and size + n > PART_BYTES:
            groups.append({})
            size = 0
        groups[-1][k] = v
        size += n
    paths = []
    for i, g in enumerate(groups):
        np.savez_compressed(_part_path(name, i), **g)
        assert os.path.getsize(_part_path(name, i)) < (1 << 20), _part_path(name, i)
        paths.append(_part_path(name, i))
    i = len(groups)
    while os.path.exists(_part_path(name, i)):   # a regenerated fixture that needs fewer parts than before
        os.remove(_part_path(name, i))
        i += 1
    return paths


def config(d):
    return json.loads(str(d["meta/config"]))


def batch_from(d, device="cpu"):
    out = []
    for i in range(7):
        out.append((torch.from_numpy(d[f"in/{i}/x"]).to(device),
                    torch.from_numpy(d[f"in/{i}/len"])))
    return out


def prefixed(d, prefix, device="cpu"):
    return {k[len(prefix):]: torch.from_numpy(d[k]).to(device) for k in d.files if k.startswith(prefix)}


def relu_flip_totals(stats):
    """(total flips, the largest flipped |z| / rms over the layers and its layer (None without a flip),
    total near) of an oracle.RELU_STATS record."""
    worst, where = 0.0, None
    for k, s in stats.items():
        r = s["max_flip"] / s["rms"] if s["max_flip"] > 0 else 0.0
        if s["flips"] and (where is None or r > worst):
            worst, where = r, k
    return sum(s["flips"] for s in stats.values()), worst, where, sum(s["near"] for s in stats.values())


def relu_flips_ok(stats, band, max_flips=32):
    """The bound on injected ReLU masks (oracle.RELU_MASKS / RELU_STATS): the masks may differ from the
    float64 oracle's own signs only where the oracle's pre-activation is within rounding of the kink,
    |z| <= band * rms(z) of its layer, and at no more than max_flips positions in all.  False for an
    empty record: a check that saw no masked layer has checked nothing."""
    if not stats:
        return False
    for s in stats.values():
        if s["max_flip"] > band * s["rms"]:
            return False
    return sum(s["flips"] for s in stats.values()) <= max_flips


def rel_err(a, b):
    a = torch.as_tensor(a).double().cpu()
    b = torch.as_tensor(b).double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-6)).item()
