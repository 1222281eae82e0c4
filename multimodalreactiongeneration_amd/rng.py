"""Host restatement (numpy) of the dropout RNG in csrc/rng.h: the specification the kernels are tested against.

Generator: Philox4x32-10.  An op that drops takes one *draw* from the per-device state
``{seed, draw}`` (functional.manual_seed / get_rng_state); every element's keep decision is a pure
function of (seed, draw, element index):

  Philox key         (lo32(seed), hi32(seed) ^ hi32(draw))
  flat element i     counter (lo32(i >> 2), hi32(i >> 2), 0xFFFFFFFF, lo32(draw)),  word i & 3
  attention element  (b, head, q, k), q the global query index:
                     counter (k >> 2, q, b * heads + head, lo32(draw)),             word k & 3

Keep iff word >= thr, thr = floor(p * 2^32) in double; kept values are scaled by float32(1 / (1 - p)).
"""
from __future__ import annotations

import numpy as np

DEFAULT_SEED = 67280421310721   # the state's seed until functional.manual_seed is called
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) broadcast together, key: two ints -> four uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & _LO for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]          # 32 x 32 -> 64 bits, exact in uint64
        c = [(p1 >> _S32) ^ c[1] ^ np.uint64(k0), p1 & _LO, (p0 >> _S32) ^ c[3] ^ np.uint64(k1), p0 & _LO]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return tuple(x.astype(np.uint32) for x in c)


def threshold(p) -> int:
    """thr = floor(p * 2^32) (double); p outside [0, 1) raises ValueError."""
    p = float(p)
    if not (0.0 <= p < 1.0):
        raise ValueError(f"dropout probability must be in [0, 1), got {p}")
    return int(p * 4294967296.0)


def keep_scale(p) -> np.float32:
    return np.float32(1.0 / (1.0 - float(p)))


def _key(seed, draw):
    seed, draw = int(seed) & (2 ** 64 - 1), int(draw) & (2 ** 64 - 1)
    return (seed & 0xFFFFFFFF, (seed >> 32) ^ (draw >> 32)), draw & 0xFFFFFFFF


def keep_mask(seed, draw, n, p) -> np.ndarray:
    """bool [n]: the keep decisions of functional.dropout's draw ``draw`` over n elements."""
    thr = threshold(p)
    key, dlo = _key(seed, draw)
    i4 = np.arange((int(n) + 3) // 4, dtype=np.uint64)
    w = philox4x32_10((i4 & _LO, i4 >> _S32, 0xFFFFFFFF, dlo), key)
    words = np.stack(w, axis=-1).reshape(-1)[:int(n)]
    return words >= np.uint32(thr)


def attention_keep_mask(seed, draw, B, H, Tq, Tk, p) -> np.ndarray:
    """bool [B, H, Tq, Tk]: the keep decisions of an attention op's draw on its probabilities."""
    thr = threshold(p)
    key, dlo = _key(seed, draw)
    k4 = np.arange((Tk + 3) // 4, dtype=np.uint64).reshape(1, 1, -1)
    q = np.arange(Tq, dtype=np.uint64).reshape(1, -1, 1)
    bh = np.arange(B * H, dtype=np.uint64).reshape(-1, 1, 1)
    w = philox4x32_10((k4, q, bh, dlo), key)
    words = np.stack(w, axis=-1).reshape(B * H, Tq, -1)[:, :, :Tk]
    return (words >= np.uint32(thr)).reshape(B, H, Tq, Tk)
