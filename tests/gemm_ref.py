"""Float64 reference, componentwise error bound and memory-guard checks for the GEMM route tests.

CPU only (numpy): tests/test_gpu_gemm_routes.py uploads what this module builds and hands back what
the kernels wrote; tests/test_cpu_gemm_ref.py checks the checker itself.

The operation (csrc/gemm.hip):

    C[m, n] = epi( alpha * sum_k op(A)(m, k) op(B)(k, n) + beta * C0[m, n] + bias[n] )

Error model.  u = 2^-24 is the fp32 unit roundoff.  With S = |alpha| sum_k |a_mk b_kn| + |beta C0| +
|bias| (+ |aux| for the residual epilogue 3), the value v the epilogue receives satisfies

    |v - v_exact| <= c(K, arith) * S

where c is derived from the arithmetic include/mrg.h documents, never from kernel output:

* "f32" (exact mode, and the few-row kernel in every mode): a K-term fmaf chain, one rounding per
  term: K u.
* "x6" (three bf16 planes per operand, six plane products): each operand is reproduced by its planes
  to 2^-24 |v| (2 u for the pair), the three dropped plane products and residual cross terms are
  <= 2^-22 |a b| per product (4 u), and each of the six plane products of each k index is one more term
  added to the fp32 accumulator, 6 K roundings in the worst case (the "K terms" of mrg.h, counted once
  per plane product): (6 K + 6) u.
* "bf16" (one plane): both operands rounded to 8 significant bits (RNE, 2^-9 each), so
  (1 + 2^-9)^2 - 1 = 2^-8 + 2^-18 per product, plus the K-term fp32 accumulation: 2^-8 + 2^-18 + K u.

To each c, E = 24 roundings are added for what follows the k loop: at most 7 slab additions per
z-group and 7 group additions in the split-K reduce (or 3 partial-block additions in the few-row
kernel), the alpha product, the beta product and its addition, the bias and aux additions (5), and
the second-order terms of (1 + u)^n - 1 for n < 2^14 (under 1 %).  E is a count of operations in the
source, not a fitted figure.

Epilogues (csrc/gemm_common.h), pushed through their Lipschitz factor L and the evaluation error of
the device's own function (sigmoid = rcp(1 + exp(-x)) on 1-ulp v_exp_f32 / v_rcp_f32: argument
rounding |x| u, exp 1 ulp, the addition, rcp 1 ulp: <= 8 u absolute for |x| <= 16; tanh = 2 sigmoid(2x)
- 1: <= 17 u, taken as 2^-20):

    0 none, 3 add aux      L = 1
    1 ReLU                 L = 1 (|max(x,0) - max(y,0)| <= |x - y|: no kink to skip)
    2 v * (aux > 0)        L = 1; aux is an INPUT, so the mask is the same on both sides: no kink
    4 tanh(v)              L = 1, + 2^-20
    5 v * (1 - x^2)        L = |1 - x^2|, + |v| 4 u (1 + x^2)
    6 v * sigmoid(v)       L = 1.1 (max |silu'|), + |v| (8 u + 2 u); aux receives v itself
    7 v * silu'(x)         L = 1.1, + |v| (8 u (1 + 2|x|) + 4 u (1 + |x|))

and finally one fp32 rounding of the result, ulp32(ref).  Because ReLU and the aux mask are
1-Lipschitz in v with an exactly known mask, no element ever has to be skipped; the checker still
counts skips (always 0 here) and enforces the 0.5 % cap so that a later kinked epilogue cannot widen
it silently.
"""
from __future__ import annotations

import ctypes
import dataclasses

import numpy as np

U = 2.0 ** -24
E_TAIL = 24
SENTINEL = np.int32(-0x35014542)      # 0xCAFEBABE: a finite, large negative fp32 (-8.3e6)
SKIP_CAP = 0.005
EPS_SIGMOID = 8 * U
EPS_TANH = 2.0 ** -20


def c_bound(K: int, arith: str) -> float:
    """c(K, arith) of the module docstring."""
    if arith == "f32":
        return (K + E_TAIL) * U
    if arith == "x6":
        return (6 * K + 6 + E_TAIL) * U
    if arith == "bf16":
        return 2.0 ** -8 + 2.0 ** -18 + (K + E_TAIL) * U
    raise ValueError(arith)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def sentinel_f32(n):
    return np.full(n, SENTINEL, dtype=np.int32).view(np.float32)


def row_offsets(rows, ld, ld_hi=0, rdiv=0):
    """RowMap.off of csrc/mrg_common.h for rows 0..rows-1."""
    r = np.arange(rows, dtype=np.int64)
    if rdiv <= 0:
        return r * ld
    return (r // rdiv) * ld_hi + (r % rdiv) * ld


@dataclasses.dataclass
class Operand:
    buf: np.ndarray      # flat fp32 allocation, NaN wherever the operand does not live
    vals: np.ndarray     # [rows, cols] fp32, the values as stored (memory layout)
    ld: int
    ld_hi: int
    rdiv: int
    off: int             # floats from the allocation to the operand's first element


def make_operand(rng, rows, cols, pad=0, rdiv=0, shift=0, off=0, scale=1.0, tail_rows=3, vals=None):
    """An operand of `rows` memory rows by `cols` contiguous columns with row pitch cols + pad, read
    through an optional two-level row map (groups of `rdiv` rows, `shift` further rows of the
    allocation between groups: the [:, shift:] slice of a [B, T + shift, cols] tensor) and starting
    `off` floats into the allocation.  Slack columns, skipped rows and `tail_rows` rows past the end
    are NaN."""
    ld = cols + pad
    ld_hi = (rdiv + shift) * ld if rdiv > 0 else 0
    ro = row_offsets(rows, ld, ld_hi, rdiv)
    size = off + (int(ro[-1]) if rows else 0) + cols + tail_rows * ld + (shift * ld if rdiv > 0 else 0)
    buf = np.full(size, np.nan, dtype=np.float32)
    if vals is None:
        vals = (rng.standard_normal((rows, cols)) * scale).astype(np.float32)
    idx = off + ro[:, None] + np.arange(cols, dtype=np.int64)[None, :]
    buf[idx] = vals
    return Operand(buf, vals, ld, ld_hi, rdiv, off)


@dataclasses.dataclass
class Output:
    buf: np.ndarray      # flat fp32 allocation as uploaded: sentinel, C0 in the valid region if given
    idx: np.ndarray      # [M, N] flat indices of the valid region
    ld: int
    off: int
    c0: np.ndarray       # [M, N] fp32 initial values (zeros when the region starts as sentinel)


def make_output(rng, M, N, pad=3, off=0, guard_rows=4, init=False):
    """An M x N output with row pitch N + pad, `guard_rows` rows after row M - 1 and `off` floats in
    front, every float the sentinel bit pattern except, with init, the valid region (C0)."""
    ld = N + pad
    buf = sentinel_f32(off + (M + guard_rows) * ld)
    idx = off + np.arange(M, dtype=np.int64)[:, None] * ld + np.arange(N, dtype=np.int64)[None, :]
    c0 = np.zeros((M, N), dtype=np.float32)
    if init:
        c0 = rng.standard_normal((M, N)).astype(np.float32)
        buf[idx] = c0
    return Output(buf, idx, ld, off, c0)


def make_aux(rng, epi, M, N):
    """aux values per epilogue: 2 draws |N(0,1)| + 0.1 with a random sign (the mask never sits at its
    kink), 5 a saved tanh in (-0.95, 0.95), 3 and 7 N(0,1)."""
    if epi == 2:
        mag = np.abs(rng.standard_normal((M, N))) + 0.1
        return (mag * rng.choice([-1.0, 1.0], size=(M, N))).astype(np.float32)
    if epi == 5:
        return rng.uniform(-0.95, 0.95, size=(M, N)).astype(np.float32)
    return rng.standard_normal((M, N)).astype(np.float32)


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def reference(opA, opB, alpha, beta, c0, bias, epi, aux, arith):
    """(ref, bound, pre, pre_bound, skip) in float64: op(A) [M, K] and op(B) [K, N] as fp32 arrays of the
    uploaded values, c0 [M, N] (ignored when beta == 0), bias [N] or None, aux [M, N] or None.  pre is
    the epilogue's argument (what epilogue 6 stores through aux)."""
    a, b = opA.astype(np.float64), opB.astype(np.float64)
    K = a.shape[1]
    alpha, beta = float(np.float32(alpha)), float(np.float32(beta))
    pre = alpha * (a @ b)
    S = abs(alpha) * (np.abs(a) @ np.abs(b))
    if beta != 0.0:
        pre = pre + beta * c0.astype(np.float64)
        S = S + np.abs(beta * c0.astype(np.float64))
    if bias is not None:
        pre = pre + bias.astype(np.float64)[None, :]
        S = S + np.abs(bias.astype(np.float64))[None, :]
    x = None if aux is None else aux.astype(np.float64)
    if epi == 3:
        S = S + np.abs(x)
    ev = c_bound(K, arith) * S
    pre_bound = ev + ulp32(pre)
    skip = np.zeros(pre.shape, dtype=bool)
    if epi == 0:
        ref, bound = pre, ev
    elif epi == 1:
        ref, bound = np.maximum(pre, 0.0), ev
    elif epi == 2:
        ref, bound = np.where(x > 0, pre, 0.0), np.where(x > 0, ev, 0.0)
    elif epi == 3:
        ref, bound = pre + x, ev
    elif epi == 4:
        ref, bound = np.tanh(pre), ev + EPS_TANH
    elif epi == 5:
        d = 1.0 - x * x
        ref, bound = pre * d, np.abs(d) * ev + np.abs(pre) * 4 * U * (1.0 + x * x)
    elif epi == 6:
        ref, bound = pre * _sigmoid(pre), 1.1 * ev + np.abs(pre) * (EPS_SIGMOID + 2 * U)
    elif epi == 7:
        s = _sigmoid(x)
        d = s * (1.0 + x * (1.0 - s))
        ref = pre * d
        bound = 1.1 * ev + np.abs(pre) * (EPS_SIGMOID * (1 + 2 * np.abs(x)) + 4 * U * (1 + np.abs(x)))
    else:
        raise ValueError(epi)
    return ref, bound + ulp32(ref), pre, pre_bound, skip


def colsum_reference(vals, beta, out0):
    """(ref, bound) of out[n] = beta out0[n] + sum_rows vals[row, n]: a sum of `rows` fp32 terms in some
    fixed tree, at most rows + E roundings relative to sum |x| + |beta out0|, plus the result's rounding."""
    v = vals.astype(np.float64)
    ref = v.sum(0)
    S = np.abs(v).sum(0)
    if beta != 0.0:
        ref = ref + beta * out0.astype(np.float64)
        S = S + np.abs(beta * out0.astype(np.float64))
    return ref, (vals.shape[0] + E_TAIL) * U * S + ulp32(ref)


def check_output(got_buf, out: Output, ref, bound, what, skip=None):
    """The checker: every valid element finite and within its own bound of ref (at most 0.5 % skipped),
    every other float of the allocation still the sentinel bit pattern.  Returns the largest
    |got - ref| / bound."""
    got_buf = np.asarray(got_buf)
    assert got_buf.shape == out.buf.shape, f"{what}: allocation changed size"
    got = got_buf[out.idx].astype(np.float64)
    if skip is None:
        skip = np.zeros(ref.shape, dtype=bool)
    nskip = int(skip.sum())
    assert nskip <= SKIP_CAP * ref.size, f"{what}: {nskip} of {ref.size} elements skipped (cap {SKIP_CAP:.1%})"
    unwritten = (got_buf.view(np.int32)[out.idx] == SENTINEL) & ~skip
    if unwritten.any():
        m, n = np.argwhere(unwritten)[0]
        raise AssertionError(f"{what}: element ({m}, {n}) was never written ({int(unwritten.sum())} in all)")
    bad = ~np.isfinite(got) & ~skip
    if bad.any():
        m, n = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: element ({m}, {n}) is {got[m, n]} ({int(bad.sum())} non-finite in all)")
    err = np.abs(got - ref)
    ratio = np.where(skip, 0.0, err / bound)
    worst = float(ratio.max()) if ratio.size else 0.0
    if worst > 1.0:
        m, n = np.unravel_index(int(ratio.argmax()), ratio.shape)
        raise AssertionError(f"{what}: element ({m}, {n}) = {got[m, n]!r}, reference {ref[m, n]!r}: error "
                             f"{err[m, n]:.3e} is {worst:.2f} x its bound {bound[m, n]:.3e} "
                             f"({int((ratio > 1).sum())} of {ratio.size} elements over)")
    mask = np.ones(got_buf.shape, dtype=bool)
    mask[out.idx] = False
    touched = mask & (got_buf.view(np.int32) != SENTINEL)
    if touched.any():
        i = int(np.flatnonzero(touched)[0]) - out.off
        raise AssertionError(f"{what}: wrote outside the output, row {i // out.ld} column {i % out.ld} of pitch "
                             f"{out.ld} ({int(touched.sum())} floats in all)")
    return worst


def check_guard(got, what):
    """A guard region uploaded as sentinels is still all sentinels."""
    bad = np.asarray(got).view(np.int32) != SENTINEL
    assert not bad.any(), f"{what}: {int(bad.sum())} guard floats overwritten, first at {int(np.flatnonzero(bad)[0])}"


# ------------------------------------------------------------------------------------------------
# Process-wide knobs of libmrg.so that the GPU test modules must leave as they found them.

def read_knobs(lib, forced_tile=None):
    """Every process-wide GEMM / LSTM knob that can be read back, by its getter or, where a knob has only
    a setter returning the previous value, by setting it and putting it back.  Left out: knobs with
    neither (mrg_lstm_config, mrg_lstm_set_local_handoff, the min_bs threshold of mrg_lstm_set_mx).
    forced_tile: a callable returning the forced GEMM tile (mrg_gemm_force_tile has no read-back: the
    GPU modules probe it with two tiny launches, see probe_forced_tile)."""
    d, bn = ctypes.c_int(-7), ctypes.c_int(-7)
    assert lib.mrg_gemm_get_glds(ctypes.byref(d), ctypes.byref(bn)) == 0
    knobs = {"gemm mode": lib.mrg_gemm_get_mode(), "glds depth": d.value, "glds bn": bn.value}

    def swap(name, fn, probe, *rest):
        prev = fn(probe, *rest)
        fn(prev, *rest)
        knobs[name] = prev
    swap("glds_wg", lib.mrg_gemm_set_glds_wg, 1)
    swap("wide", lib.mrg_gemm_set_wide, 12)
    swap("gemm blocks_per_cu", lib.mrg_gemm_set_blocks_per_cu, 0)
    swap("lstm mx", lib.mrg_lstm_set_mx, 1, 0)
    swap("lstm solo", lib.mrg_lstm_set_solo, 1)
    if forced_tile is not None:
        knobs["forced tile"] = forced_tile()
    return knobs


def probe_forced_tile(lib, launch):
    """The tile mrg_gemm_force_tile holds (-1 = heuristic), read off mrg_gemm_last_kernel after two tiny
    x6-mode products whose heuristic tiles differ: a split transposed-A product (128x128) and an
    unsplit 65-row one (64x64).  launch(transA, M, N, K, splits) runs one; a forced tile shows in both."""
    mode = lib.mrg_gemm_get_mode()
    assert lib.mrg_gemm_set_mode(1) == 0
    try:
        names = []
        for args in ((1, 5, 5, 96, 2), (0, 65, 5, 8, 1)):
            launch(*args)
            names.append(lib.mrg_gemm_last_kernel().decode())
    finally:
        assert lib.mrg_gemm_set_mode(mode) == 0
    tiles = [int(n.split(":")[1][0]) for n in names]
    assert all(n.startswith("gemm_x6_kernel:") for n in names), names
    if tiles == [0, 2]:
        return -1
    assert tiles[0] == tiles[1], names
    return tiles[0]


def knob_diff(before, after):
    return [f"{k}: {before[k]} -> {after[k]}" for k in before if before[k] != after.get(k)]

