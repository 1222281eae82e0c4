"""The GEMM route tests' checker (tests/gemm_ref.py) checked on the CPU: its float64 reference against
torch.matmul, its bound against an fp32 product that is known to be right, and its verdict on
deliberately corrupted outputs (one wrong element, one unwritten element, one write into the padding,
one write into a guard row), each of which it must reject."""
import numpy as np
import pytest
import torch

from tests import gemm_ref as R

SHAPES = [(1, 1, 1), (3, 70, 300), (65, 63, 33), (129, 45, 130)]


def _case(M, N, K, epi, ta=0, tb=1, alpha=0.75, beta=0.5, seed=0):
    rng = np.random.default_rng(seed + 1000 * epi + M + N + K)
    A = R.make_operand(rng, K if ta else M, M if ta else K, pad=5, rdiv=4 if not ta else 0, shift=2, off=1)
    B = R.make_operand(rng, N if tb else K, K if tb else N, pad=3, scale=1.0 / np.sqrt(K))
    opA = A.vals.T if ta else A.vals
    opB = B.vals.T if tb else B.vals
    bias = rng.standard_normal(N).astype(np.float32)
    aux = R.make_aux(rng, epi, M, N) if epi in (2, 3, 5, 7) else None
    out = R.make_output(rng, M, N, pad=3, off=1, init=beta != 0.0)
    return A, B, opA, opB, bias, aux, out, alpha, beta


def _torch_ref(opA, opB, alpha, beta, c0, bias, epi, aux):
    v = alpha * torch.matmul(torch.from_numpy(opA).double(), torch.from_numpy(opB).double())
    v = v + beta * torch.from_numpy(c0).double() + torch.from_numpy(bias).double()
    x = None if aux is None else torch.from_numpy(aux).double()
    if epi == 1:
        v = v.clamp_min(0)
    elif epi == 2:
        v = v * (x > 0)
    elif epi == 3:
        v = v + x
    elif epi == 4:
        v = torch.tanh(v)
    elif epi == 5:
        v = v * (1 - x * x)
    elif epi == 6:
        v = torch.nn.functional.silu(v)
    elif epi == 7:
        xg = x.clone().requires_grad_(True)
        torch.nn.functional.silu(xg).sum().backward()
        v = v * xg.grad
    return v.numpy()


@pytest.mark.parametrize("epi", range(8))
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_reference_matches_torch_float64(M, N, K, epi):
    """The numpy reference, read through the operands' row maps, is torch.matmul's float64 answer
    (epilogue 7 against autograd's silu')."""
    A, B, opA, opB, bias, aux, out, alpha, beta = _case(M, N, K, epi)
    # the values really live in the buffer where the row map says
    ro = R.row_offsets(A.vals.shape[0], A.ld, A.ld_hi, A.rdiv)
    assert np.array_equal(A.buf[A.off + ro[-1]: A.off + ro[-1] + A.vals.shape[1]], A.vals[-1])
    assert np.isnan(A.buf).sum() == A.buf.size - A.vals.size
    ref, bound, pre, pre_bound, skip = R.reference(opA, opB, alpha, beta, out.c0, bias, epi, aux, "f32")
    want = _torch_ref(opA, opB, alpha, beta, out.c0, bias, epi, aux)
    assert np.abs(ref - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    assert (bound > 0).all() and np.isfinite(bound).all()
    assert not skip.any()      # the kink cap holds on the reference alone: nothing is ever skipped


@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_bound_admits_a_plain_fp32_product(ta, tb):
    """An fp32 product computed term by term (numpy float32, a K-term chain like the f32 MFMA's) lies
    inside the "f32" bound, and so inside the looser "x6" one; the bf16 bound admits operands rounded
    to bf16, which the f32 bound rejects."""
    M, N, K = 37, 45, 53
    A, B, opA, opB, bias, aux, out, alpha, beta = _case(M, N, K, 3, ta, tb)
    acc = np.zeros((M, N), dtype=np.float32)
    for k in range(K):
        acc += opA[:, k:k + 1] * opB[k:k + 1, :]
    got = (np.float32(alpha) * acc + np.float32(beta) * out.c0 + bias[None, :] + aux).astype(np.float32)
    buf = out.buf.copy()
    buf[out.idx] = got
    for arith in ("f32", "x6", "bf16"):
        ref, bound, *_ = R.reference(opA, opB, alpha, beta, out.c0, bias, 3, aux, arith)
        assert R.check_output(buf, out, ref, bound, arith) <= 1.0
    rb = lambda v: torch.from_numpy(v.copy()).bfloat16().float().numpy()  # noqa: E731
    got16 = (np.float32(alpha) * (rb(opA).astype(np.float64) @ rb(opB).astype(np.float64)) + np.float32(beta) * out.c0
             + bias[None, :] + aux).astype(np.float32)
    buf[out.idx] = got16
    ref, bound, *_ = R.reference(opA, opB, alpha, beta, out.c0, bias, 3, aux, "bf16")
    assert R.check_output(buf, out, ref, bound, "bf16") <= 1.0
    ref, bound, *_ = R.reference(opA, opB, alpha, beta, out.c0, bias, 3, aux, "f32")
    with pytest.raises(AssertionError, match="its bound"):
        R.check_output(buf, out, ref, bound, "f32")


def test_bound_constants():
    """c(K, arith) as derived in the helper's docstring."""
    u = 2.0 ** -24
    assert R.c_bound(32, "f32") == (32 + 24) * u
    assert R.c_bound(32, "x6") == (6 * 32 + 6 + 24) * u
    assert R.c_bound(32, "bf16") == 2.0 ** -8 + 2.0 ** -18 + (32 + 24) * u
    assert R.ulp32(1.0) == 2.0 ** -23 and R.ulp32(0.0) > 0


@pytest.mark.parametrize("beta", [0.0, 0.5])
def test_checker_rejects_each_corruption(beta):
    """A right output passes; one wrong element (small against the largest entry, so a max-norm test would
    pass it), one unwritten element, one write into the row padding and one into a guard row each fail."""
    M, N, K = 65, 63, 33
    A, B, opA, opB, bias, aux, out, alpha, _ = _case(M, N, K, 0, beta=beta)
    ref, bound, *_ = R.reference(opA, opB, alpha, beta, out.c0, bias, 0, None, "x6")
    good = out.buf.copy()
    good[out.idx] = ref.astype(np.float32)
    assert R.check_output(good, out, ref, bound, "good") <= 1.0

    m, n = np.unravel_index(int(np.abs(ref).argmin()), ref.shape)
    wrong = good.copy()
    wrong[out.idx[m, n]] += np.float32(1e-4 * np.abs(ref).max())      # 1e-4 of the max norm: rel_err passes it
    assert np.abs(wrong[out.idx] - ref).max() / np.abs(ref).max() < 2e-4
    with pytest.raises(AssertionError, match=rf"element \({m}, {n}\)"):
        R.check_output(wrong, out, ref, bound, "wrong")

    unwritten = good.copy()
    unwritten[out.idx[M - 1, N - 1]] = out.buf[out.idx[M - 1, N - 1]]
    with pytest.raises(AssertionError, match=rf"element \({M - 1}, {N - 1}\)"):
        R.check_output(unwritten, out, ref, bound, "unwritten")

    padded = good.copy()
    padded[out.idx[3, N - 1] + 1] = ref[3, N - 1]
    with pytest.raises(AssertionError, match=rf"outside the output, row 3 column {N}"):
        R.check_output(padded, out, ref, bound, "padding")

    guard = good.copy()
    guard[out.off + M * out.ld] = 0.0
    with pytest.raises(AssertionError, match=rf"outside the output, row {M} column 0"):
        R.check_output(guard, out, ref, bound, "guard row")

    nan = good.copy()
    nan[out.idx[0, 0]] = np.nan
    with pytest.raises(AssertionError, match="non-finite"):
        R.check_output(nan, out, ref, bound, "nan")


def test_skip_cap_and_mask_inputs():
    """More than 0.5 % skipped elements fail a case; the epilogue-2 aux draw keeps |aux| >= 0.1, so its
    mask is the same in fp32 and float64."""
    rng = np.random.default_rng(3)
    aux = R.make_aux(rng, 2, 65, 63)
    assert np.abs(aux).min() >= 0.1 and (aux > 0).any() and (aux < 0).any()
    out = R.make_output(rng, 20, 20)
    ref = rng.standard_normal((20, 20))
    good = out.buf.copy()
    good[out.idx] = ref.astype(np.float32)
    bound = R.ulp32(ref)
    skip = np.zeros((20, 20), dtype=bool)
    skip[0, :2] = True                                                 # 2 of 400 = the cap exactly
    assert R.check_output(good, out, ref, bound, "cap", skip) <= 1.0
    skip[0, 2] = True
    with pytest.raises(AssertionError, match="skipped"):
        R.check_output(good, out, ref, bound, "cap", skip)


def test_colsum_reference_and_guard():
    rng = np.random.default_rng(5)
    v = rng.standard_normal((577, 6)).astype(np.float32)
    out0 = rng.standard_normal(6).astype(np.float32)
    ref, bound = R.colsum_reference(v, 1.0, out0)
    want = torch.from_numpy(v).double().sum(0).numpy() + out0
    assert np.abs(ref - want).max() < 1e-12
    assert (np.abs(v.sum(0) + out0 - ref) <= bound).all()
    g = R.sentinel_f32(16)
    R.check_guard(g, "guard")
    g[5] = 0.0
    with pytest.raises(AssertionError, match="first at 5"):
        R.check_guard(g, "guard")


def test_tuning_queries_are_host_state():
    """mrg_gemm_get_glds mirrors mrg_gemm_set_glds, a refused setting changes nothing, and
    mrg_gemm_last_kernel answers without a GPU (no GEMM has run on this thread: the empty string)."""
    import ctypes
    from multimodalreactiongeneration_amd import _lib
    lib = _lib.load()
    d, bn = ctypes.c_int(), ctypes.c_int()
    assert lib.mrg_gemm_get_glds(ctypes.byref(d), ctypes.byref(bn)) == 0
    start = (d.value, bn.value)
    assert start[0] in (0, 2, 3, 4) and start[1] in (64, 128)
    try:
        assert lib.mrg_gemm_set_glds(3, 64) == 0
        assert lib.mrg_gemm_get_glds(ctypes.byref(d), ctypes.byref(bn)) == 0 and (d.value, bn.value) == (3, 64)
        assert lib.mrg_gemm_set_glds(5, 64) != 0 and lib.mrg_gemm_set_glds(2, 96) != 0
        assert b"mrg_gemm_set_glds" in lib.mrg_last_error()
        assert lib.mrg_gemm_get_glds(ctypes.byref(d), ctypes.byref(bn)) == 0 and (d.value, bn.value) == (3, 64)
        assert lib.mrg_gemm_get_glds(None, ctypes.byref(bn)) != 0
    finally:
        assert lib.mrg_gemm_set_glds(*start) == 0
    before = R.read_knobs(lib)
    assert R.read_knobs(lib) == before and not R.knob_diff(before, R.read_knobs(lib))
    assert isinstance(lib.mrg_gemm_last_kernel(), bytes)
