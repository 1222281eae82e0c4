"""Every GEMM route of libmrg.so against float64 at its tile and alignment edges, through the C ABI.

Each case (tests/gemm_ref.py holds the reference, the derived bound and the checker):
  * every element within its OWN bound c(K, arith) * (|alpha| sum |a b| + |beta C0| + |bias|) of the
    float64 reference, pushed through the epilogue (no max-norm grading);
  * C with row pitch N + pad and four guard rows, pre-filled with a sentinel bit pattern: the valid
    region is all written, the rest bitwise untouched; so are the guard floats after the split-K
    workspace, and the tickets are all zero;
  * A and B with NaN in their slack columns and in rows past their extent (same allocation): a lane
    that lets a clamped or over-read value reach an accumulator turns the output NaN;
  * two runs, bitwise equal;
  * mrg_gemm_last_kernel() names the route the case was written for, so a retuned gate fails the case
    instead of silently emptying it.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import gemm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VP, CI = ctypes.c_void_p, ctypes.c_int
WS_GUARD = 1024          # sentinel floats after the split-K workspace
HEADROOM = {}            # route -> largest observed error / bound (a record, never a criterion)


def _lib():
    from multimodalreactiongeneration_amd import _lib as L
    return L, L.load()


def _stream():
    return VP(torch.cuda.current_stream().cuda_stream)


def _dev(buf):
    return torch.from_numpy(np.ascontiguousarray(buf)).to(DEV)


def _p(t, off=0):
    return None if t is None else VP(t.data_ptr() + off * t.element_size())


def _host(t):
    return t.cpu().numpy()


def _tiny_launch(lib):
    def launch(ta, M, N, K, splits):
        a = torch.zeros((K, M) if ta else (M, K), device=DEV)
        b = torch.zeros(K, N, device=DEV)
        c = torch.zeros(M, N, device=DEV)
        ws = torch.zeros(max(1, lib.mrg_gemm_workspace_bytes(M, N, splits) // 4), device=DEV)
        rc = lib.mrg_gemm_f32_ex(M, N, K, 1.0, _p(a), ta, M if ta else K, 0, 0, _p(b), 0, N, 0, 0, 0.0, _p(c), N, None,
                                 0, None, 0, _p(ws), splits, None, None, 0.0, None, _stream())
        assert rc == 0
        torch.cuda.synchronize()
    return launch


def read_knobs(lib):
    return R.read_knobs(lib, lambda: R.probe_forced_tile(lib, _tiny_launch(lib)))


@pytest.fixture(scope="module", autouse=True)
def _knobs_unchanged():
    """Every process-wide knob as the module found it, and the headroom record printed at the end."""
    L, lib = _lib()
    before = read_knobs(lib)
    yield
    torch.cuda.synchronize()
    after = read_knobs(lib)
    for route, ratio in sorted(HEADROOM.items()):
        print(f"\ngemm route headroom: {route}: largest error / bound = {ratio:.4f}", end="")
    print()
    assert not R.knob_diff(before, after), "process-wide knobs changed: " + "; ".join(R.knob_diff(before, after))


@pytest.fixture
def knobs():
    """Setter for the GEMM knobs of one test; all restored afterwards."""
    L, lib = _lib()
    d, bn = CI(), CI()
    L.check(lib.mrg_gemm_get_glds(ctypes.byref(d), ctypes.byref(bn)), "get_glds")
    mode = lib.mrg_gemm_get_mode()
    state = {"wg": None, "wide": None, "bpc": None, "tile": False}

    def set_(mode=None, glds=None, tile=None, wg=None, wide=None, bpc=None):
        if mode is not None:
            L.check(lib.mrg_gemm_set_mode(mode), "mode")
        if glds is not None:
            L.check(lib.mrg_gemm_set_glds(*glds), "glds")
        if tile is not None:
            L.check(lib.mrg_gemm_force_tile(tile), "tile")
            state["tile"] = True
        for key, fn, v in (("wg", lib.mrg_gemm_set_glds_wg, wg), ("wide", lib.mrg_gemm_set_wide, wide),
                           ("bpc", lib.mrg_gemm_set_blocks_per_cu, bpc)):
            if v is not None:
                prev = fn(v)
                if state[key] is None:
                    state[key] = prev
    yield set_
    if state["tile"]:
        lib.mrg_gemm_force_tile(-1)     # no read-back: the module fixture's probe checks the heuristic is back
    lib.mrg_gemm_set_glds(d.value, bn.value)
    lib.mrg_gemm_set_mode(mode)
    for key, fn in (("wg", lib.mrg_gemm_set_glds_wg), ("wide", lib.mrg_gemm_set_wide),
                    ("bpc", lib.mrg_gemm_set_blocks_per_cu)):
        if state[key] is not None:
            fn(state[key])


def _record(route, ratio):
    HEADROOM[route] = max(HEADROOM.get(route, 0.0), ratio)


def run_gemm(M, N, K, route, arith, *, ta=0, tb=1, alpha=1.0, beta=0.0, epi=0, bias=True, a=None, b=None, cpad=3,
             coff=0, auxpad=None, splits=1, counters=False, asum=0, asum_beta=0.0, entry="mrg_gemm_f32_ex", seed=0,
             repeats=2, ws=True):
    """One mrg_gemm_f32_ex / mrg_gemm_bf16_ex case, checked as the module docstring says.  a / b:
    make_operand keywords (pad, rdiv, shift, off); asum: 0 none, 1 asum_out, 2 asum_out and asum_out2."""
    L, lib = _lib()
    rng = np.random.default_rng([seed, M, N, K, epi, ta, tb, splits])
    A = R.make_operand(rng, K if ta else M, M if ta else K, **(a or {"pad": 4}))
    B = R.make_operand(rng, N if tb else K, K if tb else N, scale=1.0 / math.sqrt(K), **(b or {"pad": 4}))
    opA = A.vals.T if ta else A.vals
    opB = B.vals.T if tb else B.vals
    bias_h = rng.standard_normal(N).astype(np.float32) if bias else None
    aux_h = R.make_aux(rng, epi, M, N) if epi in (2, 3, 5, 7) else None
    auxpad = cpad if auxpad is None else auxpad
    out = R.make_output(rng, M, N, pad=cpad, off=coff, init=beta != 0.0)
    auxo = R.make_output(rng, M, N, pad=auxpad, init=aux_h is not None) if epi >= 2 and epi != 4 else None
    if aux_h is not None:
        auxo.buf[auxo.idx] = aux_h
    ref, bound, pre, pre_bound, skip = R.reference(opA, opB, alpha, beta, out.c0, bias_h, epi, aux_h, arith)
    sum0 = rng.standard_normal(M).astype(np.float32)
    sums = [R.make_output(rng, 1, M, pad=0, guard_rows=4) for _ in range(asum)]
    for s in sums:
        if asum_beta != 0.0:
            s.buf[s.idx] = sum0
            s.c0 = sum0[None, :]
    Ad, Bd = _dev(A.buf), _dev(B.buf)
    bias_d = None if bias_h is None else _dev(bias_h)
    ws_n = lib.mrg_gemm_workspace_bytes(M, N, splits) // 4 if ws else 0
    cnt = torch.zeros(4096, dtype=torch.int32, device=DEV) if counters else None
    fn = getattr(lib, entry)
    results = []
    for _ in range(repeats):
        Cd = _dev(out.buf)
        auxd = None if auxo is None else _dev(auxo.buf)
        wsd = _dev(R.sentinel_f32(ws_n + WS_GUARD)) if ws else None
        sd = [_dev(s.buf) for s in sums]
        L.check(fn(M, N, K, alpha, _p(Ad, A.off), ta, A.ld, A.ld_hi, A.rdiv, _p(Bd, B.off), tb, B.ld, B.ld_hi, B.rdiv,
                   beta, _p(Cd, coff), out.ld, _p(bias_d), epi, _p(auxd), 0 if auxo is None else auxo.ld, _p(wsd),
                   splits, _p(sd[0]) if asum >= 1 else None, _p(sd[1]) if asum >= 2 else None, asum_beta, _p(cnt),
                   _stream()), entry)
        got_route = lib.mrg_gemm_last_kernel().decode()
        torch.cuda.synchronize()
        assert got_route == route, f"ran {got_route}, the case was written for {route}"
        results.append((_host(Cd), None if auxd is None else _host(auxd), [_host(s) for s in sd]))
        if ws:
            R.check_guard(_host(wsd)[ws_n:], "split-K workspace guard")
        if cnt is not None:
            assert int(cnt.abs().sum()) == 0, "tickets not back at zero"
    what = f"{route} {M}x{N}x{K}"
    ratio = R.check_output(results[0][0], out, ref, bound, what, skip)
    if epi == 6:     # the pre-activation stored through aux
        ratio = max(ratio, R.check_output(results[0][1], auxo, pre, pre_bound, what + " aux"))
    elif auxo is not None:
        assert np.array_equal(results[0][1].view(np.int32), auxo.buf.view(np.int32)), "aux (an input) was written"
    for s, got in zip(sums, results[0][2]):
        sref, sbound = R.colsum_reference(opA.T, asum_beta, sum0)
        _record("asum", R.check_output(got, s, sref[None, :], sbound[None, :], what + " row sums"))
    for r in results[1:]:
        assert np.array_equal(r[0].view(np.int32), results[0][0].view(np.int32)), "not bitwise repeatable"
        for g0, g1 in zip(results[0][2], r[2]):
            assert np.array_equal(g0.view(np.int32), g1.view(np.int32)), "row sums not bitwise repeatable"
    _record(route.split(":")[0] + (" bf16" if arith == "bf16" else ""), ratio)
    return results[0][0]


# ------------------------------------------------------------------------------------------------
# gemm_rows_kernel: x6 mode, unsplit, M <= 64 (A rows) or K <= 64 (transposed A)

@pytest.mark.parametrize("M,N,K,tb,epi,a,b", [
    (1, 1, 1, 1, 0, None, None),
    (3, 70, 300, 1, 1, {"pad": 3, "off": 1}, {"pad": 1}),                   # unaligned A, odd pitches
    (63, 6, 40, 0, 2, {"pad": 4, "rdiv": 7, "shift": 2, "off": 8}, None),   # row-mapped A (a_hi, a_div)
    (64, 257, 300, 0, 3, None, {"pad": 5}),
    (64, 70, 1, 1, 0, {"pad": 0}, {"pad": 0}),
    (3, 257, 40, 1, 3, {"pad": 0, "off": 1}, {"pad": 0, "off": 3}),
])
def test_rows_kernel_plain_a(M, N, K, tb, epi, a, b, knobs):
    knobs(mode=1)
    run_gemm(M, N, K, "gemm_rows_kernel", "f32", ta=0, tb=tb, alpha=0.75, beta=0.5, epi=epi, a=a, b=b)


@pytest.mark.parametrize("M,N,K,tb,asum,asum_beta,a", [
    (1, 6, 1, 0, 1, 0.0, None),
    (63, 70, 33, 0, 2, 1.0, {"pad": 1, "off": 1}),
    (64, 257, 64, 1, 2, 0.0, {"pad": 4, "rdiv": 8, "shift": 1}),           # time-shifted rows of k
    (130, 6, 33, 1, 1, 1.0, None),
    (3, 1, 64, 0, 0, 0.0, None),
])
def test_rows_kernel_transposed_a(M, N, K, tb, asum, asum_beta, a, knobs):
    """The weight-gradient form over <= 64 rows, its bias sums (asum_out / asum_out2) fused."""
    knobs(mode=1)
    run_gemm(M, N, K, "gemm_rows_kernel", "f32", ta=1, tb=tb, beta=1.0, bias=False, a=a, asum=asum,
             asum_beta=asum_beta)


def test_rows_kernel_smooth_epilogues(knobs):
    knobs(mode=1)
    for epi in (4, 5, 6, 7):
        run_gemm(63, 70, 40, "gemm_rows_kernel", "f32", alpha=0.75, beta=0.5, epi=epi, seed=epi)


# ------------------------------------------------------------------------------------------------
# gemm_x6g_kernel: NT, K % 32 == 0, aligned, M >= 2048, N >= 256, unsplit

@pytest.mark.parametrize("depth,bn", [(2, 128), (3, 128), (4, 128), (3, 64)])
@pytest.mark.parametrize("M,N,K,epi,cpad,a", [
    (2048, 256, 32, 0, 4, None),                                            # 64x64 tiles, one k-tile
    (2049, 260, 96, 1, 4, None),                                            # one clamped row, N past a tile edge
    (2048 + 127, 257, 64, 2, 0, None),                                      # ldc = 257: scalar stores
    (2049, 1024 + 4, 160, 3, 4, {"pad": 4, "rdiv": 683, "shift": 2, "off": 8}),   # 128x128 tiles, row-mapped A
])
def test_x6g_kernel(M, N, K, epi, cpad, a, depth, bn, knobs):
    """Ring depths 2..4 against k-loops shorter than, equal to and past the ring, every tile shape, ragged
    M and N, vector and scalar stores, alpha != 1 and beta != 0."""
    knobs(mode=1, glds=(depth, bn))
    run_gemm(M, N, K, "gemm_x6g_kernel", "x6", alpha=0.75, beta=0.5, epi=epi, cpad=cpad, a=a)


@pytest.mark.parametrize("M,N,K,epi,cpad", [(2049, 260, 96, 1, 4), (2048 + 127, 257, 32, 3, 0)])
def test_x6g_kernel_one_plane(M, N, K, epi, cpad, knobs):
    """mrg_gemm_bf16_ex at the same ragged shapes, under the bf16 bound."""
    knobs(mode=1, glds=(3, 128))
    run_gemm(M, N, K, "gemm_x6g_kernel", "bf16", alpha=0.75, beta=0.5, epi=epi, cpad=cpad, entry="mrg_gemm_bf16_ex")


def test_x6g_kernel_smooth_epilogues(knobs):
    knobs(mode=1, glds=(2, 128))
    for epi in (4, 5, 6, 7):
        run_gemm(2049, 260, 64, "gemm_x6g_kernel", "x6", alpha=0.75, beta=0.5, epi=epi, cpad=4, seed=epi)


@pytest.mark.parametrize("n,epi,with_bias", [(1, 0, True), (3, 3, False), (16, 1, True)])
def test_x6g_batched(n, epi, with_bias, knobs):
    """mrg_gemm_x6g_batched at a ragged shape: each problem against float64 and bitwise equal to its own
    single launch; one case with the bias array absent, one with the aux array absent."""
    L, lib = _lib()
    knobs(mode=1, glds=(2, 128))
    M, N, K = 2049, 260, 64
    rng = np.random.default_rng([n, epi])
    As = [R.make_operand(rng, M, K, pad=4) for _ in range(n)]
    Bs = [R.make_operand(rng, N, K, pad=4, scale=1.0 / math.sqrt(K)) for _ in range(n)]
    bias = [rng.standard_normal(N).astype(np.float32) for _ in range(n)] if with_bias else None
    aux = [R.make_aux(rng, epi, M, N) for _ in range(n)] if epi >= 2 else None
    outs = [R.make_output(rng, M, N, pad=4, init=True) for _ in range(n)]
    Ad, Bd = [_dev(x.buf) for x in As], [_dev(x.buf) for x in Bs]
    bd = None if bias is None else [_dev(x) for x in bias]
    xd = None if aux is None else [_dev(np.pad(x, ((0, 0), (0, 4)))) for x in aux]
    Cd = [_dev(o.buf) for o in outs]
    arr = lambda v: None if v is None else (VP * n)(*[VP(t.data_ptr()) for t in v])  # noqa: E731
    L.check(lib.mrg_gemm_x6g_batched(n, M, N, K, 0.75, arr(Ad), K + 4, arr(Bd), K + 4, 0.5, arr(Cd), N + 4, arr(bd),
                                     epi, arr(xd), N + 4, 0, _stream()), "batched")
    assert lib.mrg_gemm_last_kernel() == b"gemm_x6g_kernel"
    torch.cuda.synchronize()
    for i in range(n):
        ref, bound, *_ = R.reference(As[i].vals, Bs[i].vals.T, 0.75, 0.5, outs[i].c0, None if bias is None else bias[i],
                                     epi, None if aux is None else aux[i], "x6")
        _record("gemm_x6g_batched", R.check_output(_host(Cd[i]), outs[i], ref, bound, f"batched problem {i}"))
        single = _dev(outs[i].buf)
        L.check(lib.mrg_gemm_f32_ex(M, N, K, 0.75, _p(Ad[i]), 0, K + 4, 0, 0, _p(Bd[i]), 1, K + 4, 0, 0, 0.5, _p(single),
                                    N + 4, None if bd is None else _p(bd[i]), epi, None if xd is None else _p(xd[i]),
                                    N + 4, None, 1, None, None, 0.0, None, _stream()), "single")
        assert lib.mrg_gemm_last_kernel() == b"gemm_x6g_kernel"
        torch.cuda.synchronize()
        assert torch.equal(single.view(torch.int32), Cd[i].view(torch.int32)), i


# ------------------------------------------------------------------------------------------------
# generic tile kernels: gemm_x6_kernel (x6 mode) and gemm_f32_kernel (exact mode)

LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]
GENERIC = [   # M, N, K, epi, a, b, cpad: vector loads (aligned, pitch % 4 == 0) and scalar ones on each operand
    (65, 63, 33, 0, {"pad": 4}, {"pad": 1}, 3),
    (129, 1, 53, 1, {"pad": 3, "off": 1}, {"pad": 4}, 2),
    (65, 129, 130, 2, {"pad": 4, "off": 4}, {"pad": 4, "off": 1}, 4),
    (129, 65, 31, 3, {"pad": 0, "off": 0}, {"pad": 0}, 0),
    (65, 65, 1, 0, {"pad": 7}, {"pad": 7}, 3),
]


def _generic_cases(tile, cases):
    """every case on the 64x64 tile, three on each forced larger tile, one to pin the heuristic"""
    return cases if tile == 2 else cases[:3] if tile >= 0 else cases[:1]


def _pitch(spec, cols):
    """pads written for a pitch of cols + pad % 4 == 0: make the pitch itself a multiple of 4 when asked"""
    spec = dict(spec)
    if spec["pad"] == 4:
        spec["pad"] = 4 + (-cols) % 4
    return spec


@pytest.mark.parametrize("tile", [0, 1, 2, -1])
@pytest.mark.parametrize("ta,tb", LAYOUTS)
def test_generic_x6_tiles(ta, tb, tile, knobs):
    """gemm_x6_kernel at every forced tile and the heuristic one.  M > 64 and K > 64 where the few-row
    kernel would take the product; the weight-gradient kernel is off for a forced tile and is kept
    off the heuristic TN cases by M % 4 != 0."""
    knobs(mode=1, tile=tile)
    for i, (M, N, K, epi, a, b, cpad) in enumerate(_generic_cases(tile, GENERIC)):
        if ta and K <= 64:
            K += 64                     # transposed A with K <= 64 is the few-row kernel's
        a2 = _pitch(a, M if ta else K)
        b2 = _pitch(b, K if tb else N)
        run_gemm(M, N, K, f"gemm_x6_kernel:{2 if tile < 0 else tile}", "x6", ta=ta, tb=tb, alpha=0.75, beta=0.5, epi=epi,
                 a=a2, b=b2, cpad=cpad, auxpad=cpad, repeats=2 if i == 0 else 1)


@pytest.mark.parametrize("tile", [0, 1, 2, -1])
@pytest.mark.parametrize("ta,tb", LAYOUTS)
def test_generic_f32_tiles(ta, tb, tile, knobs):
    """gemm_f32_kernel (exact mode), which also takes M = 1 and M = 63."""
    knobs(mode=0, tile=tile)
    more = [(1, 129, 33, 3, {"pad": 1}, {"pad": 4}, 1), (63, 65, 130, 1, {"pad": 4}, {"pad": 3}, 4)]
    for i, (M, N, K, epi, a, b, cpad) in enumerate(_generic_cases(tile, more + GENERIC)):
        a2 = _pitch(a, M if ta else K)
        b2 = _pitch(b, K if tb else N)
        run_gemm(M, N, K, f"gemm_f32_kernel:{2 if tile < 0 else tile}", "f32", ta=ta, tb=tb, alpha=0.75, beta=0.5,
                 epi=epi, a=a2, b=b2, cpad=cpad, auxpad=cpad, repeats=2 if i == 0 else 1)


@pytest.mark.parametrize("mode,route,arith", [(1, "gemm_x6_kernel:2", "x6"), (0, "gemm_f32_kernel:2", "f32")])
def test_generic_tiles_smooth_epilogues(mode, route, arith, knobs):
    knobs(mode=mode)
    for epi in (4, 5, 6, 7):
        run_gemm(65, 63, 33, route, arith, alpha=0.75, beta=0.5, epi=epi, cpad=3, seed=epi)


# ------------------------------------------------------------------------------------------------
# split-K: slabs, then the in-launch combine or one of the two reduce kernels

@pytest.mark.parametrize("splits,K", [(2, 70), (3, 65), (3, 130), (5, 100), (5, 33)])
@pytest.mark.parametrize("form", ["cnt", "reduce4", "reduce_n45", "reduce_c_off"])
def test_split_k(form, splits, K, knobs):
    """K not a multiple of 32 * splits: the dispatcher rounds the slice to whole k-tiles and recomputes
    the split count ((5, 100) runs 4 slices, (5, 33) two, the last of one element).  beta != 0, bias and
    the residual epilogue 3 must each apply exactly once, whichever pass combines the slabs."""
    knobs(mode=1)
    kc = 32 * math.ceil(math.ceil(K / splits) / 32)      # the dispatcher's slice, in whole k-tiles
    ran = math.ceil(K / kc)                              # and the split count it then runs
    assert ran > 1 and (ran != splits or K % kc != 0)
    M, N, coff, cpad = 130, 72, 0, 4
    if form == "reduce_n45":
        N = 45
    elif form == "reduce_c_off":
        coff = 1
    counters = form == "cnt"
    route = "gemm_x6_kernel:2" + ("+cnt" if counters else "")
    run_gemm(M, N, K, route, "x6", ta=0, tb=1, alpha=0.75, beta=0.5, epi=3, cpad=cpad, coff=coff, splits=splits,
             counters=counters, repeats=3 if counters else 2,
             a={"pad": 4 + (-K) % 4}, b={"pad": 4 + (-K) % 4})


@pytest.mark.parametrize("mode,route,arith", [(1, "gemm_x6_kernel:0", "x6"), (0, "gemm_f32_kernel:2", "f32")])
def test_split_k_transposed_a_and_exact(mode, route, arith, knobs):
    """Split weight-gradient shapes the LDS-DMA kernel does not take (M % 4 != 0): 128x128 tiles in x6
    mode with the row sums fused, 64x64 tiles and the column-sum kernels in exact mode."""
    knobs(mode=mode)
    run_gemm(66, 70, 100, route, arith, ta=1, tb=0, beta=1.0, bias=False, splits=3, asum=2, asum_beta=1.0,
             a={"pad": 2}, b={"pad": 2}, cpad=2)
    run_gemm(130, 45, 70, route if mode == 1 else "gemm_f32_kernel:2", arith, ta=1, tb=0, alpha=0.75, beta=0.5, epi=1,
             splits=2, cpad=3)


def test_split_k_smooth_epilogue(knobs):
    knobs(mode=1)
    run_gemm(130, 72, 130, "gemm_x6_kernel:2+cnt", "x6", alpha=0.75, beta=0.5, epi=6, cpad=4, splits=3, counters=True,
             a={"pad": 6}, b={"pad": 6})
    run_gemm(130, 45, 130, "gemm_x6_kernel:2", "x6", alpha=0.75, beta=0.5, epi=7, cpad=3, splits=3,
             a={"pad": 6}, b={"pad": 6})


# ------------------------------------------------------------------------------------------------
# gemm_x6g_wgrad_kernel: TN, K % 32 == 0, M % 4 == N % 4 == 0, M, N >= 64

@pytest.mark.parametrize("wg", [1, 0], ids=["glds", "regstaged"])
@pytest.mark.parametrize("M,N,K,splits,shifted,asum,asum_beta", [
    (64, 64, 96, 1, False, 1, 0.0),           # (K <= 64 unsplit is the few-row kernel's: K = 32 never gets here)
    (68, 132, 160, 2, True, 2, 1.0),          # slices of 96 and 64 rows, time-shifted rows on both operands
    (256, 64, 224, 3, False, 2, 0.0),         # 96 + 96 + 32
    (68, 132, 160, 3, False, 0, 0.0),         # 64 + 64 + 32
])
def test_wgrad_kernel(M, N, K, splits, shifted, asum, asum_beta, wg, knobs):
    """dW = dY^T X accumulated into a non-zero gradient (beta = 1) with the bias sums fused; with the
    LDS-DMA form off the same cases run the register-staged 128x128 tile kernel."""
    knobs(mode=1, wg=wg)
    lay = {"pad": 4, "rdiv": 16, "shift": 1, "off": 4} if shifted else {"pad": 4}
    route = "gemm_x6g_wgrad_kernel" if wg else "gemm_x6_kernel:0" if splits > 1 else "gemm_x6_kernel:2"
    run_gemm(M, N, K, route, "x6", ta=1, tb=0, beta=1.0, bias=False,
             splits=splits, asum=asum, asum_beta=asum_beta, a=dict(lay), b=dict(lay), cpad=4)


def test_wgrad_kernel_capped_grid(knobs):
    """mrg_gemm_set_blocks_per_cu(1): 8 tiles x 40 slices walk a grid of at most one block per CU."""
    knobs(mode=1, wg=1, bpc=1)
    run_gemm(512, 256, 1280, "gemm_x6g_wgrad_kernel", "x6", ta=1, tb=0, beta=1.0, bias=False, splits=40, asum=1,
             asum_beta=1.0, cpad=4)


def test_wgrad_kernel_one_plane_and_smooth(knobs):
    knobs(mode=1, wg=1)
    run_gemm(68, 132, 160, "gemm_x6g_wgrad_kernel", "bf16", ta=1, tb=0, beta=1.0, bias=False, splits=2, cpad=4,
             entry="mrg_gemm_bf16_ex")
    for epi in (4, 5, 6, 7):
        run_gemm(68, 132, 160, "gemm_x6g_wgrad_kernel", "x6", ta=1, tb=0, alpha=0.75, beta=0.5, epi=epi, splits=2,
                 cpad=4, seed=epi)


# ------------------------------------------------------------------------------------------------
# pre-split weight planes

def _split_planes(lib, L, weights, transpose):
    n = len(weights)
    wd = [_dev(w) for w in weights]
    planes = [torch.full((3 * w.size + 16,), 0x7fc0, dtype=torch.int16, device=DEV) for w in weights]
    L.check(lib.mrg_split_planes_batched(n, (VP * n)(*[VP(t.data_ptr()) for t in wd]),
                                         (VP * n)(*[VP(t.data_ptr()) for t in planes]),
                                         (CI * n)(*[w.shape[0] for w in weights]), (CI * n)(*[w.shape[1] for w in weights]),
                                         (CI * n)(*[int(transpose)] * n), _stream()), "split planes")
    torch.cuda.synchronize()
    return planes


@pytest.mark.parametrize("transpose", [0, 1])
def test_split_planes_reproduce_the_weight(transpose):
    """p0 + p1 + p2 = w to 2^-24 |w| in both orientations, at a 33 x 40 weight, +-0 and subnormals.  bf16
    cannot hold residuals below 2^-133 and fp32 subnormal residuals may be flushed, so an absolute
    2^-126 (the smallest normal fp32) is allowed on top: entries below 2^-102 are not resolved to 24 bits."""
    L, lib = _lib()
    rng = np.random.default_rng(transpose)
    ws = [rng.standard_normal((33, 40)).astype(np.float32), rng.standard_normal((64, 32)).astype(np.float32),
          (rng.standard_normal((5, 7)) * 1e30).astype(np.float32)]
    ws[0][0, :6] = np.array([0.0, -0.0, 1e-39, -3e-42, 2.0 ** -120, -2.0 ** -126], dtype=np.float32)
    planes = _split_planes(lib, L, ws, transpose)
    for w, p in zip(ws, planes):
        want = w.T if transpose else w
        ph = p.cpu()
        assert (ph[3 * w.size:] == 0x7fc0).all(), "wrote past the three planes"
        got = ph[:3 * w.size].view(torch.bfloat16).double().numpy().reshape(3, *want.shape)
        assert np.isfinite(got).all()
        err = np.abs(got.sum(0) - want.astype(np.float64))
        assert (err <= 2.0 ** -24 * np.abs(want) + 2.0 ** -126).all(), float((err / np.maximum(np.abs(want), 1e-300)).max())
        assert (got[0][want == 0] == 0).all()


@pytest.mark.parametrize("wide,route", [(0, "gemm_x6g_kernel"), (12, "gemm_x6w_kernel"), (22, "gemm_x6w_kernel")])
@pytest.mark.parametrize("M,N,K,epi,r0", [(1, 32, 32, 0, 0), (65, 64, 96, 1, 0), (2049, 260, 32, 2, 8),
                                          (65, 1024 + 4, 96, 3, 0), (65, 260, 96, 6, 0)])
def test_plane_products(M, N, K, epi, r0, wide, route, knobs):
    """mrg_gemm_x6_planes on each kernel mrg_gemm_set_wide selects; r0: B is a row slice of a taller
    weight's planes (as the Q and K, V blocks of in_proj_weight are)."""
    L, lib = _lib()
    knobs(mode=1, wide=wide)
    rng = np.random.default_rng([M, N, K, epi])
    A = R.make_operand(rng, M, K, pad=4, rdiv=13 if M > 13 else 0, shift=1, off=4)
    W = (rng.standard_normal((r0 + N + 3, K)) / math.sqrt(K)).astype(np.float32)
    planes = _split_planes(lib, L, [W], 0)[0]
    bias = rng.standard_normal(N).astype(np.float32)
    aux = R.make_aux(rng, epi, M, N) if epi in (2, 3) else None
    out = R.make_output(rng, M, N, pad=4, init=True)
    auxo = R.make_output(rng, M, N, pad=4, init=aux is not None) if epi >= 2 else None
    if aux is not None:
        auxo.buf[auxo.idx] = aux
    ref, bound, pre, pre_bound, _ = R.reference(A.vals, W[r0:r0 + N].T, 0.75, 0.5, out.c0, bias, epi, aux, "x6")
    Ad, bd = _dev(A.buf), _dev(bias)
    got = []
    for _ in range(2):
        Cd = _dev(out.buf)
        xd = None if auxo is None else _dev(auxo.buf)
        L.check(lib.mrg_gemm_x6_planes(M, N, K, 0.75, _p(Ad, A.off), A.ld, A.ld_hi, A.rdiv, _p(planes, r0 * K), K,
                                       W.size, 0.5, _p(Cd), out.ld, _p(bd), epi, _p(xd), out.ld, _stream()), "planes")
        assert lib.mrg_gemm_last_kernel().decode() == route
        torch.cuda.synchronize()
        got.append((_host(Cd), None if xd is None else _host(xd)))
    what = f"planes {route} wide={wide} {M}x{N}x{K}"
    ratio = R.check_output(got[0][0], out, ref, bound, what)
    if epi == 6:
        ratio = max(ratio, R.check_output(got[0][1], auxo, pre, pre_bound, what + " aux"))
    assert np.array_equal(got[0][0].view(np.int32), got[1][0].view(np.int32))
    _record(f"planes {route}", ratio)


@pytest.mark.parametrize("n", [1, 16])
def test_plane_products_batched(n, knobs):
    L, lib = _lib()
    knobs(mode=1)
    M, N, K, epi = 65, 260, 96, 3
    rng = np.random.default_rng(n)
    As = [R.make_operand(rng, M, K, pad=4) for _ in range(n)]
    Ws = [(rng.standard_normal((N, K)) / math.sqrt(K)).astype(np.float32) for _ in range(n)]
    planes = _split_planes(lib, L, Ws, 0)
    bias = [rng.standard_normal(N).astype(np.float32) for _ in range(n)]
    aux = [R.make_aux(rng, epi, M, N) for _ in range(n)]
    outs = [R.make_output(rng, M, N, pad=4, init=True) for _ in range(n)]
    Ad, bd = [_dev(x.buf) for x in As], [_dev(x) for x in bias]
    xd = [_dev(np.pad(x, ((0, 0), (0, 4)))) for x in aux]
    Cd = [_dev(o.buf) for o in outs]
    arr = lambda v: (VP * n)(*[VP(t.data_ptr()) for t in v])  # noqa: E731
    L.check(lib.mrg_gemm_x6_planes_batched(n, M, N, K, 0.75, arr(Ad), K + 4, arr(planes), K, N * K, 0.5, arr(Cd), N + 4,
                                           arr(bd), epi, arr(xd), N + 4, _stream()), "planes batched")
    assert lib.mrg_gemm_last_kernel() == b"gemm_x6w_kernel"
    torch.cuda.synchronize()
    for i in range(n):
        ref, bound, *_ = R.reference(As[i].vals, Ws[i].T, 0.75, 0.5, outs[i].c0, bias[i], epi, aux[i], "x6")
        _record("planes batched", R.check_output(_host(Cd[i]), outs[i], ref, bound, f"planes batched problem {i}"))


# ------------------------------------------------------------------------------------------------
# mrg_colsum_f32

@pytest.mark.parametrize("rows", [1, 63, 65, 64 * 9 + 1])
@pytest.mark.parametrize("N,beta,two,mapped", [(1, 0.0, False, False), (6, 1.0, True, True), (257, 0.0, True, True),
                                               (257, 1.0, False, False)])
def test_colsum(rows, N, beta, two, mapped):
    L, lib = _lib()
    rng = np.random.default_rng([rows, N])
    X = R.make_operand(rng, rows, N, pad=3, rdiv=5 if mapped else 0, shift=2, off=1)
    out0 = rng.standard_normal(N).astype(np.float32)
    outs = [R.make_output(rng, 1, N, pad=0) for _ in range(2 if two else 1)]
    for o in outs:
        if beta != 0.0:
            o.buf[o.idx] = out0
    ws_n = lib.mrg_colsum_workspace_bytes(rows, N) // 4
    Xd = _dev(X.buf)
    od = [_dev(o.buf) for o in outs]
    wsd = _dev(R.sentinel_f32(ws_n + WS_GUARD))
    L.check(lib.mrg_colsum_f32(rows, N, _p(Xd, X.off), X.ld, X.ld_hi, X.rdiv, beta, _p(od[0]),
                               _p(od[1]) if two else None, _p(wsd), _stream()), "colsum")
    torch.cuda.synchronize()
    ref, bound = R.colsum_reference(X.vals, beta, out0)
    for o, g in zip(outs, od):
        _record("colsum", R.check_output(_host(g), o, ref[None, :], bound[None, :], f"colsum {rows}x{N}"))
    R.check_guard(_host(wsd)[ws_n:], "colsum workspace guard")


# ------------------------------------------------------------------------------------------------
# argument checks: refused before any launch, with a message, the output untouched

def test_argument_checks_refuse_before_launch(knobs):
    L, lib = _lib()
    knobs(mode=1)
    M, N, K = 65, 64, 32
    a = torch.zeros(M * K + 8, device=DEV)
    b = torch.zeros(N * K + 8, device=DEV)
    planes = torch.zeros(3 * N * K + 8, dtype=torch.int16, device=DEV)
    c = _dev(R.sentinel_f32(M * N))
    ws = _dev(R.sentinel_f32(4 * M * N))
    S = _stream()
    one = lambda t: (VP * 1)(VP(t.data_ptr()))  # noqa: E731

    def f32(M=M, N=N, K=K, epi=0, aux=None, ws=None, splits=1):
        return lib.mrg_gemm_f32_ex(M, N, K, 1.0, _p(a), 0, K, 0, 0, _p(b), 1, K, 0, 0, 0.0, _p(c), N, None, epi, aux, N,
                                   ws, splits, None, None, 0.0, None, S)

    def planes_(K=K, epi=0, aoff=0, lda=K, ldb=K):
        return lib.mrg_gemm_x6_planes(M, N, K, 1.0, _p(a, aoff), lda, 0, 0, _p(planes), ldb, N * K, 0.0, _p(c), N, None,
                                      epi, None, N, S)

    def batched(n=1, epi=0):
        return lib.mrg_gemm_x6g_batched(n, M, N, K, 1.0, one(a), K, one(b), K, 0.0, one(c), N, None, epi, None, N, 0, S)

    def planes_batched(n=1, K=K, epi=0):
        return lib.mrg_gemm_x6_planes_batched(n, M, N, K, 1.0, one(a), K, one(planes), K, N * K, 0.0, one(c), N, None,
                                              epi, None, N, S)
    refused = {
        "split-K without a workspace": (lambda: f32(splits=2), b"mrg_gemm_f32"),
        "epilogue 2 without aux": (lambda: f32(epi=2), b"mrg_gemm_f32"),
        "epilogue 7 without aux": (lambda: f32(epi=7), b"mrg_gemm_f32"),
        "epilogue 8": (lambda: f32(epi=8), b"mrg_gemm_f32"),
        "negative size": (lambda: f32(K=-1), b"mrg_gemm_f32"),
        "planes with K % 32 != 0": (lambda: planes_(K=40), b"mrg_gemm_x6_planes"),
        "planes with epilogue 3 and no aux": (lambda: planes_(epi=3), b"mrg_gemm_x6_planes"),
        "planes with A off 16 B": (lambda: planes_(aoff=1), b"mrg_gemm_x6_planes"),
        "planes with lda % 4 != 0": (lambda: planes_(lda=K + 1), b"mrg_gemm_x6_planes"),
        "planes with ldb % 8 != 0": (lambda: planes_(ldb=K + 4), b"mrg_gemm_x6_planes"),
        "batched with n = 17": (lambda: batched(n=17), b"mrg_gemm_x6g_batched"),
        "batched with epilogue 5 and no aux": (lambda: batched(epi=5), b"mrg_gemm_x6g_batched"),
        "planes batched with n = 0": (lambda: planes_batched(n=0), b"mrg_gemm_x6_planes_batched"),
        "planes batched with K % 32 != 0": (lambda: planes_batched(K=48), b"mrg_gemm_x6_planes_batched"),
        "planes batched with epilogue 2 and no aux": (lambda: planes_batched(epi=2), b"mrg_gemm_x6_planes_batched"),
    }
    for what, (call, needle) in refused.items():
        assert call() != 0, what
        assert needle in lib.mrg_last_error(), (what, lib.mrg_last_error())
    before = read_knobs(lib)
    bad_knobs = {
        "mrg_gemm_set_mode(2)": lambda: lib.mrg_gemm_set_mode(2),
        "mrg_gemm_set_glds(1, 128)": lambda: lib.mrg_gemm_set_glds(1, 128),
        "mrg_gemm_set_glds(5, 128)": lambda: lib.mrg_gemm_set_glds(5, 128),
        "mrg_gemm_set_glds(2, 96)": lambda: lib.mrg_gemm_set_glds(2, 96),
        "mrg_gemm_force_tile(3)": lambda: lib.mrg_gemm_force_tile(3),
        "mrg_gemm_get_glds(null)": lambda: lib.mrg_gemm_get_glds(None, None),
        "mrg_lstm_set_mx(3, 0)": lambda: lib.mrg_lstm_set_mx(3, 0),
    }
    for what, call in bad_knobs.items():
        assert call() != 0, what
        assert what.split("(")[0].encode() in lib.mrg_last_error(), what
    prev = lib.mrg_gemm_set_wide(7)          # an unknown configuration is ignored, not stored
    assert lib.mrg_gemm_set_wide(prev) == prev
    assert read_knobs(lib) == before
    torch.cuda.synchronize()
    R.check_guard(_host(c), "output of refused calls")
    R.check_guard(_host(ws), "workspace of refused calls")
