"""The weight-gradient kernel's k loop (gemm_x6g_wgrad_kernel, csrc/gemm_glds.hip) at the edges of its
software pipeline: the MFMAs of one half k-step run beside the LDS reads and the bf16 split of the
next, across k-tile and ring-slot boundaries.

Every case calls Fn._wgrad with the side stream off and compares gw and gb with fp64
(gw0 + dY^T X, gb0 + sum dY) under the project's bound for these products, rel_err < 2e-6
(test_weight_grad_kernels_vs_fp64).  Shapes are the pipeline's, not the workload's: 1, 2, 3 and 5
k-tiles per K slice (prologue only, no steady state, odd and even tails), a short last slice, ragged
and exact tiles, the time-shifted RowMap operands, the bias-sum variants, the one-plane bf16 form and
a capped grid whose blocks walk several (tile, slice) items through one ring.
"""
import contextlib

import pytest
import torch

from tests.golden_util import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = 2e-6


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from multimodalreactiongeneration_amd import _lib as L
    L.load()
    yield
    from multimodalreactiongeneration_amd import functional as Fn
    torch.cuda.synchronize()
    Fn.check_errors()


@contextlib.contextmanager
def _forced_splits(splits, expect):
    """wgrad_splits answers `splits` (None: the project's own choice) for the one product `expect`."""
    from multimodalreactiongeneration_amd import gemm_ops   # _wgrad reads wgrad_splits there
    if splits is None:
        yield
        return
    orig, asked = gemm_ops.wgrad_splits, []
    gemm_ops.wgrad_splits = lambda *a: asked.append(a) or splits
    try:
        yield
    finally:
        gemm_ops.wgrad_splits = orig
    assert asked == [expect], "the product did not run with the forced split count"


def _run(dyp, xp, rows, N, In, gw0, gb0, splits, *, gb2_0=None, keep=(), **kw):
    """One Fn._wgrad call (side stream off) into fresh copies of gw0 / gb0 / gb2_0; returns them."""
    from multimodalreactiongeneration_amd import functional as Fn
    gw = gw0.to(DEV)
    gb = None if gb0 is None else gb0.to(DEV)
    gb2 = None if gb2_0 is None else gb2_0.to(DEV)
    prev = Fn.set_wgrad_stream(False)
    try:
        with _forced_splits(splits, (N, In, rows)):
            Fn._wgrad(dyp, N, xp, In, rows, N, In, gw, torch.device(DEV), gb=gb, gb2=gb2, keep=keep, **kw)
        torch.cuda.synchronize()
    finally:
        Fn.set_wgrad_stream(prev)
    return gw, gb, gb2


def _plain(rows, N, In, seed):
    g = torch.Generator().manual_seed(seed)
    dy, x = torch.randn(rows, N, generator=g), torch.randn(rows, In, generator=g)
    gw0, gb0 = torch.randn(N, In, generator=g), torch.randn(N, generator=g)
    return dy, x, gw0, gb0


def _check(gw, gb, dy, x, gw0, gb0):
    assert rel_err(gw, gw0.double() + dy.double().t() @ x.double()) < BOUND
    if gb is not None:
        assert rel_err(gb, gb0.double() + dy.double().sum(0)) < BOUND


# splits 4 over rows = 32 * 4 * n: n k-tiles per slice; 320 rows: slices of 3, 3, 3 and 1 k-tiles
# (the chunk rounds up to 96 rows); unsplit products over <= 64 rows take another kernel, so the unsplit
# case has 3 k-tiles
@pytest.mark.parametrize("rows,splits", [(128, 4), (64, 2), (256, 4), (384, 4), (640, 4), (320, 4), (96, 1)],
                         ids=["1tile", "1tile_2slices", "2tiles", "3tiles", "5tiles", "short_last_slice",
                              "3tiles_unsplit"])
def test_k_tiles_per_slice(rows, splits):
    from multimodalreactiongeneration_amd import functional as Fn
    N, In = 128, 256
    dy, x, gw0, gb0 = _plain(rows, N, In, rows + splits)
    dyd, xd = dy.to(DEV), x.to(DEV)
    gw, gb, _ = _run(Fn._ptr(dyd), Fn._ptr(xd), rows, N, In, gw0, gb0, splits, keep=(dyd, xd))
    _check(gw, gb, dy, x, gw0, gb0)


# the LDS-DMA kernel takes M, N >= 64 that are multiples of 4: ragged in both directions, ragged over
# more than one tile, one exact tile, and a half-filled row of tiles
@pytest.mark.parametrize("N,In", [(100, 68), (132, 260), (128, 128), (64, 256)])
@pytest.mark.parametrize("rows,splits", [(192, 2), (160, 1)], ids=["3tiles_x2", "5tiles"])
def test_ragged_tiles(N, In, rows, splits):
    from multimodalreactiongeneration_amd import functional as Fn
    dy, x, gw0, gb0 = _plain(rows, N, In, N + In + rows)
    dyd, xd = dy.to(DEV), x.to(DEV)
    gw, gb, _ = _run(Fn._ptr(dyd), Fn._ptr(xd), rows, N, In, gw0, gb0, splits, keep=(dyd, xd))
    _check(gw, gb, dy, x, gw0, gb0)


@pytest.mark.parametrize("splits", [1, 2, 4])
def test_time_shifted_rowmaps(splits):
    """dY = [:, 1:] and X = [:, :-1] of [B, T, F] tensors (the LSTM's dW_hh), B = 4, T = 33."""
    from multimodalreactiongeneration_amd import functional as Fn
    B, T, N, In = 4, 33, 132, 68
    g = torch.Generator().manual_seed(T + splits)
    dyf, xf = torch.randn(B, T, N, generator=g), torch.randn(B, T, In, generator=g)
    gw0, gb0 = torch.randn(N, In, generator=g), torch.randn(N, generator=g)
    dy, x = dyf[:, 1:].reshape(-1, N), xf[:, :-1].reshape(-1, In)
    dyd, xd = dyf.to(DEV), xf.to(DEV)
    kw = dict(dy_hi=T * N, dy_div=T - 1, x_hi=T * In, x_div=T - 1)
    gw, gb, _ = _run(Fn._ptr(dyd, N), Fn._ptr(xd), B * (T - 1), N, In, gw0, gb0, splits, keep=(dyd, xd), **kw)
    _check(gw, gb, dy, x, gw0, gb0)


@pytest.mark.parametrize("bias", ["gb2", "none"])
def test_bias_sum_variants(bias):
    """A second bias gradient fed by the same fused row sums, and no bias gradient at all."""
    from multimodalreactiongeneration_amd import functional as Fn
    rows, N, In, splits = 192, 256, 128, 2
    dy, x, gw0, gb0 = _plain(rows, N, In, 5 + len(bias))
    dyd, xd = dy.to(DEV), x.to(DEV)
    if bias == "gb2":
        gw, gb, gb2 = _run(Fn._ptr(dyd), Fn._ptr(xd), rows, N, In, gw0, gb0, splits, gb2_0=gb0 * 2, keep=(dyd, xd))
        _check(gw, gb, dy, x, gw0, gb0)
        assert rel_err(gb2, gb0.double() * 2 + dy.double().sum(0)) < BOUND
    else:
        gw, gb, _ = _run(Fn._ptr(dyd), Fn._ptr(xd), rows, N, In, gw0, None, splits, keep=(dyd, xd))
        assert gb is None
        _check(gw, None, dy, x, gw0, None)


@pytest.mark.parametrize("rows,splits", [(64, 2), (192, 2), (320, 4)])
def test_bf16_one_plane(rows, splits):
    """precision 'bf16' (NP = 1: one MFMA per block, almost no split to run beside it): fp64 on the
    bf16-rounded operands, as test_bf16_gemm_kernels_are_bf16_operands; the bias sums stay fp32."""
    from multimodalreactiongeneration_amd import functional as Fn
    N, In = 132, 128
    dy, x, gw0, gb0 = _plain(rows, N, In, rows)
    dyd, xd = dy.to(DEV), x.to(DEV)
    with Fn.precision("bf16"):
        gw, gb, _ = _run(Fn._ptr(dyd), Fn._ptr(xd), rows, N, In, gw0, gb0, splits, keep=(dyd, xd))
    r = lambda t: t.to(torch.bfloat16).double()   # noqa: E731
    assert rel_err(gw, gw0.double() + r(dy).t() @ r(x)) < BOUND
    assert rel_err(gb, gb0.double() + dy.double().sum(0)) < BOUND


def test_capped_grid_walks_items():
    """One block per CU and more than three (tile, slice) items per block: the ring and the epilogue
    stage are reused from item to item, each with its own prologue and tail (2 k-tiles here)."""
    from multimodalreactiongeneration_amd import functional as Fn, _lib as L
    lib = L.load()
    N = In = 512                                  # 16 tiles
    splits = -(-(3 * L.cu_count(0) + 1) // 16)    # > 3 items per block at one block per CU
    rows = 64 * splits
    dy, x, gw0, gb0 = _plain(rows, N, In, 11)
    dyd, xd = dy.to(DEV), x.to(DEV)
    prev = lib.mrg_gemm_set_blocks_per_cu(1)
    try:
        gw, gb, _ = _run(Fn._ptr(dyd), Fn._ptr(xd), rows, N, In, gw0, gb0, splits, keep=(dyd, xd))
    finally:
        lib.mrg_gemm_set_blocks_per_cu(prev)
    _check(gw, gb, dy, x, gw0, gb0)


@pytest.mark.parametrize("cap", [0, 1], ids=["uncapped", "capped"])
def test_same_call_twice_is_bitwise_equal(cap):
    from multimodalreactiongeneration_amd import functional as Fn, _lib as L
    lib = L.load()
    rows, N, In, splits = 8960, 260, 132, 56      # 5 k-tiles per slice, ragged tiles, 336 items
    dy, x, gw0, gb0 = _plain(rows, N, In, 13 + cap)
    dyd, xd = dy.to(DEV), x.to(DEV)
    prev = lib.mrg_gemm_set_blocks_per_cu(cap)
    try:
        outs = [_run(Fn._ptr(dyd), Fn._ptr(xd), rows, N, In, gw0, gb0, splits, keep=(dyd, xd)) for _ in range(2)]
    finally:
        lib.mrg_gemm_set_blocks_per_cu(prev)
    _check(outs[0][0], outs[0][1], dy, x, gw0, gb0)
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1])
