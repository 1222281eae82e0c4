"""GEMM dispatch: everything between the launch plumbing and an op's products.  The split-K policy,
the weight-gradient products and where they run, the [in][out] weight copies of the input-gradient
products, and the pre-split bf16 weight planes."""
import ctypes
import os

import torch

from . import _lib
from .launch import _ARITH, _probe, _ptr, _stream, _ws, precision
from .wgrad_streams import on_side

_CNT = {}


def _counters(device) -> torch.Tensor:
    """Split-K tickets of the in-launch slab combine (mrg_gemm_f32_ex): zeroed once, every launch
    leaves them at zero again.  One buffer per (device, stream): launches on different streams
    (e.g. a weight-gradient product on the side stream) never share tickets."""
    key = (torch.device(device).index or 0, torch.cuda.current_stream(device).cuda_stream)
    if key not in _CNT:
        _CNT[key] = torch.zeros(4096, dtype=torch.int32, device=device)  # MRG_GEMM_COUNTERS
    return _CNT[key]


def gemm(M, N, K, A, transA, lda, B, transB, ldb, C, ldc, *, alpha=1.0, beta=0.0, bias=None,
         epi=0, aux=None, ldaux=0, a_hi=0, a_div=0, b_hi=0, b_div=0, splits=1, device=None,
         asum_out=None, asum_out2=None, asum_beta=1.0):
    """C = epi(alpha op(A) op(B) + beta C + bias); A/B/C/bias/aux are ctypes pointers.

    asum_out (optional ctypes pointer): += row sums of op(A) over k, i.e. the bias gradient of a
    weight-gradient GEMM dY^T X, fused into the GEMM (mrg_gemm_f32_ex)."""
    if M == 0 or N == 0:
        return
    lib = _lib.load()
    if splits == 1 and not transA:
        splits = act_splits(M, N, K)
    ws = None
    if splits > 1 or asum_out is not None:
        ws = _ws(lib.mrg_gemm_workspace_bytes(M, N, splits), device)
    fn = lib.mrg_gemm_bf16_ex if _ARITH[0] == "bf16" else lib.mrg_gemm_f32_ex
    with _probe("gemm", 2.0 * M * N * K):
        rc = fn(M, N, K, alpha, A, transA, lda, a_hi, a_div, B, transB, ldb, b_hi, b_div,
                                 beta, C, ldc, bias, epi, aux, ldaux, _ptr(ws), splits, asum_out, asum_out2,
                                 asum_beta, _ptr(_counters(device)) if splits > 1 else None, _stream())
    _lib.check(rc, "gemm")


def act_splits(M, N, K):
    """split-K factor for activation products with few output tiles (65..~2000 rows): a handful of
    64x64 tiles walking K >= 512 is latency-bound, so spread K over the CUs."""
    tiles = ((M + 63) // 64) * ((N + 63) // 64)
    if M <= 64 or tiles >= 64 or K < 512 or (_lib.load().mrg_gemm_get_mode() != 1 and _ARITH[0] is None):
        return 1  # M <= 64: the few-row kernel (gemm_rows_kernel) needs no split
    # <= 4 slices of 64x64 tiles: the slabs (<= 64 KB per tile) are combined in-launch
    return int(max(1, min(4, K // 64, 128 // tiles)))


# Workgroups a weight-gradient product aims at.  256 (half the split-K slices of round 2's 512): most
# products run beside a recurrence with the grid capped at one block per CU (wgrad_streams._DEFER), where fewer
# slices measured faster (tools/tools_wgrad_sweep.py, capped grid: LSTM dW 1024 x 256 102 -> 98 us at
# 16 instead of 32 slices, 256 x 256 41 -> 36 us at 64 instead of 128, 512 x 256 62 -> 55 us at 32
# instead of 64) and the slab reduce reads half the slabs: 22.93 -> 22.48 ms/step on one box (128:
# 23.7).  One target for every schedule, so the split (and the summation order) depends on the shape
# only and the side-stream / deferred schedules stay bitwise equal to the single-stream one.
_WG_TARGET = int(os.environ.get("MRG_WGRAD_TARGET_WG", "256"))


def wgrad_splits(M, N, K):
    """split-K factor for weight-gradient GEMMs (small M x N output, long B*T reduction).

    About _WG_TARGET workgroups: 128x128 tiles under the x6 arithmetic (chunks of >= 128 rows),
    64x64 tiles under exact f32 (chunks of >= 256 rows); tools/tools_gemm_sweep.py measured both.
    """
    if _lib.load().mrg_gemm_get_mode() == 1 or _ARITH[0] == "bf16":
        tiles = ((M + 127) // 128) * ((N + 127) // 128)
        s = max(1, _WG_TARGET // max(1, tiles))
        return int(max(1, min(s, K // 128, 128)))
    tiles = ((M + 63) // 64) * ((N + 63) // 64)
    s = max(1, 512 // max(1, tiles))
    return int(max(1, min(s, K // 256, 64)))


def colsum(rows, N, X, ld, out, *, out2=None, beta=1.0, ld_hi=0, rdiv=0, device=None):
    if N == 0:
        return
    lib = _lib.load()
    ws = _ws(lib.mrg_colsum_workspace_bytes(rows, N), device)
    _lib.check(lib.mrg_colsum_f32(rows, N, X, ld, ld_hi, rdiv, beta, out, out2, _ptr(ws), _stream()),
               "colsum")


# Every caller outside this module writes gemm_ops._on_side(...): replacing it here replaces it for all.
def _on_side(device, rows, keep, fn, writes=None):
    """fn() (weight-gradient launches) runs where wgrad_streams.on_side puts it, now or queued."""
    # under the precision active here: precision(...) as a decorator enters the context around each call
    on_side(device, rows, keep, precision(_ARITH[0])(fn), writes)


def _wgrad(dY, ldy, X, ldx, rows, Nout, Nin, gw, device, *, dy_hi=0, dy_div=0, x_hi=0, x_div=0, gb=None,
           gb2=None, keep=()):
    """gw[Nout, Nin] += sum_rows dY[row, :]^T X[row, :]; gb (and gb2) += sum_rows dY[row, :] (fused).

    keep: the tensors behind the dY / X pointers (side-stream lifetime, see wgrad_streams.side)."""
    def issue():
        if gw is None:
            if gb is not None:
                colsum(rows, Nout, dY, ldy, _ptr(gb), out2=_ptr(gb2), ld_hi=dy_hi, rdiv=dy_div, device=device)
            return
        gemm(Nout, Nin, rows, dY, 1, ldy, X, 0, ldx, _ptr(gw), Nin, beta=1.0, a_hi=dy_hi, a_div=dy_div,
             b_hi=x_hi, b_div=x_div, splits=wgrad_splits(Nout, Nin, rows), device=device,
             asum_out=_ptr(gb), asum_out2=_ptr(gb2))
    _on_side(device, rows, keep, issue, writes=(gw, gb, gb2))


# --- [in][out] weight copies for the input-gradient products.  dX = dY W reads W [out][in] along
# n (not k): the product runs as a k-contiguous one, dY (W^T)^T, on the LDS-DMA x6 kernel
# (gemm_glds.hip) when the weight's transposed copy exists.  The forwards note the weights of their
# large products (>= _WT_MIN_ROWS rows, >= 256 inputs); the backward's first use transposes every
# noted weight in ONE launch (mrg_transpose_batched) and later uses hit the cache.  A weight noted
# again (the next step's forward: the optimizer has rewritten it in place) drops its stale copy.
# MRG_DX_TRANSPOSED=0 keeps the [out][in] operand (the register-staged kernel's n-contiguous path).
_WT_ON = [os.environ.get("MRG_DX_TRANSPOSED", "1") != "0"]
_WT_MIN_ROWS = 2048
_WT_PENDING = {}
_WT_CACHE = {}


def set_dx_transposed(on: bool) -> bool:
    prev = _WT_ON[0]
    _WT_ON[0] = bool(on)
    return prev


def _wt_key(w):
    return (w.data_ptr(), tuple(w.shape))


def _wt_note(w, rows, need=True):
    """Forward side (inside autograd Function.forward: pass ctx.needs_input_grad of the input): w
    [out][in] (a contiguous 2-D view) will serve a dX product over `rows` rows."""
    if not (need and _WT_ON[0] and rows >= _WT_MIN_ROWS and w.shape[1] >= 256 and w.shape[0] % 32 == 0
            and w.is_contiguous()) or _plane_operand(w, True) is not None:
        return
    k = _wt_key(w)
    _WT_CACHE.pop(k, None)
    _WT_PENDING[k] = w


def _wt(w):
    """Backward side: the [in][out] copy of w, or None when w was not noted in this step's forward.
    Copies are valid only within the backward pass (autograd graph task) that made them: a copy keyed
    by a pointer that a later model reuses, or made before an optimizer step, is never handed out."""
    k = _wt_key(w)
    task = torch._C._current_graph_task_id()
    t = _WT_CACHE.get(k)
    if t is not None and t[0] == task:
        return t[1]
    if k not in _WT_PENDING:
        return None
    items = list(_WT_PENDING.values())
    _WT_PENDING.clear()
    outs = [torch.empty(x.shape[1], x.shape[0], device=x.device, dtype=torch.float32) for x in items]
    n = len(items)
    VP = ctypes.c_void_p
    _lib.check(_lib.load().mrg_transpose_batched(
        n, (VP * n)(*[_ptr(x) for x in items]), (VP * n)(*[_ptr(o) for o in outs]),
        (ctypes.c_int * n)(*[x.shape[0] for x in items]), (ctypes.c_int * n)(*[x.shape[1] for x in items]),
        _stream()), "transpose")
    for x, o in zip(items, outs):
        _WT_CACHE[_wt_key(x)] = (task, o)
    return _WT_CACHE[k][1]


# --- pre-split weights: the three bf16 planes of every weight (and of its transpose), made once per
# optimizer step in ONE launch (mrg_split_planes_batched) by prepare_weight_planes at the start of a
# training forward; the forward products x W^T and the input-gradient products dY W then run on the
# LDS-DMA x6 kernel with only the activation operand split in the loop (mrg_gemm_x6_planes).  Keyed
# by the weight's storage; a row slice of a prepared weight (the Q / K,V blocks of in_proj_weight)
# resolves to its parent's planes.  On by default (MRG_WEIGHT_PLANES=0 / set_weight_planes(False) turns
# it off): with the row-owning kernel (gemm_wide.hip) and the batched plane products the headline step
# is 0.55 ms faster with it (21.10 -> 20.55 ms, A/B on one box).
_PL_ON = [os.environ.get("MRG_WEIGHT_PLANES", "1") == "1"]
_PLANES = {}


def set_weight_planes(on: bool) -> bool:
    prev = _PL_ON[0]
    _PL_ON[0] = bool(on)
    if not on:
        _PLANES.clear()
    return prev


def invalidate_weight_planes():
    """The weights changed (optimizer step): forget their planes and their [in][out] copies (_WT_CACHE)
    until the next forward notes them again, so no backward can use a transpose of old weights."""
    _PLANES.clear()
    _WT_CACHE.clear()
    _WT_PENDING.clear()


def prepare_weight_planes(weights):
    """Split every 2-D fp32 weight (rows and cols multiples of 32... any size) into bf16 planes, both
    orientations, in one launch.  Called per step before the forward (the optimizer rewrote them)."""
    _PLANES.clear()
    if not (_PL_ON[0] and _ARITH[0] is None and _lib.load().mrg_gemm_get_mode() == 1):
        return
    ws = [w for w in weights if w.dim() == 2 and w.is_cuda and w.dtype == torch.float32 and w.is_contiguous()
          and min(w.shape) >= 32]
    if not ws:
        return
    srcs, dsts, rows, cols, trs = [], [], [], [], []
    for w in ws:
        O, I = w.shape
        pw = torch.empty(3, O, I, device=w.device, dtype=torch.int16)
        pt = torch.empty(3, I, O, device=w.device, dtype=torch.int16)
        _PLANES[w.data_ptr()] = (w, pw, pt, w._version)
        for dst, tr in ((pw, 0), (pt, 1)):
            srcs.append(_ptr(w)); dsts.append(_ptr(dst)); rows.append(O); cols.append(I); trs.append(tr)
    n = len(srcs)
    VP, CI = ctypes.c_void_p, ctypes.c_int
    _lib.check(_lib.load().mrg_split_planes_batched(n, (VP * n)(*srcs), (VP * n)(*dsts), (CI * n)(*rows),
                                                    (CI * n)(*cols), (CI * n)(*trs), _stream()), "split planes")


def _plane_operand(w, transposed):
    """(pointer, ldb, plane stride) of the planes of w (or of w^T), w a prepared weight or a row slice
    of one; None when w has no planes."""
    if not _PLANES:
        return None
    ent = _PLANES.get(w.data_ptr())
    r0 = 0
    if ent is None or ent[0].shape[1] != w.shape[1]:
        ent = None
        for cand in _PLANES.values():
            par = cand[0]
            off = w.data_ptr() - par.data_ptr()
            if par.shape[1] == w.shape[1] and 0 <= off < par.numel() * 4 and off % (4 * par.shape[1]) == 0:
                ent, r0 = cand, off // (4 * par.shape[1])
                break
        if ent is None:
            return None
    par, pw, pt, ver = ent
    if par._version != ver:   # rewritten through torch since the split: stale
        return None
    O, I = par.shape
    if not transposed:   # rows r0.. of W: [rows][I]
        return ctypes.c_void_p(pw.data_ptr() + 2 * r0 * I), I, O * I
    return ctypes.c_void_p(pt.data_ptr() + 2 * r0), O, I * O   # columns r0.. of W^T: [I][O]


def _planes_gemm(M, N, K, A, lda, planes, C, ldc, *, beta=0.0, bias=None, epi=0, aux=None, ldaux=0, a_hi=0,
                 a_div=0, device=None):
    bp, ldb, bplane = planes
    with _probe("gemm", 2.0 * M * N * K):
        rc = _lib.load().mrg_gemm_x6_planes(M, N, K, 1.0, A, lda, a_hi, a_div, bp, ldb, bplane, beta, C, ldc, bias,
                                           epi, aux, ldaux, _stream())
    _lib.check(rc, "gemm (weight planes)")


def planes_batched(M, N, K, items, lda, ldc, *, epi=0, ldaux=0, beta=0.0, transposed=False):
    """Same-shape products C_p = epi(A_p w_p^T ...) (transposed: dY_p w_p, on the planes of w_p^T) in ONE
    launch on the weights' pre-split planes (mrg_gemm_x6_planes_batched); items = [(A ptr, w, C ptr,
    bias ptr | None, aux ptr | None)].  Returns False (nothing launched) when a weight has no planes
    or the planes' strides differ, so the caller takes its fp32-operand path."""
    if not (M >= _WT_MIN_ROWS and K % 32 == 0 and _ARITH[0] is None and 0 < len(items) <= 16):
        return False
    pls = [_plane_operand(w, transposed) for _, w, _, _, _ in items]
    if any(p is None for p in pls) or len({(p[1], p[2]) for p in pls}) != 1:
        return False
    n, VP = len(items), ctypes.c_void_p
    arr = lambda xs: (VP * n)(*xs)  # noqa: E731
    with _probe("gemm", 2.0 * M * N * K * n):
        rc = _lib.load().mrg_gemm_x6_planes_batched(
            n, M, N, K, 1.0, arr([it[0] for it in items]), lda, arr([p[0] for p in pls]), pls[0][1], pls[0][2], beta,
            arr([it[2] for it in items]), ldc, None if all(it[3] is None for it in items) else arr([it[3] for it in items]),
            epi, None if all(it[4] is None for it in items) else arr([it[4] for it in items]), ldaux, _stream())
    _lib.check(rc, "batched gemm (weight planes)")
    return True


def _fwd_gemm(M, N, K, A, lda, w, C, ldc, **kw):
    """C[M, N] = epi(A[M, K] w[N, K]^T ...): on the weight planes when w has them."""
    pl = _plane_operand(w, False) if (M >= _WT_MIN_ROWS and K % 32 == 0 and _ARITH[0] is None) else None
    if pl is not None:
        kw.pop("device", None)
        _planes_gemm(M, N, K, A, lda, pl, C, ldc, **kw)
    else:
        gemm(M, N, K, A, 0, lda, _ptr(w), 1, K, C, ldc, **kw)


def _dx_gemm(M, In, N, dY, ldy, w, dx, ldx, **kw):
    """dx[M, In] = epi(dY[M, N] w[N, In] ...): on the planes of w^T, else through w's [in][out] copy
    when one exists, else reading w along n."""
    if M >= _WT_MIN_ROWS and N % 32 == 0 and _ARITH[0] is None:
        pl = _plane_operand(w, True)
        if pl is not None:
            kw.pop("device", None)
            _planes_gemm(M, In, N, dY, ldy, pl, dx, ldx, **kw)
            return
    wt = _wt(w) if M >= _WT_MIN_ROWS else None
    if wt is not None:
        gemm(M, In, N, dY, 0, ldy, _ptr(wt), 1, N, dx, ldx, **kw)
    else:
        gemm(M, In, N, dY, 0, ldy, _ptr(w), 0, In, dx, ldx, **kw)
