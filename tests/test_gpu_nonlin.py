"""The MLP mixer and the swish / tanh nonlinearities on the MI355X: GEMM epilogues 4..7 in every GEMM
kernel family against fp64, the activation-carrying feed-forward / chain functions against torch fp64
autograd, the elementwise activation kernel, the reference's goldens (train step, generation), the
fast-path gates, the Q7 sample-0 broadcast and graph capture.

Tolerance: TOL = 1e-4 on golden_util.rel_err (max-norm relative).  Under bf16 precision the bound is
applied against fp64 on the bf16-rounded operands (as test_bf16_gemm_kernels_are_bf16_operands does).
"""
import ctypes
import math

import pytest
import torch

from tests.golden_util import load, config, batch_from, prefixed, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = "cuda:0"
VP = ctypes.c_void_p


@pytest.fixture(scope="module", autouse=True)
def _done():
    yield
    from multimodalreactiongeneration_amd import functional as Fn
    torch.cuda.synchronize()
    Fn.check_errors()


@pytest.fixture(params=[1, 0], ids=["x6", "exact"])
def gemm_mode(request):
    from multimodalreactiongeneration_amd import _lib as L
    lib = L.load()
    old = lib.mrg_gemm_get_mode()
    L.check(lib.mrg_gemm_set_mode(request.param), "mode")
    yield request.param
    L.check(lib.mrg_gemm_set_mode(old), "mode")


def _p(t):
    return None if t is None else VP(t.data_ptr())


def _sig(x):
    return torch.sigmoid(x)


def _epi_ref(epi, v, aux):
    """fp64 epilogue of v (after alpha / bias); aux as the GEMM reads it."""
    if epi == 4:
        return torch.tanh(v)
    if epi == 5:
        return v * (1 - aux * aux)
    if epi == 6:
        return v * _sig(v)
    s = _sig(aux)
    return v * s * (1 + aux * (1 - s))


def _problem(M, N, K, epi, seed=0, n=1):
    """Operands with |v| spanning about +-4 (alpha = 2 on a unit-variance product plus a unit bias)."""
    g = torch.Generator().manual_seed(1000 * epi + M + N + K + seed)
    out = []
    for _ in range(n):
        A = torch.randn(M, K, generator=g).to(DEV)
        W = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(DEV)
        b = torch.randn(N, generator=g).to(DEV)
        aux = None
        if epi == 5:
            aux = torch.tanh(2 * torch.randn(M, N, generator=g)).to(DEV)
        elif epi == 7:
            aux = (2 * torch.randn(M, N, generator=g)).to(DEV)
        elif epi == 6:
            aux = torch.full((M, N), float("nan"), device=DEV)
        out.append((A, W, b, aux))
    return out


def _exact(A, W, b, aux, epi, bf16=False, alpha=2.0):
    if bf16:
        A, W = A.bfloat16().float(), W.bfloat16().float()
    v = alpha * (A.double().cpu() @ W.double().cpu().T) + b.double().cpu()
    return v, _epi_ref(epi, v, None if aux is None else aux.double().cpu())


def _check_epi(C, aux, A, W, b, aux_in, epi, bf16=False):
    v, exact = _exact(A, W, b, aux_in, epi, bf16)
    assert rel_err(C, exact) < TOL
    if epi == 6:
        assert rel_err(aux, v) < TOL   # the stored pre-activation


def _launches(fn):
    """Kernel launches the library made inside fn() (the per-launch probe of mrg_probe_*): tells a batched launch from
    a loop of single ones and the in-launch split-K combine from the separate reduce kernel."""
    from multimodalreactiongeneration_amd import _lib as L
    lib = L.load()
    L.check(lib.mrg_probe_start(64), "probe")
    lib.mrg_probe_tag(0)
    try:
        out = fn()
    finally:
        lib.mrg_probe_tag(-1)
        ms, tags = (ctypes.c_float * 64)(), (ctypes.c_int * 64)()
        n = lib.mrg_probe_stop(ms, tags, 64)
    assert n >= 0
    return out, n


def _single(lib, Fn, M, N, K, A, W, b, aux, epi, bf16=False, splits=1, counters=False):
    from multimodalreactiongeneration_amd import _lib as L
    C = torch.empty(M, N, device=DEV)
    ws = None
    if splits > 1:
        ws = torch.empty(lib.mrg_gemm_workspace_bytes(M, N, splits) // 4 + 4, device=DEV)
    fn = lib.mrg_gemm_bf16_ex if bf16 else lib.mrg_gemm_f32_ex
    L.check(fn(M, N, K, 2.0, _p(A), 0, K, 0, 0, _p(W), 1, K, 0, 0, 0.0, _p(C), N, _p(b), epi, _p(aux), N, _p(ws),
               splits, None, None, 0.0, _p(Fn._counters(torch.device(DEV))) if counters else None, Fn._stream()),
            "gemm")
    torch.cuda.synchronize()
    return C


# few-row (M <= 64 in x6 / bf16 mode: (3, 70, 300), (64, 6, 40), (37, 45, 53)), unaligned scalar epilogue of the tile
# kernels ((37, 45, 53) in exact mode, (70, 45, 53) in every mode), LDS-DMA / register-staged tiles
SHAPES = [(3, 70, 300), (64, 6, 40), (37, 45, 53), (70, 45, 53), (1000, 192, 96), (300, 64, 32), (130, 200, 520),
          (2100, 256, 64)]


@pytest.mark.parametrize("epi", [4, 5, 6, 7])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_epilogues_vs_fp64(M, N, K, epi, gemm_mode):
    from multimodalreactiongeneration_amd import _lib as L
    from multimodalreactiongeneration_amd import functional as Fn
    lib = L.load()
    (A, W, b, aux), = _problem(M, N, K, epi)
    aux_in = None if aux is None else aux.clone()
    C, n = _launches(lambda: _single(lib, Fn, M, N, K, A, W, b, aux, epi))
    assert n == 1   # unsplit: one kernel, the epilogue inside it
    _check_epi(C, aux, A, W, b, aux_in, epi)


@pytest.mark.parametrize("epi", [4, 5, 6, 7])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_epilogues_bf16_precision(M, N, K, epi):
    from multimodalreactiongeneration_amd import _lib as L
    from multimodalreactiongeneration_amd import functional as Fn
    lib = L.load()
    (A, W, b, aux), = _problem(M, N, K, epi, seed=1)
    aux_in = None if aux is None else aux.clone()
    C = _single(lib, Fn, M, N, K, A, W, b, aux, epi, bf16=True)
    # the few-row kernel (M <= 64, one K slice) is fp32 FMA chains under every precision (gemm.hip,
    # gemm_rows_kernel): its reference is fp64 on the operands as they are
    _check_epi(C, aux, A, W, b, aux_in, epi, bf16=M > 64)


@pytest.mark.parametrize("epi", [4, 5, 6, 7])
@pytest.mark.parametrize("counters", [True, False], ids=["in_launch_combine", "reduce_kernel"])
def test_epilogues_split_k(epi, counters, gemm_mode):
    """split-K = 4: the epilogue (and code 6's pre-activation store) runs once, on the reduced sum; with the
    per-tile tickets the last slice of a tile combines in the launch, without them the reduce kernel does."""
    from multimodalreactiongeneration_amd import _lib as L
    from multimodalreactiongeneration_amd import functional as Fn
    lib = L.load()
    M, N, K = 130, 200, 520
    (A, W, b, aux), = _problem(M, N, K, epi, seed=2)
    aux_in = None if aux is None else aux.clone()
    C, n = _launches(lambda: _single(lib, Fn, M, N, K, A, W, b, aux, epi, splits=4, counters=counters))
    _check_epi(C, aux, A, W, b, aux_in, epi)
    # x6 with tickets: the slices' launch combines; otherwise a reduce kernel follows it
    assert n == (1 if (counters and gemm_mode == 1) else 2)
    Cb = _single(lib, Fn, M, N, K, A, W, b, aux, epi, bf16=True, splits=4, counters=counters)
    _check_epi(Cb, aux, A, W, b, aux_in, epi, bf16=True)


def _planes(lib, Fn, W):
    from multimodalreactiongeneration_amd import _lib as L
    N, K = W.shape
    CI = ctypes.c_int
    planes = torch.empty(3, N, K, dtype=torch.int16, device=DEV)
    L.check(lib.mrg_split_planes_batched(1, (VP * 1)(_p(W)), (VP * 1)(_p(planes)), (CI * 1)(N), (CI * 1)(K),
                                         (CI * 1)(0), Fn._stream()), "split")
    return planes


@pytest.mark.parametrize("epi", [4, 5, 6, 7])
def test_epilogues_on_weight_planes_every_kernel(epi):
    """mrg_gemm_x6_planes through the LDS-DMA tile kernel (set_wide 0) and the row-owning kernel (12: 64
    columns, 22: 128 columns), at the smallest shape test_weight_plane_products_every_kernel uses."""
    from multimodalreactiongeneration_amd import _lib as L
    from multimodalreactiongeneration_amd import functional as Fn
    lib = L.load()
    M, N, K = 2100, 256, 512
    (A, W, b, aux), = _problem(M, N, K, epi, seed=3)
    aux_in = None if aux is None else aux.clone()
    planes = _planes(lib, Fn, W)
    prev = lib.mrg_gemm_set_wide(0)
    try:
        for cfg in (0, 12, 22):
            lib.mrg_gemm_set_wide(cfg)
            C = torch.empty(M, N, device=DEV)
            if epi == 6:
                aux.fill_(float("nan"))
            L.check(lib.mrg_gemm_x6_planes(M, N, K, 2.0, _p(A), K, 0, 0, _p(planes), K, N * K, 0.0, _p(C), N, _p(b),
                                           epi, _p(aux), N, Fn._stream()), "planes")
            torch.cuda.synchronize()
            _check_epi(C, aux, A, W, b, aux_in, epi)
    finally:
        lib.mrg_gemm_set_wide(prev)


@pytest.mark.parametrize("epi", [4, 5, 6, 7])
@pytest.mark.parametrize("M,N,K", [(100, 96, 40), (3840, 256, 256)])
def test_epilogues_batched_match_single(M, N, K, epi, gemm_mode):
    """mrg_gemm_x6g_batched with n = 2: each product (and code 6's stored pre-activation, through the per-problem aux
    pointer) bitwise the single launch.  (3840, 256, 256) in x6 mode is inside the batched LDS-DMA kernel (ONE launch
    for both products, counted); (100, 96, 40), and exact mode, run the products one by one (two launches)."""
    from multimodalreactiongeneration_amd import _lib as L
    from multimodalreactiongeneration_amd import functional as Fn
    lib = L.load()
    n = 2
    probs = _problem(M, N, K, epi, seed=4, n=n)
    Cs = [torch.empty(M, N, device=DEV) for _ in range(n)]
    auxb = None if probs[0][3] is None else [p[3].clone() for p in probs]
    arr = lambda v: (VP * n)(*[_p(t) for t in v])  # noqa: E731
    _, launches = _launches(lambda: L.check(lib.mrg_gemm_x6g_batched(
        n, M, N, K, 2.0, arr([p[0] for p in probs]), K, arr([p[1] for p in probs]), K, 0.0, arr(Cs), N,
        arr([p[2] for p in probs]), epi, None if auxb is None else arr(auxb), N, 0, Fn._stream()), "batched"))
    assert launches == (1 if (M >= 2048 and gemm_mode == 1) else n)
    for i, (A, W, b, aux) in enumerate(probs):
        aux_in = None if aux is None else aux.clone()
        ref = _single(lib, Fn, M, N, K, A, W, b, aux, epi)
        assert torch.equal(Cs[i], ref), i
        if epi == 6:
            assert torch.equal(auxb[i], aux), i
        _check_epi(Cs[i], auxb[i] if auxb else None, A, W, b, aux_in, epi)


@pytest.mark.parametrize("epi", [4, 5, 6, 7])
def test_epilogues_batched_planes_match_single(epi):
    from multimodalreactiongeneration_amd import _lib as L
    from multimodalreactiongeneration_amd import functional as Fn
    lib = L.load()
    n, M, N, K = 2, 2100, 64, 512
    probs = _problem(M, N, K, epi, seed=5, n=n)
    planes = [_planes(lib, Fn, p[1]) for p in probs]
    Cs = [torch.empty(M, N, device=DEV) for _ in range(n)]
    auxb = None if probs[0][3] is None else [p[3].clone() for p in probs]
    arr = lambda v: (VP * n)(*[_p(t) for t in v])  # noqa: E731
    L.check(lib.mrg_gemm_x6_planes_batched(n, M, N, K, 2.0, arr([p[0] for p in probs]), K, arr(planes), K, N * K, 0.0,
                                           arr(Cs), N, arr([p[2] for p in probs]), epi,
                                           None if auxb is None else arr(auxb), N, Fn._stream()), "batched planes")
    torch.cuda.synchronize()
    for i, (A, W, b, aux) in enumerate(probs):
        aux_in = None if aux is None else aux.clone()
        ref = torch.empty(M, N, device=DEV)
        L.check(lib.mrg_gemm_x6_planes(M, N, K, 2.0, _p(A), K, 0, 0, _p(planes[i]), K, N * K, 0.0, _p(ref), N, _p(b),
                                       epi, _p(aux), N, Fn._stream()), "planes")
        torch.cuda.synchronize()
        assert torch.equal(Cs[i], ref), i
        if epi == 6:
            assert torch.equal(auxb[i], aux), i
        _check_epi(Cs[i], auxb[i] if auxb else None, A, W, b, aux_in, epi)


# ------------------------------------------------------------------ functions vs torch fp64 autograd
_TORCH_ACT = {"relu": torch.relu, "tanh": torch.tanh, "silu": torch.nn.functional.silu}


def _leaf(t, dev, dtype):
    return t.detach().to(device=dev, dtype=dtype).requires_grad_(True)


def _compare(run, tensors, upstream):
    """run(list of leaf tensors) -> output; GPU fp32 vs CPU fp64: output and every input gradient."""
    got_in = [_leaf(t, DEV, torch.float32) for t in tensors]
    ref_in = [_leaf(t, "cpu", torch.float64) for t in tensors]
    y = run(got_in, True)
    y.backward(upstream.to(DEV))
    torch.cuda.synchronize()
    yr = run(ref_in, False)
    yr.backward(upstream.double())
    assert rel_err(y, yr) < TOL
    for i, (a, b) in enumerate(zip(got_in, ref_in)):
        if b.grad is None:   # an input this form does not use (the LayerNorm affine without the LayerNorm)
            assert a.grad is None, i
            continue
        assert rel_err(a.grad, b.grad) < TOL, i


@pytest.mark.parametrize("act", ["tanh", "silu"])
@pytest.mark.parametrize("M,E,Hb", [(600, 64, 16), (3000, 256, 64)])
@pytest.mark.parametrize("resln", [False, True])
def test_ffn_activations_vs_torch(M, E, Hb, act, resln, gemm_mode):
    from multimodalreactiongeneration_amd import functional as Fn
    g = torch.Generator().manual_seed(M + E + Hb)
    x = 1.5 * torch.randn(M, E, generator=g)
    w1, b1 = torch.randn(Hb, E, generator=g) / math.sqrt(E) * 2, torch.randn(Hb, generator=g)
    w2, b2 = torch.randn(E, Hb, generator=g) / math.sqrt(Hb), torch.randn(E, generator=g)
    gam, bet = 1 + 0.1 * torch.randn(E, generator=g), 0.1 * torch.randn(E, generator=g)
    up = torch.randn(M, E, generator=g)

    def run(t, gpu):
        x, w1, b1, w2, b2, gam, bet = t
        if gpu:
            if resln:
                return Fn.ffn_residual_layernorm(x, w1, b1, w2, b2, gam, bet, 1e-5, act)
            return Fn.ffn(x, w1, b1, w2, b2, act)
        z = _TORCH_ACT[act](x @ w1.T + b1) @ w2.T + b2
        return torch.nn.functional.layer_norm(z + x, (E,), gam, bet, 1e-5) if resln else z
    _compare(run, [x, w1, b1, w2, b2, gam, bet], up)


@pytest.mark.parametrize("act", ["relu", "tanh", "silu", None])
@pytest.mark.parametrize("depth", [1, 2, 3])
def test_mlp_chain_vs_torch(depth, act, gemm_mode):
    from multimodalreactiongeneration_amd import functional as Fn
    M, E = 600, 64
    g = torch.Generator().manual_seed(depth)
    x = 1.5 * torch.randn(M, E, generator=g)
    params = []
    for _ in range(depth + 1):
        params += [torch.randn(E, E, generator=g) / math.sqrt(E) * 1.5, torch.randn(E, generator=g)]
    up = torch.randn(M, E, generator=g)

    def run(t, gpu):
        x, ps = t[0], t[1:]
        layers = list(zip(ps[0::2], ps[1::2]))
        if gpu:
            return Fn.mlp_chain(x, layers, act)
        for i, (w, b) in enumerate(layers):
            x = x @ w.T + b
            if act is not None and i < len(layers) - 1:
                x = _TORCH_ACT[act](x)
        return x
    _compare(run, [x] + params, up)


@pytest.mark.parametrize("act", ["relu", "tanh", "silu"])
@pytest.mark.parametrize("n,offset", [(1, 0), (5, 0), (4096 + 3, 0), (4096 + 3, 1)])
def test_elementwise_activation(n, offset, act):
    """forward / backward over n floats; offset 1: a base pointer that is not 16-byte aligned."""
    from multimodalreactiongeneration_amd import functional as Fn
    g = torch.Generator().manual_seed(n + offset)
    x = 2 * torch.randn(n, generator=g)
    up = torch.randn(n, generator=g)
    buf = torch.empty(n + offset + 4, device=DEV)
    xg = buf[offset:offset + n].copy_(x).detach().requires_grad_(True)
    assert xg.data_ptr() % 16 == (4 * offset) % 16
    ubuf = torch.empty(n + offset + 4, device=DEV)
    ug = ubuf[offset:offset + n].copy_(up)
    y = Fn.activation(xg, act)
    y.backward(ug)
    torch.cuda.synchronize()
    xr = x.double().requires_grad_(True)
    yr = _TORCH_ACT[act](xr)
    yr.backward(up.double())
    assert rel_err(y, yr) < TOL and rel_err(xg.grad, xr.grad) < TOL


# ------------------------------------------------------------------ models vs the reference's goldens
NAMES = ["metaformer_mlp_swish_r2_pad", "metaformer_mlp_tanh_q7_r2_pad", "metaformer_lstm_swish_q7_r1"]


def _build(d):
    from multimodalreactiongeneration_amd.model import Metaformer
    cfg = config(d)
    m = Metaformer(cfg["model"], cfg["optim"], cfg["metrics"])
    m.load_state_dict(prefixed(d, "param/"))
    return m.to(DEV)


@pytest.mark.parametrize("name", NAMES)
def test_train_step_golden(name):
    from tests.test_gpu_models import _check, _check_after, _train_step
    d = load(name)
    m = _build(d)
    batch = batch_from(d, DEV)
    with torch.no_grad():
        m.eval()
        y_eval, _ = m.forward(*[(x.clone(), n) for x, n in batch[:-1]])
        assert rel_err(y_eval, d["y_eval"]) < TOL
        m.train()
        b2 = [(x.clone(), n) for x, n in batch]
        ms = b2[2][0]
        b2[2] = (ms * (ms != -100).float(), b2[2][1])
        y, _ = m.forward(*b2[:-1])
        assert rel_err(y, d["y"]) < TOL
    loss, opt = _train_step(m, batch)
    _check(d, m, loss)
    opt.step()
    torch.cuda.synchronize()
    _check_after(d, m)


@pytest.mark.parametrize("mode", ["full", "tf"])
def test_generation_golden(mode):
    d = load("metaformer_mlp_swish_gen_r2_pad")
    m = _build(d)
    m.eval()
    with torch.no_grad():
        pred, _ = m.prediction(batch_from(d, DEV), full_generation=(mode == "full"))
    torch.cuda.synchronize()
    assert rel_err(pred, d[f"pred/{mode}"]) < TOL


@pytest.mark.parametrize("name", NAMES + ["metaformer_gru_r2_pad"])
def test_fast_paths_decline(name):
    """Plan objects and flags, no kernel patched: the encoder stack and the batched first embedding (both behind
    _fast_eligible), the generation plan and, for the new models, the fused integrator all decline.  The GRU control
    keeps the fused integrator (its integrators are plain MHA + Linear): recorded.  The ssd_loop decode belongs to
    LSTMwithSample, which none of these configs build."""
    from multimodalreactiongeneration_amd.generate import plan_for
    from multimodalreactiongeneration_amd.model import Metaformer
    d = load(name)
    m = _build(d)
    mf = m.metaformer
    assert type(m) is Metaformer and not hasattr(m, "layerd_lstm")
    assert mf._fast_eligible() is False
    with torch.no_grad():
        assert plan_for(m) is None
    x = torch.zeros(4, 8, mf.hidden_dim, device=DEV)
    fused = [blk.integrator.fused_args(x, [x, x], [None, None], [None, None]) is not None
             for blk in mf.metaformer_blocks]
    assert mf._module_path_only() is (name in NAMES)
    assert fused == [name not in NAMES] * len(mf.metaformer_blocks)
    assert [blk.integrator.use_fused for blk in mf.metaformer_blocks] == fused


def test_q7_model_other_samples_do_not_reach_the_attention_branch():
    """The B = 3 tanh / Q7 model: perturbing only sample 1's main-modality input (motion_self and its lead, at the
    frames that are not padding) leaves the attention branch of EVERY integrator and block bitwise unchanged (it is
    sample 0's), while the model output of sample 1 changes.  The branch tensors are read with forward hooks."""
    from multimodalreactiongeneration_amd.model.mixers import MHAMixer
    d = load("metaformer_mlp_tanh_q7_r2_pad")
    m = _build(d)
    m.eval()
    mixers = [integ.mixer[0].mixer.module for blk in m.metaformer.metaformer_blocks for integ in blk.integrator.integrators]
    assert len(mixers) == 4 and all(isinstance(x, MHAMixer) and x.mixer[0].nonlinearity is not None for x in mixers)
    seen = []
    hooks = [x.register_forward_hook(lambda _m, _i, out: seen.append(out.detach().clone())) for x in mixers]
    try:
        batch = batch_from(d, DEV)
        with torch.no_grad():
            y0, _ = m.forward(*[(x.clone(), n) for x, n in batch[:-1]])
            first, seen = seen, []
            b2 = [(x.clone(), n) for x, n in batch]
            for i in (2, 5):
                x = b2[i][0]
                x[1] += 0.5 * (x[1] != -100).float()
            y1, _ = m.forward(*b2[:-1])
    finally:
        for h in hooks:
            h.remove()
    torch.cuda.synchronize()
    assert len(first) == len(seen) == 4
    for a, b in zip(first, seen):
        assert a.shape[0] == 3 and torch.equal(a, b)
        assert torch.equal(a[1], a[0]) and torch.equal(a[2], a[0])
    assert torch.equal(y0[0], y1[0]) and not torch.equal(y0[1], y1[1])


def test_q7_sample0_broadcast():
    """MHAMixer with a nonlinearity: the attention branch of EVERY sample is sample 0's
    activated attention output, so perturbing sample 1's query changes nothing and only sample 0's
    query / key-value receive a gradient; values against torch fp64."""
    from multimodalreactiongeneration_amd.model.mixers import MHAMixer
    B, T, E, H = 3, 8, 32, 4
    torch.manual_seed(5)
    mixer = MHAMixer(E, H, batch_first=True, nonlinearity="tanh").to(DEV)
    q = torch.randn(B, T, E, device=DEV, requires_grad=True)
    kv = torch.randn(B, T, E, device=DEV, requires_grad=True)
    up = torch.randn(B, T, E, device=DEV)
    out = mixer(q, kv, kv)
    assert mixer.fused_residual_ln(None, q, kv, kv) is None
    out.backward(up)
    torch.cuda.synchronize()
    q2 = q.detach().clone()
    q2[1] += 1.0
    with torch.no_grad():
        assert torch.equal(mixer(q2, kv, kv), out)
        q2[0] += 1.0
        assert not torch.equal(mixer(q2, kv, kv), out)
    assert torch.equal(out[1], out[0]) and torch.equal(out[2], out[0])
    assert q.grad[1:].abs().max().item() == 0 and kv.grad[1:].abs().max().item() == 0
    ref = torch.nn.MultiheadAttention(E, H, batch_first=True).double()
    mha = mixer.mixer[0].mha
    with torch.no_grad():
        ref.in_proj_weight.copy_(mha.in_proj_weight.double().cpu())
        ref.in_proj_bias.copy_(mha.in_proj_bias.double().cpu())
        ref.out_proj.weight.copy_(mha.out_proj.weight.double().cpu())
        ref.out_proj.bias.copy_(mha.out_proj.bias.double().cpu())
    qr = q.detach().double().cpu().requires_grad_(True)
    kr = kv.detach().double().cpu().requires_grad_(True)
    yr = torch.tanh(ref(qr, kr, kr, need_weights=False)[0])[0]
    (yr.unsqueeze(0).expand(B, T, E) * up.double().cpu()).sum().backward()
    assert rel_err(out[0], yr) < TOL
    assert rel_err(q.grad, qr.grad) < TOL and rel_err(kv.grad, kr.grad) < TOL


def test_mlp_swish_step_graph_replay_bitwise():
    from multimodalreactiongeneration_amd import functional as Fn
    from multimodalreactiongeneration_amd.graphs import capture
    d = load("metaformer_mlp_swish_r2_pad")
    m = _build(d)
    opt = m.configure_optimizers()["optimizer"]
    batch = batch_from(d, DEV)
    loss_buf = torch.zeros((), device=DEV)

    def step():
        opt.zero_grad()
        loss = m.training_step([(x.clone(), n) for x, n in batch])["loss"]
        loss.backward()
        loss_buf.copy_(loss.detach())
    step()
    torch.cuda.synchronize()
    ref, ref_loss = opt.flat_grad.clone(), loss_buf.clone()
    replay = capture(step, 1)
    for _ in range(2):
        opt.flat_grad.fill_(-1.0)
        loss_buf.fill_(-1.0)
        replay()
        torch.cuda.synchronize()
        Fn.check_errors()
        assert torch.equal(opt.flat_grad, ref) and torch.equal(loss_buf, ref_loss)
