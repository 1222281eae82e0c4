"""The dense autograd Functions: Linear, the feed-forward forms, residual LayerNorm, the MLP chain, the
elementwise activation and the sample-0 broadcast."""
import torch
from torch.autograd import Function

from . import _lib, gemm_ops
from .gemm_ops import _dx_gemm, _fwd_gemm, _wgrad, _wt_note, colsum, gemm
from .launch import _gbuf, _keeps_precision, _ptr, _stream, _ws, zeros


def _rows(x, In):
    """x as contiguous [rows, In]."""
    _lib.require_device(x)
    return x.reshape(-1, In).contiguous()


def _dx(ctx, g, w, residual=None):
    """The input gradient g[M, N] w[N, In] in x's shape, None when x needs none.  residual [M, In]:
    the gradient of a residual branch around the op, added by the GEMM's epilogue (3), so the add
    autograd would run for the two uses of x disappears."""
    if not ctx.needs_input_grad[0]:
        return None
    M, (N, In) = g.shape[0], w.shape
    dx = torch.empty(M, In, device=g.device, dtype=torch.float32)
    kw = {} if residual is None else dict(epi=3, aux=_ptr(residual), ldaux=In)
    _dx_gemm(M, In, N, _ptr(g), N, w, _ptr(dx), In, device=g.device, **kw)
    return dx.view(ctx.xshape)


# ------------------------------------------------------------------ residual + LayerNorm
def _resln_fwd(a2, b2, gamma, beta, eps):
    """u = LN(a + b) over [rows, E] (both contiguous); returns (u, mean, rstd)."""
    rows, E = a2.shape
    dev = a2.device
    y = torch.empty_like(a2)
    mean = torch.empty(rows, device=dev, dtype=torch.float32)
    rstd = torch.empty(rows, device=dev, dtype=torch.float32)
    _lib.check(_lib.load().mrg_residual_layernorm_fwd(rows, E, _ptr(a2), _ptr(b2), _ptr(gamma), _ptr(beta), eps,
                                                      _ptr(y), _ptr(mean), _ptr(rstd), _stream()), "layernorm fwd")
    return y, mean, rstd


def _resln_bwd(dy2, a2, b2, gamma, beta, mean, rstd):
    """g = dL/d(a + b) of u = LN(a + b); dgamma / dbeta accumulate into the parameters' grads."""
    rows, E = a2.shape
    dev = a2.device
    g = torch.empty_like(a2)
    lib = _lib.load()
    ws = _ws(lib.mrg_residual_layernorm_bwd_workspace_bytes(rows, E), dev)
    gg, gb = _gbuf(gamma), _gbuf(beta)
    _lib.check(lib.mrg_residual_layernorm_bwd(
        rows, E, _ptr(dy2), _ptr(a2), _ptr(b2), _ptr(gamma), _ptr(mean), _ptr(rstd), _ptr(g),
        None, None, 1, _ptr(ws), _stream()), "layernorm bwd")
    if gg is not None or gb is not None:
        # dgamma / dbeta from the per-block partials: parameter gradients, off the critical path
        def reduce():
            scratch = None
            if gg is None or gb is None:
                scratch = _ws(2 * E * 4, dev).view(2, E)
            _lib.check(lib.mrg_residual_layernorm_param_reduce(
                rows, E, _ptr(ws), _ptr(gg if gg is not None else scratch[0]),
                _ptr(gb if gb is not None else scratch[1]), 1, _stream()), "layernorm param reduce")
        gemm_ops._on_side(dev, rows, (ws,), reduce, writes=(gg, gb))
    return g


class _ResLNFn(Function):
    @staticmethod
    @_keeps_precision
    def forward(ctx, a, b, gamma, beta, eps):
        E = a.shape[-1]
        a2, b2 = _rows(a, E), b.reshape(-1, E).contiguous()
        y, mean, rstd = _resln_fwd(a2, b2, gamma, beta, eps)
        ctx.save_for_backward(a2, b2, gamma, beta, mean, rstd)
        ctx.shape = a.shape
        return y.view(a.shape)

    @staticmethod
    @_keeps_precision
    def backward(ctx, dy):
        a2, b2, gamma, beta, mean, rstd = ctx.saved_tensors
        dy2 = dy.reshape(-1, a2.shape[1]).contiguous()
        dx = _resln_bwd(dy2, a2, b2, gamma, beta, mean, rstd).view(ctx.shape)
        return dx, dx, None, None, None


def residual_layernorm(y, x, gamma, beta, eps=1e-5):
    """LayerNorm(y + x) — ResidualConnection with use_layer_norm (residual_connection.py:29-31)."""
    return _ResLNFn.apply(y, x, gamma, beta, eps)


# ------------------------------------------------------------------ residual without LayerNorm
def _residual_add_launch(a, b, out):
    """out = a + b over contiguous fp32 tensors of one size (out may be a)."""
    _lib.check(_lib.load().mrg_residual_add(a.numel(), _ptr(a), _ptr(b), _ptr(out), _stream()), "residual add")
    return out


class _ResAddFn(Function):
    @staticmethod
    @_keeps_precision
    def forward(ctx, y, x):
        yc, xc = y.contiguous(), x.contiguous()
        return _residual_add_launch(yc, xc, torch.empty_like(yc))

    @staticmethod
    @_keeps_precision
    def backward(ctx, dy):
        return dy, dy


def residual_add(y, x, inplace=False):
    """y + x — ResidualConnection without a LayerNorm (residual_connection.py:29-37) where no GEMM
    epilogue carries the add; the gradient goes to both operands as it is.  inplace: write the sum
    over y when nothing can read y again, which holds only outside autograd (a recurrence keeps its
    output for the backward's recurrent weight gradient); under autograd a new tensor is returned."""
    _lib.require_device(y)
    if y.shape != x.shape:
        raise ValueError(f"residual_add: shapes differ, {tuple(y.shape)} and {tuple(x.shape)}")
    if y.dtype != torch.float32 or x.dtype != torch.float32:
        raise ValueError("residual_add: float32 tensors required")
    if inplace and y.is_contiguous() and not (torch.is_grad_enabled() and (y.requires_grad or x.requires_grad)):
        return _residual_add_launch(y, x.contiguous(), y)
    return _ResAddFn.apply(y, x)


# ------------------------------------------------------------------ Linear, alone and under LN(. + x)
def _linear_fwd(ctx, x2, w, b, residual=None):
    """x2 w^T + b (+ residual [M, N] by the GEMM's epilogue 3); w is noted for the backward's
    input-gradient product."""
    M, (N, In) = x2.shape[0], w.shape
    y = torch.empty(M, N, device=x2.device, dtype=torch.float32)
    kw = {} if residual is None else dict(epi=3, aux=_ptr(residual), ldaux=N)
    _fwd_gemm(M, N, In, _ptr(x2), In, w, _ptr(y), N, bias=_ptr(b), device=x2.device, **kw)
    _wt_note(w, M, ctx.needs_input_grad[0])
    return y


def _linear_bwd(ctx, g, x2, w, b, residual=None):
    """dW += g^T x2, db += colsum g; returns _dx."""
    M, (N, In) = g.shape[0], w.shape
    _wgrad(_ptr(g), N, _ptr(x2), In, M, N, In, _gbuf(w), g.device, gb=_gbuf(b), keep=(g, x2))
    return _dx(ctx, g, w, residual)


class _LinearFn(Function):
    @staticmethod
    @_keeps_precision
    def forward(ctx, x, w, b):
        x2 = _rows(x, w.shape[1])
        y = _linear_fwd(ctx, x2, w, b)
        ctx.save_for_backward(x2, w, b)
        ctx.xshape = x.shape
        return y.view(*x.shape[:-1], w.shape[0])

    @staticmethod
    @_keeps_precision
    def backward(ctx, dy):
        x2, w, b = ctx.saved_tensors
        return _linear_bwd(ctx, dy.reshape(-1, w.shape[0]).contiguous(), x2, w, b), None, None


def linear(x, weight, bias=None):
    return _LinearFn.apply(x, weight, bias)


class _LinResLNFn(Function):
    """LN(x W^T + b + x): FeedForward(nonlinearity none, residual, LN) (mixer_block.py:63-83)."""

    @staticmethod
    @_keeps_precision
    def forward(ctx, x, w, b, gamma, beta, eps):
        x2 = _rows(x, w.shape[0])
        z = _linear_fwd(ctx, x2, w, b)
        y, mean, rstd = _resln_fwd(z, x2, gamma, beta, eps)
        ctx.save_for_backward(x2, w, b, z, gamma, beta, mean, rstd)
        ctx.xshape = x.shape
        return y.view(x.shape)

    @staticmethod
    @_keeps_precision
    def backward(ctx, dy):
        x2, w, b, z, gamma, beta, mean, rstd = ctx.saved_tensors
        g = _resln_bwd(dy.reshape(x2.shape).contiguous(), z, x2, gamma, beta, mean, rstd)
        return _linear_bwd(ctx, g, x2, w, b, residual=g), None, None, None, None, None


def linear_residual_layernorm(x, weight, bias, gamma, beta, eps=1e-5):
    return _LinResLNFn.apply(x, weight, bias, gamma, beta, eps)


def _square(w, what):
    if w.shape[0] != w.shape[1]:
        raise ValueError(f"{what}: the residual needs equal input and output sizes, got weight {tuple(w.shape)}")


class _LinResFn(Function):
    """x W^T + b + x: FeedForward(nonlinearity none, residual, no LN) (mixer_block.py:63-83).  The
    forward GEMM adds x and the input-gradient GEMM adds dy, both by epilogue 3: no add launch and
    no [rows, E] intermediate in either direction."""

    @staticmethod
    @_keeps_precision
    def forward(ctx, x, w, b):
        x2 = _rows(x, w.shape[1])
        y = _linear_fwd(ctx, x2, w, b, residual=x2)
        ctx.save_for_backward(x2, w, b)
        ctx.xshape = x.shape
        return y.view(x.shape)

    @staticmethod
    @_keeps_precision
    def backward(ctx, dy):
        x2, w, b = ctx.saved_tensors
        g = dy.reshape(x2.shape).contiguous()
        return _linear_bwd(ctx, g, x2, w, b, residual=g), None, None


def linear_residual(x, weight, bias=None):
    _square(weight, "linear_residual")
    return _LinResFn.apply(x, weight, bias)


class _LinAddFn(Function):
    """h W^T + b + r with r in the output's shape: the last Linear of a module under a residual
    connection without LayerNorm whose skip operand r is not that Linear's input (the mixing Linear
    of LSTMModule, the projection of MultiModalAttentionBlockSequential).  r is added by the forward
    GEMM's epilogue 3; its gradient is dy as it is."""

    @staticmethod
    @_keeps_precision
    def forward(ctx, h, w, b, r):
        h2 = _rows(h, w.shape[1])
        r2 = r.reshape(-1, w.shape[0]).contiguous()
        y = _linear_fwd(ctx, h2, w, b, residual=r2)
        ctx.save_for_backward(h2, w, b)
        ctx.xshape = h.shape
        return y.view(r.shape)

    @staticmethod
    @_keeps_precision
    def backward(ctx, dy):
        h2, w, b = ctx.saved_tensors
        g = dy.reshape(-1, w.shape[0]).contiguous()
        return _linear_bwd(ctx, g, h2, w, b), None, None, (dy if ctx.needs_input_grad[3] else None)


def linear_add(h, weight, bias, r):
    """linear(h) + r, r [..., out]; the add is the GEMM's epilogue."""
    if tuple(r.shape) != (*h.shape[:-1], weight.shape[0]):
        raise ValueError(f"linear_add: r {tuple(r.shape)} is not the output's shape "
                         f"{(*h.shape[:-1], weight.shape[0])}")
    _lib.require_device(r)
    return _LinAddFn.apply(h, weight, bias, r)


# ------------------------------------------------------------------ FFN (Linear -> act -> Linear)
# Test hook (None in the product path): when a dict, every FFN forward stores the ReLU's side per
# element, {w1.data_ptr(): bool [..., Hb] (pre-activation > 0)}, so a test can evaluate the float64
# oracle at exactly this forward's kinks (oracle.RELU_MASKS; tests/test_gpu_models.py).
RELU_TAP = None


def _tap_relu(w1, h, lead_shape):
    if RELU_TAP is not None:
        RELU_TAP[w1.data_ptr()] = (h > 0).view(*lead_shape, h.shape[-1])


# Activations of the fused feed-forward forms: name -> (forward epilogue, backward epilogue, kind of
# mrg_activation_fwd / _bwd).  relu and tanh differentiate from the saved output h; silu's forward
# epilogue also stores the pre-activation (GEMM epilogue 6 writes it through aux) and its
# derivative reads that.
ACTIVATIONS = {"relu": (1, 2, 1), "tanh": (4, 5, 2), "silu": (6, 7, 3)}


def _act_codes(act):
    if act not in ACTIVATIONS:
        raise ValueError(f"activation must be one of {sorted(ACTIVATIONS)}, got {act!r}")
    return ACTIVATIONS[act]


def _act_fwd_gemm(M, Hb, In, x2, w1, b1, fe, dev):
    """(h, pre): h = act(x2 w1^T + b1) by forward epilogue fe; pre = the pre-activation (silu) or None."""
    h = torch.empty(M, Hb, device=dev, dtype=torch.float32)
    pre = torch.empty(M, Hb, device=dev, dtype=torch.float32) if fe == 6 else None
    gemm(M, Hb, In, _ptr(x2), 0, In, _ptr(w1), 1, In, _ptr(h), Hb, bias=_ptr(b1), epi=fe, aux=_ptr(pre),
         ldaux=Hb if pre is not None else 0, device=dev)
    return h, pre


def _ffn_fwd(ctx, x, w1, b1, w2, b2, act, residual=False):
    """(x2, h, pre, z): z = act(x2 w1^T + b1) w2^T + b2 over x's rows (residual: + x2, by the second
    GEMM's epilogue 3).  Only w1 is noted: the dh product reads w2 through gemm directly."""
    fe, ctx.be, _ = _act_codes(act)
    (Hb, In), N = w1.shape, w2.shape[0]
    x2 = _rows(x, In)
    M, dev = x2.shape[0], x.device
    h, pre = _act_fwd_gemm(M, Hb, In, x2, w1, b1, fe, dev)
    z = torch.empty(M, N, device=dev, dtype=torch.float32)
    kw = dict(epi=3, aux=_ptr(x2), ldaux=In) if residual else {}
    _fwd_gemm(M, N, Hb, _ptr(h), Hb, w2, _ptr(z), N, bias=_ptr(b2), device=dev, **kw)
    _wt_note(w1, M, ctx.needs_input_grad[0])
    if act == "relu":
        _tap_relu(w1, h, x.shape[:-1])
    ctx.xshape = x.shape
    return x2, h, pre, z


def _ffn_bwd(ctx, g, x2, h, pre, w1, b1, w2, b2, residual=None):
    """From g = dL/dz [M, N]: both layers' weight and bias gradients; returns _dx."""
    (Hb, In), N = w1.shape, w2.shape[0]
    M, dev = g.shape[0], g.device
    # d(pre-activation) = (g W2) * act'(.): the activation's backward fused into the GEMM epilogue
    # (relu: h > 0; tanh: 1 - h^2; silu: from the saved pre-activation)
    dh = torch.empty(M, Hb, device=dev, dtype=torch.float32)
    gemm(M, Hb, N, _ptr(g), 0, N, _ptr(w2), 0, Hb, _ptr(dh), Hb, epi=ctx.be,
         aux=_ptr(h if pre is None else pre), ldaux=Hb, device=dev)
    _wgrad(_ptr(g), N, _ptr(h), Hb, M, N, Hb, _gbuf(w2), dev, gb=_gbuf(b2), keep=(g, h))
    _wgrad(_ptr(dh), Hb, _ptr(x2), In, M, Hb, In, _gbuf(w1), dev, gb=_gbuf(b1), keep=(dh, x2))
    return _dx(ctx, dh, w1, residual)


class _FFNFn(Function):
    @staticmethod
    @_keeps_precision
    def forward(ctx, x, w1, b1, w2, b2, act="relu"):
        x2, h, pre, z = _ffn_fwd(ctx, x, w1, b1, w2, b2, act)
        ctx.save_for_backward(x2, h, w1, b1, w2, b2, pre)
        return z.view(*x.shape[:-1], w2.shape[0])

    @staticmethod
    @_keeps_precision
    def backward(ctx, dz):
        x2, h, w1, b1, w2, b2, pre = ctx.saved_tensors
        dz2 = dz.reshape(-1, w2.shape[0]).contiguous()
        return _ffn_bwd(ctx, dz2, x2, h, pre, w1, b1, w2, b2), None, None, None, None, None


def ffn(x, w1, b1, w2, b2, act="relu"):
    """Linear -> act -> Linear, act in ACTIVATIONS (relu | tanh | silu)."""
    return _FFNFn.apply(x, w1, b1, w2, b2, act)


class _FFNResLNFn(Function):
    """LN(W2 relu(W1 x + b1) + b2 + x): the metaformer block FeedForward (multi_modal_metaformer.py:328)."""

    @staticmethod
    @_keeps_precision
    def forward(ctx, x, w1, b1, w2, b2, gamma, beta, eps, act="relu"):
        x2, h, pre, z = _ffn_fwd(ctx, x, w1, b1, w2, b2, act)
        y, mean, rstd = _resln_fwd(z, x2, gamma, beta, eps)
        ctx.save_for_backward(x2, h, z, w1, b1, w2, b2, gamma, beta, mean, rstd, pre)
        return y.view(x.shape)

    @staticmethod
    @_keeps_precision
    def backward(ctx, dy):
        x2, h, z, w1, b1, w2, b2, gamma, beta, mean, rstd, pre = ctx.saved_tensors
        g = _resln_bwd(dy.reshape(x2.shape).contiguous(), z, x2, gamma, beta, mean, rstd)
        return (_ffn_bwd(ctx, g, x2, h, pre, w1, b1, w2, b2, residual=g),) + (None,) * 8


def ffn_residual_layernorm(x, w1, b1, w2, b2, gamma, beta, eps=1e-5, act="relu"):
    return _FFNResLNFn.apply(x, w1, b1, w2, b2, gamma, beta, eps, act)


class _FFNResFn(Function):
    """W2 act(W1 x + b1) + b2 + x: the residual FeedForward without a LayerNorm.  x is added by the
    second forward GEMM and dy by the input-gradient GEMM (epilogue 3 both times)."""

    @staticmethod
    @_keeps_precision
    def forward(ctx, x, w1, b1, w2, b2, act="relu"):
        x2, h, pre, z = _ffn_fwd(ctx, x, w1, b1, w2, b2, act, residual=True)
        ctx.save_for_backward(x2, h, w1, b1, w2, b2, pre)
        return z.view(x.shape)

    @staticmethod
    @_keeps_precision
    def backward(ctx, dy):
        x2, h, w1, b1, w2, b2, pre = ctx.saved_tensors
        g = dy.reshape(x2.shape).contiguous()
        return (_ffn_bwd(ctx, g, x2, h, pre, w1, b1, w2, b2, residual=g),) + (None,) * 5


def ffn_residual(x, w1, b1, w2, b2, act="relu"):
    """x + Linear -> act -> Linear (x), act in ACTIVATIONS; the output size must equal the input size."""
    if w2.shape[0] != w1.shape[1]:
        raise ValueError(f"ffn_residual: the residual needs equal input and output sizes, got {w1.shape[1]} "
                         f"and {w2.shape[0]}")
    _act_codes(act)
    return _FFNResFn.apply(x, w1, b1, w2, b2, act)


# ------------------------------------------------------------------ Linear -> act -> ... -> Linear
class _MLPChainFn(Function):
    """x -> act(W_0 x + b_0) -> ... -> W_{L-1} h + b_{L-1}: the MLP token mixer (mixer_block.py:114-166).
    Every activation is a forward GEMM epilogue (1 / 4 / 6) and every act' is the epilogue (2 / 5 / 7)
    of the next layer's input-gradient GEMM, so the chain runs no elementwise pass in either direction;
    weight and bias gradients go through _wgrad, as in _FFNFn."""

    @staticmethod
    @_keeps_precision
    def forward(ctx, x, act, *params):
        _lib.require_device(x)
        fe, ctx.be, _ = _act_codes(act)
        ws, bs = params[0::2], params[1::2]
        L = len(ws)
        dev = x.device
        h = x.reshape(-1, ws[0].shape[1]).contiguous()
        M = h.shape[0]
        hs, pres = [h], []
        for i, (w, b) in enumerate(zip(ws, bs)):
            N, In = w.shape
            last = i == L - 1
            out = torch.empty(M, N, device=dev, dtype=torch.float32)
            pre = torch.empty(M, N, device=dev, dtype=torch.float32) if (fe == 6 and not last) else None
            _fwd_gemm(M, N, In, _ptr(h), In, w, _ptr(out), N, bias=_ptr(b), epi=0 if last else fe,
                      aux=_ptr(pre), ldaux=N if pre is not None else 0, device=dev)
            _wt_note(w, M, i > 0 or ctx.needs_input_grad[0])
            if not last:
                hs.append(out)
                pres.append(pre)
            h = out
        ctx.L = L
        ctx.silu = fe == 6
        ctx.save_for_backward(*hs, *(pres if ctx.silu else ()), *ws, *bs)
        ctx.xshape = x.shape
        return h.view(*x.shape[:-1], ws[-1].shape[0])

    @staticmethod
    @_keeps_precision
    def backward(ctx, dy):
        L, saved = ctx.L, ctx.saved_tensors
        hs = saved[:L]
        pres = saved[L:2 * L - 1] if ctx.silu else None
        ws, bs = saved[-2 * L:-L], saved[-L:]
        g = dy.reshape(-1, ws[-1].shape[0]).contiguous()
        M = g.shape[0]
        dev = dy.device
        dx = None
        for i in range(L - 1, -1, -1):
            w, b = ws[i], bs[i]
            N, In = w.shape
            _wgrad(_ptr(g), N, _ptr(hs[i]), In, M, N, In, _gbuf(w), dev, gb=_gbuf(b), keep=(g, hs[i]))
            if i > 0:
                # gradient at layer i-1's pre-activation: (g W_i) * act'(.), act' in this GEMM's epilogue
                aux = pres[i - 1] if ctx.silu else hs[i]
                gp = torch.empty(M, In, device=dev, dtype=torch.float32)
                _dx_gemm(M, In, N, _ptr(g), N, w, _ptr(gp), In, epi=ctx.be, aux=_ptr(aux), ldaux=In, device=dev)
                g = gp
            else:
                dx = _dx(ctx, g, w)
        return (dx, None) + (None,) * (2 * L)


def mlp_chain(x, layers, act=None):
    """layers = [(weight, bias), ...]; act (relu | tanh | silu) after every Linear but the last; None:
    stacked linears."""
    if act is None:
        for w, b in layers:
            x = linear(x, w, b)
        return x
    if any(b is None for _, b in layers):
        raise NotImplementedError("mlp_chain: Linear without bias")
    return _MLPChainFn.apply(x, act, *[t for wb in layers for t in wb])


# ------------------------------------------------------------------ elementwise activation
class _ActFn(Function):
    """act(x) where no GEMM epilogue can carry it (the attention-output nonlinearity, for_sequential.py:47-51)."""

    @staticmethod
    @_keeps_precision
    def forward(ctx, x, act):
        _lib.require_device(x)
        ctx.kind = _act_codes(act)[2]
        xc = x.contiguous()
        y = torch.empty_like(xc)
        _lib.check(_lib.load().mrg_activation_fwd(xc.numel(), ctx.kind, _ptr(xc), _ptr(y), _stream()), "activation fwd")
        ctx.save_for_backward(xc if ctx.kind == 3 else y)
        return y

    @staticmethod
    @_keeps_precision
    def backward(ctx, dy):
        (saved,) = ctx.saved_tensors
        dyc = dy.contiguous()
        dx = torch.empty_like(saved)
        _lib.check(_lib.load().mrg_activation_bwd(saved.numel(), ctx.kind, _ptr(dyc), _ptr(saved), _ptr(dx),
                                                  _stream()), "activation bwd")
        return dx, None


def activation(x, act):
    return _ActFn.apply(x, act)


# ------------------------------------------------------------------ sample-0 broadcast
class _Sample0Fn(Function):
    """[B, ...] -> [B, ...] with every sample replaced by sample 0 (the reference's Q7 quirk: MHAMixer
    takes [0] of a bare tensor, and LN(y + x) broadcasts that sample over the batch).  Backward: the B
    gradient rows summed into sample 0 (mrg_colsum_f32 over a [B, rest] view), zeros elsewhere."""

    @staticmethod
    def forward(ctx, x):
        _lib.require_device(x)
        ctx.shape = x.shape
        return x[:1].expand(x.shape).contiguous()

    @staticmethod
    @_keeps_precision
    def backward(ctx, dy):
        B = ctx.shape[0]
        dyc = dy.contiguous()
        rest = dyc.numel() // B
        dx = zeros(*ctx.shape, device=dy.device)
        colsum(B, rest, _ptr(dyc), rest, _ptr(dx), beta=1.0, device=dy.device)
        return dx


def broadcast_sample0(x):
    return _Sample0Fn.apply(x)
