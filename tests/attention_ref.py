"""float64 reference of the attention core (the scaled-dot-product part of nn.MultiheadAttention that
csrc/attention.hip computes: no projections), the strided / guarded buffers the kernel-level tests hand
to the C ABI, and the table of cases tests/test_gpu_attention.py runs (tests/test_cpu_attention_ref.py
checks the table's own conditions on the CPU).  A plain helper, not a conftest."""
import functools
import math
from collections import namedtuple

import torch

from tests.dropout_ref import visible

B, HEADS = 2, 3          # an odd head count: head offsets h * D that are no powers of two
SENTINEL = -777.25       # exact in float32; no attention result of these inputs equals it
WIDTHS = (8, 16, 32, 64)


# ---------------------------------------------------------------- the formula
def _attention(q, k, v, heads, scale, vis, dout):
    Bq, Tq, E = q.shape
    Tk, D = k.shape[1], E // heads
    if dout is not None:
        q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    Q = q.view(Bq, Tq, heads, D).transpose(1, 2)
    K = k.view(Bq, Tk, heads, D).transpose(1, 2)
    V = v.view(Bq, Tk, heads, D).transpose(1, 2)
    S = (Q @ K.transpose(-1, -2) * scale).masked_fill(~vis.to(q.device).unsqueeze(1), float("-inf"))
    O = (torch.softmax(S, dim=-1) @ V).transpose(1, 2).reshape(Bq, Tq, E)
    lse = torch.logsumexp(S, dim=-1)
    if dout is None:
        return O.detach(), lse.detach()
    O.backward(dout)
    return O.detach(), lse.detach(), q.grad, k.grad, v.grad


def core(q, k, v, heads, scale, vis, dout=None):
    """softmax(masked_fill(Q K^T * scale, ~vis, -inf)) V per head, in double.  q [B, Tq, heads * D],
    k / v [B, Tk, heads * D], vis bool [B, Tq, Tk] (dropout_ref.visible).  Returns O [B, Tq, E] and
    lse [B, heads, Tq] (the logsumexp of the same masked scores), and dQ, dK, dV by autograd when dout
    [B, Tq, E] is given.  A fully hidden row is NaN in O and -inf in lse."""
    assert all(t.dtype == torch.float64 for t in (q, k, v)) and vis.dtype == torch.bool
    return _attention(q, k, v, heads, scale, vis, None if dout is None else dout.double())


def fp32_composite(q, k, v, heads, scale, vis, dout=None):
    """The same formula in float32 torch ops, unfused, on the device the inputs are on: what plain fp32
    arithmetic makes of these inputs (the yardstick beside the kernels' error)."""
    q, k, v = (t.float() for t in (q, k, v))
    return _attention(q, k, v, heads, scale, vis, None if dout is None else dout.float())


def slice_errs(a, ref, heads=HEADS, zero_scale=None):
    """max |a - ref| / max |ref| of every (sample, head) slice, as a [B, heads] tensor: a head with small
    values cannot hide behind one with large values.  a, ref: [B, T, heads * D], or the [B, heads, T]
    statistics when ref has that shape (told apart by ref.shape[1] == heads, so T != heads).  Positions
    where ref is not finite are left out (the caller checks those itself); a non-finite value of `a`
    anywhere else makes the slice's error inf.  zero_scale [B, heads]: the denominator of a slice whose
    reference is exactly zero everywhere (zero_scales), where the measure is otherwise undefined."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    assert a.shape == ref.shape and a.dim() == 3
    if ref.shape[1] != heads:
        a, ref = (t.reshape(t.shape[0], t.shape[1], heads, -1).permute(0, 2, 1, 3) for t in (a, ref))
    a, ref = a.reshape(a.shape[0], heads, -1), ref.reshape(ref.shape[0], heads, -1)
    ok = torch.isfinite(ref)
    zero = torch.zeros_like(ref)
    den = torch.where(ok, ref.abs(), zero).amax(-1)
    if zero_scale is not None:
        den = torch.where(den == 0, zero_scale.double(), den)
    err = torch.where(ok, (a - ref).abs(), zero).amax(-1) / den.clamp_min(1e-30)
    bad = (ok & ~torch.isfinite(a)).any(-1)
    return torch.where(bad, torch.full_like(err, float("inf")), err)


def slice_err(a, ref, heads=HEADS, zero_scale=None):
    """The largest of slice_errs."""
    return slice_errs(a, ref, heads, zero_scale).max().item()


# ---------------------------------------------------------------- strided, guarded buffers
def strided(t, row_stride, lead, spare_rows=2, sentinel=SENTINEL):
    """Place t [B, T, E] in a larger flat buffer filled with `sentinel`: `lead` floats in front, rows of
    stride row_stride >= E (batch stride T * row_stride) and spare_rows rows behind.  Returns
    (buffer, view); the view aliases the buffer."""
    Bt, T, E = t.shape
    assert row_stride >= E and lead >= 0
    buf = torch.full((lead + (Bt * T + spare_rows) * row_stride,), sentinel, dtype=t.dtype, device=t.device)
    view = buf[lead:lead + Bt * T * row_stride].view(Bt, T, row_stride)[:, :, :E]
    view.copy_(t)
    return buf, view


def outside_intact(buf, view, sentinel=SENTINEL):
    """True when every element of buf that is not an element of view still holds the sentinel."""
    out = torch.ones_like(buf, dtype=torch.bool)
    out.as_strided(view.shape, view.stride(), view.storage_offset() - buf.storage_offset()).fill_(False)
    return bool((buf[out] == sentinel).all())


# ---------------------------------------------------------------- the case table
# name: test id; pad: the padding pattern (pad_flags); qscale multiplies q (8: score standard deviation
# about 8, the row softmax close to one-hot); tags: "padded", "leading", "large_logits", "fully_masked"
Case = namedtuple("Case", "name Tq Tk causal pad qscale widths tags")

SHAPES = [(1, 1, False), (17, 33, False), (65, 129, False), (130, 70, False),
          (65, 65, True), (33, 132, True), (130, 130, True), (132, 33, True), (66, 33, True)]
PADS = ("none", "tail", "leading", "scattered")


def pad_flags(pad, Tq, Tk, causal):
    """(qpad, kpad) uint8 [B, Tq] / [B, Tk] of a padding pattern, or (None, None); the two samples differ.
    tail: the last third (sample 1: half) of the queries and of the keys, as a padded batch has them.
    leading: the first 32 (sample 1: 33) keys, so a flagged query starts its online softmax on a wholly
      hidden 32-key group; flagged is every other query among those that see a later, unflagged key.
    scattered: every third key and every fourth query (phases chosen so query 0 keeps a visible key).
    row64: query 64 and every key it sees (Tq = Tk = 65, causal: all of them): a fully hidden row."""
    if pad == "none":
        return None, None
    qpad, kpad = torch.zeros(B, Tq, dtype=torch.uint8), torch.zeros(B, Tk, dtype=torch.uint8)
    for b in range(B):
        if pad == "tail":
            qpad[b, Tq * 2 // 3 if b == 0 else Tq // 2:] = 1
            kpad[b, Tk * 2 // 3 if b == 0 else Tk // 2:] = 1
        elif pad == "leading":
            n = min(32 + b, Tk - 1)
            kpad[b, :n] = 1
            sees_later = visible(Tq, Tk, causal)[0, :, n:].any(-1).nonzero().flatten()
            qpad[b, sees_later[::2]] = 1
        elif pad == "scattered":
            kpad[b, 1 + b::3] = 1
            qpad[b, b::4] = 1
        elif pad == "row64":
            qpad[b, 64] = 1
            kpad[b, visible(Tq, Tk, causal)[0, 64]] = 1
        else:
            raise ValueError(pad)
    return qpad, kpad


def _build_cases():
    cases = []
    for Tq, Tk, causal in SHAPES:
        for pad in PADS:
            # one (query, key) pair: any padding that hides it leaves a NaN row, any other hides nothing;
            # the leading pattern needs a key past the first 32
            if pad != "none" and (Tk == 1 or (pad == "leading" and Tk <= 32)):
                continue
            tags = () if pad == "none" else ("padded", "leading") if pad == "leading" else ("padded",)
            cases.append(Case(f"{Tq}x{Tk}{'c' if causal else 'n'}-{pad}", Tq, Tk, causal, pad, 1.0, WIDTHS, tags))
    for Tq, Tk, causal in [(65, 129, False), (130, 130, True)]:
        cases.append(Case(f"{Tq}x{Tk}{'c' if causal else 'n'}-large", Tq, Tk, causal, "none", 8.0, (16, 64),
                          ("large_logits",)))
    cases.append(Case("65x65c-row64", 65, 65, True, "row64", 1.0, (8, 64), ("padded", "fully_masked")))
    return cases


CASES = _build_cases()
BY_NAME = {c.name: c for c in CASES}


def case_params(select=lambda c: True, widths=None):
    """[(case name, D)] of the cases `select` picks, at each of the case's widths (or those in `widths`)."""
    return [(c.name, D) for c in CASES if select(c) for D in c.widths if widths is None or D in widths]


def case_vis(case):
    qpad, kpad = pad_flags(case.pad, case.Tq, case.Tk, case.causal)
    return visible(case.Tq, case.Tk, case.causal, qpad, kpad, B)


@functools.lru_cache(maxsize=None)
def inputs(name, D):
    """The case's float32 inputs on the CPU, the same for every test that names it: q, k, v, dout
    [B, T, HEADS * D] standard normal (q times the case's qscale; with scale = 1 / sqrt(D) the scores have
    standard deviation qscale), the padding flags and scale.  Not to be modified."""
    c = BY_NAME[name]
    E = HEADS * D
    g = torch.Generator().manual_seed(1000 * CASES.index(c) + D)
    q, k, v, dout = (torch.randn(B, T, E, generator=g) for T in (c.Tq, c.Tk, c.Tk, c.Tq))
    qpad, kpad = pad_flags(c.pad, c.Tq, c.Tk, c.causal)
    return dict(q=q * c.qscale, k=k, v=v, dout=dout, qpad=qpad, kpad=kpad, scale=1.0 / math.sqrt(D))


def _on_inputs(fn, name, D, grads):
    x = inputs(name, D)
    q, k, v, dout = (x[n].double() for n in ("q", "k", "v", "dout"))
    r = fn(q, k, v, HEADS, x["scale"], case_vis(BY_NAME[name]), dout if grads else None)
    return dict(zip(("O", "lse", "dQ", "dK", "dV"), r))


@functools.lru_cache(maxsize=None)
def reference(name, D, grads=True):
    """core() on inputs(name, D): {"O", "lse"[, "dQ", "dK", "dV"]} in double, computed once."""
    return _on_inputs(core, name, D, grads)


@functools.lru_cache(maxsize=None)
def zero_scales(name, D):
    """The denominators slice_errs uses for dQ and dK where a slice's exact gradient is zero everywhere, as
    it is with a single visible key: dS = P (dP - delta) with dP = dO V^T and delta = rowsum(P dP) cancels
    exactly, and max |a - ref| / max |ref| divides by zero.  What fp32 arithmetic leaves there is the
    rounding of dP and delta times the other operand, so the error is measured against the size of those
    uncancelled terms: scale * max |dP| * max |K| for dQ, scale * max |dP| * max |Q| for dK, per slice."""
    x, c = inputs(name, D), BY_NAME[name]
    Q, dO = (x[n].double().view(B, c.Tq, HEADS, D).transpose(1, 2) for n in ("q", "dout"))
    K, V = (x[n].double().view(B, c.Tk, HEADS, D).transpose(1, 2) for n in ("k", "v"))
    dp = (dO @ V.transpose(-1, -2)).abs().amax((-1, -2)) * x["scale"]
    return {"dQ": dp * K.abs().amax((-1, -2)), "dK": dp * Q.abs().amax((-1, -2))}


def errors(got, name, D, outs):
    """{output: slice_errs of got[output] against reference(name, D)} for the outputs named"""
    ref, zs = reference(name, D, len(outs) > 2), zero_scales(name, D)
    return {n: slice_errs(got[n], ref[n], zero_scale=zs.get(n)) for n in outs}


@functools.lru_cache(maxsize=None)
def yardstick(name, D, grads=True):
    """errors() of fp32_composite on inputs(name, D), per output."""
    outs = ("O", "lse", "dQ", "dK", "dV") if grads else ("O", "lse")
    return errors(_on_inputs(fp32_composite, name, D, grads), name, D, outs)
