"""float64 restatements of the per-frame kernels of the scheduled-sampling decode (csrc/decode.hip), one
per C entry point and written from the contract in include/mrg.h, the guarded / poisoned buffers the
kernel-level tests hand to the C ABI, and the table of cases tests/test_gpu_decode.py runs
(tests/test_cpu_decode_ref.py ties the backward formulas to autograd and checks the table's own
conditions on the CPU).  Every function is plain torch and takes the dtype of its inputs: on float64
tensors it is the reference, on float32 tensors the fp32 composite whose error is printed beside a
kernel's as a yardstick.  A plain helper, not a conftest; it does not load the library."""
import functools
from collections import namedtuple

import numpy as np
import torch

from tests.attention_ref import SENTINEL

EPS = 1e-5
FILL = 7.0        # what an output holds before a call (the sentinel sits around it)
T_MS = 3          # frames of the ms / mask / y / dy buffers (frames 0, 1 and 2 are addressed)
SA, FMP = 128, 6  # sampler and partner-motion columns of the composition cases (as _ssd_inputs)


# ---------------------------------------------------------------- forward, one function per entry point
def gate_cell(X, w_ih, b_ih, b_hh):
    """Zero-state LSTM cell: a = X W_ih^T + b_ih + b_hh, gates (i, f, g, o) post-activation [B, 4H],
    c = sigmoid(i) tanh(g), h = sigmoid(o) tanh(c).  `a` is returned for autograd (dG is its gradient)."""
    a = X @ w_ih.t() + b_ih + b_hh
    i, f, g, o = a.chunk(4, -1)
    i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
    c = i * g
    return dict(a=a, gates=torch.cat([i, f, g, o], -1), c=c, h=o * torch.tanh(c))


def layernorm(hp, rp, gamma, beta, eps=EPS):
    """LN(hp + rp) with the biased variance; s = hp + rp is returned for autograd (g is its gradient)."""
    s = hp + rp
    mean = s.mean(-1, keepdim=True)
    rstd = ((s - mean).pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    return dict(s=s, out=(s - mean) * rstd * gamma + beta, mean=mean[:, 0], rstd=rstd[:, 0])


def gate_cell_fwd(mode, w_ih, b_ih, b_hh, xin=None, hp=None, rp=None, gamma=None, beta=None, eps=EPS):
    """mrg_ssd_gate_cell_fwd: X = xin (mode 0) or LN(hp + rp) (mode 1: mean, rstd) -> xout, gates, c, h."""
    r = {}
    if mode == 0:
        X = xin
    else:
        ln = layernorm(hp, rp, gamma, beta, eps)
        X = ln["out"]
        r.update(s=ln["s"], mean=ln["mean"], rstd=ln["rstd"])
    r.update(gate_cell(X, w_ih, b_ih, b_hh), xout=X)
    return r


def y_fwd(z, w2, b2):
    """mrg_ssd_y_fwd: y = z W2^T + b2."""
    return z @ w2.t() + b2


def feat_gate_cell_fwd(t, p, ms, wms_t, w_ih, b_ih, b_hh, z=None, w2=None, b2=None, mask=None):
    """mrg_ssd_feat_gate_cell_fwd: X = p + ms_in W_ms^T with ms_in = ms[:, 0] at t = 0 and
    mask[t-1] ? y(t-1) : ms[:, t-1] after, y(t-1) = z W2^T + b2 -> y (t > 0), xf_ms (= ms_in), xout,
    gates, c, h.  ms [B, T, FO], wms_t [FO, H]."""
    r = {}
    if t == 0:
        m = ms[:, 0]
    else:
        r["y"] = y_fwd(z, w2, b2)
        m = r["y"] if bool(mask[t - 1]) else ms[:, t - 1]
    m = m.clone()   # a node of its own: its gradient is dyx
    X = p + m @ wms_t
    r.update(gate_cell(X, w_ih, b_ih, b_hh), xf_ms=m, xout=X)
    return r


def ffn_z_fwd(hp, rp, gamma, beta, w1, b1, eps=EPS):
    """mrg_ssd_ffn_z_fwd: u = LN(hp + rp) (mean, rstd), z = relu(u W1^T + b1); pre is z before the ReLU."""
    ln = layernorm(hp, rp, gamma, beta, eps)
    pre = ln["out"] @ w1.t() + b1
    return dict(s=ln["s"], u=ln["out"], mean=ln["mean"], rstd=ln["rstd"], pre=pre, z=torch.relu(pre))


# ---------------------------------------------------------------- backward, from the saved tensors
def ln_bwd(du, h, x, gamma, mean, rstd):
    """g = d(h + x) of u = LN(h + x): rstd (gd - mean(gd) - xh mean(gd xh)), gd = du gamma."""
    xh = (h + x - mean[:, None]) * rstd[:, None]
    gd = du * gamma
    return rstd[:, None] * (gd - gd.mean(-1, keepdim=True) - xh * (gd * xh).mean(-1, keepdim=True))


def cell_bwd(g, gates, c):
    """dG [B, 4H]: the gradient of the gate pre-activations from g = dh, zero state (forget block 0)."""
    i, _, gg, o = gates.chunk(4, -1)
    tc = torch.tanh(c)
    dc = g * o * (1 - tc * tc)
    return torch.cat([dc * gg * i * (1 - i), torch.zeros_like(dc), dc * i * (1 - gg * gg), g * tc * o * (1 - o)], -1)


def row_sums_v(w1, gamma, beta):
    """v = [W1 gamma | W1 beta] [HB, 2]"""
    return torch.stack([w1 @ gamma, w1 @ beta], 1)


def ffn_bwd(t, dy, wms_t, mask, w1, w2, b1, z, h, x, gamma, mean, rstd, gates, c, dfeat_next=None, dyx_next=None,
            v=None):
    """mrg_ssd_ffn_bwd: dyt = dy + mask[t] (dfeat_next W_ms | dyx_next), dz = [z > 0] (dyt W2), du = dz W1,
    g = the LayerNorm backward of du, dG = the cell backward of g.  With v the two row sums of the
    LayerNorm backward go the kernel's way, sum du gamma = dz . v[:, 0] and sum du gamma xh =
    dz . (z - b1 - v[:, 1]) (z = u W1^T + b1 wherever dz != 0); without, they are taken over du itself."""
    nxt = torch.zeros_like(dy)
    if mask is not None and bool(mask[t]):
        if dfeat_next is not None:
            nxt = dfeat_next @ wms_t.t()
        if dyx_next is not None:
            nxt = dyx_next
    dyt = dy + nxt
    dz = (z > 0).to(dy.dtype) * (dyt @ w2)
    du = dz @ w1
    if v is None:
        g = ln_bwd(du, h, x, gamma, mean, rstd)
    else:
        H = h.shape[1]
        xh = (h + x - mean[:, None]) * rstd[:, None]
        m0, m1 = dz @ v[:, 0], (dz * (z - b1 - v[:, 1])).sum(-1)
        g = rstd[:, None] * (du * gamma - m0[:, None] / H - xh * m1[:, None] / H)
    return dict(dyt=dyt, dz=dz, du=du, g=g, dG=cell_bwd(g, gates, c))


def ln_cell_bwd(du, h, x, gamma, mean, rstd, gates, c, vt=None, wms_t=None):
    """mrg_ssd_ln_cell_bwd: g, dG of a lower layer; with vt [FM, 4H] = W_ms^T W_ih^T and wms_t [FM, H] also
    dyx = dG vt^T + g wms_t^T (= (dG W_ih + g) W_ms)."""
    g = ln_bwd(du, h, x, gamma, mean, rstd)
    r = dict(g=g, dG=cell_bwd(g, gates, c))
    if vt is not None:
        r["dyx"] = r["dG"] @ vt.t() + g @ wms_t.t()
    return r


def dx(dG, w_ih, g):
    """mrg_ssd_dx: dG W_ih + g over the i, g, o blocks (the kernel skips the forget block, which the cell
    backward leaves zero: a non-zero one in dG is to be ignored)."""
    H = g.shape[1]
    d = dG.clone()
    d[:, H:2 * H] = 0
    return d @ w_ih + g


# ---------------------------------------------------------------- the whole decode from the functions above
def decode_chain(a_s, mp, ms, mask, ps, nl, eps=EPS):
    """scheduled_sampling_decode chained from the per-entry-point forwards.  ps as _ssd_inputs orders them
    (w_f, b_f, per layer w_ih, w_hh, b_ih, b_hh, ln_w, ln_b, then w1, b1, w2, b2).  Returns y [B, T, FO]
    and per frame {"layers": [the layer records], "ffn": the ffn_z_fwd record, "y": y(t)}."""
    w_f, b_f = ps[:2]
    layers = [ps[2 + 6 * i:8 + 6 * i] for i in range(nl)]
    w1, b1, w2, b2 = ps[2 + 6 * nl:]
    n = a_s.shape[2] + mp.shape[2]
    wms_t = w_f[:, n:].t()
    P = torch.cat([a_s, mp], -1) @ w_f[:, :n].t() + b_f
    frames, z = [], None
    for t in range(a_s.shape[1]):
        L = [feat_gate_cell_fwd(t, P[:, t], ms, wms_t, layers[0][0], layers[0][2], layers[0][3], z, w2, b2, mask)]
        for i in range(1, nl):
            L.append(gate_cell_fwd(1, layers[i][0], layers[i][2], layers[i][3], hp=L[-1]["h"], rp=L[-1]["xout"],
                                   gamma=layers[i - 1][4], beta=layers[i - 1][5], eps=eps))
        f = ffn_z_fwd(L[-1]["h"], L[-1]["xout"], layers[-1][4], layers[-1][5], w1, b1, eps)
        z = f["z"]
        if t:
            frames[-1]["y"] = L[0]["y"]
        frames.append(dict(layers=L, ffn=f))
    frames[-1]["y"] = y_fwd(z, w2, b2)
    return torch.stack([f["y"] for f in frames], 1), frames


def decode_inputs(B, T, H, HB, FO, nl, seed):
    """Float32 inputs of the decode at any H / HB, drawn as tests/test_gpu_models._ssd_inputs draws them at
    H = 256, HB = 64: parameters (that order), (a_s, mp, ms, dy), mask [T] bool."""
    F = SA + FMP + FO
    g = torch.Generator().manual_seed(seed)

    def u(*shape, k):
        return (torch.rand(*shape, generator=g) * 2 - 1) * k
    ps = [u(H, F, k=F ** -0.5), u(H, k=F ** -0.5)]
    for _ in range(nl):
        ps += [u(4 * H, H, k=H ** -0.5), u(4 * H, H, k=H ** -0.5), u(4 * H, k=H ** -0.5), u(4 * H, k=H ** -0.5),
               1 + u(H, k=0.2), u(H, k=0.2)]
    ps += [u(HB, H, k=H ** -0.5), u(HB, k=H ** -0.5), u(FO, HB, k=HB ** -0.5), u(FO, k=HB ** -0.5)]
    acts = [torch.randn(B, T, n, generator=g) for n in (SA, FMP, FO, FO)]
    return ps, acts, torch.from_numpy(np.random.RandomState(seed).rand(T) < 0.5)


# (B, T, H, HB, FO, nl) of the end-to-end runs of the per-frame path, and the seed of each (one at which
# no FFN pre-activation of the float64 chain lies at the ReLU kink: tests/test_cpu_decode_ref.py)
COMPOSE = [(9, 5, 36, 7, 1, 1), (17, 4, 68, 33, 8, 3), (7, 6, 132, 64, 6, 2), (9, 5, 256, 64, 6, 1)]
COMPOSE_SEED = {c: 7000 + i for i, c in enumerate(COMPOSE)}


@functools.lru_cache(maxsize=None)
def compose_reference(case):
    """float64 autograd of decode_chain on decode_inputs(case): y, the a_s gradient, the parameter
    gradients and the FFN pre-activations [T, B, HB].  Computed once; not to be modified."""
    B, T, H, HB, FO, nl = case
    ps, (a_s, mp, ms, dy), mask = decode_inputs(B, T, H, HB, FO, nl, COMPOSE_SEED[case])
    rp = [p.double().requires_grad_(True) for p in ps]
    ra = a_s.double().requires_grad_(True)
    y, frames = decode_chain(ra, mp.double(), ms.double(), mask, rp, nl)
    (y * dy.double()).sum().backward()
    grads = [torch.zeros_like(p) if p.grad is None else p.grad for p in rp]   # None: W_hh, which the chain never reads
    return dict(y=y.detach(), da=ra.grad, grads=grads, pre=torch.stack([f["ffn"]["pre"].detach() for f in frames]))


# ---------------------------------------------------------------- the error measure
def row_errs(a, ref, blocks=1, zero_scale=None):
    """max |a - ref| / max |ref| per batch row and per block of the row (blocks = 4: the gate blocks, so
    a wrong block cannot hide behind a larger one), as a [B, blocks] tensor; a [B] vector is measured
    element by element.  A non-finite value of `a` makes its slice's error inf.  Where a slice of the
    reference is zero everywhere the error is |a| / zero_scale [B] of the row, or, without zero_scale,
    0 if `a` is exactly zero there and inf if not."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    a, ref = a.reshape(a.shape[0], blocks, -1), ref.reshape(ref.shape[0], blocks, -1)
    den, num = ref.abs().amax(-1), (a - ref).abs().amax(-1)
    if zero_scale is not None:
        den = torch.where(den == 0, zero_scale.double().cpu()[:, None].expand_as(den), den)
    err = torch.where(den == 0, torch.where(num == 0, 0.0, float("inf")).double(), num / den.clamp_min(1e-300))
    return torch.where(torch.isfinite(a).all(-1), err, torch.full_like(err, float("inf")))


def worst(a, ref, blocks=1, zero_scale=None):
    """The largest of row_errs."""
    return row_errs(a, ref, blocks, zero_scale).max().item()


BLOCKS = {"gates": 4, "dG": 4}   # outputs measured per gate block


# ---------------------------------------------------------------- guarded outputs, poisoned inputs
def guarded(rows, cols, row_stride=None, offset=0, lead=8, device="cpu"):
    """An output of `rows` rows of `cols` floats holding FILL, inside a flat buffer of SENTINEL: `lead`
    sentinels (and `offset` more) in front, rows of stride row_stride >= cols, two spare rows behind.
    Returns (buffer, [rows, cols] view); the view aliases the buffer, which attention_ref.outside_intact checks."""
    rs = cols if row_stride is None else row_stride
    assert rs >= cols and offset + cols <= rs
    buf = torch.full((lead + (rows + 2) * rs,), SENTINEL, dtype=torch.float32, device=device)
    view = buf.as_strided((rows, cols), (rs, 1), lead + offset)
    view.fill_(FILL)
    return buf, view


def poisoned(t, spare=8):
    """t (1-d or 2-d) as the leading rows of one allocation whose `spare` further rows are NaN: a kernel
    that reads row B (weight row 4H, w2 row FO, the element behind the last row) and uses it produces a
    non-finite result.  Returns the view of the real rows."""
    buf = torch.full((t.shape[0] + spare,) + tuple(t.shape[1:]), float("nan"), dtype=t.dtype, device=t.device)
    buf[:t.shape[0]] = t
    return buf[:t.shape[0]]


def poisoned_slice(t, rows_extra=1, cols_extra=2):
    """t [B, T, C] as the [:, :T, :C] slice of a NaN-filled [B + 1, T + rows_extra, C + cols_extra] buffer
    (batch stride != T * C, row stride != C)."""
    Bt, T, C = t.shape
    buf = torch.full((Bt + 1, T + rows_extra, C + cols_extra), float("nan"), dtype=t.dtype, device=t.device)
    buf[:Bt, :T, :C] = t
    return buf[:Bt, :T, :C]


# ---------------------------------------------------------------- the case table
# (B, H, HB, FO).  H: 4 the smallest, 36 / 64 the narrow template instance and its upper edge, 68 / 128
# the middle one's two edges, 132 / 252 / 256 the wide one's; B: 1, and 7 / 8 / 9 around the 8-row tiles,
# 16 / 17 around the gate kernels' 16-row tile, 33 = 4 tiles + 1 (2 + 1 of 16); HB: 1, 7 / 8 around the
# 8-column tile, 33 (the second half of the 32-lane j split, a partial tile), 64 the most; FO: 1, 6, 8.
# HB = 1 goes with small B only: a row whose single FFN unit is off has zero gradients throughout.
Case = namedtuple("Case", "name B H HB FO")
SHAPES = [(1, 4, 1, 1), (7, 4, 7, 6), (9, 36, 7, 1), (17, 36, 33, 8), (8, 64, 8, 6), (16, 64, 64, 8),
          (33, 64, 33, 1), (9, 68, 33, 8), (17, 68, 7, 6), (8, 68, 64, 1), (7, 128, 64, 6), (16, 128, 8, 1),
          (33, 128, 33, 8), (9, 132, 64, 6), (7, 132, 1, 8), (17, 132, 8, 1), (7, 252, 33, 6), (33, 252, 7, 8),
          (1, 252, 64, 1), (9, 256, 64, 6), (17, 256, 33, 8), (16, 256, 8, 1), (33, 256, 7, 6)]
LN_SHAPES = [(9, 1, 8, 6), (7, 5, 8, 6), (17, 255, 8, 6)]   # mrg_ssd_ln_cell_bwd alone takes these H


def _name(B, H, HB, FO):
    return f"B{B}-H{H}-HB{HB}-FO{FO}"


CASES = [Case(_name(*s), *s) for s in SHAPES]
LN_CASES = [Case(_name(*s), *s) for s in LN_SHAPES]
BY_NAME = {c.name: c for c in CASES + LN_CASES}
NAMES = [c.name for c in CASES]
LN_NAMES = [c.name for c in LN_CASES]
FMS = (1, 6, 8)   # the FM values mrg_ssd_ln_cell_bwd's dyx form runs at


def h_class(H):
    """The H-dispatch class of the templated kernels."""
    return "H<=64" if H <= 64 else "H<=128" if H <= 128 else "H<=256"


# every call the GPU tests compare, per kind: [(kw, outputs compared)]
FWD = ("gates", "c", "h")
CALLS = {
    "gate": [(dict(mode=0), ("xout",) + FWD), (dict(mode=1), ("xout", "mean", "rstd") + FWD)],
    "feat": [(dict(t=0, sel=0), ("xf_ms", "xout") + FWD)] +
            [(dict(t=2, sel=s), ("y", "xf_ms", "xout") + FWD) for s in (0, 1)],
    "ffn_z": [(dict(), ("u", "mean", "rstd", "z"))],
    "y": [(dict(), ("y",))],
    "ffn_bwd": [(dict(t=1, form=f, sel=s), ("dyt", "dz", "du", "g", "dG"))
                for f, s in (("none", 0), ("dfeat", 0), ("dfeat", 1), ("dyx", 0), ("dyx", 1))],
    "ln": [(dict(FM=0), ("g", "dG"))] + [(dict(FM=m), ("g", "dG", "dyx")) for m in FMS],
    "dx": [(dict(), ("dx",))],
}
ZERO_AT_H1 = ("g", "dG", "dyx")   # mrg_ssd_ln_cell_bwd at H = 1: measured against zero_scale
COND = 1e-5                        # a tenth of the bound of tests/test_gpu_decode.py


def _draw(c, seed):
    B, H, HB, FO = c.B, c.H, c.HB, c.FO
    g = torch.Generator().manual_seed(seed)

    def u(*shape, k):
        return (torch.rand(*shape, generator=g) * 2 - 1) * k

    def n(*shape, shift=0.0):
        return torch.randn(*shape, generator=g) + shift
    x = dict(w_ih=u(4 * H, H, k=H ** -0.5), b_ih=u(4 * H, k=H ** -0.5), b_hh=u(4 * H, k=H ** -0.5),
             gamma=1 + u(H, k=0.2), beta=u(H, k=0.2), w1=u(HB, H, k=H ** -0.5), b1=u(HB, k=H ** -0.5),
             w2=u(FO, HB, k=HB ** -0.5), b2=u(FO, k=HB ** -0.5), wms8=u(8, H, k=FO ** -0.5))
    # rows with a mean well away from zero: the LayerNorm mean is compared relatively
    x.update(xin=n(B, H, shift=0.5), hp=n(B, H, shift=0.5), rp=n(B, H), p=n(B, H), zprev=torch.relu(n(B, HB)),
             ms=n(B, T_MS, FO), dy=n(B, T_MS, FO), dfeat_next=n(B, H), dyx_next=n(B, FO), du_in=n(B, H),
             g_in=n(B, H), dG_in=n(B, 4 * H))
    d = {k: v.double() for k, v in x.items()}
    # the saved tensors of the backward: the float64 forward of xin, rounded to float32
    f = gate_cell(d["xin"], d["w_ih"], d["b_ih"], d["b_hh"])
    x.update(gates=f["gates"].float(), c=f["c"].float(), h=f["h"].float())
    ln = layernorm(x["h"].double(), d["xin"], d["gamma"], d["beta"])
    x.update(mean=ln["mean"].float(), rstd=ln["rstd"].float())
    # z of the backward, given as data: the pre-activation u W1^T + b1 of the saved h, x, mean, rstd (so
    # that z - b1 - W1 beta = W1 (xh gamma) wherever z > 0), about half of it negative (the kernel treats
    # z <= 0 alike), and exact zeros spread over it (relu'(0) = 0)
    xh = (x["h"].double() + d["xin"] - x["mean"].double()[:, None]) * x["rstd"].double()[:, None]
    z = ((xh * d["gamma"] + d["beta"]) @ d["w1"].t() + d["b1"]).float()
    if HB >= 7:
        z.view(-1)[3::5] = 0.0
    x["z"] = z
    x["v"] = row_sums_v(d["w1"], d["gamma"], d["beta"]).float()
    x["vt8"] = (d["wms8"] @ d["w_ih"].t()).float()
    return x


def _usable(x):
    """Every row keeps an active FFN unit (else all its gradients are zero), and both LayerNorm inputs
    have |mean| >= 1% of the row's largest element (the mean is compared relatively, row by row)."""
    if not bool((x["z"] > 0).any(-1).all()):
        return False
    for s in (x["hp"] + x["rp"], x["h"] + x["xin"]):
        if not bool((s.double().mean(-1).abs() >= 0.01 * s.abs().amax(-1)).all()):
            return False
    return True


def calls_of(c):
    """[(kind, kw, outputs)] of the calls the case runs: all of them, or mrg_ssd_ln_cell_bwd's alone"""
    kinds = CALLS if c in CASES else {"ln": CALLS["ln"]}
    return [(kind, kw, outs) for kind, calls in kinds.items() for kw, outs in calls]


def _conditioned(c, x):
    """Plain fp32 arithmetic holds every compared slice within COND of float64: no slice of the draw is a
    cancelling sum (a single y or dyx element per row at FO = 1 can be), so a kernel that misses the bound
    is wrong and not unlucky."""
    d64, d32 = as_dtype(x, torch.float64), as_dtype(x, torch.float32)
    zs = zero_scale(x["du_in"], x["gamma"], x["rstd"]) if c.H == 1 else None
    with torch.no_grad():
        for kind, kw, outs in calls_of(c):
            ref, got = call_reference(kind, d64, c, **kw), call_reference(kind, d32, c, **kw)
            for n in outs:
                if not worst(got[n], ref[n], BLOCKS.get(n, 1), zs if n in ZERO_AT_H1 else None) < COND:
                    return False
    return True


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The case's float32 tensors on the CPU, the same for every test that names it (not to be modified):
    the first seed from 100000 * (the case's index) on at which _usable and _conditioned hold."""
    c = BY_NAME[name]
    base = 100000 * (CASES + LN_CASES).index(c)
    for k in range(4000):
        x = _draw(c, base + k)
        if _usable(x) and _conditioned(c, x):
            x["seed"] = base + k
            return x
    raise RuntimeError(f"{name}: no usable seed")


def masks(t):
    """The two sampling masks [T_MS] uint8 of a call that reads mask[t]: mask[t] = 0 with every other
    entry 1, and the opposite (a read of a neighbouring entry flips the select)."""
    off = torch.ones(T_MS, dtype=torch.uint8)
    off[t] = 0
    return {0: off, 1: 1 - off}


def zero_scale(du, gamma, rstd):
    """max |du gamma| rstd per row: the size of the terms that cancel where a LayerNorm backward is
    identically zero (H = 1: gd - mean(gd) = 0 and xh = 0), against which what is left is measured."""
    return (du.double() * gamma.double()).abs().amax(-1) * rstd.double()


# ---------------------------------------------------------------- the reference of every call, by name
def as_dtype(x, dtype):
    return {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in x.items()}


def call_reference(kind, x, c, **kw):
    """What the entry point `kind` returns on the case's tensors x (float64: the reference, float32: the
    composite).  kw: mode (gate), t and sel (feat, ffn_bwd: mask[t-1] / mask[t]), form (ffn_bwd: "none",
    "dfeat", "dyx"), FM (ln: 0 without dyx)."""
    W = (x["w_ih"], x["b_ih"], x["b_hh"])
    saved = (x["h"], x["xin"], x["gamma"], x["mean"], x["rstd"], x["gates"], x["c"])
    if kind == "gate":
        if kw["mode"] == 0:
            return gate_cell_fwd(0, *W, xin=x["xin"])
        return gate_cell_fwd(1, *W, hp=x["hp"], rp=x["rp"], gamma=x["gamma"], beta=x["beta"])
    if kind == "feat":
        t = kw["t"]
        mask = masks(t - 1)[kw["sel"]] if t else None
        return feat_gate_cell_fwd(t, x["p"], x["ms"], x["wms8"][:c.FO], *W, x["zprev"], x["w2"], x["b2"], mask)
    if kind == "ffn_z":
        return ffn_z_fwd(x["hp"], x["rp"], x["gamma"], x["beta"], x["w1"], x["b1"])
    if kind == "y":
        return dict(y=y_fwd(x["zprev"], x["w2"], x["b2"]))
    if kind == "ffn_bwd":
        t, form = kw["t"], kw["form"]
        return ffn_bwd(t, x["dy"][:, t], x["wms8"][:c.FO], masks(t)[kw["sel"]], x["w1"], x["w2"], x["b1"], x["z"],
                       *saved, dfeat_next=x["dfeat_next"] if form == "dfeat" else None,
                       dyx_next=x["dyx_next"] if form == "dyx" else None)
    if kind == "ln":
        FM = kw["FM"]
        r = ln_cell_bwd(x["du_in"], *saved, vt=x["vt8"][:FM] if FM else None, wms_t=x["wms8"][:FM] if FM else None)
        if c.H == 1:
            # one element: gd - mean(gd) = 0 and xh = 0, so g, dG and dyx are zero identically (the formula
            # on a rounded saved mean leaves rounding of its own there, which is no reference)
            r = {k: torch.zeros_like(v) for k, v in r.items()}
        return r
    if kind == "dx":
        return dict(dx=dx(x["dG_in"], x["w_ih"], x["g_in"]))
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def _reference(name, kind, kw, dtype):
    with torch.no_grad():
        return call_reference(kind, as_dtype(inputs(name), dtype), BY_NAME[name], **dict(kw))


def reference(name, kind, **kw):
    """call_reference in float64 on inputs(name), computed once."""
    return _reference(name, kind, tuple(sorted(kw.items())), torch.float64)


def composite(name, kind, **kw):
    """call_reference in float32 on inputs(name): the yardstick."""
    return _reference(name, kind, tuple(sorted(kw.items())), torch.float32)
