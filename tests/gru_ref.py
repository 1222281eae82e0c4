"""float64 restatement of what the two persistent GRU kernels (csrc/gru_rec.hip: mrg_gru_fwd, mrg_gru_bwd)
write, from the header comment of that file, and the table of cases tests/test_gpu_gru_rec.py runs
(tests/test_cpu_gru_ref.py ties the forward to torch.nn.GRU and the backward to autograd, and checks the
table's own claims on the CPU).  Both functions are plain torch and take the dtype of their inputs: on
float64 tensors they are the reference, on float32 tensors the composite whose error is printed beside a
kernel's as a yardstick.  The guarded / poisoned buffers and the error measure are those of
tests/decode_ref.py and tests/attention_ref.py.  A plain helper, not a conftest; it does not load the
library."""
import functools
from collections import namedtuple

import torch

from tests.decode_ref import row_errs

BLOCKS = {"gates": 3, "dgx": 3, "dgh": 3}   # outputs measured per gate block (r, z, n)


# ---------------------------------------------------------------- the formulas
def steps(T, reverse):
    """time indices in the order the forward visits them"""
    return range(T - 1, -1, -1) if reverse else range(T)


def forward(gx, w_hh, b_hh, h0=None, reverse=False):
    """gx [B, T, 3H] = x W_ih^T + b_ih.  Per step gh = h_{t-1} W_hh^T + b_hh, r = s(gx_r + gh_r),
    z = s(gx_z + gh_z), n = tanh(gx_n + r gh_n), h_t = (1 - z) n + z h_{t-1}.  Returns y [B, T, H],
    gates [B, T, 3H] (r, z, n), ghn [B, T, H] = gh_n, and gh, the list of the per-step recurrent
    pre-activations by time index (nodes of the graph: their gradient is dgh)."""
    B, T, H3 = gx.shape
    H = H3 // 3
    h = gx.new_zeros(B, H) if h0 is None else h0
    y, gates, ghn, ghs = [None] * T, [None] * T, [None] * T, [None] * T
    for t in steps(T, reverse):
        gh = h @ w_hh.t() + b_hh
        ghs[t] = gh
        r = torch.sigmoid(gx[:, t, :H] + gh[:, :H])
        z = torch.sigmoid(gx[:, t, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(gx[:, t, 2 * H:] + r * gh[:, 2 * H:])
        h = (1 - z) * n + z * h
        y[t], gates[t], ghn[t] = h, torch.cat([r, z, n], -1), gh[:, 2 * H:]
    if T == 0:
        return dict(y=gx.new_zeros(B, 0, H), gates=gx.new_zeros(B, 0, H3), ghn=gx.new_zeros(B, 0, H), gh=[])
    return dict(y=torch.stack(y, 1), gates=torch.stack(gates, 1), ghn=torch.stack(ghn, 1), gh=ghs)


def backward(w_hh, gates, ghn, y, h0=None, dy=None, dhT=None, reverse=False):
    """From the saved gates, ghn and y (h_{t-1} is y at the step before, h0 or zero at the first):
    dh_t = dy_t + (dh carried from the step after), dn = dh (1 - z), dz = dh (h_{t-1} - n),
    dn' = dn (1 - n^2), dr = dn' ghn; dgx = (dr r (1 - r), dz z (1 - z), dn'), dgh the same with the n
    block dn' r; carried to the step before: dgh W_hh + dh z.  Returns dgx, dgh [B, T, 3H] and dh0 [B, H]."""
    B, T, H = y.shape
    dh = y.new_zeros(B, H) if dhT is None else dhT
    dgx, dgh = [None] * T, [None] * T
    order = list(steps(T, reverse))
    for i in range(T - 1, -1, -1):
        t = order[i]
        hprev = y[:, order[i - 1]] if i > 0 else (y.new_zeros(B, H) if h0 is None else h0)
        r, z, n = gates[:, t, :H], gates[:, t, H:2 * H], gates[:, t, 2 * H:]
        d = dh if dy is None else dh + dy[:, t]
        dpn = d * (1 - z) * (1 - n * n)
        gr = dpn * ghn[:, t] * r * (1 - r)
        gz = d * (hprev - n) * z * (1 - z)
        dgx[t], dgh[t] = torch.cat([gr, gz, dpn], -1), torch.cat([gr, gz, dpn * r], -1)
        dh = dgh[t] @ w_hh + d * z
    if T == 0:
        return dict(dgx=y.new_zeros(B, 0, 3 * H), dgh=y.new_zeros(B, 0, 3 * H), dh0=dh)
    return dict(dgx=torch.stack(dgx, 1), dgh=torch.stack(dgh, 1), dh0=dh)


# ---------------------------------------------------------------- the error measure
def errs(name, a, ref):
    """decode_ref.row_errs per batch row, and per gate block over all steps for gates / dgx / dgh
    ([B, T, 3H] -> [B, 3, T H]); a slice whose reference is zero everywhere must be exactly zero."""
    blocks = BLOCKS.get(name, 1)
    if blocks > 1:
        Bt, T, H3 = ref.shape
        a, ref = (t.reshape(Bt, T, blocks, H3 // blocks).transpose(1, 2) for t in (a, ref))
    return row_errs(a, ref, blocks)


def worst(name, a, ref):
    return errs(name, a, ref).max().item()


# ---------------------------------------------------------------- the case table
# (H, G): the five groups gru_rec.hip instantiates (G = 4 / 8: ring members at H = 256, mrg_gru_config;
# G = 1: a solo workgroup), each at the batch tiles gru_tile_ok admits
HG = ((256, 4), (256, 8), (128, 1), (64, 1), (32, 1))
B_RAGGED = 21            # ragged at tiles 2, 4 and 8; 168 workgroups at G = 8, tile 1
B_EXACT = (1, 8)         # one row; eight rows: eight groups at tile 1, one full group at tile 8
T_FULL, T_SHORT = 12, (1, 2, 3)
T_LAYER = 9              # the end-to-end pass
IN_LAYER = 40


def fwd_threads(H, G):
    """GruFwdCfg<H, G>::NT"""
    R = 3 * H // G
    return R * 8 // (4 if R * 8 // 2 > 1024 else 2)


def bwd_threads(H, G):
    """GruBwdCfg<H, G>::NT"""
    return 8 * H // (4 if G > 1 else 1)


def tiles(H, G):
    """the batch tiles BS with BS * U <= both thread counts (gru_tile_ok), U = H / G"""
    return tuple(bs for bs in (1, 2, 4, 8) if bs * (H // G) <= min(fwd_threads(H, G), bwd_threads(H, G)))


def self_io(H, G, bs):
    """SELF_IO of gru_bwd_kernel<H, G, BS>: CW * 64 + BS * U > NT, CW the cell waves; the cells then move
    their own saved values and stage after the GEMV, else io shadow waves at offset CW * 64 do"""
    U = H // G
    return -(-bs * U // 64) * 64 + bs * U > bwd_threads(H, G)


Tile = namedtuple("Tile", "name H G bs self_io")
TILES = [Tile(f"H{H}-G{G}-BS{bs}-{'selfio' if self_io(H, G, bs) else 'shadow'}", H, G, bs, self_io(H, G, bs))
         for H, G in HG for bs in tiles(H, G)]
TILE_BY_NAME = {t.name: t for t in TILES}
TILE_NAMES = [t.name for t in TILES]
# tile 1 and the largest tile of each (H, G): where the short sequences and the nullable forms run
EDGE_NAMES = [t.name for t in TILES if t.bs in (1, tiles(t.H, t.G)[-1])]
LARGEST_NAMES = [t.name for t in TILES if t.bs == tiles(t.H, t.G)[-1]]
GROUP_NAMES = [f"H{H}-G{G}" for H, G in HG]
GROUPS = dict(zip(GROUP_NAMES, HG))

# the backward's forms: which of h0, dy, dhT are passed and whether dh0 is asked for
Form = namedtuple("Form", "name h0 dy dhT dh0")
FORMS = [Form("full", True, True, True, True), Form("dy", True, True, False, True),
         Form("dhT", True, False, True, True), Form("none", True, False, False, True),
         Form("nodh0", True, True, True, False), Form("noh0", False, True, True, True)]
FORM_BY_NAME = {f.name: f for f in FORMS}


@functools.lru_cache(maxsize=None)
def inputs(H, B, T):
    """The float32 tensors of one shape on the CPU, the same for every test that names it (not to be
    modified), scaled like the GRU tests of tests/test_gpu_ops.py: w_hh, b_hh ~ 1 / sqrt(H), h0 * 0.5."""
    g = torch.Generator().manual_seed(1000003 * H + 1009 * B + T)
    s = H ** -0.5
    return dict(gx=torch.randn(B, T, 3 * H, generator=g), w_hh=torch.randn(3 * H, H, generator=g) * s,
                b_hh=torch.randn(3 * H, generator=g) * s, h0=torch.randn(B, H, generator=g) * 0.5,
                dy=torch.randn(B, T, H, generator=g), dhT=torch.randn(B, H, generator=g))


@functools.lru_cache(maxsize=None)
def fwd_reference(H, B, T, reverse, with_h0, dtype=torch.float64):
    """forward() on inputs(H, B, T) in `dtype` (float64: the reference, float32: the yardstick), once"""
    x = {k: v.to(dtype) for k, v in inputs(H, B, T).items()}
    with torch.no_grad():
        r = forward(x["gx"], x["w_hh"], x["b_hh"], x["h0"] if with_h0 else None, reverse)
    return {k: r[k] for k in ("y", "gates", "ghn")}


def saved(H, B, T, reverse, with_h0):
    """what the backward reads: the float64 forward rounded to float32, not a kernel's output"""
    return {k: v.float() for k, v in fwd_reference(H, B, T, reverse, with_h0).items()}


@functools.lru_cache(maxsize=None)
def bwd_reference(H, B, T, reverse, form, dtype=torch.float64):
    """backward() on saved(...) and the form's gradients in `dtype`, once"""
    f, x, s = FORM_BY_NAME[form], inputs(H, B, T), saved(H, B, T, reverse, FORM_BY_NAME[form].h0)
    c = lambda t: t.to(dtype)
    with torch.no_grad():
        return backward(c(x["w_hh"]), c(s["gates"]), c(s["ghn"]), c(s["y"]), c(x["h0"]) if f.h0 else None,
                        c(x["dy"]) if f.dy else None, c(x["dhT"]) if f.dhT else None, reverse)


@functools.lru_cache(maxsize=None)
def layer_reference(H, reverse):
    """One torch.nn.GRU layer in float64 at B_RAGGED x T_LAYER with h0: the float32 inputs and parameters
    and y, hT, dx, dh0 and the four parameter gradients of (y dy).sum() + (hT dh).sum()."""
    B, T, In = B_RAGGED, T_LAYER, IN_LAYER
    g = torch.Generator().manual_seed(77 * H + int(reverse))
    s = H ** -0.5
    p = dict(w_ih=torch.randn(3 * H, In, generator=g) * s, w_hh=torch.randn(3 * H, H, generator=g) * s,
             b_ih=torch.randn(3 * H, generator=g) * s, b_hh=torch.randn(3 * H, generator=g) * s)
    a = dict(x=torch.randn(B, T, In, generator=g), h0=torch.randn(B, H, generator=g) * 0.5,
             dy=torch.randn(B, T, H, generator=g), dh=torch.randn(B, H, generator=g))
    ref = torch.nn.GRU(In, H, batch_first=True).double()
    ref.load_state_dict({"weight_ih_l0": p["w_ih"].double(), "weight_hh_l0": p["w_hh"].double(),
                         "bias_ih_l0": p["b_ih"].double(), "bias_hh_l0": p["b_hh"].double()})
    x, h0 = a["x"].double().requires_grad_(True), a["h0"].double().requires_grad_(True)
    y, hT = ref(x.flip(1) if reverse else x, h0[None])
    y = y.flip(1) if reverse else y
    ((y * a["dy"].double()).sum() + (hT[0] * a["dh"].double()).sum()).backward()
    out = dict(y=y.detach(), hT=hT[0].detach(), dx=x.grad, dh0=h0.grad, w_ih=ref.weight_ih_l0.grad,
               w_hh=ref.weight_hh_l0.grad, b_ih=ref.bias_ih_l0.grad, b_hh=ref.bias_hh_l0.grad)
    return p, a, out
