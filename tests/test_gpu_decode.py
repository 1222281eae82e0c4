"""The seven mrg_ssd_* per-frame kernels of the scheduled-sampling decode (csrc/decode.hip) called through the
C ABI, one by one, against the float64 restatements of tests/decode_ref.py at the launch edges of its case
table: all three template instances of the H-dispatched kernels and the sizes on both sides of each
dispatch boundary, partial row and column tiles, every form of each entry point (modes, t = 0, the
sampling select both ways, the three next-frame forms of the FFN backward, the LayerNorm / cell backward
with and without dyx at FM in {1, 6, 8} and at H that is no multiple of 4), guarded outputs, NaN-poisoned
spare rows behind every input, B = 0, determinism, every argument refusal, and the per-frame path end to
end at four sizes no other test runs it at.

Error measure: max |a - ref| / max |ref| per batch row (gates and dG per gate block as well), bound
TOL = 1e-4 (the fp32 bar of tests/test_gpu_ops.py).  A slice whose reference is zero everywhere must be
exactly zero (the forget block of dG, a z row whose units are all off) or, where rounding is left over
(g, dG and dyx at H = 1), is measured against decode_ref.zero_scale.  Every comparison prints its worst
figure with the error plain fp32 torch ops make on the same inputs beside it (run with -s to see them)."""
import pytest
import torch

from tests import decode_ref as R
from tests.attention_ref import outside_intact
from tests.golden_util import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = "cuda:0"
T_MS = R.T_MS
ENTRY = {"gate": "mrg_ssd_gate_cell_fwd", "feat": "mrg_ssd_feat_gate_cell_fwd", "ffn_z": "mrg_ssd_ffn_z_fwd",
         "y": "mrg_ssd_y_fwd", "ffn_bwd": "mrg_ssd_ffn_bwd", "ln": "mrg_ssd_ln_cell_bwd", "dx": "mrg_ssd_dx"}


@pytest.fixture(scope="module")
def lib():
    from multimodalreactiongeneration_amd import _lib as L
    lib = L.load()
    yield lib
    torch.cuda.synchronize()


def _ptr(t, off=0):
    from multimodalreactiongeneration_amd.functional import _ptr as p
    return p(t, off)


def _stream():
    from multimodalreactiongeneration_amd.functional import _stream as s
    return s()


class _Bufs:
    """The device buffers of one call: inputs followed by NaN rows, outputs between sentinels."""

    def __init__(self, name):
        self.x = R.inputs(name)
        self.guards, self.outs = [], {}

    def inp(self, key, spare=8):
        t = self.x[key] if isinstance(key, str) else key
        return R.poisoned(t.to(DEV).contiguous(), spare)

    def out(self, name, rows, cols, **kw):
        buf, view = R.guarded(rows, cols, device=DEV, **kw)
        self.guards.append((buf, view))
        self.outs[name] = view
        return view

    def vec(self, name, n):
        self.outs[name] = self.out(name, 1, n)[0]
        return self.outs[name]

    def intact(self):
        return all(outside_intact(b, v) for b, v in self.guards)

    def untouched(self):
        return all(bool((v == R.FILL).all()) for v in self.outs.values())


def _args(kind, name, kw, b):
    """[(argument name, value)] of the entry point, in the order of its declaration"""
    c, x = R.BY_NAME[name], b.x
    B, H, HB, FO = c.B, c.H, c.HB, c.FO
    cell_w = [("w_ih", b.inp("w_ih")), ("b_ih", b.inp("b_ih")), ("b_hh", b.inp("b_hh"))]

    def cell_out():
        return [("gates", b.out("gates", B, 4 * H)), ("c", b.out("c", B, H)), ("h", b.out("h", B, H))]

    def saved():
        return dict(h=b.inp("h"), x=b.inp("xin"), gamma=b.inp("gamma"), mean=b.inp("mean"), rstd=b.inp("rstd"),
                    gates=b.inp("gates"), c=b.inp("c"))
    if kind == "gate":
        if kw["mode"] == 0:
            xin = b.inp("xin")
            b.xin = xin
            xout = xin if kw.get("inplace") else b.out("xout", B, H)
            a = [("xin", xin), ("hp", None), ("rp", None), ("gamma", None), ("beta", None), ("eps", R.EPS),
                 ("xout", xout), ("mean", None), ("rstd", None)]
        else:
            a = [("xin", None), ("hp", b.inp("hp")), ("rp", b.inp("rp")), ("gamma", b.inp("gamma")),
                 ("beta", b.inp("beta")), ("eps", R.EPS), ("xout", b.out("xout", B, H)),
                 ("mean", b.vec("mean", B)), ("rstd", b.vec("rstd", B))]
        return [("B", B), ("H", H), ("mode", kw["mode"])] + a + cell_w + cell_out()
    if kind == "feat":
        t, F = kw["t"], FO + 5
        ms = R.poisoned_slice(x["ms"].to(DEV))   # a [:, :, :FO] slice of a wider, longer buffer
        return [("B", B), ("H", H), ("HB", HB), ("FO", FO), ("F", F), ("t", t), ("p", b.inp("p")),
                ("z", b.inp("zprev") if t else None), ("w2", b.inp("w2")), ("b2", b.inp("b2")),
                ("mask", R.masks(t - 1)[kw["sel"]].to(DEV) if t else None), ("ms", ms), ("ms_bs", ms.stride(0)),
                ("ms_ts", ms.stride(1)), ("wms_t", b.inp(x["wms8"][:FO])),
                ("y", b.out("y", B, FO, row_stride=T_MS * FO, offset=(t - 1) * FO) if t else None),
                ("y_bs", T_MS * FO), ("xf_ms", b.out("xf_ms", B, FO, row_stride=F, offset=F - FO)),
                ("xout", b.out("xout", B, H))] + cell_w + cell_out()
    if kind == "ffn_z":
        return [("B", B), ("H", H), ("HB", HB), ("hp", b.inp("hp")), ("rp", b.inp("rp")), ("gamma", b.inp("gamma")),
                ("beta", b.inp("beta")), ("eps", R.EPS), ("u", b.out("u", B, H)), ("mean", b.vec("mean", B)),
                ("rstd", b.vec("rstd", B)), ("w1", b.inp("w1")), ("b1", b.inp("b1")), ("z", b.out("z", B, HB))]
    if kind == "y":
        return [("B", B), ("HB", HB), ("FO", FO), ("z", b.inp("zprev")), ("w2", b.inp("w2")), ("b2", b.inp("b2")),
                ("y", b.out("y", B, FO, row_stride=T_MS * FO, offset=(T_MS - 1) * FO)), ("y_bs", T_MS * FO)]
    if kind == "ffn_bwd":
        t, form, s = kw["t"], kw["form"], saved()
        dy = torch.full_like(x["dy"], float("nan"))   # [B, T_MS, FO]: frame t real, the others NaN
        dy[:, t] = x["dy"][:, t]
        return [("B", B), ("H", H), ("HB", HB), ("FO", FO), ("t", t), ("dy", b.inp(dy)[:, t]), ("dy_bs", T_MS * FO),
                ("dfeat_next", b.inp("dfeat_next") if form in ("dfeat", "both") else None),
                ("dyx_next", b.inp("dyx_next") if form in ("dyx", "both") else None),
                ("wms_t", b.inp(x["wms8"][:FO])), ("mask", R.masks(t)[kw["sel"]].to(DEV)), ("w1", b.inp("w1")),
                ("w2", b.inp("w2")), ("b1", b.inp("b1")), ("v", b.inp("v", spare=64)), ("z", b.inp("z")),
                ("dyt", b.out("dyt", B, FO)), ("dz", b.out("dz", B, HB)), ("du", b.out("du", B, H)), ("h", s["h"]),
                ("x", s["x"]), ("gamma", s["gamma"]), ("mean", s["mean"]), ("rstd", s["rstd"]),
                ("g", b.out("g", B, H)), ("gates", s["gates"]), ("c", s["c"]), ("dG", b.out("dG", B, 4 * H))]
    if kind == "ln":
        FM, s = kw["FM"], saved()
        return [("B", B), ("H", H), ("du", b.inp("du_in")), ("h", s["h"]), ("x", s["x"]), ("gamma", s["gamma"]),
                ("mean", s["mean"]), ("rstd", s["rstd"]), ("g", b.out("g", B, H)), ("gates", s["gates"]), ("c", s["c"]),
                ("dG", b.out("dG", B, 4 * H)), ("FM", FM), ("vt", b.inp(x["vt8"][:FM]) if FM else None),
                ("wms_t", b.inp(x["wms8"][:FM]) if FM else None), ("dyx", b.out("dyx", B, FM) if FM else None)]
    if kind == "dx":
        return [("B", B), ("H", H), ("dG", b.inp("dG_in")), ("w_t", b.inp(x["w_ih"].t())), ("g", b.inp("g_in")),
                ("dx", b.out("dx", B, H))]
    raise ValueError(kind)


def _call(lib, kind, name, kw, over=None, off=(), null=()):
    """One call of the entry point on the case's tensors.  over: integer arguments replaced; off: pointer
    arguments moved on by one float; null: pointer arguments passed as NULL.  Returns (status, buffers)."""
    b = _Bufs(name)
    vals = []
    for n, v in _args(kind, name, kw, b):
        if over and n in over:
            v = over[n]
        if n in null:
            v = None
        vals.append(_ptr(v, 1 if n in off else 0) if torch.is_tensor(v) else v)
    rc = getattr(lib, ENTRY[kind])(*vals, _stream())
    torch.cuda.synchronize()
    return rc, b


def _compare(kind, name, kw, outs, got):
    c, x = R.BY_NAME[name], R.inputs(name)
    ref, yard = R.reference(name, kind, **kw), R.composite(name, kind, **kw)
    zs = R.zero_scale(x["du_in"], x["gamma"], x["rstd"]) if c.H == 1 else None
    bad = {}
    for n in outs:
        scale, blocks = (zs if n in R.ZERO_AT_H1 else None), R.BLOCKS.get(n, 1)
        e, y = R.worst(got[n], ref[n], blocks, scale), R.worst(yard[n], ref[n], blocks, scale)
        form = ",".join(f"{k}={v}" for k, v in sorted(kw.items()))
        print(f"DEC {ENTRY[kind]} {R.h_class(c.H)} {name} [{form}] {n} err={e:.3e} fp32={y:.3e}")
        if not e < TOL:
            bad[n] = e
    assert not bad, f"{ENTRY[kind]} {name} {kw}: {bad}"
    return ref


def _run(lib, kind, name, kw, outs):
    """The call twice (bitwise equal), its guards, and every output against float64."""
    rc, b = _call(lib, kind, name, kw)
    assert rc == 0, lib.mrg_last_error()
    assert b.intact(), f"{ENTRY[kind]} {name} {kw}: a store outside the rows"
    rc2, b2 = _call(lib, kind, name, kw)
    assert rc2 == 0
    for n in outs:
        assert torch.equal(b.outs[n], b2.outs[n]), (n, "two runs differ")
    return b, _compare(kind, name, kw, outs, b.outs)


# ---------------------------------------------------------------- forward
@pytest.mark.parametrize("name", R.NAMES)
def test_gate_cell_fwd(lib, name):
    """Mode 0 with a separate xout (a copy of xin) and with xout == xin (nothing written to it), mode 1
    (xout = LN(hp + rp), mean, rstd); gates per block, c, h."""
    for kw, outs in R.CALLS["gate"]:
        b, ref = _run(lib, "gate", name, kw, outs)
        if kw["mode"] == 0:
            assert torch.equal(b.outs["xout"].cpu(), R.inputs(name)["xin"])
    rc, b = _call(lib, "gate", name, dict(mode=0, inplace=True))
    assert rc == 0 and b.intact() and torch.equal(b.xin.cpu(), R.inputs(name)["xin"])
    _compare("gate", name, dict(mode=0), R.FWD, b.outs)


@pytest.mark.parametrize("name", R.NAMES)
def test_feat_gate_cell_fwd(lib, name):
    """t = 0 with z = y = mask = NULL (ms_in = ms[:, 0]); t = 2 with mask[1] 0 (ms[:, 1]) and 1 (y(1)), the
    neighbouring mask entries holding the opposite value; ms a slice of a wider, longer NaN-filled buffer;
    y one frame of a [B, T, FO] buffer and xf_ms the last columns of [B, F] rows, the rest left alone."""
    for kw, outs in R.CALLS["feat"]:
        b, ref = _run(lib, "feat", name, kw, outs)
        if kw["t"]:
            want = ref["y"] if kw["sel"] else R.inputs(name)["ms"][:, 1].double()
            assert R.worst(b.outs["xf_ms"], want) < TOL
            if not kw["sel"]:
                assert torch.equal(b.outs["xf_ms"].cpu(), R.inputs(name)["ms"][:, 1])
        else:
            assert torch.equal(b.outs["xf_ms"].cpu(), R.inputs(name)["ms"][:, 0])


@pytest.mark.parametrize("name", R.NAMES)
def test_ffn_z_fwd(lib, name):
    for kw, outs in R.CALLS["ffn_z"]:
        b, ref = _run(lib, "ffn_z", name, kw, outs)
        assert bool((b.outs["z"] >= 0).all())


@pytest.mark.parametrize("name", R.NAMES)
def test_y_fwd(lib, name):
    """y at y_bs = T FO > FO: the last frame's columns of a [B, T, FO] buffer."""
    for kw, outs in R.CALLS["y"]:
        _run(lib, "y", name, kw, outs)


# ---------------------------------------------------------------- backward
@pytest.mark.parametrize("name", R.NAMES)
def test_ffn_bwd(lib, name):
    """No next frame, dfeat_next (the one-layer backward) and dyx_next, the latter two with mask[t] 0 and 1
    (mask[t - 1] and mask[t + 1] the opposite); v = [W1 gamma | W1 beta] computed in float64 and rounded;
    the reference takes the LayerNorm's row sums over du itself.  The forget block of dG is exactly zero,
    and with mask[t] = 0 the next-frame term is absent."""
    c, x = R.BY_NAME[name], R.inputs(name)
    for kw, outs in R.CALLS["ffn_bwd"]:
        b, ref = _run(lib, "ffn_bwd", name, kw, outs)
        assert bool((b.outs["dG"][:, c.H:2 * c.H] == 0).all())
        if kw["sel"] == 0:
            scale = R.zero_scale(ref["du"], x["gamma"], x["rstd"])
            left = (b.outs["dyt"].cpu().double() - x["dy"][:, kw["t"]].double()).abs().amax(-1)
            assert bool((left <= TOL * scale).all()), left.max().item()


@pytest.mark.parametrize("name", R.NAMES + R.LN_NAMES)
def test_ln_cell_bwd(lib, name):
    """Without dyx (vt = wms_t = NULL, FM = 0) and with it at FM in {1, 6, 8}; H = 1, 5 and 255 besides the
    table's.  At H = 1 the exact g, dG and dyx are zero (one element: gd - mean(gd) = 0, xh = 0); what
    the kernel leaves is measured against max |du gamma| rstd."""
    c = R.BY_NAME[name]
    for kw, outs in R.CALLS["ln"]:
        b, ref = _run(lib, "ln", name, kw, outs)
        assert bool((b.outs["dG"][:, c.H:2 * c.H] == 0).all())


@pytest.mark.parametrize("name", R.NAMES)
def test_dx(lib, name):
    """dx = dG W_ih + g with W_ih given transposed.  The dG handed in has a non-zero forget block: the
    contract says the kernel skips that block (the cell backward leaves it zero), so the reference
    multiplies with the block zeroed; a kernel that read it would be off by its whole product."""
    for kw, outs in R.CALLS["dx"]:
        _run(lib, "dx", name, kw, outs)


# ---------------------------------------------------------------- B = 0 and the refusals
SMALL = "B9-H36-HB7-FO1"
FIRST = {kind: calls[-1][0] for kind, calls in R.CALLS.items()}   # one form of each entry point
FIRST["feat"], FIRST["ffn_bwd"] = dict(t=2, sel=1), dict(t=1, form="dfeat", sel=1)


@pytest.mark.parametrize("kind", list(ENTRY))
def test_no_rows_is_a_no_op(lib, kind):
    rc, b = _call(lib, kind, SMALL, FIRST[kind], over=dict(B=0))
    assert rc == 0 and b.intact() and b.untouched()


def _refusals():
    r = []
    for kind in ENTRY:
        if kind != "y":
            r += [(kind, dict(over=dict(H=h))) for h in ((0, 257, 260) if kind == "ln" else (0, 6, 260))]
        if kind in ("feat", "ffn_z", "y", "ffn_bwd"):
            r += [(kind, dict(over=dict(HB=hb))) for hb in (0, 65)]
        if kind in ("feat", "y", "ffn_bwd"):
            r += [(kind, dict(over=dict(FO=fo))) for fo in (0, 9)]
    r.append(("ln", dict(over=dict(FM=9))))
    aligned = {"gate": ("w_ih",), "feat": ("w_ih", "wms_t", "p"), "dx": ("dG", "w_t"),
               "ffn_z": ("hp", "rp", "w1", "u"), "ffn_bwd": ("w1", "wms_t", "dfeat_next")}
    r += [(kind, dict(off=(n,))) for kind, names in aligned.items() for n in names]
    r += [("feat", dict(null=(n,))) for n in ("z", "y", "mask")]
    r.append(("ffn_bwd", dict(form="both")))
    r.append(("ln", dict(null=("vt",))))
    r.append(("ln", dict(null=("wms_t",))))
    return r


@pytest.mark.parametrize("kind,how", _refusals(), ids=lambda v: v if isinstance(v, str) else
                         "-".join(f"{k}:{v}" for k, v in v.items()).replace(" ", ""))
def test_bad_arguments_are_refused_before_any_launch(lib, kind, how):
    """Sizes outside the documented ranges, a pointer one float off where 16-byte alignment is required,
    frame t > 0 without z / y / mask, both next-frame forms at once, dyx without vt / wms_t: a non-zero
    status, mrg_last_error names the entry point, and no output has changed."""
    how = dict(how)
    kw = dict(FIRST[kind])
    if "form" in how:
        kw["form"] = how.pop("form")
    if kind == "ln":
        kw = dict(FM=6)
    rc, b = _call(lib, kind, SMALL, kw, **how)
    assert rc != 0
    assert ENTRY[kind].encode() in lib.mrg_last_error(), lib.mrg_last_error()
    assert b.intact() and b.untouched()


# ---------------------------------------------------------------- the per-frame path end to end
@pytest.mark.parametrize("case", R.COMPOSE, ids=lambda c: "x".join(map(str, c)))
def test_per_frame_decode_matches_float64(case):
    """decode.scheduled_sampling_decode on the per-frame kernels (H != 256 takes them by itself; at H = 256
    the persistent loops are switched off and restored) against float64 autograd of decode_ref.decode_chain:
    y and the sampler-output gradient per batch row, every parameter gradient; W_hh gradients exactly zero
    on both sides.  One layer runs the dfeat_next form and mrg_ssd_dx on layer 0, two and three the dyx
    form; the host's v, vt and w_t operands are part of what is compared."""
    from multimodalreactiongeneration_amd import decode as D
    from multimodalreactiongeneration_amd import functional as Fn
    B, T, H, HB, FO, nl = case
    ref = R.compose_reference(case)
    ps, (a_s, mp, ms, dy), mask = R.decode_inputs(B, T, H, HB, FO, nl, R.COMPOSE_SEED[case])
    gp = [p.to(DEV).requires_grad_(True) for p in ps]
    ga = a_s.to(DEV).requires_grad_(True)
    prev = D._LOOP[0], D._LOOP_BWD[0]
    D._LOOP[0], D._LOOP_BWD[0] = False, False
    try:
        y = D.scheduled_sampling_decode(ga, mp.to(DEV), ms.to(DEV), mask.to(DEV), gp[0], gp[1],
                                        [gp[2 + 6 * i:8 + 6 * i] for i in range(nl)], gp[2 + 6 * nl:])
        (y * dy.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        Fn.check_errors()
    finally:
        D._LOOP[0], D._LOOP_BWD[0] = prev
    assert y.shape == (B, T, FO)
    errs = {"y": R.worst(y.reshape(B, -1), ref["y"].reshape(B, -1)),
            "a_s.grad": R.worst(ga.grad.reshape(B, -1), ref["da"].reshape(B, -1))}
    for i, (p, r) in enumerate(zip(gp, ref["grads"])):
        if 2 <= i < 2 + 6 * nl and (i - 2) % 6 == 1:   # W_hh
            assert r.abs().max() == 0 and (p.grad is None or p.grad.abs().max() == 0), i
            continue
        errs[f"grad {i}"] = rel_err(p.grad, r)
    print(f"DEC decode {R.h_class(H)} {case}:", {k: f"{e:.2e}" for k, e in errs.items()})
    for k, e in errs.items():
        assert e < TOL, (k, e)
