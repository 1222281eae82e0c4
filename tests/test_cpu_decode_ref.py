"""tests/decode_ref.py checked on the CPU: its explicit backward formulas against float64 autograd through
the chained forward (every intermediate, one to three layers, the row sums both over du and through v),
the chained forward against the existing restatement of the decode (test_gpu_models._ssd_f64), the buffer
helpers and the error measure, and the conditions the case table of tests/test_gpu_decode.py must meet by
its inputs alone."""
import pytest
import torch

from tests import decode_ref as R
from tests.attention_ref import SENTINEL, outside_intact
from tests.test_gpu_models import _no_kinks, _ssd_f64, _ssd_inputs

TOL = 1e-4


# ---------------------------------------------------------------- the formulas
def _chain(nl, B=5, T=5, H=12, HB=7, FO=3, seed=11):
    ps, (a_s, mp, ms, dy), _ = R.decode_inputs(B, T, H, HB, FO, nl, seed)
    ps = [p.double().requires_grad_(True) for p in ps]
    mask = torch.tensor([1, 0, 1, 1, 0], dtype=torch.bool)[:T]
    # ms takes a gradient so that ms_in is a node of the graph in every frame, sampled or not
    y, frames = R.decode_chain(a_s.double().requires_grad_(True), mp.double(), ms.double().requires_grad_(True), mask,
                               ps, nl)
    return ps, mask, dy.double(), y, frames


@pytest.mark.parametrize("through_v", [False, True])
@pytest.mark.parametrize("nl", [1, 2, 3])
def test_backward_formulas_match_autograd(nl, through_v):
    """dy_total, dz, du, g, dG, dx and dyx of every frame and layer, run backwards frame by frame as decode.py
    runs the kernels (one layer: dfeat_next from mrg_ssd_dx; more: dyx_next from the bottom layer), against
    the gradients autograd leaves on the same nodes of the chained forward, to 1e-10."""
    ps, mask, dy, y, frames = _chain(nl)
    T = y.shape[1]
    nodes = [f["y"] for f in frames] + [f["ffn"][k] for f in frames for k in ("pre", "u", "s")]
    for f in frames:
        for i, L in enumerate(f["layers"]):
            nodes += [L["a"], L["xout"]] + ([L["s"]] if i else [L["xf_ms"]])
    for n in nodes:
        n.retain_grad()
    (y * dy).sum().backward()
    layers = [[p.detach() for p in ps[2 + 6 * i:8 + 6 * i]] for i in range(nl)]
    w1, b1, w2, b2 = (p.detach() for p in ps[2 + 6 * nl:])
    wms_t = ps[0].detach()[:, R.SA + R.FMP:].t()
    vt = wms_t @ layers[0][0].t()
    v = R.row_sums_v(w1, layers[-1][4], layers[-1][5]) if through_v else None
    seen = []

    def same(what, a, node):
        assert node.grad is not None, what
        assert R.worst(a, node.grad) < 1e-10, (what, R.worst(a, node.grad))
        seen.append(what.split()[0])

    def saved(f, i):
        """h, x, gamma, mean, rstd, gates, c of layer i: the LayerNorm after it is the next record's"""
        L, after = f["layers"][i], (f["layers"][i + 1] if i + 1 < nl else f["ffn"])
        return [t.detach() for t in (L["h"], L["xout"], layers[i][4], after["mean"], after["rstd"], L["gates"], L["c"])]
    dfeat = dyx = None
    for t in range(T - 1, -1, -1):
        f = frames[t]
        r = R.ffn_bwd(t, dy[:, t], wms_t, mask, w1, w2, b1, f["ffn"]["z"].detach(), *saved(f, nl - 1),
                      dfeat_next=dfeat if nl == 1 else None, dyx_next=dyx if nl > 1 else None, v=v)
        for k, node in (("dyt", f["y"]), ("dz", f["ffn"]["pre"]), ("du", f["ffn"]["u"]), ("g", f["ffn"]["s"]),
                        ("dG", f["layers"][-1]["a"])):
            same(f"{k} t={t}", r[k], node)
        assert bool((r["dG"][:, 12:24] == 0).all())
        g, dG = r["g"], r["dG"]
        for i in range(nl - 1, 0, -1):
            up = R.dx(dG, layers[i][0], g)
            same(f"dx t={t} layer {i}", up, f["layers"][i]["xout"])
            q = R.ln_cell_bwd(up, *saved(f, i - 1), vt=vt if i == 1 else None, wms_t=wms_t if i == 1 else None)
            same(f"g t={t} layer {i - 1}", q["g"], f["layers"][i]["s"])
            same(f"dG t={t} layer {i - 1}", q["dG"], f["layers"][i - 1]["a"])
            g, dG = q["g"], q["dG"]
            if i == 1:
                dyx = q["dyx"]
                same(f"dyx t={t}", dyx, f["layers"][0]["xf_ms"])
        dfeat = R.dx(dG, layers[0][0], g)
        same(f"dx t={t} layer 0", dfeat, f["layers"][0]["xout"])
    assert set(seen) == {"dyt", "dz", "du", "g", "dG", "dx"} | ({"dyx"} if nl > 1 else set())


def test_dx_ignores_the_forget_block():
    g = torch.Generator().manual_seed(3)
    dG, w, r = (torch.randn(*s, generator=g, dtype=torch.float64) for s in ((5, 32), (32, 8), (5, 8)))
    z = dG.clone()
    z[:, 8:16] = 0
    assert torch.equal(R.dx(dG, w, r), z @ w + r) and not torch.equal(R.dx(dG, w, r), dG @ w + r)


@pytest.mark.parametrize("B,T,nl,FO", [(5, 6, 1, 6), (3, 5, 2, 9), (4, 4, 3, 1)])
def test_chain_matches_the_existing_restatement(B, T, nl, FO):
    """decode_chain against test_gpu_models._ssd_f64 (written frame by frame around one Linear over the
    concatenated features and torch's layer_norm) on that test's own inputs."""
    ps, (a_s, mp, ms, _), mask = _ssd_inputs(B, T, nl, FO, 100 * B + nl, dtype=torch.float64)
    ry, rz = _ssd_f64(a_s, mp, ms, mask, ps, nl)
    y, frames = R.decode_chain(a_s, mp, ms, mask, ps, nl)
    assert torch.allclose(y, ry, rtol=1e-12, atol=1e-13)
    assert torch.allclose(torch.stack([f["ffn"]["pre"] for f in frames]), rz, rtol=1e-12, atol=1e-13)


def test_fp32_composite_is_the_same_formula():
    name = "B9-H68-HB33-FO8"
    for kind, calls in R.CALLS.items():
        for kw, outs in calls:
            ref, got = R.reference(name, kind, **kw), R.composite(name, kind, **kw)
            for n in outs:
                assert got[n].dtype == torch.float32 and ref[n].dtype == torch.float64
                assert R.worst(got[n], ref[n], R.BLOCKS.get(n, 1)) < 1e-5, (kind, kw, n)   # fp32 rounding only
            assert any(R.worst(got[n], ref[n], R.BLOCKS.get(n, 1)) > 0 for n in outs)


# ---------------------------------------------------------------- buffers and the measure
def test_guarded_places_the_rows_between_sentinels():
    buf, view = R.guarded(3, 4, row_stride=7, offset=2, lead=8)
    assert buf.numel() == 8 + 5 * 7 and view.shape == (3, 4) and view.stride() == (7, 1)
    assert view.data_ptr() == buf.data_ptr() + 10 * 4 and bool((view == R.FILL).all())
    assert int((buf == SENTINEL).sum()) == buf.numel() - 12 and outside_intact(buf, view)
    view.fill_(1.0)
    assert outside_intact(buf, view)
    for i in (0, 9, 14, 16, 10 + 2 * 7 + 4, buf.numel() - 1):   # lead, offset, row gaps, behind
        b2 = buf.clone()
        b2[i] = 0.0
        assert not outside_intact(b2, b2.as_strided((3, 4), (7, 1), 10)), i
    buf, view = R.guarded(1, 5)
    assert view.is_contiguous() and view.data_ptr() % 16 == buf.data_ptr() % 16


def test_poisoned_rows_follow_the_real_ones():
    t = torch.arange(12, dtype=torch.float32).view(3, 4)
    p = R.poisoned(t, spare=2)
    assert torch.equal(p, t) and p.is_contiguous()
    behind = p.as_strided((2, 4), (4, 1), 12)
    assert bool(torch.isnan(behind).all())
    v = R.poisoned(torch.ones(5), spare=3)
    assert bool(torch.isnan(v.as_strided((3,), (1,), 5)).all())
    s = R.poisoned_slice(torch.ones(2, 3, 4))
    assert s.stride() == (4 * 6, 6, 1) and bool((s == 1).all())
    whole = s.as_strided((3, 4, 6), (24, 6, 1), 0)
    assert int(torch.isnan(whole).sum()) == 3 * 4 * 6 - 2 * 3 * 4


def test_row_errs_is_per_row_and_block():
    ref = torch.ones(3, 8, dtype=torch.float64)
    ref[:, :2] = 1000.0                        # block 0 large
    a = ref.clone()
    a[1, 5] += 1e-3                            # an error in small block 2 of row 1
    e = R.row_errs(a, ref, blocks=4)
    assert e.shape == (3, 4) and abs(e[1, 2].item() - 1e-3) < 1e-12 and e.sum().item() == e[1, 2].item()
    assert abs(R.worst(a, ref) - 1e-6) < 1e-12   # hidden behind the large block without the blocks
    b = ref.clone()
    b[2, 7] = float("nan")
    assert R.row_errs(b, ref, 4)[2, 3].item() == float("inf") and R.row_errs(b, ref, 4)[:2].max().item() == 0
    # a zero slice: exact without a scale, measured against the scale with one
    z = ref.clone()
    z[:, 2:4] = 0
    c = z.clone()
    assert R.row_errs(c, z, 4).max().item() == 0
    c[0, 3] = 1e-9
    assert R.row_errs(c, z, 4)[0, 1].item() == float("inf")
    e = R.row_errs(c, z, 4, zero_scale=torch.tensor([0.5, 0.5, 0.5]))
    assert abs(e[0, 1].item() - 2e-9) < 1e-20 and e.sum().item() == e[0, 1].item()
    v = R.row_errs(torch.tensor([1.0, 2.2]), torch.tensor([1.0, 2.0]))
    assert v.shape == (2, 1) and abs(v[1, 0].item() - 0.1) < 1e-6


# ---------------------------------------------------------------- the case table
def test_case_table_covers_every_edge():
    cs = R.CASES
    assert len({c.name for c in cs}) == len(cs) and 18 <= len(cs) <= 24
    assert {c.H for c in cs} == {4, 36, 64, 68, 128, 132, 252, 256}
    assert {c.B for c in cs} == {1, 7, 8, 9, 16, 17, 33}
    assert {c.HB for c in cs} == {1, 7, 8, 33, 64}
    assert {c.FO for c in cs} == {1, 6, 8}
    assert {c.H for c in R.LN_CASES} == {1, 5, 255}
    for cl in ("H<=64", "H<=128", "H<=256"):   # every dispatch class sees a partial row and column tile
        mine = [c for c in cs if R.h_class(c.H) == cl]
        assert any(c.B % 8 and c.B % 16 for c in mine) and any(c.HB % 8 for c in mine) and any(c.H % 8 for c in mine)


@pytest.mark.parametrize("name", R.NAMES + R.LN_NAMES)
def test_case_meets_its_conditions(name):
    """By the inputs alone: every compared slice of the float64 reference is finite and non-zero, except the
    forget block of dG, a row of mrg_ssd_ffn_z_fwd's z whose units are all off (both exactly zero in the
    kernel too) and, at H = 1, g, dG and dyx of mrg_ssd_ln_cell_bwd (the only slices measured against
    zero_scale); with mask[t] = 0 the next-frame term is exactly absent; and plain fp32 arithmetic holds
    every slice within a tenth of the bound, so that a kernel that misses the bound is wrong and not
    unlucky with a cancelling slice."""
    c, x = R.BY_NAME[name], R.inputs(name)
    assert R._usable(x) and R._conditioned(c, x)
    assert c.HB < 7 or bool((x["z"] == 0).any() and (x["z"] < 0).any() and (x["z"] > 0).any())
    zs = R.zero_scale(x["du_in"], x["gamma"], x["rstd"])
    assert bool((zs > 0).all())
    for kind, kw, outs in R.calls_of(c):
        ref, yard = R.reference(name, kind, **kw), R.composite(name, kind, **kw)
        for n in outs:
            blocks = R.BLOCKS.get(n, 1)
            r = ref[n].reshape(c.B, blocks, -1)
            assert bool(torch.isfinite(r).all())
            zero = r.abs().amax(-1) == 0
            want = torch.zeros_like(zero)
            if n == "dG":
                want[:, 1] = True
            if c.H == 1 and n in R.ZERO_AT_H1:
                want[:] = True
            if kind == "ffn_z" and n == "z":
                want[:, 0] = (ref["pre"] <= 0).all(-1)
            assert torch.equal(zero, want), (kind, kw, n)
            scale = zs if (c.H == 1 and n in R.ZERO_AT_H1) else None
            e = R.worst(yard[n], ref[n], blocks, scale)
            assert e < R.COND == TOL / 10, (kind, kw, n, e)
        if kind == "ffn_bwd" and kw["sel"] == 0:
            assert torch.equal(ref["dyt"], x["dy"][:, kw["t"]].double())
        if kind == "ffn_bwd" and kw["sel"] == 1 and kw["form"] != "none":
            assert not torch.equal(ref["dyt"], x["dy"][:, kw["t"]].double())


@pytest.mark.parametrize("case", R.COMPOSE)
def test_composition_cases_stay_off_the_relu_kink(case):
    ref = R.compose_reference(case)
    B, T, H, HB, FO, nl = case
    assert ref["pre"].shape == (T, B, HB) and _no_kinks(ref["pre"])
    assert ref["y"].abs().max() > 0 and ref["da"].abs().max() > 0
    for i, g in enumerate(ref["grads"]):
        is_whh = 2 <= i < 2 + 6 * nl and (i - 2) % 6 == 1
        assert bool(g.abs().max() == 0) == is_whh, i
