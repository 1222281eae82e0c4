"""tests/gru_ref.py is itself checked on the CPU: its forward against torch.nn.GRU and its backward against
autograd of the same graph, float64 against float64 (1e-12 relative), and the case table's own claims
(the 19 instantiated tiles, which of them stage their own saved values)."""
import pytest
import torch

from tests import gru_ref as R
from tests.golden_util import rel_err

RTOL = 1e-12
B, T, IN = 5, 7, 6


def _draw(H, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    k = H ** -0.5
    return dict(x=r(B, T, IN), w_ih=r(3 * H, IN) * k, w_hh=r(3 * H, H) * k, b_ih=r(3 * H) * k, b_hh=r(3 * H) * k,
                h0=r(B, H) * 0.5, dy=r(B, T, H), dhT=r(B, H))


@pytest.mark.parametrize("with_h0", [False, True])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("H", [4, 32])
def test_forward_is_torch_gru(H, reverse, with_h0):
    """y and the last state of forward() equal a one-layer, one-direction torch.nn.GRU on gx = x W_ih^T +
    b_ih (the reverse order: the GRU on the flipped sequence); gates and ghn reproduce y step by step."""
    d = _draw(H, 10 * H + 2 * reverse + with_h0)
    ref = torch.nn.GRU(IN, H, batch_first=True).double()
    ref.load_state_dict({"weight_ih_l0": d["w_ih"], "weight_hh_l0": d["w_hh"], "bias_ih_l0": d["b_ih"],
                         "bias_hh_l0": d["b_hh"]})
    h0 = d["h0"] if with_h0 else None
    with torch.no_grad():
        yr, hr = ref(d["x"].flip(1) if reverse else d["x"], None if h0 is None else h0[None])
        yr = yr.flip(1) if reverse else yr
        f = R.forward(d["x"] @ d["w_ih"].t() + d["b_ih"], d["w_hh"], d["b_hh"], h0, reverse)
    assert rel_err(f["y"], yr) < RTOL
    assert rel_err(f["y"][:, 0 if reverse else T - 1], hr[0]) < RTOL
    # the saved tensors are those of the same steps
    order = list(R.steps(T, reverse))
    for i, t in enumerate(order):
        hp = f["y"][:, order[i - 1]] if i else (torch.zeros(B, H, dtype=torch.float64) if h0 is None else h0)
        z, n = f["gates"][:, t, H:2 * H], f["gates"][:, t, 2 * H:]
        assert rel_err((1 - z) * n + z * hp, f["y"][:, t]) < RTOL
        assert rel_err(hp @ d["w_hh"][2 * H:].t() + d["b_hh"][2 * H:], f["ghn"][:, t]) < RTOL


@pytest.mark.parametrize("form", [f.name for f in R.FORMS])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("H", [4, 32])
def test_backward_is_autograd(H, reverse, form):
    """dgx, dgh and dh0 of backward(), from the saved tensors alone, equal autograd's gradients of gx, of
    the per-step recurrent pre-activations h W_hh^T + b_hh and of h0 in the same float64 graph, for every
    form of the nullable arguments (no h0: the gradient of the zero initial state)."""
    f = R.FORM_BY_NAME[form]
    d = _draw(H, 100 * H + 2 * reverse + len(form))
    gx = (d["x"] @ d["w_ih"].t() + d["b_ih"]).requires_grad_(True)
    h0 = (d["h0"] if f.h0 else torch.zeros(B, H, dtype=torch.float64)).clone().requires_grad_(True)
    fw = R.forward(gx, d["w_hh"], d["b_hh"], h0, reverse)
    for gh in fw["gh"]:
        gh.retain_grad()
    loss = (fw["y"] * 0).sum()   # keeps every node in the graph when both gradients are absent
    if f.dy:
        loss = loss + (fw["y"] * d["dy"]).sum()
    if f.dhT:
        loss = loss + (fw["y"][:, 0 if reverse else T - 1] * d["dhT"]).sum()
    loss.backward()
    with torch.no_grad():
        bw = R.backward(d["w_hh"], fw["gates"].detach(), fw["ghn"].detach(), fw["y"].detach(),
                        d["h0"] if f.h0 else None, d["dy"] if f.dy else None, d["dhT"] if f.dhT else None, reverse)
    want = dict(dgx=gx.grad, dgh=torch.stack([gh.grad for gh in fw["gh"]], 1), dh0=h0.grad)
    for k, w in want.items():
        if f.dy or f.dhT:
            assert rel_err(bw[k], w) < RTOL, k
        else:
            assert not bw[k].any() and not w.any(), k


def test_measure_is_per_row_and_gate_block():
    """errs() takes gates / dgx / dgh per (batch row, gate block) over all steps: an error in one block of
    one row shows in that slice alone and is not scaled by a larger block; a zero reference slice must
    be met exactly."""
    ref = torch.ones(2, 3, 6, dtype=torch.float64)
    ref[:, :, 4:] = 100.0
    a = ref.clone()
    a[1, 2, 1] += 0.5   # row 1, block r
    e = R.errs("gates", a, ref)
    assert e.shape == (2, 3) and e[1, 0] == 0.5 and e.sum() == 0.5
    ref[0, :, 2:4] = 0
    a = ref.clone()
    assert R.worst("dgx", a, ref) == 0
    a[0, 0, 2] = 1e-30
    assert R.worst("dgx", a, ref) == float("inf")
    assert R.errs("y", a[:, :, :2], ref[:, :, :2]).shape == (2, 1)


def test_case_table_names_every_instance():
    """19 (H, G, BS) instances: four tiles per group, three at H = 128; tile 1 and the largest tile of the
    groups cover both SELF_IO values (from CW * 64 + BS * U > NT: tile 8 of (256, 4), (64, 1) and (32, 1)
    only); B_RAGGED is ragged at tiles 2, 4 and 8 and at most 256 workgroups at tile 1."""
    assert len(R.TILES) == 19 and len(set(R.TILE_NAMES)) == 19
    assert R.tiles(128, 1) == (1, 2, 4) and all(R.tiles(H, G) == (1, 2, 4, 8) for H, G in R.HG if H != 128)
    assert sorted((t.H, t.G, t.bs) for t in R.TILES if t.self_io) == [(32, 1, 8), (64, 1, 8), (256, 4, 8)]
    assert {R.TILE_BY_NAME[n].self_io for n in R.EDGE_NAMES} == {False, True}
    assert (R.fwd_threads(256, 4), R.fwd_threads(256, 8), R.fwd_threads(128, 1), R.fwd_threads(64, 1),
            R.fwd_threads(32, 1)) == (768, 384, 768, 768, 384)
    assert [R.bwd_threads(H, G) for H, G in R.HG] == [512, 512, 1024, 512, 256]
    assert all(R.B_RAGGED % bs for bs in (2, 4, 8)) and R.B_RAGGED * 8 <= 256
    assert R.FORM_BY_NAME["none"].dy is False and R.FORM_BY_NAME["none"].dhT is False


def test_reference_tables_are_shared_and_fp32_is_close():
    """The cached references are computed once per case, and the float32 yardstick of the same formulas is
    within the GPU tests' bound of them at the shapes they run (else the bound would ask more of a kernel
    than fp32 arithmetic gives)."""
    H, Bt, Tt = 64, R.B_RAGGED, R.T_FULL
    assert R.fwd_reference(H, Bt, Tt, False, True) is R.fwd_reference(H, Bt, Tt, False, True)
    f64, f32 = R.fwd_reference(H, Bt, Tt, True, True), R.fwd_reference(H, Bt, Tt, True, True, torch.float32)
    for k in ("y", "gates", "ghn"):
        assert f32[k].dtype == torch.float32 and R.worst(k, f32[k], f64[k]) < 1e-5, k
    b64, b32 = R.bwd_reference(H, Bt, Tt, True, "full"), R.bwd_reference(H, Bt, Tt, True, "full", torch.float32)
    for k in ("dgx", "dgh", "dh0"):
        assert R.worst(k, b32[k], b64[k]) < 1e-5, k
    none = R.bwd_reference(H, Bt, Tt, False, "none")
    assert not any(v.any() for v in none.values())
