"""tests/attention_ref.py checked on the CPU: the float64 attention core against two independent
restatements (tests/dropout_ref.mha and the oracle's mha with gen_attention_mask), and the conditions the
case table of tests/test_gpu_attention.py must meet by its inputs alone."""
import math

import pytest
import torch

from oracle import mrg_oracle as O
from tests import attention_ref as R
from tests import dropout_ref

# one causal Tk = r Tq case, one Tq = r Tk case and one padded case (leading flags, Tk = r Tq)
AGREE = ["33x132c-none", "66x33c-none", "33x132c-leading", "130x130c-scattered", "65x129n-tail"]


def _identity_mha(E):
    eye = torch.eye(E, dtype=torch.float64)
    return torch.cat([eye, eye, eye]), torch.zeros(3 * E, dtype=torch.float64), eye, torch.zeros(E, dtype=torch.float64)


@pytest.mark.parametrize("name", AGREE)
def test_core_matches_dropout_ref_and_oracle(name):
    """With identity projections and zero biases nn.MultiheadAttention is the core itself (K = V = kv)."""
    c, D = R.BY_NAME[name], 16
    x = R.inputs(name, D)
    E = R.HEADS * D
    q, kv = x["q"].double(), x["k"].double()
    out, lse = R.core(q, kv, kv, R.HEADS, x["scale"], R.case_vis(c))
    assert not torch.isnan(out).any()
    in_w, in_b, out_w, out_b = _identity_mha(E)
    ref = dropout_ref.mha(q, kv, in_w, in_b, out_w, out_b, R.HEADS, c.causal, x["qpad"], x["kpad"])
    assert torch.allclose(out, ref, rtol=1e-12, atol=1e-13)
    if not c.causal:
        return   # gen_attention_mask is always block-causal
    # the oracle reads the padding flags from feature 0 of the rows: mark them there, in q and kv alike
    main, other = q.clone(), kv.clone()
    if x["qpad"] is not None:
        main[..., 0] = torch.where(x["qpad"].bool(), torch.full_like(main[..., 0], O.PADDING_VALUE), main[..., 0])
        other[..., 0] = torch.where(x["kpad"].bool(), torch.full_like(other[..., 0], O.PADDING_VALUE), other[..., 0])
    mask = O.gen_attention_mask(main, other, R.HEADS)
    assert torch.equal(~mask[:, 0], R.case_vis(c))
    sd = {"a.in_proj_weight": in_w, "a.in_proj_bias": in_b, "a.out_proj.weight": out_w, "a.out_proj.bias": out_b}
    got, _ = R.core(main, other, other, R.HEADS, x["scale"], ~mask[:, 0])
    assert torch.allclose(got, O.mha(main, other, sd, "a.", R.HEADS, mask), rtol=1e-12, atol=1e-13)


def test_core_matches_scalar_loops():
    """O, lse and the gradients against the definition written with Python floats, element by element."""
    B, Tq, Tk, H, D = 1, 4, 8, 2, 3
    g = torch.Generator().manual_seed(5)
    q, k, v, do = (torch.randn(B, T, H * D, generator=g, dtype=torch.float64) for T in (Tq, Tk, Tk, Tq))
    qpad = torch.tensor([[0, 1, 0, 1]], dtype=torch.uint8)
    kpad = torch.tensor([[1, 0, 0, 1, 0, 0, 1, 0]], dtype=torch.uint8)
    vis = dropout_ref.visible(Tq, Tk, True, qpad, kpad, B)
    out, lse, dq, dk, dv = R.core(q, k, v, H, 0.7, vis, do)
    edq, edk, edv = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
    for h in range(H):
        d = slice(h * D, (h + 1) * D)
        for i in range(Tq):
            keys = [j for j in range(Tk) if vis[0, i, j]]
            s = {j: 0.7 * sum(float(q[0, i, c]) * float(k[0, j, c]) for c in range(d.start, d.stop)) for j in keys}
            z = sum(math.exp(s[j]) for j in keys)
            p = {j: math.exp(s[j]) / z for j in keys}
            assert abs(float(lse[0, h, i]) - math.log(z)) < 1e-12
            dp = {j: float(do[0, i, d] @ v[0, j, d]) for j in keys}
            delta = sum(p[j] * dp[j] for j in keys)
            for c in range(d.start, d.stop):
                assert abs(float(out[0, i, c]) - sum(p[j] * float(v[0, j, c]) for j in keys)) < 1e-12
            for j in keys:
                ds = p[j] * (dp[j] - delta) * 0.7
                edq[0, i, d] += ds * k[0, j, d]
                edk[0, j, d] += ds * q[0, i, d]
                edv[0, j, d] += p[j] * do[0, i, d]
    for got, exp in ((dq, edq), (dk, edk), (dv, edv)):
        assert torch.allclose(got, exp, rtol=1e-11, atol=1e-12)


def test_fp32_composite_is_the_same_formula():
    x = R.inputs("65x65c-tail", 8)
    ref = R.reference("65x65c-tail", 8)
    got = R.fp32_composite(x["q"], x["k"], x["v"], R.HEADS, x["scale"], R.case_vis(R.BY_NAME["65x65c-tail"]), x["dout"])
    assert all(t.dtype == torch.float32 for t in got)
    for n, t in zip(("O", "lse", "dQ", "dK", "dV"), got):
        assert 0 < R.slice_err(t, ref[n]) < 1e-5, n   # float32 rounding, nothing else


def test_strided_places_rows_and_guards():
    t = torch.arange(2 * 3 * 5, dtype=torch.float32).view(2, 3, 5)
    buf, view = R.strided(t, 7, 3)
    assert torch.equal(view, t) and view.stride() == (21, 7, 1) and buf.numel() == 3 + (6 + 2) * 7
    assert view.data_ptr() == buf.data_ptr() + 3 * 4 and R.outside_intact(buf, view)
    view.fill_(1.0)
    assert R.outside_intact(buf, view)
    for i in (0, 2, 3 + 5, 3 + 6, 3 + 5 * 7 + 5, buf.numel() - 1):   # lead, row gaps, the spare rows
        b2 = buf.clone()
        b2[i] = 0.0
        assert not R.outside_intact(b2, b2[3:3 + 42].view(2, 3, 7)[:, :, :5]), i


def test_slice_err_is_per_sample_and_head():
    ref = torch.ones(R.B, 4, R.HEADS * 2, dtype=torch.float64)
    ref[:, :, :2] = 1000.0                      # head 0 large
    a = ref.clone()
    a[1, 2, 5] += 1e-3                          # an error in small head 2 of sample 1
    errs = R.slice_errs(a, ref)
    assert errs.shape == (R.B, R.HEADS) and abs(errs[1, 2].item() - 1e-3) < 1e-12 and errs.sum().item() == errs[1, 2].item()
    rows = torch.ones(R.B, R.HEADS, 7, dtype=torch.float64)
    b = rows.clone()
    b[0, 1, 6] = float("nan")
    assert R.slice_errs(b, rows)[0, 1].item() == float("inf") and R.slice_errs(b, rows)[1].max().item() == 0.0
    # a slice that is zero everywhere in the reference: undefined without zero_scale, measured against it with
    z = rows.clone()
    z[1, 0] = 0.0
    a = z.clone()
    a[1, 0, 3] = 1e-6
    scale = torch.full((R.B, R.HEADS), 0.5, dtype=torch.float64)
    assert R.slice_errs(a, z)[1, 0].item() > 1e20
    errs = R.slice_errs(a, z, zero_scale=scale)
    assert abs(errs[1, 0].item() - 2e-6) < 1e-15 and errs.sum().item() == errs[1, 0].item()
    a[0, 0, 0] += 1e-3                          # zero_scale does not touch a slice with a non-zero reference
    assert abs(R.slice_errs(a, z, zero_scale=scale)[0, 0].item() - 1e-3) < 1e-12


# ---------------------------------------------------------------- the case table
def test_case_table_covers_the_grid():
    """Every shape x padding pattern is there except the padded forms of the single (query, key) pair."""
    names = {c.name for c in R.CASES}
    assert len(names) == len(R.CASES)
    for Tq, Tk, causal in R.SHAPES:
        for pad in R.PADS:
            want = pad == "none" or (Tq, Tk) != (1, 1)
            assert (f"{Tq}x{Tk}{'c' if causal else 'n'}-{pad}" in names) == want
    assert sum(len(c.widths) for c in R.CASES) <= 150


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_case_meets_its_conditions(name):
    c = R.BY_NAME[name]
    vis = R.case_vis(c)
    hidden_rows = ~vis.any(-1)
    for D in c.widths:
        ref = R.reference(name, D, "fully_masked" not in c.tags)   # such a row has no defined gradients
        nan = torch.isnan(ref["O"]).any(-1)
        if "fully_masked" in c.tags:
            assert torch.equal(nan, hidden_rows) and bool(hidden_rows[:, 64].all()) and int(hidden_rows.sum()) == R.B
            assert bool(torch.isinf(ref["lse"][:, :, 64]).all())
        else:
            assert not any(bool(torch.isnan(t).any()) or bool(torch.isinf(t).any()) for t in ref.values())
        # a slice whose reference is zero everywhere has no relative error: only the gradients of the
        # single (query, key) pair are (attention_ref.zero_scales is used there and nowhere else)
        for n, t in ref.items():
            t = torch.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0)
            if n != "lse":
                t = t.view(R.B, -1, R.HEADS, D).permute(0, 2, 1, 3)
            zero = t.reshape(R.B, R.HEADS, -1).abs().amax(-1) == 0
            assert bool(zero.all() if (c.Tk == 1 and n in ("dQ", "dK")) else not zero.any()), (n, D)
            if n in ("dQ", "dK"):
                assert bool((R.zero_scales(name, D)[n] > 0).all())
    if "padded" in c.tags:
        causal_only = dropout_ref.visible(c.Tq, c.Tk, c.causal, B=R.B)
        assert all(bool((causal_only[b] & ~vis[b]).any()) for b in range(R.B))
    else:
        assert c.pad == "none"
    if "leading" in c.tags:
        for b in range(R.B):
            assert bool((~vis[b, :, :32].any(-1) & vis[b, :, 32:].any(-1)).any())
    if "large_logits" in c.tags:
        for D in c.widths:
            x = R.inputs(name, D)
            E = R.HEADS * D
            q = x["q"].double().view(R.B, c.Tq, R.HEADS, D).transpose(1, 2)
            k = x["k"].double().view(R.B, c.Tk, R.HEADS, D).transpose(1, 2)
            s = (q @ k.transpose(-1, -2) * x["scale"]).masked_fill(~vis.unsqueeze(1), float("-inf"))
            assert 6.0 < s[torch.isfinite(s)].std().item() < 10.0 and E == q.shape[1] * D
            run = torch.full(s.shape[:-1], float("-inf"), dtype=torch.float64)
            rises = torch.zeros(s.shape[:-1], dtype=torch.long)
            for k0 in range(0, c.Tk, 32):   # the kernels' online-softmax update: 32 keys at a time, in key order
                gmax = s[..., k0:k0 + 32].amax(-1)
                rises += ((gmax > run) & torch.isfinite(run)).long()
                run = torch.maximum(run, gmax)
            assert int(rises.amax()) >= 2
