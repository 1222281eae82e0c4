"""mrg_gen_lstm, mrg_gen_linear and mrg_gen_ffn (csrc/gen.hip) through the C ABI against the float64
restatements of tests/gen_ref.py, at their launch edges: B below, at and past one 16-row tile and over
several; every prologue, mode and output form; every self-motion width class.  Each output sits between NaN
guard zones that must stay NaN, and each row-indexed input is followed by a NaN row (or sits between NaN
frames), so a read or write outside the B rows shows.

Bar: rel_err < 1e-4 (max |a - ref| / max |ref|, tests.golden_util), the TOL of test_gpu_generation_gru.py and
test_gpu_generation_ratio.py for these fp32 per-frame kernels against float64."""
import pytest
import torch

from tests.gen_ref import gen_ffn_ref, gen_linear_ref, gen_lstm_ref
from tests.gen_util import DEV, E, GUARD, _done, _guarded, _inside, _lib, _poisoned, _ptr, _stream  # noqa: F401
from tests.golden_util import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
EPS = 1e-5
HB = 64


def _arr(*ps):
    from multimodalreactiongeneration_amd.generate import _arr as arr
    return arr(*ps)


def _gen(seed):
    g = torch.Generator().manual_seed(seed)
    return lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale


def _dev(t):
    return t.to(DEV).contiguous()


def _ok(rc):
    torch.cuda.synchronize()
    assert rc == 0, _lib().mrg_last_error()


def _close(what, **pairs):
    errs = {}
    for name, (got, want) in pairs.items():
        assert bool(torch.isfinite(got).all()), name
        errs[name] = rel_err(got, want)
    print(f"{what}: rel_err " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(e < TOL for e in errs.values()), errs


# ------------------------------------------------------------------ mrg_gen_lstm
def _lstm_inputs(B, fm, seed):
    """Weights of one LSTM mixer and the inputs of one prologue (fm = 0: the LayerNorm form)."""
    rn = _gen(seed)
    d = dict(w_ih=rn(4 * E, E, scale=E ** -0.5), b_ih=rn(4 * E, scale=0.3), b_hh=rn(4 * E, scale=0.3))
    if fm:
        d.update(ms=rn(B, fm), fe_w=rn(E, fm, scale=fm ** -0.5), fe_b=rn(E, scale=0.3))
    else:
        d.update(a=rn(B, E), r=rn(B, E), ga=1.0 + rn(E, scale=0.2), be=rn(E, scale=0.2))
    return d


def _lstm_call(B, fm, d, **over):
    """d: the inputs by name; over: xw and h, and what replaces an input's pointer."""
    p = {k: _ptr(d.get(k)) for k in ("ms", "fe_w", "fe_b", "a", "r", "ga", "be", "w_ih", "b_ih", "b_hh")}
    p.update(over)
    return _lib().mrg_gen_lstm(B, fm, p["ms"], p["fe_w"], p["fe_b"], p["a"], p["r"], p["ga"], p["be"], EPS, p["xw"],
                               p["w_ih"], p["b_ih"], p["b_hh"], p["h"], _stream())


@pytest.mark.parametrize("fm", [0, 3, 6, 16])   # 0: X = LN(a + r); else X = ms W_fe^T + b_fe
@pytest.mark.parametrize("B", [1, 16, 17, 64])
def test_gen_lstm_vs_float64(B, fm):
    d = _lstm_inputs(B, fm, seed=100 * B + fm)
    dd = {k: (_poisoned(v) if k in ("ms", "a", "r") else _dev(v)) for k, v in d.items()}
    xw, h = _guarded(B * E), _guarded(B * E)
    _ok(_lstm_call(B, fm, dd, xw=_ptr(xw, GUARD), h=_ptr(h, GUARD)))
    want_x, want_h = gen_lstm_ref(eps=EPS, **d)
    _close(f"gen_lstm B={B} fm={fm}", xw=(_inside(xw, B, E), want_x), h=(_inside(h, B, E), want_h))


def test_gen_lstm_refusals():
    lib = _lib()
    B = 4
    ln = {k: _dev(v) for k, v in _lstm_inputs(B, 0, seed=5).items()}
    emb = {k: _dev(v) for k, v in _lstm_inputs(B, 16, seed=6).items()}
    xw, h = (torch.full((B, E), 7.5, device=DEV) for _ in range(2))
    wide = dict(emb, ms=torch.zeros(B, 17, device=DEV), fe_w=torch.zeros(E, 17, device=DEV))
    both = dict(emb, **{k: ln[k] for k in ("a", "r", "ga", "be")})
    weights = {k: emb[k] for k in ("w_ih", "b_ih", "b_hh")}
    cases = [("fm = 17", 17, wide, {}), ("fm = 0 with ms", 0, emb, {}), ("no prologue", 16, weights, {}),
             ("half a LayerNorm prologue", 0, dict(weights, a=ln["a"], r=ln["r"]), {}),
             # since library version 106 (the launcher mrg_gen_gru's checks came from)
             ("both prologues", 16, both, {})]
    cases += [(f"null {k}", fm, src, {k: None}) for k in ("xw", "w_ih", "b_ih", "b_hh", "h")
              for fm, src in ((16, emb), (0, ln))]
    for what, fm, src, over in cases:
        assert _lstm_call(B, fm, src, **{"xw": _ptr(xw), "h": _ptr(h), **over}) != 0, what
        assert lib.mrg_last_error(), what
        torch.cuda.synchronize()
        assert bool((xw == 7.5).all()) and bool((h == 7.5).all()), what
    assert _lstm_call(0, 16, emb, xw=_ptr(xw), h=_ptr(h)) == 0 and _lstm_call(0, 0, ln, xw=_ptr(xw), h=_ptr(h)) == 0
    torch.cuda.synchronize()
    assert bool((xw == 7.5).all()) and bool((h == 7.5).all())


# ------------------------------------------------------------------ mrg_gen_linear
def _lnp(rn):
    return 1.0 + rn(E, scale=0.2), rn(E, scale=0.2)


@pytest.mark.parametrize("keep_rows", [True, False])   # False: xw null, as the query projection calls it
@pytest.mark.parametrize("B", [1, 16, 17])
def test_gen_linear_mode0_vs_float64(B, keep_rows):
    rn = _gen(200 + B)
    a, r, (ga, be), w, bias = rn(B, E), rn(B, E), _lnp(rn), rn(E, E, scale=E ** -0.5), rn(E, scale=0.3)
    ad, rd, gad, bed, wd, bd = _poisoned(a), _poisoned(r), _dev(ga), _dev(be), _dev(w), _dev(bias)
    xw, out = _guarded(B * E), _guarded(B * E)
    _ok(_lib().mrg_gen_linear(0, B, _arr(ad), _arr(rd), _arr(gad), _arr(bed), E, None, None, None, EPS,
                              _ptr(xw, GUARD) if keep_rows else None, E if keep_rows else 0, _arr(wd), _arr(bd),
                              _ptr(out, GUARD), E, _stream()))
    want_x, want = gen_linear_ref(0, a, r, ga, be, w, bias, eps=EPS)
    pairs = dict(out=(_inside(out, B, E), want))
    if keep_rows:
        pairs["xw"] = (_inside(xw, B, E), want_x)
    else:
        assert bool(torch.isnan(xw).all())
    _close(f"gen_linear mode 0 B={B} xw={keep_rows}", **pairs)


@pytest.mark.parametrize("B", [1, 16, 17])
def test_gen_linear_mode1_vs_float64(B):
    """The two integrators; a2[i] points at frame 1 of a [3][B][256] tensor whose other frames are NaN, as
    the frame loop passes the hoisted attention outputs."""
    rn = _gen(300 + B)
    a, r, (ga, be) = rn(B, E), rn(B, E), _lnp(rn)
    a2, p2 = [rn(B, E) for _ in range(2)], [_lnp(rn) for _ in range(2)]
    w, bias = [rn(E, E, scale=E ** -0.5) for _ in range(2)], [rn(E, scale=0.3) for _ in range(2)]
    ad, rd, gad, bed = _poisoned(a), _poisoned(r), _dev(ga), _dev(be)
    att = [torch.full((3, B, E), float("nan"), device=DEV) for _ in range(2)]
    for t, src in zip(att, a2):
        t[1] = src.to(DEV)
    g2, b2 = [_dev(p[0]) for p in p2], [_dev(p[1]) for p in p2]
    wd, bd = [_dev(t) for t in w], [_dev(t) for t in bias]
    xw, out = _guarded(B * 2 * E), _guarded(B * 2 * E)
    _ok(_lib().mrg_gen_linear(1, B, _arr(ad), _arr(rd), _arr(gad), _arr(bed), E,
                              _arr(_ptr(att[0], B * E), _ptr(att[1], B * E)), _arr(*g2), _arr(*b2), EPS,
                              _ptr(xw, GUARD), 2 * E, _arr(*wd), _arr(*bd), _ptr(out, GUARD), 2 * E, _stream()))
    want_x, want = gen_linear_ref(1, a, r, ga, be, w, bias, a2, [p[0] for p in p2], [p[1] for p in p2], eps=EPS)
    _close(f"gen_linear mode 1 B={B}", xw=(_inside(xw, B, 2 * E), want_x), out=(_inside(out, B, 2 * E), want))


@pytest.mark.parametrize("B", [1, 16, 17])
def test_gen_linear_mode2_vs_float64(B):
    """cat_linear; the two halves are pointers into one [B][512] buffer, lda = 512, as the frame loop
    passes the integrators' outputs and their residual rows."""
    rn = _gen(400 + B)
    a, r = rn(B, 2 * E), rn(B, 2 * E)
    p = [_lnp(rn) for _ in range(2)]
    w, bias = rn(E, 2 * E, scale=(2 * E) ** -0.5), rn(E, scale=0.3)
    ad, rd, wd, bd = _poisoned(a), _poisoned(r), _dev(w), _dev(bias)
    gd, bed = [_dev(q[0]) for q in p], [_dev(q[1]) for q in p]
    out = _guarded(B * E)
    _ok(_lib().mrg_gen_linear(2, B, _arr(_ptr(ad), _ptr(ad, E)), _arr(_ptr(rd), _ptr(rd, E)), _arr(*gd), _arr(*bed),
                              2 * E, None, None, None, EPS, None, 0, _arr(wd), _arr(bd), _ptr(out, GUARD), E,
                              _stream()))
    halves = lambda t: [t[:, :E], t[:, E:]]
    _, want = gen_linear_ref(2, halves(a), halves(r), [q[0] for q in p], [q[1] for q in p], w, bias, eps=EPS)
    _close(f"gen_linear mode 2 B={B}", out=(_inside(out, B, E), want))


def test_gen_linear_refusals():
    lib = _lib()
    B = 4
    rn = _gen(7)
    t = [_dev(rn(B, E)) for _ in range(2)] + [_dev(rn(E)) for _ in range(2)]
    a, r, ga, be = (_arr(x, x) for x in t)
    wt, bt = _dev(rn(E, E)), _dev(rn(E))
    w, bias = _arr(wt, wt), _arr(bt, bt)
    xw, out = (torch.full((B, 2 * E), 7.5, device=DEV) for _ in range(2))

    def call(mode, B_=B, a_=a, w_=w, a2=None, out_=_ptr(out)):
        return lib.mrg_gen_linear(mode, B_, a_, r, ga, be, E, a2, a2, a2, EPS, _ptr(xw), 2 * E, w_, bias, out_, 2 * E,
                                  _stream())
    for what, rc in (("mode 3", call(3)), ("mode -1", call(-1)), ("null a", call(0, a_=None)),
                     ("null w", call(0, w_=None)), ("null out", call(2, out_=None)),
                     ("mode 1 without the second LayerNorm", call(1))):
        assert rc != 0 and lib.mrg_last_error(), what
    assert call(0, B_=0) == 0 and call(1, B_=0, a2=a) == 0
    torch.cuda.synchronize()
    assert bool((xw == 7.5).all()) and bool((out == 7.5).all())


# ------------------------------------------------------------------ mrg_gen_ffn
def _ffn_inputs(B, N, prologue, seed):
    rn = _gen(seed)
    d = dict(a=rn(B, E), w1=rn(HB, E, scale=E ** -0.5), b1=rn(HB, scale=0.3), w2=rn(N, HB, scale=HB ** -0.5),
             b2=rn(N, scale=0.3))
    if prologue:
        d.update(r=rn(B, E), ga=1.0 + rn(E, scale=0.2), be=rn(E, scale=0.2))
    return d


def _ffn_call(B, N, dd, out=None, pred=None, pred_bs=0, ms_next=None, ms_src=None, mask=None, t=0):
    p = lambda k: _ptr(dd.get(k))
    return _lib().mrg_gen_ffn(B, N, p("a"), p("r"), p("ga"), p("be"), EPS, p("w1"), p("b1"), p("w2"), p("b2"), out,
                              pred, pred_bs, ms_next, ms_src, mask, t, _stream())


@pytest.mark.parametrize("prologue", [False, True])   # X = a, or X = LN(a + r)
@pytest.mark.parametrize("B", [1, 16, 17])
def test_gen_ffn_block_vs_float64(B, prologue):
    d = _ffn_inputs(B, E, prologue, seed=500 + 2 * B + prologue)
    dd = {k: (_poisoned(v) if k in ("a", "r") else _dev(v)) for k, v in d.items()}
    out = _guarded(B * E)
    _ok(_ffn_call(B, E, dd, out=_ptr(out, GUARD)))
    _close(f"gen_ffn N=256 B={B} ln={prologue}", out=(_inside(out, B, E), gen_ffn_ref(eps=EPS, **d)))


@pytest.mark.parametrize("prologue", [False, True])
@pytest.mark.parametrize("t", [0, 2])
@pytest.mark.parametrize("N", [1, 6, 16])
@pytest.mark.parametrize("B", [1, 16, 17])
def test_gen_ffn_output_vs_float64(B, N, t, prologue):
    """The output FeedForward: y into pred[:, t] of [B][T = 3][N] (the other frames stay as they were) and
    ms_next = mask[t] ? y : ms_src; the mask is true at t = 0 and false at t = 2."""
    T = 3
    d = _ffn_inputs(B, N, prologue, seed=600 + 100 * B + 10 * N + 2 * t + prologue)
    src = _gen(B + N)(B, N)
    dd = {k: (_poisoned(v) if k in ("a", "r") else _dev(v)) for k, v in d.items()}
    mask = torch.tensor([1, 0, 0], dtype=torch.uint8, device=DEV)
    pred, nxt = _guarded(B * T * N), _guarded(B * N)
    pred[GUARD:GUARD + B * T * N] = 7.5
    srcd = _poisoned(src)
    _ok(_ffn_call(B, N, dd, pred=_ptr(pred, GUARD), pred_bs=T * N, ms_next=_ptr(nxt, GUARD), ms_src=_ptr(srcd),
                  mask=_ptr(mask), t=t))
    want, want_next = gen_ffn_ref(eps=EPS, ms_src=src, mask_t=bool(mask[t]), **d)
    got = _inside(pred, B, T, N)
    assert bool((got[:, [u for u in range(T) if u != t]] == 7.5).all())
    got_next = _inside(nxt, B, N)
    if mask[t]:
        assert torch.equal(got_next, got[:, t])
    else:
        assert torch.equal(got_next, src)
    _close(f"gen_ffn N={N} B={B} t={t} ln={prologue}", pred=(got[:, t], want), ms_next=(got_next, want_next))


def test_gen_ffn_refusals():
    lib = _lib()
    B, T = 4, 3
    blk = {k: _dev(v) for k, v in _ffn_inputs(B, E, True, seed=8).items()}
    outp = {k: _dev(v) for k, v in _ffn_inputs(B, 6, True, seed=9).items()}
    out = torch.full((B, E), 7.5, device=DEV)
    pred, nxt, src = (torch.full((B, T, 6), 7.5, device=DEV) for _ in range(3))
    mask = torch.ones(T, dtype=torch.uint8, device=DEV)
    full = dict(pred=_ptr(pred), pred_bs=T * 6, ms_next=_ptr(nxt), ms_src=_ptr(src), mask=_ptr(mask))
    without = lambda d, *ks: {k: v for k, v in d.items() if k not in ks}
    for what, rc in (("N = 6 with out alone", _ffn_call(B, 6, outp, out=_ptr(out))),
                     ("N = 256 without out", _ffn_call(B, E, blk)),
                     ("N = 17 with pred", _ffn_call(B, 17, outp, **full)),
                     ("N = 0 with pred", _ffn_call(B, 0, outp, **full)),
                     ("pred without ms_next", _ffn_call(B, 6, outp, **dict(full, ms_next=None))),
                     ("pred without the mask", _ffn_call(B, 6, outp, **dict(full, mask=None))),
                     ("null a", _ffn_call(B, E, without(blk, "a"), out=_ptr(out))),
                     ("null w2", _ffn_call(B, E, without(blk, "w2"), out=_ptr(out))),
                     ("r without gamma", _ffn_call(B, E, without(blk, "ga"), out=_ptr(out)))):
        assert rc != 0 and lib.mrg_last_error(), what
    assert _ffn_call(0, E, blk, out=_ptr(out)) == 0 and _ffn_call(0, 6, outp, **full) == 0
    torch.cuda.synchronize()
    assert all(bool((x == 7.5).all()) for x in (out, pred, nxt))
