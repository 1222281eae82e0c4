"""Fused generation for GRU embedding mixers (config_gru.yaml): mrg_gen_gru (csrc/gen.hip) through the C
ABI against the float64 restatement of tests/gen_ref.py, and the GenPlan of generate.py with GRU main
chains and / or GRU side stacks against the per-frame module forward (lstmformer.py:426-547).

Kernel bar: rel_err < 1e-4 (max |a - ref| / max |ref|, tests.golden_util: the project's kernel-vs-float64
bar).  Plan bar: rel_err(fast, slow) < 1e-5, the bar of test_generation_ratio_fused_matches_module_path:
both paths do fp32 arithmetic on the same kernel family."""
import pytest
import torch

from tests.gen_ref import gen_gru_ref
from tests.gen_util import (DEV, E, GUARD, _case, _done, _fast_both_ways, _graph_replay_is_eager,  # noqa: F401
                            _guarded, _inside, _lib, _model, _poisoned, _ptr, _stream)
from tests.golden_util import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
EPS = 1e-5
GRU3 = ("gru",) * 3


def _inputs(B, fm, seed):
    """Weights of one GRU mixer and the inputs of both prologues (fm = 0: the LayerNorm form)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale
    d = dict(w_ih=rn(3 * E, E, scale=E ** -0.5), b_ih=rn(3 * E, scale=0.3), b_hh=rn(3 * E, scale=0.3))
    if fm:
        d.update(ms=rn(B, fm), fe_w=rn(E, fm, scale=fm ** -0.5), fe_b=rn(E, scale=0.3))
    else:
        d.update(a=rn(B, E), r=rn(B, E), ga=1.0 + rn(E, scale=0.2), be=rn(E, scale=0.2))
    return d


def _run(B, fm, d):
    """(xw, h) [B, 256] of one call, each between two NaN guard zones that must stay NaN."""
    dd = {k: (_poisoned(v) if k in ("ms", "a", "r") else v.to(DEV).contiguous()) for k, v in d.items()}
    bufs = [_guarded(B * E) for _ in range(2)]
    p = lambda k: _ptr(dd.get(k))
    rc = _lib().mrg_gen_gru(B, fm, p("ms"), p("fe_w"), p("fe_b"), p("a"), p("r"), p("ga"), p("be"), EPS,
                            _ptr(bufs[0], GUARD), p("w_ih"), p("b_ih"), p("b_hh"), _ptr(bufs[1], GUARD), _stream())
    torch.cuda.synchronize()
    assert rc == 0, _lib().mrg_last_error()
    return [_inside(buf, B, E) for buf in bufs]


@pytest.mark.parametrize("fm", [0, 3, 6, 16])   # 0: X = LN(a + r); else X = ms W_fe^T + b_fe
@pytest.mark.parametrize("B", [1, 16, 17, 64])
def test_gen_gru_vs_float64(B, fm):
    d = _inputs(B, fm, seed=100 * B + fm)
    xw, h = _run(B, fm, d)
    assert bool(torch.isfinite(xw).all()) and bool(torch.isfinite(h).all())
    want_x, want_h = gen_gru_ref(eps=EPS, **d)
    ex, eh = rel_err(xw, want_x), rel_err(h, want_h)
    print(f"B={B} fm={fm}: rel_err xw {ex:.2e} h {eh:.2e}")
    assert ex < TOL and eh < TOL


def test_gen_gru_refusals():
    lib = _lib()
    B = 4
    ln = {k: v.to(DEV) for k, v in _inputs(B, 0, seed=5).items()}
    emb = {k: v.to(DEV) for k, v in _inputs(B, 16, seed=6).items()}
    xw, h = (torch.full((B, E), 7.5, device=DEV) for _ in range(2))

    def call(B_, fm, src, w_ih):
        p = lambda k: _ptr(src.get(k))
        return lib.mrg_gen_gru(B_, fm, p("ms"), p("fe_w"), p("fe_b"), p("a"), p("r"), p("ga"), p("be"), EPS, _ptr(xw),
                               w_ih, _ptr(ln["b_ih"]), _ptr(ln["b_hh"]), _ptr(h), _stream())
    w = _ptr(ln["w_ih"])
    wide = dict(emb, ms=torch.zeros(B, 17, device=DEV), fe_w=torch.zeros(E, 17, device=DEV))
    both = dict(emb, **{k: ln[k] for k in ("a", "r", "ga", "be")})
    neither = {}
    for what, args in (("fm = 17", (B, 17, wide, w)), ("both prologues", (B, 16, both, w)),
                       ("no prologue", (B, 16, neither, w)), ("null w_ih", (B, 16, emb, None)),
                       ("null w_ih, LayerNorm form", (B, 0, ln, None))):
        assert call(*args) != 0, what
        assert lib.mrg_last_error(), what
        torch.cuda.synchronize()
        assert bool((xw == 7.5).all()) and bool((h == 7.5).all()), what
    assert call(0, 16, emb, w) == 0 and call(0, 0, ln, w) == 0
    torch.cuda.synchronize()
    assert bool((xw == 7.5).all()) and bool((h == 7.5).all())


# ------------------------------------------------------------------ which models get a plan
@pytest.mark.parametrize("mixers,r", [(GRU3, 1), (GRU3, 2), (GRU3, 8), (("gru", "lstm", "lstm"), 2),
                                      (("lstm", "lstm", "gru"), 1), (("lstm", "gru", "lstm"), 1)])
def test_plan_exists(mixers, r):
    from multimodalreactiongeneration_amd.generate import plan_for
    m = _model(emb_mixers=mixers, ratio=r)
    assert m.ratio == r
    plan = plan_for(m.eval())
    assert plan is not None and plan.ratio == r
    # emb_mixers is indexed by modality (audio, partner motion, self motion = the main chain)
    assert [b.kind for b in plan.blocks] == [mixers[2]] * 5
    assert [k for k, _ in plan.enc] == list(mixers[:2])
    assert plan.loop_form is (mixers[2] == "lstm")


def test_plan_still_declined():
    from multimodalreactiongeneration_amd import configs as C
    from multimodalreactiongeneration_amd.generate import plan_for
    from multimodalreactiongeneration_amd.model import Metaformer
    from tests.golden_util import config, load
    small = dict(num_block=1, encoder_num_layer=1, emb_mixers=GRU3)
    m = _model(ratio=32, **small)
    assert m.ratio == 32 and plan_for(m.eval()) is None
    # D = 128 is no width of mrg_gen_attention: a plan at one key (no attention runs), none at two
    assert plan_for(_model(ratio=1, num_heads=2, **small).eval()) is not None
    assert plan_for(_model(ratio=2, num_heads=2, **small).eval()) is None
    # dropout: a two-layer GRU is outside the form in either mode; a one-layer model with p > 0 has a
    # plan in eval() and none in train() (its attentions would drop)
    for layers in (2, 1):
        cfg = C.lstmformer_config(**small)
        cfg[0].dropout, cfg[0].num_internal_layer = 0.1, layers
        m = Metaformer(*cfg).to(DEV)
        assert plan_for(m.train()) is None
        assert (plan_for(m.eval()) is not None) is (layers == 1)
        assert plan_for(m.train()) is None
    assert plan_for(_model(hidden=128, **small).eval()) is None
    cfg = config(load("metaformer_gru_r2_pad"))   # hidden 32
    assert plan_for(Metaformer(cfg["model"], cfg["optim"], cfg["metrics"]).to(DEV).eval()) is None


# ------------------------------------------------------------------ the plan against the module path
# (mixers by modality: audio, partner motion, self motion; ratio, B, T).  (2, 64, 9) has T * B = 576
# audio sequences, more than one launch of the GRU recurrence takes on 256 CUs
# (generate.GenPlan._side_stack), so its chunks are joined.  The last case's main chain is an LSTM:
# the persistent loop serves it, reading the GRU partner-motion stack's hoisted attention output.
CASES = [(GRU3, 1, 3, 5), (GRU3, 8, 3, 5), (GRU3, 2, 17, 4), (GRU3, 2, 64, 9), (("gru", "lstm", "lstm"), 2, 3, 5),
         (("lstm", "lstm", "gru"), 1, 3, 5), (("lstm", "gru", "lstm"), 1, 17, 4)]


@pytest.mark.parametrize("mixers,r,B,T", CASES)
def test_generation_gru_fused_matches_module_path(mixers, r, B, T):
    """The plan with GRU mixers (mrg_gen_gru in the main chain; GRU side stacks hoisted as a gate GEMM and
    the zero-state cell at ratio 1, as an r-step zero-state recurrence per frame above it) vs the
    per-frame module forward, ragged padding, scheduled-sampling mask."""
    from multimodalreactiongeneration_amd import _lib as L
    m, batch, mask, slow = _case(mixers, r, B, T)
    fast, loops = _fast_both_ways(m, batch, mask)
    # the one-launch loop is a ratio-1 path for an LSTM main chain, whatever the side stacks are
    fits = L.load().mrg_gen_loop_fits(B, L.cu_count(0)) == 1
    assert loops == {True: int(r == 1 and mixers[2] == "lstm" and fits), False: 0}
    assert fast[True].shape == slow.shape == (B, T, 6)
    assert torch.equal(fast[True], fast[False])
    err = rel_err(fast[True], slow)
    print(f"{mixers} ratio {r} B={B} T={T}: rel_err(fast, slow) {err:.2e}")
    assert err < 1e-5, err


def test_generation_gru_graph_replay():
    """gru x 3 at r = 2 captured once as a HIP graph with the mask in a device buffer, replayed for two
    masks: each replay is the eager fast path's result for its mask, bit for bit."""
    mixers, r, B, T = CASES[2]
    m, batch, mask0, _ = _case(mixers, r, B, T)
    _graph_replay_is_eager(m, batch, mask0, B, T)
