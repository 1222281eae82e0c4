"""The fused schedules' forms: named parameter groups and the recognisers of a module tree.

A fused schedule (encoder_stack.py, integrate.py, generate.py, decode.py) takes the weights of a
module subtree of one fixed shape.  The groups below name those weights; their field order is the
flattened order of the ``Function.apply`` calls and of the pointer tables in ``include/mrg.h``
(``mrg_gen_loop``, ``mrg_ssd_loop_fwd`` / ``_bwd``), so it must not move.  They are tuples:
``*group``, ``list(group)`` and ``Group._make(flat[i:j])`` all work.

A recogniser is a function of a module.  It returns the group(s) when the subtree has the form and
None otherwise, and it reads structure only: module types, counts, flags set at construction and
parameter shapes.  What can change between calls (the input tensors, their device and shape, masks,
carried state, ``training`` with a dropout, the selected arithmetic, the ``use_*`` switches) is
checked where the schedule is called, never here.  Nothing is cached on the modules.
"""
from __future__ import annotations

from typing import Any, List, NamedTuple, Optional, Tuple

from torch import nn

from .layers import LSTM, LSTMBlock as _LSTMBlockModule, LSTMLayerd, LSTMModule, ResidualConnection
from .mixers import GRUMixerBlock, GRUMixerLayerd, LSTMMixerBlock, LSTMMixerLayerd


# ------------------------------------------------------------------ named parameter groups
class LstmLn(NamedTuple):
    """LN(LSTM(x) + x), one unidirectional layer: a layer of the scheduled-sampling decode."""
    w_ih: Any
    w_hh: Any
    b_ih: Any
    b_hh: Any
    ln_w: Any
    ln_b: Any


class LstmBlock(NamedTuple):
    """u = LN1(LSTM(x) + x), LN2(u ff_w^T + ff_b + u): an LSTM mixer block of the encoder stack."""
    w_ih: Any
    w_hh: Any
    b_ih: Any
    b_hh: Any
    ln1_w: Any
    ln1_b: Any
    ff_w: Any
    ff_b: Any
    ln2_w: Any
    ln2_b: Any


class GruBlock(NamedTuple):
    """u = LN1(GRU(x) + x), LN2(u ff_w^T + ff_b + u): a GRU mixer block of the generation plan (w_ih /
    w_hh [3H, H], b_ih / b_hh [3H], torch.nn.GRU's gate order r, z, n)."""
    w_ih: Any
    w_hh: Any
    b_ih: Any
    b_hh: Any
    ln1_w: Any
    ln1_b: Any
    ff_w: Any
    ff_b: Any
    ln2_w: Any
    ln2_b: Any


class Integrator(NamedTuple):
    """u = LN1(MHA(q, kv) + q), LN2(u ff_w^T + ff_b + u): one cross-attention mixer of the integrator.
    in_w [3E, E] / in_b [3E] are nn.MultiheadAttention's packed projections (query rows, then key and
    value rows)."""
    in_w: Any
    in_b: Any
    out_w: Any
    out_b: Any
    ln1_w: Any
    ln1_b: Any
    ff_w: Any
    ff_b: Any
    ln2_w: Any
    ln2_b: Any

    @property
    def q_w(self):
        return self.in_w[:self.in_w.shape[1]]

    @property
    def kv_w(self):
        return self.in_w[self.in_w.shape[1]:]

    @property
    def q_b(self):
        return self.in_b[:self.in_w.shape[1]]

    @property
    def kv_b(self):
        return self.in_b[self.in_w.shape[1]:]


class ReluFfn(NamedTuple):
    """Linear -> ReLU -> Linear; ln is the residual LayerNorm module around it, or None."""
    w1: Any
    b1: Any
    w2: Any
    b2: Any
    ln: Any


class IntegratorForm(NamedTuple):
    """The structural half of the fused integrator (integrate.py): what the module tree fixes.
    attentions: the integrators' MultiheadAttention modules, whose dropout / training the caller reads."""
    integrators: List[Integrator]
    cat_w: Any
    cat_b: Any
    heads: int
    eps: float
    attentions: list


class FusedIntegratorArgs(NamedTuple):
    """IntegratorForm plus what one call adds (mask kind and padding flags): integrate()'s arguments."""
    params: List[Integrator]
    cat_w: Any
    cat_b: Any
    heads: int
    causal: bool
    eps: float
    qpads: list
    kpads: list


# ------------------------------------------------------------------ recognisers
def one_layer_unidirectional(rnn) -> bool:
    """The fused recurrences take layer 0's forward parameters only: a stacked or bidirectional LSTM
    (with its inter-layer dropout) runs through layers.LSTM."""
    return rnn.num_layers == 1 and not rnn.bidirectional


def _linear_residual_ln(feed_forward):
    """(Linear, LayerNorm) of a FeedForward that is LN(Linear(x) + x) with a bias, or None."""
    ff = getattr(feed_forward, "feed_forward", None)
    if not isinstance(ff, ResidualConnection) or ff.layer_norm is None:
        return None
    mods = list(ff.module.children())
    if len(mods) != 1 or not isinstance(mods[0], nn.Linear) or mods[0].bias is None:
        return None
    return mods[0], ff.layer_norm


def residual_lstm(mixer_block):
    """(LSTM, LayerNorm) of an LSTMMixerBlock whose mixer is LN(LSTM(x) + x) over one unidirectional
    layer, or None.  No FeedForward requirement: what the per-layer batched schedule needs."""
    if not isinstance(mixer_block, LSTMMixerBlock):
        return None
    res = mixer_block.mixer
    if not isinstance(res, ResidualConnection):
        return None
    ln, lstm = res.layer_norm, res.module.mixer
    if ln is None or not one_layer_unidirectional(lstm):
        return None
    return lstm, ln


def residual_lstm_form(mixer_block) -> Optional[Tuple[LstmLn, float]]:
    """(LstmLn, eps) of a residual_lstm block, or None."""
    got = residual_lstm(mixer_block)
    if got is None:
        return None
    lstm, ln = got
    return LstmLn(*lstm.direction_params(0), ln.weight, ln.bias), ln.eps


def lstm_block_form(mixer_block) -> Optional[Tuple[LstmBlock, float, float]]:
    """(LstmBlock, eps1, eps2) of a residual_lstm_form block that keeps its width (H -> H) and whose
    FeedForward is one Linear with a residual LayerNorm, or None."""
    got = residual_lstm_form(mixer_block)
    tail = _linear_residual_ln(mixer_block.feed_forward) if got is not None else None
    if tail is None:
        return None
    lay, eps1 = got
    if lay.w_ih.shape[1] != lay.w_hh.shape[1]:
        return None
    lin, ln2 = tail
    return LstmBlock(*lay, lin.weight, lin.bias, ln2.weight, ln2.bias), eps1, ln2.eps


def lstm_chain(layerd) -> Optional[list]:
    """The mixer blocks of an LSTMMixerLayerd without input / output projection, or None."""
    if not (isinstance(layerd, LSTMMixerLayerd) and layerd.input_projection is None
            and layerd.output_projection is None):
        return None
    return list(layerd.mixer)


def embedding_stack_form(metaformer_block) -> Optional[Tuple[List[List[LstmBlock]], float]]:
    """Per modality the LstmBlocks of the block's embedding stacks and their one LayerNorm eps, or
    None when a stack is outside the encoder stack's form."""
    out, eps = [], set()
    for layerd in metaformer_block.embedding.modal_embeddings:
        chain = lstm_chain(layerd)
        if chain is None:
            return None
        layers = []
        for mb in chain:
            got = lstm_block_form(mb)
            if got is None:
                return None
            layers.append(got[0])
            eps.update(got[1:])
        out.append(layers)
    if len(eps) != 1:
        return None
    return out, eps.pop()


def residual_gru(mixer_block):
    """(GRU, LayerNorm) of a GRUMixerBlock whose mixer is LN(GRU(x) + x) over one unidirectional layer,
    or None."""
    if not isinstance(mixer_block, GRUMixerBlock):
        return None
    res = mixer_block.mixer
    if not isinstance(res, ResidualConnection):
        return None
    ln, gru = res.layer_norm, res.module.mixer
    if ln is None or not one_layer_unidirectional(gru):
        return None
    return gru, ln


def gru_block_form(mixer_block) -> Optional[Tuple[GruBlock, float, float]]:
    """(GruBlock, eps1, eps2) of a residual_gru block that keeps its width (H -> H) and whose FeedForward
    is one Linear with a residual LayerNorm, or None."""
    got = residual_gru(mixer_block)
    tail = _linear_residual_ln(mixer_block.feed_forward) if got is not None else None
    if tail is None:
        return None
    gru, ln1 = got
    w_ih, w_hh, b_ih, b_hh = gru.direction_params(0)
    if w_ih.shape[1] != w_hh.shape[1]:
        return None
    lin, ln2 = tail
    return GruBlock(w_ih, w_hh, b_ih, b_hh, ln1.weight, ln1.bias, lin.weight, lin.bias, ln2.weight,
                    ln2.bias), ln1.eps, ln2.eps


def gru_chain(layerd) -> Optional[list]:
    """The mixer blocks of a GRUMixerLayerd without input / output projection, or None."""
    if not (isinstance(layerd, GRUMixerLayerd) and layerd.input_projection is None
            and layerd.output_projection is None):
        return None
    return list(layerd.mixer)


def embedding_mixer_form(metaformer_block) -> Optional[Tuple[List[Tuple[str, list]], float]]:
    """Per modality ("lstm", [LstmBlock]) or ("gru", [GruBlock]) of the block's embedding stacks and
    their one LayerNorm eps, or None when a stack is neither chain or a block is outside its form.
    What the generation plan takes (generate.py); the training schedules keep embedding_stack_form."""
    out, eps = [], set()
    for layerd in metaformer_block.embedding.modal_embeddings:
        for kind, chain, block_form in (("lstm", lstm_chain(layerd), lstm_block_form),
                                        ("gru", gru_chain(layerd), gru_block_form)):
            if chain is not None:
                break
        else:
            return None
        layers = []
        for mb in chain:
            got = block_form(mb)
            if got is None:
                return None
            layers.append(got[0])
            eps.update(got[1:])
        out.append((kind, layers))
    if len(eps) != 1:
        return None
    return out, eps.pop()


def integrator_form(integrate_modal_block) -> Optional[IntegratorForm]:
    """IntegratorForm of an IntegrateModalBlock whose integrators are single-block cross-attention
    layerds (no projections, one batch_first MHA without output nonlinearity or extra keys (bias_k, add_zero_attn), residual LN,
    one-Linear residual-LN FeedForward) of cat_linear's width, with one head count and one eps."""
    blk = integrate_modal_block
    n = len(blk.integrators)
    cw = blk.cat_linear.weight
    E = cw.shape[0]
    if blk.cat_linear.bias is None or cw.shape[1] != n * E:
        return None
    params, heads, eps, attentions = [], set(), set(), []
    for integ in blk.integrators:
        if (integ.input_projection is not None or integ.output_projection is not None or integ.self_attention
                or len(integ.mixer) != 1):
            return None
        res = integ.mixer[0].mixer
        if not (isinstance(res, ResidualConnection) and res.layer_norm is not None and len(res.module.mixer) == 1):
            return None
        if res.module.mixer[0].nonlinearity is not None:   # Q7: the module path mirrors it
            return None
        mha = res.module.mixer[0].mha
        if (not mha.batch_first or mha.in_proj_bias is None or tuple(mha.in_proj_weight.shape) != (3 * E, E)
                or mha.out_proj.bias is None or getattr(mha, "bias_k", None) is not None
                or getattr(mha, "add_zero_attn", False)):
            return None
        if getattr(mha, "record_weights", None) is not None:   # a recording attention runs as a module (its
            return None                                        # weights are kept there); read on every call

        tail = _linear_residual_ln(integ.mixer[0].feed_forward)
        if tail is None:
            return None
        lin, ln2 = tail
        heads.add(mha.num_heads)
        eps.update((res.layer_norm.eps, ln2.eps))
        attentions.append(mha)
        params.append(Integrator(mha.in_proj_weight, mha.in_proj_bias, mha.out_proj.weight, mha.out_proj.bias,
                                 res.layer_norm.weight, res.layer_norm.bias, lin.weight, lin.bias,
                                 ln2.weight, ln2.bias))
    if len(heads) != 1 or len(eps) != 1 or E % next(iter(heads)) != 0:
        return None
    return IntegratorForm(params, cw, blk.cat_linear.bias, heads.pop(), eps.pop(), attentions)


def _relu_ffn(seq, ln) -> Optional[ReluFfn]:
    mods = list(seq.children())
    if len(mods) != 3 or not isinstance(mods[1], nn.ReLU):
        return None
    if not all(isinstance(m, nn.Linear) and m.bias is not None for m in (mods[0], mods[2])):
        return None
    return ReluFfn(mods[0].weight, mods[0].bias, mods[2].weight, mods[2].bias, ln)


def relu_ffn_form(feedforward, residual: bool) -> Optional[ReluFfn]:
    """ReluFfn of a FeedForward that is Linear -> ReLU -> Linear (both with a bias); with ``residual``
    it must sit in a residual LayerNorm (ReluFfn.ln), without it must not."""
    seq = getattr(feedforward, "feed_forward", None)
    ln = None
    if residual:
        if not isinstance(seq, ResidualConnection) or seq.layer_norm is None:
            return None
        ln, seq = seq.layer_norm, seq.module
    if not isinstance(seq, nn.Sequential):
        return None
    return _relu_ffn(seq, ln)


# the decode kernels' widths (decode.hip): hidden, FFN bottleneck, output features, LayerNorm eps
_DECODE_MAX_H, _DECODE_MAX_HB, _DECODE_MAX_FO, _DECODE_EPS = 256, 64, 8, 1e-5


def decode_form(lstm_with_sample) -> Optional[Tuple[List[LstmLn], Tuple, float]]:
    """([LstmLn], (w1, b1, w2, b2), eps) of an LSTMwithSample inside the fused scheduled-sampling
    decode (decode.py), or None: every layered block is a residual LN around a 1-layer unidirectional
    LSTM of the feature projection's width H without mixing or feed-forward, the output FFN is
    Linear -> ReLU -> Linear, and 4 <= H <= 256, H % 4 == 0, bottleneck <= 64, outputs <= 8, eps 1e-5."""
    m = lstm_with_sample
    stack, seq, proj = (getattr(m, k, None) for k in ("layerd_lstm", "feed_forward", "feature_projection"))
    if not (isinstance(stack, LSTMLayerd) and isinstance(seq, nn.Sequential) and isinstance(proj, nn.Linear)):
        return None
    H = proj.weight.shape[0]
    layers = []
    for blk in stack.lstm_layered:
        if not isinstance(blk, _LSTMBlockModule) or blk.use_feed_forward:
            return None
        rc = blk.lstm_module
        if not isinstance(rc, ResidualConnection) or rc.layer_norm is None or not isinstance(rc.module, LSTMModule):
            return None
        lstm = rc.module.lstm_module
        if rc.module.mixer is not None or not isinstance(lstm, LSTM) or not one_layer_unidirectional(lstm):
            return None
        ln = rc.layer_norm
        if ln.weight.shape[0] != H or ln.eps != _DECODE_EPS:
            return None
        layers.append(LstmLn(*lstm.direction_params(0), ln.weight, ln.bias))
    ffn = _relu_ffn(seq, None)
    if ffn is None or not layers:
        return None
    if not (4 <= H <= _DECODE_MAX_H and H % 4 == 0 and ffn.w1.shape[0] <= _DECODE_MAX_HB
            and ffn.w2.shape[0] <= _DECODE_MAX_FO):
        return None
    return layers, tuple(ffn[:4]), _DECODE_EPS
