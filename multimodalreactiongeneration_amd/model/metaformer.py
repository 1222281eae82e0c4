"""Multi-modal metaformer (reference: mr_gen/model/utils/multi_modal_metaformer.py).

Module tree, constructor arguments and state_dict names follow the reference
(MultiModalEmbedding / IntegrateModalBlock / MultiModalMetaformerBlock /
MultiModalMetaformer).  ``MultiModalMetaformer.forward`` has one MI355X-
specific schedule: in the first block the per-modality LSTM encoders advance
layer by layer and every group of same-shape layers runs as ONE persistent
recurrence launch (main + audio + partner at layer 0, audio + partner above),
which is legal because the reference's recurrent state is never carried
 and the encoders are independent until the integrator.
"""
from __future__ import annotations

import os
from typing import Any, List, Tuple

import torch
from torch import nn

from .. import functional as Fn
from . import forms
from .layers import Linear, FeedForward, ResidualConnection
from .masks import BlockCausalMask, gen_attention_mask  # noqa: F401  (re-export, reference location)
from .mixers import MixerLayerdFactory, LSTMMixerBlock, split_state


def check_form_modal_num(modal_num: int, sameone, msg: str = None) -> list:
    if not isinstance(sameone, (list, tuple)):
        raise TypeError(f"must be list or tuple. but got {type(sameone)}")
    if modal_num != len(sameone):
        if len(sameone) != 1:
            raise ValueError("" if msg is None else msg)
        sameone = list(sameone) * modal_num
    return sameone



# the fused integrator also serves the T = 1 frames of autoregressive generation (one launch per
# batched projection / LayerNorm instead of per-integrator modules, no mask or concat glue);
# MRG_FUSED_T1=0 keeps those frames on the per-module path
_FUSED_MIN_T = 1 if os.environ.get("MRG_FUSED_T1", "1") == "1" else 2

class MultiModalEmbedding(nn.Module):
    def __init__(self, modal_num: int, mixer_configs):
        super().__init__()
        self.modal_num = modal_num
        self.mixer_configs = check_form_modal_num(modal_num, mixer_configs,
                                                  "modal_num must be equal to the length of mixer_configs.")
        factory = MixerLayerdFactory()
        self.modal_embeddings = nn.ModuleList([factory.build(*c) for c in self.mixer_configs])

    def forward(self, x, hx=None, other=None):
        x = check_form_modal_num(self.modal_num, x, "The length of x must be equal to modal_num.")
        hx = [None] * self.modal_num if hx is None else hx
        other = [(None,)] * self.modal_num if other is None else other
        ys, states = [], []
        for i, emb in enumerate(self.modal_embeddings):
            out = emb(x[i], hx[i], other[i])
            ys.append(out[0])
            states.append(out[1])
        return (ys, states)


class IntegrateModalBlock(nn.Module):
    """Cross-attend the main modality to each other modality, concat, cat_linear (:128-217)."""

    def __init__(self, modal_num: int, mixer_configs, output_dim: int):
        super().__init__()
        self.modal_num = modal_num
        self.mixer_configs = check_form_modal_num(modal_num - 1, mixer_configs,
                                                  "modal_num must be equal to the length + 1 of mixer_configs.")
        factory = MixerLayerdFactory()
        self.integrators = nn.ModuleList()
        width = 0
        for kind, cfg in self.mixer_configs:
            if kind != "mha":
                raise TypeError("IntegrateModalBlock only supports mha mixer.")
            self.integrators.append(factory.build(kind, cfg))
            width += cfg["output_projection_size"] if cfg.get("output_projection") else cfg["hidden_size"]
        self.cat_linear = Linear(width, output_dim)

    def check_form_input(self, other_modals, attn_mask, hx=None):
        other_modals = [other_modals] if isinstance(other_modals, torch.Tensor) else other_modals
        other_modals = check_form_modal_num(self.modal_num - 1, other_modals,
                                            "The length of other_modals must be equal to modal_num - 1.")
        attn_mask = [None] * (self.modal_num - 1) if attn_mask is None else attn_mask
        attn_mask = [attn_mask] if not isinstance(attn_mask, (list, tuple)) else attn_mask
        attn_mask = check_form_modal_num(self.modal_num - 1, attn_mask,
                                         "The length of attn_mask must be equal to modal_num - 1.")
        hx = [None] * (self.modal_num - 1) if hx is None else hx
        return other_modals, attn_mask, hx

    # ---- MI355X schedule: every integrator + the concat + cat_linear as one fused op (integrate.py)
    use_fused = os.environ.get("MRG_FUSED_INTEGRATOR", "1") == "1"

    def _fused(self, main_modal, other_modals, attn_mask, hxs):
        """integrate.integrate(...) when the block is inside its form (forms.integrator_form) and the
        call is one the fused op takes (fused_args), else None."""
        from ..integrate import integrate
        args = self.fused_args(main_modal, other_modals, attn_mask, hxs)
        if args is None:
            return None
        return integrate(main_modal, list(other_modals), args.qpads, args.kpads, args.params, args.cat_w,
                         args.cat_b, args.heads, args.causal, args.eps)

    def fused_args(self, main_modal, other_modals, attn_mask, hxs):
        """forms.FusedIntegratorArgs of the fused form (integrate.py), or None when the block is outside
        it (forms.integrator_form) or this call is: the switch off, a carried state, inputs that are not
        [B, T >= _FUSED_MIN_T, E] / [B, Tk, E] device tensors, an attention dropout that would drop, a
        mask that is not block-causal, or masks on some integrators only."""
        if not (self.use_fused and isinstance(main_modal, torch.Tensor) and main_modal.is_cuda
                and main_modal.dim() == 3 and main_modal.shape[1] >= _FUSED_MIN_T and all(h is None for h in hxs)):
            return None
        form = forms.integrator_form(self)
        B, T, E = main_modal.shape
        if form is None or form.cat_w.shape[0] != E:
            return None
        masks = []
        for mha, kv, m in zip(form.attentions, other_modals, attn_mask):
            if mha.dropout and mha.training:
                return None
            if not (isinstance(kv, torch.Tensor) and kv.dim() == 3 and kv.shape[0] == B and kv.shape[2] == E
                    and kv.is_cuda):
                return None
            if m is not None and not isinstance(m, BlockCausalMask):
                return None
            masks.append(m)
        causal = masks[0] is not None
        if len(masks) != len(form.integrators) or any((m is not None) != causal for m in masks):
            return None
        qpads = [m.main_pad if causal else None for m in masks]
        kpads = [m.other_pad if causal else None for m in masks]
        return forms.FusedIntegratorArgs(form.integrators, form.cat_w, form.cat_b, form.heads, causal, form.eps,
                                         qpads, kpads)

    def forward(self, main_modal, other_modals, attn_mask=None, hxs=None):
        other_modals, attn_mask, hxs = self.check_form_input(other_modals, attn_mask, hxs)
        out = self._fused(main_modal, other_modals, attn_mask, hxs)
        if out is not None:
            return (out, [None] * (self.modal_num - 1))
        ys, states = [], []
        for i, integ in enumerate(self.integrators):
            y, st, _ = integ(main_modal, hxs[i], other_modals[i], other_modals[i], attn_mask[i])
            ys.append(y)
            states.append(st)
        return (self.cat_linear(torch.cat(ys, dim=-1)), states)


class MultiModalMetaformerBlock(nn.Module):
    """embedding -> integrator -> FeedForward (:220-338)."""

    def __init__(self, num_modal: int, main_modal_embedding_config, integrate_configs, feedforward_configs: dict,
                 encode_other_modal: bool = False, other_modal_embedding_config=None):
        super().__init__()
        if not encode_other_modal or other_modal_embedding_config is None:
            other_modal_embedding_config = []
        if isinstance(main_modal_embedding_config, tuple):
            main_modal_embedding_config = [main_modal_embedding_config]
        if encode_other_modal:
            other_modal_embedding_config = check_form_modal_num(
                num_modal - 1, other_modal_embedding_config,
                "The length of other_modal_embedding_config must be equal to num_modal - 1.")
        integrate_configs = check_form_modal_num(num_modal - 1, integrate_configs,
                                                 "The length of integrate_configs must be equal to num_modal - 1.")
        self.num_modal = num_modal
        self.emb_num_modal = num_modal if encode_other_modal else 1
        self.encode_other_modal = encode_other_modal
        self.embedding_configs = list(main_modal_embedding_config) + list(other_modal_embedding_config)
        self.emb_mixer_type = [c[0] for c in self.embedding_configs]
        self.embedding = MultiModalEmbedding(self.emb_num_modal, self.embedding_configs)
        self.integrator = IntegrateModalBlock(num_modal, integrate_configs, feedforward_configs["hidden_size"])
        self.feedforward = FeedForward(**feedforward_configs)

    def forward(self, main_modal, other_modals=None, hx=None, prev_hx=None, main_modal_others=None,
                other_modals_others=None, integrate_attn_mask=None):
        if isinstance(main_modal, tuple):
            (main_modal, other_modals, hx, prev_hx, main_modal_others, other_modals_others,
             integrate_attn_mask) = main_modal
        first, hx, prev_hx = split_state(hx, prev_hx)
        if first is None:
            first = {"emb": None, "crm": None}
        other_modals_others = other_modals_others if other_modals_others else [None]
        other_modals_others = check_form_modal_num(self.num_modal - 1, other_modals_others,
                                                   "The length of other_modals_others must be equal to num_modal - 1.")
        mods = [main_modal] + (list(other_modals) if self.encode_other_modal else [])
        others = [main_modal_others] + list(other_modals_others)
        mods, emb_states = self.embedding(mods, first["emb"], others)
        main_modal = mods[0]
        if self.encode_other_modal:
            other_modals = mods[1:]
        main_modal, crm = self.integrator(main_modal, other_modals, integrate_attn_mask, first["crm"])
        prev_hx.append({"emb": emb_states, "crm": crm})
        main_modal = self.feedforward(main_modal)
        return (main_modal, other_modals, hx, prev_hx, main_modal_others, other_modals_others,
                integrate_attn_mask)


def _lstm_block_tail(block: LSTMMixerBlock, y, x):
    """Residual LN of the LSTM output, then the block's FeedForward."""
    y = block.mixer.combine(y, x)
    return block.feed_forward(y)


class MultiModalMetaformer(nn.Module):
    """Feature projections, metaformer blocks, output FFN (:341-509)."""

    def __init__(self, modal_num: int, hidden_dim: int, num_layer: int, main_modal_feature_dim,
                 main_mixer_type, main_mixer_configs, integrate_mixer_configs, feedforward_configs: dict,
                 output_feedforward_configs: dict, other_modal_feature_dim=None, other_mixer_type="mha",
                 other_mixer_configs=None, repeat_with_encoder: bool = False,
                 interlayer_residual: bool = False, interlayer_residual_norm: bool = True):
        super().__init__()
        if isinstance(main_modal_feature_dim, (list, tuple)):
            main_modal_feature_dim = main_modal_feature_dim[0]
        if isinstance(main_mixer_type, (list, tuple)):
            main_mixer_type = main_mixer_type[0]
        if isinstance(main_mixer_configs, (list, tuple)):
            main_mixer_configs = main_mixer_configs[0]
        main_cfgs = [(main_mixer_type, main_mixer_configs)]
        if isinstance(integrate_mixer_configs, dict):
            integrate_mixer_configs = [integrate_mixer_configs]
        integrate_mixer_configs = check_form_modal_num(modal_num - 1, integrate_mixer_configs,
                                                       "The length of integrate_mixer_configs must be equal to modal_num - 1.")
        integ_cfgs = [("mha", c) for c in integrate_mixer_configs]
        if isinstance(other_modal_feature_dim, int):
            other_modal_feature_dim = [other_modal_feature_dim]
        other_modal_feature_dim = check_form_modal_num(modal_num - 1, other_modal_feature_dim,
                                                       "The length of other_modal_feature_dim must be equal to modal_num - 1.")
        if isinstance(other_mixer_type, str):
            other_mixer_type = [other_mixer_type]
        other_mixer_type = check_form_modal_num(modal_num - 1, other_mixer_type,
                                                "The length of other_mixer_type must be equal to modal_num - 1.")
        if isinstance(other_mixer_configs, dict):
            other_mixer_configs = [other_mixer_configs]
        other_mixer_configs = check_form_modal_num(modal_num - 1, other_mixer_configs,
                                                   "The length of other_mixer_configs must be equal to modal_num - 1.")
        other_cfgs = [(other_mixer_type[i], other_mixer_configs[i]) for i in range(modal_num - 1)]
        self.modal_num, self.hidden_dim, self.num_layer = modal_num, hidden_dim, num_layer
        self.repeat_with_encoder, self.interlayer_residual = repeat_with_encoder, interlayer_residual
        self.embedding_mixer_type = [main_mixer_type] + list(other_mixer_type)
        self.feature_embedding = nn.ModuleList(
            [Linear(d, hidden_dim) for d in [main_modal_feature_dim] + list(other_modal_feature_dim)])
        blocks = [MultiModalMetaformerBlock(modal_num, main_cfgs, integ_cfgs, feedforward_configs,
                                            encode_other_modal=True, other_modal_embedding_config=other_cfgs)]
        for _ in range(num_layer - 1):
            blocks.append(MultiModalMetaformerBlock(modal_num, main_cfgs, integ_cfgs, feedforward_configs,
                                                    encode_other_modal=repeat_with_encoder,
                                                    other_modal_embedding_config=other_cfgs if repeat_with_encoder else None))
        self.metaformer_blocks = nn.ModuleList(
            [ResidualConnection(b, interlayer_residual_norm, hidden_dim) if interlayer_residual else b
             for b in blocks])
        self.output_feedforward = FeedForward(**output_feedforward_configs)
        if self._module_path_only():
            for b in blocks:   # every fused schedule declines such a model, the integrator's too
                b.integrator.use_fused = False

    # ---- MI355X schedule for a block's embedding (batched recurrences)
    def _fast_first_embedding(self, block: MultiModalMetaformerBlock, mods: List[torch.Tensor]):
        """Only reached after _fast_eligible, which established forms.residual_lstm for every mixer
        block below: no structural check is repeated here."""
        chains = [[(m.feed_forward, *forms.residual_lstm_form(m)) for m in l.mixer]
                  for l in block.embedding.modal_embeddings]
        xs = list(mods)
        depth = max(len(c) for c in chains)
        for layer in range(depth):
            active = [i for i, c in enumerate(chains) if layer < len(c)]
            groups = {}
            for i in active:
                groups.setdefault((tuple(xs[i].shape), chains[i][layer][1].w_hh.shape[1]), []).append(i)
            for idxs in groups.values():
                # at most two recurrences per launch: two batch-tile-2 problems fill the chip's
                # 512 resident workgroups; three would need batch tiles of 4 (longer GEMV per step)
                for start in range(0, len(idxs), 2):
                    part = idxs[start:start + 2]
                    # LN(LSTM(x) + x) fused per problem, then each block's FeedForward (fused too)
                    us = Fn.lstm_layers_batched([(xs[i], *chains[i][layer][1], chains[i][layer][2]) for i in part])
                    for i, u in zip(part, us):
                        xs[i] = chains[i][layer][0](u)
        return xs

    # ---- MI355X schedule: block 0's embedding stacks as one layer-wavefront (encoder_stack.py: one
    # recurrence launch and batched GEMM / LayerNorm launches per (layer, time chunk) diagonal); on by
    # default (measured 27.6 -> 26.0 ms/step), MRG_ENCODER_STACK=0 keeps the per-layer schedule
    use_encoder_stack = os.environ.get("MRG_ENCODER_STACK", "1") == "1"

    def _stack_layers(self, block: MultiModalMetaformerBlock):
        """forms.embedding_stack_form: per modality the forms.LstmBlocks of the block's LSTM stacks and
        their LayerNorm eps, or None outside the encoder stack's form."""
        return forms.embedding_stack_form(block)

    def _stack_first_block(self, block, feats):
        """Block 0's embeddings (feature Linear + every LSTM block of every modality) as one wavefront, or
        None when outside it (the per-layer schedule below then runs)."""
        from ..encoder_stack import encoder_stack, stack_eligible
        if not (self.use_encoder_stack and block.encode_other_modal and len(feats) == self.modal_num):
            return None
        got = self._stack_layers(block)
        if got is None:
            return None
        layers, eps = got
        H = self.hidden_dim
        if not (stack_eligible(H, feats[0].shape[0]) and all(f.dim() == 3 and f.is_cuda and f.shape[1] >= 8
                                                             and f.shape[0] == feats[0].shape[0] for f in feats)):
            return None
        if any(f.requires_grad for f in feats):   # the stack returns no feature gradient (features are data)
            return None
        embs = list(self.feature_embedding)
        if any(e.bias is None for e in embs):
            return None
        return encoder_stack([(f, e.weight, e.bias, l) for f, e, l in zip(feats, embs, layers)], eps)

    def _module_path_only(self) -> bool:
        """True when the model holds what only the module path runs: an MLP mixer, a swish / tanh
        activation (FeedForward or mixer), or an attention with an output nonlinearity (Q7).  The
        module tree is fixed after construction, so the scan runs once."""
        got = self.__dict__.get("_module_path_only_cached")
        if got is None:
            from .layers import MHAforSequentail
            from .mixers import MLPMixer
            got = any(isinstance(m, (MLPMixer, nn.SiLU, nn.Tanh))
                      or (isinstance(m, MHAforSequentail) and m.nonlinearity is not None)
                      for m in self.modules())
            self.__dict__["_module_path_only_cached"] = got
        return got

    def _fast_eligible(self) -> bool:
        """Every embedding of every block is an LSTM layerd without projections whose blocks are
        LN(LSTM(x) + x) over one unidirectional layer (forms.residual_lstm), and nothing in the
        model is module-path-only."""
        if self.interlayer_residual or self._module_path_only():
            return False
        for block in self.metaformer_blocks:
            for lay in block.embedding.modal_embeddings:
                chain = forms.lstm_chain(lay)
                if chain is None or any(forms.residual_lstm(m) is None for m in chain):
                    return False
        return True

    def forward(self, main_modal, other_modals, hx=None, main_modal_others=None, other_modals_others=None,
                integrate_attn_mask=None):
        """Returns (main, other_modals, per-block state record) like the reference (:476-509).

        The record the reference returns holds only None leaves (states are never
        produced), and feeding it back is stateless; both are mirrored.
        """
        fast = _none_leaves(hx) and _none_leaves(main_modal_others) and _none_leaves(other_modals_others) \
            and self._fast_eligible()
        stacked = self._stack_first_block(self.metaformer_blocks[0], [main_modal] + list(other_modals)) \
            if fast else None
        if stacked is None:
            main_modal = self.feature_embedding[0](main_modal)
            other_modals = [self.feature_embedding[i + 1](o) for i, o in enumerate(other_modals)]
        if fast:
            record = []
            for bi, block in enumerate(self.metaformer_blocks):
                mods = [main_modal] + (list(other_modals) if block.encode_other_modal else [])
                enc = stacked if (bi == 0 and stacked is not None) else self._fast_first_embedding(block, mods)
                main_modal = enc[0]
                if block.encode_other_modal:
                    other_modals = enc[1:]
                main_modal, _ = block.integrator(main_modal, other_modals, integrate_attn_mask, None)
                main_modal = block.feedforward(main_modal)
                record.append({"emb": [None] * block.emb_num_modal, "crm": [None] * (self.modal_num - 1)})
            return self.output_feedforward(main_modal), other_modals, record
        args = [other_modals, hx, None, main_modal_others, other_modals_others, integrate_attn_mask]
        for block in self.metaformer_blocks:
            main_modal, *args = block(main_modal, *args)
        main_modal = self.output_feedforward(main_modal)
        return main_modal, args[0], args[2]


def _none_leaves(x) -> bool:
    if x is None:
        return True
    if isinstance(x, dict):
        return all(_none_leaves(v) for v in x.values())
    if isinstance(x, (list, tuple)):
        return all(_none_leaves(v) for v in x)
    return False
