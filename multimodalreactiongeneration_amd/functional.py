"""Autograd functions of the MI355X path; every FLOP runs in libmrg.so (include/mrg.h).

torch is used for device memory (caching allocator), the current HIP stream
and the autograd graph only.  Parameter gradients are written straight into
``param.grad`` by the fused backward GEMMs (beta = 1 accumulation; the
functions return ``None`` for parameters), so a step needs no per-parameter
gradient copies and a flat gradient buffer (optim.FusedAdamW, ddp.GradReducer)
sees them in place.

Reference ops replaced (file:line in /root/reference):
  linear / FFN        nn.Linear + ReLU            mixer_block.py:37-87, lstm_block.py:88-96
  lstm                nn.LSTM (cuDNN RNN)         mixer_block.py:237-252, lstm_block.py:21-46,
                                                  lstm_sampler.py:16-34
  mha                 nn.MultiheadAttention       for_sequential.py:27-51, multi_modal_att.py:12-31
  residual_layernorm  ResidualConnection          residual_connection.py:20-37
  residual_add        ... without LayerNorm       residual_connection.py:29-37
  masked_loss         training_step / lossfun     lstmformer.py:313-325,372-380

This module only re-exports.  The code lives, in import order, in launch (plumbing), gemm_ops (GEMM
dispatch), then dense, recurrent, dropout, attention and losses; a switch that is rebound, not mutated
(dense.RELU_TAP, gemm_ops.wgrad_splits), must be set on the module that owns it.
"""
from .attention import (MHASpec, _MHAFn, _MHAOneKeyFn, _one_key, attn_bwd, attn_fwd, mha, mha_residual,  # noqa: F401
                        mha_residual_layernorm, visible_pairs)
from .dense import (ACTIVATIONS, RELU_TAP, _ActFn, _FFNFn, _FFNResFn, _FFNResLNFn, _LinAddFn, _LinearFn,  # noqa: F401
                    _LinResFn, _LinResLNFn, _MLPChainFn, _ResAddFn, _ResLNFn, _Sample0Fn, _act_codes,
                    _act_fwd_gemm, _resln_bwd, _resln_fwd, _tap_relu, activation, broadcast_sample0, ffn,
                    ffn_residual, ffn_residual_layernorm, linear, linear_add, linear_residual,
                    linear_residual_layernorm, mlp_chain, residual_add, residual_layernorm)
from .dropout import (_DropoutFn, _RNG, _drop_consts, _i64, _rng_device, _rng_draw, _rng_state,  # noqa: F401
                      attention_keep_mask, dropout, dropout_keep_mask, get_rng_state, manual_seed, set_rng_state)
from .gemm_ops import (_CNT, _PL_ON, _PLANES, _WG_TARGET, _WT_CACHE, _WT_MIN_ROWS, _WT_ON, _WT_PENDING,  # noqa: F401
                       _counters, _dx_gemm, _fwd_gemm, _on_side, _plane_operand, _planes_gemm, _wgrad, _wt,
                       _wt_key, _wt_note, act_splits, colsum, gemm, invalidate_weight_planes, planes_batched,
                       prepare_weight_planes, set_dx_transposed, set_weight_planes, wgrad_splits)
from .launch import (_ARITH, _CALLS, _ERR, _GRAD_LISTENER, _NATIVE, _PROBE_CAP, _PROBE_ON, _PROBES,  # noqa: F401
                     _TOUCHED, PRECISIONS, _err_flag, _flush_touched, _gbuf, _keeps_precision, _probe, _ptr,
                     _stream, _ws, check_errors, precision, probe_start, probe_stop, set_grad_listener, zero_,
                     zeros)
from .losses import (_LOSS_TYPES, _BcastLossFn, _LossFn, _flat_f32, _metric_buffers, _metric_ranges,  # noqa: F401
                     broadcast_masked_loss, clip_grad_norm_, clip_grad_value_, clip_grad_workspace, masked_loss,
                     padding_flags, target_metrics_update, target_metrics_update_broadcast, zero_padding)
from .recurrent import (_GRU_PERSIST, _GRUFn, _LSTMCellFn, _LSTMFn, gru_layer, gru_residual,  # noqa: F401
                        lstm_bidirectional_layer, lstm_bidirectional_layers, lstm_bidirectional_residual,
                        lstm_layer, lstm_layers_batched, lstm_residual, lstm_residual_layernorm)
from .wgrad_streams import (_LAST_FORK, _SIDE_MIN_ROWS, _conflicts, _fork, _writes, allow_defer,  # noqa: F401
                            beside_recurrence, hold_scratch, on_side, reset_fork_point, set_wgrad_defer,
                            set_wgrad_stream, side as _side)
