"""Host-side operators over the C ABI (include/mil_hip.h).

Two layers:
  * plain functions, one per C entry point: torch tensors in, torch tensors out, all work
    enqueued on the current HIP stream, no host sync;
  * ``torch.autograd.Function`` wrappers (``gated_attention_pool``, ``head_sigmoid``) so the
    ``aggregator`` module composes with autograd/DDP exactly like the reference's
    ABMIL (model/dim1/ABMIL.py:47-64) and ``fc`` + sigmoid (model/aggregator.py:128-131,200).
"""
from .. import _lib
# one block per module, every name that resolves as ops.NAME
from ._base import (GATE_D, _p, _stream, _f32c, X_DROP_P, X_DROP_SCALE, M_DROP_P, M_DROP_SCALE, ACT, _stream_int, grad_slot,
                    _bf16c)
from .gate import (dropout_keep_bits, dropout_keep_bits_pair, counter_add, dropout_apply_bits, _DropoutBits, dropout_bits,
                   gate_scores_fwd, attn_pool_fwd, attn_pool_partial, attn_pool_partial_h, attn_pool_bwd_from_h,
                   pool_merge_head, head_bwd_params, head_fwd, bce_fwd_bwd, head_bwd, rowdot, attn_pool_bwd, gate_bwd_params,
                   gate_bwd_params_head, gate_bwd_input, adam_step, adam_step_counted, adam_step_counted_noinc,
                   adam_step_dev, adam_step_dev_segs, sgd_step, _GatedAttentionPool, gated_attention_pool,
                   gate_bwd_input_pool, _GatedPoolHeadLoss, gated_pool_head_loss, _HeadSigmoid, head_sigmoid, cast_bf16,
                   gate_scores_fwd_bf16, attn_pool_partial_bf16, attn_pool_partial_h_bf16, attn_pool_bwd_bf16,
                   gate_bwd_params_x16, gate_bwd_params_bf16, bag_softmax)
from .linear import (gemm, gemm_aux, linear_bwd_params, colsum, act_bwd, SMALL_ROWS, _small_ok, MID_ROWS, MID_WORK, _mid_ok,
                     linear_mid_fwd, linear_mid_bwd, linear_small_fwd, linear_small_bwd, _GradBox, _sum_overflow, _ONES,
                     backward, sum_n, _ok_extra, _FanOut, fan_out, _LinearAct, _small_dw, _LinLnLin, lin_ln_lin_ok,
                     lin_ln_lin, _MlpQuickGelu, mlp_quickgelu, linear_act, split_bf16, gemm_split, FrozenSplit,
                     _LinearFrozenSplit, _MlpQuickGeluFrozenSplit, linear_frozen_split, mlp_quickgelu_frozen_split)
from .attention import (_head_dim, SEQ_MAX_TOKENS, _AttnRows, attention_rows, _AttnSeqPacked, seq_attention_ok,
                        attention_seq_packed, _AttnPool, attention_pool)
from .tokens import (_tail_view, _LayerNorm, _layer_norm_bwd, _LayerNormRes, layer_norm_res, _LayerNormBagRow,
                     layer_norm_bag_row, layer_norm, _AppendRows, append_rows, _AddPE, add_pe, ct_map_tokens, sinusoid_pe,
                     embed_tokens, gather_eot, _AddBagRow, add_bag_row)
from .losses import (_ClipContrastive, clip_contrastive_loss, _CosineEmbedding, cosine_embedding_loss)
from .absorbed import (_AbsorbQuery, _dkeys_buffer, _AbsorbedPool, _ValueProj, _value_proj_bwd, _AbsorbedPoolValue,
                       _LnbrAbsorbedPoolValue, lnbr_one_token_ok, lnbr_one_token_attention, one_token_attention, note_sites,
                       absorbed_pool_attention)
from .grouped import (_gg, _gg_nt, _gg_nn, _gg_tn, _gcs_ws, _seg_colsum, _GroupedNT, _GroupedNN, _GroupedTN, _GrpColSoftmax,
                      _RowSoftmaxT, multi_token_ok, _MultiTokenPoolCore, _MultiTokenRowsCore, multi_token_pool_attention,
                      multi_token_rows_attention)
from .transmil import (TM_H, TM_DH, TM_D, TM_M, TM_CONV, TM_PINV_ITERS, TM_QSCALE, _tm_splits, tm_deterministic, tm_pieces, tm_batch_bags, _tm_pieces_route, tm_bgemm, tm_softmax_rows,
                       tm_softmax_rows_bwd, _TmRowGather, tm_row_gather, tm_seq_index, TM_SEG_MAX, TM_SEG_STRIDE, tm_seq_index_segs, tm_seq_index_bucket, _TmPPEG, tm_ppeg,
                       tm_cls_attention, tm_cls_attention_fused, tm_lmk_attn, tm_lmk_attn_bwd, tm_tok_attn, tm_tok_attn_bwd, _tm_fused_a3,
                       _tm_fused_a1, _tm_fused_cls, _tm_pinv_fwd, _tm_fwd, _tm_fwd_bags, _tm_pinv_bwd, _tm_bwd, _tm_bwd_bags, _NystromCore, nystrom_core,
                       _NystromCoreBags, nystrom_core_bags, tm_packed, TmPackedTable, tm_packed_table_host, tm_packed_table,
                       _tm_fwd_packed, _tm_bwd_packed, _NystromCorePacked, nystrom_core_packed, tm_packed_ppeg, TmPpegTable,
                       tm_ppeg_table_host, tm_ppeg_table, _TmPPEGPacked, tm_ppeg_packed, tm_packed_cls, TmClsTable,
                       tm_cls_table_host, tm_cls_table, tm_cls_attention_packed, TmRoute, tm_route)
from .metrics import (EVAL_TILE, EVAL_MAX_ROWS, EVAL_MAX_TERMS, EVAL_LOSS_SLOTS, EVAL_FLAG_OVERFLOW, EVAL_FLAG_NAN, EVAL_OUT_WORDS,
                      eval_out_bytes, eval_push, eval_rank, eval_reduce)
