"""Rows, packed-sequence and pool attention cores (csrc/attention.hip)."""
from __future__ import annotations

import torch

from .. import _lib
from ._base import _f32c, _p, _stream


def _head_dim(I: int, H: int) -> int:
    c = I // H
    if c * H != I or c not in (32, 64):
        raise _lib.MilHipError(f"attention: internal dim {I} / {H} heads = head dim {c}; kernels support 32 and 64")
    return c


SEQ_MAX_TOKENS = 96      # csrc/attention.hip: AS_MAXT


class _AttnRows(torch.autograd.Function):
    """softmax(q k^T / sqrt(c)) v, one thread per (query row, head): sam/transformer.py:441-446 for
    image->token / token self attention, clip/model.py:183 with causal=True."""

    @staticmethod
    def forward(ctx, q, k, v, segs, H: int, causal: bool):
        q, k, v = _f32c(q, "q"), _f32c(k, "k"), _f32c(v, "v")
        Tq, I = q.shape
        C = _head_dim(I, H)
        o = torch.empty_like(q)
        lse = torch.empty((Tq, H), device=q.device, dtype=torch.float32)
        if 16 < segs.Tk_max <= SEQ_MAX_TOKENS and segs.q_lengths == segs.k_lengths:
            # whole-sequence self-attention (CLIP text blocks): LDS-staged heads on MFMA, one workgroup per (sequence, head)
            _lib.checked().mil_attn_seq_fwd(_p(q), _p(k), _p(v), I, _p(segs.q_off), segs.B, segs.Tq_max, H, C,
                                            1 if causal else 0, _p(o), _p(lse), _stream())
        else:
            _lib.checked().mil_attn_rows_fwd(_p(q), _p(k), _p(v), _p(segs.q_off), _p(segs.k_off), _p(segs.q_bag), Tq, H, C,
                                             1 if causal else 0, _p(o), _p(lse), _stream())
        ctx.segs, ctx.H, ctx.C, ctx.causal = segs, H, C, causal
        ctx.save_for_backward(q, k, v, o, lse)
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse = ctx.saved_tensors
        segs, H, C = ctx.segs, ctx.H, ctx.C
        I = H * C
        do = _f32c(do, "do")
        if (not ctx.causal) and segs.Tk_max > 16 and (segs.q_lengths != segs.k_lengths or segs.Tk_max > SEQ_MAX_TOKENS):
            # more than 16 keys per bag outside whole-sequence self-attention (`--alignment_base CT`: 160 CT tokens as
            # queries / keys): the general per-(row, head) loops (include/mil_hip.h: mil_attn_rows_bwd_general)
            dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
            ws = torch.empty(max(1, q.shape[0]) * H, device=q.device, dtype=torch.float32)
            _lib.checked().mil_attn_rows_bwd_general(_p(q), _p(k), _p(v), _p(o), _p(do), _p(lse), _p(segs.q_off), _p(segs.k_off),
                                                     _p(segs.q_bag), _p(segs.k_bag), q.shape[0], k.shape[0], H, C, _p(dq),
                                                     _p(dk), _p(dv), _p(ws), _stream())
            return dq, dk, dv, None, None, None
        if ctx.causal or segs.Tk_max > 16:
            # whole-sequence self-attention (the CLIP text blocks under learnable prompts): q, k, v share the segments
            if segs.q_lengths != segs.k_lengths or segs.Tk_max > SEQ_MAX_TOKENS:
                raise _lib.MilHipError("attention backward: > 16 keys per bag is only supported for self-attention over "
                                       f"sequences of <= {SEQ_MAX_TOKENS} tokens")
            dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
            _lib.checked().mil_attn_seq_bwd(_p(q), _p(k), _p(v), I, _p(o), _p(do), _p(lse), _p(segs.q_off), segs.B,
                                            segs.Tq_max, H, C, 1 if ctx.causal else 0, _p(dq), _p(dk), _p(dv), I,
                                            _stream())
            return dq, dk, dv, None, None, None
        dq, dk, dv = torch.empty_like(q), torch.zeros_like(k), torch.zeros_like(v)
        ws = torch.empty(max(1, segs.nblk) * 2 * 16 * I, device=q.device, dtype=torch.float32)
        _lib.checked().mil_attn_rows_bwd(_p(q), _p(k), _p(v), _p(o), _p(do), _p(lse), _p(segs.k_off), _p(segs.blk_map),
                                         _p(segs.bag_blk_off), segs.nblk, segs.B, H, C, _p(dq), _p(dk), _p(dv), _p(ws),
                                         _stream())
        return dq, dk, dv, None, None, None


def attention_rows(q, k, v, segs, H: int, causal: bool = False):
    return _AttnRows.apply(q, k, v, segs, H, causal)


class _AttnSeqPacked(torch.autograd.Function):
    """Whole-sequence self-attention on the PACKED in_proj output qkv [rows, 3 W] (clip/model.py:171-178: one
    nn.MultiheadAttention in_proj of width 3 W): the kernels read q / k / v as column blocks (row stride 3 W) and the
    backward writes dq | dk | dv into one [rows, 3 W] tensor, so the projection and its backward are ONE GEMM each."""

    @staticmethod
    def forward(ctx, qkv, segs, H: int, causal: bool):
        qkv = _f32c(qkv, "qkv")
        rows, W3 = qkv.shape
        W = W3 // 3
        C = _head_dim(W, H)
        o = torch.empty((rows, W), device=qkv.device, dtype=torch.float32)
        lse = torch.empty((rows, H), device=qkv.device, dtype=torch.float32)
        base = qkv.data_ptr()
        _lib.checked().mil_attn_seq_fwd(base, base + 4 * W, base + 8 * W, W3, _p(segs.q_off), segs.B, segs.Tq_max, H, C,
                                        1 if causal else 0, _p(o), _p(lse), _stream())
        ctx.segs, ctx.H, ctx.C, ctx.causal = segs, H, C, causal
        ctx.save_for_backward(qkv, o, lse)
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, o, lse = ctx.saved_tensors
        segs, H, C = ctx.segs, ctx.H, ctx.C
        W3 = qkv.shape[1]
        W = W3 // 3
        do = _f32c(do, "do")
        dqkv = torch.empty_like(qkv)
        base, dbase = qkv.data_ptr(), dqkv.data_ptr()
        _lib.checked().mil_attn_seq_bwd(base, base + 4 * W, base + 8 * W, W3, _p(o), _p(do), _p(lse), _p(segs.q_off),
                                        segs.B, segs.Tq_max, H, C, 1 if ctx.causal else 0, dbase, dbase + 4 * W,
                                        dbase + 8 * W, W3, _stream())
        return dqkv, None, None, None


def seq_attention_ok(segs) -> bool:
    return 16 < segs.Tk_max <= SEQ_MAX_TOKENS and segs.q_lengths == segs.k_lengths


def attention_seq_packed(qkv, segs, H: int, causal: bool = False):
    return _AttnSeqPacked.apply(qkv, segs, H, causal)


class _AttnPool(torch.autograd.Function):
    """<= 16 queries per bag over many keys (token->image attention, sam/transformer.py:293,116)."""

    @staticmethod
    def forward(ctx, q, k, v, segs, H: int):
        q, k, v = _f32c(q, "q"), _f32c(k, "k"), _f32c(v, "v")
        Tq, I = q.shape
        C = _head_dim(I, H)
        if segs.Tq_max > 16:
            raise _lib.MilHipError("attention pool form supports <= 16 queries per bag")
        o = torch.empty_like(q)
        lse = torch.empty((Tq, H), device=q.device, dtype=torch.float32)
        ws = torch.empty(max(1, segs.ntiles) * 16 * (I + 2 * H), device=q.device, dtype=torch.float32)
        _lib.checked().mil_attn_pool_fwd_mh(_p(q), _p(k), _p(v), _p(segs.q_off), _p(segs.tile_map), _p(segs.bag_tile_off),
                                            segs.ntiles, segs.B, max(1, segs.Tq_max), H, C, _p(o), _p(lse), _p(ws), _stream())
        ctx.segs, ctx.H, ctx.C = segs, H, C
        ctx.save_for_backward(q, k, v, o, lse)
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse = ctx.saved_tensors
        segs, H, C = ctx.segs, ctx.H, ctx.C
        I = H * C
        do = _f32c(do, "do")
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        ws = torch.empty(max(1, segs.ntiles) * 16 * I, device=q.device, dtype=torch.float32)
        _lib.checked().mil_attn_pool_bwd_mh(_p(q), _p(k), _p(v), _p(o), _p(do), _p(lse), _p(segs.q_off), _p(segs.tile_map),
                                            _p(segs.bag_tile_off), segs.ntiles, segs.B, max(1, segs.Tq_max), H, C, _p(dq),
                                            _p(dk), _p(dv), _p(ws), _stream())
        return dq, dk, dv, None, None


def attention_pool(q, k, v, segs, H: int):
    if segs.Tq_max > 16:          # more queries per bag than the pool form holds: the rows form (general backward)
        return _AttnRows.apply(q, k, v, segs, H, False)
    return _AttnPool.apply(q, k, v, segs, H)
