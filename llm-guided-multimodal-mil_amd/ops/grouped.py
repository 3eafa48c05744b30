"""Grouped products and the multi-token absorbed attention (csrc/linear_x.hip, skinny_gemm.h)."""
from __future__ import annotations

import torch

from .. import _lib
from ._base import _f32c, _p, _stream
from .linear import colsum, linear_act
from . import absorbed
from .absorbed import _AbsorbQuery, _ValueProj


def _gg(A, a_mode, B, b_mode, grp_off, G, max_rows, M, N, K, strideB, strideC, out, bias=None, stride_bias=0, residual=None,
        pad_rows: int = 0):
    nws = _lib.lib().mil_gemm_grouped_workspace_floats(a_mode, G, max_rows, M, N) if a_mode == 1 else 0
    ws = torch.empty(nws, device=A.device, dtype=torch.float32) if nws else None
    _lib.checked().mil_gemm_grouped_pad(_p(A), A.stride(0), a_mode, _p(B), B.stride(-2), b_mode, _p(out), out.stride(-2),
                                        _p(grp_off), G, max_rows, M, N, K, strideB, strideC, _p(bias), stride_bias,
                                        _p(residual), residual.stride(0) if residual is not None else 0, _p(ws), nws,
                                        int(pad_rows), _stream())
    return out


def _gg_nt(A, B, bias, grp_off, max_rows, zero: bool = False):
    """C[rows_g] = A[rows_g] . B[g]^T + bias[g];  A [R, K], B [G, N, K], bias [G, N] or None -> [R, N].
    zero: rows outside every group (the padding rows of a capacity bucket, segments.FusionBucket) must read 0, not
    whatever the allocation holds - the grouped kernels only write the rows of their groups."""
    G, N, K = B.shape
    out = torch.empty((A.shape[0], N), device=A.device, dtype=torch.float32)
    return _gg(A, 0, B, 0, grp_off, G, max_rows, 0, N, K, N * K, 0, out, bias, N if bias is not None else 0,
               pad_rows=A.shape[0] if zero else 0)


def _gg_nn(A, B, bias, residual, grp_off, max_rows, zero: bool = False):
    """C[rows_g] = A[rows_g] . B[g] + bias + residual;  A [R, K], B [G, K, N], bias [N] shared or None.  zero: as _gg_nt."""
    G, K, N = B.shape
    out = torch.empty((A.shape[0], N), device=A.device, dtype=torch.float32)
    return _gg(A, 0, B, 1, grp_off, G, max_rows, 0, N, K, K * N, 0, out, bias, 0, residual, pad_rows=A.shape[0] if zero else 0)


def _gg_tn(A, X, grp_off, G, max_rows):
    """C[g] = A[rows_g]^T . X[rows_g];  A [R, M], X [R, N] -> [G, M, N]."""
    M, N = A.shape[1], X.shape[1]
    out = torch.empty((G, M, N), device=A.device, dtype=torch.float32)
    return _gg(A, 1, X, 1, grp_off, G, max_rows, M, N, 0, 0, M * N, out)


def _gcs_ws(G, max_rows, ld, device):
    """Workspace of the row-parallel grouped column softmax (a few long groups), or None."""
    n = _lib.lib().mil_grp_col_softmax_workspace_floats(G, max_rows, ld)
    return torch.empty(n, device=device, dtype=torch.float32) if n else None


def _seg_colsum(Y, grp_off, G, max_rows):
    N = Y.shape[1]
    out = torch.empty((G, N), device=Y.device, dtype=torch.float32)
    nch = (max_rows + 255) // 256
    ws = torch.empty(nch * G * N, device=Y.device, dtype=torch.float32) if nch > 1 else None
    _lib.checked().mil_segment_colsum(_p(Y), _p(grp_off), G, max_rows, N, _p(out), _p(ws), _stream())
    return out


class _GroupedNT(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, B, bias, grp_off, max_rows: int):
        A, B = _f32c(A, "A"), _f32c(B, "B")
        ctx.save_for_backward(A, B, grp_off)
        ctx.max_rows, ctx.has_bias = max_rows, bias is not None
        return _gg_nt(A, B, _f32c(bias, "bias") if bias is not None else None, grp_off, max_rows)

    @staticmethod
    def backward(ctx, dC):
        A, B, grp_off = ctx.saved_tensors
        dC = _f32c(dC, "dC")
        G = B.shape[0]
        dA = _gg_nn(dC, B, None, None, grp_off, ctx.max_rows) if ctx.needs_input_grad[0] else None
        dB = _gg_tn(dC, A, grp_off, G, ctx.max_rows) if ctx.needs_input_grad[1] else None
        db = _seg_colsum(dC, grp_off, G, ctx.max_rows) if (ctx.has_bias and ctx.needs_input_grad[2]) else None
        return dA, dB, db, None, None


class _GroupedNN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, B, bias, residual, grp_off, max_rows: int):
        A, B = _f32c(A, "A"), _f32c(B, "B")
        ctx.save_for_backward(A, B, grp_off)
        ctx.max_rows, ctx.has_bias, ctx.has_res = max_rows, bias is not None, residual is not None
        return _gg_nn(A, B, _f32c(bias, "bias") if bias is not None else None,
                      _f32c(residual, "residual") if residual is not None else None, grp_off, max_rows)

    @staticmethod
    def backward(ctx, dC):
        A, B, grp_off = ctx.saved_tensors
        dC = _f32c(dC, "dC")
        G = B.shape[0]
        dA = _gg_nt(dC, B, None, grp_off, ctx.max_rows) if ctx.needs_input_grad[0] else None       # B[g] is [K, N] = [out, in]
        dB = _gg_tn(A, dC, grp_off, G, ctx.max_rows) if ctx.needs_input_grad[1] else None
        db = colsum(dC) if (ctx.has_bias and ctx.needs_input_grad[2]) else None
        return dA, dB, db, (dC if ctx.has_res else None), None, None


class _GroupedTN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, X, grp_off, G: int, max_rows: int):
        A, X = _f32c(A, "A"), _f32c(X, "X")
        ctx.save_for_backward(A, X, grp_off)
        ctx.max_rows = max_rows
        return _gg_tn(A, X, grp_off, G, max_rows)

    @staticmethod
    def backward(ctx, dC):
        A, X, grp_off = ctx.saved_tensors
        dC = _f32c(dC, "dC")
        dA = _gg_nt(X, dC, None, grp_off, ctx.max_rows) if ctx.needs_input_grad[0] else None        # dC[g] is [M, N] = [out, in]
        dX = _gg_nn(A, dC, None, None, grp_off, ctx.max_rows) if ctx.needs_input_grad[1] else None
        return dA, dX, None, None, None


class _GrpColSoftmax(torch.autograd.Function):
    """Softmax over the rows of each group, per column (columns >= TH are padding: zeros)."""

    @staticmethod
    def forward(ctx, S, grp_off, G: int, TH: int, max_rows: int = 0):
        """max_rows: length of the longest group (0 = unknown): picks the kernel shape that keeps a group in registers."""
        A = S if (S.is_contiguous() and S.dtype == torch.float32) else _f32c(S, "S").clone()
        if A is S:
            ctx.mark_dirty(S)              # in place: the scores are the fresh output of the product that formed them
        _lib.checked().mil_grp_col_softmax_ws(_p(A), A.stride(0), _p(grp_off), G, max_rows, TH,
                                              _p(_gcs_ws(G, max_rows, A.stride(0), A.device)), _stream())
        ctx.save_for_backward(A, grp_off)
        ctx.G, ctx.TH, ctx.max_rows = G, TH, max_rows
        return A

    @staticmethod
    def backward(ctx, dA):
        A, grp_off = ctx.saved_tensors
        dA = _f32c(dA, "dA")
        dS = torch.empty_like(A)
        _lib.checked().mil_grp_col_softmax_bwd_ws(_p(A), _p(dA), A.stride(0), _p(grp_off), ctx.G, ctx.max_rows, ctx.TH, _p(dS),
                                                  _p(_gcs_ws(ctx.G, ctx.max_rows, A.stride(0), A.device)), _stream())
        return dS, None, None, None, None


class _RowSoftmaxT(torch.autograd.Function):
    """Softmax over the T tokens of every (row, head); column t H + h."""

    @staticmethod
    def forward(ctx, S, T: int, H: int):
        A = S if (S.is_contiguous() and S.dtype == torch.float32) else _f32c(S, "S").clone()
        if A is S:
            ctx.mark_dirty(S)
        _lib.checked().mil_row_softmax_t(_p(A), A.stride(0), A.shape[0], T, H, _stream())
        ctx.save_for_backward(A)
        ctx.T, ctx.H = T, H
        return A

    @staticmethod
    def backward(ctx, dA):
        (A,) = ctx.saved_tensors
        dA = _f32c(dA, "dA")
        dS = torch.empty_like(A)
        _lib.checked().mil_row_softmax_t_bwd(_p(A), _p(dA), A.stride(0), A.shape[0], ctx.T, ctx.H, _p(dS), _stream())
        return dS, None, None


def multi_token_ok(E: int, H: int, t_lengths) -> bool:
    T = t_lengths[0] if len(t_lengths) else 0
    return E == 512 and H == 8 and 1 < T <= 12 and all(t == T for t in t_lengths)


class _MultiTokenPoolCore(torch.autograd.Function):
    """pooled[b] = softmax_rows(kin_b Qp_b^T)^T keys_b  - the three image-side stages of the multi-token token->image
    attention as ONE autograd node.  kin must be keys + (a constant): its gradient is folded into the keys' here, and the
    node also hands the keys back as an alias for their later consumers, so every contribution to d(keys) - values,
    scores, whatever arrives through the alias - is accumulated by the `residual` operand of the skinny products
    instead of [N, 512] elementwise adds of autograd (8 x 30 us per step at 32 bags x 1024 patches)."""

    @staticmethod
    def forward(ctx, keys, kin, Qp, segs, TH: int):
        keys_in = keys
        keys, kin, Qp = _f32c(keys, "keys"), _f32c(kin.detach(), "kin"), _f32c(Qp, "Qp")
        B, off, mr = segs.B, segs.k_off, segs.Tk_max
        z = getattr(segs, "device_lengths", False)                               # capacity bucket: padding rows read 0
        A = _gg_nt(kin, Qp, None, off, mr, zero=z)                               # scores [R, THp]
        _lib.checked().mil_grp_col_softmax_ws(_p(A), A.stride(0), _p(off), B, mr, TH, _p(_gcs_ws(B, mr, A.stride(0), A.device)),
                                              _stream())
        pooled = _gg_tn(A, keys, off, B, mr)                                     # [B, THp, E]
        ctx.segs, ctx.TH = segs, TH
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(keys, kin, Qp, A)
        if absorbed._site_tap is not None:             # model.note_attn: A holds the softmax weights, column t H + h
            absorbed._site_tap.append(dict(A=A, segs=segs, TH=TH))
        return pooled, keys_in.view_as(keys_in)

    @staticmethod
    def backward(ctx, dpooled, dkeys_pass):
        keys, kin, Qp, A = ctx.saved_tensors
        segs, TH = ctx.segs, ctx.TH
        B, off, mr = segs.B, segs.k_off, segs.Tk_max
        if dpooled is None:
            return dkeys_pass, None, None, None, None
        dpooled = _f32c(dpooled, "dpooled")
        acc = _f32c(dkeys_pass, "dkeys") if dkeys_pass is not None else None
        z = getattr(segs, "device_lengths", False)
        dA = _gg_nt(keys, dpooled, None, off, mr, zero=z)                        # dA = keys . dpooled^T
        dS = torch.zeros_like(A) if z else torch.empty_like(A)
        _lib.checked().mil_grp_col_softmax_bwd_ws(_p(A), _p(dA), A.stride(0), _p(off), B, mr, TH, _p(dS),
                                                  _p(_gcs_ws(B, mr, A.stride(0), A.device)), _stream())
        dkeys = None
        if ctx.needs_input_grad[0]:
            dkeys = _gg_nn(A, dpooled, None, acc, off, mr, zero=z)               # values path (+ what came through the alias)
            dkeys = _gg_nn(dS, Qp, None, dkeys, off, mr, zero=z)                 # + scores path (d kin = d keys)
        dQp = _gg_tn(dS, kin, off, B, mr) if ctx.needs_input_grad[2] else None
        return dkeys, None, dQp, None, None


class _MultiTokenRowsCore(torch.autograd.Function):
    """out = softmax_T(kin Kp_b^T + cb_b) Vp_b + bo + keys  - the image->token attention with absorbed projections and its
    residual as one node; kin = keys + (a constant), so d(keys) = dout + dS Kp comes out of one product launch."""

    @staticmethod
    def forward(ctx, keys, kin, Kp, cb, Vp, bo, segs, T: int, H: int):
        keys, kin = _f32c(keys, "keys"), _f32c(kin.detach(), "kin")
        Kp, cb, Vp, bo = _f32c(Kp, "Kp"), _f32c(cb, "cb"), _f32c(Vp, "Vp"), _f32c(bo, "bo")
        off, mr = segs.q_off, segs.Tq_max
        z = getattr(segs, "device_lengths", False)                               # capacity bucket: padding rows read 0
        A = _gg_nt(kin, Kp, cb, off, mr, zero=z)
        _lib.checked().mil_row_softmax_t(_p(A), A.stride(0), A.shape[0], T, H, _stream())
        out = _gg_nn(A, Vp, bo, keys, off, mr, zero=z)
        ctx.segs, ctx.T, ctx.H = segs, T, H
        ctx.save_for_backward(kin, Kp, Vp, A)
        return out

    @staticmethod
    def backward(ctx, dout):
        kin, Kp, Vp, A = ctx.saved_tensors
        segs, T, H = ctx.segs, ctx.T, ctx.H
        off, mr, B = segs.q_off, segs.Tq_max, segs.B
        dout = _f32c(dout, "dout")
        z = getattr(segs, "device_lengths", False)
        dA = _gg_nt(dout, Vp, None, off, mr, zero=z)                             # [R, THp]
        dS = torch.empty_like(A)
        _lib.checked().mil_row_softmax_t_bwd(_p(A), _p(dA), A.stride(0), A.shape[0], T, H, _p(dS), _stream())
        dkeys = _gg_nn(dS, Kp, None, dout, off, mr, zero=z) if ctx.needs_input_grad[0] else None      # residual + scores path
        dKp = _gg_tn(dS, kin, off, B, mr) if ctx.needs_input_grad[2] else None
        dcb = _seg_colsum(dS, off, B, mr) if ctx.needs_input_grad[3] else None
        dVp = _gg_tn(A, dout, off, B, mr) if ctx.needs_input_grad[4] else None
        dbo = colsum(dout) if ctx.needs_input_grad[5] else None
        return dkeys, None, dKp, dcb, dVp, dbo, None, None, None


def multi_token_pool_attention(q_tok, keys, kin, segs, Wq, bq, Wk, Wv, bv, H: int):
    """Token -> image attention for T text tokens per bag with the K / V projections absorbed
    (model/sam/transformer.py:291-295,113-118): the image side is three skinny grouped products around a column
    softmax instead of two [N, 512] x [512, 256] projections and an attention core.  segs: queries = tokens, keys = patches.
    kin must be keys + positional rows (a constant): its gradient is folded into the keys'.
    Returns (pre-out_proj output [B * T, H * C], keys alias - later consumers of the keys must use the alias)."""
    B, T = segs.B, segs.Tq_max
    TH = T * H
    C = Wq.shape[0] // H
    qp = linear_act(q_tok, Wq, bq)
    Qp = _AbsorbQuery.apply(qp, Wk, H, T, 1.0 / C ** 0.5)                        # k_proj.bias is softmax-invariant
    pooled, keys_pass = _MultiTokenPoolCore.apply(keys, kin, Qp, segs, TH)       # [B, THp, E]
    return _ValueProj.apply(pooled, Wv, bv, H, T), keys_pass


def multi_token_rows_attention(kin, k_tok, v_tok, segs, Wq, bq, Wk, bk, Wv, bv, Wo, bo, H: int, residual=None):
    """Image -> token attention (every patch over the T text tokens of its bag, sam/transformer.py:303-307) with the
    q and out projections absorbed into T x H key vectors Wq_h^T k_th (+ the scalar bq_h . k_th) and value vectors
    Wo_h v_th.  segs: queries = patches, keys = tokens.  Returns out_proj(attention) + residual, [R, E]."""
    B, T = segs.B, segs.Tk_max
    TH = T * H
    C = Wq.shape[0] // H
    scale = 1.0 / C ** 0.5
    kp = linear_act(k_tok, Wk, bk)                                                # [B * T, H * C]
    vp = linear_act(v_tok, Wv, bv)
    Kp, cb = _AbsorbQuery.apply(kp, Wq, H, T, scale, bq)                          # cb[b, t H + h] = scale * bq_h . k_th
    Vp = _AbsorbQuery.apply(vp, Wo.t().contiguous(), H, T, 1.0)                   # Vp[t, h] = Wo[:, hC:(h+1)C] v_th
    if residual is None:
        S = _GroupedNT.apply(kin, Kp, cb, segs.q_off, segs.Tq_max)
        return _GroupedNN.apply(_RowSoftmaxT.apply(S, T, H), Vp, bo, None, segs.q_off, segs.Tq_max)
    # with the keys as residual (the block form, sam/transformer.py:303-309) kin = keys + pe: one fused node
    return _MultiTokenRowsCore.apply(residual, kin, Kp, cb, Vp, bo, segs, T, H)
