"""TransMIL: Nystrom attention, PPEG and the sequence assembly (csrc/transmil.hip)."""
from __future__ import annotations

import ctypes
import dataclasses
import functools
import itertools
import math
import os
from types import SimpleNamespace
from typing import Optional

import torch

from .. import _lib
from ._base import _f32c, _p, _stream


# Nystrom attention of one bag (nystrom_attention: 8 heads x 64, 256 landmarks, 6 pseudo-inverse iterations, 33-tap residual
# conv on v) on the [n_pad, 1536] to_qkv rows of its front-zero-padded LayerNorm output; PPEG; the row gather of the
# sequence assembly.  Every product runs on mil_tm_bgemm, reading per-head operands in place out of the merged rows; with
# pieces=3 (MIL_TM_PIECES=3) the products that _tm_pieces_route names run on mil_tm_bgemm_pieces (split-bf16 MFMA) instead.
TM_H, TM_DH, TM_D, TM_M, TM_CONV, TM_PINV_ITERS = 8, 64, 512, 256, 33, 6
TM_QSCALE = TM_DH ** -0.5


def _tm_splits(M: int, N: int, batch: int, K: int) -> int:
    tiles = -(-M // 64) * -(-N // 64) * batch
    if tiles >= 256 or K < 512:
        return 1
    return max(1, min(K // 256, 512 // tiles))


def _tm_env(value, name: str) -> bool:
    """A switch of this file: the value where it is not None (a keyword, or the module attribute a caller passes), else the
    environment variable `name`, read per call; unset, "" and "0" are off."""
    if value is None:
        value = os.environ.get(name, "0") not in ("", "0")
    return bool(value)


def tm_deterministic(value=None) -> bool:       # TransMIL.deterministic: the fixed-order sums (the mil_tm_*_fixed entries)
    return _tm_env(value, "MIL_TM_DETERMINISTIC")


def tm_batch_bags(value=None) -> bool:          # TransMIL.batch_bags: the batched landmark-side chain (nystrom_core_bags)
    return _tm_env(value, "MIL_TM_BATCH_BAGS")


def tm_packed(value=None) -> bool:              # TransMIL.packed: the packed sequence (nystrom_core_packed)
    return _tm_env(value, "MIL_TM_PACKED")


def tm_packed_ppeg(value=None) -> bool:         # TransMIL.packed_ppeg: on the packed route, PPEG as one launch set (tm_ppeg_packed)
    return _tm_env(value, "MIL_TM_PACKED_PPEG")


def tm_packed_cls(value=None) -> bool:          # TransMIL.packed_cls: need_attn="cls" on the packed route (tm_cls_attention_packed)
    return _tm_env(value, "MIL_TM_PACKED_CLS")


def _tm_fused_a3(value, need_attn) -> bool:     # the landmark-query pass on its fused entries (tm_lmk_attn); the attention
    return _tm_env(value, "MIL_TM_FUSED_A3") and need_attn is False     # outputs are formed from the maps: need_attn False only


def _tm_fused_a1(value, need_attn) -> bool:     # the token-query pass on its fused entries (tm_tok_attn): the same
    return _tm_env(value, "MIL_TM_FUSED_A1") and need_attn is False


def _tm_fused_cls(value, need_attn) -> bool:    # TransMIL.fused_cls: need_attn "cls" from the fused passes' operands, both then fused
    return _tm_env(value, "MIL_TM_FUSED_CLS") and isinstance(need_attn, str) and need_attn == "cls"


def tm_pieces(value=None) -> int:
    """The split-bf16 products: TransMIL.gemm_pieces, else MIL_TM_PIECES (default 0), read per call.  0: every product on fp32
    MFMA; 3: those that _tm_pieces_route names on three-piece split-bf16 MFMA (mil_tm_bgemm_pieces); else ValueError."""
    if value is None:
        value = os.environ.get("MIL_TM_PIECES", "") or "0"
    try:
        pieces = int(value)
    except (TypeError, ValueError):
        pieces = -1
    if isinstance(value, bool) or pieces not in (0, 3):
        raise ValueError(f"TransMIL gemm pieces must be 0 or 3, got {value!r}")
    return pieces


@dataclasses.dataclass(frozen=True)
class TmRoute:
    """What one TransMIL step launches, as tm_route resolves it: how the bags run ("each", "batched", "packed"), PPEG as one
    launch set, either attention pass on its fused entries, where the per-patch cls attention comes from (None, "maps" =
    tm_cls_attention on A1 / A3, "fused", "packed"), the fixed-order sums and the split-bf16 products (0 or 3)."""
    bags: str
    ppeg_packed: bool
    fused_a1: bool
    fused_a3: bool
    cls: Optional[str]
    det: bool
    pieces: int

    def key(self) -> tuple:
        """The route's part of a graph key.  A fused switch is named only where it changes the route's launches: none on the
        packed route, which runs both passes fused whatever they say, nor a1 / a3 under the fused cls attention."""
        alone = self.bags != "packed" and self.cls != "fused"
        return ((("deterministic",) if self.det else ()) + ((("gemm_pieces", self.pieces),) if self.pieces else ())
                + (("fused_a1",) if alone and self.fused_a1 else ()) + (("fused_a3",) if alone and self.fused_a3 else ())
                + (("fused_cls",) if self.cls == "fused" else ())
                + ((("packed",) + (("ppeg",) if self.ppeg_packed else ()) + (("cls",) if self.cls == "packed" else ()))
                   if self.bags == "packed" else ("batch_bags",) if self.bags == "batched" else ()))


def tm_route(switches, n_bags: int, need_attn) -> TmRoute:
    """The route of a step of `n_bags` bags that asks for need_attn (False, True or "cls").  switches: a TransMIL module, or
    anything with its seven attributes deterministic, gemm_pieces, batch_bags, packed, packed_ppeg, packed_cls, fused_cls; each
    overrides its environment variable when it is not None.  The two fused passes have environment switches only
    (MIL_TM_FUSED_A1, MIL_TM_FUSED_A3).  This is the one statement of the precedence:
      packed   more than one bag, packed on, and need_attn False - or "cls" with packed_cls on.  Both passes run fused whatever
               their switches say; PPEG is one launch set too with packed_ppeg on (it has no effect on another route); the cls
               attention is formed on the packed rows.
      batched  otherwise, with more than one bag, need_attn False and batch_bags on.
      each     otherwise: bag by bag.  need_attn True always lands here, with both maps materialised.  "cls" with fused_cls on
               takes the cls attention from the fused passes' operands and runs both passes fused; off, from the maps.
      On each and batched fused_a1 / fused_a3 apply with need_attn False only; deterministic and gemm_pieces go with every route."""
    want_cls = isinstance(need_attn, str) and need_attn == "cls"
    if n_bags > 1 and tm_packed(switches.packed) and (need_attn is False or (want_cls and tm_packed_cls(switches.packed_cls))):
        bags, fused_a1, fused_a3, cls = "packed", True, True, "packed" if want_cls else None
    else:
        bags = "batched" if n_bags > 1 and need_attn is False and tm_batch_bags(switches.batch_bags) else "each"
        fused_cls = _tm_fused_cls(switches.fused_cls, need_attn)
        fused_a1, fused_a3 = fused_cls or _tm_fused_a1(None, need_attn), fused_cls or _tm_fused_a3(None, need_attn)
        cls = ("fused" if fused_cls else "maps") if want_cls else None
    return TmRoute(bags, bags == "packed" and tm_packed_ppeg(switches.packed_ppeg), fused_a1, fused_a3, cls,
                   tm_deterministic(switches.deterministic), tm_pieces(switches.gemm_pieces))


def _tm_pieces_route(M: int, N: int, K: int) -> bool:
    """Which products take mil_tm_bgemm_pieces when pieces == 3: those with K >= 256 - the pseudo-inverse chain and its
    backward (256^3), W, U, O, dU, dW, dq, dk, dv, dqL, dkL, and the whole-map products of need_attn True.  The K = 64
    products (A1, A2, A3, dA1, dA3, dZ) stay on mil_tm_bgemm: those that write a bag-sized map are bound by their output,
    not by the matrix pipe, and two 32-deep slices do not pay for the split."""
    return K >= 256


def _ws(nfloats: int, like):
    """A fixed-order entry's workspace: one torch.empty (inside a capture it comes from the graph's pool)."""
    return torch.empty(int(nfloats), device=like.device, dtype=torch.float32)


def tm_bgemm(A, sA, B, sB, C, sC, batch: int, M: int, N: int, K: int, alpha: float = 1.0, beta: float = 0.0,
             diag: float = 0.0, D=None, split: bool = True, deterministic: bool = False, pieces: int = 0):
    """C[b] = alpha A[b] B[b] + beta D[b] (D = C if None) + diag I over general strides (sA = (batch, row, k) etc., in floats);
    A, B, C, D are tensors or views whose data_ptr is element (0, 0) of batch 0 (mil_tm_bgemm).
    deterministic (a bool, resolved by the caller): the same split count, but the splits meet in a workspace and are added in
    ascending order (mil_tm_bgemm_fixed), and C is not zeroed for beta == 0.
    pieces (0 or 3, resolved by the caller): 3 puts the product on the split-bf16 entries (mil_tm_bgemm_pieces, _fixed) when
    _tm_pieces_route takes its shape; the split count and what deterministic means are the same on either arithmetic."""
    if pieces not in (0, 3):
        raise ValueError(f"tm_bgemm: pieces must be 0 or 3, got {pieces!r}")
    splits = _tm_splits(M, N, batch, K) if (split and D is None and diag == 0.0 and beta in (0.0, 1.0)) else 1
    pw = (pieces,) if pieces and _tm_pieces_route(M, N, K) else ()          # the extra argument of the split-bf16 entries
    if deterministic and splits > 1:
        ws = _ws(_lib.lib().mil_tm_bgemm_ws_floats(batch, M, N, splits), C)
        entry = _lib.checked().mil_tm_bgemm_pieces_fixed if pw else _lib.checked().mil_tm_bgemm_fixed
        entry(_p(A), *sA, _p(B), *sB, _p(C), *sC, _p(D), batch, M, N, K, float(alpha), float(beta), float(diag), splits, *pw,
              _p(ws), _stream())
        return C
    if splits > 1 and beta == 0.0:
        C.zero_()
        beta = 1.0
    if pw:
        _lib.checked().mil_tm_bgemm_pieces(_p(A), *sA, _p(B), *sB, _p(C), *sC, _p(D), batch, M, N, K, float(alpha), float(beta),
                                           float(diag), splits, *pw, _stream())
        return C
    _lib.checked().mil_tm_bgemm(_p(A), *sA, _p(B), *sB, _p(C), *sC, _p(D), batch, M, N, K, float(alpha), float(beta),
                                float(diag), splits, _stream())
    return C


def tm_softmax_rows(x):
    _lib.checked().mil_tm_softmax_rows(_p(x), x.numel() // x.shape[-1], x.shape[-1], _stream())
    return x


def tm_softmax_rows_bwd(p, dp):
    _lib.checked().mil_tm_softmax_rows_bwd(_p(p), _p(dp), p.numel() // p.shape[-1], p.shape[-1], _stream())
    return dp


class _TmRowGather(torch.autograd.Function):
    """dst[r] = src[idx[r]] (idx >= 0) / extra (idx == -2) / 0 (idx == -1); repeated rows add their gradients."""

    @staticmethod
    def forward(ctx, src, extra, idx, deterministic=False):
        src = _f32c(src, "src")
        E = src.shape[1]
        dst = torch.empty((idx.numel(), E), device=src.device, dtype=torch.float32)
        ex = _f32c(extra, "extra").reshape(-1) if extra is not None else None
        _lib.checked().mil_tm_row_gather(_p(src), _p(ex), _p(idx), idx.numel(), E, _p(dst), _stream())
        ctx.save_for_backward(idx)
        ctx.src_rows, ctx.has_extra = src.shape[0], extra is not None
        ctx.extra_shape = extra.shape if extra is not None else None
        ctx.deterministic = deterministic
        return dst

    @staticmethod
    def backward(ctx, ddst):
        (idx,) = ctx.saved_tensors
        ddst = _f32c(ddst, "ddst")
        E = ddst.shape[1]
        if ctx.deterministic:       # every row of dsrc and dextra is written: nothing to zero
            dsrc = torch.empty((ctx.src_rows, E), device=ddst.device, dtype=torch.float32)
            dex = torch.empty(E, device=ddst.device, dtype=torch.float32) if ctx.has_extra else None
            ws = _ws(_lib.lib().mil_tm_row_gather_ws_floats(ctx.src_rows), ddst)
            _lib.checked().mil_tm_row_gather_bwd_fixed(_p(ddst), _p(idx), idx.numel(), E, _p(dsrc), ctx.src_rows, _p(dex), _p(ws),
                                                       _stream())
            return dsrc, (dex.reshape(ctx.extra_shape) if dex is not None else None), None, None
        dsrc = torch.zeros((ctx.src_rows, E), device=ddst.device, dtype=torch.float32)
        dex = torch.zeros(E, device=ddst.device, dtype=torch.float32) if ctx.has_extra else None
        _lib.checked().mil_tm_row_gather_bwd(_p(ddst), _p(idx), idx.numel(), E, _p(dsrc), _p(dex), _stream())
        return dsrc, (dex.reshape(ctx.extra_shape) if dex is not None else None), None, None


def tm_row_gather(src, extra, idx, deterministic=None):
    """idx: device int32 [rows] (model/dim1/TransMIL.py builds it per bag on the host).  deterministic: the backward adds
    repeated rows in ascending row order instead of atomically (mil_tm_row_gather_bwd_fixed); None reads MIL_TM_DETERMINISTIC."""
    return _TmRowGather.apply(src, extra, idx, tm_deterministic(deterministic))


def tm_seq_index(len_dev, sides, idx_out, rows_dev=None, flag=None, x_tail=None):
    """idx_out (device int32, at least sum(1 + s^2) entries) <- tm_row_gather's index of the sequence assembly, from the bag
    lengths on the device (len_dev int32 [B]) and the bags' grid sides (host ints: the launch shape); rows_dev [1] <- the
    sum of the lengths; flag [1] <- 1 if a length lies outside its side's bucket (it is clamped, nothing is written out of
    range); x_tail [rows >= sum(s^2), L]: its rows behind the bags are zeroed.  One launch (two with x_tail), no host sync."""
    sides = [int(s) for s in sides]
    arr = (ctypes.c_int32 * len(sides))(*sides)
    if x_tail is not None and (x_tail.dtype != torch.float32 or not x_tail.is_contiguous()):
        raise _lib.MilHipError("tm_seq_index: x_tail must be a contiguous float32 tensor")
    _lib.checked().mil_tm_seq_index(_p(len_dev), len(sides), arr, _p(idx_out), idx_out.numel(), _p(rows_dev), _p(flag),
                                    _p(x_tail), x_tail.shape[0] if x_tail is not None else 0,
                                    x_tail.shape[1] if x_tail is not None else 0, _stream())
    return idx_out


TM_SEG_MAX = 4                      # segments per bag of a tm_seq_index_segs table (csrc/transmil.hip)
TM_SEG_STRIDE = 1 + 2 * TM_SEG_MAX  # int32 per bag: s, then (first row, length) per segment


def tm_seq_index_segs(table, total: int, x_rows: int, idx_out=None, flag=None):
    """tm_row_gather's index for bags whose rows lie in up to four pieces of the source (mil_tm_seq_index_segs): table, device
    int32 [B, TM_SEG_STRIDE] = per bag (s, first0, len0, .. first3, len3) with the segments in sequence order
    (model/dim1/TransMIL.py: segment_table builds it), total = sum(1 + s^2) (host int: the launch shape), x_rows = rows of the
    source.  Per bag [-2 | the segments' rows | the first s^2 - L of them again]; nothing leaves [0, x_rows); flag [1]
    (optional) <- 1 if a bag's rows do not fit its side.  One launch, no host sync.  Returns idx_out[:total]."""
    if table.dtype != torch.int32 or table.dim() != 2 or table.shape[1] != TM_SEG_STRIDE or not table.is_contiguous():
        raise _lib.MilHipError(f"tm_seq_index_segs: table must be contiguous int32 [B, {TM_SEG_STRIDE}], got "
                               f"{table.dtype} {tuple(table.shape)}")
    total = int(total)
    if idx_out is None:
        idx_out = torch.empty(total, device=table.device, dtype=torch.int32)
    if idx_out.dtype != torch.int32 or not idx_out.is_contiguous() or idx_out.device != table.device:
        raise _lib.MilHipError("tm_seq_index_segs: idx_out must be a contiguous int32 tensor on the table's device")
    if flag is not None and (flag.dtype != torch.int32 or flag.numel() < 1):
        raise _lib.MilHipError("tm_seq_index_segs: flag must be int32 [1]")
    _lib.checked().mil_tm_seq_index_segs(_p(table), table.shape[0], total, int(x_rows), _p(idx_out), idx_out.numel(), _p(flag),
                                         _stream())
    return idx_out[:total]


def tm_seq_index_bucket(len_dev, cap: int, tail, sides, idx_out, L_dev=None, flag=None):
    """tm_row_gather's index for the fusion model's capacity bucket (mil_tm_seq_index_bucket), from the bag lengths on the
    device: len_dev int32 [B]; cap patch rows in front of the source, then B x tail[j] rows per tail segment (host ints, at most
    TM_SEG_MAX); sides: the bags' grid sides (host ints: the launch shape).  Per bag [-2 | its tail segments | its patches | the
    first s^2 - L of those again]; nothing leaves [0, cap + B sum(tail)).  L_dev [B] (optional) <- len[b] + sum(tail); flag [1]
    (optional) <- 1 if a bag does not fit its side or the lengths exceed cap.  One launch, no host sync.  Returns
    idx_out[:sum(1 + s^2)]."""
    sides, tail = [int(s) for s in sides], [int(t) for t in tail]
    total = sum(1 + s * s for s in sides)
    if len_dev.dtype != torch.int32 or len_dev.numel() != len(sides) or not len_dev.is_contiguous():
        raise _lib.MilHipError(f"tm_seq_index_bucket: len_dev must be contiguous int32 [{len(sides)}]")
    if idx_out.dtype != torch.int32 or not idx_out.is_contiguous() or idx_out.device != len_dev.device or idx_out.numel() < total:
        raise _lib.MilHipError(f"tm_seq_index_bucket: idx_out must be a contiguous int32 tensor of >= {total} entries on len_dev's device")
    if L_dev is not None and (L_dev.dtype != torch.int32 or L_dev.numel() < len(sides)):
        raise _lib.MilHipError(f"tm_seq_index_bucket: L_dev must be int32 [{len(sides)}]")
    if flag is not None and (flag.dtype != torch.int32 or flag.numel() < 1):
        raise _lib.MilHipError("tm_seq_index_bucket: flag must be int32 [1]")
    _lib.checked().mil_tm_seq_index_bucket(_p(len_dev), len(sides), int(cap), (ctypes.c_int32 * len(tail))(*tail), len(tail),
                                           (ctypes.c_int32 * len(sides))(*sides), _p(idx_out), idx_out.numel(), _p(L_dev),
                                           _p(flag), _stream())
    return idx_out[:total]


class _TmPPEG(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, s: int, W7, b7, W5, b5, W3, b3, deterministic=False):
        x = _f32c(x, "x")
        W7, W5, W3 = _f32c(W7, "W7"), _f32c(W5, "W5"), _f32c(W3, "W3")
        y = torch.empty_like(x)
        _lib.checked().mil_tm_ppeg_fwd(_p(x), s, _p(W7), _p(_f32c(b7, "b7")), _p(W5), _p(_f32c(b5, "b5")), _p(W3),
                                       _p(_f32c(b3, "b3")), _p(y), _stream())
        ctx.save_for_backward(x, W7, W5, W3)
        ctx.s, ctx.deterministic = s, deterministic
        return y

    @staticmethod
    def backward(ctx, dy):
        x, W7, W5, W3 = ctx.saved_tensors
        dy = _f32c(dy, "dy")
        dx = torch.empty_like(x)
        if ctx.deterministic:       # the fold overwrites dWf and db
            dWf = torch.empty((TM_D, 1, 7, 7), device=x.device, dtype=torch.float32)
            db = torch.empty(TM_D, device=x.device, dtype=torch.float32)
            ws = _ws(_lib.lib().mil_tm_ppeg_ws_floats(ctx.s), x)
            _lib.checked().mil_tm_ppeg_bwd_fixed(_p(dy), _p(x), ctx.s, _p(W7), _p(W5), _p(W3), _p(dx), _p(dWf), _p(db), _p(ws),
                                                 _stream())
        else:
            dWf = torch.zeros((TM_D, 1, 7, 7), device=x.device, dtype=torch.float32)
            db = torch.zeros(TM_D, device=x.device, dtype=torch.float32)
            _lib.checked().mil_tm_ppeg_bwd(_p(dy), _p(x), ctx.s, _p(W7), _p(W5), _p(W3), _p(dx), _p(dWf), _p(db), _stream())
        # one 7 x 7 correlation map: dW7 is all of it, dW5 / dW3 its central 5 x 5 / 3 x 3; the three biases share db
        return (dx, None, dWf, db, dWf[:, :, 1:6, 1:6].contiguous(), db.clone(), dWf[:, :, 2:5, 2:5].contiguous(), db.clone(), None)


def tm_ppeg(x, s: int, W7, b7, W5, b5, W3, b3, deterministic=None):
    """PPEG (TransMIL.py:32-47) on one bag's [1 + s^2, 512] rows: cls passed through, the s x s grid through the folded
    depthwise 7 x 7.  deterministic: the weight and bias gradients from per-chunk partials added in ascending order
    (mil_tm_ppeg_bwd_fixed); None reads MIL_TM_DETERMINISTIC."""
    return _TmPPEG.apply(x, s, W7, b7, W5, b5, W3, b3, tm_deterministic(deterministic))


def tm_cls_attention(A1, Z, A3, pad: int, s: int, n=None, len_dev=None, bag: int = 0):
    """Per-patch attention of the cls token out of the Nystrom factors, without the [8, n_pad, n_pad] map (mil_tm_cls_attn):
    A1 [8, n_pad, 256] and A3 [8, 256, n_pad] softmaxed, Z [8, 256, 256] as _tm_fwd holds them, pad = n_pad - s^2 - 1 the cls
    row.  With P = A1 Z A3: out[h, i] = P[h, pad, pad + 1 + i] + (i < s^2 - N ? P[h, pad, pad + 1 + N + i] : 0) for i < N - a
    patch the square padding repeats gets the sum of its two keys - and 0 for N <= i < s^2; not renormalised (the Nystrom
    approximation can go negative).  N is the host int `n`, or len_dev[bag] read on the device (clamped into the side's
    bucket) for a replayed step.  Returns [8, s^2] fp32; 8 x 256 floats of workspace, two launches, no host sync."""
    if (n is None) == (len_dev is None):
        raise ValueError("tm_cls_attention: give the bag length either as n or as len_dev (+ bag)")
    A1, Z, A3 = _f32c(A1, "A1"), _f32c(Z, "Z"), _f32c(A3, "A3")
    n_pad = A3.shape[-1]
    if tuple(A1.shape) != (TM_H, n_pad, TM_M) or tuple(Z.shape) != (TM_H, TM_M, TM_M) or tuple(A3.shape) != (TM_H, TM_M, n_pad):
        raise _lib.MilHipError(f"tm_cls_attention: A1 {tuple(A1.shape)} / Z {tuple(Z.shape)} / A3 {tuple(A3.shape)} outside the built shape")
    if len_dev is not None and (len_dev.dtype != torch.int32 or not 0 <= int(bag) < len_dev.numel()):
        raise _lib.MilHipError("tm_cls_attention: len_dev must be int32 and hold entry `bag`")
    out = torch.empty((TM_H, int(s) * int(s)), device=A3.device, dtype=torch.float32)
    t = torch.empty((TM_H, TM_M), device=A3.device, dtype=torch.float32)
    _lib.checked().mil_tm_cls_attn(_p(A1), _p(Z), _p(A3), n_pad, int(pad), int(s), int(n) if n is not None else 0, _p(len_dev),
                                   int(bag), _p(t), _p(out), _stream())
    return out


def tm_cls_attention_fused(qkv, qL, kL, Z, lse3, pad: int, s: int, n=None, len_dev=None, bag: int = 0):
    """tm_cls_attention's output from the operands of the two fused passes, with neither A1 nor A3 formed
    (mil_tm_cls_attn_fused, csrc/cls_attn_fused.hip): qkv [n_pad, 1536] the merged rows, qL (scaled) and kL [8, 256, 64] as
    mil_tm_landmarks leaves them, Z [8, 256, 256] the last pseudo-inverse iterate, lse3 [8, 256] as tm_lmk_attn returns it,
    pad = n_pad - s^2 - 1 the cls row.  The length is the host int `n`, or len_dev[bag] read on the device (clamped into the
    side's bucket).  Returns [8, s^2] fp32, zeros from N on.  The workspace is one torch.empty of 8 x (256 + n_pad) floats;
    three launches, no atomics, no host sync, bit-reproducible."""
    if (n is None) == (len_dev is None):
        raise ValueError("tm_cls_attention_fused: give the bag length either as n or as len_dev (+ bag)")
    qkv, qL, kL, Z, lse3 = (_f32c(t, nm) for t, nm in ((qkv, "qkv"), (qL, "qL"), (kL, "kL"), (Z, "Z"), (lse3, "lse3")))
    n_pad, f32 = _fused_operands("tm_cls_attention_fused", qkv, qL=qL, kL=kL)
    if tuple(Z.shape) != (TM_H, TM_M, TM_M) or lse3.numel() != TM_H * TM_M:
        raise _lib.MilHipError(f"tm_cls_attention_fused: Z {tuple(Z.shape)} / lse3 {tuple(lse3.shape)} outside the built shape")
    if Z.device != qkv.device or lse3.device != qkv.device:
        raise _lib.MilHipError("tm_cls_attention_fused: qkv, Z and lse3 must be on one device")
    if len_dev is not None and (len_dev.dtype != torch.int32 or len_dev.device != qkv.device
                                or not 0 <= int(bag) < len_dev.numel()):
        raise _lib.MilHipError("tm_cls_attention_fused: len_dev must be int32 on qkv's device and hold entry `bag`")
    out = torch.empty((TM_H, int(s) * int(s)), **f32)
    ws = torch.empty(_lib.lib().mil_tm_cls_attn_fused_ws_floats(n_pad), **f32)
    _lib.checked().mil_tm_cls_attn_fused(_p(qkv), _p(qL), _p(kL), _p(Z), _p(lse3), n_pad, int(pad), int(s),
                                         int(n) if n is not None else 0, _p(len_dev), int(bag), _p(ws), _p(out), _stream())
    return out


def _fused_operands(op, qkv, **small):
    """The operands of a fused pass: qkv [n_pad, 1536] with n_pad a positive multiple of 256, every keyword an [8, 256, 64] tensor
    on qkv's device; `op` is the caller the message names.  Returns n_pad and the keywords of the outputs' torch.empty."""
    if (qkv.dim() != 2 or qkv.shape[1] != 3 * TM_D or qkv.shape[0] <= 0 or qkv.shape[0] % TM_M
            or any(tuple(t.shape) != (TM_H, TM_M, TM_DH) for t in small.values())):
        shapes = " / ".join(f"{k} {tuple(t.shape)}" for k, t in [("qkv", qkv), *small.items()])
        raise _lib.MilHipError(f"{op}: {shapes} outside the built shape")
    if any(t.device != qkv.device for t in small.values()):
        raise _lib.MilHipError(f"{op}: qkv, {' and '.join(small)} must be on one device")
    return qkv.shape[0], dict(device=qkv.device, dtype=torch.float32)


def _fused_dqkv(op, dqkv, qkv):
    """The [n_pad, 1536] rows a fused backward writes its columns of: the caller's, or a fresh torch.empty when None."""
    if dqkv is None:
        return torch.empty((qkv.shape[0], 3 * TM_D), device=qkv.device, dtype=torch.float32)
    if dqkv.dtype != torch.float32 or not dqkv.is_contiguous() or tuple(dqkv.shape) != (qkv.shape[0], 3 * TM_D) or dqkv.device != qkv.device:
        raise _lib.MilHipError(f"{op}: dqkv must be a contiguous float32 [n_pad, 1536] tensor on qkv's device")
    return dqkv


def _small_out(op, name, out, like):
    """An [8, 256, 64] output of a fused pass: the caller's `out` (say a bag's slice of a stacked buffer), or a fresh torch.empty."""
    if out is None:
        return torch.empty((TM_H, TM_M, TM_DH), device=like.device, dtype=torch.float32)
    if out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (TM_H, TM_M, TM_DH) or out.device != like.device:
        raise _lib.MilHipError(f"{op}: {name} must be a contiguous float32 [8, 256, 64] tensor on qkv's device")
    return out


def tm_lmk_attn(qkv, qL, out=None):
    """The landmark-query pass without its map (mil_tm_lmk_attn_fwd, csrc/landmark_attn.hip): qkv [n_pad, 1536], qL [8, 256, 64]
    (scaled, as mil_tm_landmarks leaves it) -> (W [8, 256, 64] = softmax(qL k^T) v, lse [8, 256]) over all n_pad keys.  The
    workspace is one torch.empty below the size of one map; two launches, no host sync, bit-reproducible.  out: where W goes
    (default: a fresh tensor)."""
    qkv, qL = _f32c(qkv, "qkv"), _f32c(qL, "qL")
    n, f32 = _fused_operands("tm_lmk_attn", qkv, qL=qL)
    W = _small_out("tm_lmk_attn", "out", out, qkv)
    lse = torch.empty((TM_H, TM_M), **f32)
    ws = torch.empty(_lib.lib().mil_tm_lmk_attn_ws_floats(n, 0), **f32)
    _lib.checked().mil_tm_lmk_attn_fwd(_p(qkv), _p(qL), n, _p(W), _p(lse), _p(ws), _stream())
    return W, lse


def tm_lmk_attn_bwd(qkv, qL, W, lse, dW, dqkv=None, dqL=None):
    """Backward of tm_lmk_attn (mil_tm_lmk_attn_bwd): -> (dqkv, dqL).  Columns 512 .. 1535 of dqkv [n_pad, 1536] (a fresh
    torch.empty when None) are overwritten with dk | dv, columns 0 .. 511 are left as they are; dqL [8, 256, 64] (the caller's,
    or a fresh tensor when None) is overwritten.  Three launches, no atomics, no host sync."""
    qkv, qL, W, lse, dW = (_f32c(t, nm) for t, nm in ((qkv, "qkv"), (qL, "qL"), (W, "W"), (lse, "lse"), (dW, "dW")))
    n, f32 = _fused_operands("tm_lmk_attn_bwd", qkv, qL=qL)
    if tuple(W.shape) != (TM_H, TM_M, TM_DH) or tuple(dW.shape) != (TM_H, TM_M, TM_DH) or lse.numel() != TM_H * TM_M:
        raise _lib.MilHipError(f"tm_lmk_attn_bwd: W {tuple(W.shape)} / dW {tuple(dW.shape)} / lse {tuple(lse.shape)} outside the built shape")
    dqkv = _fused_dqkv("tm_lmk_attn_bwd", dqkv, qkv)
    dqL = _small_out("tm_lmk_attn_bwd", "dqL", dqL, qkv)
    ws = torch.empty(_lib.lib().mil_tm_lmk_attn_ws_floats(n, 1), **f32)
    _lib.checked().mil_tm_lmk_attn_bwd(_p(qkv), _p(qL), _p(W), _p(lse), _p(dW), n, _p(dqkv), _p(dqL), _p(ws), _stream())
    return dqkv, dqL


def tm_tok_attn(qkv, kL, U):
    """The token-query pass without its map (mil_tm_tok_attn_fwd, csrc/token_attn.hip): qkv [n_pad, 1536], kL [8, 256, 64] (not
    scaled), U [8, 256, 64] -> (O [n_pad, 512] = softmax(64^-0.5 q kL^T) U with the heads merged, lse [8, n_pad]); every row is a
    query.  One launch, no workspace, no host sync, bit-reproducible."""
    qkv, kL, U = _f32c(qkv, "qkv"), _f32c(kL, "kL"), _f32c(U, "U")
    n, f32 = _fused_operands("tm_tok_attn", qkv, kL=kL, U=U)
    O = torch.empty((n, TM_D), **f32)
    lse = torch.empty((TM_H, n), **f32)
    nws = _lib.lib().mil_tm_tok_attn_ws_floats(n, 0)            # 0 as built: every row's 256 landmarks meet in one wave
    ws = torch.empty(nws, **f32) if nws else None
    _lib.checked().mil_tm_tok_attn_fwd(_p(qkv), _p(kL), _p(U), n, _p(O), _p(lse), _p(ws), _stream())
    return O, lse


def tm_tok_attn_bwd(qkv, kL, U, lse, dO, dqkv=None, dU=None, dkL=None):
    """Backward of tm_tok_attn (mil_tm_tok_attn_bwd): -> (dqkv, dU, dkL).  Columns 0 .. 511 of dqkv [n_pad, 1536] (a fresh
    torch.empty when None) are overwritten with dq, columns 512 .. 1535 are left as they are; dU and dkL [8, 256, 64] (the
    caller's, or fresh tensors when None) are overwritten.  The workspace is one torch.empty of half a map; two launches, no
    atomics, no host sync."""
    qkv, kL, U, lse, dO = (_f32c(t, nm) for t, nm in ((qkv, "qkv"), (kL, "kL"), (U, "U"), (lse, "lse"), (dO, "dO")))
    n, f32 = _fused_operands("tm_tok_attn_bwd", qkv, kL=kL, U=U)
    if tuple(lse.shape) != (TM_H, n) or tuple(dO.shape) != (n, TM_D) or lse.device != qkv.device or dO.device != qkv.device:
        raise _lib.MilHipError(f"tm_tok_attn_bwd: lse {tuple(lse.shape)} / dO {tuple(dO.shape)} outside the built shape or on another device")
    dqkv = _fused_dqkv("tm_tok_attn_bwd", dqkv, qkv)
    dU = _small_out("tm_tok_attn_bwd", "dU", dU, qkv)
    dkL = _small_out("tm_tok_attn_bwd", "dkL", dkL, qkv)
    ws = torch.empty(_lib.lib().mil_tm_tok_attn_ws_floats(n, 1), **f32)
    _lib.checked().mil_tm_tok_attn_bwd(_p(qkv), _p(kL), _p(U), _p(lse), _p(dO), n, _p(dqkv), _p(dU), _p(dkL), _p(ws), _stream())
    return dqkv, dU, dkL


def _tm_bg(det: bool, pieces: int):
    """tm_bgemm with the arithmetic of one core call bound: the fixed-order split-K form and / or the split-bf16 route."""
    return functools.partial(tm_bgemm, deterministic=det, pieces=pieces) if det or pieces else tm_bgemm


# ---- the Nystrom core in phases.  _tm_fwd / _tm_bwd (one bag) and _tm_fwd_bags / _tm_bwd_bags (all bags of a step) issue the
# same phases: the token-side ones per bag, the landmark-side ones on [8, 256, .] operands of one bag or on the stacked
# [nb, 8, 256, .] operands of all bags as one launch of batch 8 nb.  Every landmark-side product has K <= 256, so it runs
# unsplit at any batch (_tm_splits) and a bag's tiles are computed with the arithmetic of the batch-8 launch.
_SQ = (TM_M * TM_M, TM_M, 1)            # [., 256, 256] row-major, and its transpose
_SQT = (TM_M * TM_M, 1, TM_M)
_SL = (TM_M * TM_DH, TM_DH, 1)          # [., 256, 64] row-major, and its transpose
_SLT = (TM_M * TM_DH, 1, TM_DH)


def _tm_pinv_fwd(A2, det=False, pieces=0, nb=None):
    """Newton-Schulz pseudo-inverse of A2 [8, 256, 256]: Z0 = A2^T / (max row sum x max column sum over the bag's 8 heads), then
    six times X = A2 Z, T2 = 15 I - X (7 I - X) = X X - 7 X + 15 I, T3 = 13 I - X T2, Z = Z T3 / 4.  Returns the last Z and what
    _tm_pinv_bwd takes: (scale, arg, Zs, Xs, T2s, T3s).
    nb: A2 is [nb, 8, 256, 256], nb bags' maps stacked; each bag's Z0 is scaled by its own 8 heads (mil_tm_pinv_init_bags) and
    the products run at batch 8 nb.  None is the single bag on mil_tm_pinv_init."""
    bg = _tm_bg(det, pieces)
    H, M = TM_H, TM_M
    f32 = dict(device=A2.device, dtype=torch.float32)
    lead = () if nb is None else (nb,)
    scale = torch.empty(lead + (3 + 2 * H,), **f32)             # (s, max row sum, max column sum), per-head maxima behind
    arg = torch.empty(lead + (1 + H,), device=A2.device, dtype=torch.int32)
    Zs, Xs, T2s, T3s = [], [], [], []
    Z = torch.empty_like(A2)
    if nb is None:
        _lib.checked().mil_tm_pinv_init(_p(A2), _p(scale), _p(arg), _p(Z), _stream())
    else:
        _lib.checked().mil_tm_pinv_init_bags(_p(A2), nb, _p(scale), _p(arg), _p(Z), _stream())
    sq, batch = _SQ, H * (nb or 1)
    for _ in range(TM_PINV_ITERS):
        X = bg(A2, sq, Z, sq, torch.empty_like(Z), sq, batch, M, M, M)
        T2 = bg(X, sq, X, sq, torch.empty_like(Z), sq, batch, M, M, M, beta=-7.0, diag=15.0, D=X)
        T3 = bg(X, sq, T2, sq, torch.empty_like(Z), sq, batch, M, M, M, alpha=-1.0, diag=13.0)
        Zn = bg(Z, sq, T3, sq, torch.empty_like(Z), sq, batch, M, M, M, alpha=0.25)
        Zs.append(Z); Xs.append(X); T2s.append(T2); T3s.append(T3)
        Z = Zn
    return Z, (scale, arg, Zs, Xs, T2s, T3s)


def _tm_fwd_landmarks(qkv, qL, kL, bg, fused_a1):
    """Token side, one bag: the landmarks into qL / kL [8, 256, 64] and, unless the token-query pass runs fused, its map
    A1 [8, n_pad, 256] (not yet softmaxed).  Returns A1 or None."""
    n = qkv.shape[0]
    _lib.checked().mil_tm_landmarks(_p(qkv), n, TM_QSCALE, _p(qL), _p(kL), _stream())
    if fused_a1:
        return None
    A1 = torch.empty((TM_H, n, TM_M), device=qkv.device, dtype=torch.float32)
    bg(qkv, (TM_DH, 3 * TM_D, 1), kL, _SLT, A1, (n * TM_M, TM_M, 1), TM_H, n, TM_M, TM_DH, alpha=TM_QSCALE)
    return A1


def _tm_fwd_a2(qL, kL, A2, bg, batch):
    """Landmark side: A2 = qL kL^T (not yet softmaxed) over `batch` heads."""
    return bg(qL, _SL, kL, _SLT, A2, _SQ, batch, TM_M, TM_M, TM_DH)


def _tm_fwd_lmk(qkv, qL, A1, A2, W, bg, fused_a3):
    """Token side, one bag: the row softmax of the maps at hand - A1 (or None), A2 (None when the caller softmaxes it
    itself, stacked over the bags), A3 - and W [8, 256, 64] = softmax(qL k^T) v into `W`.  Returns (A3, lse3): the softmaxed
    map, or (fused) its rows' logsumexp."""
    n = qkv.shape[0]
    maps = [A for A in (A1, A2) if A is not None]
    if fused_a3:        # no A3: W and the rows' logsumexp straight from qL and the k | v columns
        for A in maps:
            tm_softmax_rows(A)
        _, lse3 = tm_lmk_attn(qkv, qL, W)
        return None, lse3
    A3 = torch.empty((TM_H, TM_M, n), device=qkv.device, dtype=torch.float32)
    bg(qL, _SL, qkv[:, TM_D:], (TM_DH, 1, 3 * TM_D), A3, (TM_M * n, n, 1), TM_H, TM_M, n, TM_DH)
    for A in maps + [A3]:
        tm_softmax_rows(A)
    bg(A3, (TM_M * n, n, 1), qkv[:, 2 * TM_D:], (TM_DH, 3 * TM_D, 1), W, _SL, TM_H, TM_M, TM_DH, n)
    return A3, None


def _tm_fwd_u(Z, W, U, bg, batch):
    """Landmark side: U = Z W over `batch` heads."""
    return bg(Z, _SQ, W, _SL, U, _SL, batch, TM_M, TM_DH, TM_M)


def _tm_fwd_tok(qkv, w, A1, kL, U, bg, fused_a1):
    """Token side, one bag: O [n_pad, 512] = A1 U with the heads merged (fused: straight from the q columns, kL and U), plus
    the residual conv of v.  Returns (O, lse1)."""
    n = qkv.shape[0]
    lse1 = None
    if fused_a1:        # no A1: O and the rows' logsumexp straight from the q columns, kL and U
        O, lse1 = tm_tok_attn(qkv, kL, U)
    else:
        O = torch.empty((n, TM_D), device=qkv.device, dtype=torch.float32)
        bg(A1, (n * TM_M, TM_M, 1), U, _SL, O, (TM_DH, TM_D, 1), TM_H, n, TM_DH, TM_M)
    _lib.checked().mil_tm_resconv(_p(qkv), _p(w), n, _p(O), _stream())
    return O, lse1


def _tm_fwd(qkv, w, need_attn, cls=None, fused_a3=False, fused_a1=False, fused_cls=False, det=False, pieces=0):
    """det: the split-K products on mil_tm_bgemm_fixed; kept in `saved`, so that the backward takes the fixed-order entries too.
    pieces: 3 routes the products of _tm_pieces_route to mil_tm_bgemm_pieces; kept in `saved` the same way."""
    bg = _tm_bg(det, pieces)
    if fused_cls:       # the cls attention reads qL, kL, Z and lse3 only: neither map is formed, whatever the two switches say
        fused_a3 = fused_a1 = True
    n = qkv.shape[0]
    f32 = dict(device=qkv.device, dtype=torch.float32)
    H, M, DH = TM_H, TM_M, TM_DH
    qL = torch.empty((H, M, DH), **f32)
    kL = torch.empty((H, M, DH), **f32)
    A1 = _tm_fwd_landmarks(qkv, qL, kL, bg, fused_a1)
    A2 = _tm_fwd_a2(qL, kL, torch.empty((H, M, M), **f32), bg, H)
    W = torch.empty((H, M, DH), **f32)
    A3, lse3 = _tm_fwd_lmk(qkv, qL, A1, A2, W, bg, fused_a3)
    Z, pinv = _tm_pinv_fwd(A2, det, pieces)
    U = _tm_fwd_u(Z, W, torch.empty((H, M, DH), **f32), bg, H)
    O, lse1 = _tm_fwd_tok(qkv, w, A1, kL, U, bg, fused_a1)
    attn = None
    if need_attn == "cls":  # the cls row of that map folded onto the patches, [8, s^2]: no map is formed
        attn = tm_cls_attention_fused(qkv, qL, kL, Z, lse3, **cls) if fused_cls else tm_cls_attention(A1, Z, A3, **cls)
    elif need_attn:         # A1 Z A3 [8, n_pad, n_pad] (nystrom_attention return_attn), forward only
        T = bg(A1, (n * M, M, 1), Z, _SQ, torch.empty((H, n, M), **f32), (n * M, M, 1), H, n, M, M)
        attn = bg(T, (n * M, M, 1), A3, (M * n, n, 1), torch.empty((H, n, n), **f32), (n * n, n, 1), H, n, n, M)
    saved = SimpleNamespace(qL=qL, kL=kL, A1=A1, lse1=lse1, A2=A2, A3=A3, lse3=lse3, W=W, U=U, Z=Z,
                            pinv=pinv, det=det, pieces=pieces)
    return O, attn, saved


def _tm_fwd_bags(qkvs, w, fused_a3=False, fused_a1=False, det=False, pieces=0):
    """_tm_fwd (need_attn False) over the bags of a step: the token-side phases per bag, writing each bag's landmarks and W
    into its slice of buffers stacked [nb, 8, 256, .]; then A2, its softmax, the pseudo-inverse and U once for all bags at
    batch 8 nb; then each bag's O.  Returns ([O_b], saved): the stacked landmark-side tensors plus, per bag, its maps / lse."""
    bg = _tm_bg(det, pieces)
    nb = len(qkvs)
    f32 = dict(device=qkvs[0].device, dtype=torch.float32)
    H, M, DH = TM_H, TM_M, TM_DH
    qL, kL, W = (torch.empty((nb, H, M, DH), **f32) for _ in range(3))
    bags = []
    for b, qkv in enumerate(qkvs):
        A1 = _tm_fwd_landmarks(qkv, qL[b], kL[b], bg, fused_a1)
        A3, lse3 = _tm_fwd_lmk(qkv, qL[b], A1, None, W[b], bg, fused_a3)
        bags.append(SimpleNamespace(A1=A1, A3=A3, lse1=None, lse3=lse3))
    A2 = tm_softmax_rows(_tm_fwd_a2(qL, kL, torch.empty((nb, H, M, M), **f32), bg, nb * H))
    Z, pinv = _tm_pinv_fwd(A2, det, pieces, nb=nb)
    U = _tm_fwd_u(Z, W, torch.empty((nb, H, M, DH), **f32), bg, nb * H)
    outs = []
    for b, qkv in enumerate(qkvs):
        O, bags[b].lse1 = _tm_fwd_tok(qkv, w, bags[b].A1, kL[b], U[b], bg, fused_a1)
        outs.append(O)
    saved = SimpleNamespace(qL=qL, kL=kL, A2=A2, W=W, U=U, Z=Z, pinv=pinv, det=det, pieces=pieces, bags=bags,
                            fused_a1=fused_a1, fused_a3=fused_a3)
    return outs, saved


def _tm_pinv_bwd(G, A2, scale, arg, Zs, Xs, T2s, T3s, det=False, pieces=0, nb=None):
    """dA2 from dZ (the gradient of the last iterate) by the reverse sweep of the six iterations and of Z0.  nb: as in
    _tm_pinv_fwd - the stacked form, with the grouped backward of the start."""
    bg = _tm_bg(det, pieces)
    M, batch = TM_M, TM_H * (nb or 1)
    sq, sqt = _SQ, _SQT
    dA2 = torch.zeros_like(A2)
    for t in reversed(range(TM_PINV_ITERS)):
        Z, X, T2, T3 = Zs[t], Xs[t], T2s[t], T3s[t]
        dZ = bg(G, sq, T3, sqt, torch.empty_like(Z), sq, batch, M, M, M, alpha=0.25)           # Zn = Z T3 / 4
        dT3 = bg(Z, sqt, G, sq, torch.empty_like(Z), sq, batch, M, M, M, alpha=0.25)
        dT2 = bg(X, sqt, dT3, sq, torch.empty_like(Z), sq, batch, M, M, M, alpha=-1.0)         # T3 = 13 I - X T2
        dX = bg(dT3, sq, T2, sqt, torch.empty_like(Z), sq, batch, M, M, M, alpha=-1.0, beta=-7.0, D=dT2)
        bg(dT2, sq, X, sqt, dX, sq, batch, M, M, M, beta=1.0)                                  # T2 = X X - 7 X + 15 I
        bg(X, sqt, dT2, sq, dX, sq, batch, M, M, M, beta=1.0)
        bg(dX, sq, Z, sqt, dA2, sq, batch, M, M, M, beta=1.0)                                  # X = A2 Z
        bg(A2, sqt, dX, sq, dZ, sq, batch, M, M, M, beta=1.0)
        G = dZ
    if nb is not None:
        if det:
            ws = _ws(_lib.lib().mil_tm_pinv_ws_floats_bags(nb), A2)
            _lib.checked().mil_tm_pinv_init_bwd_bags_fixed(_p(G), _p(Zs[0]), _p(scale), _p(arg), nb, _p(dA2), _p(ws), _stream())
            return dA2
        ws = torch.zeros(nb, device=A2.device, dtype=torch.float32)
        _lib.checked().mil_tm_pinv_init_bwd_bags(_p(G), _p(Zs[0]), _p(scale), _p(arg), nb, _p(dA2), _p(ws), _stream())
        return dA2
    if det:
        ws = _ws(_lib.lib().mil_tm_pinv_ws_floats(), A2)
        _lib.checked().mil_tm_pinv_init_bwd_fixed(_p(G), _p(Zs[0]), _p(scale), _p(arg), _p(dA2), _p(ws), _stream())
        return dA2
    ws = torch.zeros(1, device=A2.device, dtype=torch.float32)
    _lib.checked().mil_tm_pinv_init_bwd(_p(G), _p(Zs[0]), _p(scale), _p(arg), _p(dA2), _p(ws), _stream())
    return dA2


def _tm_bwd_tok(dO, qkv, A1, lse1, kL, U, dqkv, dU, dkL, bg):
    """Token side, one bag: dU into `dU`; fused (lse1 given) also dq into columns 0 .. 511 of dqkv before anything adds onto
    them and the pass's share of dkL into `dkL`; else dA1, returned."""
    n = qkv.shape[0]
    if lse1 is not None:
        tm_tok_attn_bwd(qkv, kL, U, lse1, dO, dqkv, dU, dkL)
        return None
    dA1 = bg(dO, (TM_DH, TM_D, 1), U, _SLT, torch.empty((TM_H, n, TM_M), device=qkv.device, dtype=torch.float32),
             (n * TM_M, TM_M, 1), TM_H, n, TM_M, TM_DH)
    bg(A1, (n * TM_M, 1, TM_M), dO, (TM_DH, TM_D, 1), dU, _SL, TM_H, TM_M, TM_DH, n)
    return dA1


def _tm_bwd_zw(dU, W, Z, dZ, dW, bg, batch):
    """Landmark side: dZ = dU W^T and dW = Z^T dU over `batch` heads."""
    bg(dU, _SL, W, _SLT, dZ, _SQ, batch, TM_M, TM_M, TM_DH)
    bg(Z, _SQT, dU, _SL, dW, _SL, batch, TM_M, TM_DH, TM_M)


def _tm_bwd_lmk(dO, qkv, w, A3, lse3, qL, W, dW, dqkv, dqL, dw, det, bg):
    """Token side, one bag: fused (lse3 given) dk | dv into dqkv and the pass's share of dqL into `dqL`, before the stages that
    add onto them; else dA3 (returned) and dv.  Then the residual conv's backward: the v columns of dqkv and dw [8 x 33]."""
    n = qkv.shape[0]
    dA3 = None
    if lse3 is not None:
        tm_lmk_attn_bwd(qkv, qL, W, lse3, dW, dqkv, dqL)
    else:
        dA3 = bg(dW, _SL, qkv[:, 2 * TM_D:], (TM_DH, 1, 3 * TM_D), torch.empty((TM_H, TM_M, n), device=qkv.device, dtype=torch.float32),
                 (TM_M * n, n, 1), TM_H, TM_M, n, TM_DH)
        bg(A3, (TM_M * n, 1, n), dW, _SL, dqkv[:, 2 * TM_D:], (TM_DH, 3 * TM_D, 1), TM_H, n, TM_DH, TM_M)    # dv = A3^T dW
    if det:
        _lib.checked().mil_tm_resconv_bwd_fixed(_p(dO), _p(qkv), _p(w), n, _p(dqkv), _p(dw),
                                                _p(_ws(_lib.lib().mil_tm_resconv_ws_floats(n), qkv)), _stream())
    else:
        _lib.checked().mil_tm_resconv_bwd(_p(dO), _p(qkv), _p(w), n, _p(dqkv), _p(dw), _stream())
    return dA3


def _tm_bwd_s1(dS1, qkv, kL, dqkv, dkL, bg):
    """Token side, one bag, materialised A1: dq into dqkv and the map's share of dkL (overwritten) from dS1."""
    n = qkv.shape[0]
    bg(dS1, (n * TM_M, TM_M, 1), kL, _SL, dqkv, (TM_DH, 3 * TM_D, 1), TM_H, n, TM_DH, TM_M, alpha=TM_QSCALE)        # dq
    bg(dS1, (n * TM_M, 1, TM_M), qkv, (TM_DH, 3 * TM_D, 1), dkL, _SL, TM_H, TM_M, TM_DH, n, alpha=TM_QSCALE)


def _tm_bwd_s2(dS2, qL, kL, dkL, dqL, fused_a3, bg, batch):
    """Landmark side: dkL += dS2^T qL; dqL += dS2 kL behind the fused landmark pass's share, else dqL = dS2 kL."""
    bg(dS2, _SQT, qL, _SL, dkL, _SL, batch, TM_M, TM_DH, TM_M, beta=1.0)
    bg(dS2, _SQ, kL, _SL, dqL, _SL, batch, TM_M, TM_DH, TM_M, beta=1.0 if fused_a3 else 0.0)


def _tm_bwd_tail(dS3, qkv, qL, dqL, dkL, dqkv, bg):
    """Token side, one bag: with a materialised A3 its share of dqL and dk from dS3; then the landmark gradients spread onto
    the q and k columns of dqkv."""
    n = qkv.shape[0]
    if dS3 is not None:
        bg(dS3, (TM_M * n, n, 1), qkv[:, TM_D:], (TM_DH, 3 * TM_D, 1), dqL, _SL, TM_H, TM_M, TM_DH, n, beta=1.0)
        bg(dS3, (TM_M * n, 1, n), qL, _SL, dqkv[:, TM_D:], (TM_DH, 3 * TM_D, 1), TM_H, n, TM_DH, TM_M)      # dk
    _lib.checked().mil_tm_landmarks_bwd(_p(dqL), _p(dkL), n, TM_QSCALE, _p(dqkv), _stream())


def _tm_bwd(dO, qkv, w, saved):
    """`saved` as _tm_fwd left it: a pass that ran fused has its lse (lse1 [8, n_pad], lse3 [8, 256]) and no map, and its
    backward takes the fused entry too."""
    s = saved
    qL, kL, A1, A2, A3, W, U, Z = s.qL, s.kL, s.A1, s.A2, s.A3, s.W, s.U, s.Z
    fused_a3 = s.lse3 is not None
    det, pieces = s.det, getattr(s, "pieces", 0)
    bg = _tm_bg(det, pieces)
    n = qkv.shape[0]
    f32 = dict(device=qkv.device, dtype=torch.float32)
    H, M, DH = TM_H, TM_M, TM_DH
    dqkv = torch.empty((n, 3 * TM_D), **f32)
    dw = torch.empty(H * TM_CONV, **f32) if det else torch.zeros(H * TM_CONV, **f32)      # the fold overwrites dw
    dU, dkL, dqL, dW = (torch.empty((H, M, DH), **f32) for _ in range(4))
    dA1 = _tm_bwd_tok(dO, qkv, A1, s.lse1, kL, U, dqkv, dU, dkL, bg)
    dZ = torch.empty((H, M, M), **f32)
    _tm_bwd_zw(dU, W, Z, dZ, dW, bg, H)
    dA3 = _tm_bwd_lmk(dO, qkv, w, A3, s.lse3, qL, W, dW, dqkv, dqL, dw, det, bg)
    dS1 = tm_softmax_rows_bwd(A1, dA1) if dA1 is not None else None
    dS3 = tm_softmax_rows_bwd(A3, dA3) if dA3 is not None else None
    dS2 = tm_softmax_rows_bwd(A2, _tm_pinv_bwd(dZ, A2, *s.pinv, det=det, pieces=pieces))
    if dS1 is not None:
        _tm_bwd_s1(dS1, qkv, kL, dqkv, dkL, bg)
    _tm_bwd_s2(dS2, qL, kL, dkL, dqL, fused_a3, bg, H)
    _tm_bwd_tail(dS3, qkv, qL, dqL, dkL, dqkv, bg)
    return dqkv, dw


def _tm_bwd_bags(dOs, qkvs, w, saved):
    """_tm_bwd over the bags of a step, `saved` as _tm_fwd_bags left it: per bag dU (and dA1 or the fused token backward) into
    stacked buffers; dZ and dW at batch 8 nb; per bag the A3 side, the residual conv and the maps' softmax backward; the
    pseudo-inverse's reverse sweep, A2's softmax backward and the two dS2 products at batch 8 nb; per bag what remains.
    Returns ([dqkv_b], dw) with dw the bags' dw_b added in bag order."""
    s = saved
    qL, kL, A2, W, U, Z = s.qL, s.kL, s.A2, s.W, s.U, s.Z
    det, pieces = s.det, s.pieces
    bg = _tm_bg(det, pieces)
    nb = len(qkvs)
    f32 = dict(device=w.device, dtype=torch.float32)
    H, M, DH = TM_H, TM_M, TM_DH
    dqkvs = [torch.empty((qkv.shape[0], 3 * TM_D), **f32) for qkv in qkvs]
    dws = torch.empty((nb, H * TM_CONV), **f32) if det else torch.zeros((nb, H * TM_CONV), **f32)
    dU, dkL, dqL, dW = (torch.empty((nb, H, M, DH), **f32) for _ in range(4))
    dA1s = [_tm_bwd_tok(dOs[b], qkvs[b], g.A1, g.lse1, kL[b], U[b], dqkvs[b], dU[b], dkL[b], bg) for b, g in enumerate(s.bags)]
    dZ = torch.empty((nb, H, M, M), **f32)
    _tm_bwd_zw(dU, W, Z, dZ, dW, bg, nb * H)
    dS3s = []
    for b, g in enumerate(s.bags):
        dA3 = _tm_bwd_lmk(dOs[b], qkvs[b], w, g.A3, g.lse3, qL[b], W[b], dW[b], dqkvs[b], dqL[b], dws[b], det, bg)
        dS3s.append(tm_softmax_rows_bwd(g.A3, dA3) if dA3 is not None else None)
        if dA1s[b] is not None:
            _tm_bwd_s1(tm_softmax_rows_bwd(g.A1, dA1s[b]), qkvs[b], kL[b], dqkvs[b], dkL[b], bg)
            dA1s[b] = None
    dS2 = tm_softmax_rows_bwd(A2, _tm_pinv_bwd(dZ, A2, *s.pinv, det=det, pieces=pieces, nb=nb))
    _tm_bwd_s2(dS2, qL, kL, dkL, dqL, s.fused_a3, bg, nb * H)
    for b in range(nb):
        _tm_bwd_tail(dS3s[b], qkvs[b], qL[b], dqL[b], dkL[b], dqkvs[b], bg)
    dw = dws[0]
    for b in range(1, nb):
        dw = dw + dws[b]
    return dqkvs, dw


class _NystromCore(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, w, need_attn, cls=None, fused_a3=False, fused_a1=False, fused_cls=False, det=False, pieces=0):
        qkv = _f32c(qkv, "qkv")
        w = _f32c(w, "res_conv.weight")
        if qkv.shape[1] != 3 * TM_D or qkv.shape[0] % TM_M or w.numel() != TM_H * TM_CONV:
            raise _lib.MilHipError(f"nystrom_core: qkv {tuple(qkv.shape)} / res_conv {tuple(w.shape)} outside the built shape")
        O, attn, saved = _tm_fwd(qkv, w, need_attn, cls, fused_a3, fused_a1, fused_cls, det, pieces)
        ctx.saved = saved
        ctx.save_for_backward(qkv, w)
        ctx.w_shape = w.shape
        if attn is not None:
            ctx.mark_non_differentiable(attn)
        return O, attn

    @staticmethod
    def backward(ctx, dO, _dattn):
        qkv, w = ctx.saved_tensors
        dqkv, dw = _tm_bwd(_f32c(dO, "dO"), qkv, w, ctx.saved)
        ctx.saved = None
        return dqkv, dw.reshape(ctx.w_shape), None, None, None, None, None, None, None


def nystrom_core(qkv, w, need_attn=False, *, pad=None, s=None, n=None, len_dev=None, bag: int = 0, fused_a3=None,
                 fused_a1=None, fused_cls=None, deterministic=None, pieces=None):
    """qkv [n_pad, 1536] (to_qkv of the front-zero-padded rows, n_pad % 256 == 0), w = res_conv.weight [8, 1, 33, 1] ->
    (out [n_pad, 512] merged heads before to_out, attn).  need_attn: False -> attn None; True -> the whole map
    [8, n_pad, n_pad]; "cls" -> the cls token's per-patch attention [8, s^2] (tm_cls_attention), which needs the bag's geometry
    as keywords: pad, s and the length as n or as len_dev (+ bag).  attn carries no gradient in any mode.
    The switches are keywords: a module passes what tm_route resolved, None reads the switch's environment variable at the call.
    fused_a3: the landmark-query pass (softmax(qL k^T) v and its backward) as one kernel family that never forms the
    [8, 256, n_pad] map (tm_lmk_attn).  fused_a1: the same for the token-query pass (softmax(q kL^T) U, tm_tok_attn) and the
    [8, n_pad, 256] map.  The two are independent and apply with need_attn False only: True and "cls" read the maps.
    fused_cls: with need_attn "cls", the cls attention from the fused passes' operands (tm_cls_attention_fused); BOTH passes then
    run fused, forward and backward, whatever the other two say, and no map is formed.
    deterministic: every sum that crosses workgroups in a fixed order (the mil_tm_*_fixed entries: split-K products, the
    pseudo-inverse scale's gradient, the res_conv weight gradient), forward and backward: two runs give the same bits.
    pieces: 0 or 3.  3 runs the core's products with K >= 256 (_tm_pieces_route) as three-piece split-bf16 products on
    v_mfma_f32_32x32x16_bf16 (mil_tm_bgemm_pieces; fp32-level error), forward and backward; the fused passes have kernels of
    their own and are untouched.  deterministic and pieces go with every need_attn and every fused switch."""
    det = tm_deterministic(deterministic)
    pieces = tm_pieces(pieces)
    if isinstance(need_attn, bool):
        return _NystromCore.apply(qkv, w, need_attn, None, _tm_fused_a3(fused_a3, need_attn), _tm_fused_a1(fused_a1, need_attn),
                                  False, det, pieces)
    if not (isinstance(need_attn, str) and need_attn == "cls"):
        raise ValueError(f"nystrom_core: need_attn must be False, True or 'cls', got {need_attn!r}")
    if pad is None or s is None or (n is None) == (len_dev is None):
        raise ValueError("nystrom_core: need_attn='cls' needs pad, s and the bag length (n, or len_dev and bag)")
    return _NystromCore.apply(qkv, w, "cls", dict(pad=int(pad), s=int(s), n=n, len_dev=len_dev, bag=int(bag)), False, False,
                              _tm_fused_cls(fused_cls, "cls"), det, pieces)


TM_MAX_BATCH_BAGS = 1024            # the bags one grouped pseudo-inverse start takes (csrc/transmil.hip)


class _NystromCoreBags(torch.autograd.Function):
    @staticmethod
    def forward(ctx, w, fused_a3, fused_a1, det, pieces, *qkvs):
        w = _f32c(w, "res_conv.weight")
        qkvs = [_f32c(qkv, "qkv") for qkv in qkvs]
        if not 1 <= len(qkvs) <= TM_MAX_BATCH_BAGS:
            raise _lib.MilHipError(f"nystrom_core_bags: {len(qkvs)} bags, built for 1 .. {TM_MAX_BATCH_BAGS}")
        for qkv in qkvs:
            if (qkv.dim() != 2 or qkv.shape[1] != 3 * TM_D or qkv.shape[0] <= 0 or qkv.shape[0] % TM_M or qkv.device != w.device
                    or w.numel() != TM_H * TM_CONV):
                raise _lib.MilHipError(f"nystrom_core_bags: qkv {tuple(qkv.shape)} / res_conv {tuple(w.shape)} outside the built "
                                       "shape, or on two devices")
        outs, saved = _tm_fwd_bags(qkvs, w, fused_a3, fused_a1, det, pieces)
        ctx.saved = saved
        ctx.save_for_backward(w, *qkvs)
        ctx.w_shape = w.shape
        return tuple(outs)

    @staticmethod
    def backward(ctx, *dOs):
        w, *qkvs = ctx.saved_tensors
        dqkvs, dw = _tm_bwd_bags([_f32c(dO, "dO") for dO in dOs], qkvs, w, ctx.saved)
        ctx.saved = None
        return (dw.reshape(ctx.w_shape), None, None, None, None, *dqkvs)


def nystrom_core_bags(qkvs, w, *, fused_a3=None, fused_a1=None, deterministic=None, pieces=None):
    """nystrom_core (need_attn False) for all bags of a step as ONE autograd function: qkvs = one [n_pad_b, 1536] per bag (each
    n_pad_b a positive multiple of 256, they may differ; 1 .. 1024 bags), w = res_conv.weight -> [out_b [n_pad_b, 512]].
    The token-side stages - the landmarks, the A1 / A3 maps or the fused passes, the residual conv - run per bag as in
    nystrom_core.  The landmark-side chain, whose shapes do not depend on the bag, runs once on buffers stacked
    [nb, 8, 256, .]: A2 and its softmax, the pseudo-inverse's start (mil_tm_pinv_init_bags: every bag scaled by the maxima of ITS
    8 heads, as the reference does with one bag per call), the 24 + 48 chain products, U, dZ, dW and the two dS2 products, each
    one launch of batch 8 nb.  These products have K <= 256 and so one split at any batch: a bag's tiles see the arithmetic
    of the bag-by-bag launch, and with deterministic=True every out_b and dqkv_b is bit-equal to nystrom_core on that bag.
    dw is the bags' dw_b added in bag order 0, 1, 2, ...
    fused_a3, fused_a1, deterministic, pieces: as in nystrom_core.  need_attn is not offered: True and "cls" keep the bag-by-bag
    route (tm_route).  No host read; every workspace is a torch.empty, so the call can be captured into a graph."""
    return list(_NystromCoreBags.apply(w, _tm_fused_a3(fused_a3, False), _tm_fused_a1(fused_a1, False),
                                       tm_deterministic(deterministic), tm_pieces(pieces), *qkvs))


# ---- a step's bags as one packed sequence (csrc/tm_packed.h): every token-side stage one launch set over all bags' rows
class TmPackedTable:
    """The segment table of the mil_tm_*_packed entries for bags of `blocks` 256-row blocks each (host ints: the launch shapes):
    `dev`, int32 [nb + 1 + total_blocks] on the device = the cumulative block counts blk_off [nb + 1], then the bag of every
    block.  Build it with tm_packed_table, outside any capture; it depends on the bags' sides alone."""

    def __init__(self, blocks, dev):
        self.blocks = tuple(int(k) for k in blocks)
        self.nb, self.total_blocks, self.dev = len(self.blocks), sum(self.blocks), dev
        self.rows = TM_M * self.total_blocks

    def args(self):
        return _p(self.dev), self.nb, self.total_blocks


def tm_packed_table_host(blocks):
    """The table's int32 values as a list: blk_off [nb + 1], then bag_of_blk [total_blocks]."""
    blocks = [int(k) for k in blocks]
    if not 1 <= len(blocks) <= TM_MAX_BATCH_BAGS or min(blocks) < 1 or sum(blocks) > (2 ** 31 - 1) // TM_M:
        raise ValueError(f"tm_packed_table: 1 .. {TM_MAX_BATCH_BAGS} bags of at least one 256-row block each, got {blocks}")
    return list(itertools.accumulate(blocks, initial=0)) + [b for b, k in enumerate(blocks) for _ in range(k)]


def _tm_table_dev(values, device):
    """A table's int32 values on `device` (default: the current GPU).  One small host-to-device copy, so a replayed step builds
    its tables once per graph key, not per step."""
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    return torch.tensor(values, dtype=torch.int32).to(device, non_blocking=True)


def tm_packed_table(blocks, device=None) -> TmPackedTable:
    """blocks: per bag n_pad / 256 -> the TmPackedTable on `device` (_tm_table_dev)."""
    return TmPackedTable(blocks, _tm_table_dev(tm_packed_table_host(blocks), device))


class TmClsTable:
    """The geometry table of mil_tm_cls_attn_packed for bags of grid sides `sides` (host ints): `dev`, int32 [2 nb + 1] on the
    device (tm_cls_table_host has the layout); `patches` = sum s^2, the patches of the output; `off` the host offsets.  Build it
    with tm_cls_table, outside any capture; it depends on the bags' sides alone."""

    def __init__(self, sides, dev):
        self.sides = tuple(int(s) for s in sides)
        self.nb, self.dev = len(self.sides), dev
        self.off = list(itertools.accumulate((s * s for s in self.sides), initial=0))
        self.patches = self.off[-1]


def tm_cls_table_host(sides):
    """The table's int32 values as a list: side [nb] | off [nb + 1], off[b] = the sum of s^2 over the bags in front of bag b -
    where bag b's [8, s_b^2] starts in the output, in patches - and off[nb] = the patches of all bags.  A table of its own and
    not the PPEG table's row_off | side: that one counts the cls rows in (row_off[b] = off[b] + b) and carries four more arrays
    sized by its own launches, and the attention should not depend on whether PPEG runs packed."""
    sides = [int(s) for s in sides]
    if not 1 <= len(sides) <= TM_MAX_BATCH_BAGS or min(sides) < 1 or sum(s * s for s in sides) > 2 ** 31 - 1:
        raise ValueError(f"tm_cls_table: 1 .. {TM_MAX_BATCH_BAGS} bags of side >= 1, at most 2^31 - 1 patches, got {sides}")
    return sides + list(itertools.accumulate((s * s for s in sides), initial=0))


def tm_cls_table(sides, device=None) -> TmClsTable:
    """sides: per bag the grid side -> the TmClsTable on `device` (_tm_table_dev)."""
    return TmClsTable(sides, _tm_table_dev(tm_cls_table_host(sides), device))


def tm_cls_attention_packed(qkv, table, qL, kL, Z, lse3, sides, n=None, len_dev=None):
    """tm_cls_attention_fused for all bags of a packed step in ONE launch set (mil_tm_cls_attn_packed, csrc/cls_attn_fused.hip):
    qkv [256 total_blocks, 1536] the packed rows, table the TmPackedTable (tm_packed_table), qL (scaled), kL [nb, 8, 256, 64],
    Z [nb, 8, 256, 256], lse3 [nb, 8, 256] as _tm_fwd_packed holds them, sides = the bags' grid sides or a TmClsTable
    (tm_cls_table; from sides it is built here - a host-to-device copy, not for a capture).  The lengths: `n`, a host list - each
    must lie in its side's bucket ((s - 1)^2, s^2], else MilHipError as from the single-bag entry; they are then uploaded, a copy
    and so not for a capture - or `len_dev`, int32 [nb] on the device, each read there and clamped into its bucket.  Exactly one
    of the two.  Returns a list of per-bag [8, s_b^2] fp32 views of ONE buffer, bag b at float 8 off_b, zeros from N_b on, each
    bit-equal to tm_cls_attention_fused on that bag's rows and slices.  One torch.empty of workspace (nb x 2048 + 2048 x
    total_blocks floats); three launches whatever the bag count, no atomics, no host read."""
    if (n is None) == (len_dev is None):
        raise ValueError("tm_cls_attention_packed: give the bag lengths either as n (host list) or as len_dev")
    qkv, qL, kL, Z, lse3 = (_f32c(t, nm) for t, nm in ((qkv, "qkv"), (qL, "qL"), (kL, "kL"), (Z, "Z"), (lse3, "lse3")))
    nb, H, M, DH = table.nb, TM_H, TM_M, TM_DH
    if (qkv.dim() != 2 or tuple(qkv.shape) != (table.rows, 3 * TM_D) or tuple(qL.shape) != (nb, H, M, DH)
            or tuple(kL.shape) != (nb, H, M, DH) or tuple(Z.shape) != (nb, H, M, M) or lse3.numel() != nb * H * M):
        raise _lib.MilHipError(f"tm_cls_attention_packed: qkv {tuple(qkv.shape)} / qL {tuple(qL.shape)} / kL {tuple(kL.shape)} / "
                               f"Z {tuple(Z.shape)} / lse3 {tuple(lse3.shape)} outside the built shape for blocks {table.blocks}")
    if any(t.device != qkv.device for t in (qL, kL, Z, lse3, table.dev)):
        raise _lib.MilHipError("tm_cls_attention_packed: qkv, qL, kL, Z, lse3 and the table must be on one device")
    ctab = sides if isinstance(sides, TmClsTable) else tm_cls_table(sides, qkv.device)
    if ctab.dev.device != qkv.device or ctab.nb != nb or any(k != -(-(s * s + 1) // M) for k, s in zip(table.blocks, ctab.sides)):
        raise _lib.MilHipError(f"tm_cls_attention_packed: sides {ctab.sides} do not go with blocks {table.blocks} (256 x blocks = "
                               "ceil((s^2 + 1) / 256) x 256), or their table is on another device")
    if n is not None:
        n = [int(v) for v in n]
        if len(n) != nb or any(not (s - 1) * (s - 1) < v <= s * s for v, s in zip(n, ctab.sides)):
            raise _lib.MilHipError(f"tm_cls_attention_packed: lengths {n} outside the buckets of sides {ctab.sides}")
        len_dev = torch.tensor(n, dtype=torch.int32).to(qkv.device, non_blocking=True)
    elif len_dev.dtype != torch.int32 or len_dev.device != qkv.device or len_dev.numel() < nb or not len_dev.is_contiguous():
        raise _lib.MilHipError(f"tm_cls_attention_packed: len_dev must be contiguous int32 on qkv's device and hold {nb} entries")
    out = torch.empty(H * ctab.patches, device=qkv.device, dtype=torch.float32)
    ws = _ws(_lib.lib().mil_tm_cls_attn_packed_ws_floats(table.total_blocks, nb), qkv)
    _lib.checked().mil_tm_cls_attn_packed(_p(qkv), _p(qL), _p(kL), _p(Z), _p(lse3), _p(ctab.dev), ctab.patches, _p(len_dev), _p(ws),
                                          _p(out), *table.args(), _stream())
    return [out[H * o:H * (o + s * s)].view(H, s * s) for o, s in zip(ctab.off, ctab.sides)]


def _tm_fwd_packed(qkv, tab, w, det=False, pieces=0, cls=None):
    """_tm_fwd_bags with both passes fused, on the packed rows: the phases in the same order, each token-side one a single
    packed launch set; the landmark-side chain (A2, its softmax, the pseudo-inverse, U) exactly as _tm_fwd_bags runs it.
    cls: None, or the keywords of tm_cls_attention_packed (sides and n or len_dev) - the bags' cls attention is then formed from
    qL, kL, Z and lse3 behind U, where _tm_fwd forms it, and returned as the third value (else None)."""
    bg = _tm_bg(det, pieces)
    nb, tb, R = tab.nb, tab.total_blocks, tab.rows
    f32 = dict(device=qkv.device, dtype=torch.float32)
    H, M, DH = TM_H, TM_M, TM_DH
    lib, ck = _lib.lib(), _lib.checked()
    qL, kL, W = (torch.empty((nb, H, M, DH), **f32) for _ in range(3))
    ck.mil_tm_landmarks_packed(_p(qkv), TM_QSCALE, _p(qL), _p(kL), *tab.args(), _stream())
    lse3 = torch.empty((nb, H, M), **f32)
    ws = _ws(lib.mil_tm_lmk_attn_packed_ws_floats(tb, nb, 0), qkv)
    ck.mil_tm_lmk_attn_fwd_packed(_p(qkv), _p(qL), _p(W), _p(lse3), _p(ws), *tab.args(), _stream())
    A2 = tm_softmax_rows(_tm_fwd_a2(qL, kL, torch.empty((nb, H, M, M), **f32), bg, nb * H))
    Z, pinv = _tm_pinv_fwd(A2, det, pieces, nb=nb)
    U = _tm_fwd_u(Z, W, torch.empty((nb, H, M, DH), **f32), bg, nb * H)
    attn = tm_cls_attention_packed(qkv, tab, qL, kL, Z, lse3, **cls) if cls is not None else None
    O = torch.empty((R, TM_D), **f32)
    lse1 = torch.empty((H, R), **f32)
    ck.mil_tm_tok_attn_fwd_packed(_p(qkv), _p(kL), _p(U), _p(O), _p(lse1), None, *tab.args(), _stream())
    ck.mil_tm_resconv_packed(_p(qkv), _p(w), _p(O), *tab.args(), _stream())
    saved = SimpleNamespace(qL=qL, kL=kL, A2=A2, W=W, U=U, Z=Z, pinv=pinv, lse1=lse1, lse3=lse3, det=det, pieces=pieces)
    return O, saved, attn


def _tm_bwd_packed(dO, qkv, tab, w, saved):
    """_tm_bwd_bags with both passes fused, on the packed rows; every column of every dqkv row is written in the order the
    bag-by-bag route writes it (dq, dk | dv, the conv's += on v, the landmarks' += on q and k).  dw is ONE sum over all bags."""
    s = saved
    qL, kL, A2, W, U, Z = s.qL, s.kL, s.A2, s.W, s.U, s.Z
    det, pieces = s.det, s.pieces
    bg = _tm_bg(det, pieces)
    nb, tb, R = tab.nb, tab.total_blocks, tab.rows
    f32 = dict(device=qkv.device, dtype=torch.float32)
    H, M, DH = TM_H, TM_M, TM_DH
    lib, ck = _lib.lib(), _lib.checked()
    dqkv = torch.empty((R, 3 * TM_D), **f32)
    dU, dkL, dqL, dW = (torch.empty((nb, H, M, DH), **f32) for _ in range(4))
    ws = _ws(lib.mil_tm_tok_attn_packed_ws_floats(tb, nb, 1), qkv)
    ck.mil_tm_tok_attn_bwd_packed(_p(qkv), _p(kL), _p(U), _p(s.lse1), _p(dO), _p(dqkv), _p(dU), _p(dkL), _p(ws), *tab.args(),
                                  _stream())
    dZ = torch.empty((nb, H, M, M), **f32)
    _tm_bwd_zw(dU, W, Z, dZ, dW, bg, nb * H)
    ws = _ws(lib.mil_tm_lmk_attn_packed_ws_floats(tb, nb, 1), qkv)
    ck.mil_tm_lmk_attn_bwd_packed(_p(qkv), _p(qL), _p(W), _p(s.lse3), _p(dW), _p(dqkv), _p(dqL), _p(ws), *tab.args(), _stream())
    if det:                                                             # the fold overwrites dw
        dw = torch.empty(H * TM_CONV, **f32)
        ws = _ws(lib.mil_tm_resconv_packed_ws_floats(tb, nb, 1), qkv)
        ck.mil_tm_resconv_bwd_packed_fixed(_p(dO), _p(qkv), _p(w), _p(dqkv), _p(dw), _p(ws), *tab.args(), _stream())
    else:
        dw = torch.zeros(H * TM_CONV, **f32)
        ck.mil_tm_resconv_bwd_packed(_p(dO), _p(qkv), _p(w), _p(dqkv), _p(dw), *tab.args(), _stream())
    dS2 = tm_softmax_rows_bwd(A2, _tm_pinv_bwd(dZ, A2, *s.pinv, det=det, pieces=pieces, nb=nb))
    _tm_bwd_s2(dS2, qL, kL, dkL, dqL, True, bg, nb * H)
    ck.mil_tm_landmarks_bwd_packed(_p(dqL), _p(dkL), TM_QSCALE, _p(dqkv), *tab.args(), _stream())
    return dqkv, dw


class _NystromCorePacked(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, w, tab, det, pieces, cls=None):
        if (qkv.dim() != 2 or qkv.shape[1] != 3 * TM_D or qkv.shape[0] != tab.rows or w.numel() != TM_H * TM_CONV
                or qkv.device != w.device or tab.dev.device != qkv.device):
            raise _lib.MilHipError(f"nystrom_core_packed: qkv {tuple(qkv.shape)} / res_conv {tuple(w.shape)} outside the built shape "
                                   f"for blocks {tab.blocks}, or on two devices")
        qkv = _f32c(qkv, "qkv")
        w = _f32c(w, "res_conv.weight")
        O, saved, attn = _tm_fwd_packed(qkv, tab, w, det, pieces, cls)
        ctx.saved, ctx.tab = saved, tab
        ctx.save_for_backward(qkv, w)
        ctx.w_shape = w.shape
        if attn is None:
            return O
        ctx.mark_non_differentiable(*attn)                  # the bags' views of one buffer, formed from the saved operands
        return (O, *attn)

    @staticmethod
    def backward(ctx, dO, *_dattn):
        qkv, w = ctx.saved_tensors
        dqkv, dw = _tm_bwd_packed(_f32c(dO, "dO"), qkv, ctx.tab, w, ctx.saved)
        ctx.saved = None
        return dqkv, dw.reshape(ctx.w_shape), None, None, None, None


def nystrom_core_packed(qkv, blocks_or_table, w, *, deterministic=None, pieces=None, need_attn=False, cls=None):
    """nystrom_core (need_attn False or "cls") for all bags of a step over ONE packed sequence: qkv [256 sum(blocks), 1536] = the bags'
    to_qkv rows of their front-zero-padded LayerNorm output one after another, bag b 256 blocks[b] rows; blocks_or_table = the
    per-bag block counts (the table is then built here: a host-to-device copy, not for a capture) or a TmPackedTable
    (tm_packed_table); w = res_conv.weight -> out [256 sum(blocks), 512], bag b's rows where its input rows are.
    The landmarks, the landmark-query pass, the token-query pass, the residual conv and their backwards are one packed launch
    set each (mil_tm_*_packed), whatever the number of bags; the landmark-side chain runs as in nystrom_core_bags on buffers
    stacked [nb, 8, 256, .].  Both passes always run fused: no A1 or A3 map exists on this route, and no attention output.
    Every bag's rows of out and (deterministic) of dqkv are bit-equal to nystrom_core_bags with both fused switches on; dw is
    one sum over all bags' 256-row chunks - atomic, or with deterministic in ascending packed order.
    deterministic, pieces: as in nystrom_core; they apply to the chain unchanged.  No host read; every workspace is a
    torch.empty, so with a TmPackedTable the call can be captured into a graph.  tm_route says which steps come here.
    need_attn: False -> out alone, as above.  "cls" -> (out, [attn_b]): the cls token's per-patch attention of every bag, [8, s_b^2]
    each with zeros from the bag's length on, all views of one buffer (tm_cls_attention_packed: one launch set for all bags);
    cls = dict(sides=.., n=[..]) with host lengths (validated and uploaded: not for a capture) or dict(sides=.., len_dev=..)
    with the lengths on the device, sides the grid sides or a TmClsTable.  The attention is formed in the forward from qL, kL, Z
    and lse3, behind U; it carries no gradient and the backward is the one of need_attn False, so out and dqkv keep their bits.
    True raises ValueError: the whole [8, n_pad, n_pad] map has no packed form."""
    if not (need_attn is False or (isinstance(need_attn, str) and need_attn == "cls")):
        raise ValueError(f"nystrom_core_packed: need_attn must be False or 'cls' (the whole map has no packed form), got {need_attn!r}")
    tab = blocks_or_table if isinstance(blocks_or_table, TmPackedTable) else tm_packed_table(blocks_or_table, qkv.device)
    if need_attn is False:
        return _NystromCorePacked.apply(qkv, w, tab, tm_deterministic(deterministic), tm_pieces(pieces))
    if not isinstance(cls, dict) or "sides" not in cls or (cls.get("n") is None) == (cls.get("len_dev") is None):
        raise ValueError("nystrom_core_packed: need_attn='cls' needs cls=dict(sides=.., n=[..]) or dict(sides=.., len_dev=..)")
    cls = dict(sides=cls["sides"], n=cls.get("n"), len_dev=cls.get("len_dev"))
    O, *attn = _NystromCorePacked.apply(qkv, w, tab, tm_deterministic(deterministic), tm_pieces(pieces), cls)
    return O, attn


# ---- PPEG of a step's bags in one launch set (csrc/tm_ppeg_packed.h): the unpadded sequences, one bag after another
class TmPpegTable:
    """The table of the mil_tm_ppeg_*_packed entries for bags of grid sides `sides` (host ints): `dev`, int32
    [4 nb + 3 + gmax + cmax] on the device (tm_ppeg_table_host has the layout); `rows` = sum (1 + s^2), the packed sequence rows;
    `chunks` = sum ceil(s / 8), what sizes the fixed-order workspace.  Build it with tm_ppeg_table, outside any capture; it
    depends on the bags' sides alone."""

    def __init__(self, sides, dev):
        self.sides = tuple(int(s) for s in sides)
        self.nb, self.dev = len(self.sides), dev
        self.rows = sum(1 + s * s for s in self.sides)
        self.chunks = sum(-(-s // 8) for s in self.sides)

    def args(self):
        return _p(self.dev), self.nb, self.rows


def tm_ppeg_table_host(sides):
    """The table's int32 values as a list, for R = sum (1 + s^2) rows, gmax = isqrt(nb (R - nb)) >= sum s and
    cmax = min(gmax, (gmax + 7 nb) // 8) >= sum ceil(s / 8) (both follow from (nb, R) alone, as the launch shapes do):
    row_off [nb + 1] | side [nb] | grow_off [nb + 1] | chunk_off [nb + 1] | bag_of_gridrow [gmax] | bag_of_chunk [cmax], the
    last two -1 behind the bags' grid rows and chunks."""
    sides = [int(s) for s in sides]
    if not 1 <= len(sides) <= TM_MAX_BATCH_BAGS or min(sides) < 1 or sum(1 + s * s for s in sides) > (2 ** 31 - 1) // TM_D:
        raise ValueError(f"tm_ppeg_table: 1 .. {TM_MAX_BATCH_BAGS} bags of side >= 1, at most {(2 ** 31 - 1) // TM_D} rows, got {sides}")
    nb = len(sides)
    row, grow, chunk = [0], [0], [0]
    for s in sides:
        row.append(row[-1] + 1 + s * s)
        grow.append(grow[-1] + s)
        chunk.append(chunk[-1] + -(-s // 8))
    gmax = math.isqrt(nb * (row[-1] - nb))
    cmax = min(gmax, (gmax + 7 * nb) // 8)
    bag_g = [b for b, s in enumerate(sides) for _ in range(s)]
    bag_c = [b for b, s in enumerate(sides) for _ in range(-(-s // 8))]
    return row + sides + grow + chunk + bag_g + [-1] * (gmax - len(bag_g)) + bag_c + [-1] * (cmax - len(bag_c))


def tm_ppeg_table(sides, device=None) -> TmPpegTable:
    """sides: per bag the grid side -> the TmPpegTable on `device` (_tm_table_dev)."""
    return TmPpegTable(sides, _tm_table_dev(tm_ppeg_table_host(sides), device))


class _TmPPEGPacked(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, tab, W7, b7, W5, b5, W3, b3, deterministic=False):
        if x.dim() != 2 or x.shape[1] != TM_D or x.shape[0] != tab.rows or tab.dev.device != x.device:
            raise _lib.MilHipError(f"tm_ppeg_packed: x {tuple(x.shape)} outside the built shape [{tab.rows}, {TM_D}] for sides "
                                   f"{tab.sides}, or on two devices")
        x = _f32c(x, "x")
        W7, W5, W3 = _f32c(W7, "W7"), _f32c(W5, "W5"), _f32c(W3, "W3")
        y = torch.empty_like(x)
        _lib.checked().mil_tm_ppeg_fwd_packed(_p(x), _p(W7), _p(_f32c(b7, "b7")), _p(W5), _p(_f32c(b5, "b5")), _p(W3),
                                              _p(_f32c(b3, "b3")), _p(y), *tab.args(), _stream())
        ctx.save_for_backward(x, W7, W5, W3)
        ctx.tab, ctx.deterministic = tab, deterministic
        return y

    @staticmethod
    def backward(ctx, dy):
        x, W7, W5, W3 = ctx.saved_tensors
        tab = ctx.tab
        dy = _f32c(dy, "dy")
        dx = torch.empty_like(x)
        if ctx.deterministic:       # the fold overwrites dWf and db
            dWf = torch.empty((TM_D, 1, 7, 7), device=x.device, dtype=torch.float32)
            db = torch.empty(TM_D, device=x.device, dtype=torch.float32)
            ws = _ws(_lib.lib().mil_tm_ppeg_packed_ws_floats(tab.chunks), x)
            _lib.checked().mil_tm_ppeg_bwd_packed_fixed(_p(dy), _p(x), _p(W7), _p(W5), _p(W3), _p(dx), _p(dWf), _p(db), _p(ws),
                                                        *tab.args(), _stream())
        else:
            dWf = torch.zeros((TM_D, 1, 7, 7), device=x.device, dtype=torch.float32)
            db = torch.zeros(TM_D, device=x.device, dtype=torch.float32)
            _lib.checked().mil_tm_ppeg_bwd_packed(_p(dy), _p(x), _p(W7), _p(W5), _p(W3), _p(dx), _p(dWf), _p(db), *tab.args(),
                                                  _stream())
        # as _TmPPEG: dW7 is the whole map, dW5 / dW3 its central 5 x 5 / 3 x 3; the three biases share db
        return (dx, None, dWf, db, dWf[:, :, 1:6, 1:6].contiguous(), db.clone(), dWf[:, :, 2:5, 2:5].contiguous(), db.clone(), None)


def tm_ppeg_packed(x, table, W7, b7, W5, b5, W3, b3, deterministic=None):
    """tm_ppeg for all bags of a step in ONE launch set: x [sum (1 + s_b^2), 512] = the bags' sequences one after another,
    table = a TmPpegTable (tm_ppeg_table) or the tuple of sides (the table is then built here: a host-to-device copy, not for a
    capture).  Every bag's rows of the result and of dx are bit-equal to tm_ppeg on that bag's slice; the weight and bias
    gradients are ONE sum over all bags' 8-grid-row chunks - atomic, or with deterministic in ascending packed order
    (mil_tm_ppeg_bwd_packed_fixed) -, where the per-bag route lets autograd add per-bag totals.  No host read; the workspace is a
    torch.empty, so with a TmPpegTable the call can be captured into a graph."""
    tab = table if isinstance(table, TmPpegTable) else tm_ppeg_table(table, x.device)
    return _TmPPEGPacked.apply(x, tab, W7, b7, W5, b5, W3, b3, tm_deterministic(deterministic))
