"""LayerNorm variants, row append, positional encodings, CT map and CLIP token embedding (csrc/attention.hip)."""
from __future__ import annotations

import torch

from .. import _lib
from ._base import _f32c, _p, _stream, _stream_int, grad_slot


def _tail_view(base, rows: int):
    """The `rows` rows reserved BEHIND `base` in its storage (layer_norm(..., tail_rows=rows) allocated them), or None."""
    if base is None or base.dim() != 2 or not base.is_contiguous() or base.storage_offset() != 0 or base.dtype != torch.float32:
        return None
    R, E = base.shape
    st = base.untyped_storage()
    if st.nbytes() != (R + rows) * E * 4:
        return None
    return torch.empty(0, device=base.device, dtype=torch.float32).set_(st, R * E, (rows, E), (E, 1))


class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps: float, tail_rows: int = 0, into_tail_of=None):
        x = _f32c(x, "x")
        rows, E = x.shape
        # tail_rows > 0: allocate room for that many more rows behind the result (see append_rows)
        y = torch.empty((rows + tail_rows, E), device=x.device, dtype=torch.float32)[:rows] if tail_rows else None
        if y is None and into_tail_of is not None:
            # the result IS the block another tensor reserved behind itself (the text tokens of the multi-modal bag,
            # model/aggregator.py:192): written in place there, append_rows then has nothing to copy
            y = _tail_view(into_tail_of.detach(), rows) if into_tail_of.shape[1] == E else None
        if y is None:
            y = torch.empty_like(x)
        stats = torch.empty((rows, 2), device=x.device, dtype=torch.float32)
        sh = _lib.shim()
        if sh is not None:
            sh.layernorm_fwd(x, _f32c(gamma, "gamma"), _f32c(beta, "beta"), eps, y, stats, _stream_int())
        else:
            _lib.checked().mil_layernorm_fwd(_p(x), _p(_f32c(gamma, "gamma")), _p(_f32c(beta, "beta")), rows, E, eps, _p(y),
                                             _p(stats), _stream())
        ctx.save_for_backward(x, gamma, stats)
        ctx.beta_param = beta               # only to look up its flat-gradient slot in backward
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, stats = ctx.saved_tensors
        dx, dg, db = _layer_norm_bwd(x, gamma, stats, dy, None, ctx.needs_input_grad[1] or ctx.needs_input_grad[2],
                                     ctx.beta_param)
        return dx, dg, db, None, None, None


def _layer_norm_bwd(x, gamma, stats, dy, dres, want_params: bool, beta=None):
    """dx (+ dres), dgamma, dbeta of a LayerNorm; frozen parameters skip their sums (and the two column-sum launches)."""
    rows, E = x.shape
    dy = _f32c(dy, "dy")
    dx = torch.empty_like(x)
    dg = db = ws = None
    if want_params:
        dg = grad_slot(gamma)
        if dg is None:
            dg = torch.empty(E, device=x.device, dtype=torch.float32)
        db = grad_slot(beta) if beta is not None else None
        if db is None:
            db = torch.empty(E, device=x.device, dtype=torch.float32)
        ws = torch.empty(_lib.lib().mil_layernorm_bwd_blocks(rows) * 2 * E, device=x.device, dtype=torch.float32)
    sh = _lib.shim()
    if sh is not None:
        sh.layernorm_bwd_res(x, gamma, dy, stats, dres, dx, dg, db, ws, _stream_int())
        return dx, dg, db
    _lib.checked().mil_layernorm_bwd_res(_p(x), _p(gamma), _p(dy), _p(stats), _p(dres), rows, E, _p(dx), _p(dg), _p(db),
                                         _p(ws), _stream())
    return dx, dg, db


class _LayerNormRes(torch.autograd.Function):
    """LayerNorm that also hands back its input (an alias): a pre-norm residual block x + f(LN(x)) (clip/model.py:183-199)
    passes THAT to the residual add, so the gradient of the residual branch arrives at this node and is added inside the
    backward kernel instead of by an elementwise launch of autograd."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps: float):
        x_in = x
        x = _f32c(x, "x")
        rows, E = x.shape
        y = torch.empty_like(x)
        stats = torch.empty((rows, 2), device=x.device, dtype=torch.float32)
        _lib.checked().mil_layernorm_fwd(_p(x), _p(_f32c(gamma, "gamma")), _p(_f32c(beta, "beta")), rows, E, eps, _p(y),
                                         _p(stats), _stream())
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, gamma, stats)
        return y, x_in.view_as(x_in)

    @staticmethod
    def backward(ctx, dy, dres):
        if dy is None:
            return dres, None, None, None
        x, gamma, stats = ctx.saved_tensors
        dres = _f32c(dres, "dres") if dres is not None else None
        dx, dg, db = _layer_norm_bwd(x, gamma, stats, dy, dres, ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
        return dx, dg, db, None


def layer_norm_res(x, gamma, beta, eps: float = 1e-5):
    """(LayerNorm(x), x) for a 2-D x - use the returned x for the residual add that skips the norm."""
    return _LayerNormRes.apply(x, gamma, beta, eps)


class _LayerNormBagRow(torch.autograd.Function):
    """LayerNorm(x + o[bag of row]) as one node (mil_layernorm_bagrow_fwd/_bwd): the sum is never materialised, and the
    backward returns dx, the per-bag sums d_o, dgamma and dbeta from one pass + one fold launch."""

    @staticmethod
    def forward(ctx, x, o, gamma, beta, eps: float, segs, tail_rows: int):
        x, o = _f32c(x, "x"), _f32c(o, "o")
        rows, E = x.shape
        y = torch.empty((rows + tail_rows, E), device=x.device, dtype=torch.float32)[:rows] if tail_rows else torch.empty_like(x)
        stats = torch.empty((rows, 2), device=x.device, dtype=torch.float32)
        _lib.checked().mil_layernorm_bagrow_fwd(_p(x), _p(o), _p(segs.q_bag), _p(_f32c(gamma, "gamma")), _p(_f32c(beta, "beta")),
                                                rows, E, eps, _p(y), _p(stats), _stream())
        ctx.segs = segs
        ctx.beta_param = beta
        ctx.save_for_backward(x, o, gamma, stats)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, o, gamma, stats = ctx.saved_tensors
        segs = ctx.segs
        dy = _f32c(dy, "dy")
        rows, E = x.shape
        dx = torch.empty_like(x)
        do = torch.empty_like(o)
        dg = grad_slot(gamma)
        if dg is None:
            dg = torch.empty(E, device=x.device, dtype=torch.float32)
        db = grad_slot(ctx.beta_param)
        if db is None:
            db = torch.empty(E, device=x.device, dtype=torch.float32)
        ws = torch.empty(_lib.lib().mil_layernorm_bwd_blocks(rows) * 4 * E, device=x.device, dtype=torch.float32)
        _lib.checked().mil_layernorm_bagrow_bwd(_p(x), _p(o), _p(segs.q_bag), _p(segs.q_off), segs.B, _p(gamma), _p(dy),
                                                _p(stats), rows, E, _p(dx), _p(do), _p(dg), _p(db), _p(ws), _stream())
        return dx, do, dg, db, None, None, None


def layer_norm_bag_row(x, o, segs, gamma, beta, eps: float = 1e-5, tail_rows: int = 0):
    """LayerNorm(x + o[bag of row]) for x [rows, E], o [B, E]; segs: AttnSegs whose QUERY side are the rows of x.  Fused
    when every bag is at least one backward workgroup's row range long (see mil_layernorm_bagrow_bwd) and the norm is
    trainable; otherwise add_bag_row followed by layer_norm."""
    rows = x.shape[0]
    # device-side lengths (segments.FusionBucket): set_lengths() has checked every bag against the block's row range
    ok = (x.dim() == 2 and rows > 64 and gamma.requires_grad == beta.requires_grad and
          (getattr(segs, "device_lengths", False) or
           min(segs.q_lengths, default=0) >= _lib.lib().mil_layernorm_bagrow_rows_per_block(rows)))
    if not ok:
        return layer_norm(add_bag_row(x, o, segs), gamma, beta, eps, tail_rows)
    return _LayerNormBagRow.apply(x, o, gamma, beta, eps, segs, tail_rows)


def layer_norm(x, gamma, beta, eps: float = 1e-5, tail_rows: int = 0, into_tail_of=None):
    lead = x.shape[:-1]
    return _LayerNorm.apply(x.reshape(-1, x.shape[-1]), gamma, beta, eps, tail_rows, into_tail_of).reshape(*lead, x.shape[-1])


class _AppendRows(torch.autograd.Function):
    """torch.cat([base, extra], 0) that does not copy `base` when it was allocated with room behind it
    (layer_norm(..., tail_rows=extra.shape[0])): only the few `extra` rows are written.  Used for the multi-modal
    bag of model/aggregator.py:192 - the [N, 512] patch tokens stay where the last LayerNorm put them."""

    @staticmethod
    def forward(ctx, base, extra, tail_reserved: bool):
        R, E = base.shape
        T = extra.shape[0]
        ctx.R = R
        st = base.untyped_storage()
        # tail_reserved is the CALLER's statement that the rows behind `base` were reserved for this purpose
        # (layer_norm(..., tail_rows=T)); without it a prefix view of somebody else's buffer would qualify too.
        if (tail_reserved and base.is_contiguous() and base.storage_offset() == 0 and base.dtype == torch.float32
                and st.nbytes() == (R + T) * E * 4):
            big = torch.empty(0, device=base.device, dtype=torch.float32).set_(st, 0, (R + T, E), (E, 1))
            if not (extra.is_contiguous() and extra.dtype == torch.float32 and extra.data_ptr() == base.data_ptr() + R * E * 4):
                big[R:].copy_(extra)          # (else: the producer already wrote them there - layer_norm(into_tail_of=base))
            return big
        return torch.cat([base, extra], 0)

    @staticmethod
    def backward(ctx, g):
        return g[:ctx.R], g[ctx.R:], None


def append_rows(base, extra, tail_reserved: bool = False):
    """torch.cat([base, extra], 0); with tail_reserved=True and `base` allocated by layer_norm(..., tail_rows=len(extra))
    the base rows are not copied."""
    return _AppendRows.apply(base, extra, tail_reserved)


class _AddPE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pe, row_bag, row_off):
        x = _f32c(x, "x")
        rows, E = x.shape
        out = torch.empty_like(x)
        _lib.checked().mil_add_pe(_p(x), _p(pe), _p(row_bag), _p(row_off), rows, E, _p(out), _stream())
        ctx.set_materialize_grads(False)      # an unused keys + pe must not send a [rows, E] tensor of zeros upstream
        return out

    @staticmethod
    def backward(ctx, g):
        return g, None, None, None


def add_pe(x, pe, row_bag, row_off):
    """x[row] + pe[position of the row inside its bag]."""
    return _AddPE.apply(x, pe, row_bag, row_off)


class _AddBagRow(torch.autograd.Function):
    """x[row] + o[bag of row]  (one-text-token fast path of the image->token attention)."""

    @staticmethod
    def forward(ctx, x, o, segs):
        x, o = _f32c(x, "x"), _f32c(o, "o")
        rows, E = x.shape
        out = torch.empty_like(x)
        _lib.checked().mil_add_bag_row(_p(x), _p(o), _p(segs.q_bag), rows, E, _p(out), _stream())
        ctx.segs = segs
        return out

    @staticmethod
    def backward(ctx, g):
        segs = ctx.segs
        g = _f32c(g, "g")
        rows, E = g.shape
        do = torch.empty((segs.B, E), device=g.device, dtype=torch.float32)
        nch = (segs.Tq_max + 255) // 256
        ws = torch.empty(nch * segs.B * E, device=g.device, dtype=torch.float32) if nch > 1 else None
        _lib.checked().mil_segment_colsum(_p(g), _p(segs.q_off), segs.B, segs.Tq_max, E, _p(do), _p(ws), _stream())
        return g, do, None


def add_bag_row(x, o, segs):
    """segs: AttnSegs whose QUERY side are the rows of x (q_bag / q_off)."""
    return _AddBagRow.apply(x, o, segs)


def ct_map_tokens(ct, model_CT: str = "resnetMC3_18"):
    """CT feature map [B, C, D, h, w] -> flat token rows [B * T, C] (sam/transformer.py:86-98): T = D tokens by a mean over
    (h, w) for resnetMC3_18, T = D * h * w by flatten + permute for medicalNet.  The map is an input (the CT encoders are
    outside the hot path), so no gradient flows into it."""
    if ct.dim() != 5:
        raise _lib.MilHipError("ct_map_tokens: expected a 5-D map [B, C, D, h, w]")
    if ct.requires_grad:
        raise NotImplementedError("the CT encoder is outside the MIL hot path: pass its output detached")
    ct = _f32c(ct, "ct")
    B, C, D, hh, ww = ct.shape
    reduce = 0 if model_CT == "medicalNet" else 1
    T = D if reduce else D * hh * ww
    out = torch.empty((B * T, C), device=ct.device, dtype=torch.float32)
    _lib.checked().mil_ct_map_tokens(_p(ct), B, C, D, hh * ww, reduce, _p(out), _stream())
    return out, T


def sinusoid_pe(n: int, E: int, device):
    pe = torch.empty((n, E), device=device, dtype=torch.float32)
    _lib.checked().mil_sinusoid_pe(_p(pe), n, E, _stream())
    return pe


# --------------------------------------------------------------------------- K4: CLIP text front/back ends
def embed_tokens(ids, table, pos):
    """token_embedding[ids] + positional_embedding  ->  [nseq * ctx, W]  (clip/model.py:340-342)."""
    nseq, ctx = ids.shape
    W = table.shape[1]
    if ids.dtype != torch.int64 or not ids.is_cuda:
        raise _lib.MilHipError("embed_tokens: ids must be int64 on the GPU")
    out = torch.empty((nseq * ctx, W), device=ids.device, dtype=torch.float32)
    _lib.checked().mil_embed_tokens(_p(ids.contiguous()), _p(_f32c(table, "table")), _p(_f32c(pos, "pos")), nseq, ctx, W,
                                    _p(out), _stream())
    return out


def gather_eot(ids, x):
    """Rows of x [nseq*ctx, W] at each sequence's EOT position (argmax of the ids)."""
    nseq, ctx = ids.shape
    W = x.shape[1]
    out = torch.empty((nseq, W), device=x.device, dtype=torch.float32)
    _lib.checked().mil_gather_eot(_p(ids.contiguous()), _p(_f32c(x, "x")), nseq, ctx, W, _p(out), _stream())
    return out
