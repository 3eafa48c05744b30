"""One-text-token token->image attention with the projections absorbed (csrc/absorbed_attn.hip)."""
from __future__ import annotations

import torch

from .. import _lib
from ._base import _f32c, _p, _stream, _stream_int, grad_slot
from .linear import SMALL_ROWS, colsum, linear_act


# A list while a model collects what its token->image sites hold (model.note_attn; note_sites() below), None otherwise: the
# forwards of the pool nodes append one record per site - tensors they have formed anyway, no launch is added or changed.
_site_tap = None


class note_sites:
    """with note_sites() as sites: every absorbed one-token pool (and multi-token pool, ops/grouped.py) that runs inside
    appends dict(keys, pe, Qp, lse, segs, C) (multi-token: dict(A, segs, TH), A the softmaxed score matrix) to `sites`, in the
    order the sites run.  absorbed_pool_attention() turns a record into the softmax weights afterwards."""

    def __enter__(self):
        global _site_tap
        self._outer, _site_tap = _site_tap, []
        return _site_tap

    def __exit__(self, *exc):
        global _site_tap
        _site_tap = self._outer
        return False


def _note_site(keys, pe, Qp, lse, segs, C):
    if _site_tap is not None:
        _site_tap.append(dict(keys=keys, pe=pe, Qp=Qp, lse=lse, segs=segs, C=C))


def absorbed_pool_attention(keys, pe, Qp, lse, segs, C: int):
    """The softmax weights of the one-token pool, attn [n_keys, 8] with attn[n][h] = exp(Qp[b][h] . (keys_n + pe_n) / sqrt(C) -
    lse[b][h]) (mil_absorbed_pool_attn: one pass over the keys).  keys, pe, Qp, lse: what the forward read and wrote (for the
    fused LayerNorm sites keys = the y it wrote).  Bag b's heads x patches view is attn[k_off[b]:k_off[b + 1]].t().  Rows of a
    capacity bucket behind the bags read 0.  No gradient."""
    keys, pe, Qp, lse = (_f32c(t.detach(), n) for t, n in ((keys, "keys"), (pe, "pe"), (Qp, "Qp"), (lse, "lse")))
    B, H, E = Qp.shape
    if keys.dim() != 2 or keys.shape[1] != E or lse.shape != (B, H):
        raise ValueError("absorbed_pool_attention: keys [n_keys, E], Qp [B, H, E], lse [B, H]")
    covered = not getattr(segs, "device_lengths", False) or getattr(segs, "pad_tiles", False)
    attn = (torch.empty if covered else torch.zeros)((keys.shape[0], H), device=keys.device, dtype=torch.float32)
    _lib.checked().mil_absorbed_pool_attn(_p(keys), _p(pe), _p(Qp), _p(lse), _p(segs.k_off), _p(segs.tile_map), segs.ntiles,
                                          B, H, C, E, _p(attn), _stream())
    return attn


class _AbsorbQuery(torch.autograd.Function):
    """Qp[b][h] = scale * Wk_h^T qp[b][h]  (also the value projection's backward map).  T > 1: the B = bags x T rows are
    the T text tokens of each bag and the result is the grouped products' operand [bags, T H padded to a multiple of 32, E]
    with zero rows behind (written by the same launch: include/mil_hip.h mil_absorb_query_pad).  With `bias` [H C] a second
    result cb [bags, THp] = scale * bias_h . qp[b][h] (the score column constant of the other projection's bias)."""

    @staticmethod
    def forward(ctx, qp, Wk, H: int, T: int = 1, scale: float = 1.0, bias=None):
        qp, Wk = _f32c(qp, "qp"), _f32c(Wk, "Wk")
        B, I = qp.shape
        E = Wk.shape[1]
        THp = H if T == 1 else T * H + (-T * H) % 32
        Qp = torch.empty((B, H, E) if T == 1 else (B // T, THp, E), device=qp.device, dtype=torch.float32)
        cb = None
        if bias is not None:
            bias = _f32c(bias, "bias")
            cb = torch.empty((B // T, THp), device=qp.device, dtype=torch.float32)
        sh = _lib.shim() if T == 1 and scale == 1.0 and bias is None else None
        if sh is not None:
            sh.absorb_query(qp, Wk, H, Qp, _stream_int())
        else:
            _lib.checked().mil_absorb_query_pad(_p(qp), _p(Wk), B, H, I // H, E, T, THp, scale, _p(bias), _p(Qp), _p(cb),
                                                _stream())
        ctx.H, ctx.T, ctx.THp, ctx.scale = H, T, THp, scale
        ctx.with_bias = bias is not None
        if bias is None:
            ctx.save_for_backward(qp, Wk)
            return Qp
        ctx.save_for_backward(qp, Wk, bias)
        return Qp, cb

    @staticmethod
    def backward(ctx, dQp, dcb=None):
        qp, Wk = ctx.saved_tensors[:2]
        bias = ctx.saved_tensors[2] if ctx.with_bias else None
        B, I = qp.shape
        E = Wk.shape[1]
        dQp = _f32c(dQp, "dQp")
        dqp = torch.empty_like(qp) if ctx.needs_input_grad[0] else None
        dWk = None
        if ctx.needs_input_grad[1]:
            dWk = grad_slot(Wk)                       # straight into optim.FlatAdam's flat gradient buffer when there is one
            if dWk is None:
                dWk = torch.empty_like(Wk)
        sh = _lib.shim() if ctx.T == 1 and ctx.scale == 1.0 and bias is None else None
        if sh is not None:
            sh.absorb_query_bwd(qp, Wk, dQp, ctx.H, dqp, dWk, _stream_int())
            return dqp, dWk, None, None, None, None
        dbias = None
        if bias is not None:
            dcb = _f32c(dcb, "dcb")
            if ctx.needs_input_grad[5] and dWk is not None:
                dbias = grad_slot(bias)
                if dbias is None:
                    dbias = torch.empty_like(bias)
        _lib.checked().mil_absorb_query_bwd_pad(_p(qp), _p(Wk), _p(dQp), B, ctx.H, I // ctx.H, E, ctx.T, ctx.THp, ctx.scale,
                                                _p(bias), _p(dcb) if bias is not None else None, _p(dqp), _p(dWk), _p(dbias),
                                                _stream())
        if bias is not None and ctx.needs_input_grad[5] and dbias is None:      # frozen weight, trainable bias: not a model case
            dbias = (qp.view(B, ctx.H, -1) * dcb.view(-1, ctx.THp)[:, :ctx.T * ctx.H].reshape(B, ctx.H, 1)).sum(0).reshape(-1) * ctx.scale
        return dqp, dWk, None, None, None, dbias


def _dkeys_buffer(keys, segs):
    """Gradient buffer of the keys for the absorbed pool's backward.  Capacity bucket (segments.FusionBucket): padding rows
    must hand ZERO upstream (their gradient feeds LayerNorm / bias sums of the layer below) - the bucket's padding tiles
    make the apply pass write those zeros itself; a device-length layout without them gets a cleared buffer."""
    if getattr(segs, "device_lengths", False) and not getattr(segs, "pad_tiles", False):
        return torch.zeros_like(keys)
    return torch.empty_like(keys)


class _AbsorbedPool(torch.autograd.Function):
    """pooled[b][h] = sum_n softmax_n(Qp[b][h] . (keys_n + pe_n) / sqrt(C)) keys_n.
    Also returns the keys unchanged (an alias): the caller hands THAT to the keys' other consumer, so both gradients
    of the keys arrive at this node and the backward folds them in one pass instead of autograd adding two [N, 512]
    tensors."""

    @staticmethod
    def forward(ctx, keys, pe, Qp, segs, C: int):
        keys_in = keys
        keys, pe, Qp = _f32c(keys, "keys"), _f32c(pe, "pe"), _f32c(Qp, "Qp")
        B, H, E = Qp.shape
        pooled = torch.empty_like(Qp)
        lse = torch.empty((B, H), device=keys.device, dtype=torch.float32)
        ws = torch.empty(max(1, segs.ntiles) * H * (E + 2), device=keys.device, dtype=torch.float32)
        _lib.checked().mil_absorbed_pool_fwd(_p(keys), _p(pe), _p(Qp), _p(segs.k_off), _p(segs.tile_map),
                                             _p(segs.bag_tile_off), segs.ntiles, B, H, C, E, _p(pooled), _p(lse), _p(ws),
                                             _stream())
        ctx.segs, ctx.C = segs, C
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(keys, pe, Qp, pooled, lse)
        _note_site(keys, pe, Qp, lse, segs, C)
        return pooled, keys_in.view_as(keys_in)

    @staticmethod
    def backward(ctx, dpooled, dkeys_pass):
        keys, pe, Qp, pooled, lse = ctx.saved_tensors
        segs, C = ctx.segs, ctx.C
        B, H, E = Qp.shape
        if dpooled is None:
            return dkeys_pass, None, None, None, None
        dpooled = _f32c(dpooled, "dpooled")
        acc = _f32c(dkeys_pass, "dkeys") if dkeys_pass is not None else None
        dkeys = _dkeys_buffer(keys, segs)
        dQp = torch.empty_like(Qp)
        n_keys = keys.shape[0]
        ws = torch.empty(max(1, segs.ntiles) * H * E + 16 * n_keys, device=keys.device, dtype=torch.float32)
        _lib.checked().mil_absorbed_pool_bwd(_p(keys), _p(pe), _p(Qp), _p(lse), _p(dpooled), _p(pooled), _p(segs.k_off),
                                             _p(segs.tile_map), _p(segs.bag_tile_off), segs.ntiles, n_keys, B, H, C, E,
                                             _p(acc), _p(dkeys), _p(dQp), _p(ws), _stream())
        return dkeys, None, dQp, None, None


class _ValueProj(torch.autograd.Function):
    """o[b][hC + c] = Wv[hC + c] . pooled[b][h] + bv[hC + c].  T > 1: pooled is the multi-token pool's result as it stands,
    [bags, T H padded to a multiple of 32, E] (row t H + h of a bag; b = bag x T + t), and its gradient comes back in that
    layout with zero padding rows - no slice / pad copies around the node."""

    @staticmethod
    def forward(ctx, pooled, Wv, bv, H: int, T: int = 1):
        pooled, Wv = _f32c(pooled, "pooled"), _f32c(Wv, "Wv")
        E = pooled.shape[-1]
        I = Wv.shape[0]
        THp = pooled.shape[1]
        B = pooled.shape[0] * T
        if T == 1 and THp != H:
            raise ValueError("pooled must be [B, H, E]")
        o = torch.empty((B, I), device=pooled.device, dtype=torch.float32)
        _lib.checked().mil_value_proj_pad(_p(pooled), _p(Wv), _p(_f32c(bv, "bv")), B, H, I // H, E, T, THp, _p(o), _stream())
        ctx.save_for_backward(pooled, Wv)
        ctx.bv_param = bv                   # only to look up its flat-gradient slot in backward
        ctx.H, ctx.T = H, T
        return o

    @staticmethod
    def backward(ctx, do):
        pooled, Wv = ctx.saved_tensors
        dpooled, dWv, dbv = _value_proj_bwd(_f32c(do, "do"), Wv, ctx.bv_param, pooled, ctx.H, ctx.T)
        return dpooled, dWv, dbv, None, None


def _value_proj_bwd(do, Wv, bv, pooled, H: int = 0, T: int = 1):
    """(dpooled, dWv, dbv) of o = Wv pooled + bv in ONE launch (mil_value_proj_bwd); parameter gradients go straight into
    their flat-buffer slots when there are any."""
    E = pooled.shape[-1]
    H = H or pooled.shape[1]
    THp = pooled.shape[1]
    B = pooled.shape[0] * T
    I = Wv.shape[0]
    dpooled = torch.empty_like(pooled)
    dWv = grad_slot(Wv)
    if dWv is None:
        dWv = torch.empty_like(Wv)
    dbv = grad_slot(bv)
    if dbv is None:
        dbv = torch.empty(I, device=do.device, dtype=torch.float32)
    if E != 512 or B > SMALL_ROWS or T > 1:
        # many rows (T text tokens per bag: B = bags x T): the one-launch form walks the rows of its bias role in turn
        _lib.checked().mil_absorb_query_pad(_p(do), _p(Wv), B, H, I // H, E, T, THp, 1.0, None, _p(dpooled), None, _stream())
        _lib.checked().mil_absorb_query_bwd_pad(_p(do), _p(Wv), _p(pooled), B, H, I // H, E, T, THp, 1.0, None, None, None,
                                                _p(dWv), None, _stream())
        return dpooled, dWv, colsum(do, out=dbv)
    sh = _lib.shim()
    if sh is not None:
        sh.value_proj_bwd(do, Wv, pooled, dpooled, dWv, dbv, _stream_int())
        return dpooled, dWv, dbv
    _lib.checked().mil_value_proj_bwd(_p(do), _p(Wv), _p(pooled), B, H, I // H, E, _p(dpooled), _p(dWv), _p(dbv), _stream())
    return dpooled, dWv, dbv


class _AbsorbedPoolValue(torch.autograd.Function):
    """_AbsorbedPool followed by _ValueProj as ONE node: o[b] = Wv pooled[b] + bv comes out of the pool's merge launch
    (mil_absorbed_pool_value_fwd) and the backward is four launches - value projection backward (dpooled, dWv, dbv), the
    per-row dots (which form the softmax constant themselves), the apply pass, the merge - where the two nodes took eight.
    Returns (o [B, H C], keys alias)."""

    @staticmethod
    def forward(ctx, keys, pe, Qp, Wv, bv, segs, C: int):
        keys_in = keys
        keys, pe, Qp, Wv = _f32c(keys, "keys"), _f32c(pe, "pe"), _f32c(Qp, "Qp"), _f32c(Wv, "Wv")
        B, H, E = Qp.shape
        pooled = torch.empty_like(Qp)
        lse = torch.empty((B, H), device=keys.device, dtype=torch.float32)
        o = torch.empty((B, Wv.shape[0]), device=keys.device, dtype=torch.float32)
        ws = torch.empty(max(1, segs.ntiles) * H * (E + 2), device=keys.device, dtype=torch.float32)
        _lib.checked().mil_absorbed_pool_value_fwd(_p(keys), _p(pe), _p(Qp), _p(segs.k_off), _p(segs.tile_map),
                                                   _p(segs.bag_tile_off), segs.ntiles, B, H, C, E, _p(Wv), _p(_f32c(bv, "bv")),
                                                   _p(pooled), _p(lse), _p(o), _p(ws), _stream())
        ctx.segs, ctx.C, ctx.bv_param = segs, C, bv
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(keys, pe, Qp, pooled, lse, Wv)
        _note_site(keys, pe, Qp, lse, segs, C)
        return o, keys_in.view_as(keys_in)

    @staticmethod
    def backward(ctx, do, dkeys_pass):
        keys, pe, Qp, pooled, lse, Wv = ctx.saved_tensors
        segs, C = ctx.segs, ctx.C
        B, H, E = Qp.shape
        if do is None:
            return dkeys_pass, None, None, None, None, None, None
        dpooled, dWv, dbv = _value_proj_bwd(_f32c(do, "do"), Wv, ctx.bv_param, pooled)
        acc = _f32c(dkeys_pass, "dkeys") if dkeys_pass is not None else None
        dkeys = _dkeys_buffer(keys, segs)
        dQp = torch.empty_like(Qp)
        n_keys = keys.shape[0]
        ws = torch.empty(max(1, segs.ntiles) * H * E + 16 * n_keys, device=keys.device, dtype=torch.float32)
        _lib.checked().mil_absorbed_pool_bwd(_p(keys), _p(pe), _p(Qp), _p(lse), _p(dpooled), _p(pooled), _p(segs.k_off),
                                             _p(segs.tile_map), _p(segs.bag_tile_off), segs.ntiles, n_keys, B, H, C, E,
                                             _p(acc), _p(dkeys), _p(dQp), _p(ws), _stream())
        return dkeys, None, dQp, dWv, dbv, None, None


class _LnbrAbsorbedPoolValue(torch.autograd.Function):
    """keys = LayerNorm(x + row[bag]) (the image->token attention of the block in front, one text token per bag:
    _LayerNormBagRow) followed by _AbsorbedPoolValue on those keys, as ONE node (mil_lnbr_absorbed_pool_value_fwd / _bwd): the
    pool's forward kernel makes the keys it reads, and the pool's rank-16 update of dkeys is added by the LayerNorm backward
    to the gradient it loads.  Returns (o [B, H C], keys [rows, E]); the keys' other consumer's gradient arrives at this node
    (dkeys) and is folded in the same pass."""

    @staticmethod
    def forward(ctx, x, row, gamma, beta, eps: float, pe, Qp, Wv, bv, segs, C: int, tail_rows: int):
        x, row, pe, Qp, Wv = _f32c(x, "x"), _f32c(row, "row"), _f32c(pe, "pe"), _f32c(Qp, "Qp"), _f32c(Wv, "Wv")
        B, H, E = Qp.shape
        rows = x.shape[0]
        y = torch.empty((rows + tail_rows, E), device=x.device, dtype=torch.float32)[:rows] if tail_rows else torch.empty_like(x)
        if not getattr(segs, "pad_tiles", False) and getattr(segs, "device_lengths", False):
            y.zero_()                                   # rows no tile covers must still hold finite values
        stats = torch.empty((rows, 2), device=x.device, dtype=torch.float32)
        pooled = torch.empty_like(Qp)
        lse = torch.empty((B, H), device=x.device, dtype=torch.float32)
        o = torch.empty((B, Wv.shape[0]), device=x.device, dtype=torch.float32)
        ws = torch.empty(max(1, segs.ntiles) * H * (E + 2), device=x.device, dtype=torch.float32)
        _lib.checked().mil_lnbr_absorbed_pool_value_fwd(_p(x), _p(row), _p(_f32c(gamma, "gamma")), _p(_f32c(beta, "beta")),
                                                        float(eps), _p(pe), _p(Qp), _p(segs.k_off), _p(segs.tile_map),
                                                        _p(segs.bag_tile_off), segs.ntiles, B, H, C, E, _p(Wv),
                                                        _p(_f32c(bv, "bv")), _p(y), _p(stats), _p(pooled), _p(lse), _p(o),
                                                        _p(ws), _stream())
        ctx.segs, ctx.C, ctx.bv_param, ctx.beta_param = segs, C, bv, beta
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, row, gamma, stats, y, pe, Qp, pooled, lse, Wv, beta)
        _note_site(y, pe, Qp, lse, segs, C)             # the keys this site read are the y it wrote
        return o, y

    @staticmethod
    def backward(ctx, do, dy_pass):
        x, row, gamma, stats, y, pe, Qp, pooled, lse, Wv, beta = ctx.saved_tensors
        segs, C = ctx.segs, ctx.C
        B, H, E = Qp.shape
        rows = x.shape[0]
        dWv = dbv = None
        if do is None:
            dpooled = torch.zeros_like(pooled)          # the attention output has no reader: LayerNorm backward alone
        else:
            dpooled, dWv, dbv = _value_proj_bwd(_f32c(do, "do"), Wv, ctx.bv_param, pooled)
        acc = _f32c(dy_pass, "dkeys") if dy_pass is not None else None
        dx = torch.empty_like(x)
        if not getattr(segs, "pad_tiles", False) and getattr(segs, "device_lengths", False):
            dx.zero_()
        d_row = torch.empty_like(row)
        dg = grad_slot(gamma)
        if dg is None:
            dg = torch.empty(E, device=x.device, dtype=torch.float32)
        db = grad_slot(ctx.beta_param)
        if db is None:
            db = torch.empty(E, device=x.device, dtype=torch.float32)
        dQp = torch.empty_like(Qp)
        nt = max(1, segs.ntiles)
        ws = torch.empty(nt * H * E + 16 * rows + 3 * nt * E, device=x.device, dtype=torch.float32)
        _lib.checked().mil_lnbr_absorbed_pool_bwd(_p(x), _p(row), _p(gamma), _p(beta), _p(stats), _p(y), _p(pe), _p(Qp), _p(lse),
                                                  _p(dpooled), _p(pooled), _p(segs.k_off), _p(segs.tile_map),
                                                  _p(segs.bag_tile_off), segs.ntiles, rows, B, H, C, E, _p(acc), _p(dx),
                                                  _p(d_row), _p(dg), _p(db), _p(dQp), _p(ws), _stream())
        return dx, d_row, dg, db, None, None, dQp, dWv, dbv, None, None, None


def lnbr_one_token_ok(x, row, gamma, beta, Wk, Wv, bv, H: int) -> bool:
    """Shapes / trainability the fused LayerNorm(x + row) -> one-token attention node is built for."""
    return (x.dim() == 2 and x.shape[1] == 512 and x.shape[0] > 64 and H == 8 and Wk.shape[1] == 512
            and Wk.shape[0] // H in (32, 64)
            and (not torch.is_grad_enabled()
                 or (gamma.requires_grad and beta.requires_grad and Wv.requires_grad and bv.requires_grad)))


def lnbr_one_token_attention(x, row, gamma, beta, eps, pe, segs, Wk, Wv, bv, H: int, qp, tail_rows: int = 0):
    """keys = LayerNorm(x + row[bag]); token->image attention (projections absorbed) of ONE text token per bag over those
    keys.  qp [B, H C]: the projected query.  Returns (attention output [B, H C] before out_proj, keys [rows, E])."""
    C = Wk.shape[0] // H
    Qp = _AbsorbQuery.apply(qp, Wk, H)
    return _LnbrAbsorbedPoolValue.apply(x, row, gamma, beta, eps, pe, Qp, Wv, bv, segs, C, tail_rows)


def one_token_attention(q_tok, keys, pe, segs, Wq, bq, Wk, Wv, bv, H: int, qp=None):
    """Token->image attention core for ONE text token per bag, projections absorbed (csrc/absorbed_attn.hip).
    q_tok [B, E] (query + its pe), keys [R, E] WITHOUT positional encoding, pe [>= max N, E].  Returns the
    pre-out_proj attention output [B, H*C] and an alias of `keys` to be used by the keys' other consumer (see
    _AbsorbedPool).  k_proj.bias does not enter (softmax-invariant).  qp: the projected query q_proj(q_tok) when the
    caller has formed it already (ops.lin_ln_lin: the projection rides in the launch that applies the LayerNorm)."""
    if qp is None:
        qp = linear_act(q_tok, Wq, bq)
    C = Wk.shape[0] // H
    Qp = _AbsorbQuery.apply(qp, Wk, H)
    if Wk.shape[1] == 512 and H == 8 and Wv.requires_grad and bv.requires_grad:
        return _AbsorbedPoolValue.apply(keys, pe, Qp, Wv, bv, segs, C)        # pool + value projection: one node
    pooled, keys_pass = _AbsorbedPool.apply(keys, pe, Qp, segs, C)
    return _ValueProj.apply(pooled, Wv, bv, H), keys_pass
