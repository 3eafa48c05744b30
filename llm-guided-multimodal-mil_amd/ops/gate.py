"""ABMIL gate, attention pool, head and loss wrappers (fp32 and bf16 storage), dropout bits, Adam and SGD
(csrc/gate_*.hip, attn_pool.hip, head_loss.hip, gated_pool_bf16.hip, dropout.hip)."""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from .. import _lib
from ..bags import BagLayout
from ._base import GATE_D, M_DROP_SCALE, X_DROP_SCALE, _bf16c, _f32c, _p, _stream, grad_slot


def dropout_keep_bits(rows: int, cols: int, p_drop: float, seed: int, offset: int, device, out=None, offset_dev=None):
    """uint32-packed keep mask [rows, cols // 32] (stored as int32) from Philox4x32-10 (csrc/dropout.hip)."""
    if cols % 32:
        raise _lib.MilHipError("dropout_keep_bits: cols must be a multiple of 32")
    if out is None:
        out = torch.empty((rows, cols // 32), device=device, dtype=torch.int32)
    _lib.checked().mil_dropout_keep_bits(_p(out), rows, cols, float(p_drop), int(seed) & (2 ** 64 - 1),
                                         int(offset) & (2 ** 64 - 1), _p(offset_dev), _stream())
    return out


def dropout_keep_bits_pair(rows: int, bags: int, cols: int, seed: int, mseed: int, counter, done):
    """(xbits [rows, cols/32] at p = 0.5, mbits [bags, cols/32] at p = 0.25) drawn at stream position counter[0] in ONE launch
    that also advances the counter (mil_dropout_keep_bits_pair); rows == 0 / bags == 0: that tensor is None."""
    dev = counter.device
    xb = torch.empty((rows, cols // 32), device=dev, dtype=torch.int32) if rows else None
    mb = torch.empty((bags, cols // 32), device=dev, dtype=torch.int32) if bags else None
    m64 = 2 ** 64 - 1
    # mdelta = 1: the head's words at the position the separate launch drew them (behind the counter's increment)
    _lib.checked().mil_dropout_keep_bits_pair(_p(xb), rows, _p(mb), bags, cols, int(seed) & m64, int(mseed) & m64, 0,
                                              _p(counter), _p(counter), _p(done), 1, _stream())
    return xb, mb


def counter_add(counter, v: int = 1):
    """counter[0] += v on the current stream (device int32)."""
    _lib.checked().mil_counter_add(_p(counter), int(v), _stream())


def dropout_apply_bits(t, bits, scale: float):
    """t = keep ? t * scale : 0 in place."""
    rows, cols = t.shape
    _lib.checked().mil_dropout_apply_bits(_p(t), _p(bits), rows, cols, float(scale), _stream())
    return t


class _DropoutBits(torch.autograd.Function):
    """y = keep ? t / (1 - p) : 0 through a packed keep-bit tensor; the backward reads the same bits."""

    @staticmethod
    def forward(ctx, t, bits, scale: float):
        ctx.save_for_backward(bits)
        ctx.scale = scale
        return dropout_apply_bits(t.detach().clone().contiguous(), bits, scale)

    @staticmethod
    def backward(ctx, dy):
        (bits,) = ctx.saved_tensors
        return dropout_apply_bits(dy.detach().clone().contiguous(), bits, ctx.scale), None, None


def dropout_bits(t, bits, scale: float):
    """Differentiable form of dropout_apply_bits (out of place): the head's Dropout(.25) of the autograd route draws the same
    Philox keep words as the fused tail (csrc/dropout.hip) instead of torch's generator."""
    return _DropoutBits.apply(t, bits, scale)


def gate_scores_fwd(x, Wv, bv, Wu, bu, w, b, save_gates: bool = True, xbits=None, xscale: float = 1.0):
    """scores [R], gates [R, 384] (or None).  ABMIL.py:52-54.  xbits: keep bits of the patch dropout (train mode)."""
    x = _f32c(x, "x")
    R, L = x.shape
    scores = torch.empty(R, device=x.device, dtype=torch.float32)
    gates = torch.empty((R, 2 * GATE_D), device=x.device, dtype=torch.float32) if save_gates else None
    _lib.checked().mil_gate_scores_fwd(_p(x), _p(_f32c(Wv, "Wv")), _p(_f32c(bv, "bv")), _p(_f32c(Wu, "Wu")),
                                       _p(_f32c(bu, "bu")), _p(_f32c(w, "w")), _p(_f32c(b, "b")), _p(scores),
                                       _p(gates), R, L, Wv.shape[0], _p(xbits), float(xscale), _stream())
    return scores, gates


def attn_pool_fwd(x, scores, layout: BagLayout, xbits=None, xscale: float = 1.0):
    """M [B, L], lse [B].  ABMIL.py:56-59 per bag."""
    x = _f32c(x, "x")
    R, L = x.shape
    if R != layout.R:
        raise _lib.MilHipError(f"attn_pool_fwd: x has {R} rows but the bag layout covers {layout.R}")
    partials = torch.empty(layout.T * (L + 2), device=x.device, dtype=torch.float32)
    M = torch.empty((layout.B, L), device=x.device, dtype=torch.float32)
    lse = torch.empty(layout.B, device=x.device, dtype=torch.float32)
    _lib.checked().mil_attn_pool_fwd(_p(x), _p(scores), _p(layout.tile_map), _p(layout.bag_tile_off), layout.T,
                                     layout.B, L, _p(partials), _p(M), _p(lse), _p(xbits), float(xscale), _stream())
    return M, lse


def attn_pool_partial(x, scores, layout: BagLayout, xbits=None, xscale: float = 1.0):
    """Tile partials only ([T*L] weighted sums then [T*2] (max, sum) pairs); merged by pool_merge_head."""
    x = _f32c(x, "x")
    R, L = x.shape
    if R != layout.R:
        raise _lib.MilHipError(f"attn_pool_partial: x has {R} rows but the bag layout covers {layout.R}")
    partials = torch.empty(layout.T * (L + 2), device=x.device, dtype=torch.float32)
    _lib.checked().mil_attn_pool_partial(_p(x), _p(scores), _p(layout.tile_map), layout.T, L, _p(partials), _p(xbits),
                                         float(xscale), _stream())
    return partials


def attn_pool_partial_h(x, scores, layout: BagLayout, Wf, xbits=None, xscale: float = 1.0, mbits=None, mscale: float = 1.0):
    """Tile partials plus hrow [R, C] = x Wf^T (head projection of every patch; lets the backward skip x)."""
    x = _f32c(x, "x")
    R, L = x.shape
    C = Wf.shape[0]
    partials = torch.empty(layout.T * (L + 2), device=x.device, dtype=torch.float32)
    hrow = torch.empty((R, C), device=x.device, dtype=torch.float32)
    _lib.checked().mil_attn_pool_partial_h(_p(x), _p(scores), _p(layout.tile_map), layout.T, L, _p(partials),
                                           _p(_f32c(Wf, "Wf")), C, _p(hrow), _p(xbits), float(xscale), _p(mbits),
                                           float(mscale), _stream())
    return partials, hrow


def attn_pool_bwd_from_h(scores, lse, hrow, dz, cdot, layout: BagLayout):
    ds = torch.empty(scores.shape[0], device=scores.device, dtype=torch.float32)
    _lib.checked().mil_attn_pool_bwd_from_h(_p(scores), _p(lse), _p(hrow), _p(dz), _p(cdot), _p(layout.tile_map),
                                            layout.T, hrow.shape[1], _p(ds), _stream())
    return ds


def pool_merge_head(partials, layout: BagLayout, L: int, Wf, bf, y=None, scale: float = 1.0, scores=None, hrow=None,
                    mbits=None, mscale: float = 1.0, loss_kind: int = 0):
    """Fused per-bag tail: returns dict(M, lse, logits, prob[, loss_bag, dz, dM, cdot[, ds]]); with labels it also
    produces each bag's scaled BCE loss and the head's backward inputs for the pool, and with the forward's head
    projections `hrow` (attn_pool_partial_h) the score gradient ds of every row as well."""
    B, C, dev = layout.B, Wf.shape[0], partials.device
    out = dict(M=torch.empty((B, L), device=dev), lse=torch.empty(B, device=dev),
               logits=torch.empty((B, C), device=dev), prob=torch.empty((B, C), device=dev))
    if y is not None:
        out.update(dz=torch.empty((B, C), device=dev), dM=torch.empty((B, L), device=dev),
                   cdot=torch.empty(B, device=dev), loss_bag=torch.empty(B, device=dev))
        if hrow is not None and scores is not None:
            # capacity bucket (segments.FusionBucket): rows outside every tile are padding and must read ds = 0 - the bucket
            # owns the buffer and its refresh() launch zeroes those rows
            dsb = getattr(layout, "ds_buffer", None)
            out["ds"] = dsb if (dsb is not None and dsb.shape[0] == scores.shape[0]) else \
                (torch.zeros if getattr(layout, "device_lengths", False) else torch.empty)(scores.shape[0], device=dev)
    if mbits is not None:
        out["Mdrop"] = torch.empty((B, L), device=dev)
    # long bags (one ragged bag per step): the tail spreads over many workgroups through a small workspace
    ws = torch.empty(_lib.lib().mil_pool_tail_workspace_floats(B), device=dev) if ("ds" in out and layout.T >= 64 * B and B <= 8) else None
    _lib.checked().mil_pool_merge_head_ws(_p(partials), _p(layout.bag_tile_off), layout.T, B, L, _p(_f32c(Wf, "Wf")),
                                          _p(_f32c(bf, "bf")), C, _p(y), float(scale), _p(out["M"]), _p(out["lse"]),
                                          _p(out["logits"]), _p(out["prob"]), _p(out.get("loss_bag")), _p(out.get("dz")),
                                          _p(out.get("dM")), _p(out.get("cdot")),
                                          _p(layout.tile_map) if "ds" in out else None, _p(scores) if "ds" in out else None,
                                          _p(hrow) if "ds" in out else None, _p(out.get("ds")), _p(mbits), float(mscale),
                                          _p(out.get("Mdrop")), int(loss_kind), _p(ws), _stream())
    return out


def head_bwd_params(dz, M, dWf, dbf, loss_bag=None, loss_out=None):
    B, L = M.shape
    _lib.checked().mil_head_bwd_params(_p(dz), _p(M), _p(dWf), _p(dbf), B, L, dz.shape[1], _p(loss_bag), _p(loss_out),
                                       _stream())


def head_fwd(M, Wf, bf):
    """logits z [B, C], p = sigmoid(z).  aggregator.py:128-131,200 (eval)."""
    M = _f32c(M, "M")
    B, L = M.shape
    C = Wf.shape[0]
    z = torch.empty((B, C), device=M.device, dtype=torch.float32)
    p = torch.empty_like(z)
    _lib.checked().mil_head_fwd(_p(M), _p(_f32c(Wf, "Wf")), _p(_f32c(bf, "bf")), _p(z), _p(p), B, L, C, _stream())
    return z, p


def bce_fwd_bwd(p, y, scale: float, loss_sum: Optional[torch.Tensor] = None):
    """Adds sum(BCE) * scale into loss_sum [1] and returns (loss_sum, dz = (p - y) * scale)."""
    B, C = p.shape
    if loss_sum is None:
        loss_sum = torch.zeros(1, device=p.device, dtype=torch.float32)
    dz = torch.empty_like(p)
    _lib.checked().mil_bce_fwd_bwd(_p(_f32c(p, "p")), _p(_f32c(y, "y")), _p(loss_sum), _p(dz), B, C, float(scale),
                                   _stream())
    return loss_sum, dz


def head_bwd(dz_or_dp, p, M, Wf):
    """(dM [B, L], dWf [C, L], dbf [C], cdot [B]).  If p is given the first argument is dL/dp."""
    B, L = M.shape
    C = Wf.shape[0]
    dM = torch.empty_like(M)
    dWf = torch.empty((C, L), device=M.device, dtype=torch.float32)
    dbf = torch.empty(C, device=M.device, dtype=torch.float32)
    cdot = torch.empty(B, device=M.device, dtype=torch.float32)
    _lib.checked().mil_head_bwd(_p(_f32c(dz_or_dp, "dz")), _p(p), _p(_f32c(M, "M")), _p(_f32c(Wf, "Wf")), _p(dM),
                                _p(dWf), _p(dbf), _p(cdot), B, L, C, _stream())
    return dM, dWf, dbf, cdot


def rowdot(a, c):
    B, L = a.shape
    out = torch.empty(B, device=a.device, dtype=torch.float32)
    _lib.checked().mil_rowdot(_p(_f32c(a, "a")), _p(_f32c(c, "c")), _p(out), B, L, _stream())
    return out


def attn_pool_bwd(x, scores, lse, dM, cdot, layout: BagLayout, want_dx: bool, xbits=None, xscale: float = 1.0):
    """ds [R] and, if requested, the pool term of dx ([R, L] = A_i dM)."""
    x = _f32c(x, "x")
    R, L = x.shape
    ds = torch.empty(R, device=x.device, dtype=torch.float32)
    dx = torch.empty_like(x) if want_dx else None
    _lib.checked().mil_attn_pool_bwd(_p(x), _p(scores), _p(lse), _p(_f32c(dM, "dM")), _p(cdot), _p(layout.tile_map),
                                     layout.T, L, _p(ds), _p(dx), _p(xbits), float(xscale), _stream())
    return ds, dx


def gate_bwd_params(x, gates, ds, w, dWv, dbv, dWu, dbu, dw, db, accumulate: bool = False,
                    workspace: Optional[torch.Tensor] = None, xbits=None, xscale: float = 1.0):
    x = _f32c(x, "x")
    R, L = x.shape
    need = _lib.lib().mil_gate_bwd_workspace_floats(R, L)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, device=x.device, dtype=torch.float32)
    _lib.checked().mil_gate_bwd_params(_p(x), _p(gates), _p(ds), _p(_f32c(w, "w")), R, L, GATE_D, _p(workspace),
                                       workspace.numel(), _p(dWv), _p(dbv), _p(dWu), _p(dbu), _p(dw), _p(db),
                                       1 if accumulate else 0, _p(xbits), float(xscale), _stream())
    return workspace


def gate_bwd_params_head(x, gates, ds, w, dWv, dbv, dWu, dbu, dw, db, dz, M, dWf, dbf, loss_bag=None, loss_out=None,
                         workspace: Optional[torch.Tensor] = None, xbits=None, xscale: float = 1.0):
    """gate_bwd_params + head_bwd_params in two launches instead of three: the head's parameter gradients are computed by
    workgroups appended to the reduce launch (mil_gate_bwd_params_head)."""
    x = _f32c(x, "x")
    R, L = x.shape
    need = _lib.lib().mil_gate_bwd_workspace_floats(R, L)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, device=x.device, dtype=torch.float32)
    B, C = dz.shape
    if M.shape[1] != L:
        raise _lib.MilHipError("gate_bwd_params_head: the bag embeddings must have the gate's input width")
    _lib.checked().mil_gate_bwd_params_head(_p(x), _p(gates), _p(ds), _p(_f32c(w, "w")), R, L, GATE_D, _p(workspace),
                                            workspace.numel(), _p(dWv), _p(dbv), _p(dWu), _p(dbu), _p(dw), _p(db), 0,
                                            _p(dz), _p(M), _p(dWf), _p(dbf), B, C, _p(loss_bag), _p(loss_out), _p(xbits),
                                            float(xscale), _stream())
    return workspace


def gate_bwd_input(gates, ds, w, Wv, Wu, dx, xbits=None, xscale: float = 1.0):
    R, L = dx.shape
    _lib.checked().mil_gate_bwd_input(_p(gates), _p(ds), _p(_f32c(w, "w")), _p(_f32c(Wv, "Wv")), _p(_f32c(Wu, "Wu")),
                                      R, L, GATE_D, _p(dx), _p(xbits), float(xscale), _stream())
    return dx


def adam_step(param, grad, exp_avg, exp_avg_sq, step: int, lr: float = 1e-5, betas=(0.9, 0.999), eps: float = 1e-8,
              weight_decay: float = 1e-7, grad_scale: float = 1.0):
    _lib.checked().mil_adam_step(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), param.numel(), int(step), lr,
                                 betas[0], betas[1], eps, weight_decay, grad_scale, _stream())


def adam_step_counted(param, grad, exp_avg, exp_avg_sq, step_counter, lr: float = 1e-5, betas=(0.9, 0.999),
                      eps: float = 1e-8, weight_decay: float = 1e-7, grad_scale: float = 1.0):
    """Adam with the step number in a device int32 (incremented by the call): same launches every step."""
    _lib.checked().mil_adam_step_counted(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), param.numel(),
                                         _p(step_counter), lr, betas[0], betas[1], eps, weight_decay, grad_scale,
                                         _stream())


def adam_step_counted_noinc(param, grad, exp_avg, exp_avg_sq, step_counter, lr: float = 1e-5, betas=(0.9, 0.999),
                            eps: float = 1e-8, weight_decay: float = 1e-7, grad_scale: float = 1.0):
    """One segment of a counted Adam step; the caller advances the counter once (counter_add)."""
    _lib.checked().mil_adam_step_counted_noinc(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), param.numel(),
                                               _p(step_counter), lr, betas[0], betas[1], eps, weight_decay, grad_scale,
                                               _stream())


def adam_step_dev(param, grad, exp_avg, exp_avg_sq, step_counter, lr_dev, betas=(0.9, 0.999), eps: float = 1e-8,
                  weight_decay: float = 1e-7, grad_scale: float = 1.0, inc: bool = True):
    """Counted Adam with the learning rate in device memory too (lr_dev [1]): a captured step follows the schedule."""
    _lib.checked().mil_adam_step_dev(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), param.numel(), _p(step_counter),
                                     _p(lr_dev), betas[0], betas[1], eps, weight_decay, grad_scale, 1 if inc else 0, _stream())


def adam_step_dev_segs(param, grad, exp_avg, exp_avg_sq, segs, step_counter, lr_dev, done_counter, betas=(0.9, 0.999),
                       eps: float = 1e-8, weight_decay: float = 1e-7, grad_scale: float = 1.0, inc: bool = True):
    """Adam over the ranges `segs` = [(begin, end), ...] of the flat buffers + the step-counter advance, one launch."""
    n = len(segs)
    b = (ctypes.c_size_t * n)(*[int(a_) for a_, _ in segs])
    e = (ctypes.c_size_t * n)(*[int(b_) for _, b_ in segs])
    _lib.checked().mil_adam_step_dev_segs(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), b, e, n, _p(step_counter), _p(lr_dev),
                                          _p(done_counter), betas[0], betas[1], eps, weight_decay, grad_scale, int(inc), _stream())


def sgd_step(param, grad, lr: float = 1e-3, weight_decay: float = 1e-7, grad_scale: float = 1.0):
    """torch.optim.SGD (no momentum, L2 weight decay) over a flat buffer, in place."""
    _lib.checked().mil_sgd_step(_p(param), _p(grad), param.numel(), lr, weight_decay, grad_scale, _stream())


# --------------------------------------------------------------------------- autograd wrappers
class _GatedAttentionPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, Wv, bv, Wu, bu, w, b, layout: BagLayout, xbits=None):
        x = _f32c(x, "x")
        need_grad = any(ctx.needs_input_grad[:7])
        xs = X_DROP_SCALE if xbits is not None else 1.0
        scores, gates = gate_scores_fwd(x, Wv, bv, Wu, bu, w.reshape(-1), b, save_gates=need_grad, xbits=xbits, xscale=xs)
        M, lse = attn_pool_fwd(x, scores, layout, xbits=xbits, xscale=xs)
        ctx.layout, ctx.xbits, ctx.xs = layout, xbits, xs
        ctx.save_for_backward(x, Wv, Wu, w, scores, gates if gates is not None else torch.empty(0, device=x.device), lse, M)
        ctx.mark_non_differentiable(scores)
        return M, scores

    @staticmethod
    def backward(ctx, dM, _dscores):
        x, Wv, Wu, w, scores, gates, lse, M = ctx.saved_tensors
        dM = _f32c(dM, "dM")
        cdot = rowdot(M, dM)
        want_dx = ctx.needs_input_grad[0]
        xbits, xs = ctx.xbits, ctx.xs
        ds, dx = attn_pool_bwd(x, scores, lse, dM, cdot, ctx.layout, want_dx, xbits=xbits, xscale=xs)
        dWv = torch.empty_like(Wv)
        dWu = torch.empty_like(Wu)
        dbv = torch.empty(GATE_D, device=x.device, dtype=torch.float32)
        dbu = torch.empty_like(dbv)
        dw = torch.empty_like(dbv)
        db = torch.empty(1, device=x.device, dtype=torch.float32)
        wflat = w.reshape(-1)
        gate_bwd_params(x, gates, ds, wflat, dWv, dbv, dWu, dbu, dw, db, xbits=xbits, xscale=xs)
        if want_dx:
            gate_bwd_input(gates, ds, wflat, Wv, Wu, dx, xbits=xbits, xscale=xs)      # also applies the dropout backward
        return dx, dWv, dbv, dWu, dbu, dw.reshape(w.shape), db, None, None


def gated_attention_pool(x, Wv, bv, Wu, bu, w, b, layout: BagLayout, xbits=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """M [B, L] (differentiable) and the raw attention scores [R] (not differentiable).  xbits: keep bits of the
    patch dropout (train mode, ABMIL.py:49): the kernels read x through the mask, no dropped copy is made."""
    return _GatedAttentionPool.apply(x, Wv, bv, Wu, bu, w, b, layout, xbits)


def _bag_order(layout):
    """(lengths, perm): per-bag row counts and the int64 device index that gathers the rows of a layout bag by bag (None when
    the bags are contiguous already).  Cached on the layout; needs its lengths on the host."""
    lengths = getattr(layout, "lengths", None)
    if lengths is None:
        lengths = getattr(layout, "k_lengths", None)          # AttnSegs-shaped: the keys of each bag, contiguous
        if lengths is None:
            raise NotImplementedError("bag_softmax: the layout's bag lengths live on the device only (capacity bucket)")
        return [int(v) for v in lengths], None
    hit = getattr(layout, "_bag_order", None)
    if hit is None:
        rb = layout.row_bag().cpu()
        perm = torch.argsort(rb, stable=True)
        same = bool((perm == torch.arange(perm.numel())).all())
        hit = layout._bag_order = ([int(v) for v in lengths], None if same else perm.to(layout.tile_map.device))
    return hit


def _bag_softmax_bucket(scores, layout):
    """bag_softmax over the multi-modal bag face of a capacity bucket (segments.FusionBucket.layout): the bags' rows are
    scattered over [cap patch rows | B tail rows per segment] and their lengths live on the device, so the weights come back
    in the ROW order of the buffer, w [R], 0 on the padding rows (mil_bag_softmax_rows: the bucket's tile map names each bag's
    rows; nothing is read on the host - capture-safe)."""
    if scores.numel() != layout.R:
        raise ValueError(f"bag_softmax: {scores.numel()} scores for a bucket of {layout.R} rows")
    w = torch.empty_like(scores)
    _lib.checked().mil_bag_softmax_rows(_p(scores), _p(layout.tile_map), _p(layout.bag_tile_off), layout.T,
                                        _p(layout.row_bag()), layout.B, layout.R, _p(w), _stream())
    return w


def bag_softmax(scores, layout_or_segs, len_dev=None):
    """The gated-attention pool's weights: w = softmax of `scores` [R] over the rows of each bag (mil_bag_softmax), returned bag
    by bag - bag b at [off[b], off[b] + lengths[b]), off = cumsum of the layout's lengths, its rows in the order they have
    in memory (a two-segment multi-modal bag: its patch rows, then its token rows).  len_dev (int32 [B], on the device): the
    layout's lengths are slot capacities and bag b has len_dev[b] rows; the rows behind them get 0.  A capacity bucket's
    multi-modal bag face (device lengths, scattered rows): see _bag_softmax_bucket - w in row order.  No gradient."""
    scores = _f32c(scores.detach(), "scores").reshape(-1)
    if getattr(layout_or_segs, "device_lengths", False) and getattr(layout_or_segs, "lengths", None) is None \
            and hasattr(layout_or_segs, "bag_tile_off") and hasattr(layout_or_segs, "row_bag"):
        return _bag_softmax_bucket(scores, layout_or_segs)
    lengths, perm = _bag_order(layout_or_segs)
    if scores.numel() != sum(lengths):
        raise ValueError(f"bag_softmax: {scores.numel()} scores for bags of {sum(lengths)} rows")
    if perm is not None:
        scores = scores.index_select(0, perm)
    off = [0]
    for n in lengths:
        off.append(off[-1] + n)
    row_off = getattr(layout_or_segs, "_bag_row_off", None)
    if row_off is None or row_off.device != scores.device:
        row_off = torch.tensor(off, dtype=torch.int32).to(scores.device)
        try:
            layout_or_segs._bag_row_off = row_off
        except AttributeError:
            pass
    if len_dev is not None and (not len_dev.is_cuda or len_dev.dtype != torch.int32 or len_dev.numel() != len(lengths)):
        raise _lib.MilHipError("bag_softmax: len_dev must be int32 [B] on the GPU")
    w = torch.empty_like(scores)
    _lib.checked().mil_bag_softmax(_p(scores), _p(row_off), _p(len_dev), len(lengths), _p(w), _stream())
    return w


def gate_bwd_input_pool(gates, ds, w, Wv, Wu, dx, scores, lse, row_bag, dM, xbits=None, xscale: float = 1.0):
    """dx = a_row dM[bag(row)] + dPre [Wv; Wu] written in ONE pass (mil_gate_bwd_input_pool): the attention pool's own input
    gradient is formed in the epilogue of the gate's input-gradient product, dx is never read."""
    R, L = dx.shape
    _lib.checked().mil_gate_bwd_input_pool(_p(gates), _p(ds), _p(_f32c(w, "w")), _p(_f32c(Wv, "Wv")), _p(_f32c(Wu, "Wu")),
                                           R, L, GATE_D, _p(dx), _p(xbits), float(xscale), _p(scores), _p(lse), _p(row_bag),
                                           _p(dM), _stream())
    return dx


class _GatedPoolHeadLoss(torch.autograd.Function):
    """ABMIL pool -> Dropout(.25) -> fc -> sigmoid -> BCELoss(mean) (or CE on the sigmoid outputs) as ONE autograd node
    (ABMIL.py:47-59 + aggregator.py:128-131,200 + train_ddp.py:95-99,323-324), on the fused per-bag tail of the image-only
    step: gate forward, pool partial pass with the head-projection by-product, one tail launch (merge, head, loss, dz, dM,
    ds) and the head's parameter gradients - 4 launches where the op-by-op route takes 17; the backward is the gate's
    weight-gradient product, its reduce, and ONE pass writing dx (pool term + gate term).
    Returns (loss [scalar], prob [B, C], logits [B, C], M [B, L]); only the loss is differentiable, and it must be the
    root of the backward pass (its incoming gradient is taken to be 1; scale through `scale`)."""

    _checked_unit_grad = False

    @staticmethod
    def forward(ctx, x, Wv, bv, Wu, bu, w, b, Wf, bf, y, layout: BagLayout, scale: float, loss_kind: int, xbits, mbits):
        x = _f32c(x, "x")
        L = x.shape[1]
        xs = X_DROP_SCALE if xbits is not None else 1.0
        ms = M_DROP_SCALE if mbits is not None else 1.0
        need_grad = any(ctx.needs_input_grad[:9])
        scores, gates = gate_scores_fwd(x, Wv, bv, Wu, bu, w.reshape(-1), b, save_gates=need_grad, xbits=xbits, xscale=xs)
        partials, hrow = attn_pool_partial_h(x, scores, layout, Wf, xbits, xs, mbits, ms)
        t = pool_merge_head(partials, layout, L, Wf, bf, _f32c(y, "y"), scale, scores, hrow, mbits, ms, loss_kind)
        loss = torch.empty(1, device=x.device, dtype=torch.float32)
        dWf = (grad_slot(Wf) if need_grad else None)
        dbf = (grad_slot(bf) if need_grad else None)
        dWf = dWf if dWf is not None else torch.empty_like(Wf)
        dbf = dbf if dbf is not None else torch.empty_like(bf)
        head_bwd_params(t["dz"], t.get("Mdrop", t["M"]), dWf, dbf, t["loss_bag"], loss)
        ctx.layout, ctx.xbits, ctx.xs = layout, xbits, xs
        ctx.params = (Wv, bv, Wu, bu, w, b)
        ctx.save_for_backward(x, Wv, Wu, w, gates if gates is not None else torch.empty(0, device=x.device), scores,
                              t["lse"], t["ds"], t["dM"], dWf, dbf)
        for o in (t["prob"], t["logits"], t["M"]):
            ctx.mark_non_differentiable(o)
        ctx.set_materialize_grads(False)        # no zero tensors for the three non-differentiable outputs
        return loss.reshape(()), t["prob"], t["logits"], t["M"]

    @staticmethod
    def backward(ctx, dloss, _dp, _dz, _dM):
        x, Wv, Wu, w, gates, scores, lse, ds, dM, dWf, dbf = ctx.saved_tensors
        if not _GatedPoolHeadLoss._checked_unit_grad and not torch.cuda.is_current_stream_capturing():
            _GatedPoolHeadLoss._checked_unit_grad = True
            if abs(float(dloss) - 1.0) > 1e-6:
                raise _lib.MilHipError("fused pool+head+loss: the loss must be the root of backward() (incoming gradient 1); "
                                       "fold any factor into `scale`")
        pW = ctx.params
        outs = []
        for prm in pW:
            slot = grad_slot(prm)
            outs.append(slot if slot is not None else torch.empty(prm.shape, device=x.device, dtype=torch.float32))
        dWv, dbv, dWu, dbu, dw, db = outs
        wflat = w.reshape(-1)
        xbits, xs = ctx.xbits, ctx.xs
        gate_bwd_params(x, gates, ds, wflat, dWv, dbv, dWu, dbu, dw, db, xbits=xbits, xscale=xs)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            gate_bwd_input_pool(gates, ds, wflat, Wv, Wu, dx, scores, lse, ctx.layout.row_bag(), dM, xbits=xbits, xscale=xs)
        return dx, dWv, dbv, dWu, dbu, dw, db, dWf, dbf, None, None, None, None, None, None


def gated_pool_head_loss(x, Wv, bv, Wu, bu, w, b, Wf, bf, y, layout: BagLayout, scale: float, loss_kind: int = 0,
                         xbits=None, mbits=None):
    """(loss, prob, logits, M) of the fused ABMIL + head + loss node (see _GatedPoolHeadLoss)."""
    return _GatedPoolHeadLoss.apply(x, Wv, bv, Wu, bu, w, b, Wf, bf, y, layout, float(scale), int(loss_kind), xbits, mbits)


class _HeadSigmoid(torch.autograd.Function):
    @staticmethod
    def forward(ctx, M, Wf, bf):
        z, p = head_fwd(M, Wf, bf)
        ctx.save_for_backward(M, Wf, p)
        ctx.mark_non_differentiable(z)
        return p, z

    @staticmethod
    def backward(ctx, dp, _dz):
        M, Wf, p = ctx.saved_tensors
        dM, dWf, dbf, _ = head_bwd(_f32c(dp, "dp"), p, M, Wf)
        return dM, dWf, dbf


def head_sigmoid(M, Wf, bf):
    """(p = sigmoid(fc(M)) [B, C] differentiable, logits z [B, C])."""
    return _HeadSigmoid.apply(M, Wf, bf)


# --------------------------------------------------------------------------- K1 bf16-storage variant (config 5)
def cast_bf16(src: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    src = _f32c(src, "src")
    if out is None:
        out = torch.empty(src.shape, device=src.device, dtype=torch.bfloat16)
    _lib.checked().mil_cast_bf16(_p(src), _p(out), src.numel(), _stream())
    return out


def gate_scores_fwd_bf16(x16, Wv16, bv, Wu16, bu, w, b, save_gates: bool = True, gates_bf16: bool = False, xbits=None,
                         xscale: float = 1.0):
    """gates_bf16: save {V | U} rounded to bf16 (what gate_bwd_params_bf16 reads) instead of fp32."""
    x16 = _bf16c(x16, "x")
    R, L = x16.shape
    scores = torch.empty(R, device=x16.device, dtype=torch.float32)
    gates = gates16 = None
    if save_gates and gates_bf16:
        gates16 = torch.empty((R, 2 * GATE_D), device=x16.device, dtype=torch.bfloat16)
    elif save_gates:
        gates = torch.empty((R, 2 * GATE_D), device=x16.device, dtype=torch.float32)
    _lib.checked().mil_gate_scores_fwd_bf16(_p(x16), _p(_bf16c(Wv16, "Wv")), _p(bv), _p(_bf16c(Wu16, "Wu")), _p(bu), _p(w),
                                            _p(b), _p(scores), _p(gates), R, L, Wv16.shape[0], _p(gates16), _p(xbits),
                                            float(xscale), _stream())
    return scores, (gates16 if gates_bf16 else gates)


def attn_pool_partial_bf16(x16, scores, layout: BagLayout, xbits=None, xscale: float = 1.0):
    x16 = _bf16c(x16, "x")
    R, L = x16.shape
    partials = torch.empty(layout.T * (L + 2), device=x16.device, dtype=torch.float32)
    _lib.checked().mil_attn_pool_partial_bf16(_p(x16), _p(scores), _p(layout.tile_map), layout.T, L, _p(partials), _p(xbits),
                                              float(xscale), _stream())
    return partials


def attn_pool_partial_h_bf16(x16, scores, layout: BagLayout, Wf, xbits=None, xscale: float = 1.0, mbits=None,
                             mscale: float = 1.0):
    """bf16 tile partials plus hrow [R, C] = x Wf^T (mil_attn_pool_partial_h_bf16)."""
    x16 = _bf16c(x16, "x")
    R, L = x16.shape
    C = Wf.shape[0]
    partials = torch.empty(layout.T * (L + 2), device=x16.device, dtype=torch.float32)
    hrow = torch.empty((R, C), device=x16.device, dtype=torch.float32)
    _lib.checked().mil_attn_pool_partial_h_bf16(_p(x16), _p(scores), _p(layout.tile_map), layout.T, L, _p(partials),
                                                _p(_f32c(Wf, "Wf")), C, _p(hrow), _p(xbits), float(xscale), _p(mbits),
                                                float(mscale), _stream())
    return partials, hrow


def attn_pool_bwd_bf16(x16, scores, lse, dM, cdot, layout: BagLayout, xbits=None, xscale: float = 1.0):
    x16 = _bf16c(x16, "x")
    R, L = x16.shape
    ds = torch.empty(R, device=x16.device, dtype=torch.float32)
    _lib.checked().mil_attn_pool_bwd_bf16(_p(x16), _p(scores), _p(lse), _p(dM), _p(cdot), _p(layout.tile_map), layout.T, L,
                                          _p(ds), _p(xbits), float(xscale), _stream())
    return ds


def gate_bwd_params_x16(x16, gates, ds, w, dWv, dbv, dWu, dbu, dw, db, accumulate: bool = False, workspace=None, xbits=None,
                        xscale: float = 1.0):
    x16 = _bf16c(x16, "x")
    R, L = x16.shape
    need = _lib.lib().mil_gate_bwd_workspace_floats(R, L)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, device=x16.device, dtype=torch.float32)
    _lib.checked().mil_gate_bwd_params_x16(_p(x16), _p(gates), _p(ds), _p(w), R, L, GATE_D, _p(workspace),
                                           workspace.numel(), _p(dWv), _p(dbv), _p(dWu), _p(dbu), _p(dw), _p(db),
                                           1 if accumulate else 0, _p(xbits), float(xscale), _stream())
    return workspace


def gate_bwd_params_bf16(x16, gates, ds, w, dWv, dbv, dWu, dbu, dw, db, accumulate: bool = False, workspace=None, xbits=None,
                         xscale: float = 1.0):
    """Weight gradients on the bf16 MFMA (dPre and x rounded to bf16, fp32 accumulate); gates: bf16 [R, 384]."""
    x16 = _bf16c(x16, "x")
    gates = _bf16c(gates, "gates")
    R, L = x16.shape
    need = _lib.lib().mil_gate_bwd_workspace_floats_bf16(R, L)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, device=x16.device, dtype=torch.float32)
    _lib.checked().mil_gate_bwd_params_bf16(_p(x16), _p(gates), _p(ds), _p(w), R, L, GATE_D, _p(workspace),
                                            workspace.numel(), _p(dWv), _p(dbv), _p(dWu), _p(dbu), _p(dw), _p(db),
                                            1 if accumulate else 0, _p(xbits), float(xscale), _stream())
    return workspace
