"""Tiled, mid and few-rows linears with their autograd nodes, the fan-out mailbox, frozen split-bf16 linears
(csrc/linear*.hip, small_linear.hip, mid_linear.hip)."""
from __future__ import annotations

import torch

from .. import _lib, deferred
from ._base import ACT, _f32c, _p, _stream, _stream_int, grad_slot


def gemm(A, a_mode: int, B, b_mode: int, M: int, N: int, K: int, out=None, bias=None, act: int = 0, residual=None,
         accumulate: bool = False, split_k: bool = True, rows_dev=None):
    """C[M,N] (+)= act(A_op . B_op + bias) + residual  (include/mil_hip.h: mil_gemm)."""
    A = _f32c(A, "A")
    B = _f32c(B, "B")
    if out is None:
        out = torch.empty((M, N), device=A.device, dtype=torch.float32)
    ws, nws = None, 0
    if split_k:
        nws = _lib.lib().mil_gemm_workspace_floats(M, N, K, a_mode)
        if nws:
            ws = torch.empty(nws, device=A.device, dtype=torch.float32)
    if rows_dev is not None:       # capacity bucket: true row count on the device (include/mil_hip.h: mil_gemm_rows)
        _lib.checked().mil_gemm_rows(_p(A), A.stride(0), a_mode, _p(B), B.stride(0), b_mode, _p(out), out.stride(0), M, N, K,
                                     _p(bias), act, _p(residual), residual.stride(0) if residual is not None else 0,
                                     1 if accumulate else 0, _p(ws), nws, _p(rows_dev), _stream())
        return out
    _lib.checked().mil_gemm(_p(A), A.stride(0), a_mode, _p(B), B.stride(0), b_mode, _p(out), out.stride(0), M, N, K,
                            _p(bias), act, _p(residual), residual.stride(0) if residual is not None else 0,
                            1 if accumulate else 0, _p(ws), nws, _stream())
    return out


def gemm_aux(A, B, b_mode: int, M: int, N: int, K: int, aux, aux_mode: int, bias=None, act: int = 0, residual=None):
    """C = act(A . B_op + bias) + residual with one auxiliary [M, N] tensor handled in the epilogue
    (include/mil_hip.h: mil_gemm_aux; aux_mode 1 = store the pre-activation, 2 = multiply by QuickGELU'(aux))."""
    A, B = _f32c(A, "A"), _f32c(B, "B")
    out = torch.empty((M, N), device=A.device, dtype=torch.float32)
    nws = _lib.lib().mil_gemm_workspace_floats(M, N, K, 0)
    ws = torch.empty(nws, device=A.device, dtype=torch.float32) if nws else None
    _lib.checked().mil_gemm_aux(_p(A), A.stride(0), 0, _p(B), B.stride(0), b_mode, _p(out), out.stride(0), M, N, K,
                                _p(bias), act, _p(residual), residual.stride(0) if residual is not None else 0, 0,
                                _p(ws), nws, _p(aux), aux.stride(0), aux_mode, _stream())
    return out


def linear_bwd_params(dy, y, act: int, x, dW_out=None, db_out=None, want_db: bool = True, rows_dev=None):
    """dW = (dy (.) act'(y))^T x and db = its column sums in one product launch + fold (mil_linear_bwd_params).
    y may be None for act 0.  Returns (dW [N, K], db [N] or None)."""
    rows, N = dy.shape
    K = x.shape[1]
    dW = dW_out if dW_out is not None else torch.empty((N, K), device=dy.device, dtype=torch.float32)
    db = None
    if want_db:
        db = db_out if db_out is not None else torch.empty(N, device=dy.device, dtype=torch.float32)
    nws = _lib.lib().mil_linear_bwd_params_workspace_floats(rows, N, K)
    ws = torch.empty(nws, device=dy.device, dtype=torch.float32)
    _lib.checked().mil_linear_bwd_params_rows(_p(dy), dy.stride(0), _p(y), y.stride(0) if y is not None else 0, act, _p(x),
                                              x.stride(0), rows, N, K, _p(dW), dW.stride(0), _p(db), 0, _p(ws), nws,
                                              _p(rows_dev), _stream())
    return dW, db


def colsum(Y, out=None, accumulate: bool = False):
    M, N = Y.shape
    if out is None:
        out = torch.empty(N, device=Y.device, dtype=torch.float32)
    nws = _lib.lib().mil_colsum_workspace_floats(M, N)
    ws = torch.empty(nws, device=Y.device, dtype=torch.float32) if nws else None
    _lib.checked().mil_colsum(_p(Y), Y.stride(0), M, N, _p(out), 1 if accumulate else 0, _p(ws), _stream())
    return out


def act_bwd(dy, y, act: int):
    if act == 0:
        return dy
    dpre = torch.empty_like(dy)
    _lib.checked().mil_act_bwd(_p(dy), _p(y), _p(dpre), dy.numel(), act, _stream())
    return dpre


SMALL_ROWS = 64        # include/mil_hip.h: MIL_SMALL_ROWS (raising it to 512 was measured: T = 10 step 6.0 -> 6.7 ms)


def _small_ok(M: int, N: int, K: int, *tensors) -> bool:
    return (0 < M <= SMALL_ROWS and K % 16 == 0 and N % 16 == 0
            and all(t is None or (t.data_ptr() % 16 == 0 and t.stride(0) % 4 == 0) for t in tensors))


MID_ROWS = 1024            # csrc/mid_linear.hip: one-launch products for layers between the few-rows and the tiled regime
MID_WORK = 340_000_000     # M * N * K up to which they beat the tiled GEMM + split-K fold (tools/kbench_mid.py)


def _mid_ok(M: int, N: int, K: int, *tensors) -> bool:
    return (SMALL_ROWS < M <= MID_ROWS and M * N * K <= MID_WORK and K % 8 == 0 and N % 8 == 0
            and all(t is None or (t.data_ptr() % 16 == 0 and t.stride(0) % 4 == 0) for t in tensors))


def linear_mid_fwd(x, W, b, act: int, residual=None):
    """nn.Linear on 65..1024 rows in one launch (include/mil_hip.h: mil_linear_mid_fwd)."""
    M, K = x.shape
    N = W.shape[0]
    y = torch.empty((M, N), device=x.device, dtype=torch.float32)
    _lib.checked().mil_linear_mid_fwd(_p(x), x.stride(0), _p(W), W.stride(0), _p(b), act, _p(residual),
                                      residual.stride(0) if residual is not None else 0, _p(y), y.stride(0), M, N, K,
                                      _stream())
    return y


def linear_mid_bwd(dy, y, act: int, x, W, need_dx: bool, need_dW: bool, need_db: bool, dW_out=None, db_out=None):
    """Backward of the same layer, one launch per product (mil_linear_mid_bwd): dx, dW (+ db from the same pass)."""
    M, N = dy.shape
    K = x.shape[1]
    dev = dy.device
    dx = torch.empty((M, K), device=dev, dtype=torch.float32) if need_dx else None
    need_dW = need_dW or need_db
    dW = (dW_out if dW_out is not None else torch.empty((N, K), device=dev, dtype=torch.float32)) if need_dW else None
    db = (db_out if db_out is not None else torch.empty(N, device=dev, dtype=torch.float32)) if need_db else None
    _lib.checked().mil_linear_mid_bwd(_p(dy), dy.stride(0), _p(y) if act else None, y.stride(0) if act else 0, act, _p(x),
                                      x.stride(0), _p(W), W.stride(0), _p(dx), K, _p(dW), dW.stride(0) if need_dW else 0,
                                      _p(db), M, N, K, _stream())
    return dx, dW, db


def linear_small_fwd(x, W, b, act: int, residual=None, x2=None):
    """Token-side nn.Linear (M <= 64 rows) in one launch (include/mil_hip.h: mil_linear_small_fwd).  x2: a second addend of
    the input (mil_linear_small_fwd_add) - returns (y, x + x2)."""
    M, K = x.shape
    N = W.shape[0]
    y = torch.empty((M, N), device=x.device, dtype=torch.float32)
    if x2 is not None:
        xin = torch.empty((M, K), device=x.device, dtype=torch.float32)
        _lib.checked().mil_linear_small_fwd_add(_p(x), x.stride(0), _p(x2), x2.stride(0), _p(xin), _p(W), W.stride(0), _p(b), act,
                                                _p(residual), residual.stride(0) if residual is not None else 0, _p(y),
                                                y.stride(0), M, N, K, _stream())
        return y, xin
    sh = _lib.shim()
    if sh is not None:          # same C entry through the torch cpp_extension binding (csrc/torch_shim.cpp)
        sh.linear_small_fwd(x, W, b, act, residual, y, _stream_int())
        return y
    _lib.checked().mil_linear_small_fwd(_p(x), x.stride(0), _p(W), W.stride(0), _p(b), act, _p(residual),
                                        residual.stride(0) if residual is not None else 0, _p(y), y.stride(0),
                                        M, N, K, _stream())
    return y


def linear_small_bwd(dy, y_or_pre, act: int, x, W, want_dx: bool, want_dW: bool, want_db: bool, dW_out=None, db_out=None,
                     extras=(), dysum=None):
    """dx, dW, db of that layer in one launch (mil_linear_small_bwd).  extras: up to three more addends of dy (the gradients
    other consumers of the layer's output sent: _FanOut), summed while the operand is staged; dysum [M, N]: receives the sum."""
    M, K = x.shape
    N = W.shape[0]
    dx = torch.empty((M, K), device=x.device, dtype=torch.float32) if want_dx else None
    dW = (dW_out if dW_out is not None else torch.empty((N, K), device=x.device, dtype=torch.float32)) if want_dW else None
    db = (db_out if db_out is not None else torch.empty(N, device=x.device, dtype=torch.float32)) if want_db else None
    yv = y_or_pre if act != 0 else None
    if extras or dysum is not None:
        e = list(extras) + [None] * (3 - len(extras))
        _lib.checked().mil_linear_small_bwd_sum(_p(dy), dy.stride(0), _p(e[0]), _p(e[1]), _p(e[2]), _p(dysum), _p(yv),
                                                yv.stride(0) if yv is not None else 0, act, _p(x), x.stride(0), _p(W),
                                                W.stride(0), _p(dx), K, _p(dW), K, _p(db), M, N, K, _stream())
        return dx, dW, db
    sh = _lib.shim()
    if sh is not None:
        sh.linear_small_bwd(dy, yv, act, x, W, dx, dW, db, _stream_int())
        return dx, dW, db
    _lib.checked().mil_linear_small_bwd(_p(dy), dy.stride(0), _p(yv), yv.stride(0) if yv is not None else 0, act,
                                        _p(x), x.stride(0), _p(W), W.stride(0), _p(dx), K, _p(dW), K, _p(db),
                                        M, N, K, _stream())
    return dx, dW, db


class _GradBox:
    """Mailbox between the node that PRODUCES a token-side tensor and the _FanOut node behind it: when the tensor has several
    consumers, _FanOut.backward leaves all but one of their gradients here and the producer's backward kernel sums them while
    it stages its operand (mil_linear_small_bwd_sum, mil_linear_small_ln_bwd3) - autograd would launch an elementwise add
    per extra consumer (6 of the fusion step's 93 launches)."""
    __slots__ = ("extras",)

    def __init__(self):
        self.extras = []

    def take(self, like=None):
        ex, self.extras = self.extras, []
        return [e for e in ex if e is not None]


def _sum_overflow(dy, extras, room: int):
    """extras beyond what the kernel takes are added the plain way; returns (dy, extras that fit)."""
    while len(extras) > room:
        dy = dy + extras.pop()
    return dy, extras


_ONES = {}


def backward(loss):
    """loss.backward() without autograd's fill launch for the root gradient: `ones_like(loss)` is a 4.7 us launch per step
    (inside every captured step); a cached constant per (device, shape) takes its place."""
    key = (loss.device, tuple(loss.shape), loss.dtype)
    one = _ONES.get(key)
    if one is None:
        if torch.cuda.is_current_stream_capturing():
            return loss.backward()          # no allocation + fill of a persistent constant inside a capture: the plain way
        one = _ONES[key] = torch.ones(loss.shape, device=loss.device, dtype=loss.dtype)
    return loss.backward(one)


def sum_n(ts):
    """Sum of 2 .. 4 same-shape fp32 tensors in ONE launch (mil_sum4); more, or odd layouts: torch's adds."""
    ts = list(ts)
    a = ts[0]
    ok = (2 <= len(ts) <= 4 and a.numel() % 4 == 0 and
          all(t.dtype == torch.float32 and t.is_contiguous() and t.shape == a.shape and t.data_ptr() % 16 == 0 for t in ts))
    if not ok:
        out = ts[0]
        for t in ts[1:]:
            out = out + t
        return out
    out = torch.empty_like(a)
    e = ts + [None] * (4 - len(ts))
    _lib.checked().mil_sum4(_p(e[0]), _p(e[1]), _p(e[2]), _p(e[3]), _p(out), a.numel(), _stream())
    return out


def _ok_extra(e, like) -> bool:
    return e.dtype == torch.float32 and e.is_contiguous() and e.shape == like.shape and e.data_ptr() % 16 == 0


class _FanOut(torch.autograd.Function):
    """n aliases of x, one per consumer.  Backward: the first gradient goes up the graph as x's gradient, the others into the
    producer's mailbox (see _GradBox) - whatever autograd itself adds to the first one stays correct, sums commute."""

    @staticmethod
    def forward(ctx, x, box, n: int):
        ctx.box = box
        return tuple(x.view_as(x) for _ in range(n))

    @staticmethod
    def backward(ctx, *grads):
        gs = [g for g in grads if g is not None]
        if not gs:
            return None, None, None
        first = gs[0]
        for g in gs[1:]:
            g = g if g.dtype == torch.float32 else g.float()
            ctx.box.extras.append(g.contiguous())
        return first, None, None


def fan_out(x, n: int):
    """n handles of x for n consumers.  When x came out of a token-side node that sums its output's gradients in-kernel
    (linear_act's few-rows path, lin_ln_lin's xn), the consumers' gradients meet there instead of in autograd's add launches;
    otherwise the handles are x itself."""
    box = getattr(x, "_mil_box", None)
    if n <= 1 or box is None or not torch.is_grad_enabled() or not x.requires_grad:
        return (x,) * n
    return _FanOut.apply(x, box, n)


class _LinearAct(torch.autograd.Function):
    """y = act(x W^T + b) (+ residual): nn.Linear (+Tanh/ReLU) of aggregator.py:44-68, sam/transformer.py:413-416,
    sam/common.py:21-26.  x [M, K], W [N, K]."""

    @staticmethod
    def forward(ctx, x, W, b, act: int, residual, rows_dev=None, box=None, x2=None):
        x = _f32c(x, "x")
        W = _f32c(W, "W")
        M, K = x.shape
        ctx.box = box
        ctx.has_x2 = x2 is not None
        ctx.rows_dev = rows_dev             # capacity bucket: rows from rows_dev[0] on are padding (zero out, zero gradient)
        N = W.shape[0]
        res = _f32c(residual, "residual") if residual is not None else None
        pre = None
        ctx.small = _small_ok(M, N, K, x, W)
        ctx.mid = (not ctx.small) and _mid_ok(M, N, K, x, W, res) and \
            not (act == ACT["quickgelu"] and any(ctx.needs_input_grad[:3]))
        if residual is not None and act != 0:
            raise _lib.MilHipError("linear_act: residual is only supported with act='none'")
        if ctx.mid:
            y = linear_mid_fwd(x, W, b, act, res)
        elif ctx.small and not (act == ACT["quickgelu"] and any(ctx.needs_input_grad[:3])):
            if x2 is not None:
                y, x = linear_small_fwd(x, W, b, act, res, _f32c(x2, "x2"))      # x: the summed input, saved for the backward
            else:
                y = linear_small_fwd(x, W, b, act, res)
        elif act == ACT["quickgelu"] and any(ctx.needs_input_grad[:3]):
            # QuickGELU's derivative needs the pre-activation: keep it (learnable-prompt path only; the frozen
            # forward uses the fused epilogue)
            pre = linear_small_fwd(x, W, b, 0) if ctx.small else gemm(x, 0, W, 0, M, N, K, bias=b, act=0)
            y = torch.empty_like(pre)
            _lib.checked().mil_quickgelu(_p(pre), None, _p(y), pre.numel(), _stream())
        else:
            y = gemm(x, 0, W, 0, M, N, K, bias=b, act=act, residual=res, rows_dev=rows_dev)
        ctx.act = act
        ctx.has_b = b is not None
        ctx.b_param = b                     # only to look up its flat-gradient slot in backward
        ctx.has_res = residual is not None
        # with a residual the saved y is not the activation output; only act == none is used with residuals
        if x2 is not None and not (ctx.small and not ctx.mid):
            raise _lib.MilHipError("linear_act: x2 is only built for the few-rows path")
        ctx.save_for_backward(x, W, y if pre is None else pre)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, W, y = ctx.saved_tensors
        dy = _f32c(dy, "dy")
        M, K = x.shape
        N = W.shape[0]
        W_slot = grad_slot(W)
        b_slot = grad_slot(ctx.b_param) if ctx.b_param is not None else None
        extras = ctx.box.take() if ctx.box is not None else []
        if extras and not (ctx.small and not ctx.mid and dy.is_contiguous() and all(_ok_extra(e, dy) for e in extras)):
            for e in extras:                    # another path, or an odd layout: the plain sums
                dy = dy + e
            extras = []
        if ctx.mid and ctx.act != ACT["quickgelu"]:
            if dy.data_ptr() % 16 or dy.stride(0) % 4:
                dy = dy.clone()
            dx, dW, db = linear_mid_bwd(dy, y, ctx.act, x, W, ctx.needs_input_grad[0], ctx.needs_input_grad[1],
                                        ctx.has_b and ctx.needs_input_grad[2], W_slot, b_slot)
            return dx, (dW if ctx.needs_input_grad[1] else None), db, None, (dy if ctx.has_res else None), None, None, None
        if ctx.small:
            if dy.data_ptr() % 16:
                dy = dy.clone()
            dy, extras = _sum_overflow(dy, extras, 3)
            want_dx = ctx.needs_input_grad[0] or (ctx.has_x2 and ctx.needs_input_grad[7])
            if extras and not want_dx:
                # no dx launch to ride on (the layer's input carries no gradient): one n-ary sum, then the deferred dW
                dy, extras = sum_n([dy] + extras), []
            want_dW, want_db = ctx.needs_input_grad[1], ctx.has_b and ctx.needs_input_grad[2]
            if (deferred.enabled() and not want_dx and want_dW and W_slot is not None and (not want_db or b_slot is not None)
                    and x.shape[1] % 4 == 0 and dy.data_ptr() % 16 == 0):
                # nothing upstream waits for this layer: its whole backward is the grouped weight-gradient launch
                deferred.queue_dw(dy, y, x, W_slot.detach(), (b_slot.detach() if want_db else None), ctx.act)
                return None, W_slot, (b_slot if want_db else None), None, (dy if ctx.has_res else None), None, None, None
            if (deferred.enabled() and want_dx and want_dW and W_slot is not None and
                    (not want_db or b_slot is not None) and x.shape[1] % 4 == 0):
                # the previous layer's backward waits for dx only: dx now, the weight / bias gradient with every other
                # queued layer's in one grouped launch at the end of the pass (deferred.py), straight into the flat buffer.
                # The queue holds aliases of its own: autograd adopts a returned gradient without a copy only while
                # nothing else references that tensor object (see grad_slot)
                dysum = torch.empty((M, N), device=dy.device, dtype=torch.float32) if extras else None
                dx, _, _ = linear_small_bwd(dy, y, ctx.act, x, W, True, False, False, extras=extras, dysum=dysum)
                dyt = dysum if extras else dy
                deferred.queue_dw(dyt, y, x, W_slot.detach(), (b_slot.detach() if want_db else None), ctx.act)
                return (dx if ctx.needs_input_grad[0] else None, W_slot, (b_slot if want_db else None), None,
                        (dyt if ctx.has_res else None), None, None, (dx if ctx.has_x2 else None))
            if extras and ctx.has_res:
                for e in extras:                # the residual branch wants the summed gradient as a tensor
                    dy = dy + e
                extras = []
            dx, dW, db = linear_small_bwd(dy, y, ctx.act, x, W, want_dx, want_dW, want_db, W_slot, b_slot, extras=extras)
            return (dx if ctx.needs_input_grad[0] else None, dW, db, None, (dy if ctx.has_res else None), None, None,
                    (dx if ctx.has_x2 else None))
        if ctx.act == ACT["quickgelu"]:
            dpre = torch.empty_like(dy)
            _lib.checked().mil_quickgelu(_p(y), _p(dy), _p(dpre), dy.numel(), _stream())     # y holds the pre-activation
        else:
            fused = ctx.needs_input_grad[1] and N % 4 == 0 and K % 4 == 0
            if fused and not ctx.needs_input_grad[0]:
                # parameters only (fc_pathology: the bag features carry no gradient): act' is applied while dy is staged
                # for the weight-gradient product, which also yields the bias gradient - no dpre tensor at all
                dW, db = linear_bwd_params(dy, y if ctx.act else None, ctx.act, x, W_slot, b_slot,
                                           ctx.has_b and ctx.needs_input_grad[2], rows_dev=ctx.rows_dev)
                return None, dW, db, None, (dy if ctx.has_res else None), None, None, None
            dpre = act_bwd(dy, y, ctx.act)
            if fused:
                dx = gemm(dpre, 0, W, 1, M, K, N)
                dW, db = linear_bwd_params(dpre, None, 0, x, W_slot, b_slot, ctx.has_b and ctx.needs_input_grad[2])
                return dx, dW, db, None, (dy if ctx.has_res else None), None, None, None
        dx = gemm(dpre, 0, W, 1, M, K, N) if ctx.needs_input_grad[0] else None
        dW = gemm(dpre, 1, x, 1, N, K, M, out=W_slot, split_k=True) if ctx.needs_input_grad[1] else None
        db = colsum(dpre, out=b_slot) if (ctx.has_b and ctx.needs_input_grad[2]) else None
        dres = dy if ctx.has_res else None
        return dx, dW, db, None, dres, None, None, None


def _small_dw(dy, yv, x, W, b, act: int):
    """(dW, db) of a few-rows layer: queued for the end-of-backward grouped launch straight into the flat gradient slots
    when optim.FlatAdam owns the parameters (deferred.py), otherwise formed now (mil_linear_small_bwd, dW role only)."""
    W_slot = grad_slot(W)
    b_slot = grad_slot(b) if b is not None else None
    if (deferred.enabled() and W_slot is not None and (b is None or b_slot is not None) and x.shape[1] % 4 == 0
            and dy.data_ptr() % 16 == 0):
        deferred.queue_dw(dy, yv, x, W_slot.detach(), (b_slot.detach() if b is not None else None), act)
        return W_slot, b_slot
    _, dW, db = linear_small_bwd(dy, yv, act, x, W, False, True, b is not None, W_slot, b_slot)
    return dW, db


class _LinLnLin(torch.autograd.Function):
    """u = z Wp^T + bp (+ resp);  xn = LayerNorm(u);  y = act((xn [+ x2]) Wc^T + bc)  - the P -> norm -> C links of the
    two-way block's token stream (sam/transformer.py:287-300) as ONE autograd node of two launches forward
    (mil_linear_small_fwd, mil_linear_small_ln_fwd) and two backward (C's input gradient; P's input gradient with the norm's
    backward and the sum of the two gradients that reach xn applied while its operand is staged, mil_linear_small_ln_bwd) -
    the op-by-op route takes three and five (a LayerNorm launch each way and autograd's add).  Returns (y, xn): later
    consumers of the norm's output use xn, whose gradient arrives here.  Weight gradients join the grouped launch."""

    @staticmethod
    def forward(ctx, z, Wp, bp, resp, gamma, beta, eps: float, x2, Wc, bc, actc: int, box=None):
        ctx.box = box
        z, Wp, Wc = _f32c(z, "z"), _f32c(Wp, "Wp"), _f32c(Wc, "Wc")
        M = z.shape[0]
        dev = z.device
        resp_c = _f32c(resp, "residual") if resp is not None else None
        u = linear_small_fwd(z, Wp, bp, 0, resp_c)
        E, N = u.shape[1], Wc.shape[0]
        y = torch.empty((M, N), device=dev, dtype=torch.float32)
        xn = torch.empty((M, E), device=dev, dtype=torch.float32)
        x2c = _f32c(x2, "x2") if x2 is not None else None
        xin = torch.empty((M, E), device=dev, dtype=torch.float32) if x2c is not None else None
        stats = torch.empty((M, 2), device=dev, dtype=torch.float32)
        _lib.checked().mil_linear_small_ln_fwd(_p(u), u.stride(0), _p(_f32c(gamma, "gamma")), _p(_f32c(beta, "beta")), float(eps),
                                               _p(x2c), x2c.stride(0) if x2c is not None else 0, _p(Wc), Wc.stride(0), _p(bc),
                                               int(actc), None, 0, _p(y), N, _p(xn), _p(xin), _p(stats), M, N, _stream())
        ctx.actc, ctx.has_res, ctx.has_x2 = int(actc), resp is not None, x2 is not None
        ctx.params = (bp, beta, bc)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(z, Wp, u, stats, gamma, xin if xin is not None else xn, Wc, y)
        return y, xn

    @staticmethod
    def backward(ctx, dy, dxn):
        z, Wp, u, stats, gamma, xin, Wc, y = ctx.saved_tensors
        bp, beta, bc = ctx.params
        M, E = u.shape
        dev = u.device
        if dy is not None:
            dy = _f32c(dy, "dy")
            if dy.data_ptr() % 16:
                dy = dy.clone()
            parts = None
            Nc = Wc.shape[0]
            if Nc >= 2048 and Nc % 2048 == 0 and not ctx.has_x2 and dy.stride(0) % 4 == 0 and y.stride(0) % 4 == 0:
                # a wide C layer (mlp.lin1): its input gradient as four partial sums over n (4 x the workgroups, one operand
                # chunk each); the norm's backward below adds them while it stages its operand
                parts = torch.empty((4, M, E), device=dev, dtype=torch.float32)
                _lib.checked().mil_linear_small_bwd_split(_p(dy), dy.stride(0), _p(y if ctx.actc != 0 else None), y.stride(0),
                                                          ctx.actc, _p(Wc), Wc.stride(0), _p(parts), M, Nc, E, 4, _stream())
                dxin = None
            else:
                dxin, _, _ = linear_small_bwd(dy, y, ctx.actc, xin, Wc, True, False, False)  # C: input gradient now ...
            dWc, dbc = _small_dw(dy, y, xin, Wc, bc, ctx.actc)                              # ... weight gradient grouped
        else:
            dxin, dWc, dbc, parts = None, None, None, None
        gs = [g for g in (dxin, dxn) if g is not None] + (ctx.box.take() if ctx.box is not None else [])
        if parts is not None:
            gs = [parts[0], parts[1], parts[2]] + gs + [parts[3]]        # slots 4 and 5 take contiguous [M, 512] addends
        if not gs:
            return (None,) * 12
        gs = [_f32c(g, "dxn") for g in gs]
        def fits(i, g):           # addends 1-3 carry their own row stride, 4-5 are read as contiguous [M, 512]
            return g.stride(1) == 1 and g.data_ptr() % 16 == 0 and (g.stride(0) % 4 == 0 if i < 3 else g.is_contiguous())
        i = 1
        while i < len(gs):        # whatever does not fit a slot is added the plain way
            if i >= 5 or not fits(i, gs[i]):
                gs[0] = gs[0] + gs.pop(i)
            else:
                i += 1
        if not fits(0, gs[0]):
            gs[0] = gs[0].contiguous()
        g1, g2, g3, g4, g5 = (gs + [None] * 4)[:5]
        dz = torch.empty_like(z) if ctx.needs_input_grad[0] else None
        du = torch.empty((M, E), device=dev, dtype=torch.float32)
        dg = grad_slot(gamma)
        if dg is None:
            dg = torch.empty(E, device=dev, dtype=torch.float32)
        db = grad_slot(beta)
        if db is None:
            db = torch.empty(E, device=dev, dtype=torch.float32)
        K = z.shape[1]
        _lib.checked().mil_linear_small_ln_bwd5(_p(g1), g1.stride(0), _p(g2), g2.stride(0) if g2 is not None else 0, _p(g3),
                                                g3.stride(0) if g3 is not None else 0, _p(g4), _p(g5), _p(u), u.stride(0),
                                                _p(stats), _p(gamma), _p(Wp), Wp.stride(0), _p(dz), K, _p(du), _p(dg), _p(db),
                                                M, K, _stream())
        dWp, dbp = _small_dw(du, None, z, Wp, bp, 0)
        return (dz, dWp, dbp, (du if ctx.has_res else None), dg, db, None, (dxin if ctx.has_x2 else None), dWc, dbc, None, None)


def lin_ln_lin_ok(z, Wp, gamma, Wc) -> bool:
    """Shapes the fused P -> LayerNorm -> C node is built for: <= 64 rows, norm width 512, 16-byte aligned operands."""
    return (z.dim() == 2 and 0 < z.shape[0] <= SMALL_ROWS and Wp.shape[0] == 512 and gamma.shape[0] == 512 and
            Wc.shape[1] == 512 and Wc.shape[0] % 16 == 0 and z.shape[1] % 16 == 0 and
            _small_ok(z.shape[0], Wp.shape[0], z.shape[1], z, Wp) and Wc.data_ptr() % 16 == 0 and
            gamma.requires_grad and Wp.requires_grad and Wc.requires_grad)


def lin_ln_lin(z, Wp, bp, resp, gamma, beta, eps, x2, Wc, bc, actc: str = "none"):
    """(y, xn) of _LinLnLin; see there.  xn carries the node's mailbox: hand it to several consumers through fan_out()."""
    box = _GradBox()
    y, xn = _LinLnLin.apply(z, Wp, bp, resp, gamma, beta, float(eps), x2, Wc, bc, ACT[actc], box)
    xn._mil_box = box
    return y, xn


class _MlpQuickGelu(torch.autograd.Function):
    """x + c_proj(QuickGELU(c_fc(x_ln)))  (clip/model.py:176-178,196-198) as one autograd node: the c_fc product stores
    its pre-activation from the epilogue, and in the backward the product dout . W2 is multiplied by QuickGELU' in its
    epilogue - no stand-alone activation forward / backward passes over the [rows, 4 W] tensors."""

    @staticmethod
    def forward(ctx, x, W1, b1, W2, b2, residual):
        x, W1, W2 = _f32c(x, "x"), _f32c(W1, "W1"), _f32c(W2, "W2")
        M, K = x.shape
        N1 = W1.shape[0]
        need = any(ctx.needs_input_grad[:5])
        if need:
            pre = torch.empty((M, N1), device=x.device, dtype=torch.float32)
            h = gemm_aux(x, W1, 0, M, N1, K, pre, 1, bias=b1, act=ACT["quickgelu"])
        else:
            pre = None
            h = gemm(x, 0, W1, 0, M, N1, K, bias=b1, act=ACT["quickgelu"])
        out = gemm(h, 0, W2, 0, M, W2.shape[0], N1, bias=b2, residual=_f32c(residual, "residual") if residual is not None else None)
        ctx.has_res = residual is not None
        keep_h = ctx.needs_input_grad[3]
        ctx.save_for_backward(x, W1, W2, pre, h if keep_h else None)
        ctx.params = (b1, b2)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, W1, W2, pre, h = ctx.saved_tensors
        b1, b2 = ctx.params
        dout = _f32c(dout, "dout")
        M, K = x.shape
        N1, N2 = W1.shape[0], W2.shape[0]
        dpre = gemm_aux(dout, W2, 1, M, N1, N2, pre, 2)                      # (dout . W2) * QuickGELU'(pre)
        dx = gemm(dpre, 0, W1, 1, M, K, N1) if ctx.needs_input_grad[0] else None
        dW1 = gemm(dpre, 1, x, 1, N1, K, M, out=grad_slot(W1)) if ctx.needs_input_grad[1] else None
        db1 = colsum(dpre, out=grad_slot(b1)) if (b1 is not None and ctx.needs_input_grad[2]) else None
        dW2 = gemm(dout, 1, h, 1, N2, N1, M, out=grad_slot(W2)) if ctx.needs_input_grad[3] else None
        db2 = colsum(dout, out=grad_slot(b2)) if (b2 is not None and ctx.needs_input_grad[4]) else None
        return dx, dW1, db1, dW2, db2, (dout if ctx.has_res else None)


def mlp_quickgelu(x, W1, b1, W2, b2, residual=None):
    """c_proj(QuickGELU(c_fc(x))) + residual; tall inputs take the fused node, a few rows the one-launch kernels."""
    if x.shape[0] <= SMALL_ROWS:
        return linear_act(linear_act(x, W1, b1, "quickgelu"), W2, b2, "none", residual=residual)
    return _MlpQuickGelu.apply(x, W1, b1, W2, b2, residual)


def linear_act(x, W, b=None, act: str = "none", residual=None, rows_dev=None, x2=None):
    """rows_dev: device int32 [1] with the true row count of a capacity bucket (x has the bucket's capacity rows; the rows behind
    the count come out as zeros and carry no gradient) - tall layers only; the few-rows kernels ignore it.
    x2: the layer's input is x + x2 (few-rows layers add it while the operand is staged; others through a plain add).
    The result carries the node's gradient mailbox (see fan_out)."""
    lead = x.shape[:-1]
    x2d = x.reshape(-1, x.shape[-1])
    if x2 is not None:
        x2 = x2.reshape(-1, x2.shape[-1])
        M, K = x2d.shape
        N = W.shape[0]
        few = (x2d.is_cuda and x2d.dtype == torch.float32 and x2.dtype == torch.float32 and x2d.is_contiguous() and x2.is_contiguous()
               and W.dtype == torch.float32 and W.is_contiguous()
               and _small_ok(M, N, K, x2d, W) and not _mid_ok(M, N, K, x2d, W, residual) and act != "quickgelu")
        if not few:
            x2d, x2 = x2d + x2, None
    box = _GradBox()
    y = _LinearAct.apply(x2d, W, b, ACT[act], residual.reshape(-1, residual.shape[-1]) if residual is not None else None, rows_dev,
                         box, x2)
    y = y.reshape(*lead, W.shape[0])
    y._mil_box = box
    return y


# --------------------------------------------------------------------------- split-bf16 products for frozen weights (opt-in)
def split_bf16(W, pieces: int):
    """uint16 [pieces, *W.shape]: bf16 summands of a frozen fp32 weight (include/mil_hip.h: mil_split_bf16)."""
    W = _f32c(W.detach(), "W")
    out = torch.empty((pieces,) + tuple(W.shape), device=W.device, dtype=torch.uint16)
    _lib.checked().mil_split_bf16(_p(W), _p(out), W.numel(), pieces, _stream())
    return out


def gemm_split(A, Wp, bias=None, act: int = 0, residual=None, aux=None, aux_mode: int = 0):
    """act(A . W^T + bias) + residual with W given as its bf16 pieces Wp [pieces, N, K] (mil_gemm_split)."""
    A = _f32c(A, "A")
    pieces, N, K = Wp.shape
    M = A.shape[0]
    out = torch.empty((M, N), device=A.device, dtype=torch.float32)
    _lib.checked().mil_gemm_split(_p(A), A.stride(0), _p(Wp), pieces, K, _p(out), N, M, N, K, _p(bias), act, _p(residual),
                                  residual.stride(0) if residual is not None else 0, _p(aux),
                                  aux.stride(0) if aux is not None else 0, aux_mode, _stream())
    return out


class FrozenSplit:
    """bf16 pieces of a frozen nn.Linear weight W [N, K] and of its transpose (for the dx half of the backward)."""

    def __init__(self, W, pieces: int):
        self.pieces = pieces
        self.fwd = split_bf16(W, pieces)                             # [pieces, N, K]
        self.bwd = split_bf16(W.detach().t().contiguous(), pieces)   # [pieces, K, N]
        self.key = (W.data_ptr(), W._version)


class _LinearFrozenSplit(torch.autograd.Function):
    """act(x W^T + b) + residual for a FROZEN W given as bf16 pieces: forward and dx on the split-bf16 product."""

    @staticmethod
    def forward(ctx, x, fs: FrozenSplit, b, residual):
        ctx.fs, ctx.has_res = fs, residual is not None
        return gemm_split(x, fs.fwd, bias=b, residual=_f32c(residual, "residual") if residual is not None else None)

    @staticmethod
    def backward(ctx, dy):
        dy = _f32c(dy, "dy")
        dx = gemm_split(dy, ctx.fs.bwd) if ctx.needs_input_grad[0] else None
        return dx, None, None, (dy if ctx.has_res else None)


class _MlpQuickGeluFrozenSplit(torch.autograd.Function):
    """The fused MLP node (_MlpQuickGelu) on split-bf16 products; both weights frozen."""

    @staticmethod
    def forward(ctx, x, fs1: FrozenSplit, b1, fs2: FrozenSplit, b2, residual):
        x = _f32c(x, "x")
        need = ctx.needs_input_grad[0]
        pre = torch.empty((x.shape[0], fs1.fwd.shape[1]), device=x.device, dtype=torch.float32) if need else None
        h = gemm_split(x, fs1.fwd, bias=b1, act=ACT["quickgelu"], aux=pre, aux_mode=1 if need else 0)
        out = gemm_split(h, fs2.fwd, bias=b2, residual=_f32c(residual, "residual") if residual is not None else None)
        ctx.fs1, ctx.fs2, ctx.has_res = fs1, fs2, residual is not None
        ctx.save_for_backward(pre)
        return out

    @staticmethod
    def backward(ctx, dout):
        (pre,) = ctx.saved_tensors
        dout = _f32c(dout, "dout")
        dpre = gemm_split(dout, ctx.fs2.bwd, aux=pre, aux_mode=2)
        dx = gemm_split(dpre, ctx.fs1.bwd)
        return dx, None, None, None, None, (dout if ctx.has_res else None)


def linear_frozen_split(x, fs: FrozenSplit, b=None, residual=None):
    return _LinearFrozenSplit.apply(x, fs, b, residual)


def mlp_quickgelu_frozen_split(x, fs1: FrozenSplit, b1, fs2: FrozenSplit, b2, residual=None):
    return _MlpQuickGeluFrozenSplit.apply(x, fs1, b1, fs2, b2, residual)
