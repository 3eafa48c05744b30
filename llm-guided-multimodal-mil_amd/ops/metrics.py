"""The evaluation log's three entries (csrc/metrics.hip): one small launch each on the current stream, no host read."""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from .. import _lib
from ._base import _f32c, _p, _stream

EVAL_TILE = 64            # MIL_EVAL_TILE: tile edge of eval_rank
EVAL_MAX_ROWS = 65536     # MIL_EVAL_MAX_ROWS
EVAL_MAX_TERMS, EVAL_LOSS_SLOTS = 3, 4
EVAL_FLAG_OVERFLOW, EVAL_FLAG_NAN = 1, 2
# 8-byte words of eval_reduce's output (MIL_EVAL_OUT_*)
(EVAL_OUT_N, EVAL_OUT_STEPS, EVAL_OUT_FLAG, EVAL_OUT_P, EVAL_OUT_NEG, EVAL_OUT_S2, EVAL_OUT_TP_AT, EVAL_OUT_FP_AT,
 EVAL_OUT_JSTAR, EVAL_OUT_ISTAR, EVAL_OUT_GE_POS, EVAL_OUT_GE_NEG, EVAL_OUT_SSTAR, EVAL_OUT_LOSS) = range(14)
EVAL_OUT_WORDS = 18


def eval_out_bytes(C: int) -> int:
    n = int(_lib.lib().mil_eval_out_bytes(int(C)))
    if n == 0:
        raise _lib.MilHipError(f"mil_eval_out_bytes: {C} classes are outside 1..64")
    return n


def eval_push(probs: Sequence[torch.Tensor], y: torch.Tensor, extra: Optional[torch.Tensor], ce: bool, capacity: int,
              log_prob: torch.Tensor, log_cls: torch.Tensor, step_b: torch.Tensor, step_loss: torch.Tensor,
              ctr: torch.Tensor) -> None:
    """Append one step: probs = the Last head's [B, C] probabilities, then the CT and Pth heads' under 'CT-Pth-Last'."""
    ps = [_f32c(p, f"probs[{i}]") for i, p in enumerate(probs)]
    y = _f32c(y, "y")
    B, C = ps[0].shape
    if any(p.shape != (B, C) for p in ps) or y.shape != (B, C):
        raise _lib.MilHipError(f"eval_push: every term and the labels must be [{B}, {C}]")
    if extra is not None:
        extra = _f32c(extra, "extra")
    ps = ps + [None] * (EVAL_MAX_TERMS - len(ps))
    _lib.checked().mil_eval_push(_p(ps[0]), _p(ps[1]), _p(ps[2]), _p(y), _p(extra), B, C, len(probs), int(bool(ce)),
                                 int(capacity), _p(log_prob), _p(log_cls), _p(step_b), _p(step_loss), _p(ctr), _stream())


def eval_rank(log_prob: torch.Tensor, log_cls: torch.Tensor, ctr: torch.Tensor, capacity: int, rank: torch.Tensor) -> None:
    _lib.checked().mil_eval_rank(_p(log_prob), _p(log_cls), _p(ctr), int(capacity), _p(rank), _stream())


def eval_reduce(log_prob: torch.Tensor, log_cls: torch.Tensor, step_b: torch.Tensor, step_loss: torch.Tensor, ctr: torch.Tensor,
                rank: Optional[torch.Tensor], capacity: int, C: int, thres: float, out: torch.Tensor) -> None:
    _lib.checked().mil_eval_reduce(_p(log_prob), _p(log_cls), _p(step_b), _p(step_loss), _p(ctr), _p(rank), int(capacity),
                                   int(C), float(thres), _p(out), _stream())
