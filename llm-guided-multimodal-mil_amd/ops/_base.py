"""Shared by every operator module: tensor-to-pointer helpers, the current stream, dtype checks, the constants and
grad_slot.  C entries are called as `_lib.checked().mil_x(...)`: a bad status raises there (_lib.py), no call site checks."""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from .. import _lib, deferred


GATE_D = 192
ACT = {"none": 0, "tanh": 1, "relu": 2, "quickgelu": 3}
X_DROP_P, X_DROP_SCALE = 0.5, 2.0            # ABMIL.py:26,49
M_DROP_P, M_DROP_SCALE = 0.25, 1.0 / 0.75    # aggregator.py:129


def _p(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _stream_int() -> int:
    return torch.cuda.current_stream().cuda_stream


def _f32c(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise _lib.MilHipError(f"{name}: expected a tensor on the MI355X (cuda) device; there is no CPU path")
    if t.dtype != torch.float32:
        raise _lib.MilHipError(f"{name}: expected float32, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _bf16c(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_cuda or t.dtype != torch.bfloat16:
        raise _lib.MilHipError(f"{name}: expected a bfloat16 tensor on the GPU")
    return t if t.is_contiguous() else t.contiguous()


def grad_slot(param):
    """The flat-gradient view optim.FlatAdam reserved for this parameter (None without FlatAdam): a backward that
    writes its result there and returns it hands autograd the final storage, so no gather copy is needed."""
    slot = getattr(param, "_mil_grad", None)
    if slot is None or slot.shape != param.shape:
        return None
    # Only the FIRST backward node of a pass may write the slot in place: were the same parameter used by a second node
    # (a shared Linear), its kernel would overwrite the first result before autograd's AccumulateGrad adds the two.  The
    # flag is cleared by FlatAdam.zero_grad() / GraphedStep; a second request in the same pass gets None, i.e. a fresh
    # tensor that autograd then accumulates into the slot.
    if getattr(param, "_mil_slot_used", False):
        # The first use's gradient may still be QUEUED (deferred.py forms it at the end of the pass): autograd is about to add
        # this node's fresh tensor to the slot, so whatever is queued for the slot has to be in it first (a Linear
        # used twice per forward - TwoWayTransformer_Both in the CT + pathology branch, aggregator.py:160-168 - lost the
        # first use's gradient and picked up stale slot contents instead).
        deferred.flush_pending()
        return None
    param._mil_slot_used = True
    # a fresh alias: autograd adopts a returned gradient without copying only if nothing else references that tensor
    return slot.detach()
