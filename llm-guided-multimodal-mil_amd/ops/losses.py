"""The two CLIP losses (csrc/head_loss.hip)."""
from __future__ import annotations

import torch

from .. import _lib
from ._base import _f32c, _p, _stream


class _ClipContrastive(torch.autograd.Function):
    @staticmethod
    def forward(ctx, out, feat):
        out, feat = _f32c(out, "out"), _f32c(feat, "feat")
        b, E = out.shape
        F_ = feat.shape[1]
        loss = torch.empty(1, device=out.device, dtype=torch.float32)
        d_out = torch.empty_like(out)
        ws = torch.empty(((F_ + 3) // 4) * 4 + F_ * b * E, device=out.device, dtype=torch.float32)
        _lib.checked().mil_clip_contrastive_loss(_p(out), _p(feat), b, F_, E, _p(loss), _p(d_out), _p(ws), _stream())
        ctx.save_for_backward(d_out)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (d_out,) = ctx.saved_tensors
        return d_out * g, None


def clip_contrastive_loss(out, feat):
    """CLIPloss_v1 (reference utils.py:261-284): out [b, E] bag embeddings vs frozen text features feat [b, F, E]."""
    return _ClipContrastive.apply(out, feat)


class _CosineEmbedding(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x1, x2, weight: float):
        x1, x2 = _f32c(x1, "x1"), _f32c(x2, "x2")
        B, E = x1.shape
        loss = torch.empty(1, device=x1.device, dtype=torch.float32)
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        d1 = torch.empty_like(x1) if need else None
        d2 = torch.empty_like(x2) if need else None
        _lib.checked().mil_cosine_embedding_loss(_p(x1), _p(x2), B, E, float(weight) / B, _p(loss), _p(d1), _p(d2), _stream())
        ctx.save_for_backward(d1, d2)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        d1, d2 = ctx.saved_tensors
        return d1 * g, d2 * g, None


def cosine_embedding_loss(x1, x2, weight: float = 1.0):
    """torch.nn.CosineEmbeddingLoss()(x1, x2, ones): mean_b (1 - cos(x1_b, x2_b)) - the 'textCosSim' term of the reference's
    training loop (train_ddp.py:102,325-329) between x_CT2CI and x_Pth2CI, [B, E] each (squeeze the token axis first)."""
    return _CosineEmbedding.apply(x1, x2, float(weight))
