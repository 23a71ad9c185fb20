"""Total-variation regulariser of stage-1 fitting: the reference's ``tv_loss`` (lib/models/losses/tv_loss.py) over the two trailing dimensions,
forward and backward each one HIP launch (csrc/tv_loss.hip).  ``codes.TVLoss`` is the registered module the configs build."""
from __future__ import annotations

import torch

from . import _cabi as C


def _slices(x: torch.Tensor):
    n = x[..., 0, 0].numel()
    return C.u32(n), C.u32(x.shape[-2]), C.u32(x.shape[-1])


class _TVSliceMeans(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: torch.Tensor, power: float):
        x = x.contiguous()
        out = torch.empty(x.shape[:-2], dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            C.check(C.lib().ssdnerf_tv_loss_forward(C.ptr(x), *_slices(x), C.f32(power), C.ptr(out), C.stream()), "tv_loss_forward")
        ctx.save_for_backward(x)
        ctx.power = power
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        (x,) = ctx.saved_tensors
        g = grad_out.to(torch.float32).contiguous()
        dx = torch.empty_like(x)
        with torch.cuda.device(x.device):
            C.check(C.lib().ssdnerf_tv_loss_backward(C.ptr(x), C.ptr(g), *_slices(x), C.f32(ctx.power), C.ptr(dx), C.stream()), "tv_loss_backward")
        return dx, None


def tv_slice_means(x: torch.Tensor, power: float = 1.0) -> torch.Tensor:
    """Mean over each ``(h, w)`` slice of ``r^power``, ``r = |(dy, dx)|`` the forward differences along the two trailing dimensions, zero-padded
    on the last row / column: ``(..., h, w)`` fp32 GPU input -> ``(...)`` fp32, differentiable once.  This is the reference's ``tv_loss`` before
    mmgen's ``weighted_loss`` reduces it.  Another dtype raises ``TypeError``; a CPU tensor, fewer than 2 dimensions or an empty shape raise
    ``ValueError``; ``power`` must be >= 1 (the library refuses others); non-contiguous input is made contiguous."""
    if x.dtype != torch.float32:
        raise TypeError(f"tv_slice_means: fp32 input only, got {x.dtype}")
    if not x.is_cuda:
        raise ValueError(f"tv_slice_means: the input must be on the GPU, got {x.device}")
    if x.dim() < 2 or x.numel() == 0:
        raise ValueError(f"tv_slice_means: expected a non-empty (..., h, w) tensor, got {tuple(x.shape)}")
    return _TVSliceMeans.apply(x, float(power))
