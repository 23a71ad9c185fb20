"""Test-view scores of a reconstruction: PSNR and SSIM as the reference logs them (``eval_psnr`` / ``eval_ssim_skimage``,
lib/core/evaluation/metrics.py:52-71, called by ``BaseNeRF.eval_and_viz``), both from one HIP launch (csrc/metrics.hip).

LPIPS, the reference's third score (``eval_and_viz``, base_nerf.py:560-570), is ``image_lpips`` with a ``lpips.LPIPSVGG`` net: the VGG16 trunk on
this library's convolution kernels and csrc/lpips.hip.  No weights ship with the project; a model computes the score when it has been given a net
(``BaseNeRF.set_lpips`` or ``test_cfg['lpips_weights']``) and ``use_lpips_metric`` is set."""
from __future__ import annotations

import math
from typing import Tuple

import torch

from . import _cabi as C


def image_metrics(pred: torch.Tensor, target: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(psnr, ssim)`` per image of two ``(..., h, w, 3)`` fp32 GPU tensors of equal shape, as fp32 tensors of the leading shape.

    ``psnr = 10 * (2 * log10(1) - log10(mse + 1e-6))`` (the reference's formula and epsilon) of the kernel's fp64-accumulated mean squared error;
    ``ssim`` is ``skimage.metrics.structural_similarity(..., channel_axis, data_range=1)`` (7 x 7 uniform window, sample covariance, per-channel
    mean over the pixels whose window lies inside the image, then the mean of the channels).  Inputs are not converted: another dtype, a CPU
    tensor, a trailing shape other than ``(h >= 7, w >= 7, 3)`` or unequal shapes raise; non-contiguous inputs are made contiguous."""
    if pred.shape != target.shape:
        raise ValueError(f"image_metrics: shapes differ: {tuple(pred.shape)} vs {tuple(target.shape)}")
    if pred.dim() < 3 or pred.shape[-1] != 3:
        raise ValueError(f"image_metrics: expected (..., h, w, 3) images, got {tuple(pred.shape)}")
    if pred.dtype != torch.float32 or target.dtype != torch.float32:
        raise TypeError(f"image_metrics: fp32 images only, got {pred.dtype} and {target.dtype}")
    if not (pred.is_cuda and target.is_cuda) or pred.device != target.device:
        raise ValueError(f"image_metrics: both images must be on one GPU, got {pred.device} and {target.device}")
    lead, (h, w) = pred.shape[:-3], pred.shape[-3:-1]
    mse = torch.empty(lead, dtype=torch.float32, device=pred.device)
    ssim = torch.empty_like(mse)
    if mse.numel() > 0:
        a, b = pred.contiguous(), target.contiguous()
        with torch.cuda.device(pred.device):
            C.check(C.lib().ssdnerf_image_metrics(C.ptr(a), C.ptr(b), C.u32(mse.numel()), C.u32(h), C.u32(w), C.ptr(mse), C.ptr(ssim), C.stream()),
                    "image_metrics")
    psnr = 10 * (2 * math.log10(1.0) - torch.log10(mse + 1e-6))
    return psnr, ssim


def image_lpips(pred: torch.Tensor, target: torch.Tensor, net, chunk: int = 32) -> torch.Tensor:
    """LPIPS v0.1 (VGG16) per image of two ``(..., h, w, 3)`` fp32 GPU tensors of equal shape with values in [0, 1], as an fp32 tensor of the leading
    shape; ``net``: a ``lpips.LPIPSVGG``.  Same input rules as ``image_metrics``, with ``h, w >= 16``; ``chunk`` pairs pass through the trunk at a time."""
    return net(pred, target, chunk=chunk)
