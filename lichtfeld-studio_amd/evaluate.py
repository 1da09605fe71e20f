"""Evaluation metrics of the reference's MetricsEvaluator (src/training/metrics/metrics.cpp): PSNR (:40-59, data range 1, MSE clamped at
1e-10), SSIM (:68-125: 11x11 Gaussian window, sigma 1.5, zero padding, mean over the map - the "same" mode of the fused SSIM kernel) and
the evaluation loop (:380-520): every validation view rendered with fast_rasterize (the EWA rasterizer, whatever was trained with),
clamped to [0,1], metrics averaged over the views. LPIPS needs the TorchScript VGG blob the reference ships separately
(.MISSING_LARGE_BLOBS) and is not computed.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import torch


def psnr(pred: torch.Tensor, target: torch.Tensor, data_range: float = 1.0, mask=None) -> float:
    """[B,C,H,W] (or [C,H,W]) -> mean over the batch of 20 log10(data_range / sqrt(mse)).
    mask (a losses.PreparedMask or a [H,W] tensor of byte values, 255 = counts fully): the masked MSE sum M (p - t)^2 / (C sum M) instead; an all-zero mask
    gives the clamped MSE's PSNR (100 dB), as an exact match does."""
    if pred.shape != target.shape:
        raise ValueError("Prediction and target must have the same shape")
    if pred.dim() == 3:
        pred, target = pred[None], target[None]
    if mask is not None:
        m = getattr(mask, "mask_u8", mask).to(device=pred.device, dtype=pred.dtype)
        if tuple(m.shape) != tuple(pred.shape[-2:]):
            raise ValueError("the mask must have the images' height and width")
        num = (m * (pred - target).pow(2)).reshape(pred.shape[0], -1).sum(1, keepdim=True)
        mse = (num / (pred.shape[1] * m.sum()).clamp_min(1.0)).clamp_min(1e-10)
        return float((20.0 * torch.log10(data_range / mse.sqrt())).mean())
    mse = (pred.contiguous() - target.contiguous()).pow(2).reshape(pred.shape[0], -1).mean(1, keepdim=True).clamp_min(1e-10)
    return float((20.0 * torch.log10(data_range / mse.sqrt())).mean())


def ssim(pred: torch.Tensor, target: torch.Tensor) -> float:
    from .losses import fused_ssim
    if pred.dim() == 3:
        pred, target = pred[None], target[None]
    return float(fused_ssim(pred.contiguous(), target.contiguous(), padding="same", train=False))


@dataclass
class EvalMetrics:
    psnr: float
    ssim: float
    num_gaussians: int
    iteration: int
    n_images: int


@torch.no_grad()
def evaluate(model, cameras: List, images: List[torch.Tensor], iteration: int = 0, background: Optional[torch.Tensor] = None,
             rasterizer: str = "fastgs", masks: Optional[List] = None, antialiased: bool = False,
             filter3d: Optional[torch.Tensor] = None, alphas: Optional[List] = None) -> EvalMetrics:
    """cameras: rasterizer.Camera per validation view; images: the ground truth [3,H,W] in [0,1]. rasterizer="fastgs" is the reference's protocol
    (metrics.cpp:430 renders with fast_rasterize whatever was trained with); "gut" renders with the 3DGUT rasterizer instead - what a model trained with
    --gut was optimised for: 3DGUT has no screen-space dilation, the EWA renderer adds its 0.3-pixel low-pass to Gaussians the training shrank below a
    pixel (profiles/r04/scale_train_*: up to 13 dB between the two numbers on an MCMC model with noise injection).
    masks (parallel to images; None entries = unmasked views): the PSNR is the masked one (psnr(mask=...)). SSIM stays UNMASKED: its 11x11 window has no
    per-pixel form that a mask could weight without printing the mask's edge into the statistics.
    antialiased: the fastgs renders run in the antialiased mode (fastgs.FastGSSettings.antialiased) - for a model trained with GutTrainer(antialiasing=True).
    filter3d: the [N] variances of the 3D smoothing filter the model was trained with (GutTrainer.update_filter3d(); fastgs.FastGSSettings.filter3d): the renders are
    the filtered ones. A model whose parameters were baked (filter3d.bake) is evaluated without it.
    alphas (parallel to images; uint8 [H,W] planes of RGBA ground truth, loader.preload_alphas, or None entries): each such ground-truth image is composited over
    `background` (a * gt + (1 - a) * bg, a = u8 / 255: ops.background_compose) before PSNR and SSIM - the render is composited over the same colour."""
    from .fastgs import fast_rasterize
    from .rasterizer import rasterize
    if rasterizer not in ("fastgs", "gut"):
        raise ValueError("rasterizer must be 'fastgs' or 'gut'")
    if antialiased and rasterizer != "fastgs":
        raise ValueError("antialiased evaluation is wired into the fastgs rasterizer only")
    if filter3d is not None and rasterizer != "fastgs":
        raise ValueError("filter3d evaluation is wired into the fastgs rasterizer only")
    render = (lambda c, m, b: fast_rasterize(c, m, b, antialiased=antialiased, filter3d=filter3d)) if rasterizer == "fastgs" else rasterize
    dev = model.means.device
    bg = background if background is not None else torch.zeros(3, device=dev)
    ps, ss = [], []
    if masks is not None and len(masks) != len(images):
        raise ValueError("masks must be parallel to images")
    if alphas is not None and len(alphas) != len(images):
        raise ValueError("alphas must be parallel to images")
    bg_floats = tuple(float(v) for v in bg.detach().cpu().reshape(-1)) if alphas is not None and any(a is not None for a in alphas) else None
    for i, (cam, gt) in enumerate(zip(cameras, images)):
        img = torch.clamp(render(cam, model, bg).image, 0.0, 1.0)
        gt = gt.to(dev)
        if alphas is not None and alphas[i] is not None:
            from .ops import background_compose
            gt = background_compose(bg_floats, target_rgb=gt.contiguous(), target_alpha=alphas[i].to(dev).contiguous())[1]
        ps.append(psnr(img, gt, mask=masks[i] if masks is not None else None))
        ss.append(ssim(img, gt))
    n = max(len(ps), 1)
    return EvalMetrics(sum(ps) / n, sum(ss) / n, int(model.means.shape[0]), iteration, len(ps))
