"""Mirror of the reference's fused SSIM API over the HIP kernels of csrc/ssim.hip:
`fusedssim` / `fusedssim_backward` (include/kernels/ssim.cuh:11-30, src/training/kernels/ssim.cu:430-510), the autograd
wrapper `fused_ssim(img1, img2, padding, train)` (include/kernels/fused_ssim.cuh:30-131: "valid" crops 5 pixels per side when
H, W > 10; returns the MEAN of the map) and the photometric loss of Trainer::compute_photometric_loss
(src/training/trainer.cpp:115-128): (1 - lambda) * L1 + lambda * (1 - SSIM).
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Tuple

import torch

from .capi import LfsError, check, load_library, ptr, require_gpu, stream, workspace

K_C1 = 0.01 * 0.01
K_C2 = 0.03 * 0.03


def fusedssim(C1: float, C2: float, img1: torch.Tensor, img2: torch.Tensor, train: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """-> (ssim_map, dm_dmu1, dm_dsigma1_sq, dm_dsigma12), all [B,CH,H,W]; the derivative tensors are empty when train is False."""
    img1, img2 = img1.contiguous(), img2.contiguous()
    require_gpu(img1, img2)
    if img1.dim() != 4 or img1.shape != img2.shape:
        raise LfsError("fusedssim expects two [B,CH,H,W] tensors of the same shape")
    B, CH, H, W = img1.shape
    ssim_map = torch.empty_like(img1)
    if train:
        dm1, ds1, ds12 = torch.empty_like(img1), torch.empty_like(img1), torch.empty_like(img1)
    else:
        dm1 = ds1 = ds12 = None
    check(load_library().lfs_fused_ssim_fwd(C.c_uint32(B), C.c_uint32(CH), C.c_uint32(H), C.c_uint32(W), C.c_float(C1), C.c_float(C2),
                                            ptr(img1), ptr(img2), ptr(ssim_map), ptr(dm1), ptr(ds1), ptr(ds12), stream()), "fusedssim")
    if not train:
        e = torch.empty(0, dtype=img1.dtype, device=img1.device)
        return ssim_map, e, e, e
    return ssim_map, dm1, ds1, ds12


def fusedssim_backward(C1: float, C2: float, img1, img2, dL_dmap, dm_dmu1, dm_dsigma1_sq, dm_dsigma12) -> torch.Tensor:
    img1, img2, dL_dmap = img1.contiguous(), img2.contiguous(), dL_dmap.contiguous()
    dm_dmu1, dm_dsigma1_sq, dm_dsigma12 = dm_dmu1.contiguous(), dm_dsigma1_sq.contiguous(), dm_dsigma12.contiguous()
    require_gpu(img1, img2, dL_dmap, dm_dmu1, dm_dsigma1_sq, dm_dsigma12)
    B, CH, H, W = img1.shape
    out = torch.empty_like(img1)
    check(load_library().lfs_fused_ssim_bwd(C.c_uint32(B), C.c_uint32(CH), C.c_uint32(H), C.c_uint32(W), C.c_float(C1), C.c_float(C2),
                                            ptr(img1), ptr(img2), ptr(dL_dmap), ptr(dm_dmu1), ptr(dm_dsigma1_sq), ptr(dm_dsigma12), ptr(out),
                                            stream()), "fusedssim_backward")
    return out


class _FusedSSIM(torch.autograd.Function):
    """fused_ssim.cuh:30-107"""

    @staticmethod
    def forward(ctx, img1, img2, padding: str, train: bool):
        if padding not in ("same", "valid"):
            raise ValueError(f'fused_ssim: padding must be "same" or "valid" (got "{padding}")')
        img1, img2 = img1.contiguous(), img2.contiguous()
        if img1.dim() == 3:
            img1 = img1.unsqueeze(0)
        if img2.dim() == 3:
            img2 = img2.unsqueeze(0)
        if img1.dim() != 4 or img2.dim() != 4:
            raise ValueError("fused_ssim expects 4D tensors [N,C,H,W]")
        if img1.shape != img2.shape:
            raise ValueError("img1 and img2 must have the same shape")
        m, dm1, ds1, ds12 = fusedssim(K_C1, K_C2, img1, img2, train)
        h, w = m.shape[2], m.shape[3]
        if padding == "valid" and h > 10 and w > 10:
            m = m[:, :, 5:h - 5, 5:w - 5]
        ctx.save_for_backward(img1.detach(), img2, dm1, ds1, ds12)
        ctx.padding = padding
        return m

    @staticmethod
    def backward(ctx, grad_out):
        img1, img2, dm1, ds1, ds12 = ctx.saved_tensors
        dL_dmap = grad_out
        if ctx.padding == "valid":
            full = torch.zeros_like(img1)
            h, w = full.shape[2], full.shape[3]
            if h > 10 and w > 10:
                full[:, :, 5:h - 5, 5:w - 5] = dL_dmap
            dL_dmap = full
        return fusedssim_backward(K_C1, K_C2, img1, img2, dL_dmap, dm1, ds1, ds12), None, None, None


def fused_ssim(img1: torch.Tensor, img2: torch.Tensor, padding: str = "same", train: bool = True) -> torch.Tensor:
    """Mean SSIM (scalar tensor), differentiable w.r.t. img1 (fused_ssim.cuh:124-131)."""
    return _FusedSSIM.apply(img1.contiguous(), img2, padding, train).mean()


def photometric_loss(rendered: torch.Tensor, gt: torch.Tensor, lambda_dssim: float = 0.2) -> torch.Tensor:
    """Trainer::compute_photometric_loss (trainer.cpp:115-128) on [3,H,W] or [B,3,H,W] images, through autograd."""
    if rendered.dim() == 3:
        rendered = rendered.unsqueeze(0)
    if gt.dim() == 3:
        gt = gt.unsqueeze(0)
    l1 = torch.nn.functional.l1_loss(rendered, gt)
    ssim_loss = 1.0 - fused_ssim(rendered, gt, "valid", True)
    return (1.0 - lambda_dssim) * l1 + lambda_dssim * ssim_loss


def photometric_loss_fwd_bwd(render_hwc: torch.Tensor, target_chw: torch.Tensor, lambda_dssim: float, weight: float, loss_acc: torch.Tensor) -> torch.Tensor:
    """Fused extension used by fused.py: loss_acc += weight * photometric_loss(clamp(render, 0, 1), target); returns dL/d(render)
    in the rasterizer's HWC layout. Two kernel launches, no intermediate image tensors."""
    target_chw = target_chw.contiguous()
    require_gpu(render_hwc, target_chw, loss_acc)
    H, W = render_hwc.shape[-3], render_hwc.shape[-2]
    assert render_hwc.shape[-1] == 3 and tuple(target_chw.shape) == (3, H, W), (render_hwc.shape, target_chw.shape)
    lib = load_library()
    ws = workspace(lib.lfs_photometric_loss_workspace_bytes(C.c_uint32(H), C.c_uint32(W)), render_hwc.device, "photometric")
    v = torch.empty_like(render_hwc)
    check(lib.lfs_photometric_loss_fwd_bwd(C.c_uint32(H), C.c_uint32(W), ptr(render_hwc), ptr(target_chw), C.c_float(lambda_dssim), C.c_float(weight),
                                           ptr(v), ptr(loss_acc), ptr(ws), C.c_size_t(ws.numel()), stream()), "photometric_loss_fwd_bwd")
    return v


def photometric_loss_chw_fwd_bwd(render_chw: torch.Tensor, target_chw: torch.Tensor, lambda_dssim: float, weight: float, loss_acc: torch.Tensor) -> torch.Tensor:
    """The same for the fastgs rasterizer's CHW image, which reaches the loss un-clamped (fast_rasterizer.cpp:63): returns dL/d(render) [3,H,W]."""
    target_chw = target_chw.contiguous()
    require_gpu(render_chw, target_chw, loss_acc)
    H, W = render_chw.shape[-2], render_chw.shape[-1]
    assert render_chw.is_contiguous() and tuple(render_chw.shape[-3:]) == (3, H, W) and tuple(target_chw.shape) == (3, H, W), (render_chw.shape, target_chw.shape)
    lib = load_library()
    ws = workspace(lib.lfs_photometric_loss_workspace_bytes(C.c_uint32(H), C.c_uint32(W)), render_chw.device, "photometric")
    v = torch.empty_like(render_chw)
    check(lib.lfs_photometric_loss_chw_fwd_bwd(C.c_uint32(H), C.c_uint32(W), ptr(render_chw), ptr(target_chw), C.c_float(lambda_dssim), C.c_float(weight),
                                               ptr(v), ptr(loss_acc), ptr(ws), C.c_size_t(ws.numel()), stream()), "photometric_loss_chw_fwd_bwd")
    return v


class PreparedMask(NamedTuple):
    """A training-size mask on the device: mask_u8 uint8 [H,W] (255 = the pixel counts fully, 0 = ignored) and sums int64[2] = {sum over the image, sum over
    the SSIM crop}, the two exact integers the masked loss kernels normalise with (read on the device)."""
    mask_u8: torch.Tensor
    sums: torch.Tensor


def prepare_mask(mask_u8_device: torch.Tensor, out_width: int, out_height: int, invert: bool = False, threshold: int = -1) -> PreparedMask:
    """lfs_mask_prepare: a uint8 [h,w] plane -> the mask at the training resolution (the sample positions and 8-bit re-quantisation of u8_to_chw_f32), then
    threshold (>= threshold -> 255, else 0; negative keeps soft values), then invert; and its two integer sums. Asynchronous."""
    src = mask_u8_device.contiguous()
    require_gpu(src)
    if src.dim() != 2 or src.dtype != torch.uint8:
        raise LfsError("prepare_mask expects a uint8 [h,w] tensor")
    sh, sw = src.shape
    dst = torch.empty(int(out_height), int(out_width), dtype=torch.uint8, device=src.device)
    sums = torch.empty(2, dtype=torch.int64, device=src.device)
    check(load_library().lfs_mask_prepare(ptr(src), C.c_uint32(sw), C.c_uint32(sh), ptr(dst), C.c_uint32(int(out_width)), C.c_uint32(int(out_height)),
                                          C.c_uint32(int(bool(invert))), C.c_int32(int(threshold)), ptr(sums), stream()), "mask_prepare")
    return PreparedMask(dst, sums)


class PreparedDepth(NamedTuple):
    """A depth (or inverse-depth) target at the training resolution on the device: target float32 [H,W] with NaN where the source was not finite and > 0, the
    optional mask it was prepared with (uint8 [H,W], or None) and sums int64[1] = sum over the valid pixels of the mask byte (255 without a mask) - 255 x the sum
    of the per-pixel weights, the exact integer the depth loss normalises with (read on the device)."""
    target: torch.Tensor
    mask_u8: torch.Tensor | None
    sums: torch.Tensor


def prepare_depth(target_f32: torch.Tensor, mask: PreparedMask | torch.Tensor | None = None) -> PreparedDepth:
    """lfs_depth_prepare: a float32 [H,W] plane (device) -> PreparedDepth. mask: a PreparedMask or a uint8 [H,W] device tensor of the same size. Asynchronous."""
    src = target_f32.contiguous()
    require_gpu(src)
    if src.dim() == 3 and src.shape[0] == 1:
        src = src[0]
    if src.dim() != 2 or src.dtype != torch.float32:
        raise LfsError("prepare_depth expects a float32 [H,W] tensor")
    H, W = src.shape
    m = mask.mask_u8 if isinstance(mask, PreparedMask) else mask
    if m is not None:
        m = m.contiguous()
        require_gpu(m)
        if tuple(m.shape) != (H, W) or m.dtype != torch.uint8:
            raise LfsError(f"prepare_depth: the mask must be uint8 [{H},{W}] (got {tuple(m.shape)})")
    out = torch.empty_like(src)
    sums = torch.empty(1, dtype=torch.int64, device=src.device)
    check(load_library().lfs_depth_prepare(C.c_uint32(H), C.c_uint32(W), ptr(src), ptr(m), ptr(out), ptr(sums), stream()), "depth_prepare")
    return PreparedDepth(out, m, sums)


def depth_l1_loss_fwd_bwd(depth: torch.Tensor, target: PreparedDepth, weight: float, loss_acc: torch.Tensor) -> torch.Tensor:
    """lfs_depth_l1_loss_fwd_bwd: loss_acc += weight * sum m |D - t| / max(sum m, 1) over the valid (and masked-in) pixels; returns dL/d(depth), shaped like depth
    ([1,H,W] or [H,W])."""
    depth = depth.contiguous()
    require_gpu(depth, target.target, target.mask_u8, target.sums, loss_acc)
    H, W = target.target.shape
    if depth.numel() != H * W or depth.dtype != torch.float32:
        raise LfsError(f"depth_l1_loss_fwd_bwd: the depth map must be float32 with {H}x{W} elements (got {tuple(depth.shape)})")
    g = torch.empty_like(depth)
    check(load_library().lfs_depth_l1_loss_fwd_bwd(C.c_uint32(H), C.c_uint32(W), ptr(depth), ptr(target.target), ptr(target.mask_u8), ptr(target.sums),
                                                   C.c_float(weight), ptr(g), ptr(loss_acc), stream()), "depth_l1_loss_fwd_bwd")
    return g


def loss_fwd_bwd(kind: str, render: torch.Tensor, target_chw: torch.Tensor, weight: float, loss_acc: torch.Tensor, chw: bool, clamp: bool,
                 lambda_dssim: float = 0.2, mask: PreparedMask | None = None, alpha: torch.Tensor | None = None, alpha_weight: float = 0.0):
    """General fused loss: kind "mse" | "l1_ssim"; render [H,W,3] (chw False) or [3,H,W]; clamp = clamp(render, 0, 1) first (gradient masked).
    loss_acc += weight * loss; returns dL/d(render) in the render's layout.
    mask (a PreparedMask of the render's size): the masked forms - every pixel weighted by its mask byte, normalised by the mask's sums; the SSIM map itself is
    that of the unmasked images. alpha [H,W] (with mask, "l1_ssim" only) adds weight * alpha_weight * sum (255 - M) alpha / (255 H W) and makes the return value
    (v_render, v_alpha). mask=None is the unmasked call, unchanged."""
    target_chw = target_chw.contiguous()
    render = render.contiguous()
    require_gpu(render, target_chw, loss_acc)
    H, W = (render.shape[-2], render.shape[-1]) if chw else (render.shape[-3], render.shape[-2])
    assert tuple(target_chw.shape) == (3, H, W) and render.shape[0 if chw else -1] == 3, (render.shape, target_chw.shape)
    lib = load_library()
    v = torch.empty_like(render)
    if mask is None:
        if alpha is not None:
            raise ValueError("loss_fwd_bwd: alpha needs a mask")
    else:
        require_gpu(mask.mask_u8, mask.sums, alpha)
        if tuple(mask.mask_u8.shape) != (H, W) or mask.mask_u8.dtype != torch.uint8 or mask.sums.dtype != torch.int64 or mask.sums.numel() != 2:
            raise LfsError(f"loss_fwd_bwd: the mask must be uint8 [{H},{W}] with int64[2] sums (got {tuple(mask.mask_u8.shape)})")
        if alpha is not None and (kind != "l1_ssim" or alpha.numel() != H * W or alpha.dtype != torch.float32):
            raise LfsError("loss_fwd_bwd: alpha is a float32 [H,W] tensor of the l1_ssim loss")
    if kind == "mse" and mask is not None:
        check(lib.lfs_mse_loss_masked_fwd_bwd(C.c_uint32(H), C.c_uint32(W), ptr(render), C.c_uint32(int(chw)), C.c_uint32(int(clamp)), ptr(target_chw),
                                              ptr(mask.mask_u8), ptr(mask.sums), C.c_float(weight), ptr(v), ptr(loss_acc), stream()), "mse_loss_masked_fwd_bwd")
    elif kind == "l1_ssim" and mask is not None:
        ws = workspace(lib.lfs_photometric_loss_workspace_bytes(C.c_uint32(H), C.c_uint32(W)), render.device, "photometric")
        v_alpha = torch.empty_like(alpha) if alpha is not None else None
        check(lib.lfs_photometric_loss_masked_fwd_bwd(C.c_uint32(H), C.c_uint32(W), ptr(render), C.c_uint32(int(chw)), C.c_uint32(int(clamp)), ptr(target_chw),
                                                      ptr(mask.mask_u8), ptr(mask.sums), C.c_float(lambda_dssim), C.c_float(weight), ptr(alpha),
                                                      C.c_float(alpha_weight), ptr(v_alpha), ptr(v), ptr(loss_acc), ptr(ws), C.c_size_t(ws.numel()), stream()),
              "photometric_loss_masked_fwd_bwd")
        if alpha is not None:
            return v, v_alpha
    elif kind == "mse":
        check(lib.lfs_mse_loss_ex_fwd_bwd(C.c_uint32(H), C.c_uint32(W), ptr(render), C.c_uint32(int(chw)), C.c_uint32(int(clamp)), ptr(target_chw), C.c_float(weight),
                                          ptr(v), ptr(loss_acc), stream()), "mse_loss_ex_fwd_bwd")
    elif kind == "l1_ssim":
        ws = workspace(lib.lfs_photometric_loss_workspace_bytes(C.c_uint32(H), C.c_uint32(W)), render.device, "photometric")
        check(lib.lfs_photometric_loss_ex_fwd_bwd(C.c_uint32(H), C.c_uint32(W), ptr(render), C.c_uint32(int(chw)), C.c_uint32(int(clamp)), ptr(target_chw),
                                                  C.c_float(lambda_dssim), C.c_float(weight), ptr(v), ptr(loss_acc), ptr(ws), C.c_size_t(ws.numel()), stream()),
              "photometric_loss_ex_fwd_bwd")
    else:
        raise ValueError(f"unknown loss {kind!r}")
    return v


def masked_photometric_loss(rendered: torch.Tensor, gt: torch.Tensor, mask: PreparedMask, lambda_dssim: float = 0.2) -> torch.Tensor:
    """The masked L1 + D-SSIM of lfs_photometric_loss_masked_fwd_bwd through autograd, on [3,H,W] images: built on _FusedSSIM's map of the UNMASKED images
    (padding "valid": the crop, and the kept quirk that an image too small to crop gets no SSIM gradient), weighted per pixel by the mask and normalised by
    its device-side sums. For the autograd step form and as a cross-check of the fused kernel."""
    if rendered.dim() != 3 or gt.dim() != 3:
        raise ValueError("masked_photometric_loss expects [3,H,W] images")
    H, W = rendered.shape[-2], rendered.shape[-1]
    m = mask.mask_u8.to(rendered.dtype)
    s_img, s_crop = mask.sums[0].to(rendered.dtype), mask.sums[1].to(rendered.dtype)
    zero = rendered.new_zeros(())
    l1 = torch.where(s_img > 0, (m * (rendered - gt).abs()).sum() / (3.0 * s_img.clamp_min(1.0)), zero)
    smap = _FusedSSIM.apply(rendered.contiguous(), gt, "valid", True)[0]
    mc = m[5:H - 5, 5:W - 5] if (H > 10 and W > 10) else m
    ssim_term = torch.where(s_crop > 0, 1.0 - (mc * smap).sum() / (3.0 * s_crop.clamp_min(1.0)), zero)
    return (1.0 - lambda_dssim) * l1 + lambda_dssim * ssim_term
