"""Contribution pruning over csrc/fastgs_contrib.hip: what a Gaussian contributes to the training images, and the pruning rules built on it.

    w_ip = T_ip * alpha_ip      the blending weight of Gaussian i at pixel p (T: the transmittance in front of it), over exactly the pixels the forward blends i into

`compute_contribution` reduces it over a sequence of cameras on the device: max_w (RadSplat prunes max_w < 0.01), sum_w (the summed hit weight of LightGaussian /
Mini-Splatting) and n_pix (the number of (pixel, view) pairs). The statistic follows the IMAGE: an instance that only ever terminates pixels (the forward stops a
pixel there without blending it) has max_w = 0; removing it lets those pixels run on with the transmittance they had (< 0.1), so a prune is a training-time
operation that the remaining iterations heal. `prune_mask` turns the statistic into the bool mask GutTrainer._remove_gaussians / strategy.remove_gaussians take.

The kernel adds into a 16-byte row per Gaussian with integer atomics only - same bits on every run and in any order of views. Its pixel counter is 32 bits wide:
the rows are folded into 64-bit tensors every floor((2^32 - 1) / (W * H)) views (FOLD_VIEWS overrides the interval), which changes no bit of the result."""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence

import torch

from .capi import LfsError, require_gpu
from .fastgs import FastGSSettings, _forward

FIX_BITS = 24                        # fraction bits of the fixed-point sum (csrc/fastgs_contrib.hip: CONTRIB_FIX)
FOLD_VIEWS: Optional[int] = None     # views between two folds of the [N,4] buffer; None: floor((2^32 - 1) / (W * H)), the most the 32-bit pixel counter allows
RADSPLAT_THRESHOLD = 0.01


class ContributionStats(NamedTuple):
    max_w: torch.Tensor    # float32 [N]: max over all blended (pixel, view) pairs of w
    sum_w: torch.Tensor    # float64 [N]: sum of w (exact sum of the per-wavefront partial sums, each rounded once to 2^-24)
    n_pix: torch.Tensor    # int64 [N]: number of blended (pixel, view) pairs
    views: int


def new_stats_buffer(N: int, device) -> torch.Tensor:
    """the zero-filled int32 [N,4] buffer ops.fastgs_view_contribution adds into"""
    return torch.zeros((int(N), 4), dtype=torch.int32, device=device)


def unpack_stats(stats: torch.Tensor):
    """int32 [N,4] -> (max_w float32 [N], n_pix int64 [N], sum_fixed int64 [N]); the sum in units of 2^-24"""
    max_w = stats[:, 0].contiguous().view(torch.float32)
    n_pix = stats[:, 1].to(torch.int64) & 0xFFFFFFFF
    sum_fixed = stats.view(torch.int64)[:, 1].contiguous()
    return max_w, n_pix, sum_fixed


def view_contribution(means, scales_raw, rotations_raw, opacities_raw, sh_coefficients_0, sh_coefficients_rest, w2c, settings: FastGSSettings, stats: torch.Tensor):
    """One view: preprocess, render (fastgs._forward: the same calls, settings.antialiased and settings.filter3d honoured), then the view's statistic ADDED to `stats`
    (int32 [N,4]). -> (image, alpha, n_instances) of the render. The only host read is the forward's n_instances."""
    from .ops import fastgs_view_contribution
    image, alpha, pws, iws, n_instances = _forward(means, scales_raw, rotations_raw, opacities_raw, sh_coefficients_0, sh_coefficients_rest, w2c, settings, False)
    fastgs_view_contribution(pws, iws, n_instances, means.shape[0], settings.width, settings.height, stats)
    return image, alpha, n_instances


def camera_settings(camera, model, antialiased: bool = False, filter3d: Optional[torch.Tensor] = None) -> FastGSSettings:
    """the FastGSSettings fastgs.fast_rasterize builds for a rasterizer.Camera (near 0.01, far 1e10, the model's active SH degree)"""
    w2c = camera.world_view_transform.reshape(-1, 4, 4)[0]
    K = camera.K.reshape(-1, 3, 3)[0].cpu()
    R, t = w2c[:3, :3], w2c[:3, 3]
    deg = model.get_active_sh_degree()
    return FastGSSettings(cam_position=(-(R.T @ t)).contiguous(), active_sh_bases=(deg + 1) ** 2, width=int(camera.image_width), height=int(camera.image_height),
                          focal_x=float(K[0, 0]), focal_y=float(K[1, 1]), center_x=float(K[0, 2]), center_y=float(K[1, 2]), near_plane=0.01, far_plane=1e10,
                          antialiased=bool(antialiased), filter3d=filter3d)


def fold_interval(width: int, height: int) -> int:
    """views a [N,4] buffer may take before its 32-bit pixel counter could wrap: floor((2^32 - 1) / (W * H)), at least 1"""
    return max(1, (2 ** 32 - 1) // max(1, int(width) * int(height)))


@torch.no_grad()
def compute_contribution(model, cameras: Sequence, *, antialiased: bool = False, filter3d: Optional[torch.Tensor] = None) -> ContributionStats:
    """The statistic of `model` (a SplatModel) over `cameras` (a sequence of rasterizer.Camera; the renders are the trainer's: fastgs, black background, the model's
    active SH degree, `antialiased` and the [N] `filter3d` variances as FastGSSettings takes them). No host read per view beyond the forward's n_instances."""
    means, sh0, shN, raw_scales, raw_quats, raw_opac = [p.detach() for p in model.parameters()]
    require_gpu(means)
    N, dev = means.shape[0], means.device
    max_w = torch.zeros(N, dtype=torch.float32, device=dev)
    n_pix = torch.zeros(N, dtype=torch.int64, device=dev)
    sum_fixed = torch.zeros(N, dtype=torch.int64, device=dev)
    buf, pending, views = new_stats_buffer(N, dev), 0, 0

    def fold():
        nonlocal max_w, n_pix, sum_fixed
        m, c, s = unpack_stats(buf)
        max_w = torch.maximum(max_w, m)
        n_pix += c
        sum_fixed += s
        buf.zero_()

    for cam in cameras:
        st = camera_settings(cam, model, antialiased, filter3d)
        every = FOLD_VIEWS if FOLD_VIEWS is not None else fold_interval(st.width, st.height)
        if pending >= every:
            fold()
            pending = 0
        view_contribution(means, raw_scales, raw_quats, raw_opac, sh0, shN, cam.world_view_transform, st, buf)
        pending, views = pending + 1, views + 1
    if pending:
        fold()
    return ContributionStats(max_w, sum_fixed.to(torch.float64) * (2.0 ** -FIX_BITS), n_pix, views)


def prune_mask(stats: ContributionStats, *, threshold: Optional[float] = None, keep: Optional[int] = None) -> torch.Tensor:
    """bool [N], True = remove. Exactly one of
    threshold: max_w < threshold (RadSplat: 0.01) - a Gaussian no training ray weights that much;
    keep=K:    the N - K Gaussians of lowest sum_w, ties by index (lowest first), so exactly N - K are marked (K >= N: none)."""
    if (threshold is None) == (keep is None):
        raise ValueError("prune_mask takes exactly one of threshold= and keep=")
    if threshold is not None:
        return stats.max_w < float(threshold)
    N, K = stats.sum_w.shape[0], int(keep)
    if K < 0:
        raise ValueError("keep must be >= 0")
    mask = torch.zeros(N, dtype=torch.bool, device=stats.sum_w.device)
    if K < N:
        order = torch.sort(stats.sum_w, stable=True).indices   # ascending; stable: equal sums stay in index order
        mask[order[:N - K]] = True
    return mask
