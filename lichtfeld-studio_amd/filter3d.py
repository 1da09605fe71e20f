"""The 3D smoothing filter of Mip-Splatting (Yu et al., CVPR 2024, section 4.1) over csrc/filter3d.hip - the other half of the antialiased mode (its 2D Mip filter).

    v_i = variance_scale / nu_i^2,   nu_i = max over the training cameras that see Gaussian i of max(fx, fy) / z_ic

`compute_filter3d` evaluates it on the device from ALL training cameras; the per-primitive kernels of the fastgs rasterizer apply it when the tensor is handed
to them (fastgs.FastGSSettings.filter3d): scales sqrt(s^2 + v), opacity sigmoid(raw) * kappa with kappa = prod_k s_k / s'_k. `bake` folds the filter into the raw
parameters, so that a file written from them renders in any viewer as it was trained: a filtered render of (raw_scales, raw_opacities, v) IS the default render
of bake(...). A baked file is NOT a resume point: training on from it would filter the already filtered scales a second time."""
from __future__ import annotations

import ctypes as C
from typing import Sequence, Tuple, Union

import torch

from .capi import LfsError, check, load_library, ptr, require_gpu, stream, workspace

CAMERA_DWORDS = 18   # lfs_filter3d_camera: w2c rows 0-2 (12 floats), fx, fy, cx, cy (4 floats), width, height (2 uint32)
DEFAULT_VARIANCE = 0.2   # the paper's


def pack_cameras(cameras: Sequence = (), *, viewmats: torch.Tensor = None, Ks: torch.Tensor = None, width=None, height=None, device=None) -> torch.Tensor:
    """-> int32 [C, 18] tensor holding C lfs_filter3d_camera records (the float fields as their bit patterns). Either a sequence of rasterizer.Camera (one view each),
    or viewmats [C,4,4] + Ks [C,3,3] + width / height (one int for all views or one per view)."""
    if viewmats is None:
        cameras = list(cameras)
        if len(cameras) == 0:
            return torch.zeros((0, CAMERA_DWORDS), dtype=torch.int32, device=device if device is not None else "cpu")
        viewmats = torch.stack([c.world_view_transform.reshape(-1, 4, 4)[0] for c in cameras])
        Ks = torch.stack([c.K.reshape(-1, 3, 3)[0] for c in cameras])
        width, height = [int(c.image_width) for c in cameras], [int(c.image_height) for c in cameras]
    viewmats, Ks = viewmats.detach().reshape(-1, 4, 4).to(torch.float32), Ks.detach().reshape(-1, 3, 3).to(torch.float32)
    n = viewmats.shape[0]
    if Ks.shape[0] != n:
        raise LfsError("pack_cameras: viewmats and Ks differ in their number of views")
    dev = device if device is not None else viewmats.device
    wh = torch.empty((n, 2), dtype=torch.int32)
    wh[:, 0] = torch.as_tensor(width, dtype=torch.int32).expand(n) if not isinstance(width, int) else width
    wh[:, 1] = torch.as_tensor(height, dtype=torch.int32).expand(n) if not isinstance(height, int) else height
    floats = torch.cat([viewmats[:, :3, :].reshape(n, 12), Ks[:, 0, 0:1], Ks[:, 1, 1:2], Ks[:, 0, 2:3], Ks[:, 1, 2:3]], dim=1).contiguous()
    return torch.cat([floats.view(torch.int32).to(dev), wh.to(dev)], dim=1).contiguous()


def compute_filter3d(means: torch.Tensor, cameras: Union[Sequence, torch.Tensor], variance_scale: float = DEFAULT_VARIANCE, out: torch.Tensor = None) -> torch.Tensor:
    """-> filter_var [N] float32 on means' device (lfs_filter3d_compute). cameras: a packed tensor of pack_cameras (any device; moved if needed) or a sequence of
    rasterizer.Camera. No host read: the result is ready in stream order. A Gaussian no camera sees takes the weakest constraint any seen one has; no camera, or no
    Gaussian seen at all: zeros (the unfiltered model)."""
    packed = cameras if isinstance(cameras, torch.Tensor) else pack_cameras(cameras, device=means.device)
    if packed.dtype != torch.int32 or packed.dim() != 2 or packed.shape[1] != CAMERA_DWORDS:
        raise LfsError(f"compute_filter3d: the packed cameras are an int32 [C, {CAMERA_DWORDS}] tensor (pack_cameras)")
    means = means.detach().contiguous()
    packed = packed.to(means.device).contiguous()
    require_gpu(means, packed)
    if means.dim() != 2 or means.shape[1] != 3 or means.dtype != torch.float32:
        raise LfsError("compute_filter3d: means must be float32 [N,3]")
    N = means.shape[0]
    if out is None:
        out = torch.empty(N, dtype=torch.float32, device=means.device)
    elif out.shape != (N,) or out.dtype != torch.float32 or out.device != means.device or not out.is_contiguous():
        raise LfsError("compute_filter3d: out must be a contiguous float32 [N] tensor on the device of means")
    lib = load_library()
    ws = workspace(lib.lfs_filter3d_workspace_bytes(), means.device, "filter3d")
    check(lib.lfs_filter3d_compute(C.c_uint32(N), ptr(means), C.c_uint32(packed.shape[0]), ptr(packed), C.c_float(variance_scale), ptr(out), ptr(ws), C.c_size_t(ws.numel()),
                                   stream()), "filter3d_compute")
    return out


def bake(model_or_raw, filter_var: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(raw_scales', raw_opacities') with the filter folded in: 1/2 log(exp(2 raw_scale) + v) and logit(sigmoid(raw) * kappa), kappa = prod_k s_k / s'_k, evaluated in
    float64 and returned in the inputs' dtype and shape. model_or_raw: a SplatModel, or the pair (raw_scales [N,3], raw_opacities [N] | [N,1]). Plain tensor arithmetic
    (export time, any device). log kappa = 1/2 sum_k log1p(-u_k) with u_k = v / (s_k^2 + v), so nothing overflows for large scales and nothing cancels for small v."""
    raw_scales, raw_opac = model_or_raw if isinstance(model_or_raw, (tuple, list)) else (model_or_raw.raw_scales, model_or_raw.raw_opacities)
    rs, ro = raw_scales.detach().to(torch.float64), raw_opac.detach().to(torch.float64)
    v = filter_var.detach().to(torch.float64).reshape(-1, 1)
    if v.shape[0] != rs.shape[0]:
        raise LfsError(f"bake: filter_var has {v.shape[0]} elements, the model {rs.shape[0]} Gaussians")
    s2 = torch.exp(2.0 * rs)
    scales = 0.5 * torch.log(s2 + v)
    scales = torch.where((v > 0) & torch.isfinite(s2), scales, rs)                         # v = 0 rows: the raw value itself; exp overflowed in float64: the filter is negligible
    u = torch.where(v > 0, v / (s2 + v), torch.zeros_like(s2))
    log_kappa = 0.5 * torch.log1p(-u).sum(dim=1)                                            # -inf where some s_k^2 underflowed against v: opacity 0
    log_sig = -torch.nn.functional.softplus(-ro.reshape(-1))                               # log sigmoid(raw)
    log_o = log_sig + log_kappa
    logit = log_o - torch.log(-torch.expm1(log_o))                                          # log(o / (1 - o))
    logit = torch.where(log_kappa == 0, ro.reshape(-1), logit)                             # v = 0 rows: the raw value itself, bit for bit
    return scales.to(raw_scales.dtype), logit.reshape(raw_opac.shape).to(raw_opac.dtype)


class Filter3dSchedule:
    """When the trainer recomputes the filter - pure host logic: before the first step, at the step after one in which the strategy changed the model, and otherwise
    every `every` steps (counted from the last computation)."""

    def __init__(self, every: int = 100):
        if int(every) < 1:
            raise ValueError("every must be >= 1")
        self.every, self.steps_since, self.dirty = int(every), None, True

    def due(self) -> bool:
        return self.dirty or self.steps_since is None or self.steps_since >= self.every

    def computed(self) -> None:
        self.steps_since, self.dirty = 0, False

    def step_done(self, model_changed: bool = False) -> None:
        if self.steps_since is not None:
            self.steps_since += 1
        self.dirty = self.dirty or bool(model_changed)
