"""Mirror of the reference's DEFAULT training rasterizer over csrc/fastgs_{prep,blend}.hip:
`fast_gs::rasterization::forward_wrapper / backward_wrapper` (fastgs/rasterization/include/rasterization_api.h:27-75),
the autograd Function `FastGSRasterize` (src/training/rasterization/fast_rasterizer_autograd.cpp:8-186) and
`fast_rasterize` (fast_rasterizer.cpp:12-68: near 0.01, far 1e10, background blended outside the op).

The reference returns four opaque buffer tensors + five integers from the forward and hands them to the backward; here the
state is two workspace tensors (primitive / instance) and `n_instances`.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from .capi import FastgsBackwardArgs, FastgsShRestAdam, FastgsView, FastgsViewExt, LfsError, check, load_library, ptr, require_gpu, stream, workspace
from .rasterizer import Camera, RenderMode, RenderOutput, SplatModel


@dataclass
class FastGSSettings:  # rasterization_api.h:12-24
    cam_position: torch.Tensor
    active_sh_bases: int
    width: int
    height: int
    focal_x: float
    focal_y: float
    center_x: float
    center_y: float
    near_plane: float
    far_plane: float
    antialiased: bool = False   # opacity * sqrt(det(Sigma2d) / det(Sigma2d + 0.3 I)) (LFS_FASTGS_ANTIALIASED; the reference's OptimizationParameters::antialiasing)
    depth: str = "none"         # "depth" | "invdepth": the records also carry z | 1 / z (LFS_FASTGS_DEPTH | LFS_FASTGS_INVDEPTH) for forward_wrapper_depth
    filter3d: Optional[torch.Tensor] = None   # [N] filter variances of the 3D smoothing filter (filter3d.compute_filter3d; lfs_fastgs_view_ext.filter3d_var): scales
                                              # sqrt(s^2 + v), opacity sigmoid(raw) * prod s / s'. Forward and backward of one view take the same tensor. No gradient.
    absgrad: bool = False       # LFS_FASTGS_ABSGRAD: densification_info takes the norm of the per-pixel ABSOLUTE screen-space gradients (AbsGS / gsplat's absgrad); the
                                # workspace remembers it, the render and every gradient are the default mode's


ANTIALIASED = 1         # LFS_FASTGS_ANTIALIASED
ABSGRAD = 32            # LFS_FASTGS_ABSGRAD
DEPTH_FLAGS = {"none": 0, "depth": 4, "invdepth": 8}   # LFS_FASTGS_DEPTH, LFS_FASTGS_INVDEPTH
ASYNC_READBACK = True   # False: n_instances via a stream synchronisation (A/B timing)


def _filter3d_operand(s: FastGSSettings, N: int, device) -> Optional[torch.Tensor]:
    """the contiguous float32 [N] device tensor behind FastGSSettings.filter3d (None: the unfiltered entries are called, the code path of a build without the filter)"""
    v = s.filter3d
    if v is None:
        return None
    v = v.detach().reshape(-1).contiguous()
    if v.numel() != N or v.dtype != torch.float32 or v.device != device:
        raise LfsError(f"FastGSSettings.filter3d must be a float32 tensor of N = {N} elements on {device} (got {tuple(v.shape)}, {v.dtype}, {v.device})")
    require_gpu(v)
    return v


def view_struct(s: FastGSSettings, means, scales_raw, rotations_raw, opacities_raw, sh0, sh_rest, w2c, cam_position, primitive_workspace) -> FastgsView:
    """lfs_fastgs_view of contiguous device tensors (opacities_raw: None for the backward). Keeps no reference to them: callers hold them for the duration of the call."""
    return FastgsView(means.shape[0], ptr(means), ptr(scales_raw), ptr(rotations_raw), ptr(opacities_raw), ptr(sh0), ptr(sh_rest), sh_rest.shape[1] if sh_rest.dim() == 3 else 0,
                      ptr(w2c), ptr(cam_position), s.active_sh_bases, s.width, s.height, s.focal_x, s.focal_y, s.center_x, s.center_y, s.near_plane, s.far_plane,
                      ptr(primitive_workspace), primitive_workspace.numel())


def forward_wrapper(means, scales_raw, rotations_raw, opacities_raw, sh_coefficients_0, sh_coefficients_rest, w2c, s: FastGSSettings):
    """-> (image [3,H,W], alpha [1,H,W], primitive_workspace, instance_workspace, n_instances). s.antialiased: the antialiased mode; the primitive workspace
    remembers it, so backward_wrapper takes the same arguments in both modes. (s.depth is honoured in the preprocess, but this function returns no depth plane:
    forward_wrapper_depth does.)"""
    return _forward(means, scales_raw, rotations_raw, opacities_raw, sh_coefficients_0, sh_coefficients_rest, w2c, s, False)


def forward_wrapper_depth(means, scales_raw, rotations_raw, opacities_raw, sh_coefficients_0, sh_coefficients_rest, w2c, s: FastGSSettings):
    """-> (image, alpha, depth [1,H,W], primitive_workspace, instance_workspace, n_instances) with s.depth "depth" | "invdepth": depth = sum_i w_i d_i, d_i = z_i or
    1 / z_i in camera space - the ACCUMULATED value (the reference's D / RGB_D); image and alpha are forward_wrapper's bit for bit."""
    if s.depth not in ("depth", "invdepth"):
        raise LfsError(f"forward_wrapper_depth needs FastGSSettings.depth 'depth' or 'invdepth' (got {s.depth!r})")
    return _forward(means, scales_raw, rotations_raw, opacities_raw, sh_coefficients_0, sh_coefficients_rest, w2c, s, True)


def _forward(means, scales_raw, rotations_raw, opacities_raw, sh_coefficients_0, sh_coefficients_rest, w2c, s: FastGSSettings, want_depth: bool):
    w2c = w2c.reshape(-1, 4, 4)[0].contiguous()
    cam_position = s.cam_position.reshape(-1)[:3].contiguous()
    opac = opacities_raw.reshape(-1)
    tensors = [means, scales_raw, rotations_raw, opac, sh_coefficients_0, sh_coefficients_rest, w2c, cam_position]
    tensors = [t.contiguous() for t in tensors]
    require_gpu(*tensors)
    means, scales_raw, rotations_raw, opac, sh0, shr, w2c, cam_position = tensors
    N = means.shape[0]
    total_rest = shr.shape[1] if shr.dim() == 3 else 0
    if s.active_sh_bases > 1 + total_rest:
        raise LfsError("active_sh_bases exceeds the stored SH coefficients")
    lib, dev = load_library(), means.device
    pws = torch.empty(lib.lfs_fastgs_primitive_workspace_bytes(C.c_uint32(N), C.c_uint32(s.width), C.c_uint32(s.height)), dtype=torch.uint8, device=dev)
    n_inst_dev = torch.zeros(1, dtype=torch.int64, device=dev)
    if s.depth not in DEPTH_FLAGS:
        raise LfsError(f"FastGSSettings.depth must be 'none', 'depth' or 'invdepth' (got {s.depth!r})")
    flags = (ANTIALIASED if s.antialiased else 0) | DEPTH_FLAGS[s.depth] | (ABSGRAD if s.absgrad else 0)
    view = view_struct(s, means, scales_raw, rotations_raw, opac, sh0, shr, w2c, cam_position, pws)
    f3d = _filter3d_operand(s, N, dev)
    if f3d is None:
        check(lib.lfs_fastgs_view_preprocess(C.byref(view), C.c_uint32(flags), ptr(n_inst_dev), stream()), "fastgs_view_preprocess")
    else:
        ext = FastgsViewExt(ptr(f3d))
        check(lib.lfs_fastgs_view_preprocess_ex(C.byref(view), C.c_uint32(flags), C.byref(ext), ptr(n_inst_dev), stream()), "fastgs_view_preprocess_ex")
    # the one host sync (forward.cu:114-117 reads n_visible_primitives and n_instances): waits for the read-back event the library queued before
    # its SH kernel, so the GPU keeps working through the host round trip
    if ASYNC_READBACK:
        n_host = C.c_int64(0)
        check(lib.lfs_fastgs_wait_n_instances(C.byref(n_host)), "fastgs_wait_n_instances")
        n_instances = int(n_host.value)
    else:
        n_instances = int(n_inst_dev.item())
    iws = torch.empty(max(256, lib.lfs_fastgs_instance_workspace_bytes(C.c_uint32(s.width), C.c_uint32(s.height), C.c_int64(n_instances))), dtype=torch.uint8, device=dev)
    image = torch.empty((3, s.height, s.width), dtype=means.dtype, device=dev)
    alpha = torch.empty((1, s.height, s.width), dtype=means.dtype, device=dev)
    depth = torch.empty((1, s.height, s.width), dtype=means.dtype, device=dev) if want_depth else None
    check(lib.lfs_fastgs_view_render(C.byref(view), C.c_int64(n_instances), ptr(iws), C.c_size_t(iws.numel()), ptr(image), ptr(alpha), ptr(depth), stream()), "fastgs_view_render")
    return (image, alpha, depth, pws, iws, n_instances) if want_depth else (image, alpha, pws, iws, n_instances)


def backward_wrapper(densification_info: Optional[torch.Tensor], grad_image, grad_alpha, image, alpha, means, scales_raw, rotations_raw,
                     sh_coefficients_0, sh_coefficients_rest, primitive_workspace, instance_workspace, w2c, s: FastGSSettings, n_instances: int, out=None,
                     adam_sh_rest: Optional[dict] = None, grad_w2c: Optional[torch.Tensor] = None, grad_depth: Optional[torch.Tensor] = None):
    """-> (grad_means, grad_scales_raw, grad_rotations_raw, grad_opacities_raw [N,1], grad_sh_coefficients_0, grad_sh_coefficients_rest);
    densification_info [2,N] (when given and non-empty) is accumulated into in place (kernels_backward.cuh:229-232).
    Extension `adam_sh_rest` (FusedAdam.prepare_inline of sh_coefficients_rest; single-view steps): the rest-coefficient gradient is not
    written, the coefficients and their moments are updated in place by the SH backward (lfs_fastgs_view_backward_args.adam).
    `grad_w2c` (pose optimisation; a contiguous float32 out buffer of 16 elements, e.g. zeros_like(w2c)): the camera gradient the reference's backward returns
    when w2c requires grad (rasterization_api.cu:133-136) is WRITTEN into it - rows 0-2 = sum over the visible primitives of dL/d(mean in camera space) (x) (mean, 1),
    row 3 = 0 (lfs_fastgs_view_backward_args.grad_w2c). None: no camera gradient. Not combined with adam_sh_rest.
    `grad_depth` ([1,H,W] or [H,W]; the workspace of a forward with s.depth on): the gradient of forward_wrapper_depth's depth plane (lfs_fastgs_view_backward_args.grad_depth) - depth
    is blended as a fourth channel, and dL/dz reaches grad_means and, with grad_w2c, row 2 of the camera gradient. Not combined with adam_sh_rest."""
    w2c = w2c.reshape(-1, 4, 4)[0].contiguous()
    cam_position = s.cam_position.reshape(-1)[:3].contiguous()
    grad_image, grad_alpha, alpha = grad_image.contiguous(), grad_alpha.contiguous(), alpha.contiguous()
    means, scales_raw, rotations_raw, shr = means.contiguous(), scales_raw.contiguous(), rotations_raw.contiguous(), sh_coefficients_rest.contiguous()
    sh0 = sh_coefficients_0.contiguous()  # (the reference's backward does not need sh0; the SH backward kernel here shares its operand list with the forward)
    require_gpu(grad_image, grad_alpha, alpha, means, scales_raw, rotations_raw, sh0, shr, w2c, cam_position)
    N = means.shape[0]
    total_rest = shr.shape[1] if shr.dim() == 3 else 0
    dens = densification_info if (densification_info is not None and densification_info.numel() > 0) else None
    if dens is not None and (tuple(dens.shape) != (2, N) or not dens.is_contiguous()):
        raise LfsError("densification_info must be a contiguous [2,N] tensor")
    if out is not None:  # extension: write into the caller's (contiguous) buffers, e.g. views of the data-parallel gradient bucket
        g_means, g_scales, g_rot, g_opac, g_sh0, g_shr = out
        require_gpu(*out)
    else:
        g_means, g_scales, g_rot = torch.empty_like(means), torch.empty_like(scales_raw), torch.empty_like(rotations_raw)
        g_opac = torch.empty((N, 1), dtype=means.dtype, device=means.device)
        g_sh0 = torch.empty((N, 1, 3), dtype=means.dtype, device=means.device)
        g_shr = torch.empty_like(shr)
    if grad_depth is not None and adam_sh_rest is not None:
        raise LfsError("grad_depth is not available together with adam_sh_rest: depth supervision takes the separate optimizer")
    if grad_w2c is not None:
        if adam_sh_rest is not None:
            raise LfsError("grad_w2c is not available together with adam_sh_rest: pose optimisation takes the separate optimizer")
        if grad_w2c.numel() != 16 or grad_w2c.dtype != torch.float32 or not grad_w2c.is_contiguous():
            raise LfsError("grad_w2c must be a contiguous float32 buffer of 16 elements ([4,4] or [1,4,4])")
        require_gpu(grad_w2c)
    if grad_depth is not None:
        grad_depth = grad_depth.contiguous()
        require_gpu(grad_depth)
        if grad_depth.numel() != s.width * s.height or grad_depth.dtype != torch.float32:
            raise LfsError("grad_depth must be a float32 [1,H,W] tensor")
    lib = load_library()
    ws = workspace(lib.lfs_fastgs_w2c_workspace_bytes(C.c_uint32(N)), means.device, "fastgs_w2c") if grad_w2c is not None else None
    adam = None
    if adam_sh_rest is not None and total_rest > 0:
        a = adam_sh_rest
        if not sh_coefficients_rest.is_contiguous():
            raise LfsError("adam_sh_rest needs the parameter tensor itself (contiguous), it is updated in place")
        adam = FastgsShRestAdam(ptr(sh_coefficients_rest), ptr(a["exp_avg"]), ptr(a["exp_avg_sq"]), a["lr"], a["beta1"], a["beta2"], a["eps"], a["bc1_rcp"], a["bc2_sqrt_rcp"])
    view = view_struct(s, means, scales_raw, rotations_raw, None, sh0, shr, w2c, cam_position, primitive_workspace)
    args = FastgsBackwardArgs(n_instances, ptr(instance_workspace), instance_workspace.numel(), ptr(grad_image), ptr(grad_alpha), ptr(alpha), ptr(grad_depth), ptr(dens),
                              ptr(g_means), ptr(g_scales), ptr(g_rot), ptr(g_opac), ptr(g_sh0), ptr(g_shr), ptr(grad_w2c), ptr(ws), ws.numel() if ws is not None else 0,
                              C.pointer(adam) if adam is not None else None)
    f3d = _filter3d_operand(s, N, means.device)
    if f3d is not None:
        ext = FastgsViewExt(ptr(f3d))
        check(lib.lfs_fastgs_view_backward_ex(C.byref(view), C.byref(args), C.byref(ext), stream()),
              "fastgs_view_backward_ex (LFS_E_INVALID here also means: the forward of this workspace ran without FastGSSettings.filter3d, or more than 256 filtered or "
              "depth-mode forwards were started since without their backward and it was forgotten)")
        return g_means, g_scales, g_rot, g_opac, g_sh0, g_shr
    check(lib.lfs_fastgs_view_backward(C.byref(view), C.byref(args), stream()),
          "fastgs_view_backward" if grad_depth is None else
          "fastgs_view_backward with grad_depth (LFS_E_INVALID here also means: this workspace is not known as a depth-mode workspace - its forward ran without "
          "FastGSSettings.depth, or more than 256 depth-mode forwards were started since without their backward and it was forgotten)")
    return g_means, g_scales, g_rot, g_opac, g_sh0, g_shr


class FastGSRasterize(torch.autograd.Function):
    """fast_rasterizer_autograd.cpp:8-186"""

    @staticmethod
    def forward(ctx, means, scales_raw, rotations_raw, opacities_raw, sh0, sh_rest, w2c, densification_info, settings: FastGSSettings):
        depth = None
        if settings.depth != "none":   # (image, alpha, depth): the accumulated depth, so that autograd can divide by alpha outside the op
            image, alpha, depth, pws, iws, n_instances = forward_wrapper_depth(means, scales_raw, rotations_raw, opacities_raw, sh0, sh_rest, w2c, settings)
        else:
            image, alpha, pws, iws, n_instances = forward_wrapper(means, scales_raw, rotations_raw, opacities_raw, sh0, sh_rest, w2c, settings)
        ctx.save_for_backward(image, alpha, means, scales_raw, rotations_raw, sh0, sh_rest, w2c)
        ctx.state = (pws, iws, n_instances, settings, densification_info, opacities_raw.shape)
        return (image, alpha) if depth is None else (image, alpha, depth)

    @staticmethod
    def backward(ctx, grad_image, grad_alpha, grad_depth=None):
        image, alpha, means, scales_raw, rotations_raw, sh0, sh_rest, w2c = ctx.saved_tensors
        pws, iws, n_instances, settings, dens, opac_shape = ctx.state
        g_w2c = torch.empty_like(w2c, memory_format=torch.contiguous_format) if ctx.needs_input_grad[6] else None   # pose optimisation: fast_rasterizer_autograd.cpp hands grad_w2c on
        g = backward_wrapper(dens, grad_image, grad_alpha, image, alpha, means, scales_raw, rotations_raw, sh0, sh_rest, pws, iws, w2c, settings, n_instances,
                             grad_w2c=g_w2c, grad_depth=grad_depth)
        return g[0], g[1], g[2], g[3].reshape(opac_shape), g[4], g[5], g_w2c, None, None


def fast_rasterize(camera: Camera, model: SplatModel, bg_color: torch.Tensor, densification_info: Optional[torch.Tensor] = None, antialiased: bool = False,
                   render_mode: RenderMode = RenderMode.RGB, depth_kind: str = "depth", filter3d: Optional[torch.Tensor] = None, absgrad: bool = False) -> RenderOutput:
    """fast_rasterizer.cpp:12-68; antialiased: FastGSSettings.antialiased (an extension: the reference's fast_rasterize has no such argument).
    render_mode (the reference's RenderMode, which its EWA path ignores): D / RGB_D fill RenderOutput.depth [1,H,W] with the accumulated sum w_i d_i, ED / RGB_ED with
    that over alpha.clamp_min(1e-10) (rasterizer.py's rule); D / ED return image None (the colour is still rendered inside). depth_kind "depth": d = z,
    "invdepth": d = 1 / z. RGB: everything as before. filter3d: FastGSSettings.filter3d, the [N] variances of the 3D smoothing filter (no gradient flows into it).
    absgrad: FastGSSettings.absgrad - the backward accumulates the absolute-gradient norm into densification_info; nothing else changes."""
    render_mode = RenderMode(render_mode)
    if depth_kind not in ("depth", "invdepth"):
        raise ValueError(f"depth_kind must be 'depth' or 'invdepth' (got {depth_kind!r})")
    W, H = int(camera.image_width), int(camera.image_height)
    K = camera.K.reshape(-1, 3, 3)[0]
    w2c = camera.world_view_transform
    R, t = w2c.reshape(-1, 4, 4)[0][:3, :3], w2c.reshape(-1, 4, 4)[0][:3, 3]
    deg = model.get_active_sh_degree()
    settings = FastGSSettings(cam_position=(-(R.T @ t)).contiguous(), active_sh_bases=(deg + 1) ** 2, width=W, height=H,
                              focal_x=float(K[0, 0]), focal_y=float(K[1, 1]), center_x=float(K[0, 2]), center_y=float(K[1, 2]), near_plane=0.01, far_plane=1e10, antialiased=bool(antialiased),
                              depth="none" if render_mode == RenderMode.RGB else depth_kind, filter3d=filter3d, absgrad=bool(absgrad))
    out = FastGSRasterize.apply(model.means, model.raw_scales, model.raw_quats, model.raw_opacities, model.sh0, model.shN, w2c, densification_info, settings)
    image, alpha = out[0], out[1]
    depth = None
    if render_mode != RenderMode.RGB:
        depth = out[2] if render_mode in (RenderMode.D, RenderMode.RGB_D) else out[2] / alpha.clamp_min(1e-10)
    image = image + (1.0 - alpha) * bg_color.view(3, 1, 1) if render_mode in (RenderMode.RGB, RenderMode.RGB_D, RenderMode.RGB_ED) else None
    return RenderOutput(image=image, alpha=alpha, depth=depth, means2d=None, depths=None, radii=None, visibility=None, width=W, height=H, n_isects=0)


def mse_loss_chw_fwd_bwd(render_chw: torch.Tensor, target_chw: torch.Tensor, weight: float, loss_acc: torch.Tensor) -> torch.Tensor:
    """loss_acc += weight * mse(render, target) (no clamp: fast_rasterize hands the image on as is); returns dL/d(render) [3,H,W]."""
    target_chw = target_chw.contiguous()
    require_gpu(render_chw, target_chw, loss_acc)
    H, W = render_chw.shape[-2], render_chw.shape[-1]
    v = torch.empty_like(render_chw)
    check(load_library().lfs_mse_loss_chw_fwd_bwd(C.c_uint32(H), C.c_uint32(W), ptr(render_chw), ptr(target_chw), C.c_float(weight), ptr(v), ptr(loss_acc), stream()),
          "mse_loss_chw_fwd_bwd")
    return v


def render_and_backward(settings: FastGSSettings, w2c: torch.Tensor, model: SplatModel, target_chw: torch.Tensor, weight: float, grads, loss_acc: torch.Tensor,
                        densification_info: Optional[torch.Tensor] = None, loss: str = "mse", lambda_dssim: float = 0.2, bilateral=None, image_idx: int = 0,
                        adam_shN: Optional[dict] = None, grad_w2c: Optional[torch.Tensor] = None, mask=None, mask_alpha_weight: float = 0.0,
                        depth_target=None, depth_weight: float = 0.0, visibility_bits: Optional[torch.Tensor] = None, accumulate_visibility: bool = False,
                        background=None, target_alpha: Optional[torch.Tensor] = None):
    """One training view without an autograd graph (black background unless `background` says otherwise; loss "mse" or the trainer's "l1_ssim", trainer.cpp:122-125):
    forward, [bilateral-grid slice, trainer.cpp:662-664,] loss, backward; the gradients of (means, sh0, shN, raw_scales, raw_quats,
    raw_opacities) are WRITTEN into `grads` (param-group order); the bilateral grid's gradient is accumulated into its .grad;
    `grad_w2c` (optional out buffer, pose optimisation): the camera gradient is written into it (backward_wrapper).
    mask (a losses.PreparedMask): the masked loss on `shown`; with mask_alpha_weight > 0 ("segment", l1_ssim) the opacity penalty outside the mask, whose
    gradient replaces the zero alpha gradient of the backward.
    depth_target (a losses.PreparedDepth; settings.depth "depth" | "invdepth" says what it holds): loss_acc += weight * depth_weight * the masked L1 between the
    accumulated depth map and the target (lfs_depth_l1_loss_fwd_bwd), and the backward is the depth one. None: everything as before.
    visibility_bits (int32 [ceil(N / 32)], visible-only Adam): bit i is written - with accumulate_visibility ORed - from the view's n_touched column right after
    the forward (ops.fastgs_view_visibility): set exactly where the backward counts Gaussian i as visible. None: nothing is launched.
    background (three Python floats, passed to the kernels by value; None = black): the image the bilateral grid and the loss see is image + (1 - alpha) * bg
    (ops.background_compose right after the forward and the visibility bits, trainer.cpp:656-664 - fast_rasterize's expression, the same bits), and after the loss
    and the bilateral backward ops.background_compose_bwd turns dL/d(shown) into the alpha gradient of the backward (on top of segment mode's). dL/d(image) is
    dL/d(shown) itself.
    target_alpha (uint8 [H,W] on the device): the target the loss sees is a * target + (1 - a) * bg, a = u8 / 255 - composited over THIS step's background, black
    included - written into a scratch tensor kept across steps, in the launch that composes the render (target_chw itself is never written).
    With background None or (0, 0, 0) and target_alpha None nothing new is launched: the step is the one without the two arguments, bit for bit.
    -> (image, alpha, n_instances): the rasterizer's own image, before the background."""
    bg = None
    if background is not None:
        bg = tuple(float(v) for v in background)
        if len(bg) != 3 or not all(v == v and abs(v) != float("inf") for v in bg):
            raise LfsError(f"background must be three finite floats (got {background!r})")
        if bg == (0.0, 0.0, 0.0):
            bg = None
    if target_alpha is not None:
        if target_alpha.dtype != torch.uint8 or tuple(target_alpha.shape) != (settings.height, settings.width):
            raise LfsError(f"target_alpha must be a uint8 [{settings.height},{settings.width}] tensor (got {target_alpha.dtype}, {tuple(target_alpha.shape)})")
        target_alpha = target_alpha.contiguous()
    means, sh0, shN, raw_scales, raw_quats, raw_opac = [p.detach() for p in model.parameters()]
    g_means, g_sh0, g_shN, g_scales, g_quats, g_opac = grads
    with torch.no_grad():
        v_depth = None
        if depth_target is not None:
            from .losses import depth_l1_loss_fwd_bwd
            image, alpha, depth, pws, iws, n_inst = forward_wrapper_depth(means, raw_scales, raw_quats, raw_opac, sh0, shN, w2c, settings)
            v_depth = depth_l1_loss_fwd_bwd(depth, depth_target, weight * depth_weight, loss_acc)
        else:
            image, alpha, pws, iws, n_inst = forward_wrapper(means, raw_scales, raw_quats, raw_opac, sh0, shN, w2c, settings)
        if visibility_bits is not None:
            from .ops import fastgs_view_visibility
            fastgs_view_visibility(pws, means.shape[0], settings.width, settings.height, visibility_bits, accumulate_visibility)
        composed = image
        if bg is not None or target_alpha is not None:
            from .ops import background_compose
            t_out = None
            if target_alpha is not None:
                target_chw = target_chw.contiguous()
                t_out = getattr(render_and_backward, "_target", None)
                if t_out is None or t_out.shape != target_chw.shape or t_out.device != target_chw.device:
                    t_out = render_and_backward._target = torch.empty_like(target_chw)
            if bg is not None:   # out of place: `image` stays the rasterizer's (it is returned)
                composed, t_out = background_compose(bg, image, alpha, None, target_chw if t_out is not None else None, target_alpha, t_out)
            else:                # black: the render is its own composite, only the target is
                _, t_out = background_compose((0.0, 0.0, 0.0), target_rgb=target_chw, target_alpha=target_alpha, target_out=t_out)
            if t_out is not None:
                target_chw = t_out
        shown = composed if bilateral is None else bilateral.apply_fused(composed, image_idx, chw=True)
        v_alpha = None
        if mask is not None:
            from .losses import loss_fwd_bwd
            if mask_alpha_weight > 0.0:
                v_image, v_alpha = loss_fwd_bwd(loss, shown, target_chw, weight, loss_acc, chw=True, clamp=False, lambda_dssim=lambda_dssim, mask=mask,
                                                alpha=alpha, alpha_weight=mask_alpha_weight)
            else:
                v_image = loss_fwd_bwd(loss, shown, target_chw, weight, loss_acc, chw=True, clamp=False, lambda_dssim=lambda_dssim, mask=mask)
        elif loss == "l1_ssim":
            from .losses import photometric_loss_chw_fwd_bwd
            v_image = photometric_loss_chw_fwd_bwd(shown, target_chw, lambda_dssim, weight, loss_acc)
        elif loss == "mse":
            v_image = mse_loss_chw_fwd_bwd(shown, target_chw, weight, loss_acc)
        else:
            raise ValueError(f"unknown loss {loss!r}")
        if bilateral is not None:
            v_image = bilateral.apply_fused_backward(composed, image_idx, v_image, chw=True)
        if bg is not None:   # d(shown)/d(alpha) = -bg: into the alpha gradient of the backward, in place on segment mode's
            from .ops import background_compose_bwd
            v_alpha = background_compose_bwd(bg, v_image, v_alpha, v_alpha)
        if not hasattr(render_and_backward, "_zero") or render_and_backward._zero.shape != alpha.shape or render_and_backward._zero.device != alpha.device:
            render_and_backward._zero = torch.zeros_like(alpha)
        backward_wrapper(densification_info, v_image, render_and_backward._zero if v_alpha is None else v_alpha, image, alpha, means, raw_scales, raw_quats, sh0, shN, pws, iws, w2c, settings, n_inst,
                         out=(g_means, g_scales, g_quats, g_opac.view(-1, 1), g_sh0, g_shN), adam_sh_rest=adam_shN, grad_w2c=grad_w2c, grad_depth=v_depth)
    return image, alpha, n_inst
