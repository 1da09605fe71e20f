"""A plain float64 PyTorch model of ONE training step of the --gut path (test infrastructure only): activations, SH colours, the world-space rasterizer over given tile
lists, the loss with its regularisers, the MCMC noise and Adam. Written from the reference's sources, cited per function - not from oracle/*.hpp, the kernels or the
numpy chain rules of tests/test_gpu_pipeline.py - and differentiated by torch.autograd only: there is no hand-derived gradient in this file.

What is an INPUT, not modelled: the tile lists (tile_offsets, flatten_ids) and the visibility mask (radii > 0) of the projection. The thresholds of the rasterizer
(alpha < 1/255 skipped, the Gaussian that would bring T to <= 1e-4 ends the pixel) are masks (torch.where), so autograd differentiates what the reference's backward
differentiates: the contributions that were composited."""
import torch

import ssim_reference

F64 = torch.float64
ALPHA_MIN, ALPHA_MAX, T_MIN = 1.0 / 255.0, 0.999, 1e-4


def f64(a):
    return None if a is None else torch.as_tensor(a).detach().to("cpu", F64).clone()


# ---- SplatData getters (src/core/splat_data.cpp: get_rotation / get_scaling / get_opacity) ----------------------------------------------------------------------
def activations(raw_quats, raw_scales, raw_opac):
    return raw_quats / raw_quats.norm(dim=-1, keepdim=True), torch.exp(raw_scales), torch.sigmoid(raw_opac)


# ---- spherical harmonics (tests/torch_impl.cpp:221-321 of the reference) ----------------------------------------------------------------------------------------
def sh_bases(n_bases, d):
    """d [...,3] unit vectors -> [..., n_bases]"""
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    b = [torch.full_like(x, 0.2820947917738781)]
    if n_bases > 1:
        a = -0.48860251190292
        b += [a * y, -a * z, a * x]
    if n_bases > 4:
        z2 = z * z
        tb = -1.092548430592079 * z
        a = 0.5462742152960395
        c1, s1 = x * x - y * y, 2 * x * y
        b += [a * s1, tb * y, 0.9461746957575601 * z2 - 0.3153915652525201, tb * x, a * c1]
    if n_bases > 9:
        tc = -2.285228997322329 * z2 + 0.4570457994644658
        tb = 1.445305721320277 * z
        a = -0.5900435899266435
        c2, s2 = x * c1 - y * s1, x * s1 + y * c1
        b += [a * s2, tb * s1, tc * y, z * (1.865881662950577 * z2 - 1.119528997770346), tc * x, tb * c1, a * c2]
    if n_bases > 16:
        td = z * (-4.683325804901025 * z2 + 2.007139630671868)
        tc = 3.31161143515146 * z2 - 0.47308734787878
        tb = -1.770130769779931 * z
        a = 0.6258357354491763
        c3, s3 = x * c2 - y * s2, x * s2 + y * c2
        b += [a * s3, tb * s2, tc * s1, td * y,
              1.984313483298443 * z2 * (1.865881662950577 * z2 - 1.119528997770346) - 1.006230589874905 * (0.9461746957575601 * z2 - 0.3153915652525201),
              td * x, tc * c1, tb * c2, a * c3]
    return torch.stack(b[:n_bases], -1)


def spherical_harmonics(degree, dirs, coeffs):
    """dirs [N,3] (any length), coeffs [N,K,3] -> [N,3]; coefficients beyond (degree + 1)^2 do not take part"""
    nb = (degree + 1) ** 2
    assert coeffs.shape[-2] >= nb
    d = dirs / dirs.norm(dim=-1, keepdim=True)
    return (sh_bases(nb, d).unsqueeze(-1) * coeffs[..., :nb, :]).sum(-2)


def sh_colors(degree, means, sh0, shN, viewmat, visible):
    """rasterizer.cpp:249-266: directions from the camera position, masked by radii > 0, + 0.5, clamped at 0"""
    campos = torch.linalg.inv(viewmat)[:3, 3]
    col = spherical_harmonics(degree, means - campos, torch.cat([sh0, shN], 1))
    col = torch.where(visible[:, None], col, torch.zeros_like(col))
    return torch.clamp_min(col + 0.5, 0.0)


# ---- rasterization from world space (gsplat/RasterizeToPixelsFromWorld3DGSFwd.cu:133-275) ------------------------------------------------------------------------
def quat_to_rotmat(q):
    """gsplat/Utils.cuh:80-102 (w, x, y, z; normalises by itself) -> [N,3,3], rows as written mathematically (glm's constructor takes columns)"""
    q = q / q.norm(dim=-1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)


def pixel_rays(viewmat, K, xs, ys):
    """gsplat/Cameras.cuh:457-470 + 261-265, global shutter: pixel centres, unit camera ray, world = R^T ray from -R^T t. xs, ys: integer pixel coordinates [P]"""
    R, t = viewmat[:3, :3], viewmat[:3, 3]
    u = (xs.to(F64) + 0.5 - K[0, 2]) / K[0, 0]
    v = (ys.to(F64) + 0.5 - K[1, 2]) / K[1, 1]
    d = torch.stack([u, v, torch.ones_like(u)], -1)
    d = d / d.norm(dim=-1, keepdim=True)
    return -(R.T @ t), d @ R          # (d @ R = (R^T d^T)^T)


def rasterize(means, quats, scales, opac, colors, viewmat, K, bg, W, H, tile, tile_offsets, flatten_ids):
    """-> render [H,W,3], alpha [H,W]. tile_offsets [th,tw] and flatten_ids [I] (one camera): the tile lists, front to back. bg [3] or None."""
    th, tw = (H + tile - 1) // tile, (W + tile - 1) // tile
    offs = [int(v) for v in torch.as_tensor(tile_offsets).reshape(-1)] + [int(len(flatten_ids))]
    flat = torch.as_tensor(flatten_ids).long()
    Rg = quat_to_rotmat(quats)
    M = Rg.transpose(1, 2) / scales[:, :, None]                    # S^-1 R^T
    rows = []
    for ty in range(th):
        cols = []
        for tx in range(tw):
            y0, y1, x0, x1 = ty * tile, min(ty * tile + tile, H), tx * tile, min(tx * tile + tile, W)
            ys, xs = torch.meshgrid(torch.arange(y0, y1), torch.arange(x0, x1), indexing="ij")
            ray_o, ray_d = pixel_rays(viewmat, K, xs.reshape(-1), ys.reshape(-1))
            g = flat[offs[ty * tw + tx]:offs[ty * tw + tx + 1]]
            P = ray_d.shape[0]
            if len(g) == 0:
                pix, T = torch.zeros(P, 3, dtype=F64), torch.ones(P, dtype=F64)
            else:
                Mg = M[g]
                gro = torch.einsum("gij,gj->gi", Mg, ray_o[None] - means[g])                 # [G,3]
                grd = torch.einsum("gij,pj->pgi", Mg, ray_d)                                   # [P,G,3]
                grd = grd / grd.norm(dim=-1, keepdim=True)
                c = torch.linalg.cross(grd, gro[None].expand_as(grd), dim=-1)
                a = torch.clamp(opac[g][None] * torch.exp(-0.5 * (c * c).sum(-1)), max=ALPHA_MAX)   # [P,G]
                with torch.no_grad():
                    valid = a >= ALPHA_MIN
                    live = valid & (torch.cumprod(torch.where(valid, 1 - a, torch.ones_like(a)), 1) > T_MIN)   # (the product only falls: once at <= 1e-4, the pixel is done)
                a = torch.where(live, a, torch.zeros_like(a))
                Tin = torch.cumprod(1 - a, 1)
                T = Tin[:, -1]
                Tbefore = torch.cat([torch.ones(P, 1, dtype=F64), Tin[:, :-1]], 1)
                pix = (a * Tbefore) @ colors[g]
            out = pix if bg is None else pix + T[:, None] * bg[None]
            cols.append((out.reshape(y1 - y0, x1 - x0, 3), (1 - T).reshape(y1 - y0, x1 - x0)))
        rows.append((torch.cat([c[0] for c in cols], 1), torch.cat([c[1] for c in cols], 1)))
    render = torch.cat([r[0] for r in rows], 0)
    alpha_img = torch.cat([r[1] for r in rows], 0)
    return render, alpha_img


# ---- loss (rasterizer.cpp:401: the image is clamp(render, 0, 1) as CHW; trainer.cpp:103-158) --------------------------------------------------------------------
L1_TAU = 1e-5   # |image - target| below this is "undecided" for a float32 implementation: some hundred ulp of a value in [0, 1], the rounding a render accumulates over a long tile list


def photometric(image_chw, target_chw, kind, lambda_dssim=0.2, undecided=None):
    """undecided (bool, like the image): elements whose |image - target| term is left out of the L1 mean - see step_gradients"""
    if kind == "mse":
        return ((image_chw - target_chw) ** 2).mean()
    assert kind == "l1_ssim"
    if undecided is None:
        return ssim_reference.photometric_loss(image_chw[None], target_chw[None], lambda_dssim)
    l1 = torch.where(undecided, torch.zeros_like(image_chw), (image_chw - target_chw).abs()).sum() / image_chw.numel()
    return (1 - lambda_dssim) * l1 + lambda_dssim * (1 - ssim_reference.fused_ssim(image_chw[None], target_chw[None], "valid"))


def step_loss(params, degree, viewmat, K, bg, W, H, tile, tile_offsets, flatten_ids, visible, target_chw, kind="mse", lambda_dssim=0.2, weight=1.0,
              scale_reg=0.0, opacity_reg=0.0, undecided=None):
    """params: the six tensors in FusedAdam's group order (means, sh0, shN, raw_scales, raw_quats, raw_opacities), float64.
    -> (total loss, weight * photometric part, render [H,W,3], clamped image [3,H,W])"""
    means, sh0, shN, raw_scales, raw_quats, raw_opac = params
    quats, scales, opac = activations(raw_quats, raw_scales, raw_opac)
    colors = sh_colors(degree, means, sh0, shN, viewmat, visible)
    render, _ = rasterize(means, quats, scales, opac, colors, viewmat, K, bg, W, H, tile, tile_offsets, flatten_ids)
    image = torch.clamp(render.permute(2, 0, 1), 0.0, 1.0)
    photo = weight * photometric(image, target_chw, kind, lambda_dssim, undecided(image) if undecided is not None else None)
    return photo + scale_reg * scales.mean() + opacity_reg * opac.mean(), photo, render, image


def step_gradients(params, *args, **kw):
    """-> (six gradients d total / d raw parameter by autograd, weight * photometric loss as a float, render, free)
    free: |x| has no derivative at 0, and where |image - target| < L1_TAU a float32 implementation may land on either side of it. Those elements of the L1 term
    (a handful per image, usually none) are left OUT of the gradients; for each of them `free` holds the six gradients of its term with the sign +1: any
    gradients + sum_u s_u free[u] with s_u in [-1, 1] - the subdifferential - is what a correct implementation may produce (fit_free)."""
    leaves = [f64(p).requires_grad_(True) for p in params]
    args = [f64(a) if torch.is_tensor(a) and a.is_floating_point() else a for a in args]
    kind, target = kw.get("kind", "mse"), args[-1]
    mark = (lambda image: (image.detach() - target).abs() < L1_TAU) if kind == "l1_ssim" else None
    total, photo, render, image = step_loss(leaves, *args, undecided=mark, **kw)
    zeros = lambda gs: [torch.zeros_like(p) if g is None else g for g, p in zip(gs, leaves)]
    free = []
    if mark is not None:
        coef = kw.get("weight", 1.0) * (1 - kw.get("lambda_dssim", 0.2)) / image.numel()
        for idx in mark(image).nonzero().tolist():
            free.append(zeros(torch.autograd.grad(coef * image[tuple(idx)], leaves, allow_unused=True, retain_graph=True)))
    grads = zeros(torch.autograd.grad(total, leaves, allow_unused=True))
    return grads, float(photo.detach()), render.detach(), free


def fit_free(got, grads, free, skip=()):
    """-> grads + sum_u s_u free[u], s_u in [-1, 1] chosen (least squares over the tensors not in `skip`, each scaled by its own norm) closest to `got`"""
    if not free:
        return grads
    use = [k for k in range(len(grads)) if k not in skip and grads[k].numel()]
    w = [1.0 / (float(grads[k].norm()) + 1e-300) for k in use]
    A = torch.stack([torch.cat([(f[k] * wk).reshape(-1) for k, wk in zip(use, w)]) for f in free], 1)
    b = torch.cat([((torch.as_tensor(got[k], dtype=F64) - grads[k]) * wk).reshape(-1) for k, wk in zip(use, w)])
    s = torch.linalg.lstsq(A, b[:, None]).solution[:, 0].clamp(-1.0, 1.0)
    return [g + sum(float(su) * f[k] for su, f in zip(s, free)) for k, g in enumerate(grads)]


# ---- MCMC noise (gsplat/RelocationCUDA.cu:88-144; applied by mcmc.cpp:349-393 in post_backward: after the backward, before the optimizer step) -----------------
def noise_term(raw_opac, raw_scales, raw_quats, noise, lr):
    """-> what add_noise adds to the means: lr * sigmoid(-100 (opacity - 0.005)) * (R diag(s^2) R^T) noise"""
    R = quat_to_rotmat(raw_quats)
    cov = R @ torch.diag_embed(torch.exp(2 * raw_scales)) @ R.transpose(1, 2)
    factor = lr / (1 + torch.exp(100 * torch.sigmoid(raw_opac) - 0.5))
    return factor[:, None] * torch.einsum("nij,nj->ni", cov, noise)


# ---- Adam (src/training/optimizers/fused_adam.cpp:66-92 + fastgs/optimizer/include/adam_kernels.cuh:28-35) -------------------------------------------------------
def adam_scalars(beta1, beta2, step_count):
    return 1.0 / (1.0 - beta1 ** step_count), 1.0 / (1.0 - beta2 ** step_count) ** 0.5


def adam_moments(m, v, g, beta1, beta2):
    return beta1 * m + (1 - beta1) * g, beta2 * v + (1 - beta2) * g * g


def adam_delta(m_new, v_new, lr, eps, bc1_rcp, bc2_sqrt_rcp):
    """-> the change of the parameter for the NEW moments"""
    return -(lr * bc1_rcp) * m_new / (torch.sqrt(v_new) * bc2_sqrt_rcp + eps)
