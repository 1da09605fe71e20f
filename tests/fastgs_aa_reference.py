"""Exact host model of the fastgs antialiased mode's opacity compensation, independent of the code under test:
rho = sqrt(max(0, det(Sigma2d) / det(Sigma2d + 0.3 I))) with Sigma2d = J W Sigma3d W^T J^T, J the EWA Jacobian at the camera-space point clamped to 1.15 x the
image (kernels_forward.cuh). float64 throughout: numpy for values, torch with straight-through clamps (the backward's convention) for derivatives."""
import numpy as np
import torch

DILATION = 0.3


def _rho(xp, means, scales_raw, rot_raw, w2c, fx, fy, cx, cy, W, H, clamp):
    q = rot_raw / ((rot_raw ** 2).sum(-1) ** 0.5)[:, None]
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = xp.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                  2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)
    M = R * xp.exp(scales_raw)[:, None, :]                       # Sigma3d = M M^T
    cam = means @ w2c[:3, :3].T + w2c[:3, 3]
    depth = cam[:, 2]
    tx = clamp(cam[:, 0] / depth, (-0.15 * W - cx) / fx, (1.15 * W - cx) / fx)
    ty = clamp(cam[:, 1] / depth, (-0.15 * H - cy) / fy, (1.15 * H - cy) / fy)
    j1 = (fx / depth)[:, None] * (w2c[0, :3] - tx[:, None] * w2c[2, :3])     # rows of J W
    j2 = (fy / depth)[:, None] * (w2c[1, :3] - ty[:, None] * w2c[2, :3])
    u, v = (j1[:, :, None] * M).sum(1), (j2[:, :, None] * M).sum(1)          # M^T (J W)^T
    a0, b, c0 = (u * u).sum(-1), (u * v).sum(-1), (v * v).sum(-1)
    return (a0 * c0 - b * b) / ((a0 + DILATION) * (c0 + DILATION) - b * b)   # rho^2 before the max(0, .)


def rho64(means, scales_raw, rot_raw, w2c, fx, fy, cx, cy, W, H):
    """[N] float64 values; inputs are taken at float32 (what the device sees), arithmetic in float64"""
    a = [np.asarray(v, np.float32).astype(np.float64) for v in (means, scales_raw, rot_raw, w2c)]
    return np.sqrt(np.maximum(0.0, _rho(np, *a, fx, fy, cx, cy, W, H, np.clip)))


def rho_vjp(weight, means, scales_raw, rot_raw, w2c, fx, fy, cx, cy, W, H):
    """J_rho^T weight -> (d means, d scales_raw, d rot_raw), float64 numpy; rows with weight 0 (invisible primitives; rho = 0 among them) are exact zeros"""
    m, s, q, w = [torch.tensor(np.asarray(v, np.float32).astype(np.float64), requires_grad=k < 3) for k, v in enumerate((means, scales_raw, rot_raw, w2c))]
    wt = torch.tensor(np.asarray(weight, np.float64))
    st = lambda v, lo, hi: v + (v.clamp(lo, hi) - v).detach()    # the value is clamped, the derivative is the unclamped one's
    r2 = _rho(torch, m, s, q, w, fx, fy, cx, cy, W, H, st)
    on = wt != 0
    (wt * torch.sqrt(torch.where(on, r2, torch.ones_like(r2)))).sum().backward()
    return tuple(np.where(on.numpy()[:, None], g.grad.numpy(), 0.0) for g in (m, s, q))
