"""Float64 PyTorch model of the masked losses (test infrastructure only), written from the formulas of DESIGN.md §8 "Masked training" on top of
tests/ssim_reference.py. M is the mask as a float64 [H,W] tensor of byte values (255 = the pixel counts fully, 0 = ignored); r, t are [3,H,W].

    L1m   = sum_c sum_p M_p |r - t| / (3 S_img)                    (0 when S_img == 0)
    SSIMm = sum_c sum_{p in crop} M_p ssim_{c,p} / (3 S_crop)       (the SSIM map of the UNMASKED images)
    loss  = (1 - lambda) L1m + lambda (1 - SSIMm)                   (the SSIM term is 0 when S_crop == 0)

crop = the interior with 5 pixels removed per side when H > 10 and W > 10, else the whole image - and then, the kept quirk of the unmasked loss, the SSIM term
contributes its value and no gradient."""
import torch

import ssim_reference as ref


def can_crop(H, W):
    return H > 10 and W > 10


def crop(x):
    """the last two dimensions cropped by the loss's rule"""
    H, W = x.shape[-2], x.shape[-1]
    return x[..., 5:H - 5, 5:W - 5] if can_crop(H, W) else x


def sums(M):
    """(S_img, S_crop) as Python ints"""
    return int(M.sum().item()), int(crop(M).sum().item())


def masked_l1(r, t, M):
    s_img = M.sum()
    return (M * (r - t).abs()).sum() / (3 * s_img) if float(s_img) > 0 else r.sum() * 0


def masked_ssim_term(r, t, M):
    """lambda's factor: 1 - SSIMm (0 under an empty crop); no gradient when the image cannot be cropped"""
    H, W = r.shape[-2], r.shape[-1]
    Mc = crop(M)
    if float(Mc.sum()) <= 0:
        return r.sum() * 0
    smap = ref.ssim_map(r[None], t[None])[0]
    if not can_crop(H, W):
        smap = smap.detach()
    return 1 - (Mc * crop(smap)).sum() / (3 * Mc.sum())


def masked_photometric_loss(r, t, M, lam):
    return (1 - lam) * masked_l1(r, t, M) + lam * masked_ssim_term(r, t, M)


def masked_mse(r, t, M):
    s_img = M.sum()
    return (M * (r - t) ** 2).sum() / (3 * s_img) if float(s_img) > 0 else r.sum() * 0


def alpha_penalty(alpha, M, w_a):
    """-> (value, d value / d alpha): w_a * sum (255 - M) alpha / (255 H W)"""
    H, W = M.shape
    g = w_a * (255 - M) / (255.0 * H * W)
    return (g * alpha).sum(), g
