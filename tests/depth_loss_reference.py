"""float64 numpy model of the depth loss (lfs_depth_prepare + lfs_depth_l1_loss_fwd_bwd):
    valid_p = target finite and > 0,  m_p = valid_p * M_p / 255 (M_p the mask byte; 1 without a mask),
    loss = weight * sum_p m_p |D_p - t_p| / max(sum_p m_p, 1),   dloss/dD_p = weight * m_p * sign(D_p - t_p) / max(sum_p m_p, 1)."""
import numpy as np


def weights(target, mask_u8=None):
    t = np.asarray(target, np.float64)
    valid = np.isfinite(t) & (t > 0)
    m = valid.astype(np.float64)
    if mask_u8 is not None:
        m = m * (np.asarray(mask_u8).astype(np.float64) / 255.0)
    return valid, m


def int_sum(target, mask_u8=None):
    """the integer lfs_depth_prepare leaves on the device: sum over the valid pixels of the mask byte (255 without a mask)"""
    valid, _ = weights(target, mask_u8)
    M = np.full(valid.shape, 255, np.int64) if mask_u8 is None else np.asarray(mask_u8).astype(np.int64)
    return int((M * valid).sum())


def loss_and_grad(depth, target, mask_u8, weight):
    D = np.asarray(depth, np.float32).astype(np.float64)
    valid, m = weights(target, mask_u8)
    t = np.where(valid, np.asarray(target, np.float64), 0.0)
    diff = np.where(valid, D - t, 0.0)
    norm = max(m.sum(), 1.0)
    return float(weight * (m * np.abs(diff)).sum() / norm), weight * m * np.sign(diff) / norm
