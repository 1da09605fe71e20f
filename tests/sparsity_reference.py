"""numpy restatement of the reference's ADMM sparsity optimiser (src/training/components/sparsity_optimizer.cpp), independent of the product code:
in float32 - operation for operation, the model the kernels have to match bit for bit given the same activated opacities - and in float64, the yardstick of
the loss and gradient bounds. The schedule predicates restate the header's inequalities (sparsity_optimizer.hpp:102-117)."""
import numpy as np

f32 = np.float32


def num_to_prune_f32(prune_ratio, n):
    """static_cast<int>(config_.prune_ratio * size): float times size_t is a FLOAT product, then truncation"""
    return int(f32(prune_ratio) * f32(n))


def num_to_prune_f64(prune_ratio, n):
    """what plain Python arithmetic gives instead: the double product of the float-rounded ratio"""
    return int(float(f32(prune_ratio)) * n)


def kth_smallest(x, k):
    """sort(x)[k - 1] in torch.sort's / np.sort's order (NaN last, -0 == +0)"""
    return np.sort(np.asarray(x).reshape(-1), kind="stable")[k - 1]


def prune_z(v, k):
    """sparsity_optimizer.cpp:152-168 with index = k: (v > sort(v)[k - 1]) * v, zeros for k == 0"""
    if k == 0:
        return np.zeros_like(v)
    thr = kth_smallest(v, k)
    return np.where(v > thr, v, np.zeros_like(v))


def update_state(opa, u, k):
    """:83-86 -> (z, u') in the dtype of the inputs: z = prune_z(opa + u); u' = u + (opa - z)"""
    v = opa + u
    z = prune_z(v, k)
    return z, u + (opa - z)


def sigmoid64(raw):
    return 1.0 / (1.0 + np.exp(-np.asarray(raw, np.float64)))


def loss_and_grad64(raw, z, u, rho, scale=1.0):
    """compute_loss (:57-59) and its gradient w.r.t. the raw opacities in float64: scale rho / 2 |d|^2, scale rho d opa (1 - opa), d = opa - z + u"""
    opa = sigmoid64(raw)
    d = opa - np.asarray(z, np.float64) + np.asarray(u, np.float64)
    return scale * 0.5 * rho * float((d * d).sum()), scale * rho * d * opa * (1.0 - opa)


def prune_mask_is_valid(raw, mask, n_prune):
    """exactly n_prune ones, every pruned value <= every kept one"""
    raw, mask = np.asarray(raw).reshape(-1), np.asarray(mask).reshape(-1).astype(bool)
    if int(mask.sum()) != n_prune:
        return False
    if n_prune == 0 or n_prune == raw.shape[0]:
        return True
    return bool(raw[mask].max() <= raw[~mask].min())


def should_update(it, start, steps, every):
    rel = it - start
    return it >= start and rel > 0 and rel < steps and rel % every == 0


def should_apply_loss(it, start, steps):
    return it >= start and it < start + steps


def should_prune(it, start, steps):
    return it == start + steps
