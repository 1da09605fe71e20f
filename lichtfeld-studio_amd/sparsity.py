"""ADMM sparsity optimisation: opacity pruning to a target Gaussian count (the reference's src/training/components/sparsity_optimizer.{hpp,cpp},
--enable-sparsity). After the base run the trainer keeps training for `sparsify_steps` iterations with the penalty rho / 2 |sigmoid(raw) - z + u|^2 on the
opacities, where z is the projection of sigmoid(raw) + u onto "at most (1 - prune_ratio) N non-zeros" and u the scaled dual variable, both refreshed every
`update_every` iterations; then the prune_ratio N Gaussians of lowest opacity are removed.

  select_kth               sort(x)[k - 1] without a sort: a radix select, result on the device
  admm_update              z, u <- the ADMM state update (sparsity_optimizer.cpp:83-86, prune_z :152-168)
  admm_loss_grad           the penalty and its gradient w.r.t. the raw opacities (compute_loss :57-59 + autograd backward)
  admm_prune_mask          the final mask (get_prune_mask :110-123)
  ADMMSparsityOptimizer    the reference class over them

The four operators are HIP kernels behind the C ABI (csrc/sparsity.hip). None of them reads anything back to the host: the reference's sort, its
`(z == 0).sum().item()` statistics and the `.item()` calls of the final prune have no counterpart here.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from .capi import LfsError, check, load_library, ptr, require_gpu, stream, workspace

Tensor = torch.Tensor


def _size_t(fn):
    fn.restype = C.c_size_t
    return fn


def _flat_f32(t: Tensor, what: str) -> Tensor:
    if t.dtype != torch.float32:
        raise LfsError(f"{what} must be float32")
    t = t.detach()
    if not t.is_contiguous():
        raise LfsError(f"{what} must be contiguous")
    return t.view(-1)


def select_kth(x: Tensor, k: int, out: Optional[Tensor] = None) -> Tensor:
    """f32 [N], 1 <= k <= N -> f32 [1] on the device: sort(x)[k - 1] in torch.sort's order (-0 == +0, NaN above +inf)."""
    x = _flat_f32(x, "select_kth: x")
    require_gpu(x, out)
    lib = load_library()
    N = x.shape[0]
    if out is None:
        out = torch.zeros(1, dtype=torch.float32, device=x.device)
    ws = workspace(_size_t(lib.lfs_select_kth_workspace_bytes)(C.c_int64(N)), x.device, "sparsity")
    check(lib.lfs_select_kth_f32(ptr(x), C.c_int64(N), C.c_int64(int(k)), ptr(out), ptr(ws), C.c_size_t(ws.numel()), stream()), "select_kth")
    return out


def admm_update(raw_opacities: Tensor, u: Tensor, z: Tensor, k: int) -> None:
    """In place: z = prune_z(sigmoid(raw) + u) with the k-th smallest as threshold (k == 0: z = 0), u += sigmoid(raw) - z."""
    raw, u_, z_ = _flat_f32(raw_opacities, "admm_update: raw_opacities"), _flat_f32(u, "admm_update: u"), _flat_f32(z, "admm_update: z")
    require_gpu(raw, u_, z_)
    N = raw.shape[0]
    if u_.shape[0] != N or z_.shape[0] != N:
        raise LfsError("admm_update: u and z must have one element per opacity")
    lib = load_library()
    ws = workspace(_size_t(lib.lfs_admm_update_workspace_bytes)(C.c_int64(N)), raw.device, "sparsity")
    check(lib.lfs_admm_update(ptr(raw), ptr(u_), ptr(z_), C.c_int64(N), C.c_int64(int(k)), ptr(ws), C.c_size_t(ws.numel()), stream()), "admm_update")


def admm_loss_grad(raw_opacities: Tensor, z: Tensor, u: Tensor, rho: float, scale: float, g_raw_opacities: Tensor, accumulate: bool,
                   loss: Optional[Tensor] = None) -> None:
    """g_raw_opacities (+)= scale rho d sigmoid'(raw), loss[0] += scale rho / 2 sum d^2 with d = sigmoid(raw) - z + u. `loss` None: the gradient only."""
    raw, z_, u_ = _flat_f32(raw_opacities, "admm_loss_grad: raw_opacities"), _flat_f32(z, "admm_loss_grad: z"), _flat_f32(u, "admm_loss_grad: u")
    g = _flat_f32(g_raw_opacities, "admm_loss_grad: g_raw_opacities")
    require_gpu(raw, z_, u_, g, loss)
    N = raw.shape[0]
    if z_.shape[0] != N or u_.shape[0] != N or g.shape[0] != N:
        raise LfsError("admm_loss_grad: z, u and the gradient must have one element per opacity")
    if loss is not None and (loss.dtype != torch.float32 or loss.numel() < 1):
        raise LfsError("admm_loss_grad: loss must be a float32 tensor")
    lib = load_library()
    ws = workspace(_size_t(lib.lfs_admm_loss_grad_workspace_bytes)(C.c_int64(N)), raw.device, "sparsity")
    check(lib.lfs_admm_loss_grad(ptr(raw), ptr(z_), ptr(u_), C.c_int64(N), C.c_float(rho), C.c_float(scale), ptr(g), C.c_int(int(bool(accumulate))), ptr(loss),
                                 ptr(ws), C.c_size_t(ws.numel()), stream()), "admm_loss_grad")


def admm_prune_mask(raw_opacities: Tensor, n_prune: int) -> Tensor:
    """-> bool [N] with exactly n_prune ones: the lowest raw opacities, ties at the boundary value to the lowest indices."""
    raw = _flat_f32(raw_opacities, "admm_prune_mask: raw_opacities")
    require_gpu(raw)
    N = raw.shape[0]
    lib = load_library()
    mask = torch.empty(N, dtype=torch.uint8, device=raw.device)
    ws = workspace(_size_t(lib.lfs_admm_prune_mask_workspace_bytes)(C.c_int64(N)), raw.device, "sparsity")
    check(lib.lfs_admm_prune_mask(ptr(raw), C.c_int64(N), C.c_int64(int(n_prune)), ptr(mask), ptr(ws), C.c_size_t(ws.numel()), stream()), "admm_prune_mask")
    return mask.view(torch.bool)


def num_to_prune(prune_ratio: float, n: int) -> int:
    """static_cast<int>(prune_ratio * size) with a float ratio (sparsity_optimizer.cpp:111, :149, :157): the product is single precision, truncated."""
    return int(np.float32(prune_ratio) * np.float32(n))


@dataclass
class Config:  # ADMMSparsityOptimizer::Config, sparsity_optimizer.hpp:87-93
    sparsify_steps: int = 15000
    init_rho: float = 0.0005
    prune_ratio: float = 0.6
    update_every: int = 50
    start_iteration: int = 30000


class ADMMSparsityOptimizer:
    """sparsity_optimizer.hpp:85-135. compute_loss + backward() are ONE call here, add_loss_and_grad."""
    Config = Config

    def __init__(self, config: Optional[Config] = None):
        self.config = config if config is not None else Config()
        self.u: Optional[Tensor] = None
        self.z: Optional[Tensor] = None
        self._initialized = False

    # -- the schedule: the header's inequalities -----------------------------------------------------------------------
    def should_update(self, it: int) -> bool:
        c = self.config
        rel = it - c.start_iteration
        return it >= c.start_iteration and rel > 0 and rel < c.sparsify_steps and rel % c.update_every == 0

    def should_apply_loss(self, it: int) -> bool:
        c = self.config
        return it >= c.start_iteration and it < (c.start_iteration + c.sparsify_steps)

    def should_prune(self, it: int) -> bool:
        c = self.config
        return it == (c.start_iteration + c.sparsify_steps)

    def is_initialized(self) -> bool:
        return self._initialized

    def get_num_to_prune(self, raw_opacities: Optional[Tensor]) -> int:
        if raw_opacities is None or raw_opacities.numel() == 0:
            return 0
        return num_to_prune(self.config.prune_ratio, raw_opacities.numel())

    # -- state ---------------------------------------------------------------------------------------------------------
    def initialize(self, raw_opacities: Tensor) -> None:
        """u = 0, z = prune_z(sigmoid(raw) + u) (:27-29): the state update's z on a zero-filled u."""
        if raw_opacities is None or raw_opacities.numel() == 0:
            raise LfsError("Invalid opacity tensor for initialization")
        n = raw_opacities.numel()
        self.z = torch.empty(n, dtype=torch.float32, device=raw_opacities.device)
        scratch = torch.zeros(n, dtype=torch.float32, device=raw_opacities.device)
        admm_update(raw_opacities, scratch, self.z, self.get_num_to_prune(raw_opacities))   # (the u the call returns is discarded: initialize keeps u = 0, :28-29)
        self.u = scratch.zero_()
        self._initialized = True

    def update_state(self, raw_opacities: Tensor) -> None:
        if not self._initialized:
            return self.initialize(raw_opacities)
        if raw_opacities is None or raw_opacities.numel() == 0:
            raise LfsError("Invalid opacity tensor for state update")
        if raw_opacities.numel() != self.u.numel():
            raise LfsError("the number of Gaussians changed during the sparsification phase")
        admm_update(raw_opacities, self.u, self.z, self.get_num_to_prune(raw_opacities))

    def add_loss_and_grad(self, raw_opacities: Tensor, grad_view: Tensor, loss_acc: Optional[Tensor], scale: float = 1.0) -> None:
        """grad_view += scale dL/draw, loss_acc += scale L for L = rho / 2 |sigmoid(raw) - z + u|^2. Initialises the state on first use (trainer.cpp:179)."""
        if not self._initialized:
            self.initialize(raw_opacities)
        if raw_opacities.numel() != self.u.numel():
            raise LfsError("the number of Gaussians changed during the sparsification phase")
        admm_loss_grad(raw_opacities, self.z, self.u, self.config.init_rho, scale, grad_view, True, loss_acc)

    def get_prune_mask(self, raw_opacities: Tensor) -> Tensor:
        if raw_opacities is None or raw_opacities.numel() == 0:
            raise LfsError("Invalid opacity tensor for pruning")
        return admm_prune_mask(raw_opacities, self.get_num_to_prune(raw_opacities))
