"""Minimal stand-in for Trainer::train_step (/root/reference/src/training/trainer.cpp:579-760) on
the --gut path: render -> loss -> backward -> (all-reduce) -> FusedAdam::step -> zero_grad ->
scheduler.step. The reference's app shell (dataset IO, strategies, viewer, checkpoints) is out of
scope; the loss here is the rasterizer-only MSE of SURVEY.md §8d.
"""
from __future__ import annotations

import math

from dataclasses import dataclass
from typing import List, Optional

import torch

from . import dist as lfs_dist
from .fused_adam import ExponentialLR, FusedAdam, default_param_groups
from .rasterizer import Camera, RenderMode, SplatModel, rasterize
from .scenes import Scene


@dataclass(frozen=True)
class StepPlan:
    """Which form of the training step runs, and with which fusions (GutTrainer._train_step dispatches on it)."""
    path: str            # "fastgs" | "autograd" | "cxx_all" | "cxx_views" | "batch_views" | "py_views"
    inline_shN: bool     # shN's Adam update happens inside the SH backward (no shN gradient tensor)
    inline_all: bool     # every parameter is updated by the backward kernels (no gradient tensors at all)
    inline_shard: bool   # SH-sharded: the owners' multi-view SH backward applies the shard's Adam update
    multi: bool          # the multi-rank code path (world > 1, or LFS_DIST_FORCE_COLLECTIVES on one GPU)
    skip_deferred: bool  # the shN segment stays out of the flat all-reduce
    freeze_shN: bool = False   # one-call form with options (plan_step(one_call=True)): FusedAdam skips shN this step (iteration <= 1000), the tail leaves it alone


def plan_step(*, rasterizer: str, fused_l2: bool, world: int, force_collectives: bool, sh_sharded: bool, shard_rows: int, n_views: int, loss: str,
              strategy: Optional[str], refining: bool, iteration: int, has_shN: bool, optimizer_fused: bool, bilateral: bool, inline_shN_adam: bool = True,
              inline_all_adam: bool = True, cxx_step: bool = True, batch_views: bool = True, factored_sh: bool = False, one_call: bool = False,
              masked: bool = False) -> StepPlan:
    """Pure function of the configuration -> the step form. The rules, in the order they are applied:
      * fastgs rasterizer -> its own step; fused_l2 off -> torch autograd over the op-by-op mirror.
      * shN's Adam update moves into the SH backward (inline_shN) when Adam reads shN anyway (iteration > 1000, fused_adam.cpp:68-70), there IS an shN, the
        optimizer is the fused one, and the strategy does not touch shN before the optimizer step: no strategy, or MCMC between refinements (post_backward then
        only adds noise to the means, mcmc.cpp:362-384) - never on refining iterations (relocation rewrites shN rows and moments first).
        - replicated layout: additionally one view on one rank (gradient of a single view, no all-reduce: nothing else needs the tensor)
        - several views on one rank (batch_views): inside the ONE multi-view SH backward
        - SH-sharded, one view per rank: the owners' multi-view backward updates the shard (inline_shard)
      * inline_all (no gradient tensor at all) = inline_shN on one view / one rank + MSE + no strategy + no bilateral grid.
      * C++ step driver (cxx_step): inline_all -> ONE call (cxx_all); otherwise its per-view form whenever the layout is replicated and the rank has one view
        or runs the multi-rank path (cxx_views). Several views on one rank without collectives -> batch_views. Everything else - SH-sharded ranks, cxx_step
        off - -> the kernels enqueued from Python view by view (py_views).
      * one_call (opt-in, GutTrainer(one_call=True)): one view on one rank ALSO takes the one-call form (cxx_all, lfs_gut_train_step_opt) for what the reference trains -
        loss "mse" or "l1_ssim", no strategy or MCMC between refinements (its noise is folded into the tail), at ANY iteration (<= 1000: freeze_shN, the tail skips
        shN as FusedAdam does) - given the fused optimizer, an shN, cxx_step and no bilateral grid. Everything else keeps the form it has with the keyword off.
      * masked (the step carries an image mask): never the one-call form (cxx_all), neither through inline_all nor through one_call - the one-call C++ step
        computes its loss inside, without a mask; the step takes the form it has without those two rules (GutTrainer raises for batch_views / py_views).
      * pose optimisation is not an input: GutTrainer's constructor admits it on the fastgs rasterizer of one rank only, whose plan has no inline form."""
    multi = world > 1 or force_collectives
    if rasterizer == "fastgs":
        return StepPlan("fastgs", False, False, False, multi, iteration <= 1000)
    if not fused_l2:
        return StepPlan("autograd", False, False, False, multi, iteration <= 1000)
    strat_ok = strategy is None or (strategy == "mcmc" and not refining)
    adam_reads_shN = iteration > 1000 and has_shN and optimizer_fused
    inline_one = inline_shN_adam and not multi and not sh_sharded and n_views == 1 and strat_ok and adam_reads_shN
    inline_all = inline_one and inline_all_adam and strategy is None and loss == "mse" and not bilateral and not masked
    inline_shard = inline_shN_adam and sh_sharded and n_views == 1 and adam_reads_shN and shard_rows > 0 and not refining
    skip_deferred = iteration <= 1000 or sh_sharded
    if (one_call and not masked and cxx_step and not multi and not sh_sharded and n_views == 1 and strat_ok and has_shN and optimizer_fused and not bilateral
            and loss in ("mse", "l1_ssim")):
        return StepPlan("cxx_all", adam_reads_shN, True, False, multi, skip_deferred, freeze_shN=not adam_reads_shN)
    if factored_sh and multi and not sh_sharded:
        # replicated layout with the factored SH exchange (dist.ColorGradExchange): per view rasterizer backward + finish, rows gathered, ONE multi-view SH backward
        # over every rank's views with shN's Adam update inside whenever Adam reads shN and no refinement rewrites it first; sh0 / shN never enter the all-reduce
        if not cxx_step:
            # (a shape the speculative C++ step does not take - GutTrainer.__init__ rejects factored_sh for those up front; densification growing N past the index-bit
            #  limit mid-run lands here: an error on every rank at the same iteration, N is replicated)
            raise ValueError("the factored SH exchange runs through the C++ step driver (cxx_step): unsupported problem shape or cxx_step switched off")
        return StepPlan("cxx_factored", inline_shN_adam and strat_ok and adam_reads_shN, False, False, multi, True)
    if inline_all and cxx_step:
        return StepPlan("cxx_all", True, True, False, multi, skip_deferred)
    if cxx_step and not sh_sharded and (multi or n_views == 1):
        return StepPlan("cxx_views", inline_one, False, False, multi, skip_deferred)
    if batch_views and not multi and not sh_sharded and n_views > 1:
        return StepPlan("batch_views", inline_shN_adam and strat_ok and adam_reads_shN, False, False, multi, skip_deferred)
    return StepPlan("py_views", inline_one, inline_all, inline_shard, multi, skip_deferred)


class GutTrainer:
    def __init__(self, scene: Scene, device, iterations: int = 7000, world: int = 1, rank: int = 0,
                 views_per_rank: int = 1, fused_adam: bool = True, fused_l2: bool = True, loss: str = "mse", lambda_dssim: float = 0.2,
                 strategy: Optional[str] = None, opt_params=None, scene_scale: float = 1.0, seed: int = 0, rasterizer: str = "gut",
                 use_bilateral_grid: bool = False, bilateral_grid_dims=(16, 16, 8), bilateral_grid_lr: float = 2e-3, tv_loss_weight: float = 10.0,
                 sh_sharded: Optional[bool] = None, factored_sh: bool = False, one_call: bool = False, pose_optimization: str = "none", pose_lr: float = 1e-5,
                 enable_sparsity: bool = False, sparsify_steps: int = 15000, init_rho: float = 0.0005, prune_ratio: float = 0.6, sparsity_update_every: int = 50,
                 mask_mode: str = "none", mask_alpha_weight: float = 1.0, antialiasing: bool = False, depth_loss: str = "none", depth_weight=(1.0, 0.01),
                 filter3d: bool = False, filter3d_every: int = 100, filter3d_variance: float = 0.2, absgrad: bool = False, visible_adam: bool = False,
                 contribution_prune_at=(), contribution_threshold: float = 0.01, background=(0.0, 0.0, 0.0), background_mode: str = "constant",
                 background_jitter: bool = True):
        """strategy: None (fixed set of Gaussians: the benchmark), "mcmc" (strategies.MCMC: relocation + growth + SGLD noise, with
        the scale / opacity regularisers of trainer.cpp:132-158) or "default" (ADC; needs densification_info, see strategies.py).
        `seed` seeds the strategy's generator: the same on every rank, so replicas densify identically.
        one_call: one view per step on one rank takes the one-call C++ step (no host read, no gradient tensors) for loss "l1_ssim", for MCMC between refinements and
        while iteration <= 1000 as well, not only for the MSE benchmark configuration (plan_step). Same trajectory as the default forms; off by default. A model with
        SH degree 4 (more than 16 coefficients per channel) keeps the default forms: the switch has no effect there.
        pose_optimization: "none" | "direct" | "mlp" (trainer.cpp:366-389; poseopt.py): a learned correction of every training camera's world-to-camera transform,
        trained with Adam(pose_lr) on the camera gradient of the fastgs backward. fastgs rasterizer, one rank.
        enable_sparsity (trainer.cpp:331-360; sparsity.py): the run is extended by `sparsify_steps` iterations after the `iterations` of the base run. During them the
        ADMM penalty (init_rho) pulls the opacities towards a state with prune_ratio of them at zero, refreshed every sparsity_update_every iterations, and no
        strategy refinement, noise or SH-degree change happens; at the last iteration int(prune_ratio * N) Gaussians of lowest opacity are removed. `total_iterations`
        is the length of the whole run. The learning-rate schedule stays the base run's.
        mask_mode: "none" | "ignore" | "segment" (DESIGN.md 8 "Masked training"): what train_step(masks=...) does with a view's mask. "ignore": the loss weights every
        pixel by its mask byte (the masked loss kernels). "segment": additionally the rendered opacity outside the mask is penalised with mask_alpha_weight (L1 + D-SSIM
        on the fastgs rasterizer, whose backward takes an alpha gradient; the autograd form of the 3DGUT rasterizer as well).
        antialiasing (OptimizationParameters::antialiasing): every fastgs render of the trainer runs in the antialiased mode (FastGSSettings.antialiased).
        fastgs rasterizer only.
        filter3d (filter3d.py): the 3D smoothing filter of Mip-Splatting - every fastgs render of the trainer takes the per-Gaussian filter variance
        computed over ALL training views (filter3d_variance: the paper's 0.2). It is recomputed before the first step, after every iteration in which the strategy
        changed the model (an ADC refinement, an MCMC relocation or growth, the sparsity prune), and otherwise every filter3d_every iterations (the means move).
        Every rank computes the same filter from the replicated means: no collective. Combines with antialiasing (together: Mip-Splatting), masks, the depth loss,
        pose optimisation (the filter uses the stored cameras) and sparsity. fastgs rasterizer only. export_model() returns the raw parameters: bake them
        (filter3d.bake) before writing a file for a viewer.
        absgrad (AbsGS, gsplat's absgrad): ADC's densification_info takes the norm of the per-pixel ABSOLUTE screen-space gradients, which do not cancel
        on a large Gaussian over fine texture (FastGSSettings.absgrad on every view whose backward feeds densification_info). Renders and gradients are unchanged.
        fastgs rasterizer with strategy="default" only; OptimizationParameters.for_strategy("default", absgrad=True) carries the matching grad_threshold.
        depth_loss: "none" | "invdepth" | "depth" (DESIGN.md 8g): what train_step(depths=...) supervises - the accumulated inverse depth (the Inria trainer's
        convention: monocular depth, scale and offset fitted per image) or the accumulated depth of the view against a losses.PreparedDepth, by a masked L1 whose weight
        decays exponentially from depth_weight[0] (first iteration) to depth_weight[1] (iteration `iterations`) - the log-linear interpolation of the Inria trainer's
        depth_l1_weight. fastgs rasterizer, one rank. With "none" (and on steps without depths) the trainer plans and computes what it always did.
        visible_adam (gsplat's visible_adam / SelectiveAdam, the official code's sparse_adam): the optimizer step updates only the Gaussians that at least
        one view of the step projected onto a tile (n_touched != 0 after the preprocess - the predicate of the backward's visibility count); parameters and Adam moments
        of the others are neither read nor written, so they keep their values instead of drifting along a stale momentum, and the step streams 1652 B per VISIBLE
        Gaussian. The step counts, and with them the bias corrections, stay global. Consequence: gradient terms that reach every Gaussian - MCMC's scale and opacity
        regularisers - do not move Gaussians outside the step's views. On an iteration in which the strategy refines (rows are replaced before the optimizer runs) the
        step is the dense one. fastgs rasterizer, one rank, without enable_sparsity and one_call. Off: the trainer plans and computes what it always did.
        contribution_prune_at (contribution.py): at the end of each listed iteration (1-based, after the optimizer step) the blending-weight statistic
        is computed over ALL training views with the trainer's own render settings (antialiasing, the current 3D filter, camera(v)), and every Gaussian whose
        maximum blending weight over all training rays is below contribution_threshold (RadSplat's 0.01) is removed - parameters, both Adam moments and the
        strategy's accumulators follow as in every other removal; the 3D filter is recomputed and the visibility words are rebuilt. The statistic follows the image:
        an instance that only terminates pixels counts as 0, so a prune is a training-time operation that the remaining iterations heal. fastgs rasterizer, one
        rank, not with strategy="mcmc" (it holds the count), sh_sharded or one_call. Empty (default): the trainer plans and computes what it always did.
        background, background_mode (background.py): the colour every step composites its render - and, with train_step(alphas=...), its RGBA targets -
        over. background: "black" | "white" | a triple in [0,1] (the official trainer's --white_background). background_mode "constant": that colour; "random": one
        colour per step, shared by the step's views, from torch.rand(3) on a CPU generator seeded with `seed` (the same on every rank and in every rerun, no device
        read; the official trainer's random_background); "modulated": the reference's bg_modulation - a sine-modulated colour mixed into `background` for the first
        three quarters of the run (background_jitter: its +-0.03 jitter, from the same CPU generator). The fastgs route hands the three floats to its compose kernels
        by value (fastgs.render_and_backward(background=)); on the 3DGUT route, whose kernels read the colour from device memory, it is copied into self.bg before
        the step. Every step form of both routes takes it. `last_background` is the colour of the last step. With the defaults nothing new is launched, self.bg is
        never written and every plan is what it was."""
        from . import background as lfs_background
        self.background = lfs_background.parse_background(background)
        if background_mode not in lfs_background.MODES:
            raise ValueError(f"Invalid background mode: {background_mode} (one of {lfs_background.MODES})")
        self.background_mode, self.background_jitter = background_mode, bool(background_jitter)
        self._bg_generator = torch.Generator().manual_seed(int(seed))   # CPU: every rank draws the same colours, nothing is read back
        self.last_background = self.background
        self._step_bg = None            # the colour of the step in flight when it is not black (None: the step composes nothing)
        self._alphas = None             # the step's RGBA planes (fastgs route; the other routes composite their targets before the step)
        contribution_prune_at = tuple(int(i) for i in contribution_prune_at)
        if contribution_prune_at:
            if rasterizer == "gut":
                raise ValueError("contribution_prune_at is not wired into the 3DGUT route (rasterizer='gut'): the blending-weight statistic is a kernel of the EWA "
                                 "blend path. Use rasterizer='fastgs'.")
            if world > 1:
                raise ValueError("contribution_prune_at is implemented for one rank (world == 1): every rank would have to reduce the statistic over all views. Use world=1.")
            if sh_sharded:
                raise ValueError("contribution_prune_at cannot be combined with sh_sharded: that layout belongs to the fused 3DGUT step. Use sh_sharded=False.")
            if strategy == "mcmc":
                raise ValueError("contribution_prune_at cannot be combined with strategy='mcmc': MCMC holds the Gaussian count and would relocate onto the freed rows. "
                                 "Use strategy='default' or no strategy.")
            if one_call:
                raise ValueError("contribution_prune_at cannot be combined with one_call: the one-call C++ step keeps its own view of the model's size. Use one_call=False.")
            bad = [i for i in contribution_prune_at if not 1 <= i <= int(iterations)]
            if bad:
                raise ValueError(f"contribution_prune_at names iterations outside 1..{int(iterations)}: {bad}")
            if not 0.0 < float(contribution_threshold) < 1.0:
                raise ValueError(f"contribution_threshold must lie in (0, 1) (got {contribution_threshold}): it is compared with a blending weight")
        self.contribution_prune_at, self.contribution_threshold = frozenset(contribution_prune_at), float(contribution_threshold)
        self.contribution_log = []      # (iteration, N before, N after) of every contribution prune
        if visible_adam:
            if rasterizer == "gut":
                raise ValueError("visible_adam is not wired into the 3DGUT route (rasterizer='gut'): nothing on that route produces the visibility bits yet, and its "
                                 "fused tail applies Adam itself. Use rasterizer='fastgs'.")
            if world > 1:
                raise ValueError("visible_adam is implemented for one rank (world == 1): the visibility bits would need an OR-reduction across ranks. Use world=1.")
            if enable_sparsity:
                raise ValueError("visible_adam cannot be combined with enable_sparsity: the ADMM penalty must reach every opacity. Use visible_adam=False for a "
                                 "sparsifying run.")
            if one_call:
                raise ValueError("visible_adam cannot be combined with one_call: the one-call C++ step applies Adam inside its own kernels. Use one_call=False.")
            if not fused_adam:
                raise ValueError("visible_adam needs fused_adam=True: the visible-only update is the one multi-tensor launch")
        self.visible_adam = bool(visible_adam)
        self._vis_bits = None           # int32 [ceil(N / 32)]: the union of the step's views, rebuilt when N changes
        if depth_loss not in ("none", "invdepth", "depth"):
            raise ValueError(f"Invalid depth loss: {depth_loss}")
        if depth_loss != "none":
            if rasterizer == "gut":
                raise ValueError("depth supervision is not wired into the 3DGUT route (rasterizer='gut'): its step forms render and differentiate colour only. "
                                 "Use rasterizer='fastgs'.")
            if world > 1:
                raise ValueError("depth supervision is implemented for one rank (world == 1)")
            if len(depth_weight) != 2 or not (float(depth_weight[0]) > 0 and float(depth_weight[1]) > 0):
                raise ValueError("depth_weight is (initial, final), both > 0: the weight is interpolated in the logarithm")
        self.depth_loss, self.depth_weight = depth_loss, (float(depth_weight[0]), float(depth_weight[1]))
        self._depths = None
        if antialiasing and rasterizer == "gut":
            raise ValueError("antialiasing is not wired into the 3DGUT route (rasterizer='gut'): its fused and autograd steps render without the opacity compensation. "
                             "Use rasterizer='fastgs'.")
        self.antialiasing = bool(antialiasing)
        if filter3d and rasterizer == "gut":
            raise ValueError("filter3d is not wired into the 3DGUT route (rasterizer='gut'): its step forms render the unfiltered scales and opacities. "
                             "Use rasterizer='fastgs'.")
        if absgrad and rasterizer == "gut":
            raise ValueError("absgrad is not wired into the 3DGUT route (rasterizer='gut'): its densification_info comes from the finish pass, the per-pixel absolute "
                             "sums would have to come from the rasterizer backward itself. Use rasterizer='fastgs'.")
        if absgrad and strategy != "default":
            raise ValueError("absgrad changes what ADC reads from densification_info: it needs strategy='default'")
        self.absgrad = bool(absgrad)
        if filter3d and int(filter3d_every) < 1:
            raise ValueError("filter3d_every must be >= 1")
        from .filter3d import Filter3dSchedule
        self.filter3d, self.filter3d_variance = bool(filter3d), float(filter3d_variance)
        self.filter3d_schedule = Filter3dSchedule(int(filter3d_every)) if filter3d else None
        self.filter3d_var = None        # [N] float32: the filter of the model as it stands (None: off)
        self.filter3d_computes = 0      # how many times it was computed (tests, tools)
        self._f3d_cameras = None        # the packed training cameras, built once
        if mask_mode not in ("none", "ignore", "segment"):
            raise ValueError(f"Invalid mask mode: {mask_mode}")
        if mask_mode == "segment":
            if rasterizer == "gut" and fused_l2:
                raise ValueError("mask_mode='segment' is not wired into the fused forms of the 3DGUT rasterizer (rasterizer='gut', fused_l2=True): their backward calls "
                                 "carry no alpha gradient. Use rasterizer='fastgs', or mask_mode='ignore'.")
            if loss != "l1_ssim" and rasterizer == "fastgs":
                raise ValueError("mask_mode='segment' on the fastgs rasterizer needs loss='l1_ssim': the opacity penalty is part of the masked L1 + D-SSIM kernel")
        self.mask_mode, self.mask_alpha_weight = mask_mode, float(mask_alpha_weight)
        self._masks = None
        if pose_optimization not in ("none", "direct", "mlp"):
            raise ValueError(f"Invalid pose optimization type: {pose_optimization}")
        if pose_optimization != "none":
            if rasterizer == "gut":   # trainer.cpp:371-374
                raise ValueError("The 3DGUT rasterizer doesn't have camera gradients yet. Please disable pose optimization or disable gut.")
            if world > 1:
                raise ValueError("pose optimisation is implemented for one rank (world == 1)")
        self.one_call = bool(one_call)
        self.device, self.world, self.rank, self.views_per_rank = device, world, rank, views_per_rank
        sc = scene.to(device)
        self.scene = sc
        mk = lambda t: t.clone().contiguous().requires_grad_(True)
        # Data-parallel layout. Default (round 3): the north-star one - Gaussians REPLICATED, per-rank forward / backward, one all-reduce of the flat gradient
        # bucket before the fused Adam step. sh_sharded=True opts into dist.ShExchange (shN and its Adam state owned by one rank each: 14 instead of 59 floats per
        # Gaussian in the all-reduce; fused 3DGUT step, no strategy or MCMC). bench.py --gpus N times both.
        # factored_sh=True (round 4) keeps the replicated layout and shrinks its collective: the SH gradients are exchanged as dL/dcolour rows (all-gather, 12 B per
        # Gaussian and view) and assembled by every rank itself (dist.ColorGradExchange); only 11 of 59 floats per Gaussian remain in the all-reduce.
        if sh_sharded is None:
            sh_sharded = False
        if factored_sh and (sh_sharded or not (fused_l2 and rasterizer == "gut")):
            raise ValueError("factored_sh is a variant of the replicated layout of the fused 3DGUT step")
        self.factored_sh = bool(factored_sh)
        if self.factored_sh:   # fail at construction, on every rank alike, not in the middle of a run (plan_step has no fallback form for this layout)
            from .capi import load_library
            if not load_library().lfs_gut_step_supported(int(sc.means.shape[0]), int(sc.width), int(sc.height), 16):
                raise ValueError("factored_sh needs a problem shape the C++ step driver takes (lfs_gut_step_supported: <= 512 tile rows, Gaussian index + tile column in 32 bits)")
        self.color_exchange = None
        if sh_sharded and not (fused_l2 and rasterizer == "gut" and strategy in (None, "mcmc")):
            raise ValueError("sh_sharded needs the fused 3DGUT step (no strategy, or MCMC: its refinement steps run on the gathered tensors)")
        self.sh_exchange = lfs_dist.ShExchange(sc.means.shape[0], world, rank) if sh_sharded else None
        shN0 = self.sh_exchange.shard(sc.shN) if sh_sharded else sc.shN
        # scenes built from a point cloud (loader.colmap_scene) carry active_sh_degree = 0: the SH schedule of the reference starts there
        self.model = SplatModel(mk(sc.means), mk(sc.sh0), mk(shN0), mk(sc.raw_scales), mk(sc.raw_quats), mk(sc.raw_opacities), sc.sh_degree,
                                active_sh_degree=sc.extra.get("active_sh_degree"))
        self.rasterizer = rasterizer  # "gut" (3DGUT, the north-star path) | "fastgs" (the reference's default EWA rasterizer)
        self._fg_settings = {}
        self.strategy = None
        self.strategy_kind = strategy
        self._resize_suspended, self._resize_pending = False, False
        self.batch_views = True          # one rank, several views per step: SH forward / backward once over all views (False: view by view, A/B and tests)
        # [2,N] for ADC: (visibility count, screen-space gradient norm) - from the fastgs backward (kernels_backward.cuh:233-236), or, on the 3DGUT route, the
        # screen-equivalent norm from the densifying finish pass of the fused step forms (the reference's --gut leaves it unfilled and never densifies)
        self.densification_info = None
        self._dens_step = None           # the fused 3DGUT step in flight: the tensor its views add to (None: no ADC, or past stop_refine)
        self.scale_reg = self.opacity_reg = 0.0
        if strategy == "default" and rasterizer != "fastgs" and not fused_l2:
            # the statistic is computed by the finish pass of the fused gradient-tensor step forms; torch autograd over the op-by-op mirror (fused_l2=False) has no such
            # pass, and grow / prune would silently never run
            raise ValueError("strategy='default' (ADC) with rasterizer='gut' needs the fused step (fused_l2=True): densification_info comes from its finish pass, "
                             "which the autograd form does not have. Use fused_l2=True or rasterizer='fastgs'.")
        if strategy is not None:
            from . import strategies
            op = opt_params or strategies.OptimizationParameters.for_strategy(strategy, iterations=iterations, **({"absgrad": True} if self.absgrad else {}))
            gen = torch.Generator(device=device).manual_seed(seed)
            cls = {"mcmc": strategies.MCMC, "default": strategies.DefaultStrategy}[strategy]
            self.strategy = cls(self.model, op, scene_scale=scene_scale, generator=gen, on_resize=self._on_resize)
            self.optimizer, self.scheduler = self.strategy.optimizer, self.strategy.scheduler
            if strategy == "mcmc":
                self.scale_reg, self.opacity_reg = op.scale_reg, op.opacity_reg
            lambda_dssim = op.lambda_dssim
        else:
            self.optimizer = FusedAdam(default_param_groups(self.model), fused=fused_adam)
            self.scheduler = ExponentialLR(self.optimizer, gamma=0.01 ** (1.0 / iterations), param_group_index=0)
        self.sh_degree_interval = 1000     # without a strategy the trainer keeps the SH schedule itself (strategies do it in post_backward)
        self.bg = torch.zeros(3, device=device)
        if self.background != (0.0, 0.0, 0.0):   # a constant colour is written here, once; the per-step modes write it before every step (_set_step_background)
            self.bg = torch.tensor(self.background, dtype=torch.float32, device=device)
        # appearance model of BASELINE config 5 (trainer.cpp:66-99: Adam(lr, eps 1e-15) + warm-up exponential schedule), fastgs path only
        self.bilateral, self.tv_loss_weight = None, tv_loss_weight
        if use_bilateral_grid:
            if rasterizer == "gut" and not fused_l2:
                raise ValueError("the bilateral grid is wired into the fused training steps (fastgs, or 3DGUT with fused_l2)")
            from .bilateral_grid import BilateralGrid
            from .fused_adam import WarmupExponentialLR
            gx, gy, gl = bilateral_grid_dims
            self.bilateral = BilateralGrid(sc.viewmats.shape[0], gx, gy, gl, device=device)
            self.bilateral.grids.grad = torch.zeros_like(self.bilateral.grids)
            self.bilateral_optimizer = torch.optim.Adam([self.bilateral.grids], lr=bilateral_grid_lr, eps=1e-15)
            self.bilateral_scheduler = WarmupExponentialLR(self.bilateral_optimizer, gamma=0.01 ** (1.0 / iterations), warmup_steps=1000, warmup_start_factor=0.01)
        # fused_l2: explicit forward/backward through the fused kernels (fused.py) instead of torch autograd over
        # the op-by-op mirror (rasterizer.py); gradients land directly in the flat bucket the all-reduce works on.
        self.fused_l2 = fused_l2
        self.loss_kind, self.lambda_dssim = loss, lambda_dssim  # "mse" | "l1_ssim" (trainer.cpp:115-128)
        self.bucket = lfs_dist.GradBucket(self.model.parameters(), deferred=self._deferred()) if (world > 1 or fused_l2) else None  # 2 = shN
        self.loss_acc = torch.zeros(1, device=device)
        self.inline_all_adam = True   # one view / one rank / MSE: all six parameters are updated inside the backward kernels (fused.backward_adam_all)
        self.fused_tail = True        # ... whose three per-Gaussian tail passes (SH backward + Adam, finish + Adam, next step's SH colours) are ONE launch (lfs_gut_train_step_ex)
        self._next_view = None        #     the view the NEXT step renders, when the trainer knows it (round-robin schedule, or train_step(next_views=...))
        self.cxx_step = True          # ... and that step is ONE C++ call without a host read on the critical path (gut_step.GutStep -> csrc/gut_step.hip);
        self._gut_step = None         #     False: the same kernels enqueued call by call from Python (fused.py; tests compare the two)
        self.inline_shN_adam = True   # see train_step; False keeps the SH backward and the optimizer separate (tests compare the two)
        self.iteration = 0
        self.last_plan: Optional[StepPlan] = None   # the form the last step took (plan_step): tests and tools read it
        self.last_n_isects = 0
        # pose optimisation (trainer.cpp:366-389, :648-649, :763-765): None for "none" - nothing below then differs from a trainer without the argument
        self.pose_module, self.pose_optimizer = None, None
        self.last_grad_w2c = None     # [1,4,4]: the camera gradient of the last view rendered with pose optimisation on (tests and tools read it)
        if pose_optimization != "none":
            from .poseopt import make_pose_module
            self.pose_module = make_pose_module(pose_optimization, int(sc.viewmats.shape[0])).to(device)
            self.pose_optimizer = torch.optim.Adam(self.pose_module.parameters(), lr=pose_lr)
        self._last_radii = None
        self._last_visible = None
        # ADMM sparsity (trainer.cpp:331-360): None when off - nothing below then differs from a trainer without the arguments
        self.base_iterations = self.total_iterations = int(iterations)
        self.sparsity = None
        if enable_sparsity:
            from .sparsity import ADMMSparsityOptimizer, Config as SparsityConfig
            self.sparsity = ADMMSparsityOptimizer(SparsityConfig(sparsify_steps=int(sparsify_steps), init_rho=float(init_rho), prune_ratio=float(prune_ratio),
                                                                 update_every=int(sparsity_update_every), start_iteration=int(iterations)))
            self.total_iterations = int(iterations) + int(sparsify_steps)
            if self.strategy is not None:
                # the strategy's own iteration count stays the base run's (refinement windows, the scheduler's gamma), but its optimizer steps through the phase:
                # the reference's strategies keep the base count for that guard too and train nothing towards z
                self.strategy.step_limit = self.total_iterations
        self._sparsity_added_at = -1

    def _sparsity_applies(self) -> bool:
        """this iteration carries the ADMM term (should_apply_loss)"""
        return self.sparsity is not None and self.sparsity.should_apply_loss(self.iteration)

    def _past_base(self) -> bool:
        """sparsification phase proper: no strategy.post_backward, no SH-degree change (trainer.cpp:745-750: post_backward only while iter <= base)"""
        return self.total_iterations != self.base_iterations and self.iteration > self.base_iterations

    def _add_sparsity_term(self, grad_view=None, loss_acc=None) -> None:
        """The ADMM penalty's gradient into the raw-opacity gradient (default: the flat bucket's segment) and its value into the loss accumulator, 1 / world of both
        per rank: after the backward of the step's last view, before that segment is all-reduced. Once per step - the forms that send the segment early call it
        themselves, the common tail then finds it done."""
        if not self._sparsity_applies() or self._sparsity_added_at == self.iteration:
            return
        self._sparsity_added_at = self.iteration
        with torch.no_grad():
            self.sparsity.add_loss_and_grad(self.model.raw_opacities.detach(), self.bucket.views[5] if grad_view is None else grad_view,
                                            self.loss_acc if loss_acc is None else loss_acc, 1.0 / self.world)

    def _sparsity_after_step(self) -> None:
        """trainer.cpp:776-784, after the optimizer step: the state update on the iterations should_update names, the prune at the last iteration."""
        sp = self.sparsity
        if sp is None:
            return
        if sp.should_update(self.iteration):
            sp.update_state(self.model.raw_opacities.detach())
        if sp.should_prune(self.iteration):
            mask = sp.get_prune_mask(self.model.raw_opacities.detach())
            self._remove_gaussians(mask)
            self.sparsity = None   # (trainer.cpp:240: the optimiser object is dropped after the prune)

    def _contribution_after_step(self) -> None:
        """contribution_prune_at: after the optimizer step of a listed iteration, the statistic over all training views and the RadSplat prune (contribution.py)."""
        if self.iteration not in self.contribution_prune_at:
            return
        from .contribution import compute_contribution, prune_mask
        n_before = int(self.model.means.shape[0])
        cameras = [self.camera(v) for v in range(int(self.scene.viewmats.shape[0]))]
        stats = compute_contribution(self.model, cameras, antialiased=self.antialiasing, filter3d=self.update_filter3d())
        mask = prune_mask(stats, threshold=self.contribution_threshold)
        self._remove_gaussians(mask)
        n_after = int(self.model.means.shape[0])
        if n_after != n_before:   # as after a refinement: the filter belongs to the rows that are left, the visibility words are rebuilt for the new count
            self.update_filter3d(force=True)
            self._vis_bits = None
            if self.densification_info is not None and self.densification_info.shape[1] == n_before:   # ADC's accumulators keep the rows of the Gaussians that stay
                self.densification_info = self.densification_info[:, mask.logical_not()].contiguous()
        self.contribution_log.append((self.iteration, n_before, n_after))
        print(f"[contribution prune] iteration {self.iteration}: N {n_before} -> {n_after} (max blending weight < {self.contribution_threshold:g})")

    @torch.no_grad()
    def _remove_gaussians(self, mask: torch.Tensor) -> None:
        """strategy.remove_gaussians(mask), or the same surgery (strategy_utils.cpp:57-129: index_select on every parameter and both Adam moments) on the trainer's
        own optimizer when there is no strategy. SH-sharded: on the gathered shN, re-sharded for the new count."""
        if self.strategy is not None:
            fn = lambda: self.strategy.remove_gaussians(mask)
        else:
            def fn():
                keep = mask.logical_not().nonzero().squeeze(-1)
                if keep.numel() == mask.numel():
                    return
                for i, name in enumerate(("means", "sh0", "shN", "raw_scales", "raw_quats", "raw_opacities")):
                    old = getattr(self.model, name)
                    new = old.detach().index_select(0, keep).contiguous().requires_grad_(old.requires_grad)
                    self.optimizer.replace_param(i, old, new, lambda t: t.index_select(0, keep))
                    setattr(self.model, name, new)
                self._on_resize()
        if self.sh_exchange is not None:
            self._refine_with_full_shN(fn)
        else:
            fn()

    def _deferred(self):
        """bucket segments that stay out of the flat all-reduce: shN (2) while Adam does not read it; with the factored exchange sh0 (1) and shN always"""
        return [1, 2] if getattr(self, "factored_sh", False) else [2]

    def _on_resize(self) -> None:
        """The strategy replaced parameter tensors (densification): the flat gradient bucket has to follow."""
        if self._resize_suspended:      # (_refine_with_full_shN: shN is gathered right now - one rebuild when the shard is back)
            self._resize_pending = True
            return
        if self.bucket is not None:
            self.bucket = lfs_dist.GradBucket(self.model.parameters(), deferred=self._deferred())

    @property
    def last_visible(self):
        """bool [N]: Gaussians with radii > 0 in the last rendered view"""
        if self._last_radii is not None:
            return (self._last_radii[0] > 0).all(-1)
        return self._last_visible

    def _fastgs_settings(self, view: int):
        from .fastgs import FastGSSettings
        st = self._fg_settings.get(view)
        if st is None:  # intrinsics / camera centre read back once per view, not per step
            sc = self.scene
            K = sc.Ks[view].cpu()
            w2c = sc.viewmats[view]
            cam_pos = (-(w2c[:3, :3].T @ w2c[:3, 3])).contiguous()
            deg = self.model.get_active_sh_degree()
            st = FastGSSettings(cam_pos, (deg + 1) ** 2, sc.width, sc.height, float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), 0.01, 1e10, self.antialiasing)
            self._fg_settings[view] = st
        st.active_sh_bases = (self.model.get_active_sh_degree() + 1) ** 2
        st.depth = "none"   # (_train_step_fastgs switches a view with a depth target to the trainer's depth kind)
        st.filter3d = self.filter3d_var
        st.absgrad = False   # (_train_step_fastgs sets it on the views whose backward feeds densification_info)
        return st

    def update_filter3d(self, force: bool = False):
        """Recompute the 3D smoothing filter when the schedule says so (or force) -> the [N] variances, None with filter3d off. Called at the start of every fastgs
        step; evaluation code calls it to get the filter of the current model."""
        if not self.filter3d:
            return None
        N = self.model.means.shape[0]
        if force or self.filter3d_var is None or self.filter3d_var.shape[0] != N or self.filter3d_schedule.due():
            from .filter3d import compute_filter3d, pack_cameras
            if self._f3d_cameras is None:
                sc = self.scene
                self._f3d_cameras = pack_cameras(viewmats=sc.viewmats, Ks=sc.Ks, width=int(sc.width), height=int(sc.height), device=self.device)
            self.filter3d_var = compute_filter3d(self.model.means, self._f3d_cameras, self.filter3d_variance)
            self.filter3d_schedule.computed()
            self.filter3d_computes += 1
        return self.filter3d_var

    def depth_weight_at(self, iteration: int) -> float:
        """the depth loss weight of (1-based) iteration `iteration`: depth_weight[0] at the first, depth_weight[1] at iteration `iterations` and after, log-linear between"""
        w0, w1 = self.depth_weight
        tt = min(max((iteration - 1) / max(self.base_iterations - 1, 1), 0.0), 1.0)
        return float(math.exp((1.0 - tt) * math.log(w0) + tt * math.log(w1)))

    def _train_step_fastgs(self, targets, views, total_views):
        """The same step through the fastgs (EWA) rasterizer - the reference's default training path (trainer.cpp:656-760): fused
        preprocess -> blend -> [bilateral grid] -> loss ("mse" | "l1_ssim") -> blend backward -> preprocess backward (raw-parameter
        gradients straight into the flat bucket) -> all-reduce -> strategy.post_backward (ADC fed by the rasterizer's
        densification_info, or MCMC) -> fused Adam. The step's background colour (background.py) and RGBA planes go to the compose kernels by value / pointer;
        with the defaults (black, no alphas) nothing of that is launched."""
        from .fastgs import render_and_backward as fg_step
        self.update_filter3d()
        if self.bucket is None:
            self.bucket = lfs_dist.GradBucket(self.model.parameters(), deferred=self._deferred())
        params = self.model.parameters()
        N = params[0].shape[0]
        self.loss_acc.zero_()
        dens = None
        if self.strategy is not None and self.strategy_kind == "default" and self.iteration < self.strategy.params.stop_refine:
            if self.densification_info is None or self.densification_info.shape[1] != N:   # default_strategy.cpp:312-314
                self.densification_info = torch.zeros((2, N), device=self.device)
            dens = self.densification_info
        if len(views) > 1 and (not hasattr(self, "_fg_tmp") or self._fg_tmp[0].shape[0] != N):
            self._fg_tmp = [torch.empty_like(v) for v in self.bucket.views]
        inline = None   # one view on one rank, Adam reading shN: the SH backward inside lfs_fastgs_view_backward (args.adam) updates shN itself
        if (self.inline_shN_adam and self.world == 1 and len(views) == 1 and self.strategy is None and self.iteration > 1000 and self.model.shN.shape[1] > 0
                and getattr(self.optimizer, "fused", False) and self.pose_module is None   # (the optimizer-fused backward has no camera gradient)
                and self._depths is None                                                    # (... and no depth gradient)
                and not self.visible_adam):                                                  # (... and it updates every row of shN)
            inline = self.optimizer.prepare_inline(self.model.shN)
        vis = None
        if self.visible_adam:
            if self._vis_bits is None or self._vis_bits.numel() != (N + 31) // 32:
                self._vis_bits = torch.zeros((N + 31) // 32, dtype=torch.int32, device=self.device)
            vis = self._vis_bits
        for k, v in enumerate(views):
            dst = self.bucket.views if k == 0 else self._fg_tmp
            w2c, w2c_adj, g_w2c = self.scene.viewmats[v:v + 1].contiguous(), None, None
            if self.pose_module is not None:
                # trainer.cpp:648-649: the adjusted transform under autograd; cam_position stays the stored camera's (Camera(const Camera&, transform) copies it)
                w2c_adj = self.pose_module(w2c, [v])
                w2c, g_w2c = w2c_adj.detach().contiguous(), torch.empty_like(w2c)
            st, depth_args = self._fastgs_settings(v), {}
            st.absgrad = self.absgrad and dens is not None
            if self._depths is not None and self._depths[k % len(self._depths)] is not None:
                st.depth = self.depth_loss
                depth_args = {"depth_target": self._depths[k % len(self._depths)], "depth_weight": self.depth_weight_at(self.iteration)}
            _, _, self.last_n_isects = fg_step(st, w2c, self.model, targets[k % len(targets)],
                                               1.0 / total_views, dst, self.loss_acc, densification_info=dens, loss=self.loss_kind,
                                               lambda_dssim=self.lambda_dssim, bilateral=self.bilateral, image_idx=v, adam_shN=inline, grad_w2c=g_w2c,
                                               **self._fastgs_mask_args(k), **depth_args, **self._fastgs_background_args(k),
                                               **({"visibility_bits": vis, "accumulate_visibility": k > 0} if vis is not None else {}))
            if w2c_adj is not None:
                w2c_adj.backward(g_w2c)   # accumulates into the module's parameters over the views of the step
                self.last_grad_w2c = g_w2c
            if k > 0:
                for a, b in zip(self.bucket.views, self._fg_tmp):
                    a.add_(b)
        if self.scale_reg > 0 or self.opacity_reg > 0:   # trainer.cpp:132-158, once per step and 1/world of it per rank
            with torch.no_grad():
                raw_scales, raw_opac = params[3].detach(), params[5].detach()
                if self.scale_reg > 0:
                    self.bucket.views[3].add_(torch.exp(raw_scales), alpha=self.scale_reg / self.world / raw_scales.numel())
                    self.loss_acc += self.scale_reg / self.world * torch.exp(raw_scales).mean()
                if self.opacity_reg > 0:
                    sg = torch.sigmoid(raw_opac)
                    self.bucket.views[5].add_((sg * (1 - sg)).view_as(self.bucket.views[5]), alpha=self.opacity_reg / self.world / raw_opac.numel())
                    self.loss_acc += self.opacity_reg / self.world * sg.mean()
        self._last_radii = None
        self._add_sparsity_term()
        self.bucket.all_reduce(skip_deferred=self.iteration <= 1000)
        for p, gv in zip(params, self.bucket.views):
            p.grad = gv
        self._bilateral_step()
        if self.strategy is not None:
            if self._past_base():
                pass
            elif self.strategy_kind == "default":
                if dens is not None and self.world > 1 and self.strategy.is_refining(self.iteration):
                    lfs_dist.all_reduce_sum(dens)   # replicas must take the same densification decisions
                self.densification_info = self.strategy.post_backward(self.iteration, dens)
            else:
                self.strategy.post_backward(self.iteration)
            # (a refinement has replaced rows since the bits were written: that step stays the dense one; so does none at all past the strategy's step limit)
            if (vis is not None and self.iteration < self.strategy.step_limit and self.model.means.shape[0] == N
                    and (self._past_base() or not self.strategy.is_refining(self.iteration))):
                self.optimizer.set_visibility(vis, N)
            self.strategy.step(self.iteration)
        else:
            if vis is not None:
                self.optimizer.set_visibility(vis, N)
            self.optimizer.step(self.iteration)
            self.scheduler.step()
        if self.pose_optimizer is not None:   # trainer.cpp:763-765: after the model's optimizer step
            self.pose_optimizer.step()
            self.pose_optimizer.zero_grad(set_to_none=True)
        if self.filter3d:
            changed = self.strategy is not None and not self._past_base() and self.strategy.is_refining(self.iteration)
            self.filter3d_schedule.step_done(model_changed=changed or self.model.means.shape[0] != N)
        return self.loss_acc

    def _mask_of(self, k: int):
        """the PreparedMask of the step's k-th view, or None (no masks this step, or that view has none)"""
        return None if self._masks is None else self._masks[k % len(self._masks)]

    def _fastgs_mask_args(self, k: int) -> dict:
        m = self._mask_of(k)
        if m is None:
            return {}
        return {"mask": m, "mask_alpha_weight": self.mask_alpha_weight if self.mask_mode == "segment" else 0.0}

    def _fastgs_background_args(self, k: int) -> dict:
        """the background colour and the RGBA plane of the step's k-th view for fastgs.render_and_backward - {} on a black step without alphas: the parent's call"""
        out = {}
        if self._step_bg is not None:
            out["background"] = self._step_bg
        a = None if self._alphas is None else self._alphas[k % len(self._alphas)]
        if a is not None:
            out["target_alpha"] = a
        return out

    def background_for_step(self, iteration: int):
        """The colour of (1-based) `iteration` -> three Python floats (background.background_for_step with this trainer's base colour, mode and generator). The random
        and the jittered modes DRAW from the generator: train_step calls this once per step."""
        from .background import background_for_step
        return background_for_step(iteration, self.base_iterations, self.background, self.background_mode, self._bg_generator, self.background_jitter)

    def _set_step_background(self) -> None:
        """Before a step: its colour -> last_background, _step_bg (fastgs route: by value) and, on the other routes, self.bg. The copy is stream-ordered from a FRESH
        host tensor: a pinned buffer reused across steps with non_blocking=True would be read when the copy executes, not when it is enqueued - by then the host may
        hold the next step's colour. A constant colour was written at construction: nothing is copied, and with the defaults nothing ever is."""
        if self.background_mode == "constant":
            bg = self.background
        else:
            bg = self.background_for_step(self.iteration + 1)
            if self.rasterizer != "fastgs":
                self.bg.copy_(torch.tensor(bg, dtype=torch.float32))
        self.last_background = bg
        self._step_bg = None if bg == (0.0, 0.0, 0.0) else bg

    def _composite_targets(self, targets, alphas):
        """RGBA targets on the routes other than fastgs: each target with a plane is composited over the step's colour by a target-only call of the compose entry
        before the step form sees it (a new tensor: the resident image is reused every epoch)"""
        from .ops import background_compose
        out = []
        for t, a in zip(targets, alphas):
            out.append(t if a is None else background_compose(self.last_background, target_rgb=t.contiguous(), target_alpha=a)[1])
        return out

    def _bilateral_step(self) -> None:
        """trainer.cpp:699-705, :758-761: TV regulariser (1/world of it per rank), sum of the ranks' grid gradients, Adam + warm-up schedule."""
        if self.bilateral is None:
            return
        if self.tv_loss_weight > 0:
            self.bilateral.tv_loss_fused(self.tv_loss_weight / self.world, self.loss_acc)
        if self.world > 1:
            lfs_dist.all_reduce_sum(self.bilateral.grids.grad)
        self.bilateral_optimizer.step()
        self.bilateral_optimizer.zero_grad(set_to_none=False)
        self.bilateral_scheduler.step()

    def _refine_with_full_shN(self, fn) -> None:
        """SH-sharded + a densification strategy: the strategy's index surgery (relocation, growth, pruning) addresses Gaussians globally, so for a
        refinement step shN and its Adam moments are all-gathered (3 x 180 B / Gaussian, every `refine_every` iterations: < 1 % of the traffic of
        the steps in between), the unchanged replicated strategy code runs - identically on every rank - and the result is re-sharded for the new N."""
        ex, opt = self.sh_exchange, self.optimizer
        old = self.model.shN
        n_before, grad_before = self.model.means.shape[0], old.grad
        self._resize_suspended, self._resize_pending = True, False
        st = opt._state(old)
        m_full, v_full = ex.gather_rows(st["exp_avg"]), ex.gather_rows(st["exp_avg_sq"])
        full = ex.gather_rows(old.detach()).contiguous().requires_grad_(True)
        opt.replace_param(2, old, full, lambda t: m_full if t is st["exp_avg"] else v_full)
        self.model.shN = full
        self.sh_exchange = None
        try:
            fn()
        finally:
            cur = self.model.shN
            st2 = opt._state(cur)
            ex2 = lfs_dist.ShExchange(self.model.means.shape[0], self.world, self.rank)
            ms, vs = ex2.shard(st2["exp_avg"]).clone(), ex2.shard(st2["exp_avg_sq"]).clone()
            shard = ex2.shard(cur.detach()).clone().requires_grad_(True)
            opt.replace_param(2, cur, shard, lambda t: ms if t is st2["exp_avg"] else vs)
            # nothing was added or removed and the strategy kept the tensor (relocation works in place): the shard keeps its gradient, so this
            # step's Adam update of shN happens as it does in the replicated layout and in the reference
            if cur is full and self.model.means.shape[0] == n_before and grad_before is not None:
                shard.grad = grad_before
            self.model.shN = shard
            self.sh_exchange = ex2
            self._resize_suspended = False
            if self._resize_pending or self.model.means.shape[0] != n_before:
                self._on_resize()

    def full_shN(self) -> torch.Tensor:
        """[N,K-1,3] on every rank (all-gathers the owners' rows when SH-sharded): export, evaluation."""
        return self.model.shN.detach() if self.sh_exchange is None else self.sh_exchange.gather_rows(self.model.shN.detach())

    def export_model(self) -> SplatModel:
        """The complete model on this rank (SH-sharded: shN all-gathered; every rank must call it): what loader.save_ply / evaluate.evaluate take."""
        m = self.model
        out = SplatModel(m.means.detach(), m.sh0.detach(), self.full_shN(), m.raw_scales.detach(), m.raw_quats.detach(), m.raw_opacities.detach(), m.max_sh_degree,
                         active_sh_degree=m.active_sh_degree)
        return out

    def camera(self, view: int) -> Camera:
        sc = self.scene
        return Camera(sc.viewmats[view:view + 1].contiguous(), sc.Ks[view:view + 1].contiguous(), sc.width, sc.height)

    def train_step(self, targets: List[torch.Tensor], views: Optional[List[int]] = None, views_all: Optional[List[List[int]]] = None,
                   next_views: Optional[List[int]] = None, masks: Optional[List] = None, depths: Optional[List] = None, alphas: Optional[List] = None) -> float:
        """alphas: a list parallel to `targets` of uint8 [H,W] device planes (the alpha channel of an RGBA target, loader.preload_alphas) or None (that view is opaque):
        the target the loss sees is a * target + (1 - a) * background, a = u8 / 255, over THIS step's colour, black included. fastgs route: composited inside the step
        (fastgs.render_and_backward(target_alpha=)); every other route: by a target-only call of the compose entry before the step form sees the target, so every
        form takes it. A step whose alphas are all None is the step without the argument.
        depths: a list parallel to `targets` of losses.PreparedDepth (at the training resolution; what depth_loss names: inverse depth or depth) or None (that
        view has no depth target); needs depth_loss "invdepth" or "depth". A step whose depths are all None is the step without the argument.
        masks: a list parallel to `targets` of losses.PreparedMask (at the training resolution) or None (that view is unmasked); needs mask_mode "ignore" or
        "segment". A step whose masks are all None is the unmasked step.
        next_views: with an explicit `views`, the views the NEXT call will pass (a data loader knows them: src/training/dataloader.cpp prefetches) - the one-call step's
        fused tail then evaluates their SH colours on the side. Without `views` the round-robin schedule names them."""
        self._next_view = None
        if self.world == 1 and self.views_per_rank == 1:
            if views is None and views_all is None:
                self._next_view = lfs_dist.views_for_step(self.iteration + 1, self.rank, self.world, self.scene.viewmats.shape[0], self.views_per_rank)[0]
            elif next_views:
                self._next_view = int(next_views[0])
        self._masks = None
        if masks is not None and any(m is not None for m in masks):
            if self.mask_mode == "none":
                raise ValueError("train_step(masks=...) needs GutTrainer(mask_mode='ignore' | 'segment') (mask_mode='none')")
            if len(masks) != len(targets):
                raise ValueError("masks must be parallel to targets")
            self._masks = list(masks)
        self._alphas = None
        if alphas is not None and any(a is not None for a in alphas):
            if len(alphas) != len(targets):
                raise ValueError("alphas must be parallel to targets")
            sc = self.scene
            for a in alphas:
                if a is not None and (not torch.is_tensor(a) or a.dtype != torch.uint8 or tuple(a.shape) != (int(sc.height), int(sc.width))):
                    raise ValueError(f"train_step(alphas=...): every plane is a uint8 [{int(sc.height)},{int(sc.width)}] tensor or None (got "
                                     f"{(a.dtype, tuple(a.shape)) if torch.is_tensor(a) else type(a).__name__})")
            self._alphas = [None if a is None else a.contiguous() for a in alphas]
        self._set_step_background()
        if self._alphas is not None and self.rasterizer != "fastgs":
            targets, self._alphas = self._composite_targets(targets, self._alphas), None
        self._depths = None
        if depths is not None and any(d is not None for d in depths):
            if self.depth_loss == "none":
                raise ValueError("train_step(depths=...) needs GutTrainer(depth_loss='invdepth' | 'depth') (depth_loss='none')")
            if len(depths) != len(targets):
                raise ValueError("depths must be parallel to targets")
            self._depths = list(depths)
        try:
            out = self._train_step(targets, views, views_all)
        finally:
            self._masks = None
            self._depths = None
            self._alphas = None
        # the SH schedule, AFTER the backward / optimizer step of the iteration, where the strategies keep it (post_backward: mcmc.cpp:366-368,
        # default_strategy.cpp) - iteration 1000, 2000, ... still renders with the old degree, as the reference does; without a strategy the trainer does it
        if (self.strategy is None and self.iteration % self.sh_degree_interval == 0 and self.model.active_sh_degree < self.model.max_sh_degree
                and not self._past_base()):
            self.model.active_sh_degree += 1
        self._sparsity_after_step()
        self._contribution_after_step()
        return out

    def _train_step(self, targets: List[torch.Tensor], views: Optional[List[int]] = None, views_all: Optional[List[List[int]]] = None) -> float:
        """One optimisation step on this rank's share of the global view batch. `views` overrides this rank's views of the round-robin
        schedule; SH-sharded AND with the factored SH exchange every rank must know every rank's views: pass `views_all` (one list per rank) with an explicit
        schedule (a bare `views` raises there when world > 1).
        WHICH of the step forms runs is decided by plan_step (a pure function of the configuration, table-tested in tests/test_host_logic.py);
        each form is one method below."""
        self.iteration += 1
        if views_all is not None:
            views = views_all[self.rank]
        elif views is not None and self.sh_exchange is not None and self.world > 1:
            raise ValueError("SH-sharded: pass views_all (every rank's views), the SH owners evaluate them")
        elif views is not None and self.factored_sh and self.world > 1:
            # the factored exchange evaluates the SH backward over the views of ALL ranks: with only this rank's views overridden the cameras of the round-robin
            # schedule would be paired with the gathered dL/dcolour rows of other views - sh0 / shN / the direction term of dL/dmeans silently wrong
            raise ValueError("factored SH exchange: pass views_all (every rank's views), each rank evaluates the SH backward over all of them")
        if views is None:
            views = lfs_dist.views_for_step(self.iteration - 1, self.rank, self.world, self.scene.viewmats.shape[0], self.views_per_rank)
        self._views_all = views_all
        total_views = self.world * len(views)
        plan = self.last_plan = self._plan(len(views))   # (kept for tests and tools: which form the step took)
        if self._masks is not None and plan.path in ("batch_views", "py_views"):
            raise ValueError(f"masked training is not wired into the {plan.path} step form (rasterizer={self.rasterizer!r}, world={self.world}, views per step="
                             f"{len(views)}, sh_sharded={self.sh_exchange is not None}, cxx_step={self.cxx_step}): masks run in the fastgs, autograd, cxx_views and "
                             "cxx_factored forms")
        if self._depths is not None and plan.path != "fastgs":
            raise ValueError(f"depth supervision is not wired into the {plan.path} step form: it runs in the fastgs form only")
        if plan.path != "cxx_all" and self._gut_step is not None:
            self._gut_step.colors_for = None   # (another step form is about to change the parameters: colours a fused tail left for this step are void)
        if plan.path == "fastgs":
            return self._train_step_fastgs(targets, views, total_views)
        if plan.path == "autograd":
            return self._step_autograd(targets, views, total_views)
        if not plan.inline_all:
            self.loss_acc.zero_()   # (the all-inline step stores the loss: no fill launch)
        self._dens_step = self._densification_target()
        if self._dens_step is not None and (plan.path == "cxx_all" or plan.inline_all or plan.inline_shard):
            raise ValueError(f"ADC on the 3DGUT route needs a gradient-tensor step form, plan_step chose {plan.path}")   # (plan_step keeps strategy='default' out of them)
        if plan.path == "cxx_all":
            self._step_cxx_all(plan, targets, views, total_views)
        elif plan.path == "cxx_views":
            self._step_cxx_views(plan, targets, views, total_views)
        elif plan.path == "cxx_factored":
            self._step_cxx_factored(plan, targets, views, total_views)
        elif plan.path == "batch_views":
            self._step_batch_views(plan, targets, views, total_views)
        else:
            self._step_py_views(plan, targets, views, total_views)
        return self._finish_fused_step(plan)

    def _densification_target(self) -> Optional[torch.Tensor]:
        """ADC on the 3DGUT route: the [2,N] tensor this step's views add their statistic to, (re-)allocated zeroed at the current N as _train_step_fastgs does
        (default_strategy.cpp:312-314); None without ADC and from stop_refine on."""
        if self.strategy is None or self.strategy_kind != "default" or self._past_base() or self.iteration >= self.strategy.params.stop_refine:
            return None
        N = self.model.means.shape[0]
        if self.densification_info is None or self.densification_info.shape[1] != N:
            self.densification_info = torch.zeros((2, N), device=self.device)
        return self.densification_info

    def _cxx_supported(self) -> bool:
        """Shapes the speculative C++ step does not take (more than 512 tile rows, the index-bit limit, debug bit 5: csrc/intersect.hip would return
        LFS_E_UNSUPPORTED) run the same kernels enqueued call by call from Python (the py_views form) instead of failing."""
        from .capi import load_library
        sc = self.scene
        return bool(load_library().lfs_gut_step_supported(int(self.model.means.shape[0]), int(sc.width), int(sc.height), 16))

    def _plan(self, n_views: int) -> "StepPlan":
        st = self.strategy
        return plan_step(rasterizer=self.rasterizer, fused_l2=self.fused_l2, world=self.world, force_collectives=bool(lfs_dist._FORCE),
                         sh_sharded=self.sh_exchange is not None, shard_rows=(self.sh_exchange.n if self.sh_exchange is not None else 0), n_views=n_views,
                         loss=self.loss_kind, strategy=(None if st is None else self.strategy_kind), refining=bool(st is not None and st.is_refining(self.iteration)),
                         iteration=self.iteration, has_shN=self.model.shN.shape[1] > 0, optimizer_fused=bool(getattr(self.optimizer, "fused", False)),
                         # (the ADMM term needs the opacity gradient as a tensor: no all-inline and no one-call form while it applies)
                         bilateral=self.bilateral is not None, inline_shN_adam=self.inline_shN_adam, inline_all_adam=self.inline_all_adam and not self._sparsity_applies(),
                         cxx_step=self.cxx_step and self.rasterizer != "fastgs" and self.fused_l2 and self._cxx_supported(), batch_views=self.batch_views,
                         factored_sh=self.factored_sh, masked=self._masks is not None,
                         # (a strategy stops updating at its last iteration, strategies._StrategyBase.step: those steps keep the split form; so does a model with
                         #  SH degree 4 - K = 25 > 16: the fused tail, which carries the freeze and the noise, has no instantiation for it)
                         one_call=(self.one_call and (st is None or self.iteration < st.params.iterations) and 1 + self.model.shN.shape[1] <= 16
                                   and not self._sparsity_applies()))

    def _gut(self):
        from .gut_step import GutStep
        if self._gut_step is None:
            self._gut_step = GutStep(self.device)
        return self._gut_step

    def _step_cxx_all(self, plan, targets, views, total_views) -> None:
        """One view, one rank, MSE, iteration > 1000: forward + backward + Adam on all six tensors as ONE C++ call (csrc/gut_step.hip), no gradient tensors.
        With one_call=True also L1 + D-SSIM, MCMC between refinements (the step's noise is drawn HERE, from the strategy's generator, where post_backward would have
        drawn it) and iteration <= 1000 (plan.freeze_shN: no inline state for shN - FusedAdam.step counts the skipped step itself, as in the split form)."""
        names = ("means", "sh0", "raw_scales", "raw_quats", "raw_opacities") if plan.freeze_shN else ("shN", "means", "sh0", "raw_scales", "raw_quats", "raw_opacities")
        inline_all = {name: self.optimizer.prepare_inline(getattr(self.model, name)) for name in names}
        gs, sc, v = self._gut(), self.scene, views[0]
        N = self.model.means.shape[0]
        extra = {}
        if self.one_call:
            extra = dict(loss=self.loss_kind, lambda_dssim=self.lambda_dssim, freeze_shN=plan.freeze_shN)
            if self.strategy is not None:
                extra["noise"], extra["noise_lr"] = self.strategy.draw_noise()
        opt_form = bool(extra) and (self.loss_kind != "mse" or plan.freeze_shN or "noise" in extra)   # lfs_gut_train_step_opt: always the fused-tail form
        self.last_n_isects = gs.train_step([p.detach() for p in self.model.parameters()], inline_all, self.model.get_active_sh_degree(), sc.width, sc.height,
                                           sc.viewmats[v], sc.Ks[v], self.bg, targets[0], 1.0 / total_views, self.loss_acc, self.scale_reg, self.opacity_reg,
                                           fused_tail=self.fused_tail or opt_form,
                                           next_viewmat=None if self._next_view is None else sc.viewmats[self._next_view], **extra)
        self._last_radii = gs.view("radii", torch.int32, (1, N, 2))

    @property
    def pipelined(self) -> bool:
        """Always False: the two-stream form of the one-call step was measured, rejected and removed (benchmark drivers still assign and read the attribute)."""
        return False

    @pipelined.setter
    def pipelined(self, value) -> None:
        if value:
            raise ValueError("the two-stream (pipelined) training step was removed: measured -4.5 % at best and slower on most variants "
                             "(profiles/r06/pipeline/README.md); the last commit that contains it is 13aac0e")

    def _view_loss(self, gs, view: int, target, weight: float, mask=None):
        """The loss of the view gs.view_forward() left in the step workspace -> (v_render, fold): dL/d(render) [H,W,3] from the loss kernels (bilateral grid, L1 + D-SSIM)
        with fold None, or v_render None and fold = the target the rasterizer backward derives the clamped MSE from itself. The loss is added to loss_acc.
        With a mask it is always the loss-kernel route (the masked kernels), never the folded MSE."""
        sc = self.scene
        if mask is not None:
            from .losses import loss_fwd_bwd
            render = gs.view("render", torch.float32, (sc.height, sc.width, 3))
            if self.bilateral is not None:
                shown = self.bilateral.apply_fused(render, view, chw=False)
                v_shown = loss_fwd_bwd(self.loss_kind, shown, target, weight, self.loss_acc, chw=False, clamp=False, lambda_dssim=self.lambda_dssim, mask=mask)
                return self.bilateral.apply_fused_backward(render, view, v_shown, chw=False), None
            return loss_fwd_bwd(self.loss_kind, render, target, weight, self.loss_acc, chw=False, clamp=True, lambda_dssim=self.lambda_dssim, mask=mask), None
        if self.bilateral is not None:   # clamp -> slice -> loss on the un-clamped result -> slice backward (fused.render_and_backward does the same)
            from .losses import loss_fwd_bwd
            render = gs.view("render", torch.float32, (sc.height, sc.width, 3))
            shown = self.bilateral.apply_fused(render, view, chw=False)
            v_shown = loss_fwd_bwd(self.loss_kind, shown, target, weight, self.loss_acc, chw=False, clamp=False, lambda_dssim=self.lambda_dssim)
            return self.bilateral.apply_fused_backward(render, view, v_shown, chw=False), None
        if self.loss_kind == "l1_ssim":
            from .losses import photometric_loss_fwd_bwd
            return photometric_loss_fwd_bwd(gs.view("render", torch.float32, (1, sc.height, sc.width, 3)), target, self.lambda_dssim, weight, self.loss_acc), None
        return None, target

    def _step_cxx_views(self, plan, targets, views, total_views) -> None:
        """Gradient-tensor form of the C++ step (data-parallel ranks with the north-star layout - replicated Gaussians, one all-reduce of the flat bucket -,
        single-rank steps while iteration <= 1000, and every step whose loss is not the folded MSE: L1 + D-SSIM, bilateral grid, MCMC): per view one speculative
        forward + two backward calls; the host looks at the forward's (pinned) counts once per view, after it has enqueued the forward. The loss kernels run
        between forward and backward on the image the forward left in the step workspace. The SH backward runs BEFORE the finish pass, so on the last view of a
        rank the shN segment (45 of 59 floats per Gaussian at degree 3) is on the wire, in 4 chunks, while the finish kernel still runs; the remaining 14 floats
        follow in all_reduce(). One view on one rank with Adam reading shN (plan.inline_shN): the SH backward applies shN's update itself."""
        inline = self.optimizer.prepare_inline(self.model.shN) if plan.inline_shN else None
        gs, sc = self._gut(), self.scene
        ps = [p.detach() for p in self.model.parameters()]
        deg, N = self.model.get_active_sh_degree(), self.model.means.shape[0]
        weight = 1.0 / total_views
        for k, v in enumerate(views):
            vm, Km, tgt = sc.viewmats[v], sc.Ks[v], targets[k % len(targets)]
            self.last_n_isects = gs.view_forward(ps, deg, sc.width, sc.height, vm, Km, self.bg)
            v_render, fold = self._view_loss(gs, v, tgt, weight, self._mask_of(k))
            gs.view_backward_sh(ps, deg, sc.width, sc.height, vm, Km, self.bg, self.bucket.views, k > 0, target_chw=fold, weight=weight,
                                loss_acc=self.loss_acc, v_render=v_render, adam_shN=inline)
            if plan.multi and k == len(views) - 1 and self.iteration > 1000 and ps[2].numel():
                self.bucket.all_reduce_early([2], chunks=4)
            gs.view_backward_finish(ps, deg, sc.width, sc.height, vm, Km, self.bg, self.bucket.views, k > 0, target_chw=fold, weight=weight,
                                    loss_acc=self.loss_acc, scale_reg=self.scale_reg / self.world if k == 0 else 0.0,
                                    opacity_reg=self.opacity_reg / self.world if k == 0 else 0.0, densification_info=self._dens_step)
        self._last_radii = gs.view("radii", torch.int32, (1, N, 2))

    def _step_cxx_factored(self, plan, targets, views, total_views) -> None:
        """Replicated layout, factored SH exchange. Per view of this rank: speculative forward, loss, rasterizer backward + finish (means / scales / quaternions /
        opacities gradients into the bucket, dL/dcolour rows - clamp-masked - into the send buffer). Then: the rows of all ranks are all-gathered, the all-reduce of
        the 11 remaining floats per Gaussian starts behind them (asynchronously, on RCCL's stream), and the multi-view SH backward runs over the views of ALL ranks in
        rank-major order: sh0's gradient -> bucket, shN's Adam update inside (or its gradient -> bucket on refining iterations, or nothing while iteration <= 1000),
        the direction term of the means gradient -> added after the all-reduce has landed. Every rank executes the same sums in the same order."""
        from . import fused
        gs, sc = self._gut(), self.scene
        ps = [p.detach() for p in self.model.parameters()]
        deg, N = self.model.get_active_sh_degree(), self.model.means.shape[0]
        ex = self.color_exchange
        if ex is None or ex.n != N or ex.vpr != len(views):
            ex = self.color_exchange = lfs_dist.ColorGradExchange(N, self.world, self.rank, len(views), self.device)
        weight = 1.0 / total_views
        for k, v in enumerate(views):
            vm, Km, tgt = sc.viewmats[v], sc.Ks[v], targets[k % len(targets)]
            self.last_n_isects = gs.view_forward(ps, deg, sc.width, sc.height, vm, Km, self.bg)
            v_render, fold = self._view_loss(gs, v, tgt, weight, self._mask_of(k))
            gs.view_backward_rows(ps, deg, sc.width, sc.height, vm, Km, self.bg, self.bucket.views, k > 0, ex.send[k], target_chw=fold, weight=weight,
                                  loss_acc=self.loss_acc, v_render=v_render, scale_reg=self.scale_reg / self.world if k == 0 else 0.0,
                                  opacity_reg=self.opacity_reg / self.world if k == 0 else 0.0, densification_info=self._dens_step)
        self._last_radii = gs.view("radii", torch.int32, (1, N, 2))
        # Round 6: the all-gather goes FIRST. Collectives of one communicator execute in issue order on RCCL's stream; the multi-view SH backward below waits for the
        # gathered rows and for nothing else, the 11-float all-reduce is only needed by the optimizer afterwards - issued second it travels UNDER the SH backward
        # (rounds 4 - 5 issued it first: the rows, and with them the SH backward, started one all-reduce later).
        rows = ex.gather()                                            # [world * views, N, 3], rank-major
        self._add_sparsity_term()                                     # (the opacity segment leaves with the early all-reduce)
        self.bucket.all_reduce_early([0, 3, 4, 5], chunks=1)          # 11 floats per Gaussian, on RCCL's stream while the SH backward runs
        every = self._views_all or [lfs_dist.views_for_step(self.iteration - 1, j, self.world, sc.viewmats.shape[0], len(views)) for j in range(self.world)]
        if rows.shape[0] != len(every) * len(views):                  # (one GPU forced through the collectives: the gathered rows are this rank's own)
            every = [list(views)]
        vms = torch.stack([sc.viewmats[v] for e in every for v in e]).contiguous()
        adam = self.optimizer.prepare_inline(self.model.shN) if plan.inline_shN else None
        want_shN_grad = adam is None and self.iteration > 1000 and self.model.shN.shape[1] > 0     # a refining iteration: relocation first, then the optimizer
        ex.v_dirs.zero_()
        fused.sh_model_bwd_views(deg, ps[0], vms, ps[1], ps[2], None, None, rows, self.bucket.views[1], self.bucket.views[2] if want_shN_grad else None, ex.v_dirs,
                                 False, adam=adam)
        self._pending_v_dirs = ex.v_dirs

    def _step_batch_views(self, plan, targets, views, total_views) -> None:
        """Several views per step on one rank: the SH stages run ONCE over all views (fused.render_views_and_backward), and shN's Adam update moves into
        that one SH backward when the optimizer would read the gradient anyway."""
        from .fused import render_views_and_backward
        inline_v = self.optimizer.prepare_inline(self.model.shN) if plan.inline_shN else None
        outs = render_views_and_backward([self.camera(v) for v in views], self.model, self.bg, [targets[k % len(targets)] for k in range(len(views))],
                                         1.0 / total_views, self.bucket.views, self.loss_acc, loss=self.loss_kind, lambda_dssim=self.lambda_dssim,
                                         scale_reg=self.scale_reg, opacity_reg=self.opacity_reg, adam_shN=inline_v, bilateral=self.bilateral,
                                         image_idxs=list(views), densification_info=self._dens_step)
        self.last_n_isects, self._last_radii = outs[-1].n_isects, outs[-1].radii

    def _step_py_views(self, plan, targets, views, total_views) -> None:
        """The fused kernels enqueued call by call from Python (fused.render_and_backward), view by view: the SH-sharded layout, cxx_step = False (the tests hold
        the C++ step to this path bit for bit), and the fallback of the C++ step."""
        from .fused import render_and_backward
        inline = self.optimizer.prepare_inline(self.model.shN) if (plan.inline_shN and not plan.inline_all) else None
        inline_shard = self.optimizer.prepare_inline(self.model.shN) if plan.inline_shard else None
        inline_all = None
        if plan.inline_all:
            inline_all = {name: self.optimizer.prepare_inline(getattr(self.model, name)) for name in ("shN", "means", "sh0", "raw_scales", "raw_quats", "raw_opacities")}
        every = None
        if self.sh_exchange is not None:  # what every rank renders at sub-step k (the owners evaluate SH for all of them)
            every = self._views_all or [lfs_dist.views_for_step(self.iteration - 1, j, self.world, self.scene.viewmats.shape[0], len(views)) for j in range(self.world)]
        # ADC, several views on one rank: the SH direction terms of dL/dmeans are summed apart from the rasterizer parts and added once, as the batched form adds them -
        # the two single-rank forms then take the same refinement decisions from bit-equal parameters (tests/test_gpu_gut_densify.py)
        dirs = None
        if self._dens_step is not None and len(views) > 1 and self.sh_exchange is None and self.world == 1:
            dirs = torch.zeros_like(self.bucket.views[0])
        for k, v in enumerate(views):
            vm_all = None if every is None else [self.scene.viewmats[e[k]:e[k] + 1].contiguous() for e in every]
            out = render_and_backward(self.camera(v), self.model, self.bg, targets[k % len(targets)], 1.0 / total_views,
                                      self.bucket.views, self.loss_acc, accumulate=k > 0, loss=self.loss_kind, lambda_dssim=self.lambda_dssim,
                                      # regularisers: once per step, and 1/world of them per rank (the all-reduce sums the ranks)
                                      scale_reg=self.scale_reg / self.world if k == 0 else 0.0,
                                      opacity_reg=self.opacity_reg / self.world if k == 0 else 0.0,
                                      sh_exchange=self.sh_exchange, viewmats_all=vm_all, adam_shN=inline, adam_shard=inline_shard, adam_all=inline_all,
                                      bilateral=self.bilateral, image_idx=v, densification_info=self._dens_step, v_dirs_acc=dirs,
                                      # last view: scales / quats / opacities gradients are final before the SH backward starts - their all-reduce overlaps with it
                                      # (the ADMM term goes into the opacity gradient before it leaves)
                                      on_geometry_grads=(lambda: (self._add_sparsity_term(), self.bucket.all_reduce_early([3, 4, 5]))) if (self.world > 1 and k == len(views) - 1) else None)
            self.last_n_isects, self._last_radii = out.n_isects, out.radii
        if dirs is not None:
            self.bucket.views[0].add_(dirs)

    def _finish_fused_step(self, plan):
        """What follows the backward of every fused step form: all-reduce of the flat bucket, the bilateral grid's own optimizer, strategy / optimizer step."""
        params = self.model.parameters()
        self._add_sparsity_term()
        # the deferred segment (shN) stays out of the all-reduce while Adam does not read it (iteration <= 1000) and, SH-sharded, always
        self.bucket.all_reduce(skip_deferred=plan.skip_deferred)
        if plan.path == "cxx_factored":   # the SH direction term of dL/dmeans, summed over every rank's views by the multi-view SH backward: identical on all ranks
            self.bucket.views[0].add_(self._pending_v_dirs)
        self._bilateral_step()
        for p, gv in zip(params, self.bucket.views):
            p.grad = gv
        if self.strategy is not None:  # trainer.cpp:741-760: post_backward (may replace the parameter tensors) then step
            if self._past_base():      # (trainer.cpp:745-750: none of it during the sparsification phase)
                pass
            elif plan.path == "cxx_all":   # (one_call: the noise went into the tail - what is left of post_backward is the SH schedule)
                self.strategy.post_backward_schedule(self.iteration)
            elif self.strategy_kind == "default":   # ADC fed by the finish pass's statistic, as _train_step_fastgs feeds it from the fastgs backward
                dens, self._dens_step = self._dens_step, None
                if dens is not None and plan.multi and self.strategy.is_refining(self.iteration):
                    lfs_dist.all_reduce_sum(dens)   # replicas must take the same densification decisions
                self.densification_info = self.strategy.post_backward(self.iteration, dens)
            elif self.sh_exchange is not None and self.strategy.is_refining(self.iteration):
                self._refine_with_full_shN(lambda: self.strategy.post_backward(self.iteration))
            else:
                self.strategy.post_backward(self.iteration)
            self.strategy.step(self.iteration)  # FusedAdam skips tensors without a gradient, as the reference's does after add_new_gs
        else:
            self.optimizer.step(self.iteration)
            self.scheduler.step()
        return self.loss_acc  # this rank's share of the loss (a 1-element tensor, read it after a sync)

    def _step_autograd(self, targets, views, total_views):
        """torch autograd over the op-by-op mirror of gs::training::rasterize (rasterizer.py): the reference's own structure, kept as the comparison path."""
        loss_value = None
        for k, v in enumerate(views):
            out = rasterize(self.camera(v), self.model, self.bg, 1.0, False, False, RenderMode.RGB)
            mask = self._mask_of(k)
            if mask is not None:
                tgt = targets[k % len(targets)]
                if self.loss_kind == "l1_ssim":
                    from .losses import masked_photometric_loss
                    loss = masked_photometric_loss(out.image, tgt, mask, self.lambda_dssim) / total_views
                else:
                    m, s_img = mask.mask_u8.to(out.image.dtype), mask.sums[0].to(out.image.dtype)
                    loss = torch.where(s_img > 0, (m * (out.image - tgt) ** 2).sum() / (3.0 * s_img.clamp_min(1.0)), out.image.new_zeros(())) / total_views
                if self.mask_mode == "segment":
                    loss = loss + self.mask_alpha_weight / total_views * ((255.0 - mask.mask_u8.to(out.alpha.dtype)) * out.alpha.reshape(mask.mask_u8.shape)).sum() / (
                        255.0 * mask.mask_u8.numel())
            elif self.loss_kind == "l1_ssim":
                from .losses import photometric_loss
                loss = photometric_loss(out.image, targets[k % len(targets)], self.lambda_dssim) / total_views
            else:
                loss = torch.nn.functional.mse_loss(out.image, targets[k % len(targets)]) / total_views
            if k == 0 and self.scale_reg > 0:
                loss = loss + self.scale_reg / self.world * self.model.get_scaling().mean()
            if k == 0 and self.opacity_reg > 0:
                loss = loss + self.opacity_reg / self.world * self.model.get_opacity().mean()
            loss.backward()
            loss_value = loss.detach()
            self.last_n_isects, self._last_visible = out.n_isects, out.visibility
        if self._sparsity_applies():   # where the reference's sparsity loss.backward() accumulates: p.grad, before the all-reduce
            self._add_sparsity_term(self.model.raw_opacities.grad, loss_value)
        if self.bucket is not None:
            params = self.model.parameters()
            self.bucket.gather([p.grad for p in params])
            self.bucket.all_reduce(skip_deferred=self.iteration <= 1000)
            for p, gv in zip(params, self.bucket.views):
                p.grad = gv
        if self.strategy is not None:
            if not self._past_base():
                self.strategy.post_backward(self.iteration)
            self.strategy.step(self.iteration)
            return loss_value
        self.optimizer.step(self.iteration)
        self.optimizer.zero_grad(set_to_none=True)
        self.scheduler.step()
        return loss_value
