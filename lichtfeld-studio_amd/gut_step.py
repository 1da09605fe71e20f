"""Host side of csrc/gut_step.hip: the --gut training step as ONE C call - lfs_gut_train_step (three tail passes), lfs_gut_train_step_opt (the fused tail, with the
photometric loss, the MCMC noise and the shN freeze as options; lfs_gut_train_step_ex is the same call without options) - and its split form for gradient tensors:
lfs_gut_view_forward, then lfs_gut_view_backward, its two halves
lfs_gut_view_backward_sh / _finish, or lfs_gut_view_backward_rows for the factored exchange. Mirrors what Trainer::train_step does around rasterize() on the --gut path
(/root/reference/src/training/trainer.cpp:579-770, rasterization/rasterizer.cpp:200-344) - minus the host synchronisation of
gsplat/Intersect.cpp:75-76: the intersection lists live in a workspace sized for a CAPACITY, the count stays on the device, and this class
looks at the (pinned) counts only after the whole step has been enqueued. An attempt that did not fit (count above capacity, or a tile list longer
than the sort classes launched) updated nothing - the kernels check a device flag - and is simply run again with a larger workspace.

torch is the allocator here (one uint8 tensor per workspace, one pinned int64[3] for the counts) and owns the stream; nothing else.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import torch

from .capi import LfsError, check, load_library, stream

GROUPS = ("means", "sh0", "shN", "raw_scales", "raw_quats", "raw_opacities")   # FusedAdam group order (strategy_utils.cpp:35-40)


class StepArgs(C.Structure):  # lfs_gut_step_args
    _fields_ = [("N", C.c_uint32), ("K", C.c_uint32), ("sh_degree", C.c_uint32), ("image_width", C.c_uint32), ("image_height", C.c_uint32), ("tile_size", C.c_uint32),
                ("means", C.c_void_p), ("sh0", C.c_void_p), ("shN", C.c_void_p), ("raw_scales", C.c_void_p), ("raw_quats", C.c_void_p), ("raw_opacities", C.c_void_p),
                ("exp_avg", C.c_void_p * 6), ("exp_avg_sq", C.c_void_p * 6), ("adam", (C.c_float * 6) * 6),
                ("viewmat", C.c_void_p), ("Kmat", C.c_void_p), ("background", C.c_void_p), ("target_chw", C.c_void_p),
                ("loss_weight", C.c_float), ("scale_reg", C.c_float), ("opacity_reg", C.c_float), ("loss", C.c_void_p)]


class StepLayout(C.Structure):  # lfs_gut_step_layout
    _fields_ = [(k, C.c_size_t) for k in ("bytes", "render", "alpha", "last_ids", "radii", "means2d", "depths", "colors", "quats", "scales", "opacities",
                                          "tile_offsets", "flatten_ids", "isect_ids", "counts", "abort_flag")]


class StepOptions(C.Structure):  # lfs_gut_step_options
    _fields_ = [("loss_kind", C.c_uint32), ("lambda_dssim", C.c_float), ("freeze_shN", C.c_uint32), ("noise", C.c_void_p), ("noise_lr", C.c_float),
                ("loss_workspace", C.c_void_p), ("loss_workspace_bytes", C.c_size_t)]


class ViewExt(C.Structure):  # lfs_gut_view_ext
    _fields_ = [("densification_info", C.c_void_p)]


LOSS_KINDS = {"mse": 0, "l1_ssim": 1}


class GutStep:
    """One workspace + the capacity bookkeeping for steps of one (N, W, H, tile) shape on one device."""

    def __init__(self, device, tile: int = 16, initial_capacity: Optional[int] = None, margin: float = 1.25):
        self.device = torch.device(device)
        self.tile = tile
        self.margin = margin
        self.capacity = int(initial_capacity) if initial_capacity else 0
        self.assumed_longest = 1024
        self.ws: Optional[torch.Tensor] = None
        self.layout: Optional[StepLayout] = None
        self.shape = None
        self.counts = torch.zeros(3, dtype=torch.int64).pin_memory()
        self._stamp = 0
        self.n_isects = 0
        self.longest = 0
        self.wait_poll_s = 5.0    # how long _wait spins on the pinned counts before it falls back to a stream synchronisation
        self.retries = 0          # attempts that did not fit (each one is re-run): a few right after start-up or a densification, none in steady state
        self.colors_for = None    # fused tail (lfs_gut_train_step_opt): what the workspace's SH colours were evaluated for by the previous step - (viewmat pointer and version, N, K,
                                  # degree, workspace pointer, pointers and versions of means / sh0 / shN) - or None; a step for exactly that skips its SH colour kernel
        self.colour_launches_saved = 0
        self.loss_ws: Optional[torch.Tensor] = None   # lfs_gut_train_step_opt, loss "l1_ssim": the SSIM derivative maps + dL/d(render) (lfs_gut_step_loss_workspace_bytes)

    # ---- workspace --------------------------------------------------------------------------------------------------------------------------
    def _ensure(self, N: int, W: int, H: int) -> None:
        lib = load_library()
        if self.capacity <= 0:
            self.capacity = max(4 * N, 1 << 16)       # first guess: ~4 tile entries per Gaussian (SYN-B: 4.4); the first step corrects it
        shape = (N, W, H, self.capacity, int(lib.lfs_get_debug_flags()))   # (debug bit 4, the deterministic backward, adds a 64-bit accumulator to the workspace)
        if self.shape == shape and self.ws is not None:
            return
        lay = StepLayout()
        check(lib.lfs_gut_step_layout_for(C.c_uint32(N), C.c_uint32(W), C.c_uint32(H), C.c_uint32(self.tile), C.c_int64(self.capacity), C.byref(lay)), "gut_step_layout_for")
        if self.ws is None or self.ws.numel() < lay.bytes:
            self.ws = None                            # (release the old block before the larger one is requested)
            self.ws = torch.empty(int(lay.bytes), dtype=torch.uint8, device=self.device)
        self.layout, self.shape = lay, shape

    def _grow(self, n_isects: int, longest: int) -> None:
        self.capacity = max(int(n_isects * self.margin) + 1024, self.capacity)
        self.assumed_longest = max(int(longest * self.margin), self.assumed_longest)
        self.shape = None

    def view(self, name: str, dtype, shape: Sequence[int]) -> torch.Tensor:
        """A tensor view of one workspace region (render [H,W,3] f32, alpha [H,W] f32, radii [N,2] i32, ...): valid until the next step."""
        off = getattr(self.layout, name)
        n = 1
        for d in shape:
            n *= int(d)
        nbytes = n * torch.empty((), dtype=dtype).element_size()
        return self.ws[off:off + nbytes].view(dtype).view(*shape)

    # ---- argument block -----------------------------------------------------------------------------------------------------------------------
    def _args(self, params: Sequence[torch.Tensor], sh_degree: int, W: int, H: int, viewmat: torch.Tensor, Kmat: torch.Tensor, bg: Optional[torch.Tensor],
              target_chw: Optional[torch.Tensor], weight: float, scale_reg: float, opacity_reg: float, loss_acc: Optional[torch.Tensor],
              adam: Optional[Dict[str, dict]]) -> StepArgs:
        means, sh0, shN, raw_scales, raw_quats, raw_opac = params
        for t in (*params, viewmat, Kmat, bg, target_chw, loss_acc):
            if t is not None and (not t.is_cuda or not t.is_contiguous() or t.dtype != torch.float32):
                raise LfsError("gut_step: every tensor must be a contiguous float32 CUDA (HIP) tensor")
        a = StepArgs()
        a.N, a.K, a.sh_degree = means.shape[0], 1 + shN.shape[1], sh_degree
        a.image_width, a.image_height, a.tile_size = W, H, self.tile
        a.means, a.sh0, a.shN = means.data_ptr(), sh0.data_ptr(), (shN.data_ptr() if shN.numel() else None)
        a.raw_scales, a.raw_quats, a.raw_opacities = raw_scales.data_ptr(), raw_quats.data_ptr(), raw_opac.data_ptr()
        if adam is not None:
            for k, name in enumerate(GROUPS):
                d = adam.get(name)
                if d is None:   # (view_backward_sh takes shN's state alone)
                    continue
                a.exp_avg[k], a.exp_avg_sq[k] = d["exp_avg"].data_ptr(), d["exp_avg_sq"].data_ptr()
                for j, key in enumerate(("lr", "beta1", "beta2", "eps", "bc1_rcp", "bc2_sqrt_rcp")):
                    a.adam[k][j] = d[key]
        a.viewmat, a.Kmat = viewmat.data_ptr(), Kmat.data_ptr()
        a.background = bg.data_ptr() if bg is not None else None
        a.target_chw = target_chw.data_ptr() if target_chw is not None else None
        a.loss_weight, a.scale_reg, a.opacity_reg = weight, scale_reg, opacity_reg
        a.loss = loss_acc.data_ptr() if loss_acc is not None else None
        return a

    def _wait(self) -> bool:
        """-> did the attempt fit? (the counts were written by the scan kernel long before the host got here)"""
        lib = load_library()
        n, lg = C.c_int64(0), C.c_int64(0)
        # the stamp usually is there already; when the step sits behind other work on the stream (the previous step's all-reduce, a first-collective RCCL
        # initialisation that can take longer than any fixed timeout) the host simply waits for the stream and looks again - it only gives up when the stream
        # has DRAINED and the stamp of this step is still missing
        rc = lib.lfs_gut_step_wait(C.c_void_p(self.counts.data_ptr()), C.c_int64(self._stamp), C.c_double(self.wait_poll_s), C.byref(n), C.byref(lg))
        if rc != 0:
            torch.cuda.current_stream(self.device).synchronize()
            rc = lib.lfs_gut_step_wait(C.c_void_p(self.counts.data_ptr()), C.c_int64(self._stamp), C.c_double(1.0), C.byref(n), C.byref(lg))
        if rc != 0:
            raise LfsError("gut_step: the stream has drained and the intersection counts of this step never arrived in pinned host memory")
        self.n_isects, self.longest = int(n.value), int(lg.value)
        return bool(lib.lfs_gut_step_fits(n, lg, C.c_int64(self.capacity), C.c_int64(self.assumed_longest)))

    def _after_fit(self) -> None:
        # stay ahead of a slowly growing scene: enlarge BEFORE the next step would overflow (a re-run costs a whole step, a reallocation nothing)
        if self.n_isects > 0.92 * self.capacity or self.longest > 0.92 * self._class_limit():
            self._grow(self.n_isects, self.longest)

    def _class_limit(self) -> int:
        a = self.assumed_longest
        return 1024 if a <= 1024 else 4096 if a <= 4096 else 16384 if a <= 16384 else 1 << 62

    # ---- the step -------------------------------------------------------------------------------------------------------------------------------
    def _ws_args(self):
        """the trailing arguments of every speculative entry point: capacity, assumed_longest, workspace, workspace_bytes, host_counts, stamp, stream"""
        return (C.c_int64(self.capacity), C.c_int64(self.assumed_longest), C.c_void_p(self.ws.data_ptr()), C.c_size_t(self.ws.numel()),
                C.c_void_p(self.counts.data_ptr()), C.c_int64(self._stamp), stream())

    def _attempt(self, N: int, W: int, H: int, args, enqueue, what: str, after_fit: bool = True) -> int:
        """The one attempt loop of train_step (all forms) and view_forward: workspace -> argument block (args()) -> stamp -> enqueue(a) -> counts. An attempt that fitted
        returns n_isects; one that did not applied nothing and is run again with a larger workspace. enqueue may return a callable(fitted) for book-keeping of its own
        between the look at the counts and the growth of the workspace."""
        for attempt in range(4):
            self._ensure(N, W, H)
            a = args()
            self._stamp += 1
            settle = enqueue(a)
            fitted = self._wait()
            if settle is not None:
                settle(fitted)
            if fitted:
                if after_fit:
                    self._after_fit()
                return self.n_isects
            self.retries += 1
            self._grow(self.n_isects, self.longest)
        raise LfsError(f"gut_step: the {what} did not fit its workspace after 4 attempts")

    def train_step(self, params: Sequence[torch.Tensor], adam: Dict[str, dict], sh_degree: int, W: int, H: int, viewmat: torch.Tensor, Kmat: torch.Tensor,
                   bg: Optional[torch.Tensor], target_chw: torch.Tensor, weight: float, loss_acc: torch.Tensor, scale_reg: float = 0.0,
                   opacity_reg: float = 0.0, fused_tail: bool = False, next_viewmat: Optional[torch.Tensor] = None,
                   loss: str = "mse", lambda_dssim: float = 0.2, freeze_shN: bool = False, noise: Optional[torch.Tensor] = None, noise_lr: float = 0.0) -> int:
        """Forward + backward + Adam on all six parameter tensors, in place; *loss_acc = weight * mse. `adam[name]` = FusedAdam.prepare_inline(param) for
        the six names of GROUPS. Returns n_isects. Default: lfs_gut_train_step (three tail passes).
        fused_tail: lfs_gut_train_step_opt - SH backward, the six Adam updates and (next_viewmat: the view the NEXT step renders, a tensor that stays untouched until then)
        the next step's SH colours in one launch; a following step for exactly that view (same tensor, same N / K / degree / workspace) skips its SH colour kernel.
        loss "l1_ssim" (with lambda_dssim), freeze_shN (iteration <= 1000: FusedAdam skips shN - `adam` then needs no "shN" entry) and noise [N,3] + noise_lr (the MCMC
        strategy's draw and lr * noise_lr, added to the means in front of their Adam update as lfs_add_noise would) are that call's options: the fused-tail form for
        what the reference trains. An attempt that did not fit applied nothing, the noise included: the re-run takes the same noise tensor."""
        lib = load_library()
        N = params[0].shape[0]
        K = 1 + params[2].shape[1]
        opts = None
        if loss != "mse" or freeze_shN or noise is not None:
            if not fused_tail:
                raise LfsError("gut_step: loss / freeze_shN / noise need the fused-tail form (fused_tail=True)")
            if loss not in LOSS_KINDS:
                raise LfsError(f"gut_step: unknown loss {loss!r}")
            opts = StepOptions()
            opts.loss_kind, opts.lambda_dssim, opts.freeze_shN = LOSS_KINDS[loss], float(lambda_dssim), int(bool(freeze_shN))
            if noise is not None:
                if not noise.is_cuda or not noise.is_contiguous() or noise.dtype != torch.float32 or noise.numel() != 3 * N:
                    raise LfsError("gut_step: noise must be a contiguous float32 CUDA (HIP) tensor [N,3]")
                opts.noise, opts.noise_lr = noise.data_ptr(), float(noise_lr)
            if opts.loss_kind == 1:
                need = int(lib.lfs_gut_step_loss_workspace_bytes(C.c_uint32(W), C.c_uint32(H)))
                if self.loss_ws is None or self.loss_ws.numel() < need:
                    self.loss_ws = None
                    self.loss_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
                opts.loss_workspace, opts.loss_workspace_bytes = self.loss_ws.data_ptr(), self.loss_ws.numel()
        if fused_tail:
            # (replaced parameter tensors void the colours too - and so does an in-place write to the view matrix, means, sh0 or shN between the two steps: their
            #  autograd version counters, which a detach() or an index view shares with its base, as the C++ GutTrainStep compares them. The step's own updates go
            #  through raw pointers and leave the counters alone: the fast path stays.)
            key = lambda vm: (vm.data_ptr(), vm._version, N, K, sh_degree, self.ws.data_ptr(), params[0].data_ptr(), params[1].data_ptr(), params[2].data_ptr(),
                              params[0]._version, params[1]._version, params[2]._version)
            nxt = next_viewmat if (next_viewmat is not None and K <= 16) else None

            def enqueue(a):
                ready = self.colors_for is not None and self.colors_for == key(viewmat)
                self.colors_for = None   # (whatever happens below, the colours of THIS view are consumed / overwritten)
                check(lib.lfs_gut_train_step_opt(C.byref(a), C.byref(opts) if opts is not None else None, C.c_void_p(nxt.data_ptr()) if nxt is not None else None,
                                                 C.c_int(int(ready)), *self._ws_args()), "gut_train_step_opt")

                def settle(fitted):
                    if fitted:
                        if nxt is not None:
                            self.colors_for = key(nxt)
                        self.colour_launches_saved += int(ready)
                    elif ready:   # the tail returned without writing anything, so colours that were ready still are - unless _grow replaces the workspace
                        self.colors_for = key(viewmat)
                return settle
        else:
            def enqueue(a):
                self.colors_for = None
                check(lib.lfs_gut_train_step(C.byref(a), *self._ws_args()), "gut_train_step")
        return self._attempt(N, W, H, lambda: self._args(params, sh_degree, W, H, viewmat, Kmat, bg, target_chw, weight, scale_reg, opacity_reg, loss_acc, adam),
                             enqueue, "step")

    def view_forward(self, params: Sequence[torch.Tensor], sh_degree: int, W: int, H: int, viewmat, Kmat, bg) -> int:
        """Forward of one view into the workspace (render / alpha / radii via .view()); re-run on overflow. Returns n_isects."""
        lib = load_library()
        self.colors_for = None   # (this forward evaluates its own colours into the workspace)
        return self._attempt(params[0].shape[0], W, H, lambda: self._args(params, sh_degree, W, H, viewmat, Kmat, bg, None, 0.0, 0.0, 0.0, None, None),
                             lambda a: check(lib.lfs_gut_view_forward(C.byref(a), *self._ws_args()), "gut_view_forward"), "view", after_fit=False)

    def _backward_call(self, fn_name: str, params, sh_degree, W, H, viewmat, Kmat, bg, grads, accumulate, target_chw, weight, loss_acc, v_render, scale_reg, opacity_reg,
                       adam=None, rows_out=None, densification_info=None):
        """densification_info [2,N] (ADC's statistic, added to by the view's finish pass): the call goes to the entry's _ex form; None: the entry itself."""
        lib = load_library()
        a = self._args(params, sh_degree, W, H, viewmat, Kmat, bg, target_chw, weight, scale_reg, opacity_reg, loss_acc, adam)
        for g in grads:
            if not g.is_cuda or not g.is_contiguous():
                raise LfsError("gut_step: gradient tensors must be contiguous CUDA (HIP) tensors")
        gp = (C.c_void_p * 6)(*[g.data_ptr() if g.numel() else None for g in grads])
        ws, nb = C.c_void_p(self.ws.data_ptr()), C.c_size_t(self.ws.numel())
        ext = ()
        if densification_info is not None:
            d = densification_info
            if not d.is_cuda or not d.is_contiguous() or d.dtype != torch.float32 or tuple(d.shape) != (2, params[0].shape[0]):
                raise LfsError("gut_step: densification_info must be a contiguous float32 CUDA (HIP) tensor [2,N]")
            e = ViewExt()
            e.densification_info = d.data_ptr()
            ext, fn_name = (C.byref(e),), fn_name + "_ex"
        if fn_name.startswith("lfs_gut_view_backward_finish"):
            check(getattr(lib, fn_name)(C.byref(a), C.c_int64(self.capacity), gp, C.c_int(int(accumulate)), *ext, ws, nb, stream()), fn_name)
            return
        if v_render is not None:
            v_render = v_render.contiguous()
        rows = () if rows_out is None else (C.c_void_p(rows_out.data_ptr()),)   # (lfs_gut_view_backward_rows: dL/dcolour [N,3], in front of the workspace)
        check(getattr(lib, fn_name)(C.byref(a), C.c_int64(self.capacity), C.c_void_p(v_render.data_ptr()) if v_render is not None else None, gp,
                                    C.c_int(int(accumulate)), *rows, *ext, ws, nb, stream()), fn_name)

    def view_backward(self, params: Sequence[torch.Tensor], sh_degree: int, W: int, H: int, viewmat, Kmat, bg, grads: List[torch.Tensor], accumulate: bool, *,
                      target_chw: Optional[torch.Tensor] = None, weight: float = 0.0, loss_acc: Optional[torch.Tensor] = None,
                      v_render: Optional[torch.Tensor] = None, scale_reg: float = 0.0, opacity_reg: float = 0.0,
                      densification_info: Optional[torch.Tensor] = None) -> None:
        """Backward of the view view_forward() left in the workspace, into the six gradient tensors (group order): written, or added to with `accumulate`.
        With target_chw the clamped MSE (weight) is folded into the backward and loss_acc += it; otherwise v_render [H,W,3] is dL/d(render).
        densification_info [2,N] (ADC, strategies.DefaultStrategy): for every Gaussian visible in this view row 0 += 1 and row 1 += the screen-equivalent norm of
        the view's own rasterizer part of dL/dmeans - by the finish pass, whatever `accumulate` is."""
        self._backward_call("lfs_gut_view_backward", params, sh_degree, W, H, viewmat, Kmat, bg, grads, accumulate, target_chw, weight, loss_acc, v_render,
                            scale_reg, opacity_reg, densification_info=densification_info)

    def view_backward_sh(self, params, sh_degree, W, H, viewmat, Kmat, bg, grads, accumulate, *, target_chw=None, weight=0.0, loss_acc=None, v_render=None,
                         adam_shN: Optional[dict] = None) -> None:
        """First half of view_backward: rasterizer backward + SH backward. grads[1] (sh0) and grads[2] (shN) are final for this view when it has run.
        adam_shN (FusedAdam.prepare_inline(shN); one view per step): shN is updated in place by the SH backward instead and grads[2] is left alone."""
        self._backward_call("lfs_gut_view_backward_sh", params, sh_degree, W, H, viewmat, Kmat, bg, grads, accumulate, target_chw, weight, loss_acc, v_render, 0.0, 0.0,
                            adam=None if adam_shN is None else {"shN": adam_shN})

    def view_backward_rows(self, params, sh_degree, W, H, viewmat, Kmat, bg, grads, accumulate, rows_out: torch.Tensor, *, target_chw=None, weight=0.0, loss_acc=None,
                           v_render=None, scale_reg: float = 0.0, opacity_reg: float = 0.0, densification_info: Optional[torch.Tensor] = None) -> None:
        """The view's backward for the factored gradient exchange (dist.ColorGradExchange): grads[0] (means, without the SH direction term), grads[3..5] written / added
        to, dL/dcolour -> rows_out [N,3], masked with the clamp of the SH colours (colour > 0) - what the multi-view SH backward of every rank takes as it is.
        densification_info: as view_backward."""
        if not rows_out.is_cuda or not rows_out.is_contiguous() or rows_out.numel() != 3 * params[0].shape[0]:
            raise LfsError("gut_step: rows_out must be a contiguous CUDA (HIP) tensor [N,3]")
        self._backward_call("lfs_gut_view_backward_rows", params, sh_degree, W, H, viewmat, Kmat, bg, grads, accumulate, target_chw, weight, loss_acc, v_render,
                            scale_reg, opacity_reg, rows_out=rows_out, densification_info=densification_info)
        N = params[0].shape[0]
        rows_out.view(N, 3).mul_(self.view("colors", torch.float32, (N, 3)) > 0)   # clamp_min backward of rasterizer.cpp:262 (colours of invisible Gaussians: rows are 0 anyway)

    def view_backward_finish(self, params, sh_degree, W, H, viewmat, Kmat, bg, grads, accumulate, *, target_chw=None, weight=0.0, loss_acc=None,
                             scale_reg: float = 0.0, opacity_reg: float = 0.0, densification_info: Optional[torch.Tensor] = None) -> None:
        """Second half: accumulator rows + dL/d(dirs) -> grads[0], grads[3..5]; loss_acc += the fused MSE of the first half (when target_chw was given).
        densification_info: as view_backward (the SH direction term this half adds to grads[0] does not enter it)."""
        self._backward_call("lfs_gut_view_backward_finish", params, sh_degree, W, H, viewmat, Kmat, bg, grads, accumulate, target_chw, weight, loss_acc, None,
                            scale_reg, opacity_reg, densification_info=densification_info)
