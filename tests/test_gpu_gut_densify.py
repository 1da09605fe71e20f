"""GPU: ADC's densification statistic on the 3DGUT route - raster_finish_densify_kernel behind the _ex entries of the gradient-tensor backwards.

For one view and Gaussian i, with v = the rasterizer's part of dL/dmean_i of THAT view (what the old lfs_gut_view_backward_rows writes to grads[0]):
    g_c = R v,  z = (R (mu_i - origin)).z,  s_i = sqrt((g_c.x z W / (2 fx))^2 + (g_c.y z H / (2 fy))^2)      (R = the view matrix's rotation = Rinv^T)
    visible_i = radii[i,0] > 0 and radii[i,1] > 0;  densification_info[0,i] += visible_i,  densification_info[1,i] += visible_i ? s_i : 0
The bound of the value test is derived, not measured: two three-term dot products (5 roundings each), their product, the precomputed scale (2 roundings) and its
product, a square, a sum and a square root are fewer than 16 float32 roundings of quantities bounded by |v| |mu - origin| max(W / (2 fx), H / (2 fy)); the factor 32
carries 2 x slack. The same bodies run on the wavefront emulator (tests/test_emulated_gut_densify.py)."""
import contextlib
import ctypes as C
import dataclasses
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ["means", "sh0", "shN", "raw_scales", "raw_quats", "raw_opacities"]


@contextlib.contextmanager
def _deterministic(lfs):
    lib = lfs.load_library()
    try:
        lib.lfs_set_debug_flags(16)
        yield lib
    finally:
        lib.lfs_set_debug_flags(0)


def _second_view():
    """a view that is not the identity (syn_a's own is): rotated about y and x, moved sideways - a transposed Rinv or a world-space depth would show"""
    a, b = 0.35, -0.2
    Ry = torch.tensor([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    Rx = torch.tensor([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
    vm = torch.eye(4)
    vm[:3, :3] = Rx @ Ry
    vm[:3, 3] = torch.tensor([1.2, -0.4, 0.8])
    return vm.to(DEV).contiguous()


class _Case:
    """syn_a with n Gaussians at SH degree 2, one GutStep, an explicit dL/d(render) of scale 1e-3"""

    def __init__(self, n, seed=11):
        from lichtfeld_studio_amd import scenes
        from lichtfeld_studio_amd.gut_step import GutStep
        sc = self.sc = scenes.syn_a(n=n, sh_degree=2)
        self.N, self.W, self.H, self.deg = n, sc.width, sc.height, 2
        self.params = [t.to(DEV).contiguous() for t in (sc.means, sc.sh0, sc.shN, sc.raw_scales, sc.raw_quats, sc.raw_opacities)]
        self.views = [sc.viewmats[0].to(DEV).contiguous(), _second_view()]
        self.K = sc.Ks[0].to(DEV).contiguous()
        self.bg = torch.zeros(3, device=DEV)
        self.v_render = (torch.randn(self.H, self.W, 3, generator=torch.Generator().manual_seed(seed)) * 1e-3).to(DEV)
        self.gs = GutStep(DEV)

    def grads(self):
        return [torch.zeros_like(p) for p in self.params]

    def forward(self, view=0):
        self.gs.view_forward(self.params, self.deg, self.W, self.H, self.views[view], self.K, self.bg)
        return self.gs.view("radii", torch.int32, (self.N, 2)).clone()

    def rows(self, view=0, grads=None, accumulate=False, dens=None):
        """forward + lfs_gut_view_backward_rows[_ex] -> (grads, rows [N,3], radii)"""
        grads = self.grads() if grads is None else grads
        rows = torch.zeros(self.N, 3, device=DEV)
        radii = self.forward(view)
        kw = {} if dens is None else {"densification_info": dens}
        self.gs.view_backward_rows(self.params, self.deg, self.W, self.H, self.views[view], self.K, self.bg, grads, accumulate, rows, v_render=self.v_render, **kw)
        return grads, rows, radii

    def dens_of_rows(self, view=0):
        dens = torch.zeros(2, self.N, device=DEV)
        self.rows(view, dens=dens)
        return dens


def _model(case, v, view, radii):
    """float64 -> (visible, s, bound) per Gaussian"""
    vm, K = case.views[view].double(), case.K.double()
    R, t = vm[:3, :3], vm[:3, 3]
    origin = -(R.T @ t)
    d = case.params[0].double() - origin
    g_c, z = v.double() @ R.T, (d @ R.T)[:, 2]
    sx, sy = case.W / (2 * K[0, 0]), case.H / (2 * K[1, 1])
    s = torch.sqrt((g_c[:, 0] * z * sx) ** 2 + (g_c[:, 1] * z * sy) ** 2)
    bound = 32 * 2.0 ** -24 * v.double().norm(dim=-1) * d.norm(dim=-1) * max(float(sx), float(sy))
    return (radii > 0).all(-1), s, bound


# ---- 1. values ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,view", [(1, 0), (63, 0), (65, 0), (257, 0), (257, 1), (6000, 0), (6000, 1)])
def test_statistic_matches_the_float64_formula_and_the_gradients_keep_their_bits(lfs, n, view):
    """N = 1 / 63 / 65 / 257 / 6000: the tail-lane clamp (tail lanes hold the last row's operands and must not add twice), more than one wavefront, more than one
    workgroup; on syn_a's own (identity) view and on a rotated, shifted one."""
    with _deterministic(lfs):
        case = _Case(n)
        g_old, rows_old, radii = case.rows(view)                      # the OLD entry: grads[0] = v by its contract (written, no SH direction term)
        dens = torch.zeros(2, n, device=DEV)
        g_new, rows_new, radii_new = case.rows(view, dens=dens)
        torch.cuda.synchronize()
    assert torch.equal(radii, radii_new) and torch.equal(rows_old, rows_new)
    for name, a, b in zip(NAMES, g_old, g_new):
        assert torch.equal(a, b), name
    visible, s, bound = _model(case, g_old[0], view, radii)
    err = (dens[1].double() - torch.where(visible, s, torch.zeros_like(s))).abs()
    print(f"N {n} view {view}: visible {int(visible.sum())}, max s {float(s[visible].max()) if visible.any() else 0.0:.3e}, max err / bound "
          f"{float((err / bound.clamp_min(1e-300))[visible].max()) if visible.any() else 0.0:.3f}")
    if n >= 63:
        assert bool(visible.any()) and float(s[visible].max()) > 0
    assert torch.equal(dens[0], visible.to(dens.dtype))
    assert bool((err <= bound).all()), float((err - bound).max())
    assert bool((dens[:, ~visible] == 0).all())


def test_statistic_is_positive_somewhere_on_the_single_gaussian_scene(lfs):
    """N = 1 of the value test may or may not be on screen; one Gaussian placed in front of the camera is, and is counted once."""
    with _deterministic(lfs):
        case = _Case(1)
        case.params[0].copy_(torch.tensor([[0.1, -0.1, 4.0]]))
        dens = case.dens_of_rows(0)
        torch.cuda.synchronize()
    assert float(dens[0, 0]) == 1.0 and float(dens[1, 0]) > 0


# ---- 2. per view under accumulation ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 6000])
def test_accumulating_call_adds_the_views_own_statistic(lfs, n):
    """Two views into the same gradient tensors (accumulate on the second) and the same densification_info: float32(dens_view0) + float32(dens_view1), bit for bit -
    the statistic comes from the view's own v, not from the bucket the gradient is added into."""
    with _deterministic(lfs):
        case = _Case(n)
        d0, d1 = case.dens_of_rows(0), case.dens_of_rows(1)
        dens = torch.zeros(2, n, device=DEV)
        grads, _, _ = case.rows(0, dens=dens)
        case.rows(1, grads=grads, accumulate=True, dens=dens)
        torch.cuda.synchronize()
    assert float(d0[1].max()) > 0 and float(d1[1].max()) > 0 and not torch.equal(d0, d1)
    assert torch.equal(dens, d0 + d1)


# ---- 3. combined entry, and its two halves --------------------------------------------------------------------------------------------------------------------------
def test_combined_entry_and_its_halves_give_the_bits_of_the_rows_entry(lfs, n=6000):   # (n: the emulated run takes a smaller scene)
    """lfs_gut_view_backward_ex and lfs_gut_view_backward_sh + lfs_gut_view_backward_finish_ex run the SH backward first and hand dL/d(dirs) to the finish pass: the
    statistic is the rows entry's, so the SH direction term does not enter it."""
    with _deterministic(lfs):
        case = _Case(n)
        gs, a = case.gs, (case.params, case.deg, case.W, case.H, case.views[1], case.K, case.bg)
        want = case.dens_of_rows(1)
        g_rows, _, _ = case.rows(1)
        d_comb, g_comb = torch.zeros(2, case.N, device=DEV), case.grads()
        case.forward(1)
        gs.view_backward(*a, g_comb, False, v_render=case.v_render, densification_info=d_comb)
        d_half, g_half = torch.zeros(2, case.N, device=DEV), case.grads()
        case.forward(1)
        gs.view_backward_sh(*a, g_half, False, v_render=case.v_render)
        gs.view_backward_finish(*a, g_half, False, densification_info=d_half)
        g_plain = case.grads()
        case.forward(1)
        gs.view_backward(*a, g_plain, False, v_render=case.v_render)
        torch.cuda.synchronize()
    assert float(want[1].max()) > 0
    assert torch.equal(d_comb, want) and torch.equal(d_half, want)
    assert not torch.equal(g_comb[0], g_rows[0]), "the SH direction term is in the combined entry's dL/dmeans"
    for name, x, y, z in zip(NAMES, g_comb, g_half, g_plain):
        assert torch.equal(x, z) and torch.equal(y, z), name


# ---- 4. operator-level entry ------------------------------------------------------------------------------------------------------------------------------------------
def test_operator_route_gives_the_same_bits_and_refuses_without_the_fused_finish(lfs, n=6000):   # (n: the emulated run takes a smaller scene)
    from lichtfeld_studio_amd import fused, scenes
    from lichtfeld_studio_amd.capi import stream
    from lichtfeld_studio_amd.gut_step import GutStep, ViewExt
    from lichtfeld_studio_amd.trainer import GutTrainer
    sc = scenes.syn_a(n=n, sh_degree=2)
    tr = GutTrainer(sc, DEV, iterations=100)
    target = torch.rand(3, sc.height, sc.width, generator=torch.Generator().manual_seed(6)).to(DEV) * 0.7
    params = [p.detach() for p in tr.model.parameters()]
    N, W, H, deg = params[0].shape[0], sc.width, sc.height, tr.model.get_active_sh_degree()
    vm, Km = tr.scene.viewmats[0], tr.scene.Ks[0]
    with _deterministic(lfs) as lib:
        g_op, l_op, d_op = [torch.zeros_like(p) for p in params], torch.zeros(1, device=DEV), torch.zeros(2, N, device=DEV)
        fused.render_and_backward(tr.camera(0), tr.model, tr.bg, target, 0.5, g_op, l_op, accumulate=False, densification_info=d_op)   # lfs_gut_finish_grads_ex
        g_ref, l_ref = [torch.zeros_like(p) for p in params], torch.zeros(1, device=DEV)
        fused.render_and_backward(tr.camera(0), tr.model, tr.bg, target, 0.5, g_ref, l_ref, accumulate=False)
        gs = GutStep(DEV)
        g_cx, l_cx, d_cx = [torch.zeros_like(p) for p in params], torch.zeros(1, device=DEV), torch.zeros(2, N, device=DEV)
        gs.view_forward(params, deg, W, H, vm, Km, tr.bg)
        gs.view_backward(params, deg, W, H, vm, Km, tr.bg, g_cx, False, target_chw=target, weight=0.5, loss_acc=l_cx, densification_info=d_cx)
        torch.cuda.synchronize()
        assert float(d_op[0].sum()) > 0 and float(d_op[1].max()) > 0
        assert torch.equal(d_op, d_cx)
        for name, x, y, z in zip(NAMES, g_op, g_ref, g_cx):
            assert torch.equal(x, y) and torch.equal(x, z), name
        # the three-kernel A/B form has no such pass
        try:
            fused.FUSE_FINISH_GRADS = False
            with pytest.raises(ValueError, match="FUSE_FINISH_GRADS"):
                fused.render_and_backward(tr.camera(0), tr.model, tr.bg, target, 0.5, g_op, l_op, accumulate=False, densification_info=d_op)
        finally:
            fused.FUSE_FINISH_GRADS = True
        # ext NULL, and ext with a NULL pointer: the _ex entry is the old entry
        v_render = (torch.randn(H, W, 3, generator=torch.Generator().manual_seed(7)) * 1e-3).to(DEV)
        g_old, rows_old = [torch.zeros_like(p) for p in params], torch.zeros(N, 3, device=DEV)
        gs.view_forward(params, deg, W, H, vm, Km, tr.bg)
        gs.view_backward_rows(params, deg, W, H, vm, Km, tr.bg, g_old, False, rows_old, v_render=v_render)
        mask = gs.view("colors", torch.float32, (N, 3)) > 0      # (GutStep.view_backward_rows applies the clamp mask to the rows the C entry wrote)
        for ext in (None, C.byref(ViewExt())):
            g_ex, rows_ex = [torch.zeros_like(p) for p in params], torch.zeros(N, 3, device=DEV)
            gs.view_forward(params, deg, W, H, vm, Km, tr.bg)
            a = gs._args(params, deg, W, H, vm, Km, tr.bg, None, 0.0, 0.0, 0.0, None, None)
            gp = (C.c_void_p * 6)(*[g.data_ptr() if g.numel() else None for g in g_ex])
            rc = lib.lfs_gut_view_backward_rows_ex(C.byref(a), C.c_int64(gs.capacity), C.c_void_p(v_render.data_ptr()), gp, C.c_int(0), C.c_void_p(rows_ex.data_ptr()), ext,
                                                   C.c_void_p(gs.ws.data_ptr()), C.c_size_t(gs.ws.numel()), stream())
            torch.cuda.synchronize()
            assert rc == 0
            assert torch.equal(rows_ex * mask, rows_old)
            for name, x, y in zip(NAMES, g_ex, g_old):
                assert torch.equal(x, y), name
        # densification_info without radii: LFS_E_INVALID before any launch (nothing is written)
        ext = ViewExt()
        ext.densification_info = d_cx.data_ptr()
        before = d_cx.clone()
        p = lambda t: C.c_void_p(t.data_ptr())
        quats, scales, opac = (gs.view(k, torch.float32, s) for k, s in (("quats", (N, 4)), ("scales", (N, 3)), ("opacities", (N,))))
        rc = lib.lfs_gut_finish_grads_ex(C.c_uint32(N), p(params[0]), p(params[4]), p(quats), p(scales), p(opac), C.c_float(0.0), C.c_float(0.0), C.c_int(0), p(g_ex[0]), p(g_ex[3]),
                                         p(g_ex[4]), p(g_ex[5]), p(rows_ex), None, None, C.byref(ext), C.c_void_p(gs.ws.data_ptr()), C.c_size_t(gs.ws.numel()), stream())
        torch.cuda.synchronize()
        assert rc == -1 and torch.equal(d_cx, before)


# ---- 5. trainer -------------------------------------------------------------------------------------------------------------------------------------------------------
def _adc_params(**kw):
    from lichtfeld_studio_amd import strategies
    # Refinements at iterations 10, 20 and 30 (start_refine 5, refine_every 10); reset_every 50 keeps the opacity reset, which throws the loss back on purpose, out of
    # the 40 steps. grad_threshold: this scene starts far from its target - at iteration 9, 91 % of the visible Gaussians are above the default 2e-4 on EITHER rasterizer
    # (3DGUT 1368 of 1458, fastgs 1372 of 1457; median 1.1e-3 / 1.2e-3, 90th percentile 3.8e-3 / 4.0e-3) - and a clone is not render-preserving (two Gaussians of the
    # same opacity in one place), so a refinement that clones nearly everything costs more loss (+0.035 on both routes) than ten steps win back. 4e-3 is the scene's
    # 90th percentile: about a tenth of the Gaussians grows per refinement, as on a real scene.
    return strategies.OptimizationParameters.for_strategy("default", **dict(dict(iterations=300, start_refine=5, refine_every=10, stop_refine=200, reset_every=50,
                                                                                 sh_degree_interval=1000, grad_threshold=4e-3), **kw))


def _adc_scene(n_views=1):
    """syn_a with 1500 Gaussians to start from, and per view the image of the same scene with 6000 (more Gaussians than the start)"""
    from lichtfeld_studio_amd import scenes
    from lichtfeld_studio_amd.rasterizer import rasterize
    from lichtfeld_studio_amd.trainer import GutTrainer
    sc, full = scenes.syn_a(n=1500, sh_degree=1), scenes.syn_a(n=6000, sh_degree=1)
    if n_views > 1:
        vms = torch.stack([sc.viewmats[0]] + [_second_view().cpu()] * (n_views - 1))
        sc = dataclasses.replace(sc, viewmats=vms, Ks=sc.Ks[:1].repeat(n_views, 1, 1))
        full = dataclasses.replace(full, viewmats=vms, Ks=sc.Ks)
    src = GutTrainer(full, DEV, iterations=100)
    with torch.no_grad():
        targets = [rasterize(src.camera(v), src.model, src.bg).image.detach().clone() for v in range(n_views)]
    return sc, targets


def _adc_trainer(sc, **kw):
    from lichtfeld_studio_amd.trainer import GutTrainer
    return GutTrainer(sc, DEV, iterations=300, rasterizer="gut", strategy="default", loss="l1_ssim", opt_params=_adc_params(), **kw)


def test_trainer_runs_adc_on_the_3dgut_route(lfs):
    with _deterministic(lfs):
        sc, targets = _adc_scene()
        a, b = _adc_trainer(sc), _adc_trainer(sc)
        b.cxx_step = False                                   # the same kernels enqueued from Python (py_views)
        n0, counts, losses = a.model.means.shape[0], [], []
        for it in range(1, 41):
            la, _ = a.train_step(targets, views=[0]), b.train_step(targets, views=[0])
            losses.append(float(la))
            counts.append(a.model.means.shape[0])
            assert a.last_plan.path == "cxx_views" and b.last_plan.path == "py_views", (a.last_plan, b.last_plan)
            if it == 9:
                d9 = a.densification_info.clone()
            if it in (10, 20):                               # a refinement: grown, and the statistic re-zeroed at the new N
                assert a.model.means.shape[0] > counts[-2], (it, counts)
                assert tuple(a.densification_info.shape) == (2, a.model.means.shape[0]) and float(a.densification_info.abs().sum()) == 0
        torch.cuda.synchronize()
    print(f"Gaussians {n0} -> {counts[9]} -> {counts[19]} -> {counts[-1]}; loss before the first refinement {losses[8]:.5f}, at the end {losses[-1]:.5f}")
    assert float(d9[0].max()) == 9 and float(d9[1].max()) > 0 and tuple(d9.shape) == (2, n0)
    assert counts[8] == n0 and losses[-1] < losses[8]
    assert b.model.means.shape[0] == a.model.means.shape[0]
    for name, p, q in zip(NAMES, a.model.parameters(), b.model.parameters()):
        assert torch.equal(p, q), name
    assert torch.equal(a.densification_info, b.densification_info)


def _two_view_twins(lfs):
    with _deterministic(lfs):
        sc, targets = _adc_scene(n_views=2)
        a, b = _adc_trainer(sc, views_per_rank=2), _adc_trainer(sc, views_per_rank=2)
        b.batch_views = False
        for it in range(1, 13):
            a.train_step(targets, views=[0, 1]), b.train_step(targets, views=[0, 1])
            if it == 1:
                d1 = a.densification_info.clone(), b.densification_info.clone()
            if it == 9:
                d9 = a.densification_info.clone(), b.densification_info.clone()
        torch.cuda.synchronize()
    assert a.last_plan.path == "batch_views" and b.last_plan.path == "py_views"
    return a, b, d1, d9


def test_trainer_two_views_batched_and_view_by_view_reach_the_same_count(lfs):
    """Two views per step on one rank: batch_views (the SH stages once over both views) against the view-by-view form. The first step's statistic - same parameters
    going in - is bit-equal, both views count, and the refinement at iteration 10 leaves both with the same N and a re-zeroed statistic of that size."""
    a, b, d1, d9 = _two_view_twins(lfs)
    assert torch.equal(d1[0], d1[1]) and float(d1[0][0].max()) == 2 and float(d1[0][1].max()) > 0
    assert float(d9[0][0].max()) == 18 and torch.equal(d9[0][0], d9[1][0])
    print(f"Gaussians after the refinement at iteration 10: batched {a.model.means.shape[0]}, view by view {b.model.means.shape[0]}; max |d statistic| at iteration 9 "
          f"{float((d9[0][1] - d9[1][1]).abs().max()):.3e} of {float(d9[0][1].max()):.3e}")
    assert a.model.means.shape[0] == b.model.means.shape[0] > 1500
    assert tuple(a.densification_info.shape) == tuple(b.densification_info.shape) == (2, a.model.means.shape[0])


def test_trainer_two_views_batched_and_view_by_view_are_bit_equal(lfs):
    """The two-view twin, bit for bit in the deterministic mode. Without ADC the two forms differ in the last bit of dL/dmeans - batched (v_0 + v_1) + (d_0 + d_1)
    (rasterizer parts v_k of the views, SH direction terms d_k from the ONE multi-view SH backward), view by view ((v_0 + d_0) + v_1) + d_1; tests/test_gpu_fused.py holds
    them to 2e-5. Under ADC the view-by-view step sums the direction terms apart (fused.render_and_backward(v_dirs_acc=)) and adds them once, the batched association:
    the same refinement decisions from the same parameters."""
    a, b, _, _ = _two_view_twins(lfs)
    assert a.model.means.shape[0] == b.model.means.shape[0]
    worst = {name: float((p - q).abs().max()) for name, p, q in zip(NAMES, a.model.parameters(), b.model.parameters())}
    print("max |batched - view by view| per parameter:", worst)
    for name, p, q in zip(NAMES, a.model.parameters(), b.model.parameters()):
        assert torch.equal(p, q), (name, worst[name])


# ---- 6. forced collectives --------------------------------------------------------------------------------------------------------------------------------------------
def test_forced_collectives_take_the_factored_step_with_the_same_statistic(lfs):
    from lichtfeld_studio_amd import dist as lfs_dist
    with _deterministic(lfs):
        sc, targets = _adc_scene()
        plain = _adc_trainer(sc)
        for _ in range(9):
            plain.train_step(targets, views=[0])
        forced_flag = lfs_dist._FORCE
        try:
            lfs_dist._FORCE = True
            forced = _adc_trainer(sc, factored_sh=True)
            for _ in range(9):
                forced.train_step(targets, views=[0])
            path = forced.last_plan.path
            for _ in range(2):                               # iteration 10 refines under the forced collectives too
                forced.train_step(targets, views=[0])
        finally:
            lfs_dist._FORCE = forced_flag
        torch.cuda.synchronize()
    assert plain.last_plan.path == "cxx_views" and path == "cxx_factored" and forced.last_plan.multi
    assert forced.model.means.shape[0] > 1500


def test_forced_collectives_statistic_of_one_step_equals_the_unforced_one(lfs):
    from lichtfeld_studio_amd import dist as lfs_dist
    with _deterministic(lfs):
        sc, targets = _adc_scene()
        plain = _adc_trainer(sc)
        plain.train_step(targets, views=[0])
        forced_flag = lfs_dist._FORCE
        try:
            lfs_dist._FORCE = True
            forced = _adc_trainer(sc, factored_sh=True)
            forced.train_step(targets, views=[0])
        finally:
            lfs_dist._FORCE = forced_flag
        torch.cuda.synchronize()
    assert forced.last_plan.path == "cxx_factored"
    assert float(plain.densification_info[1].max()) > 0 and torch.equal(plain.densification_info, forced.densification_info)


# ---- 7. combinations that still raise ---------------------------------------------------------------------------------------------------------------------------------
def test_combinations_without_a_finish_pass_still_raise(lfs):
    from lichtfeld_studio_amd import scenes
    from lichtfeld_studio_amd.trainer import GutTrainer
    sc = scenes.syn_a(n=500, sh_degree=1)
    with pytest.raises(ValueError, match="fused_l2"):
        GutTrainer(sc, DEV, iterations=100, rasterizer="gut", strategy="default", fused_l2=False)
    with pytest.raises(ValueError, match="3DGUT"):
        GutTrainer(sc, DEV, iterations=100, rasterizer="gut", strategy="default", absgrad=True)
    with pytest.raises(ValueError, match="sh_sharded"):
        GutTrainer(sc, DEV, iterations=100, rasterizer="gut", strategy="default", sh_sharded=True)
    assert GutTrainer(sc, DEV, iterations=100, rasterizer="gut", strategy="default").strategy_kind == "default"


def test_library_exports_the_ex_entries(lfs):
    raw = C.CDLL(lfs.library_path())
    for name in ("lfs_gut_view_backward_ex", "lfs_gut_view_backward_finish_ex", "lfs_gut_view_backward_rows_ex", "lfs_gut_finish_grads_ex"):
        assert hasattr(raw, name), name
