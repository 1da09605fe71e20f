"""GPU parity: bilateral-grid slice fwd / bwd and TV loss (csrc/bilateral_grid.hip) against oracle/bilateral.py
(float64 = truth). Tolerances (fp32, stated): forward |diff| <= 2e-5 * (1 + |ref|); grad_rgb rel-L2 <= 2e-5 after setting
aside pixels whose luma sits within 1e-4 of a z-cell boundary (the discontinuity mask :150 flips there); grad_grid rel-L2 <= 2e-5
(float atomics: order-dependent rounding only); TV loss rel 1e-5, TV grad rel-L2 1e-6, accumulate form rtol 1e-5 / atol 1e-7.

Which kernel runs is decided on the host from (L, H, W, h, w) (lfs_bilateral_slice_plan); the limit cases (tests/bilateral_cases.py) put a shape on either side
of every decision and on every column-tile count of the windowed MFMA backward, and each asserts the plan it is there for before it runs.

Measured on the MI355X (largest forward |diff| / (1 + |ref|) | grad_rgb rel-L2 | grad_grid rel-L2; all against the bound 2e-5):
  8,16,16 120x200  window nt {1,3,4}            1.16e-6 | 5.97e-7 | 7.66e-7        2,16,16 8x20    bwd LDS 69 632 B: generic    4.38e-7 | 2.69e-7 | 7.88e-7
  8,8,8 64x20      window nt {4}, 64 columns    7.20e-7 | 3.11e-7 | 4.63e-7        16,8,8 16x20    fwd window == 6144           1.06e-6 | 3.64e-7 | 7.73e-7
  5,16,16 40x300   window nt {2}, 20/25 columns 9.85e-7 | 5.02e-7 | 6.59e-7        4,16,16 8x20    fwd window 6912: generic     6.16e-7 | 5.44e-7 | 7.87e-7
  3,12,20 33x257   window nt {1,2}              2.53e-7 | 9.73e-8 | 1.36e-7        3,1,5 4x70      H == 1                       1.26e-7 | 1.15e-7 | 2.31e-7
  2,16,16 33x130   window, 5 y0 per 8 rows      6.66e-7 | 1.81e-7 | 4.86e-7        3,5,1 70x4      W == 1                       1.19e-7 | 1.21e-7 | 1.63e-7
  2,16,16 8x80     window, LDS 63 488 B         7.79e-7 | 2.73e-7 | 7.54e-7        1,1,1 2x2       all extents 1                4.75e-8 | 3.78e-8 | 3.31e-8
  colours in [-0.3, 1.3], no clamp_input:  8,16,16 120x200 (window) 1.68e-6 | 6.01e-7 | 7.64e-7;  8,16,16 67x131 (generic) 9.58e-7 | 5.59e-7 | 7.07e-7
  pixels kept by the z-cell-boundary mask: >= 0.9996 in every L > 1 case (cap 0.99)
TV (loss rel, bound 1e-5 | grad rel-L2, bound 1e-6): 100x12x8x16x16 2.63e-7 | 8.20e-8; 3x12x7x9x11 1.05e-7 | 5.21e-8; 2x12x1x4x5 9.49e-8 | 4.96e-8;
  2x12x3x1x5 1.66e-8 | 4.77e-8; 2x12x3x4x1 4.82e-8 | 4.31e-8; 1x12x1x1x1 loss 0 and gradient 0 exactly."""
import numpy as np
import pytest
import torch

import bilateral_cases as bc
from gpu_util import n, noise_allclose, noise_check, rel_l2, t
from oracle import bilateral as ob
from lichtfeld_studio_amd.capi import LfsError

pytestmark = pytest.mark.gpu


def _case(seed, L, H, W, h, w, lo=0.02, hi=0.98):
    rng = np.random.default_rng(seed)
    grid = (np.broadcast_to(np.eye(4)[:3].reshape(12)[:, None, None, None], (12, L, H, W)) + 0.3 * rng.standard_normal((12, L, H, W))).astype(np.float32)
    rgb = (rng.random((h, w, 3)) * (hi - lo) + lo).astype(np.float32)
    go = rng.standard_normal((h, w, 3)).astype(np.float32)
    return grid, rgb, go


# LDS window path (big images), generic path (grid finer than the pixel tiles), ragged sizes, L = 1
CASES = [dict(L=8, H=16, W=16, h=270, w=480), dict(L=8, H=16, W=16, h=67, w=131), dict(L=4, H=40, W=90, h=24, w=100),
         dict(L=1, H=3, W=2, h=9, w=70), dict(L=8, H=16, W=16, h=2, w=2)]


def _check_slice_against_oracle(bg, label, grid, rgb, go):
    """forward, grad_grid and grad_rgb of one input against the float64 oracle at the file's bounds; prints every figure before it asserts"""
    L = grid.shape[1]
    out = n(bg.slice_forward(t(grid), t(rgb)))
    ref = ob.slice_forward(grid, rgb, np.float64)
    gg, gr = bg.slice_backward(t(grid), t(rgb), t(go))
    rgg, rgr = ob.slice_backward(grid, rgb, go, np.float64)
    z = (0.299 * rgb[..., 0].astype(np.float64) + 0.587 * rgb[..., 1] + 0.114 * rgb[..., 2]) * (L - 1)
    ok = np.abs(z - np.round(z)) > 1e-4
    fwd, e_gr = float((np.abs(out - ref) / (1 + np.abs(ref))).max()), rel_l2(n(gr)[ok], rgr[ok]) if L > 1 else rel_l2(n(gr), rgr)
    print(f"bilateral slice {label}: forward {fwd:.3e} (bound 2e-5), grad_rgb rel-L2 {e_gr:.3e} (bound 2e-5), pixels kept {ok.mean():.5f}")
    assert np.all(np.abs(out - ref) <= 2e-5 * (1 + np.abs(ref))), np.abs(out - ref).max()
    noise_check(f"bilateral grid grad vs fp64 oracle {label}", rel_l2(n(gg), rgg), 2e-5)
    assert ok.mean() > 0.99 or L == 1
    assert e_gr < 2e-5, e_gr


@pytest.mark.parametrize("cfg", CASES)
def test_slice_forward_backward_match_oracle(lfs, cfg):
    from lichtfeld_studio_amd import bilateral_grid as bg
    assert tuple(int(v) for v in bg.slice_plan(**cfg)) == tuple(dict(bc.CASES_PLANS)[tuple(cfg.values())])     # the paths the comment above names
    grid, rgb, go = _case(3, **cfg)
    _check_slice_against_oracle(bg, cfg, grid, rgb, go)


def _assert_plan(bg, case):
    """the kernels this shape runs are the ones the case is there for: the library's own plan, and for the windowed backward the column-tile counts and
    accumulator flushes its strips / wavefronts reach, from the float32 expressions of grid_coord / tile_window"""
    L, H, W, h, w = case.dims
    plan = bg.slice_plan(*case.dims)
    assert tuple(int(v) for v in plan) == tuple(case.plan), (case.dims, plan)
    if plan.bwd_window:
        nt = bc.column_tiles(L, W, w)
        assert set(nt) == case.nt and set(bc.strip_columns(L, W, w)) == case.cols and max(nt) <= plan.col_tiles <= 4, (case.dims, nt)
        if case.dims in bc.FLUSHES:
            assert bc.max_y0_per_wave(H, h) == bc.FLUSHES[case.dims]
    else:
        assert case.nt is None


@pytest.mark.parametrize("case", bc.LIMIT_CASES, ids=lambda c: "L{}_{}x{}_{}x{}".format(*c.dims))
def test_slice_kernel_paths_at_their_limits_match_oracle(lfs, case):
    """Every kernel path of csrc/bilateral_grid.hip on either side of the host's decision (tests/bilateral_cases.py says what each shape pins), same inputs
    recipe, oracle and bounds as test_slice_forward_backward_match_oracle."""
    from lichtfeld_studio_amd import bilateral_grid as bg
    _assert_plan(bg, case)
    L, H, W, h, w = case.dims
    grid, rgb, go = _case(3, L, H, W, h, w)
    _check_slice_against_oracle(bg, case.dims, grid, rgb, go)


@pytest.mark.parametrize("dims", bc.UNCLAMPED, ids=lambda d: "L{}_{}x{}_{}x{}".format(*d))
def test_slice_unclamped_out_of_range_colours_match_oracle(lfs, dims):
    """colours in [-0.3, 1.3] WITHOUT clamp_input: make_tap's two-sided z0 / z1 clamps (guidance below level 0 and above level L - 1), which the oracle
    carries too; one windowed and one generic backward shape"""
    from lichtfeld_studio_amd import bilateral_grid as bg
    plan = bg.slice_plan(*dims)
    assert tuple(int(v) for v in plan) == tuple(dict([(c.dims, c.plan) for c in bc.LIMIT_CASES] + bc.CASES_PLANS)[dims])
    grid, rgb, go = _case(3, *dims, lo=-0.3, hi=1.3)
    luma = rgb @ np.array([0.299, 0.587, 0.114])
    assert (luma < 0).mean() > 0.02 and (luma > 1).mean() > 0.02       # both clamps are exercised
    _check_slice_against_oracle(bg, f"{dims} colours in [-0.3, 1.3]", grid, rgb, go)


def test_slice_chw_and_clamp_extensions(lfs):
    """chw layout == permuted hwc bit for bit; clamp_input == torch.clamp before the op, gradient masked outside [0, 1]."""
    from lichtfeld_studio_amd import bilateral_grid as bg
    grid, rgb, go = _case(5, 8, 16, 16, 120, 200, lo=-0.3, hi=1.3)
    G, x, g = t(grid), t(rgb), t(go)
    ref_out = bg.slice_forward(G, x.clamp(0, 1))
    out = bg.slice_forward(G, x, clamp_input=True)
    assert torch.equal(out, ref_out)
    out_chw = bg.slice_forward(G, x.permute(2, 0, 1).contiguous(), chw=True, clamp_input=True)
    assert torch.equal(out_chw.permute(1, 2, 0), ref_out)
    gg0, gr0 = bg.slice_backward(G, x.clamp(0, 1), g)
    gg1, gr1 = bg.slice_backward(G, x, g, clamp_input=True)
    inside = ((x >= 0) & (x <= 1)).float()
    assert torch.equal(gr1, gr0 * inside)
    noise_allclose("bilateral clamp_input grid grad", gg1, gg0, rtol=1e-4, atol=1e-5 * float(gg0.abs().max()))
    gg2, gr2 = bg.slice_backward(G, x.permute(2, 0, 1).contiguous(), g.permute(2, 0, 1).contiguous(), chw=True, clamp_input=True)
    assert torch.equal(gr2.permute(1, 2, 0), gr1)
    noise_allclose("bilateral chw grid grad", gg2, gg1, rtol=1e-4, atol=1e-5 * float(gg0.abs().max()))
    # accumulation into an existing gradient
    acc = torch.ones_like(G)
    bg.slice_backward(G, x, g, clamp_input=True, grad_grid=acc)
    noise_allclose("bilateral accumulate grid grad", acc - 1, gg1, rtol=1e-4, atol=2e-5 * float(gg0.abs().max()))
    with pytest.raises(LfsError):
        bg.slice_forward(G[:11], x)
    with pytest.raises(LfsError):
        bg.slice_forward(G, x[:1])      # h < 2: the uniform coordinate divides by (h - 1)


def test_tv_loss_and_module(lfs):
    from lichtfeld_studio_amd import bilateral_grid as bg
    rng = np.random.default_rng(9)
    grids = rng.standard_normal((5, 12, 8, 16, 16)).astype(np.float32)
    G = t(grids)
    tv = float(bg.tv_loss_forward(G))
    ref = float(ob.tv_forward(grids, np.float64))
    assert abs(tv - ref) < 1e-5 * ref
    gr = n(bg.tv_loss_backward(G, torch.tensor(0.37)))
    assert rel_l2(gr, ob.tv_backward(grids, 0.37, np.float64)) < 1e-6
    acc = torch.ones_like(G)
    bg.tv_loss_backward(G, 0.37, acc)
    assert np.allclose(n(acc) - 1, gr, rtol=1e-5, atol=1e-7)

    # the module: identity at init, autograd through apply() and tv_loss() equals the raw entry points
    m = bg.BilateralGrid(3, 16, 16, 8)
    img = torch.rand(3, 90, 160, device="cuda:0") * 1.2 - 0.1
    out = m.apply(img, 1)
    assert torch.allclose(out, img.clamp(0, 1), atol=1e-6) and float(m.tv_loss()) == 0.0
    with torch.no_grad():
        m.grids.add_(0.1 * torch.randn_like(m.grids))
    img.requires_grad_(True)
    loss = (m.apply(img[None], 2)[0] ** 2).sum() + 10.0 * m.tv_loss()
    loss.backward()
    g_img, g_grid = img.grad.clone(), m.grids.grad.clone()
    assert float(g_grid[0].abs().max()) > 0 and float(g_grid[2].abs().max()) > float(g_grid[0].abs().max())   # image 0: only the TV term
    # fused (no-autograd) path, CHW layout
    m.grids.grad = None
    loss_acc = torch.zeros(1, device="cuda:0")
    x = img.detach()
    y = m.apply_fused(x, 2, chw=True)
    gx = m.apply_fused_backward(x, 2, 2 * y, chw=True)
    m.tv_loss_fused(10.0, loss_acc)
    assert torch.allclose(gx, g_img, rtol=1e-4, atol=1e-6)
    noise_allclose("bilateral fused-path grid grad", m.grids.grad, g_grid, rtol=1e-4, atol=1e-5 * float(g_grid.abs().max()))
    assert abs(float(loss_acc) + float((y ** 2).sum()) - float(loss)) < 1e-4 * float(loss)


# second pass of both grid-stride loops (2 457 600 elements > 2048 x 1024 and > 8192 x 256), odd extents, each extent of 1 (tv_scales drops that direction), all of them
TV_SHAPES = [(100, 12, 8, 16, 16), (3, 12, 7, 9, 11), (2, 12, 1, 4, 5), (2, 12, 3, 1, 5), (2, 12, 3, 4, 1), (1, 12, 1, 1, 1)]


@pytest.mark.parametrize("shape", TV_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tv_loss_shapes_match_oracle(lfs, shape):
    from lichtfeld_studio_amd import bilateral_grid as bg
    grids = np.random.default_rng(9).standard_normal(shape).astype(np.float32)
    G = t(grids)
    tv = float(bg.tv_loss_forward(G))
    ref = float(ob.tv_forward(grids, np.float64))
    gr = n(bg.tv_loss_backward(G, torch.tensor(0.37)))
    rgr = ob.tv_backward(grids, 0.37, np.float64)
    acc = torch.ones_like(G)
    bg.tv_loss_backward(G, 0.37, acc)
    if shape[2:] == (1, 1, 1):      # no differences in any direction
        assert ref == 0.0 and tv == 0.0 and not gr.any() and not rgr.any() and bool((acc == 1).all())
        return
    print(f"bilateral tv {shape}: loss rel {abs(tv - ref) / ref:.3e} (bound 1e-5), grad rel-L2 {rel_l2(gr, rgr):.3e} (bound 1e-6)")
    assert abs(tv - ref) < 1e-5 * ref
    assert rel_l2(gr, rgr) < 1e-6
    assert np.allclose(n(acc) - 1, gr, rtol=1e-5, atol=1e-7)
    assert np.array_equal(n(acc), np.float32(1) + gr)       # the accumulate form is the same sum followed by one float32 add


def test_gut_trainer_with_bilateral_grid_matches_autograd_composition(lfs):
    """3DGUT fused step + bilateral grid (clamp -> slice -> un-clamped L1 + SSIM loss -> slice backward -> rasterizer backward, TV regulariser,
    grid optimizer) against torch autograd over rasterize() + BilateralGrid.apply() + photometric_loss(): loss and first-step gradients."""
    from lichtfeld_studio_amd import bilateral_grid as bg, losses, scenes
    from lichtfeld_studio_amd.rasterizer import rasterize
    from lichtfeld_studio_amd.trainer import GutTrainer
    from gpu_util import rel_l2
    dev = torch.device("cuda:0")
    sc = scenes.syn_a(n=4000, sh_degree=1)
    tr = GutTrainer(sc, dev, iterations=300, loss="l1_ssim", use_bilateral_grid=True, tv_loss_weight=10.0)
    with torch.no_grad():
        tr.bilateral.grids.add_(0.05 * torch.randn(tr.bilateral.grids.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(3)))
    target = (scenes.target_image(sc.height, sc.width) * 0.8 + 0.1).to(dev)
    out = rasterize(tr.camera(0), tr.model, tr.bg, 1.0, False, False)
    shown = tr.bilateral.apply(out.image, 0)
    loss_ref = losses.photometric_loss(shown, target, 0.2) + 10.0 * tr.bilateral.tv_loss()
    loss_ref.backward()
    ref_grads = [p.grad.clone() for p in tr.model.parameters()]
    ref_grid = tr.bilateral.grids.grad.clone()
    for p in tr.model.parameters():
        p.grad = None
    tr.bilateral.grids.grad = torch.zeros_like(tr.bilateral.grids)
    grids_before = tr.bilateral.grids.detach().clone()
    loss = tr.train_step([target], views=[0])
    assert abs(float(loss) - float(loss_ref)) < 3e-6 * max(1.0, float(loss_ref))
    for name, g, r in zip(["means", "sh0", "shN", "raw_scales", "raw_quats", "raw_opacities"], tr.bucket.views, ref_grads):
        assert rel_l2(n(g), n(r).reshape(n(g).shape)) < 2e-3, (name, rel_l2(n(g), n(r).reshape(n(g).shape)))
    assert float(ref_grid.abs().max()) > 0 and bool((tr.bilateral.grids.detach() != grids_before).any())
    losses_seen = [float(tr.train_step([target], views=[0])) for _ in range(40)]
    assert np.isfinite(losses_seen).all() and losses_seen[-1] < losses_seen[0]
