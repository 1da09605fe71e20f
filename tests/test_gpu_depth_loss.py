"""GPU parity of the depth loss (lfs_depth_prepare, lfs_depth_l1_loss_fwd_bwd) against the float64 numpy model of tests/depth_loss_reference.py (the formulas of
DESIGN.md 8g). Bounds: those tests/test_gpu_masked_loss.py holds the masked losses to - loss 2e-6 absolute, gradient 1e-5 of the tensor's max.
Sizes: 50 x 35 (no multiple of a wavefront or a workgroup: the grid-stride tail) and 1 x 1. The same bodies run on the wavefront emulator in
tests/test_emulated_depth_loss.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import depth_loss_reference as dref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WEIGHT = 0.5
LOSS0 = 0.25   # the accumulator's value before the call: the entry ADDS to it
SHAPES = [(35, 50), (1, 1)]
CASES = ["no_mask", "soft_mask", "all_invalid", "one_valid"]


def _inputs(case, H, W, seed=0):
    """-> (depth map, raw target with invalid pixels of every sort, mask uint8 or None) as numpy"""
    rng = np.random.RandomState(seed)
    depth = (rng.rand(H, W) * 2.0 + 0.2).astype(np.float32)
    target = (rng.rand(H, W) * 2.0 + 0.2).astype(np.float32)
    mask = rng.randint(0, 256, size=(H, W)).astype(np.uint8) if case == "soft_mask" else None
    if case in ("no_mask", "soft_mask") and H * W > 1:
        bad = rng.rand(H, W) < 0.3
        target[bad] = rng.choice(np.array([0.0, -1.5, np.nan, np.inf, -np.inf], np.float32), size=int(bad.sum()))
        target[0, 0] = depth[0, 0]                                  # D == t: sign(0) = 0
    elif case == "all_invalid":
        target[:] = rng.choice(np.array([0.0, -2.0, np.nan, np.inf], np.float32), size=(H, W))
    elif case == "one_valid":
        keep = target[H // 2, W // 2]
        target[:] = np.nan
        target[H // 2, W // 2] = keep
    return depth, target, mask


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_depth_l1_value_and_gradient_match_the_f64_model(lfs, shape, case):
    from lichtfeld_studio_amd import losses
    H, W = shape
    depth, target, mask = _inputs(case, H, W)
    pd = losses.prepare_depth(torch.from_numpy(target).to(DEV), None if mask is None else torch.from_numpy(mask).to(DEV))
    valid, _ = dref.weights(target, mask)
    got_t = pd.target.cpu().numpy()
    assert np.array_equal(np.isnan(got_t), ~valid) and np.array_equal(got_t[valid], target[valid])      # the sentinel, and the values kept as they are
    assert pd.sums.cpu().tolist() == [dref.int_sum(target, mask)]                                       # the exact integer, on the device
    for shape_d in ((1, H, W), (H, W)):
        loss = torch.full((1,), LOSS0, device=DEV)
        g = losses.depth_l1_loss_fwd_bwd(torch.from_numpy(depth).to(DEV).reshape(shape_d), pd, WEIGHT, loss)
        want, g_want = dref.loss_and_grad(depth, target, mask, WEIGHT)
        err_l = abs(float(loss) - LOSS0 - want)
        err_g = float(np.abs(g.cpu().numpy().reshape(H, W).astype(np.float64) - g_want).max())
        print(f"{case} {H}x{W}: loss {float(loss) - LOSS0:.8f} (model {want:.8f}, |diff| {err_l:.2e} < 2e-6), gradient max |diff| {err_g:.2e} "
              f"(< 1e-5 x {np.abs(g_want).max():.3e} + 1e-12)")
        assert tuple(g.shape) == shape_d and bool(torch.isfinite(g).all()) and bool(torch.isfinite(loss).all())
        assert err_l < 2e-6 and err_g < 1e-5 * float(np.abs(g_want).max()) + 1e-12
        if case == "all_invalid":
            assert float(loss) == LOSS0 and float(g.abs().max()) == 0.0
        else:
            assert float(g.abs().max()) > 0 and float((g.cpu().reshape(H, W) != 0).sum()) <= int(valid.sum())
    if case == "one_valid":      # sum m = 1 (or a soft weight below 1 -> the normaliser stays 1)
        assert int((g != 0).sum()) == 1 and abs(float(g.abs().max()) - WEIGHT) < 1e-7


def test_depth_loss_ignores_the_map_where_the_target_is_invalid_and_prepare_is_idempotent(lfs):
    from lichtfeld_studio_amd import losses
    H, W = 35, 50
    depth, target, mask = _inputs("soft_mask", H, W, seed=3)
    m = torch.from_numpy(mask).to(DEV)
    pd = losses.prepare_depth(torch.from_numpy(target).to(DEV), m)
    again = losses.prepare_depth(pd.target, losses.PreparedMask(m, torch.zeros(2, dtype=torch.int64, device=DEV)))
    assert torch.equal(again.sums, pd.sums) and torch.equal(torch.isnan(again.target), torch.isnan(pd.target))
    # in place: target_out = target_in (the C entry directly; prepare_depth always allocates)
    plane, sums = torch.from_numpy(target).to(DEV), torch.full((1,), -1, dtype=torch.int64, device=DEV)
    assert losses.load_library().lfs_depth_prepare(C.c_uint32(H), C.c_uint32(W), losses.ptr(plane), losses.ptr(m), losses.ptr(plane), losses.ptr(sums), losses.stream()) == 0
    assert torch.equal(sums, pd.sums) and torch.equal(torch.isnan(plane), torch.isnan(pd.target)) and torch.equal(plane[~torch.isnan(plane)], pd.target[~torch.isnan(pd.target)])
    poisoned = depth.copy()
    poisoned[~dref.weights(target, mask)[0]] = np.nan                # a NaN in the render where nothing is supervised must not reach the loss
    la, lb = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    ga = losses.depth_l1_loss_fwd_bwd(torch.from_numpy(depth).to(DEV), pd, 1.0, la)
    gb = losses.depth_l1_loss_fwd_bwd(torch.from_numpy(poisoned).to(DEV), pd, 1.0, lb)
    assert torch.equal(ga, gb) and bool(torch.isfinite(lb).all()) and abs(float(la) - float(lb)) < 2e-6


def test_depth_entry_points_refuse_bad_arguments_before_any_launch(lfs):
    from lichtfeld_studio_amd import losses
    lib = losses.load_library()
    H, W = 9, 13
    p, u32 = losses.ptr, C.c_uint32
    d, tgt = torch.rand(H, W, device=DEV), torch.rand(H, W, device=DEV)
    out, g = torch.full((H, W), 7.0, device=DEV), torch.full((H, W), 7.0, device=DEV)
    sums, loss = torch.full((1,), 5, dtype=torch.int64, device=DEV), torch.full((1,), 3.0, device=DEV)
    prepare = lambda h=H, w=W, i=tgt, o=out, s=sums: lib.lfs_depth_prepare(u32(h), u32(w), p(i), None, p(o), p(s), losses.stream())
    l1 = lambda h=H, w=W, dd=d, t=tgt, s=sums, gg=g, l=loss: lib.lfs_depth_l1_loss_fwd_bwd(u32(h), u32(w), p(dd), p(t), None, p(s), C.c_float(1.0), p(gg), p(l), losses.stream())
    INVALID = -1
    assert prepare(s=None) == INVALID and prepare(i=None) == INVALID and prepare(o=None) == INVALID
    assert l1(dd=None) == INVALID and l1(t=None) == INVALID and l1(s=None) == INVALID and l1(gg=None) == INVALID and l1(l=None) == INVALID
    assert l1(h=0) == 0 and l1(w=0) == 0
    torch.cuda.synchronize()
    assert float(loss) == 3.0 and bool((g == 7.0).all()) and bool((out == 7.0).all()) and sums.cpu().tolist() == [5]
    assert prepare(h=0) == 0 and sums.cpu().tolist() == [0]           # an empty plane: the sum is written (zero), nothing else
    assert prepare() == 0 and l1() == 0
    torch.cuda.synchronize()
    assert sums.cpu().tolist() == [255 * H * W] and float(loss) != 3.0 and torch.equal(out, tgt)
