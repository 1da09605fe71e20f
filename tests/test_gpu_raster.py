"""GPU parity: K7 / K8 world-space rasterization forward and backward vs the oracle.

Tolerance model (the reference itself uses __expf / rsqrt / fast division and a
warp-order-dependent float accumulation, so fp32 bit equality does not exist even between two of
its own runs):
  forward : mean |rgb diff| <= 2e-6; <= 0.1 % of pixels deviate by more than 1/255 + 1e-4 (one
            alpha-threshold / early-termination flip moves a pixel by at most one contribution);
            alpha likewise; last_ids equal on >= 99.9 % of the pixels.
  backward: per-tensor relative L2 error vs the fp64 oracle <= 2e-4 (measured: ~1e-5) with the threshold-flip
            Gaussians COUNTED (gpu_util.rows_check: <= 2 rows per tensor may be off by more than 1 % of the
            largest row - ONE alpha-threshold flip at one pixel moves one Gaussian's geometry gradient by
            ~1e-3 of the tensor norm), same vs the fp32 oracle up to its own distance from fp64; the
            oracle's forward outputs are fed to both sides. At the full 1M / 3M sizes: test_gpu_headline_parity.py.
"""
import os

import numpy as np
import pytest
import torch

from gpu_util import atomic_noise_bar, make_gaussians, n, noise_check, pinhole_K, rel_l2, rows_check, small_rotation_viewmat, t

pytestmark = pytest.mark.gpu


def _lists(oracle, means, quats, scales, opac, vm0, vm1, K, W, H, ts, model, shutter, rad, tan, thin):
    C = K.shape[0]
    radii, m2, d, _, _ = oracle.projection_ut_3dgs_fused(means, quats, scales, opac, vm0, vm1, K, W, H, camera_model=int(model),
                                                         rs_type=int(shutter), radial_coeffs=rad, tangential_coeffs=tan, thin_prism_coeffs=thin)
    tw, th = (W + ts - 1) // ts, (H + ts - 1) // ts
    _, ids, flat = oracle.intersect_tile(m2, radii, d, C, ts, tw, th, True)
    return oracle.intersect_offset(ids, C, tw, th), flat


def _run(oracle, lfs, ops, rng, N, W, H, ts=16, C=1, cdim=3, bg=True, masks=None, model=None, shutter=None, rad=None, tan=None, thin=None,
         vm1=None, spread=1.0, smin=0.01, smax=0.06, check_bwd=True, bwd_bar=2e-4):
    model = lfs.CameraModelType.PINHOLE if model is None else model
    shutter = lfs.ShutterType.GLOBAL if shutter is None else shutter
    means, quats, scales, opac = make_gaussians(rng, N, spread=spread, smin=smin, smax=smax)
    vm0 = np.stack([small_rotation_viewmat(rng, 0.05 + 0.1 * c, 0.1) for c in range(C)])
    K = pinhole_K(0.8 * W, W, H, C)
    colors = rng.random((C, N, cdim)).astype(np.float32)
    opacs = np.tile(opac[None], (C, 1)) * rng.uniform(0.8, 1.0, (C, 1)).astype(np.float32)
    bgc = rng.random((C, cdim)).astype(np.float32) if bg else None
    offs, flat = _lists(oracle, means, quats, scales, opac, vm0, vm1, K, W, H, ts, model, shutter, rad, tan, thin)
    assert len(flat) > 0
    args_o = (means, quats, scales, colors, opacs, bgc, masks, W, H, ts, vm0, vm1, K, int(model), int(shutter), rad, tan, thin, offs, flat)
    o_rc, o_ra, o_li = oracle.rasterize_fwd(*args_o)
    args_g = (t(means), t(quats), t(scales), t(colors), t(opacs), t(bgc), t(masks, torch.bool), W, H, ts, t(vm0), t(vm1), t(K), model, None, shutter,
              t(rad), t(tan), t(thin), t(offs, torch.int32), t(flat, torch.int32))
    g_rc, g_ra, g_li = ops.rasterize_to_pixels_from_world_3dgs_fwd(*args_g)
    assert g_rc.shape == (C, H, W, cdim) and g_ra.shape == (C, H, W, 1) and g_li.shape == (C, H, W) and g_li.dtype == torch.int32
    d = np.abs(n(g_rc) - o_rc)
    assert d.mean() < 2e-6, d.mean()
    assert (d > 1 / 255 + 1e-4).mean() < 1e-3
    da = np.abs(n(g_ra) - o_ra)
    assert da.mean() < 2e-6 and (da > 1 / 255 + 1e-4).mean() < 1e-3
    assert (n(g_li) == o_li).mean() > 0.999
    assert (o_ra > 0.05).mean() > 0.05, "degenerate test scene"
    if not check_bwd:
        return
    v_rc = rng.standard_normal(o_rc.shape).astype(np.float32)
    v_ra = rng.standard_normal(o_ra.shape).astype(np.float32)
    og = oracle.rasterize_bwd(*args_o, o_ra, o_li, v_rc, v_ra)
    og64 = oracle.rasterize_bwd(*args_o, o_ra, o_li, v_rc, v_ra, dtype=np.float64)
    gg = ops.rasterize_to_pixels_from_world_3dgs_bwd(*args_g, t(o_ra), t(o_li, torch.int32), t(v_rc), t(v_ra))
    for name, a, b, c in zip(["v_means", "v_quats", "v_scales", "v_colors", "v_opacities"], gg, og, og64):
        assert a.shape == tuple(b.shape), name
        assert np.isfinite(n(a)).all(), name
        # fp64 oracle = truth. An alpha-threshold flip (alpha vs 1/255 or the 0.999 cap, v_exp_f32 vs exp) hits single (pixel, Gaussian) pairs:
        # such rows are counted (<= 2 per tensor in these 3 000 - 10 000-Gaussian scenes) and everything else has to agree to 2e-4.
        def per_gauss(x):   # one row per Gaussian (per (camera, Gaussian) for colours and opacities)
            x = np.asarray(x)
            return x.reshape(-1, 1) if name == "v_opacities" else x.reshape(-1, x.shape[-1])
        e64, flips64, rest64 = rows_check(per_gauss(n(a)), per_gauss(c), bar=bwd_bar, max_flips=2)
        e32, flips32, rest32 = rows_check(per_gauss(n(a)), per_gauss(b), bar=max(bwd_bar, 3 * rel_l2(b, c)), max_flips=2)
        print(f"raster bwd {name}: vs fp64 oracle rel-L2 {e64:.2e} flips {flips64} rest {rest64:.2e} | vs fp32 oracle {e32:.2e} flips {flips32} rest {rest32:.2e}")
        assert rest64 < bwd_bar, (name, e64, flips64, rest64)
        assert rest32 < max(bwd_bar, 3 * rel_l2(b, c)), (name, e32, flips32, rest32)
    return gg


def test_raster_pinhole_rgb(lfs, oracle_mod):
    from lichtfeld_studio_amd import ops
    _run(oracle_mod, lfs, ops, np.random.default_rng(0), 10000, 256, 256)


def test_raster_ragged_image_no_background(lfs, oracle_mod):
    from lichtfeld_studio_amd import ops
    _run(oracle_mod, lfs, ops, np.random.default_rng(1), 4000, 203, 117, bg=False)


@pytest.mark.parametrize("cdim", [1, 2, 4])
def test_raster_channel_counts(lfs, oracle_mod, cdim):
    """depth (1) and RGB+depth (4) render modes of rasterizer.cpp:278-297"""
    from lichtfeld_studio_amd import ops
    _run(oracle_mod, lfs, ops, np.random.default_rng(2 + cdim), 3000, 128, 96, cdim=cdim)


@pytest.mark.parametrize("ts", [8, 24, 32, 48])
def test_raster_other_tile_sizes(lfs, oracle_mod, ts):
    """24 -> 9 cells per tile, one wavefront per workgroup; 32 / 48 also exercise the opt-in 16x8 cells (8 resp. 18 per tile)"""
    from lichtfeld_studio_amd import ops
    _run(oracle_mod, lfs, ops, np.random.default_rng(10 + ts), 3000, 160, 100, ts=ts)


def test_raster_two_cameras(lfs, oracle_mod):
    """C > 1: geometry indexed with g % N, colours / opacities with the flattened id."""
    from lichtfeld_studio_amd import ops
    _run(oracle_mod, lfs, ops, np.random.default_rng(20), 3000, 128, 96, C=2)


def test_raster_tile_masks(lfs, oracle_mod):
    from lichtfeld_studio_amd import ops
    rng = np.random.default_rng(21)
    masks = rng.random((1, 6, 8)) > 0.3
    _run(oracle_mod, lfs, ops, rng, 3000, 128, 96, masks=masks)


def test_raster_dense_scene_early_termination(lfs, oracle_mod):
    """big opaque Gaussians: pixels saturate (T <= 1e-4) long before the tile list ends"""
    from lichtfeld_studio_amd import ops
    _run(oracle_mod, lfs, ops, np.random.default_rng(22), 6000, 128, 128, spread=0.4, smin=0.05, smax=0.3)


def test_raster_opencv_distortion(lfs, oracle_mod):
    from lichtfeld_studio_amd import ops
    _run(oracle_mod, lfs, ops, np.random.default_rng(23), 3000, 128, 96,
         rad=np.array([[-0.1, 0.02, 0.0, 0.0]], np.float32), tan=np.array([[0.001, -0.002]], np.float32))


def test_raster_fisheye(lfs, oracle_mod):
    from lichtfeld_studio_amd import ops
    _run(oracle_mod, lfs, ops, np.random.default_rng(24), 3000, 128, 128, model=lfs.CameraModelType.FISHEYE,
         rad=np.array([[0.01, -0.002, 0.0, 0.0]], np.float32))


@pytest.mark.parametrize("shutter", [0, 3])
def test_raster_rolling_shutter(lfs, oracle_mod, shutter):
    """per-pixel ray origin: the kernels' non-uniform-origin path"""
    from lichtfeld_studio_amd import ops
    rng = np.random.default_rng(25 + shutter)
    _run(oracle_mod, lfs, ops, rng, 3000, 128, 96, shutter=lfs.ShutterType(shutter), vm1=small_rotation_viewmat(rng, 0.12, 0.2)[None])


def test_raster_empty_intersections(lfs):
    from lichtfeld_studio_amd import ops
    dev = "cuda:0"
    N, W, H = 10, 64, 48
    means = torch.randn(N, 3, device=dev); quats = torch.randn(N, 4, device=dev); scales = torch.rand(N, 3, device=dev) + 0.1
    colors = torch.rand(1, N, 3, device=dev); opac = torch.rand(1, N, device=dev); bg = torch.tensor([[0.3, 0.2, 0.1]], device=dev)
    offs = torch.zeros((1, 3, 4), dtype=torch.int32, device=dev); flat = torch.zeros(0, dtype=torch.int32, device=dev)
    vm = torch.eye(4, device=dev)[None].contiguous(); K = torch.tensor([[[50., 0, 32], [0, 50., 24], [0, 0, 1]]], device=dev)
    rc, ra, li = ops.rasterize_to_pixels_from_world_3dgs_fwd(means, quats, scales, colors, opac, bg, None, W, H, 16, vm, None, K,
                                                             lfs.CameraModelType.PINHOLE, None, lfs.ShutterType.GLOBAL, None, None, None, offs, flat)
    assert torch.allclose(rc, bg.view(1, 1, 1, 3).expand_as(rc)) and float(ra.abs().max()) == 0 and int(li.abs().max()) == 0
    g = ops.rasterize_to_pixels_from_world_3dgs_bwd(means, quats, scales, colors, opac, bg, None, W, H, 16, vm, None, K,
                                                    lfs.CameraModelType.PINHOLE, None, lfs.ShutterType.GLOBAL, None, None, None, offs, flat,
                                                    ra, li, torch.ones_like(rc), torch.ones_like(ra))
    assert all(float(x.abs().max()) == 0 for x in g)


def test_raster_unsupported_channels_raises(lfs):
    from lichtfeld_studio_amd import ops
    dev = "cuda:0"
    z = lambda *s: torch.zeros(*s, device=dev)
    with pytest.raises(RuntimeError):
        ops.rasterize_to_pixels_from_world_3dgs_fwd(z(4, 3), z(4, 4), z(4, 3), z(1, 4, 7), z(1, 4), None, None, 32, 32, 16,
                                                    torch.eye(4, device=dev)[None].contiguous(), None, torch.eye(3, device=dev)[None].contiguous(),
                                                    lfs.CameraModelType.PINHOLE, None, lfs.ShutterType.GLOBAL, None, None, None,
                                                    torch.zeros((1, 2, 2), dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.int32, device=dev))


def test_raster_refuses_more_rows_than_the_backward_can_address(lfs):
    """cameras x Gaussians >= 2^25: the backward's buffer atomic addresses 2 GB of accumulator rows and relies on 0x80000000 being out of range (lfs_raster_common.cuh,
    RED_BUF_DEAD / RED_MAX_ROWS) - the entry points refuse such a call up front (raster_check: LFS_E_UNSUPPORTED -> RuntimeError) instead of running it; one row fewer is accepted."""
    from lichtfeld_studio_amd import ops
    dev = "cuda:0"
    z = lambda *s: torch.zeros(*s, device=dev)
    def call(N):
        return ops.rasterize_to_pixels_from_world_3dgs_fwd(z(N, 3), z(N, 4), z(N, 3), z(1, N, 3), z(1, N), None, None, 32, 32, 16,
                                                           torch.eye(4, device=dev)[None].contiguous(), None, torch.eye(3, device=dev)[None].contiguous(),
                                                           lfs.CameraModelType.PINHOLE, None, lfs.ShutterType.GLOBAL, None, None, None,
                                                           torch.zeros((1, 2, 2), dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.int32, device=dev))
    with pytest.raises(RuntimeError):
        call(1 << 25)
    rc, ra, li = call((1 << 25) - 1)   # (no intersections: the image is empty, the call is valid)
    assert float(ra.abs().max()) == 0.0
    torch.cuda.empty_cache()


def test_raster_bwd_is_linear_in_output_gradients_full_size(lfs):
    """BASELINE config-2 sized property test (no oracle needed): the backward is linear in
    (v_render_colors, v_render_alphas), fwd is deterministic, alpha in [0, 1], gradients finite."""
    from lichtfeld_studio_amd import ops, scenes
    from lichtfeld_studio_amd.rasterizer import Camera, SplatModel, rasterize
    dev = torch.device("cuda:0")
    sc = scenes.syn_b(n=1_000_000, n_views=4).to(dev)
    model = SplatModel(sc.means, sc.sh0, sc.shN, sc.raw_scales, sc.raw_quats, sc.raw_opacities, 3)
    cam = Camera(sc.viewmats[:1].contiguous(), sc.Ks[:1].contiguous(), sc.width, sc.height)
    with torch.no_grad():
        a = rasterize(cam, model, torch.zeros(3, device=dev))
        b = rasterize(cam, model, torch.zeros(3, device=dev))
    assert torch.equal(a.image, b.image) and torch.equal(a.alpha, b.alpha)
    assert float(a.alpha.min()) >= 0 and float(a.alpha.max()) <= 1 and a.n_isects > 3_000_000
    # linearity through the raw op
    quats = torch.nn.functional.normalize(sc.raw_quats, dim=-1); scales = sc.raw_scales.exp(); opac = torch.sigmoid(sc.raw_opacities)[None]
    radii, m2, d, _, _ = ops.projection_ut_3dgs_fused(sc.means, quats, scales, opac[0], cam.world_view_transform, None, cam.K, sc.width, sc.height,
                                                      0.3, 0.01, 1e4, 0.0, False, lfs.CameraModelType.PINHOLE)
    _, ids, flat, offs = ops.intersect_tile(m2, radii, d, None, None, 1, 16, 120, 68, True, return_offsets=True)
    colors = torch.rand(1, sc.N, 3, device=dev)
    fa = (sc.means, quats, scales, colors, opac, None, None, sc.width, sc.height, 16, cam.world_view_transform, None, cam.K,
          lfs.CameraModelType.PINHOLE, None, lfs.ShutterType.GLOBAL, None, None, None, offs, flat)
    rc, ra, li = ops.rasterize_to_pixels_from_world_3dgs_fwd(*fa)
    g = torch.Generator(device=dev).manual_seed(0)
    v1, v2 = torch.randn(rc.shape, device=dev, generator=g), torch.randn(rc.shape, device=dev, generator=g)
    w1, w2 = torch.randn(ra.shape, device=dev, generator=g), torch.randn(ra.shape, device=dev, generator=g)
    g1 = ops.rasterize_to_pixels_from_world_3dgs_bwd(*fa, ra, li, v1, w1)
    g2 = ops.rasterize_to_pixels_from_world_3dgs_bwd(*fa, ra, li, v2, w2)
    g12 = ops.rasterize_to_pixels_from_world_3dgs_bwd(*fa, ra, li, (2 * v1 - 3 * v2).contiguous(), (2 * w1 - 3 * w2).contiguous())
    for x1, x2, x12 in zip(g1, g2, g12):
        assert torch.isfinite(x12).all()
        lin = 2 * x1 - 3 * x2
        assert float((x12 - lin).norm() / (lin.norm() + 1e-20)) < 1e-4


def _cull_on_off(lfs, fn):
    lib = lfs.load_library()
    try:
        lib.lfs_set_debug_flags(1)   # per-cell lists = full tile lists
        ref = fn()
    finally:
        lib.lfs_set_debug_flags(0)
    return ref, fn()


@pytest.mark.parametrize("kind", ["small", "needles", "huge_and_near", "low_opacity", "flat_disks"])
def test_cell_culling_is_conservative(lfs, oracle_mod, kind):
    """The per-8x8-cell culling (raster_cull_kernel) may only drop entries that cannot reach alpha >= 1/255 on any
    ray of the cell: forward outputs must be BIT-identical with culling on and off; the backward BIT-identical in the deterministic accumulation mode
    (order-independent integer sums: a culled entry contributes nothing either way), and equal up to the float-atomic summation order in the default mode."""
    from lichtfeld_studio_amd import ops
    rng = np.random.default_rng({"small": 40, "needles": 41, "huge_and_near": 42, "low_opacity": 43, "flat_disks": 44}[kind])
    N, W, H, ts = 6000, 200, 136, 16
    means, quats, scales, opac = make_gaussians(rng, N, spread=1.5, smin=0.01, smax=0.05)
    if kind == "needles":
        scales = (np.exp(rng.uniform(np.log(1e-4), np.log(0.5), (N, 3)))).astype(np.float32)
    elif kind == "huge_and_near":
        scales[: N // 4] *= 40.0                                   # screen-filling
        means[N // 4: N // 2, 2] = rng.uniform(0.02, 0.3, N // 4)  # right in front of the camera plane
        means[N // 2: N // 2 + 200, 2] = rng.uniform(-0.5, 0.0, 200)  # behind the camera (never listed by the projection, listed here on purpose)
    elif kind == "low_opacity":
        opac = rng.uniform(0.0, 0.02, N).astype(np.float32)
        opac[::7] = 0.9
    elif kind == "flat_disks":   # (round 5) the shape of a trained scene: one axis 20 - 100 x thinner than the other two - the silhouette conic (lfs_cull_conic.cuh) of a disk seen edge-on
        scales = (rng.random((N, 3)) * 0.2 + 0.05).astype(np.float32)
        thin = rng.integers(0, 3, N)
        scales[np.arange(N), thin] = scales.max(-1) / rng.uniform(20.0, 100.0, N).astype(np.float32)
    vm0 = small_rotation_viewmat(rng, 0.2, 0.3)[None]
    K = pinhole_K(0.8 * W, W, H, 1)
    colors = rng.random((1, N, 3)).astype(np.float32)
    tw, th = (W + ts - 1) // ts, (H + ts - 1) // ts
    # adversarial lists: EVERY Gaussian is listed in EVERY tile (depth-sorted) - culling has to sort it out
    depth = (means @ vm0[0, :3, :3].T + vm0[0, :3, 3])[:, 2]
    order = np.argsort(depth, kind="stable").astype(np.int32)
    n_t = tw * th
    per_tile = 400
    flat = np.concatenate([np.sort(rng.choice(N, per_tile, replace=False)) for _ in range(n_t)]).astype(np.int32)
    flat = order[flat.reshape(n_t, per_tile)].reshape(-1)  # ascending depth inside each tile
    offs = (np.arange(n_t, dtype=np.int32) * per_tile).reshape(1, th, tw)
    args = (t(means), t(quats), t(scales), t(colors), t(opac[None]), None, None, W, H, ts, t(vm0), None, t(K), lfs.CameraModelType.PINHOLE, None,
            lfs.ShutterType.GLOBAL, None, None, None, t(offs, torch.int32), t(flat, torch.int32))
    (r0, a0, l0), (r1, a1, l1) = _cull_on_off(lfs, lambda: ops.rasterize_to_pixels_from_world_3dgs_fwd(*args))
    assert torch.equal(r0, r1) and torch.equal(a0, a1) and torch.equal(l0, l1)
    assert float(a1.max()) > 0.05, "degenerate scene"
    v_rc, v_ra = t(rng.standard_normal(tuple(r1.shape)).astype(np.float32)), t(rng.standard_normal(tuple(a1.shape)).astype(np.float32))
    bwd = lambda: ops.rasterize_to_pixels_from_world_3dgs_bwd(*args, a1, l1, v_rc, v_ra)
    lib = lfs.load_library()

    def with_flags(flags):
        try:
            lib.lfs_set_debug_flags(flags)
            return bwd()
        finally:
            lib.lfs_set_debug_flags(0)
    for i, (x_off, x_on) in enumerate(zip(with_flags(16 | 1), with_flags(16))):   # the exact statement
        assert torch.isfinite(x_on).all()
        assert torch.equal(x_off, x_on), f"deterministic mode, culling on vs off: bwd[{i}] differs"
    g0, g1 = _cull_on_off(lfs, bwd)
    g2, g3, g4 = bwd(), bwd(), bwd()  # run-to-run noise of the float atomics (large and heavy-tailed for ill-conditioned needles: four draws; the bar is wide -
    for i, (x0, x1, x2, x3, x4) in enumerate(zip(g0, g1, g2, g3, g4)):   # the sharp check is the deterministic one above)
        assert torch.isfinite(x1).all()
        noise_check(f"cull on/off bwd[{i}] {kind}", rel_l2(n(x0), n(x1)), atomic_noise_bar(x1, x2, x3, x4, floor=5e-5, k=24.0))


def test_cell_culling_full_size_bit_identical(lfs):
    """SYN-B (1M Gaussians, 1080p) through the real projection / intersection lists."""
    from lichtfeld_studio_amd import scenes
    from lichtfeld_studio_amd.rasterizer import Camera, SplatModel, rasterize
    dev = torch.device("cuda:0")
    sc = scenes.syn_b(n=1_000_000, n_views=4).to(dev)
    model = SplatModel(sc.means, sc.sh0, sc.shN, sc.raw_scales, sc.raw_quats, sc.raw_opacities, 3)
    cam = Camera(sc.viewmats[1:2].contiguous(), sc.Ks[1:2].contiguous(), sc.width, sc.height)
    with torch.no_grad():
        a, b = _cull_on_off(lfs, lambda: rasterize(cam, model, torch.zeros(3, device=dev)))
    assert torch.equal(a.image, b.image) and torch.equal(a.alpha, b.alpha)


def test_prepared_backward_equals_self_contained_backward(lfs, oracle_mod):
    """lfs_rasterize_..._bwd_prepared (reuses the forward's records and per-cell lists) vs the self-contained entry."""
    from lichtfeld_studio_amd import ops
    rng = np.random.default_rng(77)
    N, W, H, ts = 5000, 176, 144, 16
    means, quats, scales, opac = make_gaussians(rng, N)
    vm0 = small_rotation_viewmat(rng, 0.1, 0.1)[None]
    K = pinhole_K(0.8 * W, W, H, 1)
    colors = rng.random((1, N, 3)).astype(np.float32)
    offs, flat = _lists(oracle_mod, means, quats, scales, opac, vm0, None, K, W, H, ts, lfs.CameraModelType.PINHOLE, lfs.ShutterType.GLOBAL, None, None, None)
    args = (t(means), t(quats), t(scales), t(colors), t(opac[None]), t(rng.random((1, 3)).astype(np.float32)), None, W, H, ts, t(vm0), None, t(K),
            lfs.CameraModelType.PINHOLE, None, lfs.ShutterType.GLOBAL, None, None, None, t(offs, torch.int32), t(flat, torch.int32))
    rc, ra, li, ws = ops.rasterize_to_pixels_from_world_3dgs_fwd(*args, own_workspace=True)
    rc2, ra2, li2 = ops.rasterize_to_pixels_from_world_3dgs_fwd(*args)
    assert torch.equal(rc, rc2) and torch.equal(ra, ra2) and torch.equal(li, li2)
    v_rc, v_ra = torch.randn_like(rc), torch.randn_like(ra)
    ga = ops.rasterize_to_pixels_from_world_3dgs_bwd(*args, ra, li, v_rc, v_ra, prepared_workspace=ws)
    gb = ops.rasterize_to_pixels_from_world_3dgs_bwd(*args, ra, li, v_rc, v_ra)
    gc = ops.rasterize_to_pixels_from_world_3dgs_bwd(*args, ra, li, v_rc, v_ra)   # a second draw of the float-atomic sums: the bar is relative to their own noise
    for i, (a, b, c) in enumerate(zip(ga, gb, gc)):
        noise_check(f"prepared vs self-contained bwd[{i}]", rel_l2(n(a), n(b)), atomic_noise_bar(c, b))


def test_deterministic_backward_mode_is_bit_reproducible(lfs, oracle_mod):
    """lfs_set_debug_flags(16): the backward's per-Gaussian sums go through order-independent integer atomics (maximum of |total| per slot, then
    64-bit fixed-point adds 40 bits below it) instead of float atomics: repeated runs are BIT-identical, and the result agrees with the
    default mode to the float-atomics' own rounding noise. Also through the fused training step (loss folded into the backward)."""
    from lichtfeld_studio_amd import ops, scenes
    from lichtfeld_studio_amd.fused import render_and_backward
    from lichtfeld_studio_amd.trainer import GutTrainer
    rng = np.random.default_rng(77)
    N, W, H = 20000, 320, 240
    means, quats, scales, opac = make_gaussians(rng, N, smin=0.01, smax=0.08)
    vm0 = np.stack([small_rotation_viewmat(rng, 0.05, 0.1)])
    K = pinhole_K(0.8 * W, W, H, 1)
    colors = rng.random((1, N, 3)).astype(np.float32)
    offs, flat = _lists(oracle_mod, means, quats, scales, opac, vm0, None, K, W, H, 16, lfs.CameraModelType.PINHOLE, lfs.ShutterType.GLOBAL, None, None, None)
    args = (t(means), t(quats), t(scales), t(colors), t(opac[None]), t(rng.random((1, 3)).astype(np.float32)), None, W, H, 16, t(vm0), None, t(K),
            lfs.CameraModelType.PINHOLE, None, lfs.ShutterType.GLOBAL, None, None, None, t(offs, torch.int32), t(flat, torch.int32))
    rc, ra, li = ops.rasterize_to_pixels_from_world_3dgs_fwd(*args)
    v_rc, v_ra = torch.randn_like(rc), torch.randn_like(ra)
    ref = ops.rasterize_to_pixels_from_world_3dgs_bwd(*args, ra, li, v_rc, v_ra)
    ref2 = ops.rasterize_to_pixels_from_world_3dgs_bwd(*args, ra, li, v_rc, v_ra)  # second draw of the float-atomic mode: its own run-to-run noise
    lib = lfs.load_library()
    try:
        lib.lfs_set_debug_flags(16)
        runs = [ops.rasterize_to_pixels_from_world_3dgs_bwd(*args, ra, li, v_rc, v_ra) for _ in range(3)]
        sc = scenes.syn_a(n=8000, sh_degree=1)
        target = scenes.target_image(sc.height, sc.width).to("cuda:0")
        fused = []
        for _ in range(2):
            tr = GutTrainer(sc, torch.device("cuda:0"), iterations=100)
            grads = [torch.zeros_like(p) for p in tr.model.parameters()]
            loss = torch.zeros(1, device="cuda:0")
            render_and_backward(tr.camera(0), tr.model, tr.bg, target, 1.0, grads, loss, accumulate=False)
            fused.append([g.clone() for g in grads])
    finally:
        lib.lfs_set_debug_flags(0)
    for name, a, b, c, r, r2 in zip(["v_means", "v_quats", "v_scales", "v_colors", "v_opacities"], *runs, ref, ref2):
        assert torch.equal(a, b) and torch.equal(a, c), name
        assert torch.isfinite(a).all()
        # the float-atomic operand is ONE draw of an order-dependent sum (run-to-run ~1e-5 on v_quats): the bar is max(2e-5, 5 x that noise), never a
        # constant on the noise floor (round 3's 1e-5 bar failed at 1.000015e-05 on the driver's box)
        noise_check(f"deterministic vs float-atomic {name}", rel_l2(n(a), n(r)), atomic_noise_bar(r2, r))
    for a, b in zip(*fused):
        assert torch.equal(a, b) and float(a.abs().max()) > 0


def test_instruction_properties_the_backward_relies_on(tmp_path):
    """tests/hw_probe.hip, compiled and run here: v_rcp_f32 is exact at 1.0 (and on every power of two), v_mul_legacy_f32 gives 0 * inf = 0 * NaN = 0 - what
    the alpha = 0 lanes of raster_bwd_kernel and mul_zero (raster.hip / lfs_raster_common.cuh, round 6) assume and what no parity bar would notice."""
    import json
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    exe = str(tmp_path / "hw_probe")
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hw_probe.hip")
    r = subprocess.run([hipcc, "-O2", "--offload-arch=gfx950", src, "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    d = json.loads(r.stdout.strip().splitlines()[-1])
    print(d)
    assert d["rcp_of_one_bits"] == "0x3f800000" and d["rcp_exact_on_powers_of_two"] == 1 and d["mul_legacy_zero_times_anything_is_zero"] == 1, d


def test_lds_reduction_asm_block_agrees_with_the_compiler_generated_stores(lfs, tmp_path):
    """The backward's 16-value (3DGUT) / 9-value (EWA) wave reduction stores its values with ds_write_addtid_b32 from an inline-asm block that sets M0 (saved and
    restored inside the block, lfs_raster_common.cuh). The second library of the build (build.build_variants: -DLFS_RED_ADDTID=0, plain ds_write2_b32 stores the
    compiler schedules itself) runs the same inputs in a subprocess: the per-Gaussian sums may differ in the order of their additions only. 3DGUT gradients in
    the deterministic accumulation mode (run-to-run bit-identical within a library): 5e-5 relative L2 (the two layouts add a wavefront's 64 values in different orders); EWA gradients (float atomics): noise-relative."""
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    variant = os.path.join(os.path.dirname(here), "lichtfeld-studio_amd", "liblfs_gsplat_red_ds_write2.so")
    if not os.path.exists(variant):
        pytest.skip("liblfs_gsplat_red_ds_write2.so not built (__graft_entry__.build())")
    res = {}
    for tag, libpath in (("default", None), ("ds_write2", variant)):
        env = dict(os.environ)
        env.pop("LFS_GSPLAT_LIB", None)
        if libpath:
            env["LFS_GSPLAT_LIB"] = libpath
        out = str(tmp_path / f"{tag}.npz")
        r = subprocess.run([sys.executable, os.path.join(here, "lds_reduction_probe.py"), out], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        res[tag] = dict(np.load(out))
    a, b = res["default"], res["ds_write2"]
    for k in [k for k in a if k.startswith("gut_")]:
        assert np.isfinite(a[k]).all() and np.abs(a[k]).max() > 0
        noise_check(f"LDS reduction asm vs ds_write2 {k}", rel_l2(a[k], b[k]), 5e-5)   # (measured 1e-7 .. 1.2e-5: v_quats is a difference of large terms)
    for name in ["means", "sh0", "shN", "raw_scales", "raw_quats", "raw_opacities"]:
        x0, x1, y0 = a[f"fastgs0_{name}"], a[f"fastgs1_{name}"], b[f"fastgs0_{name}"]
        if np.abs(x0).max() == 0:
            assert np.abs(y0).max() == 0
            continue
        noise_check(f"EWA LDS reduction asm vs ds_write2 {name}", rel_l2(y0, x0), atomic_noise_bar(x0, x1, b[f"fastgs1_{name}"]))


def test_every_refused_rasterizer_call_returns_its_code_and_writes_nothing(lfs):
    """tests/raster_refusals.py on the real library: each single-fault call of the forward, the five backwards, lfs_gut_finish_grads and lfs_gut_finish_adam
    returns the code of its row and leaves its outputs and its workspace untouched (the emulated runner: tests/test_emulated_raster_refusals.py)."""
    import raster_refusals
    assert raster_refusals.run_all() == sum(len(entries) for entries, _, _, _ in raster_refusals.ROWS)
