"""GPU: the antialiased mode of the fastgs (EWA) rasterizer (lfs_fastgs_view_preprocess, LFS_FASTGS_ANTIALIASED).

The mode multiplies a primitive's opacity by rho = sqrt(max(0, det(Sigma2d) / det(Sigma2d + 0.3 I))) before anything looks at it, so an antialiased render of
(..., raw) IS the ordinary render of (..., raw' = logit(sigmoid(raw) * rho)). Every value test here rests on that identity, with rho from the float64 host model
tests/fastgs_aa_reference.py (independent of the code under test): the forward against the default mode AND the CPU oracle at raw'; the backward against the chain
rule composed from the default mode's backward at raw' (itself held to the float64 oracle) and the model's J_rho. Tolerances are the ones tests/test_gpu_fastgs.py
holds this rasterizer to."""
import contextlib
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from fastgs_aa_reference import rho64, rho_vjp
from fastgs_raw import preprocess_raw as _preprocess_raw, render_and_backward_raw as _render_and_backward_raw
from gpu_util import n, noise_check, rel_l2, rows_check, t
from test_oracle_fastgs import _scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
MIN_ALPHA = 1.0 / 255.0
CFGS = [dict(N=3000, W=160, H=112, seed=0, deg=3), dict(N=1500, W=64, H=64, seed=2, deg=1, spread=0.4),
        dict(N=257, W=48, H=32, seed=4, deg=0, spread=0.3)]   # the last: one primitive past a 256-thread workgroup
KEYS = ("means", "scales_raw", "rot_raw", "opac_raw", "sh0", "sh_rest", "w2c")
GRADS = ("means", "scales_raw", "rot_raw", "opac_raw", "sh0", "sh_rest")


def _settings(sc, antialiased=False):
    from lichtfeld_studio_amd.fastgs import FastGSSettings
    return FastGSSettings(t(sc["cam_pos"]), sc["active_sh_bases"], sc["W"], sc["H"], sc["fx"], sc["fy"], sc["cx"], sc["cy"], 0.01, 1e10, antialiased)


def _dev(sc):
    return [t(sc[k]) for k in KEYS]


def _geom(sc):
    return (sc["means"], sc["scales_raw"], sc["rot_raw"], sc["w2c"], sc["fx"], sc["fy"], sc["cx"], sc["cy"], sc["W"], sc["H"])


def _sigmoid32(raw):
    """sigmoid in float64 of the float32 logit the device sees"""
    return 1.0 / (1.0 + np.exp(-np.asarray(raw, np.float32).astype(np.float64)))


def _compensated(sc):
    """-> (rho64, the scene with raw' = logit(sigmoid(raw) * rho64); -30 where rho64 = 0)"""
    rho = rho64(*_geom(sc))
    o = _sigmoid32(sc["opac_raw"]) * rho
    with np.errstate(divide="ignore"):
        raw2 = np.where(rho > 0, np.log(o) - np.log1p(-o), -30.0)
    return rho, dict(sc, opac_raw=raw2)


@functools.lru_cache(maxsize=None)
def _case(idx):
    """(scene, rho64, compensated scene) of configuration idx: computed once, never modified"""
    sc = _scene(**CFGS[idx])
    rho, sc2 = _compensated(sc)
    return sc, rho, sc2


def _oracle_fwd(o, sc, dtype):
    return o.fastgs_forward(sc["means"], sc["scales_raw"], sc["rot_raw"], sc["opac_raw"], sc["sh0"], sc["sh_rest"], sc["w2c"], sc["cam_pos"],
                            sc["active_sh_bases"], sc["W"], sc["H"], sc["fx"], sc["fy"], sc["cx"], sc["cy"], dtype=dtype)


@contextlib.contextmanager
def _deterministic(lfs):
    """debug bit 4: the blending backward accumulates with integer atomics, the same bits on every run (set BEFORE the forward: the workspace carries the rows)"""
    lib = lfs.load_library()
    lib.lfs_set_debug_flags(16)
    try:
        yield lib
    finally:
        lib.lfs_set_debug_flags(0)


def _upstream(sc, seed=5):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((3, sc["H"], sc["W"])).astype(np.float32), rng.standard_normal((1, sc["H"], sc["W"])).astype(np.float32)


def _fwd_bwd(sc, antialiased, dens=True, grad_w2c=None):
    """forward + backward of the Python mirror -> (image, alpha, n_instances, six gradients, densification_info, primitive workspace)"""
    from lichtfeld_studio_amd import fastgs
    s, a = _settings(sc, antialiased), _dev(sc)
    image, alpha, pws, iws, n_inst = fastgs.forward_wrapper(*a, s)
    gi, ga = _upstream(sc)
    d = torch.zeros(2, len(sc["means"]), device=DEV) if dens else None
    g = fastgs.backward_wrapper(d, t(gi), t(ga), image, alpha, a[0], a[1], a[2], a[4], a[5], pws, iws, a[6], s, n_inst, grad_w2c=grad_w2c)
    return image, alpha, n_inst, g, d, pws


def _n_touched(pws, N):
    """the n_touched array of a primitive workspace (csrc/lfs_fastgs.cuh: rec 64 B, mean2d 8 B, conic_opacity 16 B, bounds 8 B per primitive, each block 256-aligned)"""
    al = lambda v: (v + 255) & ~255
    off = al(64 * N) + al(8 * N) + al(16 * N) + al(8 * N)
    return pws[off:off + 4 * N].cpu().numpy().view(np.uint32)


def _image_bounds(label, a, b):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    print(f"{label}: mean |diff| {d.mean():.3e} (<= 2e-6), beyond 1/255 + 1e-4: {(d > 1 / 255 + 1e-4).mean():.2e} (<= 1e-3), max {d.max():.3e}")
    assert d.mean() <= 2e-6 and (d > 1 / 255 + 1e-4).mean() <= 1e-3, (label, d.mean(), d.max())


# ---- 1. forward = the ordinary forward at the compensated opacity -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(CFGS)), ids=lambda i: f"N{CFGS[i]['N']}")
def test_antialiased_forward_is_the_default_forward_at_the_compensated_opacity(lfs, oracle_mod, idx):
    from lichtfeld_studio_amd import fastgs
    sc, rho, sc2 = _case(idx)
    frac = float((rho < 0.9).mean())
    print(f"rho64 percentiles 5/50/95: {np.percentile(rho, [5, 50, 95])}, share below 0.9: {frac:.3f}")
    assert frac > 0.10, "the scene does not exercise the mode"
    assert np.abs(sc2["opac_raw"] - sc["opac_raw"]).max() > 0.1      # (an implementation that ignores the flag renders raw, not raw')
    img_a, al_a, _, _, n_a = fastgs.forward_wrapper(*_dev(sc), _settings(sc, True))
    img_d, al_d, _, _, n_d = fastgs.forward_wrapper(*_dev(sc2), _settings(sc2, False))
    _image_bounds("antialiased vs default at raw': image", n(img_a), n(img_d))
    _image_bounds("antialiased vs default at raw': alpha", n(al_a), n(al_d))
    print(f"n_instances antialiased {n_a}, default at raw' {n_d}")
    assert abs(n_a - n_d) <= 3 and n_a > 0        # a tile test can flip on the last bit of the power threshold
    f32 = _oracle_fwd(oracle_mod, sc2, np.float32)
    _image_bounds("antialiased vs oracle at raw': image", n(img_a), f32["image"])
    _image_bounds("antialiased vs oracle at raw': alpha", n(al_a)[0], f32["alpha"])
    assert abs(n_a - len(f32["ids"])) <= 3 and f32["alpha"].max() > 0.3
    img_0 = fastgs.forward_wrapper(*_dev(sc), _settings(sc, False))[0]
    assert float((img_0 - img_a).abs().max()) > 1e-2                  # the mode changes the picture


# ---- 2. backward = the chain rule over the default backward at raw' ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _expected_grads(idx):
    """(default-mode result at raw' on the device, expected antialiased gradients in float64). Needs the deterministic mode set by the caller."""
    sc, rho, sc2 = _case(idx)
    ref = _fwd_bwd(sc2, False)
    g2 = [n(x).astype(np.float64) for x in ref[3]]
    N = len(rho)
    o2 = _sigmoid32(sc2["opac_raw"])
    A = g2[3].reshape(N) / (1.0 - o2)                                  # sum alpha dL/dalpha = o_eff dL/do_eff
    vis = (rho > 0) & (A != 0)
    jm, js, jq = rho_vjp(np.where(vis, A / np.where(vis, rho, 1.0), 0.0), *_geom(sc))
    exp = [g2[0] + jm, g2[1] + js, g2[2] + jq, (A * (1.0 - _sigmoid32(sc["opac_raw"]))).reshape(N, 1), g2[4], g2[5]]
    assert np.abs(jm).max() > 1e-3 * np.abs(g2[0]).max() and np.abs(js).max() > 1e-3 * np.abs(g2[1]).max()   # the rho term is not lost in the bound
    return ref, exp


def _rows(label, a, b, N):
    a, b = np.asarray(a, np.float64).reshape(N, -1), np.asarray(b, np.float64).reshape(N, -1)
    assert np.isfinite(a).all(), label
    if np.abs(b).max() == 0:
        assert np.abs(a).max() == 0, label
        return
    e, flips, rest = rows_check(a, b, bar=5e-4, max_flips=3)
    print(f"{label}: rel-L2 {e:.2e}, flip rows {flips}, without them {rest:.2e} (< 5e-4)")
    assert rest < 5e-4, (label, e, flips, rest)


@pytest.mark.parametrize("idx", range(len(CFGS)), ids=lambda i: f"N{CFGS[i]['N']}")
def test_antialiased_backward_is_the_composition(lfs, oracle_mod, idx):
    sc, rho, sc2 = _case(idx)
    N = len(rho)
    with _deterministic(lfs):
        ref, exp = _expected_grads(idx)
        got = _fwd_bwd(sc, True)
    for name, a, b in zip(GRADS, got[3], exp):
        _rows(f"antialiased bwd {name} vs composition", n(a), b, N)
    # densification_info keeps its definition (dL/dmean2d only): the default mode's at raw'. Visibility can differ where n_instances can (a tile test on the last
    # bit of the power threshold, <= 3 instances); the norms are held as tests/test_gpu_fastgs.py holds them
    da, dd = n(got[4]), n(ref[4])
    assert int((da[0] != dd[0]).sum()) <= 3 and da[0].sum() > 0
    e, flips, rest = rows_check(da[1][:, None], dd[1][:, None], bar=1e-3, max_flips=3)
    assert rest < 1e-3, (e, flips, rest)
    # the anchor: the default-mode backward at raw' against the float64 oracle, as tests/test_gpu_fastgs.py does
    gi, ga = _upstream(sc)
    f64 = _oracle_fwd(oracle_mod, sc2, np.float64)
    og = oracle_mod.fastgs_backward(f64, sc2["means"], sc2["scales_raw"], sc2["rot_raw"], sc2["opac_raw"], sc2["sh0"], sc2["sh_rest"], sc2["w2c"], sc2["cam_pos"],
                                    sc2["active_sh_bases"], sc2["W"], sc2["H"], sc2["fx"], sc2["fy"], sc2["cx"], sc2["cy"], gi, ga, dtype=np.float64)
    for name, a, b in list(zip(GRADS, ref[3], og[:6]))[:4]:
        _rows(f"default bwd at raw' {name} vs oracle", n(a), b, N)


# ---- 3. the cuts ---------------------------------------------------------------------------------------------------------------------------------------------
def _quat_of(R):
    """wxyz of a rotation matrix with trace > -1"""
    w = 0.5 * np.sqrt(1.0 + np.trace(R))
    return np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])


def _scene_with_cut_cases():
    """the default small scene + four primitives (indices N0 .. N0+3): an edge-on disk, one just below and one just above the o_eff cut, one below the sigmoid cut"""
    sc = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in _scene().items()}
    N0 = len(sc["means"])
    Rc, tc = sc["w2c"][:3, :3], sc["w2c"][:3, 3]
    world = lambda p: Rc.T @ (np.asarray(p, np.float64) - tc)
    add = lambda k, rows: np.concatenate([sc[k], np.asarray(rows, np.float64).reshape((len(rows),) + sc[k].shape[1:])])
    centre, inside = world([0.0, 0.0, 4.0]), world([0.3, 0.3, 4.0])   # `inside` projects to (45.6, 37.4): the interior of tile (2, 2)
    sc["means"] = add("means", [centre, inside, inside, inside])
    # disk: local axis 0 (scale e^-12) = the camera's x axis, perpendicular to the view ray through the image centre; the other two axes span the ray and camera y
    sc["scales_raw"] = add("scales_raw", [[-12.0, np.log(0.2), np.log(0.2)]] + [[np.log(0.02)] * 3] * 3)
    sc["rot_raw"] = add("rot_raw", [_quat_of(Rc.T)] + [[1.0, 0.0, 0.0, 0.0]] * 3)
    sc["sh0"] = add("sh0", np.full((4, 1, 3), 0.5))
    sc["sh_rest"] = add("sh_rest", np.zeros((4, 15, 3)))
    sc["opac_raw"] = add("opac_raw", [2.0, 0.0, 0.0, -6.0])
    rho = rho64(*_geom(sc))
    cut = np.log(MIN_ALPHA / rho[N0 + 1]) - np.log1p(-MIN_ALPHA / rho[N0 + 1])     # sigmoid(cut) * rho64 = 1/255
    sc["opac_raw"][N0 + 1], sc["opac_raw"][N0 + 2] = cut - 1e-2, cut + 1e-2
    return sc, rho, N0


def test_antialiased_cuts(lfs):
    sc, rho, N0 = _scene_with_cut_cases()
    disk, below, above, faint = N0, N0 + 1, N0 + 2, N0 + 3
    N = len(rho)
    assert rho[disk] < 1e-3 and 0.1 < rho[below] < 0.9 and (rho < 0.9).mean() > 0.10
    sig = _sigmoid32(sc["opac_raw"])
    assert sig[below] > MIN_ALPHA and sig[below] * rho[below] < MIN_ALPHA < sig[above] * rho[above] and sig[faint] < MIN_ALPHA
    aa, de = _fwd_bwd(sc, True), _fwd_bwd(sc, False)
    nt_a, nt_d = _n_touched(aa[5], N), _n_touched(de[5], N)
    for i in (disk, below, faint):
        assert nt_a[i] == 0 and n(aa[4])[0, i] == 0, i
        for g in aa[3]:
            row = n(g)[i]
            assert np.isfinite(row).all() and (row == 0).all(), i
    assert nt_a[above] > 0 and n(aa[4])[0, above] == 1
    assert nt_d[disk] > 0 and nt_d[below] > 0 and nt_d[faint] == 0    # the default mode draws the disk: a 0.3 px^2 wide line at full opacity - what the mode exists for
    for g in aa[3]:
        assert bool(torch.isfinite(g).all())


# ---- 4. the default mode is untouched ---------------------------------------------------------------------------------------------------------------------------
def _same_bits(x, y):
    assert x[2] == y[2] and torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
    for p, q in zip(x[3], y[3]):
        assert torch.equal(p, q)
    assert torch.equal(x[4], y[4])


def test_default_mode_is_untouched(lfs):
    from lichtfeld_studio_amd import fastgs
    sc = _case(0)[0]
    with _deterministic(lfs) as lib:
        a, s = _dev(sc), _settings(sc)
        gi, ga = [t(x) for x in _upstream(sc)]
        rc0, pws0, n0 = _preprocess_raw(lib, a, s, 0)      # (two independent calls: the flag-less entry point this compared against is flags = 0 of the one entry)
        rc1, pws1, n1 = _preprocess_raw(lib, a, s, 0)
        assert rc0 == 0 and rc1 == 0
        base, ex = _render_and_backward_raw(lib, a, s, pws0, n0, gi, ga), _render_and_backward_raw(lib, a, s, pws1, n1, gi, ga)
        _same_bits(base, ex)
        assert float(base[3][0].abs().max()) > 0
        # a workspace last used antialiased: the next default-mode preprocess rewrites the mode word, the backward is the default one
        rc2, pws2, n2 = _preprocess_raw(lib, a, s, 1)
        aa = _render_and_backward_raw(lib, a, s, pws2, n2, gi, ga)
        assert rc2 == 0 and not torch.equal(aa[3][1], base[3][1]) and not torch.equal(aa[0], base[0])
        rc3, _, n3 = _preprocess_raw(lib, a, s, 0, pws=pws2)
        assert rc3 == 0
        _same_bits(base, _render_and_backward_raw(lib, a, s, pws2, n3, gi, ga))
    lib = lfs.load_library()
    # the workspace size is the parent commit's: rec 192000 + mean2d 24064 + conic 48128 + bounds 24064 + n_touched 12032 + depth 12032 + 3 x 512 (70 tiles) + 256 +
    # n_contrib 71680 + acc 192000
    assert lib.lfs_fastgs_primitive_workspace_bytes(C.c_uint32(3000), C.c_uint32(160), C.c_uint32(112)) == 577792
    # an unknown flag: LFS_E_INVALID before any launch, nothing written
    a, s = _dev(sc), _settings(sc)
    pws = torch.full((lib.lfs_fastgs_primitive_workspace_bytes(C.c_uint32(3000), C.c_uint32(160), C.c_uint32(112)),), 0xA5, dtype=torch.uint8, device=DEV)
    n_dev = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    for flags in (2, 3, 0x80000000):
        rc, _, _ = _preprocess_raw(lib, a, s, flags, pws=pws, n_dev=n_dev)
        torch.cuda.synchronize()
        assert rc == -1 and int(n_dev.item()) == -7 and bool((pws == 0xA5).all())
    # N = 0 and N = 1 in both modes
    for N in (0, 1):
        for aa_mode in (False, True):
            cut = dict(sc, **{k: sc[k][:N] for k in KEYS[:6]})
            out = _fwd_bwd(cut, aa_mode, grad_w2c=torch.full((4, 4), NAN, device=DEV) if N else None)
            assert bool(torch.isfinite(out[0]).all()) and bool(torch.isfinite(out[1]).all()) and (N > 0 or (out[2] == 0 and float(out[0].abs().max()) == 0))
            for g in out[3]:
                assert g.shape[0] == N and bool(torch.isfinite(g).all())


# ---- 5. pose gradient -----------------------------------------------------------------------------------------------------------------------------------------
def test_antialiased_pose_gradient(lfs):
    from test_gpu_fastgs_w2c import _expected
    idx = 2                                                            # SH degree 0: grad_means = R^T dcam exactly
    sc, rho, _ = _case(idx)
    N = len(rho)
    with _deterministic(lfs):
        _, exp = _expected_grads(idx)
        gw1, gw2 = torch.full((4, 4), NAN, device=DEV), torch.full((4, 4), NAN, device=DEV)
        r1, r2 = _fwd_bwd(sc, True, grad_w2c=gw1), _fwd_bwd(sc, True, grad_w2c=gw2)
    assert torch.equal(gw1, gw2) and all(torch.equal(p, q) for p, q in zip(r1[3], r2[3]))     # the same bits on two runs
    gm = n(r1[3][0])
    _rows("antialiased w2c entry: grad_means vs composition", gm, exp[0], N)
    E, M = _expected(sc, gm)
    out = n(gw1).astype(np.float64)
    err = float(np.abs(out[:3] - E).max())
    print(f"antialiased grad_w2c identity: max |grad_w2c - E| {err:.3e}, bound 1e-5 M = {1e-5 * M:.3e}")
    assert np.isfinite(out).all() and (out[3] == 0).all() and M > 0 and err <= 1e-5 * M


# ---- 6. the routes agree ----------------------------------------------------------------------------------------------------------------------------------------
def test_libtorch_route_matches_the_ctypes_route_bit_for_bit(lfs):
    from lichtfeld_studio_amd import _lfs_torch_ops as m
    from lichtfeld_studio_amd import fastgs
    sc = _case(1)[0]
    a, cam = _dev(sc), t(sc["cam_pos"])
    fr = (sc["active_sh_bases"], sc["W"], sc["H"], sc["fx"], sc["fy"], sc["cx"], sc["cy"], 0.01, 1e10)
    gi, ga = [t(x) for x in _upstream(sc)]
    none = torch.empty(0, device=DEV)
    with _deterministic(lfs):
        image, alpha, _, prim, inst, n_inst = m.fastgs_forward(*a, cam, *fr, antialiased=True)
        g1 = m.fastgs_backward_wrapper(none, gi, ga, image, alpha, a[0], a[1], a[2], a[5], prim, none, inst, none, a[6], cam, *fr, 0, n_inst, 0, 0, 0)
        s = fastgs.FastGSSettings(cam, *fr, True)
        img2, al2, pws, iws, n2 = fastgs.forward_wrapper(*a, s)
        g2 = fastgs.backward_wrapper(None, gi, ga, img2, al2, a[0], a[1], a[2], a[4], a[5], pws, iws, a[6], s, n2)
        img0 = m.fastgs_forward(*a, cam, *fr, antialiased=False)[0]
        img_ref = m.fastgs_forward_wrapper(*a, cam, *fr)[0]
    assert n_inst == n2 and torch.equal(image, img2) and torch.equal(alpha, al2)
    for p, q in zip(g1[:6], g2):
        assert torch.equal(p.reshape(q.shape), q)
    assert torch.equal(img0, img_ref) and not torch.equal(img0, image)


def test_antialiased_inline_shN_adam_matches_separate_optimizer(lfs):
    """tests/test_gpu_fastgs.py::test_fastgs_inline_shN_adam_matches_separate_optimizer with antialiasing=True: the optimizer-fused backward reads the mode from the
    workspace like every other form of lfs_fastgs_view_backward."""
    from gpu_util import noise_allclose
    from lichtfeld_studio_amd import scenes
    from lichtfeld_studio_amd.trainer import GutTrainer
    dev = torch.device(DEV)
    sc = scenes.syn_a(n=6000, sh_degree=3)
    target = scenes.target_image(sc.height, sc.width).to(dev)
    a, b = [GutTrainer(sc, dev, iterations=100, rasterizer="fastgs", antialiasing=True) for _ in range(2)]
    b.inline_shN_adam = False
    a.iteration = b.iteration = 998
    la = [float(a.train_step([target], views=[0])) for _ in range(12)]
    lb = [float(b.train_step([target], views=[0])) for _ in range(12)]
    noise_check("antialiased fastgs inline shN Adam: 12 losses", float(np.max(np.abs(np.array(la) - lb) / np.abs(lb))), 1e-4)
    assert la[-1] < la[0]
    moved = float((a.model.shN.detach() - sc.shN.to(dev)).abs().max())
    assert moved > 0 and float((a.model.shN - b.model.shN).detach().abs().max()) <= 0.05 * moved + 1e-6
    sa, sb = a.optimizer._state(a.model.shN), b.optimizer._state(b.model.shN)
    assert sa["step_count"] == sb["step_count"] == 12
    noise_allclose("antialiased fastgs inline shN exp_avg", sa["exp_avg"], sb["exp_avg"], rtol=1e-3, atol=1e-7)


# ---- 7. trainer and evaluation ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mse", "l1_ssim", "adc"])
def test_antialiased_trainer_step_matches_autograd(lfs, kind):
    """GutTrainer(antialiasing=True) against fast_rasterize(antialiased=True) + torch autograd: the bounds of test_fastgs_trainer_step_matches_autograd"""
    from lichtfeld_studio_amd import fastgs, losses, scenes
    from lichtfeld_studio_amd.trainer import GutTrainer
    dev = torch.device(DEV)
    sc = scenes.syn_a(n=4000, sh_degree=2)
    kw = dict(loss="l1_ssim") if kind == "l1_ssim" else dict(strategy="default") if kind == "adc" else {}
    tr = GutTrainer(sc, dev, iterations=100, rasterizer="fastgs", antialiasing=True, **kw)
    target = scenes.target_image(sc.height, sc.width).to(dev)
    ref = fastgs.fast_rasterize(tr.camera(0), tr.model, torch.zeros(3, device=dev), antialiased=True)
    plain = fastgs.fast_rasterize(tr.camera(0), tr.model, torch.zeros(3, device=dev))
    assert float((ref.image - plain.image).abs().max()) > 1e-3
    loss_ref = losses.photometric_loss(ref.image, target, tr.lambda_dssim) if kind == "l1_ssim" else torch.nn.functional.mse_loss(ref.image, target)
    loss_ref.backward()
    ref_grads = [p.grad.clone() for p in tr.model.parameters()]
    for p in tr.model.parameters():
        p.grad = None
    loss = tr.train_step([target], views=[0])
    print(f"{kind}: loss {float(loss):.8f}, autograd {float(loss_ref):.8f}")
    assert abs(float(loss) - float(loss_ref)) < 1e-6
    for name, g, r in zip(["means", "sh0", "shN", "raw_scales", "raw_quats", "raw_opacities"], tr.bucket.views, ref_grads):
        e = rel_l2(n(g), n(r).reshape(n(g).shape))
        print(f"{kind} {name}: rel-L2 {e:.2e} (< 1e-4)")
        assert e < 1e-4, name
    if kind == "adc":
        for _ in range(2):
            tr.train_step([target], views=[0])
        assert tr.densification_info is not None and float(tr.densification_info[0].sum()) > 0 and float(tr.densification_info[1].sum()) > 0


def test_antialiasing_off_is_the_old_trainer_and_gut_refuses(lfs):
    from lichtfeld_studio_amd import scenes
    from lichtfeld_studio_amd.trainer import GutTrainer
    dev = torch.device(DEV)
    sc = scenes.syn_a(n=4000, sh_degree=2)
    with pytest.raises(ValueError, match="not wired into the 3DGUT route"):
        GutTrainer(sc, dev, iterations=100, rasterizer="gut", antialiasing=True)
    target = scenes.target_image(sc.height, sc.width).to(dev)
    with _deterministic(lfs):
        a, b = GutTrainer(sc, dev, iterations=100, rasterizer="fastgs", antialiasing=False), GutTrainer(sc, dev, iterations=100, rasterizer="fastgs")
        for _ in range(5):
            a.train_step([target], views=[0]), b.train_step([target], views=[0])
        for p, q in zip(a.model.parameters(), b.model.parameters()):
            assert torch.equal(p, q)
        assert not a.antialiasing and not b.antialiasing and a.last_plan == b.last_plan


def test_evaluate_antialiased(lfs):
    """a model whose Gaussians are a quarter of their size (sub-pixel): against targets rendered antialiased, the PSNR with the flag is higher than without"""
    from lichtfeld_studio_amd import evaluate, fastgs, scenes
    from lichtfeld_studio_amd.rasterizer import Camera, SplatModel
    dev = torch.device(DEV)
    sc = scenes.syn_a(n=4000, sh_degree=2).to(dev)
    model = SplatModel(sc.means, sc.sh0, sc.shN, sc.raw_scales - float(np.log(4.0)), sc.raw_quats, sc.raw_opacities, 2)
    cams = [Camera(sc.viewmats[v:v + 1].contiguous(), sc.Ks[v:v + 1].contiguous(), sc.width, sc.height) for v in range(min(2, sc.viewmats.shape[0]))]
    with torch.no_grad():
        targets = [torch.clamp(fastgs.fast_rasterize(c, model, torch.zeros(3, device=dev), antialiased=True).image, 0, 1) for c in cams]
    on, off = evaluate.evaluate(model, cams, targets, antialiased=True), evaluate.evaluate(model, cams, targets)
    print(f"PSNR with the flag {on.psnr:.2f} dB, without {off.psnr:.2f} dB")
    assert on.psnr > off.psnr
    with pytest.raises(ValueError, match="fastgs rasterizer only"):
        evaluate.evaluate(model, cams, targets, rasterizer="gut", antialiased=True)


# ---- 8. tools/train_colmap.py --antialiasing ---------------------------------------------------------------------------------------------------------------------------
def test_train_colmap_tool_antialiasing(lfs, tmp_path):
    import json
    from test_gpu_dataprep import _synthetic_colmap
    base = _synthetic_colmap(str(tmp_path), n_views=8)[0]
    out = str(tmp_path / "run")
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "train_colmap.py")
    r = subprocess.run([sys.executable, tool, "-d", base, "-i", "30", "--strategy", "default", "--eval", "--test-every", "4", "--sh-degree", "1", "-o", out, "--antialiasing"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["antialiasing"] is True and res["rasterizer"] == "fastgs" and os.path.exists(res["ply"]) and res["iterations"] == 30 and np.isfinite(res["psnr"])
    r = subprocess.run([sys.executable, tool, "-d", base, "-i", "30", "-o", out, "--antialiasing", "--gut"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--antialiasing is not wired into the 3DGUT route" in r.stderr
