"""GPU: the 3D smoothing filter of the fastgs (EWA) rasterizer (lfs_filter3d_compute, lfs_fastgs_view_preprocess_ex / _backward_ex).

With v the per-Gaussian filter variance, the filtered modes use s' = sqrt(s^2 + v) and o' = sigmoid(raw) prod s / s' wherever the default mode uses exp(raw_scale) and
sigmoid(raw), so a filtered render of (raw_scales, raw, v) IS the default render of the baked parameters (log s', logit o'), and the backward is the chain rule
over the default backward there. Every value test rests on that identity, with v, s', o' and the chain rule from the float64 host model
tests/fastgs_filter3d_reference.py (independent of the code under test). Scenes, bounds and helpers are those of tests/test_gpu_fastgs_antialiased.py."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fastgs_filter3d_reference as ref
import test_gpu_fastgs_antialiased as aa
from fastgs_raw import instance_workspace, render_raw, view_of
from gpu_util import n, rel_l2, rows_check, t
from test_oracle_fastgs import _scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
MIN_ALPHA = 1.0 / 255.0
CFGS, KEYS, GRADS = aa.CFGS, aa.KEYS, aa.GRADS


def _settings(sc, antialiased=False, depth="none", v=None):
    from lichtfeld_studio_amd.fastgs import FastGSSettings
    return FastGSSettings(t(sc["cam_pos"]), sc["active_sh_bases"], sc["W"], sc["H"], sc["fx"], sc["fy"], sc["cx"], sc["cy"], 0.01, 1e10, antialiased, depth,
                          None if v is None else t(v))


@functools.lru_cache(maxsize=None)
def _case(idx):
    """(scene, v float32 from the host model at the scene's own camera, baked scene, kappa, u) of configuration idx: computed once, never modified"""
    sc = _scene(**CFGS[idx])
    v = ref.filter_var64(sc["means"], [ref.camera_of_scene(sc)]).astype(np.float32)
    sc2, kappa, u = ref.baked_scene(sc, v)
    return sc, v, sc2, kappa, u


def _fwd_bwd(sc, antialiased=False, v=None, dens=True, grad_w2c=None, depth="none", grad_depth=None):
    """forward + backward of the Python mirror -> (image, alpha, n_instances, six gradients, densification_info, primitive workspace, depth plane)"""
    from lichtfeld_studio_amd import fastgs
    s, a = _settings(sc, antialiased, depth, v), aa._dev(sc)
    plane = None
    if depth != "none":
        image, alpha, plane, pws, iws, n_inst = fastgs.forward_wrapper_depth(*a, s)
    else:
        image, alpha, pws, iws, n_inst = fastgs.forward_wrapper(*a, s)
    gi, ga = aa._upstream(sc)
    d = torch.zeros(2, len(sc["means"]), device=DEV) if dens else None
    g = fastgs.backward_wrapper(d, t(gi), t(ga), image, alpha, a[0], a[1], a[2], a[4], a[5], pws, iws, a[6], s, n_inst, grad_w2c=grad_w2c,
                                grad_depth=None if grad_depth is None else t(grad_depth))
    return image, alpha, n_inst, g, d, pws, plane


# ---- 1. lfs_filter3d_compute against the host model -------------------------------------------------------------------------------------------------------------
CTR = np.array([0.0, 0.0, 4.0])


@functools.lru_cache(maxsize=None)
def _camera_set():
    """six cameras on a ring around CTR looking at it, each with its own focal length and image size, and a seventh at camera 0's place looking the other way"""
    cams = []
    for k in range(6):
        a = 2 * np.pi * k / 6
        eye = CTR + np.array([2 * np.sin(a), 0.3 * np.cos(2 * a), -2 * np.cos(a)])
        W, H, fx = 64 + 8 * k, 48, 60.0 + 15 * k
        cams.append(dict(w2c=ref.look_at(eye, CTR), fx=fx, fy=1.1 * fx, cx=W / 2, cy=H / 2, W=W, H=H))
    eye0 = CTR + np.array([0.0, 0.3, -2.0])
    cams.append(dict(w2c=ref.look_at(eye0, 2 * eye0 - CTR), fx=60.0, fy=66.0, cx=32.0, cy=24.0, W=64, H=48))
    return cams


@functools.lru_cache(maxsize=None)
def _points():
    """the means of _scene(N=3000, W=160, H=112, seed=0), with every point that lies within 1e-4 (relative) of a boundary of some camera's 'seen' test moved off it"""
    means = np.asarray(_scene(N=3000, W=160, H=112, seed=0)["means"], np.float32).astype(np.float64)
    cams = _camera_set()
    for _ in range(8):
        close = np.zeros(len(means), bool)
        for c in cams:
            close |= ref.boundary_distance(means, c) < 1e-4
        if not close.any():
            break
        means[close] += 3e-3
        means = means.astype(np.float32).astype(np.float64)
    for c in cams:
        assert (ref.boundary_distance(means, c) >= 1e-4).all()
    return means


def _packed(cams):
    from lichtfeld_studio_amd import filter3d
    if not cams:
        return torch.zeros((0, filter3d.CAMERA_DWORDS), dtype=torch.int32, device=DEV)
    vm = torch.as_tensor(np.stack([c["w2c"] for c in cams]), dtype=torch.float32)
    Ks = torch.as_tensor(np.stack([[[c["fx"], 0, c["cx"]], [0, c["fy"], c["cy"]], [0, 0, 1]] for c in cams]), dtype=torch.float32)
    return filter3d.pack_cameras(viewmats=vm, Ks=Ks, width=[c["W"] for c in cams], height=[c["H"] for c in cams], device=DEV)


def test_the_camera_set_exercises_the_kernel():
    """on the model alone: what the sizes below rely on"""
    means, cams = _points(), _camera_set()
    nu, arg, seen, z, _, _ = ref.nu64(means, cams)
    share = np.array([(arg == c).mean() for c in range(len(cams))])
    print(f"argmax shares {np.round(share, 3)}, unseen {(arg < 0).mean():.3f}, pairs with z <= 0.2: {(z <= 0.2).sum()}")
    assert (share[:6] >= 0.05).all() and share[6] == 0 and not seen[6].any()
    assert (arg < 0).mean() >= 0.01 and (z <= 0.2).any()


@pytest.mark.parametrize("C_", [0, 1, 7])
@pytest.mark.parametrize("N", [1, 255, 256, 257, 3000])
def test_filter3d_compute_matches_the_host_model(lfs, N, C_):
    from lichtfeld_studio_amd import filter3d
    means, cams = _points()[:N], _camera_set()[:C_]
    exp, tol = ref.filter_var64(means, cams), ref.filter_var_tolerance(means, cams)
    got = filter3d.compute_filter3d(t(means), _packed(cams))
    again = filter3d.compute_filter3d(t(means), _packed(cams))
    assert torch.equal(got, again)                                       # the same bits on two runs
    g = n(got).astype(np.float64)
    assert g.shape == (N,) and np.isfinite(g).all()
    if C_ == 0 or not (ref.nu64(means, cams)[0] > 0).any():
        assert (exp == 0).all() and (g == 0).all()
        return
    # identical seen sets: an unseen Gaussian takes exactly the minimum, a seen one a value of its own; every row within the derived bound
    ratio = np.abs(g - exp) / tol
    print(f"N {N} C {C_}: worst |v - v64| / bound {ratio.max():.3f}, v range [{exp.min():.3e}, {exp.max():.3e}]")
    assert (ratio <= 1.0).all(), (N, C_, ratio.max())
    unseen = ref.nu64(means, cams)[0] == 0
    assert (g[unseen] == g.max()).all() and (g > 0).all()


def test_filter3d_compute_edges(lfs):
    from lichtfeld_studio_amd import filter3d
    lib = lfs.load_library()
    # N = 0: LFS_OK without a launch - nothing is dereferenced
    assert lib.lfs_filter3d_compute(C.c_uint32(0), None, C.c_uint32(3), None, C.c_float(0.2), None, None, C.c_size_t(0), None) == 0
    assert filter3d.compute_filter3d(torch.zeros((0, 3), device=DEV), _packed(_camera_set())).shape == (0,)
    # every camera blind, and C = 0: zeros
    means = _points()[:257]
    assert float(filter3d.compute_filter3d(t(means), _packed(_camera_set()[6:])).abs().max()) == 0
    assert float(filter3d.compute_filter3d(t(means), _packed([])).abs().max()) == 0
    # argument checks: before any launch, the output keeps its fill
    m, cams = t(means), _packed(_camera_set())
    out = torch.full((257,), 7.0, device=DEV)
    ws = torch.zeros(256, dtype=torch.uint8, device=DEV)
    call = lambda mp, cp, op, c=7: lib.lfs_filter3d_compute(C.c_uint32(257), mp, C.c_uint32(c), cp, C.c_float(0.2), op, C.c_void_p(ws.data_ptr()), C.c_size_t(256), None)
    p = lambda x: C.c_void_p(x.data_ptr())
    assert call(p(m), p(cams), None) == -1 and call(p(m), None, p(out)) == -1 and call(None, p(cams), p(out)) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call(p(m), None, p(out), c=0) == 0                           # NULL cameras with C = 0 is the camera-less call
    torch.cuda.synchronize()
    assert bool((out == 0.0).all())


# ---- 2. forward = the default forward at the baked parameters -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(CFGS)), ids=lambda i: f"N{CFGS[i]['N']}")
def test_filtered_forward_is_the_default_forward_at_the_baked_parameters(lfs, oracle_mod, idx):
    from lichtfeld_studio_amd import fastgs
    sc, v, sc2, kappa, _ = _case(idx)
    frac = float((kappa < 0.9).mean())
    print(f"kappa percentiles 5/50/95: {np.percentile(kappa, [5, 50, 95])}, share below 0.9: {frac:.3f}")
    assert frac > 0.10, "the scene does not exercise the filter"
    img_f, al_f, _, _, n_f = fastgs.forward_wrapper(*aa._dev(sc), _settings(sc, v=v))
    img_d, al_d, _, _, n_d = fastgs.forward_wrapper(*aa._dev(sc2), _settings(sc2))
    aa._image_bounds("filtered vs default at the baked parameters: image", n(img_f), n(img_d))
    aa._image_bounds("filtered vs default at the baked parameters: alpha", n(al_f), n(al_d))
    print(f"n_instances filtered {n_f}, default at the baked parameters {n_d}")
    assert abs(n_f - n_d) <= 3 and n_f > 0
    f32 = aa._oracle_fwd(oracle_mod, sc2, np.float32)
    aa._image_bounds("filtered vs oracle at the baked parameters: image", n(img_f), f32["image"])
    aa._image_bounds("filtered vs oracle at the baked parameters: alpha", n(al_f)[0], f32["alpha"])
    assert abs(n_f - len(f32["ids"])) <= 3 and f32["alpha"].max() > 0.3
    img_0 = fastgs.forward_wrapper(*aa._dev(sc), _settings(sc))[0]
    assert float((img_0 - img_f).abs().max()) > 1e-2                  # the filter changes the picture


# ---- 3. backward = the chain rule over the default backward at the baked parameters ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _expected_grads(idx, antialiased=False):
    """(default-mode [or antialiased] result at the baked parameters on the device, expected filtered gradients in float64). Needs the deterministic mode set by the caller."""
    sc, v, sc2, _, _ = _case(idx)
    base = _fwd_bwd(sc2, antialiased)
    g2 = [n(x).astype(np.float64) for x in base[3]]
    N = len(v)
    gs, go, su = ref.chain64(g2[1], g2[3].reshape(N), sc, v)
    assert np.abs(su).max() > 1e-3 * np.abs(g2[1]).max()               # the S u term is not lost inside the bound
    return base, [g2[0], gs, g2[2], go.reshape(N, 1), g2[4], g2[5]]


def _check_dens(got, base):
    """densification_info keeps its definition (dL/dmean2d only): the default mode's at the baked parameters, held as tests/test_gpu_fastgs_antialiased.py holds it"""
    da, dd = n(got[4]), n(base[4])
    assert int((da[0] != dd[0]).sum()) <= 3 and da[0].sum() > 0
    e, flips, rest = rows_check(da[1][:, None], dd[1][:, None], bar=1e-3, max_flips=3)
    assert rest < 1e-3, (e, flips, rest)


@pytest.mark.parametrize("idx", range(len(CFGS)), ids=lambda i: f"N{CFGS[i]['N']}")
def test_filtered_backward_is_the_composition(lfs, idx):
    sc, v, _, _, _ = _case(idx)
    with aa._deterministic(lfs):
        base, exp = _expected_grads(idx)
        got = _fwd_bwd(sc, False, v)
    for name, a, b in zip(GRADS, got[3], exp):
        aa._rows(f"filtered bwd {name} vs composition", n(a), b, len(v))
    _check_dens(got, base)


# ---- 4. combinations ------------------------------------------------------------------------------------------------------------------------------------------------
def test_filter_with_antialiasing(lfs):
    idx = 1
    sc, v, sc2, _, _ = _case(idx)
    with aa._deterministic(lfs):
        base, exp = _expected_grads(idx, True)
        got = _fwd_bwd(sc, True, v)
    aa._image_bounds("filter + antialiased vs antialiased at the baked parameters: image", n(got[0]), n(base[0]))
    aa._image_bounds("filter + antialiased vs antialiased at the baked parameters: alpha", n(got[1]), n(base[1]))
    assert abs(got[2] - base[2]) <= 3
    for name, a, b in zip(GRADS, got[3], exp):
        aa._rows(f"filter + antialiased bwd {name} vs composition", n(a), b, len(v))
    _check_dens(got, base)
    plain = _fwd_bwd(sc, False, v)
    assert float((plain[0] - got[0]).abs().max()) > 1e-3               # both halves act


@pytest.mark.parametrize("kind", ["depth", "invdepth"])
def test_filter_with_depth(lfs, kind):
    idx = 1
    sc, v, sc2, _, _ = _case(idx)
    gd = np.random.default_rng(9).standard_normal((1, sc["H"], sc["W"])).astype(np.float32)
    with aa._deterministic(lfs):
        base = _fwd_bwd(sc2, False, None, depth=kind, grad_depth=gd)
        got = _fwd_bwd(sc, False, v, depth=kind, grad_depth=gd)
    # depth = sum_i w_i d_i: an error eps in the weights (what the image bounds allow) shows as eps * max d; max d over the primitives in front of the camera
    z = ref.project64(sc["means"], ref.camera_of_scene(sc))[2]
    dmax = float(z[z > 0.01].max()) if kind == "depth" else float(1.0 / z[z > 0.01].min())
    aa._image_bounds(f"filter + {kind}: depth plane / max d", n(got[6]) / dmax, n(base[6]) / dmax)
    assert torch.equal(got[0], _fwd_bwd(sc, False, v, dens=False)[0])  # image: the same bits with and without the depth plane
    N = len(v)
    g2 = [n(x).astype(np.float64) for x in base[3]]
    gs, go, _ = ref.chain64(g2[1], g2[3].reshape(N), sc, v)
    for name, a, b in zip(GRADS, got[3], [g2[0], gs, g2[2], go.reshape(N, 1), g2[4], g2[5]]):
        aa._rows(f"filter + {kind} bwd {name} vs composition", n(a), b, N)
    no_gd = _fwd_bwd(sc, False, v, depth=kind)
    assert not torch.equal(no_gd[3][0], got[3][0])                      # grad_depth reaches grad_means


def test_filtered_pose_gradient(lfs):
    from test_gpu_fastgs_w2c import _expected
    idx = 2                                                            # SH degree 0: grad_means = R^T dcam exactly
    sc, v, sc2, _, _ = _case(idx)
    N = len(v)
    with aa._deterministic(lfs):
        _, exp = _expected_grads(idx)
        gw1, gw2, gwb = [torch.full((4, 4), NAN, device=DEV) for _ in range(3)]
        r1, r2 = _fwd_bwd(sc, False, v, grad_w2c=gw1), _fwd_bwd(sc, False, v, grad_w2c=gw2)
        rb = _fwd_bwd(sc2, False, None, grad_w2c=gwb)
    assert torch.equal(gw1, gw2) and all(torch.equal(p, q) for p, q in zip(r1[3], r2[3]))     # the same bits on two runs
    gm = n(r1[3][0])
    aa._rows("filtered w2c entry: grad_means vs composition", gm, exp[0], N)
    E, M = _expected(sc, gm)
    out = n(gw1).astype(np.float64)
    err = float(np.abs(out[:3] - E).max())
    print(f"filtered grad_w2c identity: max |grad_w2c - E| {err:.3e}, bound 1e-5 M = {1e-5 * M:.3e}")
    assert np.isfinite(out).all() and (out[3] == 0).all() and M > 0 and err <= 1e-5 * M
    # ... and it is the camera gradient at the baked parameters: the rows of grad_means agree to 5e-4 in rel-L2 there (above), so by Cauchy-Schwarz the sums
    # sum_i d_i (x) (m_i, 1) differ by at most 5e-4 |grad_means|_F |(m, 1)|_F, plus the two identities' own 1e-5 M
    m1 = np.concatenate([np.asarray(sc["means"], np.float64), np.ones((N, 1))], 1)
    bound = 5e-4 * np.linalg.norm(n(rb[3][0]).astype(np.float64)) * np.linalg.norm(m1) + 2e-5 * M
    diff = float(np.abs(out - n(gwb).astype(np.float64)).max())
    print(f"filtered grad_w2c vs the baked parameters': max |diff| {diff:.3e}, bound {bound:.3e}")
    assert diff <= bound


def test_filtered_inline_shN_adam_matches_separate_optimizer(lfs):
    """tests/test_gpu_fastgs.py::test_fastgs_inline_shN_adam_matches_separate_optimizer with filter3d=True: the optimizer-fused backward (args->adam) takes the filter"""
    from gpu_util import noise_allclose, noise_check
    from lichtfeld_studio_amd import scenes
    from lichtfeld_studio_amd.trainer import GutTrainer
    dev = torch.device(DEV)
    sc = scenes.syn_a(n=6000, sh_degree=3)
    target = scenes.target_image(sc.height, sc.width).to(dev)
    a, b = [GutTrainer(sc, dev, iterations=100, rasterizer="fastgs", filter3d=True) for _ in range(2)]
    b.inline_shN_adam = False
    a.iteration = b.iteration = 998
    la = [float(a.train_step([target], views=[0])) for _ in range(12)]
    lb = [float(b.train_step([target], views=[0])) for _ in range(12)]
    noise_check("filtered fastgs inline shN Adam: 12 losses", float(np.max(np.abs(np.array(la) - lb) / np.abs(lb))), 1e-4)
    assert la[-1] < la[0] and a.filter3d_var is not None and float(a.filter3d_var.max()) > 0
    moved = float((a.model.shN.detach() - sc.shN.to(dev)).abs().max())
    assert moved > 0 and float((a.model.shN - b.model.shN).detach().abs().max()) <= 0.05 * moved + 1e-6
    sa, sb = a.optimizer._state(a.model.shN), b.optimizer._state(b.model.shN)
    assert sa["step_count"] == sb["step_count"] == 12
    noise_allclose("filtered fastgs inline shN exp_avg", sa["exp_avg"], sb["exp_avg"], rtol=1e-3, atol=1e-7)


# ---- 5. the cuts ----------------------------------------------------------------------------------------------------------------------------------------------------
def _scene_with_cut_cases():
    """the default small scene + three primitives (indices N0 .. N0+2): one just below and one just above the o' cut, one behind the camera whose v is NaN"""
    sc = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in _scene().items()}
    N0 = len(sc["means"])
    Rc, tc = sc["w2c"][:3, :3], sc["w2c"][:3, 3]
    world = lambda p: Rc.T @ (np.asarray(p, np.float64) - tc)
    add = lambda k, rows: np.concatenate([sc[k], np.asarray(rows, np.float64).reshape((len(rows),) + sc[k].shape[1:])])
    inside = world([0.3, 0.3, 4.0])                                    # projects into the interior of tile (2, 2)
    sc["means"] = add("means", [inside, inside, world([0.0, 0.0, -2.0])])
    sc["scales_raw"] = add("scales_raw", [[np.log(0.02)] * 3] * 3)
    sc["rot_raw"] = add("rot_raw", [[1.0, 0.0, 0.0, 0.0]] * 3)
    sc["sh0"] = add("sh0", np.full((3, 1, 3), 0.5))
    sc["sh_rest"] = add("sh_rest", np.zeros((3, 15, 3)))
    sc["opac_raw"] = add("opac_raw", [0.0, 0.0, 2.0])
    v = ref.filter_var64(sc["means"], [ref.camera_of_scene(sc)]).astype(np.float32)
    kappa = ref.effective64(sc["scales_raw"], sc["opac_raw"], v)[1]
    cut = np.log(MIN_ALPHA / kappa[N0]) - np.log1p(-MIN_ALPHA / kappa[N0])         # sigmoid(cut) * kappa = 1/255
    sc["opac_raw"][N0], sc["opac_raw"][N0 + 1] = cut - 1e-2, cut + 1e-2
    v[N0 + 2] = NAN
    return sc, v, kappa, N0


def test_filtered_cuts(lfs):
    sc, v, kappa, N0 = _scene_with_cut_cases()
    below, above, behind = N0, N0 + 1, N0 + 2
    N = len(v)
    sig = aa._sigmoid32(sc["opac_raw"])
    assert 0.1 < kappa[below] < 0.9 and sig[below] >= MIN_ALPHA and sig[below] * kappa[below] < MIN_ALPHA < sig[above] * kappa[above]
    fl, de = _fwd_bwd(sc, False, v), _fwd_bwd(sc, False, None)
    nt_f, nt_d = aa._n_touched(fl[5], N), aa._n_touched(de[5], N)
    for i in (below, behind):
        assert nt_f[i] == 0 and n(fl[4])[0, i] == 0, i
        for g in fl[3]:
            row = n(g)[i]
            assert np.isfinite(row).all() and (row == 0).all(), i
    assert nt_f[above] > 0 and n(fl[4])[0, above] == 1
    assert nt_d[below] > 0 and nt_d[behind] == 0                       # the default mode draws the one the filter cuts
    assert bool(torch.isfinite(fl[0]).all()) and all(bool(torch.isfinite(g).all()) for g in fl[3])
    # v = 0 rows behave as default rows: with v = 0 everywhere the filtered forms compute the default forms' values
    with aa._deterministic(lfs):
        zero, plain = _fwd_bwd(sc, False, np.zeros(N, np.float32)), _fwd_bwd(sc, False, None)
    assert zero[2] == plain[2] and torch.equal(zero[0], plain[0]) and torch.equal(zero[1], plain[1]) and torch.equal(zero[4], plain[4])
    for p, q in zip(zero[3], plain[3]):
        assert torch.equal(p, q)


# ---- 6. / 7. the entries: nothing else moved, and the argument checks -------------------------------------------------------------------------------------------------
def _ext(v):
    """(byref'able lfs_fastgs_view_ext or None, keep-alive) for: "old" (no ext argument exists), None (ext = NULL), "null" (ext->filter3d_var = NULL), a tensor"""
    from lichtfeld_studio_amd.capi import FastgsViewExt
    if v is None:
        return None
    return C.byref(FastgsViewExt(None if isinstance(v, str) else C.c_void_p(v.data_ptr())))


def _preprocess(lib, a, s, flags, how, pws=None):
    from lichtfeld_studio_amd.capi import ptr, stream
    N = a[0].shape[0]
    if pws is None:
        pws = torch.zeros(max(256, lib.lfs_fastgs_primitive_workspace_bytes(C.c_uint32(N), C.c_uint32(s.width), C.c_uint32(s.height))), dtype=torch.uint8, device=DEV)
    n_dev = torch.zeros(1, dtype=torch.int64, device=DEV)
    view = view_of(a, s, pws)
    if isinstance(how, str) and how == "old":
        rc = lib.lfs_fastgs_view_preprocess(C.byref(view), C.c_uint32(flags), ptr(n_dev), stream())
    else:
        rc = lib.lfs_fastgs_view_preprocess_ex(C.byref(view), C.c_uint32(flags), _ext(how), ptr(n_dev), stream())
    return rc, pws, n_dev


def _backward(lib, a, s, pws, iws, n_inst, gi, ga, alpha, grads, how, dens=None):
    from lichtfeld_studio_amd.capi import FastgsBackwardArgs, ptr, stream
    args = FastgsBackwardArgs(n_inst, ptr(iws), iws.numel(), ptr(gi), ptr(ga), ptr(alpha), None, ptr(dens), *[ptr(g) for g in grads], None, None, 0, None)
    view = view_of(a, s, pws)
    if isinstance(how, str) and how == "old":
        return lib.lfs_fastgs_view_backward(C.byref(view), C.byref(args), stream())
    return lib.lfs_fastgs_view_backward_ex(C.byref(view), C.byref(args), _ext(how), stream())


def _grad_buffers(sc, fill):
    N = len(sc["means"])
    return [torch.full(shape, fill, device=DEV) for shape in ((N, 3), (N, 3), (N, 4), (N, 1), (N, 1, 3), (N, 15, 3))]


def _run_entries(lib, sc, how, gi, ga):
    """preprocess, render and backward through one family of entries -> (rc's, image, alpha, n_instances, gradients, densification_info)"""
    a, s = aa._dev(sc), _settings(sc)
    rc0, pws, n_dev = _preprocess(lib, a, s, 0, how)
    n_inst = int(n_dev.item())
    iws = instance_workspace(lib, s, n_inst)
    image, alpha = torch.empty((3, s.height, s.width), device=DEV), torch.empty((1, s.height, s.width), device=DEV)
    rc1 = render_raw(lib, a, s, pws, n_inst, iws, image, alpha)
    grads, dens = _grad_buffers(sc, NAN), torch.zeros(2, len(sc["means"]), device=DEV)
    rc2 = _backward(lib, a, s, pws, iws, n_inst, gi, ga, alpha, grads, how, dens)
    return (rc0, rc1, rc2), image, alpha, n_inst, grads, dens


def test_the_old_entries_and_the_ex_entries_without_a_filter_agree_bit_for_bit(lfs):
    sc = _case(0)[0]
    gi, ga = [t(x) for x in aa._upstream(sc)]
    with aa._deterministic(lfs) as lib:
        old, null_ext, null_ptr = [_run_entries(lib, sc, how, gi, ga) for how in ("old", None, "null")]
    for other in (null_ext, null_ptr):
        assert old[0] == other[0] == (0, 0, 0) and old[3] == other[3] > 0
        assert torch.equal(old[1], other[1]) and torch.equal(old[2], other[2]) and torch.equal(old[5], other[5])
        for p, q in zip(old[4], other[4]):
            assert torch.equal(p, q) and bool(torch.isfinite(p).all())
    lib = lfs.load_library()
    assert lib.lfs_fastgs_primitive_workspace_bytes(C.c_uint32(3000), C.c_uint32(160), C.c_uint32(112)) == 577792      # the parent commit's
    # the public flags keep their set on the _ex entry too
    a, s = aa._dev(sc), _settings(sc)
    for flags in (2, 16, 1 << 16, 0x80000000):
        assert _preprocess(lib, a, s, flags, None)[0] == -1 and _preprocess(lib, a, s, flags, "old")[0] == -1


def test_a_backward_that_disagrees_with_the_forward_about_the_filter_is_refused(lfs):
    sc, v = _case(2)[0], _case(2)[1]
    lib = lfs.load_library()
    a, s, vt = aa._dev(sc), _settings(sc), t(_case(2)[1])
    gi, ga = [t(x) for x in aa._upstream(sc)]
    for fwd, bwds in ((vt, ("old", None, "null")), ("old", (vt,)), (None, (vt,))):
        rc, pws, n_dev = _preprocess(lib, a, s, 0, fwd)
        assert rc == 0
        n_inst = int(n_dev.item())
        iws = instance_workspace(lib, s, n_inst)
        image, alpha = torch.empty((3, s.height, s.width), device=DEV), torch.empty((1, s.height, s.width), device=DEV)
        assert render_raw(lib, a, s, pws, n_inst, iws, image, alpha) == 0
        for bwd in bwds:
            grads = _grad_buffers(sc, 7.0)
            assert _backward(lib, a, s, pws, iws, n_inst, gi, ga, alpha, grads, bwd) == -1
            torch.cuda.synchronize()
            assert all(bool((g == 7.0).all()) for g in grads)            # nothing was launched
        grads = _grad_buffers(sc, 7.0)                                     # the matching backward still runs on that workspace
        assert _backward(lib, a, s, pws, iws, n_inst, gi, ga, alpha, grads, fwd) == 0
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(g).all()) for g in grads) and not bool((grads[0] == 7.0).all())


# ---- 8. layers --------------------------------------------------------------------------------------------------------------------------------------------------------
def test_libtorch_route_matches_the_ctypes_route_bit_for_bit(lfs):
    from lichtfeld_studio_amd import _lfs_torch_ops as m
    from lichtfeld_studio_amd import fastgs
    sc, v = _case(1)[0], t(_case(1)[1])
    a, cam = aa._dev(sc), t(sc["cam_pos"])
    fr = (sc["active_sh_bases"], sc["W"], sc["H"], sc["fx"], sc["fy"], sc["cx"], sc["cy"], 0.01, 1e10)
    gi, ga = [t(x) for x in aa._upstream(sc)]
    none = torch.empty(0, device=DEV)
    with aa._deterministic(lfs):
        image, alpha, _, prim, inst, n_inst = m.fastgs_forward(*a, cam, *fr, antialiased=True, filter3d_var=v)
        g1 = m.fastgs_backward(none, gi, ga, None, alpha, a[0], a[1], a[2], a[5], prim, inst, a[6], cam, *fr, n_inst, filter3d_var=v)
        s = fastgs.FastGSSettings(cam, *fr, True, "none", v)
        img2, al2, pws, iws, n2 = fastgs.forward_wrapper(*a, s)
        g2 = fastgs.backward_wrapper(None, gi, ga, img2, al2, a[0], a[1], a[2], a[4], a[5], pws, iws, a[6], s, n2)
        img_aa = m.fastgs_forward(*a, cam, *fr, antialiased=True)[0]
    assert n_inst == n2 and torch.equal(image, img2) and torch.equal(alpha, al2)
    for p, q in zip(g1[:6], g2):
        assert torch.equal(p.reshape(q.shape), q)
    assert not torch.equal(img_aa, image)
    with pytest.raises(RuntimeError):                                      # the plain backward on a filtered workspace is refused
        m.fastgs_backward_wrapper(none, gi, ga, image, alpha, a[0], a[1], a[2], a[5], prim, none, inst, none, a[6], cam, *fr, 0, n_inst, 0, 0, 0)


@pytest.mark.parametrize("kind", ["mse", "mip_l1_ssim"])
def test_filtered_trainer_step_matches_autograd(lfs, kind):
    """GutTrainer(filter3d=True) against fast_rasterize(filter3d=) + torch autograd: the bounds of test_fastgs_trainer_step_matches_autograd"""
    from lichtfeld_studio_amd import fastgs, losses, scenes
    from lichtfeld_studio_amd.trainer import GutTrainer
    dev = torch.device(DEV)
    sc = scenes.syn_a(n=4000, sh_degree=2)
    mip = kind == "mip_l1_ssim"
    tr = GutTrainer(sc, dev, iterations=100, rasterizer="fastgs", filter3d=True, antialiasing=mip, **(dict(loss="l1_ssim") if mip else {}))
    target = scenes.target_image(sc.height, sc.width).to(dev)
    v = tr.update_filter3d()
    assert v.shape == (4000,) and float(v.min()) > 0 and tr.filter3d_computes == 1
    out = fastgs.fast_rasterize(tr.camera(0), tr.model, torch.zeros(3, device=dev), antialiased=mip, filter3d=v)
    plain = fastgs.fast_rasterize(tr.camera(0), tr.model, torch.zeros(3, device=dev), antialiased=mip)
    assert float((out.image - plain.image).detach().abs().max()) > 1e-3
    loss_ref = losses.photometric_loss(out.image, target, tr.lambda_dssim) if mip else torch.nn.functional.mse_loss(out.image, target)
    loss_ref.backward()
    ref_grads = [p.grad.clone() for p in tr.model.parameters()]
    for p in tr.model.parameters():
        p.grad = None
    loss = tr.train_step([target], views=[0])
    print(f"{kind}: loss {float(loss):.8f}, autograd {float(loss_ref):.8f}")
    assert abs(float(loss) - float(loss_ref)) < 1e-6 and tr.filter3d_computes == 1     # the step used the filter it already had
    for name, g, r in zip(["means", "sh0", "shN", "raw_scales", "raw_quats", "raw_opacities"], tr.bucket.views, ref_grads):
        e = rel_l2(n(g), n(r).reshape(n(g).shape))
        print(f"{kind} {name}: rel-L2 {e:.2e} (< 1e-4)")
        assert e < 1e-4, name


def test_filter3d_off_is_the_old_trainer_and_gut_refuses(lfs):
    from lichtfeld_studio_amd import scenes
    from lichtfeld_studio_amd.trainer import GutTrainer
    dev = torch.device(DEV)
    sc = scenes.syn_a(n=4000, sh_degree=2)
    with pytest.raises(ValueError, match="not wired into the 3DGUT route"):
        GutTrainer(sc, dev, iterations=100, rasterizer="gut", filter3d=True)
    target = scenes.target_image(sc.height, sc.width).to(dev)
    with aa._deterministic(lfs):
        a, b = GutTrainer(sc, dev, iterations=100, rasterizer="fastgs", filter3d=False), GutTrainer(sc, dev, iterations=100, rasterizer="fastgs")
        for _ in range(5):
            a.train_step([target], views=[0]), b.train_step([target], views=[0])
        for p, q in zip(a.model.parameters(), b.model.parameters()):
            assert torch.equal(p, q)
        assert a.filter3d_var is None and b.filter3d_var is None and a.filter3d_computes == 0 and a.last_plan == b.last_plan


def test_trainer_recomputes_the_filter_on_schedule_and_after_a_refinement(lfs):
    from lichtfeld_studio_amd import scenes, strategies
    from lichtfeld_studio_amd.trainer import GutTrainer
    dev = torch.device(DEV)
    sc = scenes.syn_a(n=1500, sh_degree=1)
    target = scenes.target_image(sc.height, sc.width).to(dev)
    # no strategy: exactly every filter3d_every steps (before steps 1, 5, 9)
    tr = GutTrainer(sc, dev, iterations=100, rasterizer="fastgs", filter3d=True, filter3d_every=4)
    counts = []
    for _ in range(9):
        tr.train_step([target], views=[0])
        counts.append(tr.filter3d_computes)
    assert counts == [1, 1, 1, 1, 2, 2, 2, 2, 3], counts
    # ADC: a refinement at iteration 6 (start_refine 3, refine_every 3) changes N; the step after it runs with a filter of the new N, computed anew
    op = strategies.OptimizationParameters.for_strategy("default", iterations=100)
    op.start_refine, op.refine_every, op.grad_threshold = 3, 3, 1e-9
    tr = GutTrainer(sc, dev, iterations=100, rasterizer="fastgs", strategy="default", opt_params=op, filter3d=True, filter3d_every=1000)
    seen = []
    for _ in range(8):
        tr.train_step([target], views=[0])
        seen.append((tr.iteration, int(tr.model.means.shape[0]), int(tr.filter3d_var.shape[0]), tr.filter3d_computes))
    print(seen)
    n_before, n_after = seen[4][1], seen[5][1]                            # iteration 6 refines
    assert n_after != n_before, "the refinement did not change the model: the test does not exercise the hook"
    assert seen[4][3] == 1 and seen[5][2] == n_before                    # the filter of step 6 was the old model's ...
    assert seen[6][2] == seen[6][1] == n_after and seen[6][3] == 2       # ... step 7 computed the new one's
    assert seen[7][3] == 2                                                # and nothing recomputes between refinements before filter3d_every


def test_evaluate_filter3d(lfs):
    """a model whose Gaussians are a quarter of their size (sub-pixel): against targets rendered with the filter, the PSNR with it is higher than without"""
    from lichtfeld_studio_amd import evaluate, fastgs, filter3d, scenes
    from lichtfeld_studio_amd.rasterizer import Camera, SplatModel
    dev = torch.device(DEV)
    sc = scenes.syn_a(n=4000, sh_degree=2).to(dev)
    model = SplatModel(sc.means, sc.sh0, sc.shN, sc.raw_scales - float(np.log(4.0)), sc.raw_quats, sc.raw_opacities, 2)
    cams = [Camera(sc.viewmats[v:v + 1].contiguous(), sc.Ks[v:v + 1].contiguous(), sc.width, sc.height) for v in range(min(2, sc.viewmats.shape[0]))]
    v = filter3d.compute_filter3d(model.means, cams)
    with torch.no_grad():
        targets = [torch.clamp(fastgs.fast_rasterize(c, model, torch.zeros(3, device=dev), filter3d=v).image, 0, 1) for c in cams]
        # the baked model renders the same picture without the operand
        rs, ro = filter3d.bake(model, v)
        baked = SplatModel(sc.means, sc.sh0, sc.shN, rs, sc.raw_quats, ro, 2)
        again = torch.clamp(fastgs.fast_rasterize(cams[0], baked, torch.zeros(3, device=dev)).image, 0, 1)
    aa._image_bounds("baked model vs filtered render", n(again), n(targets[0]))
    on, off = evaluate.evaluate(model, cams, targets, filter3d=v), evaluate.evaluate(model, cams, targets)
    print(f"PSNR with the filter {on.psnr:.2f} dB, without {off.psnr:.2f} dB")
    assert on.psnr > off.psnr
    with pytest.raises(ValueError, match="fastgs rasterizer only"):
        evaluate.evaluate(model, cams, targets, rasterizer="gut", filter3d=v)


def test_train_colmap_tool_mip_splatting(lfs, tmp_path):
    """--mip-splatting: trains and evaluates with both filters; the PLY it writes holds the baked scales and opacities of the model it also writes unfiltered"""
    from test_gpu_dataprep import _synthetic_colmap
    from lichtfeld_studio_amd import filter3d, loader
    base = _synthetic_colmap(str(tmp_path), n_views=8)[0]
    out = str(tmp_path / "run")
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "train_colmap.py")
    r = subprocess.run([sys.executable, tool, "-d", base, "-i", "12", "--strategy", "default", "--eval", "--test-every", "4", "--sh-degree", "1", "-o", out, "--mip-splatting",
                        "--filter3d-every", "5"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["antialiasing"] is True and res["filter3d"] is True and res["rasterizer"] == "fastgs" and res["iterations"] == 12 and np.isfinite(res["psnr"])
    baked, raw = loader.load_ply(res["ply"], device=DEV), loader.load_ply(res["ply_unfiltered"], device=DEV)
    scene = loader.colmap_scene(base, "images", split="train", test_every=4, sh_degree=1, init_scaling=1.0, init_opacity=0.1, device=DEV)[0]
    v = filter3d.compute_filter3d(raw.means, filter3d.pack_cameras(viewmats=scene.viewmats, Ks=scene.Ks, width=int(scene.width), height=int(scene.height), device=DEV))
    rs, ro = filter3d.bake(raw, v)
    assert float(v.min()) > 0 and torch.equal(baked.means, raw.means)
    assert float((baked.raw_scales - raw.raw_scales).abs().max()) > 1e-3      # the file is not the raw model
    assert float((baked.raw_scales - rs).abs().max()) <= 1e-6 * float(rs.abs().max()) + 1e-6
    assert float((baked.raw_opacities.reshape(-1) - ro.reshape(-1)).abs().max()) <= 1e-5
    r = subprocess.run([sys.executable, tool, "-d", base, "-i", "12", "-o", out, "--filter3d", "--gut"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--filter3d is not wired into the 3DGUT route" in r.stderr
