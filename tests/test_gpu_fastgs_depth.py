"""GPU: the depth modes of the fastgs (EWA) rasterizer (LFS_FASTGS_DEPTH / LFS_FASTGS_INVDEPTH, the depth plane of lfs_fastgs_view_render, grad_depth of lfs_fastgs_view_backward).

A depth render is a colour render whose colour is d_i (= z_i or 1 / z_i in camera space). Every value test here rests on that identity, with z_i from the float64
host model tests/fastgs_depth_reference.py (independent of the code under test): with s = max d_i, the degree-0 "twin" scene has red = d_i / s, and
  - the depth map / s is the twin's red channel from a render without a depth plane, and the float32 oracle's;
  - the depth-only backward (g_image = 0, g_alpha = 0, g_depth = G) is the twin's default backward with g_image = (G s, 0, 0), plus dL/dz_i = dL/dd_i dd/dz along
    w2c[2,:3] in grad_means and in row 2 of grad_w2c, with dL/dd_i = grad_sh0'[:,0,0] / C0 / s read off the twin.
Tolerances are the ones tests/test_gpu_fastgs.py, tests/test_gpu_fastgs_antialiased.py and tests/test_gpu_fastgs_w2c.py hold this rasterizer to.
All of it also runs on the wavefront emulator (tests/test_emulated_fastgs_depth.py), except the 3000-Gaussian case of the linearity test (reason there)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from fastgs_depth_reference import C0, d64, twin
from fastgs_raw import backward_raw, instance_workspace, render_raw
from gpu_util import n, rel_l2, rows_check, t
from test_gpu_fastgs_antialiased import (GRADS, KEYS, _compensated, _deterministic, _image_bounds, _oracle_fwd, _preprocess_raw, _render_and_backward_raw, _rows,
                                         _same_bits, _upstream)
from test_oracle_fastgs import _scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
# the three configurations of the antialiased tests + one whose size is no multiple of 8 or 16 (partial cells and tiles)
CFGS = [dict(N=3000, W=160, H=112, seed=0, deg=3), dict(N=1500, W=64, H=64, seed=2, deg=1, spread=0.4), dict(N=257, W=48, H=32, seed=4, deg=0, spread=0.3),
        dict(N=600, W=50, H=35, seed=6, deg=2)]
KINDS = ("depth", "invdepth")
IDS = lambda i: f"N{CFGS[i]['N']}"
LFS_FASTGS_DEPTH, LFS_FASTGS_INVDEPTH = 4, 8
INVALID = -1


def _settings(sc, antialiased=False, depth="none"):
    from lichtfeld_studio_amd.fastgs import FastGSSettings
    return FastGSSettings(t(sc["cam_pos"]), sc["active_sh_bases"], sc["W"], sc["H"], sc["fx"], sc["fy"], sc["cx"], sc["cy"], 0.01, 1e10, antialiased, depth)


def _dev(sc):
    return [t(sc[k]) for k in KEYS]


@functools.lru_cache(maxsize=None)
def _case(idx, kind):
    """(scene, twin scene, s, dd/dz in float64) of configuration idx: computed once, never modified"""
    sc = _scene(**CFGS[idx])
    tw, s = twin(sc, kind)
    return sc, tw, s, d64(sc["means"], sc["w2c"], kind)[1]


def _forward_depth(sc, kind, aa=False):
    """-> (image, alpha, depth, primitive workspace, instance workspace, n_instances, device arguments, settings)"""
    from lichtfeld_studio_amd import fastgs
    a, s = _dev(sc), _settings(sc, aa, kind)
    return (*fastgs.forward_wrapper_depth(*a, s), a, s)


def _forward_default(sc, aa=False):
    from lichtfeld_studio_amd import fastgs
    a, s = _dev(sc), _settings(sc, aa)
    image, alpha, pws, iws, n_inst = fastgs.forward_wrapper(*a, s)
    return image, alpha, None, pws, iws, n_inst, a, s


def _backward(st, gi, ga, gd=None, grad_w2c=None):
    """backward_wrapper on a forward state of _forward_depth / _forward_default -> (six gradients, densification_info)"""
    from lichtfeld_studio_amd import fastgs
    image, alpha, _, pws, iws, n_inst, a, s = st
    dens = torch.zeros(2, a[0].shape[0], device=DEV)
    g = fastgs.backward_wrapper(dens, gi, ga, image, alpha, a[0], a[1], a[2], a[4], a[5], pws, iws, a[6], s, n_inst, grad_w2c=grad_w2c, grad_depth=gd)
    return g, dens


def _g_depth(sc, seed=9):
    return np.random.default_rng(seed).standard_normal((1, sc["H"], sc["W"])).astype(np.float32)


def _zeros(sc):
    return torch.zeros(3, sc["H"], sc["W"], device=DEV), torch.zeros(1, sc["H"], sc["W"], device=DEV)


# ---- 1. forward: depth map / s = the twin's red channel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aa", [False, True], ids=["plain", "antialiased"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("idx", range(len(CFGS)), ids=IDS)
def test_depth_forward_is_the_colour_forward_of_the_twin(lfs, oracle_mod, idx, kind, aa):
    sc, tw, s, _ = _case(idx, kind)
    image, alpha, depth, _, _, n_inst, _, _ = _forward_depth(sc, kind, aa)
    ref = _forward_default(sc, aa)
    assert n_inst == ref[5] and n_inst > 0
    assert torch.equal(image, ref[0]) and torch.equal(alpha, ref[1])                       # colour and alpha: the default render bit for bit
    assert tuple(depth.shape) == (1, sc["H"], sc["W"]) and bool(torch.isfinite(depth).all())
    got = n(depth)[0].astype(np.float64) / s
    tw_img = _forward_default(tw, aa)[0]
    _image_bounds(f"{kind} map / s vs the twin's red channel (render without a depth plane)", got, n(tw_img)[0])
    f32 = _oracle_fwd(oracle_mod, _compensated(tw)[1] if aa else tw, np.float32)           # (the oracle has no antialiased mode: the twin at the compensated opacity)
    _image_bounds(f"{kind} map / s vs the float32 oracle on the twin", got, f32["image"][0])
    # the scene exercises it: the expected depth (map / alpha) varies by more than 20 % over the covered pixels - a pixel some instance contributed to has alpha >=
    # 1/255 - and so does d_i over the visible primitives (float64 host model; visibility from the oracle). One scene cannot reach the first figure: the 257
    # Gaussians of spread 0.3 have d_i within 30 % of each other, and every pixel of the 48 x 32 image blends several of them, which contracts the range of the
    # per-pixel means to 0.103 - 0.110 (float64 oracle, both kinds, both modes). That scene is held to 10 %, half the figure, and to the 20 % on d_i like the others.
    al, dm = n(alpha)[0].astype(np.float64), n(depth)[0].astype(np.float64)
    covered = al > 1.0 / 255.0
    ed = dm[covered] / al[covered]
    var = float((ed.max() - ed.min()) / ed.min())
    vis = f32["n_touched"] > 0
    d_vis = d64(sc["means"], sc["w2c"], kind)[0][vis]
    var_d = float((d_vis.max() - d_vis.min()) / d_vis.min())
    need = 0.1 if CFGS[idx]["N"] == 257 else 0.2
    print(f"alpha max {al.max():.3f} (> 0.3), covered pixels {int(covered.sum())}, map / alpha over them {ed.min():.4f} .. {ed.max():.4f}: varies by {var:.3f} (> {need}); "
          f"d_i over the {int(vis.sum())} visible primitives varies by {var_d:.3f} (> 0.2)")
    assert al.max() > 0.3 and var > need and var_d > 0.2, "the scene does not exercise the mode"


# ---- 2. backward, depth only -------------------------------------------------------------------------------------------------------------------------------------
BWD_CASES = [(i, k, False) for i in range(len(CFGS)) for k in KINDS] + [(2, "depth", True), (3, "invdepth", True)]


@pytest.mark.parametrize("idx,kind,aa", BWD_CASES, ids=lambda v: {True: "antialiased", False: "plain"}[v] if isinstance(v, bool) else IDS(v) if isinstance(v, int) else v)
def test_depth_only_backward_is_the_twins_colour_backward(lfs, oracle_mod, idx, kind, aa):
    sc, tw, s, dddz = _case(idx, kind)
    N = len(dddz)
    G = _g_depth(sc)
    gi_tw = np.zeros((3, sc["H"], sc["W"]), np.float32)
    gi_tw[0] = G[0] * np.float32(s)
    zi, za = _zeros(sc)
    row2 = np.asarray(sc["w2c"], np.float32).astype(np.float64)[2, :3]
    with _deterministic(lfs):
        got, dens = _backward(_forward_depth(sc, kind, aa), zi, za, t(G))
        ref, dens_tw = _backward(_forward_default(tw, aa), t(gi_tw), za)
    g2 = [n(x).astype(np.float64) for x in ref]
    dldd = g2[4][:, 0, 0] / C0 / s                                                          # dL/d(red) / s = sum w G = dL/dd_i, read off the twin
    assert np.abs(dldd).max() > 0
    exp_means = g2[0] + row2[None, :] * (dldd * dddz)[:, None]
    assert np.abs(exp_means - g2[0]).max() > 1e-3 * np.abs(g2[0]).max()                     # the dL/dz term is not lost in the bound
    for name, a, b in zip(GRADS[:4], got[:4], [exp_means, g2[1], g2[2], g2[3]]):
        _rows(f"{kind} bwd {name} vs the twin", n(a), b, N)
    assert float(got[4].abs().max()) == 0.0 and float(got[5].abs().max()) == 0.0           # grad_sh0, grad_sh_rest: exactly zero
    # densification_info keeps its definition (dL/dmean2d only): the twin's
    da, dd = n(dens), n(dens_tw)
    assert np.array_equal(da[0], dd[0]) and da[0].sum() > 0
    e, flips, rest = rows_check(da[1][:, None], dd[1][:, None], bar=1e-3, max_flips=3)
    print(f"densification norms vs the twin: rel-L2 {e:.2e}, flip rows {flips}, without them {rest:.2e} (< 1e-3)")
    assert rest < 1e-3, (e, flips, rest)
    if aa:
        return   # (the oracle has no antialiased mode; the antialiased default backward is held to it by tests/test_gpu_fastgs_antialiased.py)
    # directly against the float64 oracle on the twin
    f64 = _oracle_fwd(oracle_mod, tw, np.float64)
    og = oracle_mod.fastgs_backward(f64, tw["means"], tw["scales_raw"], tw["rot_raw"], tw["opac_raw"], tw["sh0"], tw["sh_rest"], tw["w2c"], tw["cam_pos"],
                                    tw["active_sh_bases"], tw["W"], tw["H"], tw["fx"], tw["fy"], tw["cx"], tw["cy"], gi_tw, np.zeros((1, sc["H"], sc["W"]), np.float32),
                                    dtype=np.float64)
    o_means = og[0] + row2[None, :] * (og[4][:, 0, 0] / C0 / s * dddz)[:, None]
    for name, a, b in zip(GRADS[:4], got[:4], [o_means, og[1], og[2], og[3]]):
        _rows(f"{kind} bwd {name} vs the float64 oracle on the twin", n(a), b, N)


# ---- 3. linearity ----------------------------------------------------------------------------------------------------------------------------------------------------
LINEARITY_CASES = [(0, "depth"), (1, "invdepth"), (3, "depth")]
CASE_IDS = lambda v: IDS(v) if isinstance(v, int) else v


@pytest.mark.parametrize("idx,kind", LINEARITY_CASES, ids=CASE_IDS)
def test_depth_backward_is_linear_in_its_three_gradients(lfs, idx, kind):
    sc = _case(idx, kind)[0]
    gi, ga = [t(x) for x in _upstream(sc)]
    gd = t(_g_depth(sc))
    zi, za = _zeros(sc)
    with _deterministic(lfs):
        st = _forward_depth(sc, kind)
        full = _backward(st, gi, ga, gd)[0]
        colour = _backward(st, gi, ga, torch.zeros_like(gd))[0]
        depth_only = _backward(st, zi, za, gd)[0]
        plain = _backward(st, gi, ga)[0]                                                    # the backward without grad_depth on the same (depth-mode) workspace
    for name, a, b, c, p in zip(GRADS, full, colour, depth_only, plain):
        if a.numel() == 0:
            continue
        e = rel_l2(n(a), n(b).astype(np.float64) + n(c).astype(np.float64))
        e0 = rel_l2(n(b), n(p))
        print(f"{name}: backward(gi, ga, gd) vs backward(gi, ga, 0) + backward(0, 0, gd) rel-L2 {e:.2e}; backward(gi, ga, 0) vs backward(gi, ga) {e0:.2e} (both <= 1e-6)")
        assert e <= 1e-6 and e0 <= 1e-6, (name, e, e0)
    assert float(depth_only[0].abs().max()) > 0 and float((full[0] - colour[0]).abs().max()) > 0


# ---- 4. camera gradient ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx,kind", [(2, "depth"), (3, "invdepth"), (0, "depth")], ids=lambda v: IDS(v) if isinstance(v, int) else v)
def test_depth_camera_gradient(lfs, idx, kind):
    from test_gpu_fastgs_w2c import _expected
    sc, tw, s, dddz = _case(idx, kind)
    G = _g_depth(sc)
    gi_tw = np.zeros((3, sc["H"], sc["W"]), np.float32)
    gi_tw[0] = G[0] * np.float32(s)
    zi, za = _zeros(sc)
    with _deterministic(lfs):
        gw1, gw2, gwt = [torch.full((4, 4), NAN, device=DEV) for _ in range(3)]
        r1 = _backward(_forward_depth(sc, kind), zi, za, t(G), grad_w2c=gw1)[0]
        r2 = _backward(_forward_depth(sc, kind), zi, za, t(G), grad_w2c=gw2)[0]
        rt = _backward(_forward_default(tw), t(gi_tw), za, grad_w2c=gwt)[0]
    assert torch.equal(gw1, gw2) and all(torch.equal(p, q) for p, q in zip(r1, r2))        # the same bits on two runs
    out, out_tw = n(gw1).astype(np.float64), n(gwt).astype(np.float64)
    # (a) the identity of tests/test_gpu_fastgs_w2c.py on the entry point's own grad_means (g_image = 0: no SH term in them, whatever the degree)
    E, M = _expected(sc, n(r1[0]))
    err = float(np.abs(out[:3] - E).max())
    print(f"{kind} grad_w2c identity: max |grad_w2c - E| {err:.3e}, bound 1e-5 M = {1e-5 * M:.3e}")
    assert np.isfinite(out).all() and (out[3] == 0).all() and M > 0 and err <= 1e-5 * M
    # (b) on top of the twin's value: rows 0 and 1 are the twin's, row 2 carries sum_i dL/dz_i (mean_i, 1) - float64 model, dL/dd_i read off the twin
    dldz = n(rt[4]).astype(np.float64)[:, 0, 0] / C0 / s * dddz
    m1 = np.concatenate([np.asarray(sc["means"], np.float32).astype(np.float64), np.ones((len(dldz), 1))], 1)
    extra = dldz @ m1
    M2 = M + float((np.abs(dldz) * np.linalg.norm(m1, axis=1)).sum())
    diff = out[:3] - out_tw[:3]
    e01, e2 = float(np.abs(diff[:2]).max()), float(np.abs(diff[2] - extra).max())
    print(f"{kind} grad_w2c - the twin's: rows 0-1 max {e01:.3e}, row 2 - sum dL/dz (m, 1) max {e2:.3e}, bound 1e-5 M = {1e-5 * M2:.3e}; |row 2 term| {np.abs(extra).max():.3e}")
    assert np.abs(extra).max() > 1e-3 * M2 and e01 <= 1e-5 * M2 and e2 <= 1e-5 * M2


# ---- 5. the default mode is untouched; flag errors ----------------------------------------------------------------------------------------------------------------------
def test_default_mode_is_untouched_by_the_depth_modes(lfs):
    sc = _case(0, "depth")[0]
    with _deterministic(lfs) as lib:
        a, s = _dev(sc), _settings(sc)
        gi, ga = [t(x) for x in _upstream(sc)]
        rc0, pws0, n0 = _preprocess_raw(lib, a, s, 0)
        rc1, pws1, n1 = _preprocess_raw(lib, a, s, 0)
        assert rc0 == 0 and rc1 == 0
        base = _render_and_backward_raw(lib, a, s, pws0, n0, gi, ga)
        _same_bits(base, _render_and_backward_raw(lib, a, s, pws1, n1, gi, ga))
        assert float(base[3][0].abs().max()) > 0
        # a workspace last used in a depth mode: colour, alpha and the default backward do not see the flag ...
        for flag in (LFS_FASTGS_DEPTH, LFS_FASTGS_INVDEPTH):
            rc2, pws2, n2 = _preprocess_raw(lib, a, s, flag)
            assert rc2 == 0
            _same_bits(base, _render_and_backward_raw(lib, a, s, pws2, n2, gi, ga))
            # ... and the next default preprocess into it gives today's render and backward, and takes the depth plane away again
            rc3, _, n3 = _preprocess_raw(lib, a, s, 0, pws=pws2)
            assert rc3 == 0
            _same_bits(base, _render_and_backward_raw(lib, a, s, pws2, n3, gi, ga))
            assert _render_depth_rc(lib, sc, pws2, int(n3.item())) == INVALID
    lib = lfs.load_library()
    assert lib.lfs_fastgs_primitive_workspace_bytes(C.c_uint32(3000), C.c_uint32(160), C.c_uint32(112)) == 577792    # the parent commit's size
    # flag errors: both depth flags, unknown bits -> LFS_E_INVALID before any launch, nothing written
    a, s = _dev(sc), _settings(sc)
    pws = torch.full((577792,), 0xA5, dtype=torch.uint8, device=DEV)
    n_dev = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    for flags in (LFS_FASTGS_DEPTH | LFS_FASTGS_INVDEPTH, LFS_FASTGS_DEPTH | LFS_FASTGS_INVDEPTH | 1, 2, 16, 0x80000000 | LFS_FASTGS_DEPTH):
        rc, _, _ = _preprocess_raw(lib, a, s, flags, pws=pws, n_dev=n_dev)
        torch.cuda.synchronize()
        assert rc == INVALID and int(n_dev.item()) == -7 and bool((pws == 0xA5).all()), flags
    # the depth plane and the depth gradient on a workspace whose preprocess carried no depth flag: LFS_E_INVALID, no launch
    st = _forward_default(sc)
    image, alpha, _, pws, iws, n_inst, a, s = st
    assert _render_depth_rc(lib, sc, pws, n_inst) == INVALID
    gd = t(_g_depth(sc))
    grads = [torch.full_like(x, 7.0) for x in (a[0], a[1], a[2], a[3].reshape(-1, 1), a[4], a[5])]
    def bwd_depth(pws_, iws_, gd_):
        return backward_raw(lib, a, s, pws_, iws_, n_inst, gi, ga, alpha, None, grads, gd=gd_)
    assert bwd_depth(pws, iws, gd) == INVALID
    torch.cuda.synchronize()
    assert all(bool((g == 7.0).all()) for g in grads)
    std = _forward_depth(sc, "depth")
    assert std[5] == n_inst and bwd_depth(std[3], std[4], None) == 0                      # no grad_depth: the plain backward, which takes a depth workspace
    assert bwd_depth(std[3], std[4], gd) == 0 and not bool((grads[0] == 7.0).all())
    # forwards without a depth flag between a depth forward and its backward do not cost it its place in the host's table (20 > any small table; evaluation renders
    # and other views do exactly this), a default forward into a depth workspace's own address does
    small = _case(2, "invdepth")[0]
    sts = _forward_depth(small, "invdepth")
    others = [_forward_default(small) for _ in range(20)]
    zi, za = _zeros(small)
    g, _ = _backward(sts, zi, za, t(_g_depth(small)))
    assert float(g[0].abs().max()) > 0 and len({o[3].data_ptr() for o in others}) == 20
    # N = 0 and N = 1
    for N in (0, 1):
        cut = dict(sc, **{k: sc[k][:N] for k in KEYS[:6]})
        for kind in KINDS:
            stc = _forward_depth(cut, kind)
            zi, za = _zeros(cut)
            gw = torch.full((4, 4), NAN, device=DEV)
            g, _ = _backward(stc, zi, za, t(_g_depth(cut)), grad_w2c=gw)
            assert bool(torch.isfinite(stc[2]).all()) and (N > 0 or float(stc[2].abs().max()) == 0) and bool(torch.isfinite(gw).all())
            for x in g:
                assert x.shape[0] == N and bool(torch.isfinite(x).all())


# ---- 5b. the optimizer-fused backward has no camera gradient and no depth gradient ----------------------------------------------------------------------------------------
def test_adam_is_refused_with_grad_w2c_and_with_grad_depth(lfs):
    """args.adam together with grad_w2c or with grad_depth: LFS_E_INVALID before any launch (the rule fastgs.backward_wrapper states as an LfsError, held by the library
    itself). The forward ran in a depth mode and the w2c workspace is valid, so each call is accepted once adam is taken away: the combination is what is refused.
    Every output buffer, the parameter the fused form would update and its moments are pre-filled and found untouched."""
    from lichtfeld_studio_amd.capi import ptr
    lib = lfs.load_library()
    sc = _scene(N=300, W=80, H=64, deg=1)
    N = len(sc["means"])
    image, alpha, depth, pws, iws, n_inst, a, s = _forward_depth(sc, "depth")
    assert n_inst > 0 and a[5].shape[1] > 0
    gi, ga = [t(x) for x in _upstream(sc)]
    gd = t(_g_depth(sc))
    shr = a[5].clone()
    a_fused = a[:5] + [shr] + a[6:]
    grads = [torch.full_like(x, 7.0) for x in (a[0], a[1], a[2], a[3].reshape(-1, 1), a[4], a[5])]
    gw, dens = torch.full((4, 4), 7.0, device=DEV), torch.full((2, N), 7.0, device=DEV)
    m1, m2 = torch.full_like(shr, 3.0), torch.full_like(shr, 5.0)
    ws = torch.full((lib.lfs_fastgs_w2c_workspace_bytes(C.c_uint32(N)),), 0xA5, dtype=torch.uint8, device=DEV)
    tail = (ptr(gw), ptr(ws), ws.numel())
    call = lambda **kw: backward_raw(lib, a_fused, s, pws, iws, n_inst, gi, ga, alpha, dens, grads, **kw)
    assert call(adam=(shr, m1, m2), w2c_tail=tail) == INVALID
    assert call(adam=(shr, m1, m2), gd=gd) == INVALID
    assert call(adam=(shr, m1, m2), gd=gd, w2c_tail=tail) == INVALID
    torch.cuda.synchronize()
    assert all(bool((g == 7.0).all()) for g in grads) and bool((gw == 7.0).all()) and bool((dens == 7.0).all()) and bool((ws == 0xA5).all())
    assert torch.equal(shr, a[5]) and bool((m1 == 3.0).all()) and bool((m2 == 5.0).all())
    dens.zero_()
    assert call(gd=gd, w2c_tail=tail) == 0 and not bool((grads[0] == 7.0).all()) and bool(torch.isfinite(gw).all())     # without adam: accepted


def _render_depth_rc(lib, sc, pws, n_inst):
    W, H = sc["W"], sc["H"]
    s = _settings(sc)
    image, alpha, depth = torch.full((3, H, W), 5.0, device=DEV), torch.full((1, H, W), 5.0, device=DEV), torch.full((1, H, W), 5.0, device=DEV)
    rc = render_raw(lib, _dev(sc), s, pws, n_inst, instance_workspace(lib, s, n_inst), image, alpha, depth)
    if rc != 0:
        torch.cuda.synchronize()
        assert bool((image == 5.0).all()) and bool((depth == 5.0).all())                   # refused before any launch
    return rc


# ---- 6. the Python layers: fast_rasterize's five render modes and autograd through FastGSRasterize ---------------------------------------------------------------------
def test_fast_rasterize_render_modes_and_autograd(lfs):
    from lichtfeld_studio_amd import fastgs
    from lichtfeld_studio_amd.rasterizer import Camera, RenderMode, SplatModel
    sc = _case(3, "depth")[0]
    a = _dev(sc)
    K = torch.tensor([[sc["fx"], 0, sc["cx"]], [0, sc["fy"], sc["cy"]], [0, 0, 1]], dtype=torch.float32, device=DEV)
    cam = Camera(a[6].reshape(1, 4, 4).contiguous(), K.reshape(1, 3, 3), sc["W"], sc["H"])
    model = SplatModel(a[0], a[4], a[5], a[1], a[2], a[3].reshape(-1, 1), 2)
    bg = torch.zeros(3, device=DEV)
    with _deterministic(lfs):
        rgb = fastgs.fast_rasterize(cam, model, bg)
        outs = {m: fastgs.fast_rasterize(cam, model, bg, render_mode=m) for m in (RenderMode.D, RenderMode.ED, RenderMode.RGB_D, RenderMode.RGB_ED)}
        inv = fastgs.fast_rasterize(cam, model, bg, render_mode=RenderMode.RGB_D, depth_kind="invdepth")
        _, _, dacc, _, _, _, _, _ = _forward_depth(sc, "depth")
        assert rgb.depth is None and outs[RenderMode.D].image is None and outs[RenderMode.ED].image is None
        assert torch.equal(outs[RenderMode.RGB_D].image, rgb.image) and torch.equal(outs[RenderMode.RGB_ED].image, rgb.image)
        assert torch.equal(outs[RenderMode.D].depth, dacc) and torch.equal(outs[RenderMode.RGB_D].depth, dacc)
        ed = dacc / rgb.alpha.clamp_min(1e-10)
        assert torch.equal(outs[RenderMode.ED].depth, ed) and torch.equal(outs[RenderMode.RGB_ED].depth, ed)
        assert not torch.equal(inv.depth, dacc) and torch.equal(inv.image, rgb.image)
        # autograd: a loss on the expected depth and the image, against the hand-made chain rule over backward_wrapper
        params = [p.clone().requires_grad_(True) for p in (a[0], a[4], a[5], a[1], a[2], a[3].reshape(-1, 1))]
        m2 = SplatModel(*params, 2)
        o = fastgs.fast_rasterize(cam, m2, bg, render_mode=RenderMode.RGB_ED)
        Wi, Wd = [t(x) for x in _upstream(sc, seed=11)]
        ((o.image * Wi).sum() + (o.depth * Wd).sum()).backward()
        st = _forward_depth(sc, "depth")
        al = st[1].clamp_min(1e-10)
        g_alpha = -(Wd * st[2] / (al * al)) * (st[1] >= 1e-10)
        hand, _ = _backward(st, Wi, g_alpha, Wd / al)
    for name, p, h in zip(("means", "sh0", "shN", "raw_scales", "raw_quats", "raw_opacities"), params, (hand[0], hand[4], hand[5], hand[1], hand[2], hand[3])):
        e = rel_l2(n(p.grad), n(h).reshape(n(p.grad).shape))
        print(f"autograd through RGB_ED, {name}: rel-L2 against the hand-made chain {e:.2e} (<= 1e-6)")
        assert e <= 1e-6, (name, e)
