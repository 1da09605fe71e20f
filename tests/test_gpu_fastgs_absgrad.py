"""GPU: absolute screen-space gradients for densification in the fastgs (EWA) rasterizer (LFS_FASTGS_ABSGRAD, AbsGS / gsplat's absgrad).

The flag changes one thing: what a backward with densification_info adds to row 1 - the norm of the per-pixel ABSOLUTE shares of dL/dmean2d instead of the norm of their
signed sum. Every value here is held to the float64 host model tests/fastgs_absgrad_reference.py (independent of the code under test, itself held to the oracle's
densification_info by tests/test_fastgs_absgrad_reference.py, which also checks on the CPU that the scenes and seeds used here stay within the flip-row budget).
Row 1 is compared with rows_check(bar=1e-3, max_flips=3), the rule tests/test_gpu_fastgs_depth.py holds these norms to.
All of it also runs on the wavefront emulator (tests/test_emulated_fastgs_absgrad.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import fastgs_absgrad_reference as ref
from fastgs_raw import backward_raw, instance_workspace, preprocess_raw, render_raw
from gpu_util import n, rows_check, t
from test_gpu_fastgs_antialiased import KEYS, _deterministic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
ABSGRAD, INVALID = 32, -1
K = 0.5 * 1.4426950408889634   # the scale of the record's conic, and so of slots 10 / 11 of the accumulator row


def _settings(sc, absgrad=False, aa=False, depth="none", f3d=None):
    from lichtfeld_studio_amd.fastgs import FastGSSettings
    return FastGSSettings(t(sc["cam_pos"]), sc["active_sh_bases"], sc["W"], sc["H"], sc["fx"], sc["fy"], sc["cx"], sc["cy"], 0.01, 1e10, aa, depth, f3d, absgrad)


def _dev(sc):
    return [t(sc[k]) for k in KEYS]


def _run(sc, gi, ga, absgrad, aa=False, gd=None, f3d=None, dens=True, want_w2c=False, calls=1):
    """forward + `calls` backwards of the Python mirror -> dict(image, alpha, grads, dens, gw, pws)"""
    from lichtfeld_studio_amd import fastgs
    a, s = _dev(sc), _settings(sc, absgrad, aa, "depth" if gd is not None else "none", None if f3d is None else t(f3d))
    if gd is not None:
        image, alpha, _, pws, iws, n_inst = fastgs.forward_wrapper_depth(*a, s)
    else:
        image, alpha, pws, iws, n_inst = fastgs.forward_wrapper(*a, s)
    d = torch.zeros(2, a[0].shape[0], device=DEV) if dens else None
    gw = torch.full((4, 4), NAN, device=DEV) if want_w2c else None
    for _ in range(calls):
        g = fastgs.backward_wrapper(d, t(gi), t(ga), image, alpha, a[0], a[1], a[2], a[4], a[5], pws, iws, a[6], s, n_inst, grad_w2c=gw, grad_depth=t(gd))
    return dict(image=image, alpha=alpha, grads=g, dens=d, gw=gw, pws=pws, n_inst=n_inst)


def _al(v):
    return (v + 255) & ~255


def _rows_of(pws, N, W, H):
    """(conic_opacity [N,4], accumulator rows [N,16]) of a primitive workspace (csrc/lfs_fastgs.cuh: prim_ws)"""
    T, P = ((W + 15) // 16) * ((H + 15) // 16), W * H
    raw = pws.cpu().numpy()
    o_conic = _al(64 * N) + _al(8 * N)
    o_acc = o_conic + _al(16 * N) + _al(8 * N) + 2 * _al(4 * N) + 2 * _al(4 * T) + _al(4 * (T + 1)) + 256 + _al(4 * P)
    return raw[o_conic:o_conic + 16 * N].copy().view(np.float32).reshape(N, 4), raw[o_acc:o_acc + 64 * N].copy().view(np.float32).reshape(N, 16)


def _check_norms(label, dens, model):
    da = n(dens).astype(np.float64)
    assert np.array_equal(da[0], model["dens_abs"][0]) and da[0].sum() > 0, label
    e, flips, rest = rows_check(da[1][:, None], model["dens_abs"][1][:, None], bar=1e-3, max_flips=3)
    print(f"{label}: absgrad norms vs the float64 model rel-L2 {e:.2e}, flip rows {flips}, without them {rest:.2e} (< 1e-3); {model['instances']} instances")
    assert rest < 1e-3, (label, e, flips, rest)


# ---- 1. values ------------------------------------------------------------------------------------------------------------------------------------------------------
VALUE_CASES = [(i, "plain", det) for i in range(len(ref.CFGS)) for det in (True, False)] + [(i, v, True) for i in ref.VARIANT_SCENES for v in ref.VARIANTS[1:]]


@pytest.mark.parametrize("idx,variant,det", VALUE_CASES,
                         ids=lambda v: {True: "deterministic", False: "float-atomics"}[v] if isinstance(v, bool) else ref.SCENE_IDS(v) if isinstance(v, int) else v)
def test_absgrad_densification_info_matches_the_float64_model(lfs, oracle_mod, idx, variant, det):
    import contextlib
    sc = ref.scene(idx)
    gi, ga = ref.upstream(sc)
    model = ref.variant_model(oracle_mod, idx, variant)
    kw = dict(gd=ref.g_depth_of(sc)) if variant == "depth" else dict(aa=True) if variant == "aa" else dict(f3d=ref.filter_var_of(sc)) if variant == "f3d" else {}
    with (_deterministic(lfs) if det else contextlib.nullcontext()):
        out = _run(sc, gi, ga, True, **kw)
        base = _run(sc, gi, ga, False, **kw)
    _check_norms(f"{ref.SCENE_IDS(idx)} {variant}", out["dens"], model)
    # |sum| <= sum |.| per component: never below the default mode's norm, less the rounding of two float32 summations (1e-4, test 3)
    da, db = n(out["dens"]).astype(np.float64), n(base["dens"]).astype(np.float64)
    assert np.array_equal(da[0], db[0]) and (da[1] >= db[1] * (1 - 1e-4)).all()
    if len(sc["means"]) >= 200:
        assert da[1].sum() > 1.05 * db[1].sum()                             # and it is not the default mode's


# ---- 2. the case the feature exists for -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("det", [True, False], ids=["deterministic", "float-atomics"])
def test_a_gaussian_whose_signed_gradient_cancels_is_seen_by_absgrad(lfs, oracle_mod, det):
    """one isotropic Gaussian centred exactly on a pixel corner (24, 24) in the interior of tile (1, 1), uniform positive grad_image, black background"""
    import contextlib
    sc = ref.single_gaussian_scene(64, 48, (24.0, 24.0))
    gi, ga = np.ones((3, 48, 64), np.float32), np.zeros((1, 48, 64), np.float32)
    model = ref.model_of(oracle_mod, "corner", sc, gi, ga)
    with (_deterministic(lfs) if det else contextlib.nullcontext()):
        dabs, ddef = n(_run(sc, gi, ga, True)["dens"]), n(_run(sc, gi, ga, False)["dens"])
    print(f"default norm {ddef[1, 0]:.3e}, absgrad norm {dabs[1, 0]:.3e}, float64 model {model['dens_abs'][1, 0]:.6e}")
    assert dabs[0, 0] == 1 and ddef[0, 0] == 1 and dabs[1, 0] > 0
    assert ddef[1, 0] < 1e-3 * dabs[1, 0]
    assert abs(dabs[1, 0] - model["dens_abs"][1, 0]) < 1e-3 * model["dens_abs"][1, 0]


# ---- 3. nothing to cancel ----------------------------------------------------------------------------------------------------------------------------------------------
def test_without_cancellation_the_absolute_sum_is_the_signed_one(lfs):
    """one isotropic Gaussian (B = 0) whose centre lies left of every pixel it reaches, uniform positive gradient: every gx_p has one sign, Gx = |A S1|. Read off the
    accumulator rows: slot 0 = S1 of a default backward, slot 10 = k Gx of an absgrad backward (k = 0.5 log2(e)). 1e-4: two summation orders of a few hundred same-sign
    float32 terms. The rows also show the layout: slot 9 zero without depth, slots 12 .. 15 zero, slots 10 / 11 zero in the default form."""
    sc = ref.single_gaussian_scene(64, 48, (0.25, 24.0))
    gi, ga = np.ones((3, 48, 64), np.float32), np.zeros((1, 48, 64), np.float32)
    with _deterministic(lfs):
        ra, rd = _run(sc, gi, ga, True), _run(sc, gi, ga, False)
    conic, acc_abs = _rows_of(ra["pws"], 1, 64, 48)
    _, acc_def = _rows_of(rd["pws"], 1, 64, 48)
    A, B = float(conic[0, 0]), float(conic[0, 1])
    S1, Gx = float(acc_def[0, 0]), float(acc_abs[0, 10]) / K
    print(f"A {A:.6f} B {B:.2e}; S1 {S1:.6e}, |A S1| {abs(A * S1):.6e}, Gx {Gx:.6e}: relative difference {abs(Gx - abs(A * S1)) / abs(A * S1):.2e} (<= 1e-4)")
    assert B == 0 and S1 != 0 and abs(Gx - abs(A * S1)) <= 1e-4 * abs(A * S1)
    assert np.array_equal(acc_abs[0, :9], acc_def[0, :9])                   # slots 0 .. 8: the default form's bits
    assert (acc_abs[0, 9] == 0) and (acc_abs[0, 12:] == 0).all() and acc_abs[0, 11] > 0 and (acc_def[0, 9:] == 0).all()


# ---- 4. the gradients are untouched ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [2, 3], ids=ref.SCENE_IDS)
def test_gradients_and_render_are_bit_identical_with_and_without_the_flag(lfs, idx):
    sc = ref.scene(idx)
    gi, ga = ref.upstream(sc)
    with _deterministic(lfs) as lib:
        base = _run(sc, gi, ga, False, want_w2c=True)
        with_dens = None
        for dens in (True, False):
            out = _run(sc, gi, ga, True, dens=dens, want_w2c=True)
            with_dens = with_dens or out
            assert out["n_inst"] == base["n_inst"] and torch.equal(out["image"], base["image"]) and torch.equal(out["alpha"], base["alpha"])
            assert torch.equal(out["gw"], base["gw"]) and bool(torch.isfinite(out["gw"]).all())
            for p, q in zip(out["grads"], base["grads"]):
                assert torch.equal(p, q)
        assert float(base["grads"][0].abs().max()) > 0
        gd = ref.g_depth_of(sc)                                             # the depth form of the blend backward as well
        bd, od = _run(sc, gi, ga, False, gd=gd, want_w2c=True), _run(sc, gi, ga, True, gd=gd, want_w2c=True)
        assert torch.equal(od["gw"], bd["gw"]) and all(torch.equal(p, q) for p, q in zip(od["grads"], bd["grads"]))
        assert not torch.equal(bd["grads"][0], base["grads"][0]) and not torch.equal(od["dens"], bd["dens"])
        # slots 10 / 11 are observable nowhere else: a default-mode forward + backward on the SAME workspace object after an absgrad one gives the default densification_info
        a, s = _dev(sc), _settings(sc)
        N = a[0].shape[0]
        gi_t, ga_t = t(gi), t(ga)

        def fwd_bwd(flags, pws):
            rc, pws, n_dev = preprocess_raw(lib, a, s, flags, pws=pws)
            assert rc == 0
            n_inst = int(n_dev.item())
            iws = instance_workspace(lib, s, n_inst)
            image, alpha = torch.empty((3, s.height, s.width), device=DEV), torch.empty((1, s.height, s.width), device=DEV)
            assert render_raw(lib, a, s, pws, n_inst, iws, image, alpha) == 0
            d = torch.zeros(2, N, device=DEV)
            grads = [torch.empty_like(x) for x in (a[0], a[1], a[2], a[3].reshape(-1, 1), a[4], a[5])]
            assert backward_raw(lib, a, s, pws, iws, n_inst, gi_t, ga_t, alpha, d, grads) == 0
            return pws, d
        pws, d_abs = fwd_bwd(ABSGRAD, None)
        _, d_def = fwd_bwd(0, pws)
        assert torch.equal(d_abs, with_dens["dens"]) and torch.equal(d_def, base["dens"]) and not torch.equal(d_abs, d_def)


# ---- 5. flags ----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_flag_values_accumulation_and_the_optimizer_fused_backward(lfs):
    sc = ref.scene(2)
    gi, ga = ref.upstream(sc)
    lib = lfs.load_library()
    a, s = _dev(sc), _settings(sc)
    N = a[0].shape[0]
    for flags in (32, 32 | 1, 32 | 4, 32 | 8, 32 | 8 | 1):
        rc, _, n_dev = preprocess_raw(lib, a, s, flags)
        assert rc == 0 and int(n_dev.item()) > 0, flags
    size = lib.lfs_fastgs_primitive_workspace_bytes(C.c_uint32(N), C.c_uint32(s.width), C.c_uint32(s.height))
    pws = torch.full((size,), 0xA5, dtype=torch.uint8, device=DEV)
    n_dev = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    for flags in (32 | 4 | 8, 2, 16, 64, 1 << 16, 0x80000000, 32 | 2, 32 | 16, 32 | 64):
        rc, _, _ = preprocess_raw(lib, a, s, flags, pws=pws, n_dev=n_dev)
        torch.cuda.synchronize()
        assert rc == INVALID and int(n_dev.item()) == -7 and bool((pws == 0xA5).all()), flags   # refused before any launch
    with _deterministic(lfs):
        one, two = _run(sc, gi, ga, True), _run(sc, gi, ga, True, calls=2)
        assert torch.equal(two["dens"][0], 2 * one["dens"][0]) and float(one["dens"][0].max()) == 1 and torch.equal(two["dens"][1], 2 * one["dens"][1])
        # args->adam (the optimizer-fused SH backward) on an absgrad workspace: accepted, the same densification_info
        rc, pws, n_dev = preprocess_raw(lib, a, s, ABSGRAD)
        n_inst = int(n_dev.item())
        iws = instance_workspace(lib, s, n_inst)
        image, alpha = torch.empty((3, s.height, s.width), device=DEV), torch.empty((1, s.height, s.width), device=DEV)
        assert rc == 0 and render_raw(lib, a, s, pws, n_inst, iws, image, alpha) == 0
        shr = a[5].clone()
        d = torch.zeros(2, N, device=DEV)
        grads = [torch.full_like(x, 7.0) for x in (a[0], a[1], a[2], a[3].reshape(-1, 1), a[4], a[5])]
        assert backward_raw(lib, a[:5] + [shr] + a[6:], s, pws, iws, n_inst, t(gi), t(ga), alpha, d, grads, adam=(shr, torch.zeros_like(shr), torch.zeros_like(shr))) == 0
        assert torch.equal(d, one["dens"]) and not torch.equal(shr, a[5]) and torch.equal(grads[0], one["grads"][0])


# ---- 6. trainer ----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_trainer_densifies_by_absolute_gradients(lfs):
    from lichtfeld_studio_amd import scenes, strategies
    from lichtfeld_studio_amd.trainer import GutTrainer
    dev = torch.device(DEV)
    sc = scenes.syn_a(n=4000, sh_degree=1)                                  # the small ADC scene of tests/test_gpu_fastgs.py, refining sooner
    target = (scenes.target_image(sc.height, sc.width) * 0.8 + 0.1).to(dev)
    sched = dict(iterations=300, start_refine=3, refine_every=4, stop_refine=200, reset_every=100000, sh_degree_interval=1000)
    OP = strategies.OptimizationParameters
    assert OP.for_strategy("default", absgrad=True).grad_threshold == 8e-4 and OP.for_strategy("default").grad_threshold == 2e-4
    assert OP.for_strategy("default", absgrad=True, grad_threshold=3e-4).grad_threshold == 3e-4
    with pytest.raises(ValueError, match="3DGUT"):
        GutTrainer(sc, dev, iterations=100, rasterizer="gut", strategy="mcmc", absgrad=True)
    with pytest.raises(ValueError, match="strategy='default'"):
        GutTrainer(sc, dev, iterations=100, rasterizer="fastgs", strategy="mcmc", absgrad=True)
    with pytest.raises(ValueError, match="strategy='default'"):
        GutTrainer(sc, dev, iterations=100, rasterizer="fastgs", absgrad=True)
    mk = lambda **kw: GutTrainer(sc, dev, iterations=300, rasterizer="fastgs", loss="l1_ssim", strategy="default", **kw)
    with _deterministic(lfs):
        a, b = [mk(opt_params=OP.for_strategy("default", absgrad=True, **sched), absgrad=True) for _ in range(2)]
        c = mk(opt_params=OP.for_strategy("default", absgrad=True, **sched))   # the same threshold, signed gradients
        assert a.strategy.params.grad_threshold == 8e-4 and mk(absgrad=True).strategy.params.grad_threshold == 8e-4
        n0 = a.model.means.shape[0]
        for step in range(4):                                                # iteration 4 is the first refinement
            for tr in (a, b, c):
                tr.train_step([target], views=[0])
            if step == 2:
                da, dc = a.densification_info.clone(), c.densification_info.clone()
        assert a._fg_settings[0].absgrad and not c._fg_settings[0].absgrad
        assert torch.equal(da[0], dc[0]) and float(da[0].max()) == 3 and bool((da[1] >= dc[1] * (1 - 1e-4)).all()) and float(da[1].sum()) > 1.05 * float(dc[1].sum())
        print(f"Gaussians after the first refinement: absgrad {a.model.means.shape[0]}, signed gradients at the same threshold {c.model.means.shape[0]} (from {n0})")
        assert a.model.means.shape[0] > n0, "ADC never densified"
        assert a.model.means.shape[0] == b.model.means.shape[0] and all(torch.equal(p, q) for p, q in zip(a.model.parameters(), b.model.parameters()))
        # absgrad=False is the trainer without the argument
        e, f = mk(opt_params=OP.for_strategy("default", **sched), absgrad=False), mk(opt_params=OP.for_strategy("default", **sched))
        for _ in range(5):
            e.train_step([target], views=[0]), f.train_step([target], views=[0])
        assert all(torch.equal(p, q) for p, q in zip(e.model.parameters(), f.model.parameters())) and e.last_plan == f.last_plan and not e.absgrad
        assert torch.equal(e.densification_info, f.densification_info) and not e._fg_settings[0].absgrad


# ---- 7. libtorch ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_libtorch_route_matches_the_ctypes_route_bit_for_bit(lfs):
    from lichtfeld_studio_amd import _lfs_torch_ops as m
    sc = ref.scene(3)
    a, cam = _dev(sc), t(sc["cam_pos"])
    N = a[0].shape[0]
    fr = (sc["active_sh_bases"], sc["W"], sc["H"], sc["fx"], sc["fy"], sc["cx"], sc["cy"], 0.01, 1e10)
    gi, ga = ref.upstream(sc)
    none = torch.empty(0, device=DEV)
    with _deterministic(lfs):
        for aa in (False, True):
            image, alpha, _, prim, inst, n_inst = m.fastgs_forward(*a, cam, *fr, antialiased=aa, absgrad=True)
            d1 = torch.zeros(2, N, device=DEV)
            g1 = m.fastgs_backward_wrapper(d1, t(gi), t(ga), image, alpha, a[0], a[1], a[2], a[5], prim, none, inst, none, a[6], cam, *fr, 0, n_inst, 0, 0, 0)
            out = _run(sc, gi, ga, True, aa=aa)
            assert n_inst == out["n_inst"] and torch.equal(image, out["image"]) and torch.equal(alpha, out["alpha"])
            assert torch.equal(d1, out["dens"]) and float(d1[1].sum()) > 0
            for p, q in zip(g1[:6], out["grads"]):
                assert torch.equal(p.reshape(q.shape), q)
            off = m.fastgs_forward(*a, cam, *fr, antialiased=aa, absgrad=False)    # absgrad = false: the default densification_info
            d0 = torch.zeros(2, N, device=DEV)
            m.fastgs_backward_wrapper(d0, t(gi), t(ga), off[0], off[1], a[0], a[1], a[2], a[5], off[3], none, off[4], none, a[6], cam, *fr, 0, off[5], 0, 0, 0)
            assert torch.equal(d0, _run(sc, gi, ga, False, aa=aa)["dens"]) and not torch.equal(d0, d1)
