"""lfs_gut_train_step_opt - the one-call training step for what the reference trains: L1 + D-SSIM instead of the folded MSE, the MCMC strategy's noise folded in front
of the means' Adam update, shN frozen while iteration <= 1000 - on the wavefront emulator (the whole product library as host code, tests/emul_util.py), held BIT FOR BIT
on all six parameters and twelve moments to the composition of the entry points it replaces:

    lfs_gut_view_forward | [lfs_photometric_loss_fwd_bwd] | lfs_gut_view_backward into gradient tensors | [lfs_add_noise] | lfs_adam_step_multi over the non-frozen groups

over several consecutive steps with the views taking turns, so that every step after the first renders with the SH colours the previous step's tail evaluated for it
(from the noised, updated mean). Sums are sequential on the emulator, so the loss values are compared for equality as well."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

LFS_E_UNSUPPORTED = -2
W, H, TILE = 64, 48, 16


class AdamTensor(C.Structure):  # lfs_adam_tensor
    _fields_ = [("param", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("grad", C.c_void_p), ("n_elements", C.c_int64),
                ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("bc1", C.c_float), ("bc2", C.c_float)]


def _defs():
    src = open(os.path.join(ROOT, "lichtfeld-studio_amd", "gut_step.py")).read()
    ns = {}
    exec("import ctypes as C\n" + src[src.index("class StepArgs"):src.index("class GutStep")], ns)   # (the ctypes structures only: the module imports the GPU loader)
    return ns


@pytest.fixture(scope="module")
def emu():
    import emul_util
    if not emul_util.available():
        pytest.skip("no clang++ to build the emulated kernels")
    lib = emul_util.library()
    assert hasattr(lib, "lfs_gut_train_step_opt"), "the library has no lfs_gut_train_step_opt"
    lib.lfs_gut_step_loss_workspace_bytes.restype = C.c_size_t
    return lib


def _scene(seed, N, K, degree):
    from gpu_util import make_gaussians, pinhole_K, small_rotation_viewmat
    rng = np.random.default_rng(seed)
    means, quats, scales, opac = make_gaussians(rng, N, spread=1.0, smin=0.02, smax=0.12)
    raw_opac = np.log(opac / (1 - opac)).astype(np.float32)
    raw_opac[rng.random(N) < 0.1] = -6.0                                      # some below 1/255: never listed by the projection - noise and Adam reach them all the same
    sc = dict(means=means, raw_quats=quats, raw_scales=np.log(scales).astype(np.float32), raw_opac=raw_opac,
              sh0=(rng.standard_normal((N, 1, 3)) * 0.5).astype(np.float32), shN=(rng.standard_normal((N, K - 1, 3)) * 0.2).astype(np.float32),
              K=pinhole_K(0.8 * W, W, H, 1)[0], bg=rng.random(3).astype(np.float32), Kn=K, degree=degree)
    sc["vms"] = [np.ascontiguousarray(small_rotation_viewmat(np.random.default_rng(s), a, b), np.float32) for s, a, b in ((1, 0.08, 0.15), (77, 0.2, 0.3), (5, 0.12, 0.1))]
    sc["target"] = rng.random((3, H, W)).astype(np.float32)
    sc["noise"] = [rng.standard_normal((N, 3)).astype(np.float32) for _ in range(8)]
    return sc


NAMES = ("means", "sh0", "shN", "raw_scales", "raw_quats", "raw_opac")
LRS = (1e-3, 1e-2, 5e-4, 5e-3, 1e-3, 5e-2)
NOISE_LR = 0.8   # lr * noise_lr of mcmc.hpp is 1.6e-4 * 5e5 = 80 at the start of a run; the random scene has larger Gaussians than a trained one


def _adam_scalars(k, t):
    return (LRS[k], 0.9, 0.999, 1e-15, 1.0 / (1.0 - 0.9 ** t), 1.0 / np.sqrt(1.0 - 0.999 ** t))


def _train(lib, sc, form, steps, loss="mse", freeze=False, noise=False, shrink_on_step=None, capacity=None, opts_null=False, on_step=None):
    """form: "opt" (lfs_gut_train_step_opt) | "ex" (lfs_gut_train_step_ex) | "ref" (the composition of the split entry points).
    shrink_on_step: that step's FIRST attempt runs with a capacity of 8 entries; the state after it is recorded (`after_failed`) and the step is run again.
    A scene may name its own image size (sc["W"], sc["H"]) and have no background (sc["bg"] None); on_step(it, params, m, v, loss) is called after every step
    (tests/test_emulated_step_reference.py looks at each step through it)."""
    W, H = sc.get("W", globals()["W"]), sc.get("H", globals()["H"])
    ns = _defs()
    StepArgs, StepLayout, StepOptions = ns["StepArgs"], ns["StepLayout"], ns["StepOptions"]
    N = sc["means"].shape[0]
    capacity = capacity or 64 * N
    lay = StepLayout()
    assert lib.lfs_gut_step_layout_for(C.c_uint32(N), C.c_uint32(W), C.c_uint32(H), C.c_uint32(TILE), C.c_int64(capacity), C.byref(lay)) == 0
    ws = np.full(int(lay.bytes) + 64, 0xA5, np.uint8)             # garbage: the step must not rely on a clean workspace
    lws_bytes = int(lib.lfs_gut_step_loss_workspace_bytes(C.c_uint32(W), C.c_uint32(H)))
    pws_bytes = int(lib.lfs_photometric_loss_workspace_bytes(C.c_uint32(H), C.c_uint32(W)))
    assert lws_bytes >= pws_bytes + 12 * W * H
    lws = np.full(lws_bytes + 64, 0xA5, np.uint8)
    params = [np.ascontiguousarray(sc[k], np.float32).copy() for k in NAMES]
    m = [np.zeros_like(p) for p in params]
    v = [np.zeros_like(p) for p in params]
    grads = [np.zeros_like(p) for p in params]
    v_render = np.zeros((H, W, 3), np.float32)
    Km, target = [np.ascontiguousarray(sc[k], np.float32) for k in ("K", "target")]
    bg = None if sc["bg"] is None else np.ascontiguousarray(sc["bg"], np.float32)
    vms = sc["vms"]
    lossv = np.zeros(1, np.float32)
    out = dict(losses=[], fitted=[], rc=[], after_failed=None)
    colours_ready = False
    for it in range(steps):
        vm = vms[it % 3]
        a = StepArgs()
        a.N, a.K, a.sh_degree, a.image_width, a.image_height, a.tile_size = N, sc["Kn"], sc["degree"], W, H, TILE
        a.means, a.sh0, a.shN, a.raw_scales, a.raw_quats, a.raw_opacities = [p.ctypes.data for p in params]
        for k in range(6):
            for j, val in enumerate(_adam_scalars(k, it + 1)):
                a.adam[k][j] = val
        a.viewmat, a.Kmat, a.background = vm.ctypes.data, Km.ctypes.data, (None if bg is None else bg.ctypes.data)
        a.loss_weight, a.scale_reg, a.opacity_reg = 1.0, 0.01, 0.01
        nz = sc["noise"][it] if noise else None
        attempts = [8, capacity] if shrink_on_step == it else [capacity]
        for cap in attempts:
            counts = np.zeros(3, np.int64)
            tail = (C.c_int64(cap), C.c_int64(1 << 20), C.c_void_p(ws.ctypes.data), C.c_size_t(int(lay.bytes)), C.c_void_p(counts.ctypes.data), C.c_int64(it + 1), None)
            if form in ("opt", "ex"):
                for k in range(6):
                    if form == "opt" and freeze and k == 2:
                        continue                                  # (frozen: shN's moments may be NULL)
                    a.exp_avg[k], a.exp_avg_sq[k] = m[k].ctypes.data, v[k].ctypes.data
                a.target_chw, a.loss = target.ctypes.data, lossv.ctypes.data
                nxt = vms[(it + 1) % 3] if it + 1 < steps else None
                nxt_p = C.c_void_p(nxt.ctypes.data) if nxt is not None else None
                if form == "ex":
                    rc = lib.lfs_gut_train_step_ex(C.byref(a), nxt_p, C.c_int(int(colours_ready)), *tail)
                else:
                    o = StepOptions()
                    o.loss_kind, o.lambda_dssim, o.freeze_shN = (1 if loss == "l1_ssim" else 0), 0.2, int(freeze)
                    if nz is not None:
                        o.noise, o.noise_lr = nz.ctypes.data, NOISE_LR
                    o.loss_workspace, o.loss_workspace_bytes = lws.ctypes.data, lws_bytes
                    rc = lib.lfs_gut_train_step_opt(C.byref(a), None if opts_null else C.byref(o), nxt_p, C.c_int(int(colours_ready)), *tail)
                out["rc"].append(rc)
                if rc != 0:
                    return dict(out, params=params, m=m, v=v)
                fit = bool(lib.lfs_gut_step_fits(C.c_int64(int(counts[0])), C.c_int64(int(counts[1])), C.c_int64(cap), C.c_int64(1 << 20)))
                if fit:
                    colours_ready = nxt is not None and sc["Kn"] <= 16   # (the three-pass tail of degree 4 leaves no colours)
            else:
                lossv[0] = 0.0
                assert lib.lfs_gut_view_forward(C.byref(a), *tail) == 0
                fit = bool(lib.lfs_gut_step_fits(C.c_int64(int(counts[0])), C.c_int64(int(counts[1])), C.c_int64(cap), C.c_int64(1 << 20)))
                if fit:
                    gp = (C.c_void_p * 6)(*[g.ctypes.data for g in grads])
                    a.loss = lossv.ctypes.data
                    if loss == "l1_ssim":
                        render = ws[lay.render:lay.render + 12 * W * H]
                        assert lib.lfs_photometric_loss_fwd_bwd(C.c_uint32(H), C.c_uint32(W), C.c_void_p(render.ctypes.data), C.c_void_p(target.ctypes.data), C.c_float(0.2),
                                                                C.c_float(1.0), C.c_void_p(v_render.ctypes.data), C.c_void_p(lossv.ctypes.data), C.c_void_p(lws.ctypes.data),
                                                                C.c_size_t(pws_bytes), None) == 0
                        a.target_chw = None
                        vr = C.c_void_p(v_render.ctypes.data)
                    else:
                        a.target_chw = target.ctypes.data
                        vr = None
                    assert lib.lfs_gut_view_backward(C.byref(a), C.c_int64(cap), vr, gp, C.c_int(0), C.c_void_p(ws.ctypes.data), C.c_size_t(int(lay.bytes)), None) == 0
                    if nz is not None:   # mcmc.cpp:362-393: post_backward (noise) before the optimizer step
                        assert lib.lfs_add_noise(C.c_uint32(N), C.c_void_p(params[5].ctypes.data), C.c_void_p(params[3].ctypes.data), C.c_void_p(params[4].ctypes.data),
                                                 C.c_void_p(nz.ctypes.data), C.c_void_p(params[0].ctypes.data), C.c_float(NOISE_LR), None) == 0
                    groups = [k for k in range(6) if not (freeze and k == 2)]
                    ts = (AdamTensor * len(groups))()
                    for j, k in enumerate(groups):
                        ts[j].param, ts[j].exp_avg, ts[j].exp_avg_sq, ts[j].grad, ts[j].n_elements = (params[k].ctypes.data, m[k].ctypes.data, v[k].ctypes.data,
                                                                                                     grads[k].ctypes.data, params[k].size)
                        ts[j].lr, ts[j].beta1, ts[j].beta2, ts[j].eps, ts[j].bc1, ts[j].bc2 = _adam_scalars(k, it + 1)
                    assert lib.lfs_adam_step_multi(ts, C.c_int32(len(groups)), None) == 0
            out["fitted"].append(fit)
            if not fit:
                out["after_failed"] = dict(params=[p.copy() for p in params], m=[x.copy() for x in m], v=[x.copy() for x in v])
        out["losses"].append(float(lossv[0]))
        if on_step is not None:
            on_step(it, params, m, v, float(lossv[0]))
    return dict(out, params=params, m=m, v=v)


def _same_state(a, b):
    for k in range(6):
        assert np.array_equal(a["params"][k], b["params"][k]), NAMES[k]
        assert np.array_equal(a["m"][k], b["m"][k]) and np.array_equal(a["v"][k], b["v"][k]), NAMES[k]


@pytest.mark.parametrize("N", [65, 3000])
@pytest.mark.parametrize("K,degree", [(4, 1), (9, 2), (16, 3)])
@pytest.mark.parametrize("noise", [False, True], ids=["no_noise", "noise"])
@pytest.mark.parametrize("freeze", [0, 1], ids=["shN_updated", "shN_frozen"])
@pytest.mark.parametrize("loss", ["mse", "l1_ssim"])
def test_one_call_step_with_options_matches_the_split_composition_bit_for_bit(emu, loss, freeze, noise, K, degree, N):
    sc = _scene(1000 * K + N, N, K, degree)
    steps = 4
    ref = _train(emu, sc, "ref", steps, loss=loss, freeze=bool(freeze), noise=noise)
    new = _train(emu, sc, "opt", steps, loss=loss, freeze=bool(freeze), noise=noise)
    assert all(ref["fitted"]) and all(new["fitted"]) and new["rc"] == [0] * steps
    assert ref["losses"][0] > 0 and ref["losses"] == new["losses"]
    _same_state(ref, new)
    assert sum(int((ref["m"][k] != 0).sum()) for k in range(6)) > 50, "no gradient reached the parameters"
    if freeze:   # shN and its moments keep their bytes
        assert np.array_equal(new["params"][2], np.ascontiguousarray(sc["shN"], np.float32)) and not new["m"][2].any() and not new["v"][2].any()
    else:
        assert new["m"][2].any()
    if noise:    # ... and the noise did move the means (against the same run without it)
        quiet = _train(emu, sc, "opt", steps, loss=loss, freeze=bool(freeze), noise=False)
        assert not np.array_equal(quiet["params"][0], new["params"][0])


@pytest.mark.parametrize("K,degree", [(4, 1), (16, 3)])
def test_null_and_all_zero_options_are_the_fused_tail_step(emu, K, degree):
    sc = _scene(31 + K, 400, K, degree)
    ex = _train(emu, sc, "ex", 3)
    for opts_null in (True, False):
        new = _train(emu, sc, "opt", 3, opts_null=opts_null)
        assert new["rc"] == [0, 0, 0] and ex["losses"] == new["losses"] and ex["losses"][0] > 0
        _same_state(ex, new)


@pytest.mark.parametrize("loss", ["mse", "l1_ssim"])
def test_attempt_that_does_not_fit_applies_nothing_not_even_the_noise(emu, loss):
    sc = _scene(77, 500, 16, 3)
    ref = _train(emu, sc, "ref", 3, loss=loss, noise=True)
    new = _train(emu, sc, "opt", 3, loss=loss, noise=True, shrink_on_step=1)
    assert new["fitted"] == [True, False, True, True]
    one = _train(emu, sc, "opt", 1, loss=loss, noise=True)
    # (the one-step run names no next view, the three-step run does: the parameters cannot tell)
    _same_state(one, new["after_failed"])
    assert ref["losses"] == new["losses"]
    _same_state(ref, new)
    # ... and with shN frozen on top
    ref = _train(emu, sc, "ref", 2, loss=loss, noise=True, freeze=True)
    new = _train(emu, sc, "opt", 2, loss=loss, noise=True, freeze=True, shrink_on_step=0)
    assert new["fitted"] == [False, True, True]
    for k, name in enumerate(NAMES):
        assert np.array_equal(new["after_failed"]["params"][k], np.ascontiguousarray(sc[name], np.float32)), name
        assert not new["after_failed"]["m"][k].any() and not new["after_failed"]["v"][k].any()
    _same_state(ref, new)


@pytest.mark.parametrize("freeze,noise", [(True, False), (False, True), (True, True)])
def test_degree_4_with_freeze_or_noise_is_unsupported_and_changes_nothing(emu, freeze, noise):
    sc = _scene(5, 300, 25, 4)
    new = _train(emu, sc, "opt", 1, loss="l1_ssim", freeze=freeze, noise=noise)
    assert new["rc"] == [LFS_E_UNSUPPORTED]
    for k, name in enumerate(NAMES):
        assert np.array_equal(new["params"][k], np.ascontiguousarray(sc[name], np.float32)), name
        assert not new["m"][k].any() and not new["v"][k].any()


def test_degree_4_with_the_photometric_loss_alone_takes_the_three_pass_tail(emu):
    sc = _scene(6, 300, 25, 4)
    ref = _train(emu, sc, "ref", 2, loss="l1_ssim")
    new = _train(emu, sc, "opt", 2, loss="l1_ssim")
    assert new["rc"] == [0, 0] and ref["losses"] == new["losses"]
    _same_state(ref, new)
