"""The one-call training step (lfs_gut_train_step_opt), the fused-tail step (lfs_gut_train_step_ex) and the composition of the split entry points, on the wavefront
emulator (tests/emul_util.py), against tests/step_reference.py: a plain float64 PyTorch model of the step written from the reference's sources and differentiated by
torch.autograd alone. The other tests of these entry points (tests/test_emulated_step_options.py) hold them bit for bit to each other; this file holds them to something
that shares neither the kernels' nor the oracle's reading of the maths: a regulariser's normalisation, the clamp mask, the quaternion-normalisation term, the handed-over
SH colours and the order of noise and Adam all show here. Every step of a run is checked (tests/step_reference_checks.py: gradients teacher-forced through the moments,
the loss value, the update, exact zeros on unlisted rows and clamped colours), with three views taking turns, so that every step after the first renders with the colours
the previous tail handed over. The update's margins are those of profiles/r08/step_reference_margins.json."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import step_reference as R  # noqa: E402
import step_reference_checks as chk  # noqa: E402
from test_emulated_step_options import _train, emu  # noqa: E402,F401

GOLD = os.path.join(HERE, "golden")


def test_reference_sh_basis_reproduces_the_reference_codes_output():
    """tests/golden/sh_fwd.npz is the output of the reference's own spherical_harmonics (fp32): the float64 basis of step_reference.py lies within fp32 rounding of it -
    a few ulp of the largest colour per degree (the sum of up to 25 products of magnitude <= 1 each rounded at 6e-8: 25 x 6e-8 x max|coefficient| < 5e-6)"""
    g = np.load(os.path.join(GOLD, "sh_fwd.npz"))
    for deg in range(5):
        got = R.spherical_harmonics(deg, torch.from_numpy(g["dirs"]).double(), torch.from_numpy(g[f"coeffs{deg}"]).double()).numpy()
        want = g[f"colors{deg}"]
        assert got.shape == want.shape
        assert np.abs(got - want).max() < 5e-6 * max(1.0, np.abs(g[f"coeffs{deg}"]).max()), (deg, np.abs(got - want).max())


def test_reference_adam_and_noise_are_the_float64_limit_of_the_oracles():
    """oracle.adam_step / oracle.add_noise have float64 builds: the PyTorch formulas of step_reference.py agree with them to float64 rounding (the oracle is not the
    source of the formulas - the reference's adam_kernels.cuh and RelocationCUDA.cu are - but a typo in either would show)"""
    import oracle
    rng = np.random.default_rng(3)
    p, m, g = rng.standard_normal((3, 500))
    v = rng.random(500) * 1e-2
    lr, b1, b2, eps = 1e-2, 0.9, 0.999, 1e-15
    bc1, bc2 = R.adam_scalars(b1, b2, 7)
    p1, m1, v1 = oracle.adam_step(p, m, v, g, lr, b1, b2, eps, bc1, bc2, dtype=np.float64)
    mm, vv = R.adam_moments(torch.from_numpy(m), torch.from_numpy(v), torch.from_numpy(g), b1, b2)
    np.testing.assert_allclose(mm.numpy(), m1, rtol=1e-13)
    np.testing.assert_allclose(vv.numpy(), v1, rtol=1e-13)
    np.testing.assert_allclose(p + R.adam_delta(mm, vv, lr, eps, bc1, bc2).numpy(), p1, rtol=1e-12, atol=1e-15)
    ro, rs, rq, nz, mu = rng.standard_normal(200) * 3 - 3, rng.standard_normal((200, 3)) - 2, rng.standard_normal((200, 4)), rng.standard_normal((200, 3)), rng.standard_normal((200, 3))
    moved = oracle.add_noise(ro, rs, rq, nz, mu, 0.8, dtype=np.float64)
    shift = R.noise_term(*[torch.from_numpy(x) for x in (ro, rs, rq, nz)], 0.8).numpy()
    np.testing.assert_allclose(mu + shift, moved, rtol=1e-12, atol=1e-15)
    assert np.abs(shift).max() > 1e-3


def _run(emu, sc, form, steps, loss, freeze, noise, label, guard=True):
    import oracle
    state = dict(params=[np.ascontiguousarray(sc[k], np.float32).copy() for k in chk.NAMES],
                 m=[np.zeros_like(np.ascontiguousarray(sc[k], np.float32)) for k in chk.NAMES],
                 v=[np.zeros_like(np.ascontiguousarray(sc[k], np.float32)) for k in chk.NAMES])
    seen = []

    def on_step(it, params, m, v, loss_value):
        after = dict(params=[x.copy() for x in params], m=[x.copy() for x in m], v=[x.copy() for x in v])
        chk.check_step(oracle, f"{label} {form}", sc, it, dict(state), after, loss_value, loss, bool(freeze), sc["noise"][it] if noise else None, guard=guard)
        state.update(after)
        seen.append(it)

    out = _train(emu, sc, form, steps, loss=loss, freeze=bool(freeze), noise=noise, on_step=on_step)
    assert out["rc"] == ([0] * steps if form != "ref" else [])
    assert all(out["fitted"]) and seen == list(range(steps))
    return out


@pytest.mark.parametrize("N", [65, 3000])
@pytest.mark.parametrize("K,degree", [(1, 0), (4, 1), (16, 3)])
@pytest.mark.parametrize("noise", [False, True], ids=["no_noise", "noise"])
@pytest.mark.parametrize("freeze", [0, 1], ids=["shN_updated", "shN_frozen"])
@pytest.mark.parametrize("loss", ["mse", "l1_ssim"])
def test_one_call_step_against_the_float64_autograd_model(emu, loss, freeze, noise, K, degree, N):
    """K = 1 (no shN at all): the one-call forms do not take such a model (csrc/gut_step.hip: "degree-0-only models take the gradient-tensor step" - see
    test_one_call_forms_refuse_a_model_without_shN), so these cases run the split composition with the same loss, freeze and noise."""
    sc = chk.make_scene(2000 * K + N, N, K, degree)
    _run(emu, sc, "opt" if K > 1 else "ref", 4 if N == 65 else 3, loss, freeze, noise, f"{loss} freeze={freeze} noise={noise} K={K} N={N}")


@pytest.mark.parametrize("form", ["opt", "ex"])
def test_one_call_forms_refuse_a_model_without_shN(emu, form):
    sc = chk.make_scene(2065, 65, 1, 0)
    out = _train(emu, sc, form, 1, loss="mse" if form == "ex" else "l1_ssim")
    assert out["rc"] == [-1]   # LFS_E_INVALID
    for k, name in enumerate(chk.NAMES):
        assert np.array_equal(out["params"][k], np.ascontiguousarray(sc[name], np.float32)) and not out["m"][k].any() and not out["v"][k].any(), name


@pytest.mark.parametrize("form", ["ex", "ref"])
@pytest.mark.parametrize("K,degree,N", [(4, 1, 65), (4, 1, 3000), (16, 3, 3000)])
def test_fused_tail_step_and_split_composition_against_the_float64_autograd_model(emu, form, K, degree, N):
    """lfs_gut_train_step_ex (the MSE step without options) and the split entry points (forward | backward into gradient tensors | Adam) on the same scenes"""
    sc = chk.make_scene(2000 * K + N, N, K, degree)
    _run(emu, sc, form, 3, "mse", 0, False, f"mse K={K} N={N}")


@pytest.mark.parametrize("form,loss,freeze,noise", [("opt", "l1_ssim", 1, True), ("ref", "l1_ssim", 0, True), ("ex", "mse", 0, False)])
def test_ragged_image_without_background(emu, form, loss, freeze, noise):
    """203 x 117: partial tiles on both edges; no background pointer"""
    sc = chk.make_scene(11, 3000, 16, 3, W=203, H=117, background=False)
    _run(emu, sc, form, 3, loss, freeze, noise, f"ragged {loss}")


@pytest.mark.parametrize("form,loss,freeze,noise", [("opt", "l1_ssim", 0, True), ("opt", "mse", 1, False)])
def test_dense_scene_with_early_termination(emu, form, loss, freeze, noise):
    """1500 large Gaussians close together at 128 x 128: most pixels end on the transmittance threshold long before their tile list does"""
    sc = chk.make_scene(19, 1500, 16, 3, W=128, H=128, spread=0.4, smin=0.05, smax=0.3)
    _run(emu, sc, form, 3, loss, freeze, noise, f"dense {loss}")
