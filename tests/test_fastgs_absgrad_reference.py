"""CPU: the host model of the absgrad densification signal (tests/fastgs_absgrad_reference.py) is held to the oracle, and the scenes and seeds of the GPU tests
(tests/test_gpu_fastgs_absgrad.py) are held to the conditions those tests rest on: each contains what it is there for, and a float32 evaluation of the model stays
within the three flip rows of rows_check(bar=1e-3) against the float64 one - the budget the GPU comparison is given."""
import numpy as np
import pytest

from fastgs_absgrad_reference import (CFGS, SCENE_IDS, VARIANT_SCENES, VARIANTS, absgrad_model, model_of, oracle_forward, scene, single_gaussian_scene, upstream,
                                      variant_model)
from gpu_util import rows_check


@pytest.mark.parametrize("idx", range(len(CFGS)), ids=SCENE_IDS)
def test_signed_sums_of_the_model_reproduce_the_oracles_densification_info(oracle_mod, idx):
    sc = scene(idx)
    gi, ga = upstream(sc)
    f64 = oracle_forward(oracle_mod, sc, np.float64)
    m = absgrad_model(f64, gi, ga, sc["W"], sc["H"])
    og = oracle_mod.fastgs_backward(f64, sc["means"], sc["scales_raw"], sc["rot_raw"], sc["opac_raw"], sc["sh0"], sc["sh_rest"], sc["w2c"], sc["cam_pos"],
                                    sc["active_sh_bases"], sc["W"], sc["H"], sc["fx"], sc["fy"], sc["cx"], sc["cy"], gi, ga, dtype=np.float64)
    dens = og[6]
    assert np.array_equal(dens[0], m["dens_signed"][0]) and dens[0].sum() > 0
    err = np.abs(dens[1] - m["dens_signed"][1]).max() / np.abs(dens[1]).max()
    print(f"signed norms, model vs oracle.fastgs_backward (float64): max |diff| / max {err:.2e} (<= 1e-12), {m['instances']} instances")
    assert err <= 1e-12
    # |sum| <= sum |.| per component, so the absgrad norm is never below the default one
    assert (m["dens_abs"][1] >= m["dens_signed"][1] * (1 - 1e-12)).all() and m["dens_abs"][1].sum() > m["dens_signed"][1].sum()


@pytest.mark.parametrize("idx", range(len(CFGS)), ids=SCENE_IDS)
def test_scenes_contain_what_they_are_there_for_and_stay_within_the_flip_budget(oracle_mod, idx):
    sc = scene(idx)
    N = CFGS[idx]["N"]
    gi, ga = upstream(sc)
    f64 = oracle_forward(oracle_mod, sc, np.float64)
    b = f64["bounds"][0]
    tiles0 = int(f64["n_touched"][0])
    print(f"Gaussian 0: bounds {b}, n_touched {tiles0}")
    assert tiles0 >= 4                                                    # (a) its row is summed across wavefronts
    if N >= 2:
        assert f64["n_touched"][1] == 0                                   # (c)
    if N >= 200:                                                          # (b) pixels that stop before the end of their tile list
        gw = (sc["W"] + 15) // 16
        py, px = np.divmod(np.arange(sc["W"] * sc["H"]), sc["W"])
        t = (py // 16) * gw + px // 16
        length = (f64["offsets"][1:] - f64["offsets"][:-1])[t]
        nc = f64["n_contrib"].reshape(-1)
        early = int(((nc > 0) & (nc < length) & (f64["alpha"].reshape(-1) > 0.999)).sum())
        print(f"pixels terminated early by the opaque stack: {early}")
        assert early >= 16
    for label, g in (("random", (gi, ga)), ("uniform", (np.ones_like(gi), np.zeros_like(ga)))):
        m64 = model_of(oracle_mod, (idx, label), sc, *g)
        m32 = model_of(oracle_mod, (idx, label), sc, *g, dtype=np.float32)
        assert np.array_equal(m32["dens_abs"][0], m64["dens_abs"][0])
        e, flips, rest = rows_check(m32["dens_abs"][1][:, None], m64["dens_abs"][1][:, None], bar=1e-3, max_flips=3)
        print(f"{label} gradients: float32 model vs float64 model rel-L2 {e:.2e}, flip rows {flips}, without them {rest:.2e} (< 1e-3)")
        assert rest < 1e-3, (label, e, flips, rest)


def test_a_gaussian_on_a_pixel_corner_cancels_in_the_signed_sum_only(oracle_mod):
    """the cancellation scene of the GPU tests: centre exactly on a pixel corner in the interior of a tile, uniform positive gradient, black background - the signed
    sums vanish by symmetry, the absolute ones do not"""
    sc = single_gaussian_scene(64, 48, (24.0, 24.0))
    f64 = oracle_forward(oracle_mod, sc, np.float64)
    assert abs(f64["mean2d"][0, 0] - 24.0) < 1e-9 and abs(f64["mean2d"][0, 1] - 24.0) < 1e-9 and abs(f64["conic_opacity"][0, 1]) < 1e-12
    m = absgrad_model(f64, np.ones((3, 48, 64)), np.zeros((1, 48, 64)), 64, 48)
    print(f"signed norm {m['dens_signed'][1, 0]:.3e}, absgrad norm {m['dens_abs'][1, 0]:.3e}")
    assert m["dens_abs"][1, 0] > 0 and m["dens_signed"][1, 0] < 1e-9 * m["dens_abs"][1, 0]


@pytest.mark.parametrize("variant", VARIANTS[1:])
@pytest.mark.parametrize("idx", VARIANT_SCENES, ids=SCENE_IDS)
def test_the_other_forms_stay_within_the_flip_budget(oracle_mod, idx, variant):
    m64, m32 = variant_model(oracle_mod, idx, variant), variant_model(oracle_mod, idx, variant, np.float32)
    plain = variant_model(oracle_mod, idx, "plain")
    assert np.array_equal(m32["dens_abs"][0], m64["dens_abs"][0])
    e, flips, rest = rows_check(m32["dens_abs"][1][:, None], m64["dens_abs"][1][:, None], bar=1e-3, max_flips=3)
    moved = float(np.linalg.norm(m64["dens_abs"][1] - plain["dens_abs"][1]) / np.linalg.norm(plain["dens_abs"][1]))
    print(f"{variant}: float32 model vs float64 model rel-L2 {e:.2e}, flip rows {flips}, without them {rest:.2e} (< 1e-3); the form moves the norms by {moved:.2e} (> 1e-2)")
    assert rest < 1e-3 and moved > 1e-2, (variant, e, flips, rest, moved)
