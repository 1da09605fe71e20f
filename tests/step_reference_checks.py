"""What tests/test_emulated_step_reference.py and tests/test_gpu_step_reference.py share: the scenes (with their degenerate rows), the tile lists of the oracle's
projection, the fp32 ORACLE composition that guards the inputs, and the per-step checks of a training step against tests/step_reference.py (float64, autograd).

A step is checked TEACHER-FORCED: the reference is evaluated at the parameters the step started from, and its gradient is compared with the gradient the step must
have used - recovered from its first moments, g = (m_k - b1 m_{k-1}) / (1 - b1), and g^2 from the second ones - so that nothing drifts over the steps of a run.

Bars. Gradients: gpu_util.rows_check at the project's backward bar (2e-4, at most two flip rows: tests/test_gpu_raster.py); the fp32 oracle composition has to pass the
same check with NO row set aside on every scene (a guard on the inputs: a scene on which plain fp32 arithmetic itself misses the bar says nothing about the kernels).
Loss value: 2e-6 absolute (tests/test_gpu_loss.py). Update: four times the distance of the fp32 oracle (oracle.adam_step, oracle.add_noise) from the float64 formula
on the same kind of inputs, recorded in profiles/r08/step_reference_margins.json (the builds differ in __expf and contraction: hence the factor).
Rows where the reference gives exact zeros (Gaussians the projection did not list - raw opacity -6, behind the camera -, colour channels clamped at 0) are compared
exactly: their first moments are b1 * m_{k-1} to the bit."""
import json
import os

import numpy as np
import torch

import step_reference as R
from gpu_util import make_gaussians, pinhole_K, rows_check, small_rotation_viewmat

HERE = os.path.dirname(os.path.abspath(__file__))
MARGINS_FILE = os.path.join(os.path.dirname(HERE), "profiles", "r08", "step_reference_margins.json")
RECORD = os.environ.get("LFS_STEP_REFERENCE_RECORD", "")   # development: append one JSON line per checked step (how the margins file was measured)

NAMES = ("means", "sh0", "shN", "raw_scales", "raw_quats", "raw_opac")
LRS = (1e-3, 1e-2, 5e-4, 5e-3, 1e-3, 5e-2)
B1, B2, EPS = 0.9, 0.999, 1e-15
NOISE_LR = 0.8
LAMBDA, WEIGHT, SCALE_REG, OPACITY_REG = 0.2, 1.0, 0.01, 0.01
TILE = 16
GRAD_BAR, MAX_FLIPS, LOSS_BAR = 2e-4, 2, 2e-6
# a gradient that is the regulariser's alone, recovered from fp32 moments: eps32 (6e-8) x 10 (the division by 1 - b1) x the few roundings of exp / sigmoid and the product
REG_ONLY_RTOL = 1e-5
VIEWS = ((1, 0.08, 0.15), (77, 0.2, 0.3), (5, 0.12, 0.1))


def make_scene(seed, N, K, degree, W=64, H=48, spread=1.0, smin=0.02, smax=0.12, background=True):
    """Random Gaussians in front of three nearby cameras, with the rows that hit masks and edges: ~10 % raw opacity -6 (below 1/255: never listed), ~4 % behind the
    camera, ~5 % with colours driven negative (sh0 = -8: clamped at 0, no SH gradient) and ~5 % above 1 (sh0 = +3: the render leaves [0, 1], the loss clamps it)."""
    rng = np.random.default_rng(seed)
    means, quats, scales, opac = make_gaussians(rng, N, spread=spread, smin=smin, smax=smax)
    raw_opac = np.log(opac / (1 - opac)).astype(np.float32)
    faint = rng.random(N) < 0.1
    raw_opac[faint] = -6.0
    behind = rng.random(N) < 0.04
    means[behind, 2] = -means[behind, 2]
    sh0 = (rng.standard_normal((N, 1, 3)) * 0.5).astype(np.float32)
    dark, bright = rng.random(N) < 0.05, rng.random(N) < 0.05
    sh0[dark], sh0[bright & ~dark] = -8.0, 3.0
    sc = dict(means=means, raw_quats=quats, raw_scales=np.log(scales).astype(np.float32), raw_opac=raw_opac, sh0=sh0,
              shN=(rng.standard_normal((N, K - 1, 3)) * 0.2).astype(np.float32), K=pinhole_K(0.8 * W, W, H, 1)[0],
              bg=rng.random(3).astype(np.float32) if background else None, Kn=K, degree=degree, W=W, H=H, faint=faint, behind=behind, dark=dark)
    sc["vms"] = [np.ascontiguousarray(small_rotation_viewmat(np.random.default_rng(s), a, b), np.float32) for s, a, b in VIEWS]
    sc["target"] = rng.random((3, H, W)).astype(np.float32)
    sc["noise"] = [rng.standard_normal((N, 3)).astype(np.float32) for _ in range(8)]
    return sc


def adam_scalars(k, t):
    return (LRS[k], B1, B2, EPS, 1.0 / (1.0 - B1 ** t), 1.0 / np.sqrt(1.0 - B2 ** t))


# ---- the oracle's part: tile lists (inputs of the reference) and the fp32 composition (the guard) ---------------------------------------------------------------
def _activated(params):
    raw_q, raw_s, raw_o = params[4], params[3], params[5]
    qn = np.linalg.norm(raw_q, axis=-1, keepdims=True)
    return raw_q / qn, qn, np.exp(raw_s), 1 / (1 + np.exp(-raw_o))


def tile_lists(o, params, vm, K, W, H):
    """the oracle's projection + intersect_tile / intersect_offset on fp32 parameters (pinned bit-exact to the kernels' elsewhere) -> offsets, flatten_ids, visible"""
    quats, _, scales, opac = _activated(params)
    radii, m2, d, _, _ = o.projection_ut_3dgs_fused(params[0], quats, scales, opac, vm[None], None, K[None], W, H)
    tw, th = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    _, ids, flat = o.intersect_tile(m2, radii, d, 1, TILE, tw, th, True)
    offs = o.intersect_offset(ids, 1, tw, th)
    return offs, flat, (radii[0] > 0).all(-1)


def oracle_gradients(o, params, degree, vm, K, bg, W, H, target, kind, lists, lam=LAMBDA, scale_reg=SCALE_REG, opacity_reg=OPACITY_REG):
    """One step's loss and gradients w.r.t. the raw parameters from the fp32 oracle (tests/test_gpu_pipeline.py::_oracle_step, with the background, the regularisers
    and L1 + D-SSIM - dL/d(image) of that loss from fp32 autograd over tests/ssim_reference.py)"""
    offs, flat, mask = lists
    means = params[0]
    quats, qn, scales, opac = _activated(params)
    N = means.shape[0]
    sh = np.concatenate([params[1], params[2]], 1)
    dirs = means - np.linalg.inv(vm.astype(np.float64))[:3, 3].astype(np.float32)
    col = o.spherical_harmonics_fwd(degree, dirs, sh, mask)
    colors = np.maximum(col + 0.5, 0)[None]
    bgs = None if bg is None else bg[None]
    geo = (W, H, TILE, vm[None], None, K[None], 0, 4, None, None, None, offs, flat)
    rc, ra, li = o.rasterize_fwd(means, quats, scales, colors, opac[None], bgs, None, *geo)
    img_raw = torch.from_numpy(np.ascontiguousarray(rc[0].transpose(2, 0, 1))).requires_grad_(True)
    loss = WEIGHT * R.photometric(img_raw.clamp(0, 1), torch.from_numpy(target), kind, lam)   # (fp32: its |x| takes whichever side its own render lands on)
    v_img, = torch.autograd.grad(loss, img_raw)
    v_rc = np.ascontiguousarray(v_img.numpy().transpose(1, 2, 0))[None].astype(np.float32)
    gm, gq, gs, gc, go = o.rasterize_bwd(means, quats, scales, colors, opac[None], bgs, None, *geo, ra, li, v_rc, np.zeros_like(ra))
    g_col = np.where(col + 0.5 > 0, gc[0], 0).astype(np.float32)
    g_sh, g_dirs = o.spherical_harmonics_bwd(degree, dirs, sh, mask, g_col, True)
    g_raw_o = (go[0] + np.float32(opacity_reg / N)) * opac * (1 - opac)
    g_raw_s = (gs + np.float32(scale_reg / (3 * N))) * scales
    g_raw_q = (gq - (gq * quats).sum(-1, keepdims=True) * quats) / qn
    return [gm + g_dirs, g_sh[:, :1], g_sh[:, 1:], g_raw_s, g_raw_q, g_raw_o], float(loss.detach())


# ---- the checks -------------------------------------------------------------------------------------------------------------------------------------------------
def _f32c(x):
    return np.float64(np.float32(x))


def recovered_gradients(before, after, k):
    """-> (g, g^2) the step used for tensor k, from its moments (float64 arithmetic on the fp32 values and the fp32 constants of the kernel)"""
    b1, b2 = _f32c(B1), _f32c(B2)
    one_b1, one_b2 = np.float64(np.float32(1) - np.float32(B1)), np.float64(np.float32(1) - np.float32(B2))
    g = (after["m"][k].astype(np.float64) - b1 * before["m"][k]) / one_b1
    g2 = (after["v"][k].astype(np.float64) - b2 * before["v"][k]) / one_b2
    return g, g2


def update_distance(p_before, p_after, delta64):
    """max over elements of |(p_k - p_{k-1}) - delta64| / (|p_{k-1}| + |delta64|): in units of the rounding of an fp32 parameter and of its step"""
    if p_before.size == 0:
        return 0.0
    d = p_after.astype(np.float64) - p_before.astype(np.float64)
    return float((np.abs(d - delta64) / (np.abs(p_before) + np.abs(delta64) + 1e-300)).max())


def margins():
    with open(MARGINS_FILE) as f:
        return json.load(f)["margin"]


def check_step(o, label, sc, it, before, after, loss_value, kind, freeze, noise, guard=True, grad_check=None, adam=None, noise_lr=NOISE_LR, lam=LAMBDA,
               scale_reg=SCALE_REG, opacity_reg=OPACITY_REG, update=True):
    """before / after: dict(params=[6], m=[6], v=[6]) of fp32 numpy arrays around step `it` (0-based; view it % 3). noise: the step's draw [N,3] or None.
    adam(k) -> (lr, b1, b2, eps, bc1_rcp, bc2_sqrt_rcp) of tensor k in this step (default: adam_scalars(k, it + 1), the emulated driver's).
    grad_check(name, what, a, ref): replaces the rows_check assertion of the gradients (the float-atomics GPU case passes its own bar)."""
    adam = adam or (lambda k: adam_scalars(k, it + 1))
    W, H, degree, N = sc["W"], sc["H"], sc["degree"], sc["means"].shape[0]
    vm, K, bg, target = sc["vms"][it % 3], sc["K"], sc["bg"], sc["target"]
    p0 = [np.ascontiguousarray(p, np.float32) for p in before["params"]]
    lists = tile_lists(o, p0, vm, K, W, H)
    offs, flat, visible = lists
    assert len(flat) > 0, label
    grads_t, photo, render, free = R.step_gradients([torch.from_numpy(p) for p in p0], degree, torch.from_numpy(vm), torch.from_numpy(K),
                                            None if bg is None else torch.from_numpy(bg), W, H, TILE, offs[0], flat, torch.from_numpy(visible),
                                            torch.from_numpy(target), kind=kind, lambda_dssim=lam, weight=WEIGHT, scale_reg=scale_reg, opacity_reg=opacity_reg)
    report = dict(label=label, step=it, grad={}, update={}, undecided=len(free))
    if free:
        print(f"{label} step {it}: {len(free)} element(s) of the L1 term within {R.L1_TAU} of 0: their sign is left to the implementation")
    skip = [k for k, name in enumerate(NAMES) if (freeze and k == 2) or (name == "shN" and degree == 0)]
    as_np = lambda gs: [g.numpy() for g in gs]

    grads = as_np(grads_t)

    # (0) the edges are there: unlisted rows of both kinds, a clamped loss
    assert (sc["faint"] & ~visible).sum() == sc["faint"].sum() and (sc["behind"] & ~visible).sum() == sc["behind"].sum(), label
    assert float(render.max()) > 1.0 or N < 100, (label, "no render value outside [0, 1]")

    # (1) the guard: the fp32 oracle composition against the reference, no row set aside
    if guard:
        og, oloss = oracle_gradients(o, p0, degree, vm, K, bg, W, H, target, kind, lists, lam, scale_reg, opacity_reg)
        grads = as_np(R.fit_free(og, grads_t, free))
        assert abs(oloss - photo) < LOSS_BAR, (label, "guard: oracle loss", oloss, photo)
        for k, name in enumerate(NAMES):
            if grads[k].size == 0 or (name == "shN" and degree == 0):
                continue
            for what, a, ref in (("g", og[k], grads[k]), ("g2", og[k].astype(np.float64) ** 2, grads[k] ** 2)):
                total, flips, rest = rows_check(a, ref, bar=GRAD_BAR, max_flips=MAX_FLIPS)
                report["grad"][f"oracle {name} {what}"] = total
                assert flips == 0 and total < GRAD_BAR, (label, "guard: the fp32 oracle misses the bar on this scene", name, what, total, flips, rest)

    grads = as_np(R.fit_free([recovered_gradients(before, after, k)[0] for k in range(6)], grads_t, free, skip))

    # (2) loss value
    print(f"{label} step {it}: loss {loss_value:.8f} reference {photo:.8f}")
    assert abs(loss_value - photo) < LOSS_BAR, (label, it, loss_value, photo)

    # (3) gradients, teacher-forced
    unlisted = ~visible
    for k, name in enumerate(NAMES):
        if grads[k].size == 0:
            continue
        if freeze and k == 2:   # counted, not updated: parameter and moments keep their bytes
            for key in ("params", "m", "v"):
                assert np.array_equal(before[key][k], after[key][k]), (label, it, "frozen shN", key)
            continue
        g, g2 = recovered_gradients(before, after, k)
        ref = grads[k]
        if name == "shN" and degree == 0:   # coefficients beyond the active degree take no part
            assert not ref.any() and not after["m"][k].any() and not after["v"][k].any(), (label, it, name)
            continue
        for what, a, r in (("g", g, ref), ("g2", g2, ref ** 2)):
            total, flips, rest = rows_check(a, r, bar=GRAD_BAR, max_flips=MAX_FLIPS)
            print(f"{label} step {it}: {name} {what} rel L2 {total:.3e}, {flips} rows set aside -> {rest:.3e}")
            report["grad"][f"{name} {what}"] = (total, flips, rest)
            if grad_check is not None:
                grad_check(name, what, a, r)
            else:
                assert rest < GRAD_BAR, (label, it, name, what, total, flips, rest)
        # exact zeros of the reference: the moments only decay (lfs_adam.cuh: un-fused IEEE, b1 * m + (1 - b1) * 0)
        zero = np.zeros(ref.shape, bool)
        reg = {"raw_scales": scale_reg, "raw_opac": opacity_reg}.get(name, 0.0)
        if reg == 0:   # (every tensor but the two with a regulariser - and those too when it is switched off)
            zero[unlisted] = True
            assert not ref[unlisted].any(), (label, name, "the reference has a gradient on an unlisted row")
        if name in ("sh0", "shN"):
            with torch.no_grad():
                col = R.spherical_harmonics(degree, torch.from_numpy(p0[0]).double() - torch.linalg.inv(torch.from_numpy(vm).double())[:3, 3],
                                            torch.from_numpy(np.concatenate([p0[1], p0[2]], 1)).double()).numpy() + 0.5
            clamped = visible[:, None] & (col < -1e-3)                 # (clearly below 0: fp32 and float64 agree on the side)
            assert clamped[sc["dark"] & visible].all(), label
            cl = np.broadcast_to(clamped[:, None, :], ref.shape)
            assert not ref[cl].any(), (label, name, "the reference has an SH gradient on a clamped channel")
            zero |= cl
        if zero.any():
            assert np.array_equal(after["m"][k][zero], np.float32(B1) * before["m"][k][zero]), (label, it, name, "first moment where the reference's gradient is exactly 0")
            assert np.array_equal(after["v"][k][zero], np.float32(B2) * before["v"][k][zero]), (label, it, name, "second moment where the reference's gradient is exactly 0")
        if reg > 0 and unlisted.any():       # unlisted rows receive the regulariser's gradient and nothing else
            # (+ what the recovery itself loses where an earlier view left a large moment: m_k and the two products it is the sum of are rounded at 2^-24 |m| each)
            slack = 4 * 2.0 ** -24 * np.maximum(np.abs(after["m"][k]), np.abs(before["m"][k])).astype(np.float64)[unlisted] / (1 - B1)
            miss = np.abs(g[unlisted] - ref[unlisted]) - REG_ONLY_RTOL * np.abs(ref[unlisted]) - slack
            assert (miss <= 0).all(), (label, it, name, "regulariser on unlisted rows", float(miss.max()))
            assert (ref[unlisted] > 0).all()

    # (4) update: p_k - p_{k-1} against float64 Adam on the step's own new moments (+ the float64 noise on the means)
    t64 = [torch.from_numpy(p).double() for p in p0]
    if not update:
        return report
    nz = None if noise is None else np.ascontiguousarray(noise, np.float32)
    recorded = None if RECORD else margins()
    for k, name in enumerate(NAMES):
        if p0[k].size == 0 or (freeze and k == 2):
            continue
        lr, b1, b2, eps, bc1, bc2 = [float(np.float32(x)) for x in adam(k)]
        m1, v1 = torch.from_numpy(after["m"][k]).double(), torch.from_numpy(after["v"][k]).double()
        delta = R.adam_delta(m1, v1, lr, eps, bc1, bc2)
        if k == 0 and nz is not None:
            shift = R.noise_term(t64[5], t64[3], t64[4], torch.from_numpy(nz).double(), float(np.float32(noise_lr)))
            assert float(shift[torch.from_numpy(sc["faint"])].abs().min()) > 0     # the faint rows are the ones the noise moves most
            delta = delta + shift
        d_dev = update_distance(p0[k], after["params"][k], delta.numpy())
        # the fp32 oracle on the same inputs: noise, then Adam with the gradient the step used (its moments then are the step's, to rounding)
        p_or = p0[k] if not (k == 0 and nz is not None) else o.add_noise(p0[5], p0[3], p0[4], nz, p0[0], noise_lr)
        g32 = recovered_gradients(before, after, k)[0].astype(np.float32)
        p_or, m_or, v_or = o.adam_step(p_or, before["m"][k], before["v"][k], g32, lr, b1, b2, eps, bc1, bc2)
        delta_or = R.adam_delta(torch.from_numpy(m_or).double(), torch.from_numpy(v_or).double(), lr, eps, bc1, bc2)
        if k == 0 and nz is not None:
            delta_or = delta_or + shift
        d_or = update_distance(p0[k], p_or, delta_or.numpy())
        # four times the fp32 oracle's own distance: on this step's inputs, and not below its (recorded) maximum over the emulated grid - on 65 Gaussians the oracle can
        # happen to round like float64 everywhere, which says nothing about a build with another exp
        bar = 4.0 * d_or if recorded is None else max(4.0 * d_or, recorded[name + ("+noise" if k == 0 and nz is not None else "")])
        print(f"{label} step {it}: update {name} distance {d_dev:.3e} (fp32 oracle {d_or:.3e}, bar {bar:.3e})")
        report["update"][name + ("+noise" if k == 0 and nz is not None else "")] = (d_dev, d_or)
        assert d_dev <= bar, (label, it, name, "update", d_dev, d_or, bar)
    if RECORD:
        with open(RECORD, "a") as f:
            f.write(json.dumps(report) + "\n")
    return report
