"""GPU: grad_w2c, the camera gradient of the fastgs backward that the reference's pose optimisation trains on (grad_w2c of lfs_fastgs_view_backward; reference:
rasterization_api.cu:133-136, kernels_backward.cuh:165-183), through the C ABI, the Python mirror, the libtorch wrapper, pose recovery and the trainer.

The frozen oracle never asks for grad_w2c, so nothing here compares against a golden: at SH degree 0 the reference's grad_means is exactly R^T dcam, which ties the
new output to gradients the rest of the suite holds to the oracle (`_expected`); at degree 1 the colour -> position term is removed on the host first.

The blending backward sums with float atomics whose order differs from run to run, so two backward calls do not see the same accumulator rows. Where a check is
"bit for bit on the same state" the rows are HELD: one backward fills them, then lfs_fastgs_set_debug_flags(2) makes the following calls reuse them (`_held_acc`).
The first four test bodies also run on the emulated library (tests/test_emulated_fastgs_w2c.py).

Said outright: two of the issue's checks are worded as bit-identity and are met to the letter ONLY under these conditions. "Two calls give bit-identical grad_w2c"
and "the six gradients are bit-identical to the backward without grad_w2c on the same state" are asserted bitwise with the accumulator rows held; two free-running calls are
printed and held to a bound derived from the run-to-run difference of grad_means (test 3). "pose_optimization='none' is bit-identical in parameters to a trainer
built without the argument" is asserted bitwise on the 3DGUT path (the default rasterizer) in its deterministic accumulation mode; on the fastgs path two trainers
never agree in bits, with or without the argument, and the comparison is held to the suite's float-atomic noise floor (test 7)."""
import contextlib
import ctypes as C
import math

import numpy as np
import pytest
import torch

from gpu_util import n, noise_check, rel_l2, t
from test_oracle_fastgs import _scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _settings(sc):
    from lichtfeld_studio_amd.fastgs import FastGSSettings
    return FastGSSettings(t(sc["cam_pos"]), sc["active_sh_bases"], sc["W"], sc["H"], sc["fx"], sc["fy"], sc["cx"], sc["cy"], 0.01, 1e10)


def _scene_with_hidden_third(**cfg):
    """test_oracle_fastgs._scene with every third Gaussian (index 2, 5, 8, ...) mirrored behind the camera: n_touched == 0 there"""
    sc = _scene(**cfg)
    sc["means"][2::3, 2] *= -1.0
    return sc


@contextlib.contextmanager
def _held_acc(lib):
    lib.lfs_fastgs_set_debug_flags(2)
    try:
        yield
    finally:
        lib.lfs_fastgs_set_debug_flags(0)


class _State:
    """one forward + upstream gradients; backward(grad_w2c=...) runs the Python mirror's backward on it"""

    def __init__(self, sc, seed=5):
        from lichtfeld_studio_amd import fastgs
        self.sc, self.s = sc, _settings(sc)
        self.dev = {k: t(sc[k]) for k in ("means", "scales_raw", "rot_raw", "opac_raw", "sh0", "sh_rest", "w2c")}
        self.image, self.alpha, self.pws, self.iws, self.n_inst = fastgs.forward_wrapper(*[self.dev[k] for k in ("means", "scales_raw", "rot_raw", "opac_raw", "sh0", "sh_rest", "w2c")], self.s)
        rng = np.random.default_rng(seed)
        self.gi, self.ga = t(rng.standard_normal((3, sc["H"], sc["W"]))), t(rng.standard_normal((1, sc["H"], sc["W"])))

    def backward(self, grad_w2c=None, dens=None):
        from lichtfeld_studio_amd import fastgs
        d = self.dev
        return fastgs.backward_wrapper(dens, self.gi, self.ga, self.image, self.alpha, d["means"], d["scales_raw"], d["rot_raw"], d["sh0"], d["sh_rest"], self.pws, self.iws,
                                       d["w2c"], self.s, self.n_inst, grad_w2c=grad_w2c)


def _expected(sc, grad_means, sh_term=None):
    """float64 on the host: d_i = R grad_means_i, E[r,c] = sum_i d_i[r] (m_i, 1)[c], and the scale M of the bound (the issue's formulas)"""
    R = np.asarray(sc["w2c"], np.float32).astype(np.float64)[:3, :3]
    m1 = np.concatenate([np.asarray(sc["means"], np.float32).astype(np.float64), np.ones((len(sc["means"]), 1))], 1)
    gm = np.asarray(grad_means, np.float64)
    g = gm if sh_term is None else gm - sh_term
    d = g @ R.T
    E = d.T @ m1
    if sh_term is None:
        M = float((np.linalg.norm(d, axis=1) * np.linalg.norm(m1, axis=1)).sum())
    else:
        M = float(((np.linalg.norm(gm, axis=1) + np.linalg.norm(sh_term, axis=1)) * np.linalg.norm(m1, axis=1)).sum())
    return E, M


def _check_identity(st, sh_term_of=None):
    N = len(st.sc["means"])
    gw = torch.full((4, 4), NAN, device=DEV)
    g = st.backward(grad_w2c=gw)
    gm = n(g[0])
    rows = int((np.abs(gm).max(axis=1) > 0).sum())
    assert rows * 4 >= N, (rows, N)                      # at least a quarter of the Gaussians carry a gradient ...
    if N >= 63:
        assert rows < N                                   # ... and some carry none (the mirrored third)
    E, M = _expected(st.sc, gm, None if sh_term_of is None else sh_term_of(g))
    out = n(gw).astype(np.float64)
    assert np.isfinite(out).all() and (out[3] == 0).all()
    err = float(np.abs(out[:3] - E).max())
    print(f"grad_w2c identity N={N}: max|grad_w2c - E| = {err:.3e}, bound 1e-5 M = {1e-5 * M:.3e}, ratio {err / (1e-5 * M):.4f}, rows with a gradient {rows}")
    assert M > 0 and err <= 1e-5 * M, (err, 1e-5 * M)
    return out


# ---- 1. identity at SH degree 0, ragged sizes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [dict(N=2000, W=203, H=117, seed=1), dict(N=1, W=80, H=64, seed=4), dict(N=63, W=80, H=64, seed=2), dict(N=65, W=80, H=64, seed=3),
                                 dict(N=257, W=80, H=64, seed=4), dict(N=1000, W=80, H=64, seed=6)], ids=lambda c: f"N{c['N']}")
def test_grad_w2c_is_the_sum_of_dcam_times_mean_at_sh_degree_0(lfs, cfg):
    """active_sh_bases = 1: no colour -> position term, grad_means = R^T dcam exactly, so grad_w2c[:3] = sum_i (R grad_means_i) (x) (m_i, 1).
    Bound 1e-5 M, M = sum |d_i| |(m_i, 1)|: per-term rounding <= ~8 ulp, fixed-order tree over <= 4096 terms and <= 16 partial rows <= ~24 ulp, together
    < 32 x 2^-24 ~ 2e-6; the bound is 5 x that (it presumes the deterministic reduction)."""
    _check_identity(_State(_scene_with_hidden_third(deg=0, **cfg)))


# ---- 2. the SH colour -> position term is not in it -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [dict(N=257, W=80, H=64, seed=5), dict(N=3000, W=160, H=112, seed=0)], ids=lambda c: f"N{c['N']}")
def test_grad_w2c_leaves_out_the_sh_colour_term(lfs, cfg):
    """degree 1, non-zero sh_rest: grad_means = R^T dcam + (colour -> position term of the SH backward). The term is rebuilt on the host in float64 from grad_sh0 and
    sh_rest and taken off before the identity of test 1 is applied; summing the final grad_means instead would miss the bound by about three orders of magnitude."""
    sc = _scene_with_hidden_third(deg=1, **cfg)
    assert sc["active_sh_bases"] == 4 and np.abs(sc["sh_rest"][:, :3]).max() > 0

    def sh_term(g):
        v = n(g[4]).astype(np.float64)[:, 0, :] / 0.28209479177387814
        rest = np.asarray(sc["sh_rest"], np.float32).astype(np.float64)
        D = np.asarray(sc["means"], np.float32).astype(np.float64) - np.asarray(sc["cam_pos"], np.float32).astype(np.float64)
        L = np.linalg.norm(D, axis=1, keepdims=True)
        d = D / L
        gd = 0.4886025119029199 * np.stack([-(v * rest[:, 2, :]).sum(1), -(v * rest[:, 0, :]).sum(1), (v * rest[:, 1, :]).sum(1)], 1)
        term = (gd - d * (gd * d).sum(1, keepdims=True)) / L
        assert np.abs(term).max() > 0
        return term

    _check_identity(_State(sc), sh_term_of=sh_term)


# ---- 3. no disturbance, full write, determinism --------------------------------------------------------------------------------------------------------------
def _raw_backward(lib, st, dens, grads, w2c_tail=None):
    """lfs_fastgs_view_backward through ctypes, without (w2c_tail None) or with w2c_tail = (grad_w2c ptr, workspace ptr, workspace bytes); -> return code"""
    from fastgs_raw import backward_raw
    a = [st.dev[k] for k in ("means", "scales_raw", "rot_raw", "opac_raw", "sh0", "sh_rest", "w2c")]
    return backward_raw(lib, a, st.s, st.pws, st.iws, st.n_inst, st.gi, st.ga, st.alpha, dens, grads, w2c_tail=w2c_tail)


def _grad_buffers(st):
    d = st.dev
    N = d["means"].shape[0]
    return [torch.full_like(d["means"], NAN), torch.full_like(d["scales_raw"], NAN), torch.full_like(d["rot_raw"], NAN), torch.full((N, 1), NAN, device=DEV),
            torch.full((N, 1, 3), NAN, device=DEV), torch.full_like(d["sh_rest"], NAN)]


def test_w2c_entry_point_disturbs_nothing_writes_fully_and_is_deterministic(lfs):
    from lichtfeld_studio_amd.capi import ptr
    lib = lfs.load_library()
    st = _State(_scene(N=3000, W=160, H=112, seed=0, deg=3))
    N = 3000
    ws = torch.empty(lib.lfs_fastgs_w2c_workspace_bytes(C.c_uint32(N)), dtype=torch.uint8, device=DEV)
    assert ws.numel() >= 12 * 4 * math.ceil(N / 256)
    # (for the record: two full backward calls, each with its own float-atomic blending backward)
    free = []
    for _ in range(2):
        gw, g, dens = torch.full((4, 4), NAN, device=DEV), _grad_buffers(st), torch.zeros(2, N, device=DEV)
        assert _raw_backward(lib, st, dens, g, (ptr(gw), ptr(ws), ws.numel())) == 0
        free.append((gw, g))
    print("two full backward calls with grad_w2c bit-identical (blending backward re-run):", torch.equal(free[0][0], free[1][0]),
          "| rel-L2 of the difference", rel_l2(n(free[0][0]), n(free[1][0])))
    with _held_acc(lib):   # the accumulator rows of the last call above, for every call below
        plain, dens_plain = _grad_buffers(st), torch.zeros(2, N, device=DEV)
        assert _raw_backward(lib, st, dens_plain, plain) == 0
        runs = []
        for _ in range(2):
            gw, g, dens = torch.full((4, 4), NAN, device=DEV), _grad_buffers(st), torch.zeros(2, N, device=DEV)
            assert _raw_backward(lib, st, dens, g, (ptr(gw), ptr(ws), ws.numel())) == 0
            runs.append((gw, g, dens))
    for gw, g, dens in runs:
        for name, a, b in zip(["means", "scales_raw", "rot_raw", "opac_raw", "sh0", "sh_rest"], g, plain):
            assert torch.isfinite(b).all() and torch.equal(a, b), name            # the six gradients: bit for bit what the backward without grad_w2c writes
        assert torch.equal(dens, dens_plain) and float(dens[0].sum()) > 0
        assert torch.isfinite(gw).all() and bool((gw[3] == 0).all()) and float(gw[:3].abs().max()) > 0   # NaN-filled on entry: every element was written
    assert torch.equal(runs[0][0], runs[1][0])                                     # same bits from run to run
    assert torch.equal(runs[0][0], free[1][0])                                     # ... and the bits of the full call whose accumulator rows were held
    # The two free-running calls differ only through the accumulator rows. grad_w2c is linear in dcam_i = R (grad_means_i - sh_i), sh_i the colour -> position term, so
    # |delta grad_w2c[r,c]| <= sum_i (|delta grad_means_i| + |delta sh_i|) |(m_i, 1)| + the rounding of the two fixed-order sums (2 x 2e-6 M, test 1's derivation).
    # sh_i is about 1 % of grad_means_i and made of the same accumulator rows; its share of the difference is taken as no larger than grad_means' own: a factor 2.
    gm0, gm1 = n(free[0][1][0]).astype(np.float64), n(free[1][1][0]).astype(np.float64)
    m1 = np.sqrt((n(st.dev["means"]).astype(np.float64) ** 2).sum(1) + 1.0)
    M = float((np.linalg.norm(gm1, axis=1) * m1).sum())
    bar = 2.0 * float((np.linalg.norm(gm0 - gm1, axis=1) * m1).sum()) + 4e-6 * M
    noise_check("grad_w2c of two blending backwards, max |difference| against the propagated difference of grad_means", float((free[0][0] - free[1][0]).abs().max()), bar)


# ---- 4. edges --------------------------------------------------------------------------------------------------------------------------------------------------
def test_grad_w2c_edges_empty_scene_nothing_visible_and_return_codes(lfs):
    from lichtfeld_studio_amd.capi import ptr
    lib = lfs.load_library()
    # N = 0
    sc = _scene(N=4, W=80, H=64, seed=0, deg=0)
    for k in ("means", "scales_raw", "rot_raw", "opac_raw", "sh0", "sh_rest"):
        sc[k] = sc[k][:0]
    st = _State(sc)
    assert st.n_inst == 0
    gw = torch.full((1, 4, 4), NAN, device=DEV)
    st.backward(grad_w2c=gw)
    assert bool((gw == 0).all())
    # nothing visible: the whole scene behind the camera
    sc = _scene(N=300, W=80, H=64, seed=1, deg=1)
    sc["means"][:, 2] *= -1.0
    st = _State(sc)
    assert st.n_inst == 0
    gw = torch.full((4, 4), NAN, device=DEV)
    g = st.backward(grad_w2c=gw)
    assert bool((gw == 0).all()) and all(bool((x == 0).all()) for x in g)
    # return codes (nothing is launched)
    need = lib.lfs_fastgs_w2c_workspace_bytes(C.c_uint32(300))
    assert lib.lfs_fastgs_w2c_workspace_bytes(C.c_uint32(0)) > 0 and need >= 2 * 48
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    gw.fill_(NAN)
    grads = _grad_buffers(st)
    assert _raw_backward(lib, st, None, grads, (ptr(gw), ptr(ws), need - 1)) == -3       # LFS_E_WORKSPACE
    assert _raw_backward(lib, st, None, grads, (ptr(gw), None, need)) == -3
    assert _raw_backward(lib, st, None, grads, (None, ptr(ws), need)) == -1              # LFS_E_INVALID
    assert bool(torch.isnan(gw).all()) and bool(torch.isnan(grads[0]).all())
    assert _raw_backward(lib, st, None, grads, (ptr(gw), ptr(ws), need)) == 0 and bool((gw == 0).all())
    from lichtfeld_studio_amd.capi import LfsError
    with pytest.raises(LfsError):
        st.backward(grad_w2c=torch.zeros(3, 4, device=DEV))
    with pytest.raises(LfsError):                                                          # 16 elements, but strided: the kernel writes 16 consecutive floats
        st.backward(grad_w2c=torch.zeros(4, 8, device=DEV)[:, ::2])
    ws4 = torch.empty(need + 16, dtype=torch.uint8, device=DEV)[4:]                         # the partial rows are read as float4
    assert ptr(ws4).value % 16 == 4 and _raw_backward(lib, st, None, grads, (ptr(gw), ptr(ws4), need)) == -1


# ---- 5. surfaces -------------------------------------------------------------------------------------------------------------------------------------------------
def test_autograd_function_returns_the_wrappers_grad_w2c(lfs):
    """FastGSRasterize with a w2c that requires grad: w2c.grad in w2c's shape, the very bits backward_wrapper(grad_w2c=...) writes for the same upstream gradient (on
    the accumulator rows the autograd backward left: see the module docstring); None when not required."""
    from lichtfeld_studio_amd import fastgs
    lib = lfs.load_library()
    sc = _scene_with_hidden_third(N=1500, W=96, H=64, seed=3, deg=2)
    s = _settings(sc)
    a = [t(sc[k]) for k in ("means", "scales_raw", "rot_raw", "opac_raw", "sh0", "sh_rest")]
    rng = np.random.default_rng(8)
    gi, ga = t(rng.standard_normal((3, sc["H"], sc["W"]))), t(rng.standard_normal((1, sc["H"], sc["W"])))
    for shape in ((1, 4, 4), (4, 4)):
        w2c = t(sc["w2c"]).reshape(shape).requires_grad_()
        means = a[0].clone().requires_grad_()
        image, alpha = fastgs.FastGSRasterize.apply(means, *a[1:], w2c, None, s)
        node = image.grad_fn
        torch.autograd.backward([image, alpha], [gi, ga])
        assert w2c.grad is not None and w2c.grad.shape == w2c.shape and float(w2c.grad.abs().max()) > 0
        pws, iws, n_inst = node.state[:3]
        out = torch.full((4, 4), NAN, device=DEV)
        with _held_acc(lib):
            g = fastgs.backward_wrapper(None, gi, ga, image.detach(), alpha.detach(), a[0], a[1], a[2], a[4], a[5], pws, iws, w2c.detach(), s, n_inst, grad_w2c=out)
        assert torch.equal(out.reshape(shape), w2c.grad) and torch.equal(g[0], means.grad)
    w2c = t(sc["w2c"])
    means = a[0].clone().requires_grad_()
    image, alpha = fastgs.FastGSRasterize.apply(means, *a[1:], w2c, None, s)
    torch.autograd.backward([image, alpha], [gi, ga])
    assert w2c.grad is None and means.grad is not None


def test_libtorch_backward_wrapper_honours_w2c_requires_grad(lfs):
    """fast_gs::rasterization::backward_wrapper through the pybind module: a 7th element shaped like w2c when w2c requires grad, bit-equal to the ctypes path on the
    same accumulator rows; still None otherwise."""
    import lichtfeld_studio_amd  # noqa: F401
    import glob
    import os
    if not glob.glob(os.path.join(os.path.dirname(lfs.__file__), "_lfs_torch_ops*.so")):
        pytest.skip("_lfs_torch_ops.so not built (python lichtfeld-studio_amd/build.py --torch-ops)")
    from lichtfeld_studio_amd import _lfs_torch_ops as m   # (a module that exists and does not import is a failure, not a skip)
    from lichtfeld_studio_amd import fastgs
    lib = lfs.load_library()
    sc = _scene_with_hidden_third(N=1500, W=96, H=64, seed=9, deg=2)
    a = [t(sc[k]) for k in ("means", "scales_raw", "rot_raw", "opac_raw", "sh0", "sh_rest", "w2c")]
    cam = t(sc["cam_pos"])
    fr = (sc["active_sh_bases"], sc["W"], sc["H"], sc["fx"], sc["fy"], sc["cx"], sc["cy"], 0.01, 1e10)
    image, alpha, prim, tile, inst, bucket, n_vis, n_inst, n_buckets, s0, s1 = m.fastgs_forward_wrapper(*a, cam, *fr)
    gi, ga = torch.randn_like(image), torch.randn_like(alpha)
    none = torch.empty(0, device=DEV)
    for shape in ((4, 4), (1, 4, 4)):
        w2c = a[6].clone().reshape(shape).requires_grad_()
        g1 = m.fastgs_backward_wrapper(none, gi, ga, image, alpha, a[0], a[1], a[2], a[5], prim, tile, inst, bucket, w2c, cam, *fr, n_vis, n_inst, n_buckets, s0, s1)
        assert len(g1) == 7 and g1[6] is not None and g1[6].shape == w2c.shape and not g1[6].requires_grad
        out = torch.full((4, 4), NAN, device=DEV)
        with _held_acc(lib):
            g2 = fastgs.backward_wrapper(None, gi, ga, image, alpha, a[0], a[1], a[2], a[4], a[5], prim, inst, a[6], fastgs.FastGSSettings(cam, *fr), n_inst, grad_w2c=out)
        assert torch.equal(g1[6].reshape(4, 4), out) and float(out.abs().max()) > 0 and bool((out[3] == 0).all())
        assert torch.equal(g1[0], g2[0])
    g3 = m.fastgs_backward_wrapper(none, gi, ga, image, alpha, a[0], a[1], a[2], a[5], prim, tile, inst, bucket, a[6], cam, *fr, n_vis, n_inst, n_buckets, s0, s1)
    assert len(g3) == 7 and g3[6] is None


# ---- 6. pose recovery with frozen Gaussians ------------------------------------------------------------------------------------------------------------------------
def test_pose_recovery_with_frozen_gaussians(lfs):
    """A perturbed camera finds its way back on grad_w2c alone: 60 Adam(1e-3) steps of DirectPoseOptimization(1) through FastGSRasterize autograd, MSE against the render
    at the true pose, cam_position held at the true camera's. Conditions (loss <= 0.1 x initial, pose error <= 0.75 x initial) chosen from a float64 simulation of
    exactly this loop with the reference's gradient formula: loss 4.61e-4 -> 3.30e-6 (/140), |w2c_adj[:3] - w2c_true[:3]|_F 0.0428 -> 0.0161 (x0.38); a second scene
    (400 Gaussians, 80x64, seed 0): /68 and x0.58."""
    from lichtfeld_studio_amd import fastgs
    from lichtfeld_studio_amd.poseopt import DirectPoseOptimization
    sc = _scene(N=1000, W=96, H=64, seed=7, deg=0)
    s = _settings(sc)                       # cam_position: the true camera's, throughout
    a = [t(sc[k]) for k in ("means", "scales_raw", "rot_raw", "opac_raw", "sh0", "sh_rest")]
    w2c_true = t(sc["w2c"]).reshape(1, 4, 4)
    with torch.no_grad():
        target, _ = fastgs.FastGSRasterize.apply(*a, w2c_true, None, s)
    ang = -0.008
    P = torch.eye(4, dtype=torch.float64)
    P[:2, :2] = torch.tensor([[math.cos(ang), -math.sin(ang)], [math.sin(ang), math.cos(ang)]], dtype=torch.float64)
    P[:3, 3] = torch.tensor([0.02, 0.02, -0.03], dtype=torch.float64)
    start = (torch.as_tensor(sc["w2c"], dtype=torch.float64) @ P).float().reshape(1, 4, 4).to(DEV)
    mod = DirectPoseOptimization(1).to(DEV)
    opt = torch.optim.Adam(mod.parameters(), lr=1e-3)
    losses, errs = [], []
    for _ in range(61):                     # 60 steps; the 61st pass only evaluates the final pose
        w2c_adj = mod(start, [0])
        image, _ = fastgs.FastGSRasterize.apply(*a, w2c_adj, None, s)
        loss = torch.nn.functional.mse_loss(image, target)
        losses.append(float(loss))
        errs.append(float((w2c_adj[0, :3] - w2c_true[0, :3]).norm()))
        if len(losses) == 61:
            break
        opt.zero_grad()
        loss.backward()
        opt.step()
    print(f"pose recovery: loss {losses[0]:.3e} -> {losses[-1]:.3e} (/{losses[0] / losses[-1]:.1f}), pose error {errs[0]:.4f} -> {errs[-1]:.4f} (x{errs[-1] / errs[0]:.2f})")
    assert losses[0] > 0 and errs[0] > 0.03
    assert losses[-1] <= 0.1 * losses[0], (losses[0], losses[-1])
    assert errs[-1] <= 0.75 * errs[0], (errs[0], errs[-1])


def _same_loss(label, la, lb):
    """Two steps on the same state report the same loss up to the order of its float-atomic sum: the loss kernels add one partial sum per wavefront or workgroup
    (<= 1280 of them at 256x256) into the accumulator in whatever order they retire. A random-order fp32 sum of n terms wanders by about sqrt(n) 2^-24 ~ 2e-6 of
    the total; the bar is 5 x that, 1e-5 of the loss - the bar the suite already holds loss values of this size to (test_gpu_fused.py)."""
    la, lb = float(la), float(lb)
    assert math.isfinite(la) and lb > 0
    noise_check(label, abs(la - lb), 1e-5 * lb)


# ---- 7. trainer ------------------------------------------------------------------------------------------------------------------------------------------------------
def _three_view_syn_a():
    """SYN-A (one camera) with its camera listed three times: the pose modules get three embedding rows, the tests train row 1"""
    from lichtfeld_studio_amd import scenes
    sc = scenes.syn_a(n=4000, sh_degree=2)
    sc.viewmats, sc.Ks = sc.viewmats.repeat(3, 1, 1).contiguous(), sc.Ks.repeat(3, 1, 1).contiguous()
    return sc


def test_trainer_direct_pose_optimisation_matches_autograd_and_trains_one_row(lfs):
    from lichtfeld_studio_amd import fastgs, scenes
    from lichtfeld_studio_amd.rasterizer import Camera
    from lichtfeld_studio_amd.trainer import GutTrainer
    dev = torch.device(DEV)
    sc = _three_view_syn_a()
    tr = GutTrainer(sc, dev, iterations=100, rasterizer="fastgs", pose_optimization="direct")
    assert tr.pose_module is not None and tuple(tr.pose_module.camera_embeddings.weight.shape) == (3, 9)
    assert tr.pose_optimizer.param_groups[0]["lr"] == 1e-5
    target = scenes.target_image(sc.height, sc.width).to(dev)
    w2c = tr.scene.viewmats[1:2].clone().requires_grad_()
    ref = fastgs.fast_rasterize(Camera(w2c, tr.scene.Ks[1:2].contiguous(), sc.width, sc.height), tr.model, torch.zeros(3, device=dev))
    torch.nn.functional.mse_loss(ref.image, target).backward()
    for p in tr.model.parameters():
        p.grad = None
    tr.train_step([target], views=[1])
    assert tr.last_plan.path == "fastgs" and tr.last_grad_w2c.shape == (1, 4, 4)
    e = rel_l2(n(tr.last_grad_w2c), n(w2c.grad))
    print(f"trainer last_grad_w2c vs autograd: rel-L2 {e:.2e}")
    assert float(w2c.grad.abs().max()) > 0 and e < 1e-4, e
    for _ in range(3):
        tr.train_step([target], views=[1])
    w = tr.pose_module.camera_embeddings.weight.detach()
    assert float(w[1].abs().max()) > 0 and float(w[[0, 2]].abs().max()) == 0
    assert all(p.grad is None for p in tr.pose_module.parameters())            # zero_grad after the step
    tr.iteration = 1500                                                        # Adam reads shN: the inline-shN backward has no camera gradient and must not be taken
    before = tr.last_grad_w2c
    tr.train_step([target], views=[1])
    assert tr.last_grad_w2c is not before and torch.isfinite(tr.last_grad_w2c).all() and tr.model.shN.grad is not None


def test_trainer_mlp_pose_optimisation_starts_at_the_identity(lfs):
    from lichtfeld_studio_amd import scenes
    from lichtfeld_studio_amd.trainer import GutTrainer
    dev = torch.device(DEV)
    sc = _three_view_syn_a()
    target = scenes.target_image(sc.height, sc.width).to(dev)
    torch.manual_seed(0)
    tr = GutTrainer(sc, dev, iterations=100, rasterizer="fastgs", pose_optimization="mlp")
    plain = GutTrainer(sc, dev, iterations=100, rasterizer="fastgs")
    last = tr.pose_module.mlp[-1]
    assert float(last.weight.abs().max()) == 0 and float(last.bias.abs().max()) == 0
    with torch.no_grad():
        assert torch.equal(tr.pose_module(tr.scene.viewmats, [0, 1, 2]), tr.scene.viewmats)     # zero last layer: the transform is the identity
    l_pose, l_plain = float(tr.train_step([target], views=[1])), float(plain.train_step([target], views=[1]))
    _same_loss("mlp pose optimisation, first step vs no pose optimisation", l_pose, l_plain)       # the first step rendered the stored pose
    assert float(last.weight.abs().max()) > 0 or float(last.bias.abs().max()) > 0                # ... and moved the last layer away from zero
    assert float(last.bias.abs().max()) > 0
    for _ in range(2):
        assert math.isfinite(float(tr.train_step([target], views=[1])))


def test_trainer_pose_optimisation_refusals_and_none_is_the_old_trainer(lfs):
    from lichtfeld_studio_amd import scenes
    from lichtfeld_studio_amd.trainer import GutTrainer
    dev = torch.device(DEV)
    sc = scenes.syn_a(n=4000, sh_degree=2)
    with pytest.raises(ValueError, match="3DGUT rasterizer doesn't have camera gradients"):
        GutTrainer(sc, dev, iterations=100, rasterizer="gut", pose_optimization="direct")
    with pytest.raises(ValueError, match="one rank"):
        GutTrainer(sc, dev, iterations=100, rasterizer="fastgs", pose_optimization="mlp", world=2)
    with pytest.raises(ValueError, match="Invalid pose optimization type"):
        GutTrainer(sc, dev, iterations=100, rasterizer="fastgs", pose_optimization="sideways")
    target = scenes.target_image(sc.height, sc.width).to(dev)
    # "none" on the 3DGUT path in its deterministic accumulation mode (integer atomics): a step is the same bits with and without the argument
    lib = lfs.load_library()
    lib.lfs_set_debug_flags(16)
    try:
        a, b = GutTrainer(sc, dev, iterations=100, pose_optimization="none"), GutTrainer(sc, dev, iterations=100)
        assert a.pose_module is None and a.pose_optimizer is None and a.last_grad_w2c is None
        la, lb = a.train_step([target], views=[0]), b.train_step([target], views=[0])
        _same_loss("3DGUT step, pose_optimization='none' vs no argument", la, lb)
        assert a.last_plan == b.last_plan
        for p, q in zip(a.model.parameters(), b.model.parameters()):
            assert torch.equal(p, q)
    finally:
        lib.lfs_set_debug_flags(0)
    # ... and on the fastgs path. The blending backward sums with float atomics, so two trainers never agree in bits there, with or without the argument: the
    # gradients are held to the suite's floor for one float-atomic draw against another (gpu_util.atomic_noise_bar: rel-L2 2e-5). The parameters after this
    # FIRST Adam step moved by lr * g / (|g| + eps) = +-lr whatever the last bits of g, so they agree far below the step itself (rel-L2 1e-5 of the tensor).
    a, b = GutTrainer(sc, dev, iterations=100, rasterizer="fastgs", pose_optimization="none"), GutTrainer(sc, dev, iterations=100, rasterizer="fastgs")
    assert a.pose_module is None and a.pose_optimizer is None
    la, lb = a.train_step([target], views=[0]), b.train_step([target], views=[0])
    _same_loss("fastgs step, pose_optimization='none' vs no argument", la, lb)
    assert a.last_plan == b.last_plan and a.last_grad_w2c is None
    for k, (p, q) in enumerate(zip(a.model.parameters(), b.model.parameters())):
        if p.numel():
            noise_check(f"fastgs step, pose_optimization='none' vs no argument, gradient {k}", rel_l2(n(p.grad), n(q.grad)), 2e-5)
            noise_check(f"fastgs step, pose_optimization='none' vs no argument, parameter {k}", rel_l2(n(p), n(q)), 1e-5)
