"""The libtorch route of the fastgs depth modes (lfs::fastgs_forward / lfs::fastgs_backward of include/lfs_gsplat_torch.hpp with FastgsOptions::depth, next to the
untouched fast_gs::rasterization::*): the backend library defines them (CPU, no GPU), and on the GPU they give the bits of the ctypes route - also with every other
mode of FastgsOptions switched on at once."""
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BACKEND = os.path.join(ROOT, "lichtfeld-studio_amd", "liblfs_gsplat_torch.so")
DEV = "cuda:0"


def test_backend_library_defines_the_depth_wrappers():
    if not os.path.exists(BACKEND):
        pytest.skip("liblfs_gsplat_torch.so not built")
    defined = subprocess.run(["nm", "-DC", "--defined-only", BACKEND], capture_output=True, text=True, check=True).stdout
    for name in ("lfs::fastgs_forward(", "lfs::fastgs_backward(", "fast_gs::rasterization::forward_wrapper(", "fast_gs::rasterization::backward_wrapper("):
        assert name in defined, name
    header = open(os.path.join(ROOT, "include", "lfs_gsplat_torch.hpp")).read()
    assert "FastgsForwardOut fastgs_forward(" in header and "FastgsGrads fastgs_backward(" in header


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["depth", "invdepth"])
def test_libtorch_depth_route_matches_the_ctypes_route_bit_for_bit(lfs, kind):
    from gpu_util import t
    from lichtfeld_studio_amd import _lfs_torch_ops as m
    from lichtfeld_studio_amd import fastgs
    from test_gpu_fastgs_antialiased import _deterministic, _upstream
    from test_gpu_fastgs_depth import _case, _dev, _g_depth
    sc = _case(3, kind)[0]
    a, cam = _dev(sc), t(sc["cam_pos"])
    fr = (sc["active_sh_bases"], sc["W"], sc["H"], sc["fx"], sc["fy"], sc["cx"], sc["cy"], 0.01, 1e10)
    gi, ga = [t(x) for x in _upstream(sc)]
    gd = t(_g_depth(sc))
    none = torch.empty(0, device=DEV)
    with _deterministic(lfs):
        image, alpha, depth, prim, inst, n_inst = m.fastgs_forward(*a, cam, *fr, antialiased=True, depth=2 if kind == "invdepth" else 1)
        g1 = m.fastgs_backward(none, gi, ga, gd, alpha, a[0], a[1], a[2], a[5], prim, inst, a[6], cam, *fr, n_inst)
        w2c_g = a[6].clone().requires_grad_(True)
        g1w = m.fastgs_backward(none, gi, ga, gd, alpha, a[0], a[1], a[2], a[5], prim, inst, w2c_g, cam, *fr, n_inst)
        s = fastgs.FastGSSettings(cam, *fr, True, kind)
        img2, al2, d2, pws, iws, n2 = fastgs.forward_wrapper_depth(*a, s)
        g2 = fastgs.backward_wrapper(None, gi, ga, img2, al2, a[0], a[1], a[2], a[4], a[5], pws, iws, a[6], s, n2, grad_depth=gd)
        gw = torch.empty(4, 4, device=DEV)
        g2w = fastgs.backward_wrapper(None, gi, ga, img2, al2, a[0], a[1], a[2], a[4], a[5], pws, iws, a[6], s, n2, grad_depth=gd, grad_w2c=gw)
        ref_img = m.fastgs_forward(*a, cam, *fr, antialiased=True)[0]
    assert n_inst == n2 and torch.equal(image, img2) and torch.equal(alpha, al2) and torch.equal(depth, d2) and torch.equal(image, ref_img)
    assert float(depth.abs().max()) > 0 and (g1[6] is None or g1[6].numel() == 0)     # no camera gradient unless w2c asks for one
    for p, q in zip(g1[:6], g2):
        assert torch.equal(p.reshape(q.shape), q)
    for p, q in zip(g1w[:6], g2w):
        assert torch.equal(p.reshape(q.shape), q)
    assert torch.equal(g1w[6].reshape(4, 4), gw) and float(gw[2].abs().max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("idx", [2, 1], ids=["N257_deg0", "N1500_deg1"])
def test_libtorch_route_runs_every_mode_at_once(lfs, idx):
    """antialiased + inverse depth + absgrad + the 3D filter in ONE forward / backward, with grad_depth, densification_info and a camera gradient: a combination the
    trainer runs through FastGSSettings, and that lfs::fastgs_forward / lfs::fastgs_backward must give bit for bit. N = 257: one primitive past a 256-thread
    workgroup, degree 0 without rest coefficients (sh_rest [N,0,3]: NULL operands on both routes); N = 1500: degree 1."""
    import numpy as np

    import fastgs_filter3d_reference as f3d
    from gpu_util import t
    from lichtfeld_studio_amd import _lfs_torch_ops as m
    from lichtfeld_studio_amd import fastgs
    from test_gpu_fastgs_antialiased import _deterministic, _upstream
    from test_gpu_fastgs_depth import _case, _dev, _g_depth
    sc = _case(idx, "invdepth")[0]
    a, cam = _dev(sc), t(sc["cam_pos"])
    N = a[0].shape[0]
    if sc["active_sh_bases"] == 1:   # the scenes store 15 rest coefficients whatever their degree: at degree 0 none is active, and the model comes without them
        a[5] = a[5][:, :0].contiguous()
    assert a[5].shape[1] == (0 if idx == 2 else 15)
    v = t(f3d.filter_var64(sc["means"], [f3d.camera_of_scene(sc)]).astype(np.float32))   # as tests/test_gpu_fastgs_filter3d.py: _case
    fr = (sc["active_sh_bases"], sc["W"], sc["H"], sc["fx"], sc["fy"], sc["cx"], sc["cy"], 0.01, 1e10)
    gi, ga = [t(x) for x in _upstream(sc)]
    gd = t(_g_depth(sc))
    with _deterministic(lfs):
        image, alpha, depth, prim, inst, n_inst = m.fastgs_forward(*a, cam, *fr, antialiased=True, depth=2, absgrad=True, filter3d_var=v)
        d1 = torch.zeros(2, N, device=DEV)
        g1 = m.fastgs_backward(d1, gi, ga, gd, alpha, a[0], a[1], a[2], a[5], prim, inst, a[6].clone().requires_grad_(True), cam, *fr, n_inst, filter3d_var=v)
        s = fastgs.FastGSSettings(cam, *fr, True, "invdepth", v, True)
        img2, al2, dep2, pws, iws, n2 = fastgs.forward_wrapper_depth(*a, s)
        d2, gw = torch.zeros(2, N, device=DEV), torch.empty(4, 4, device=DEV)
        g2 = fastgs.backward_wrapper(d2, gi, ga, img2, al2, a[0], a[1], a[2], a[4], a[5], pws, iws, a[6], s, n2, grad_depth=gd, grad_w2c=gw)
    assert n_inst == n2 and torch.equal(image, img2) and torch.equal(alpha, al2) and torch.equal(depth, dep2)
    for p, q in zip(g1[:6], g2):
        assert torch.equal(p.reshape(q.shape), q)
    assert torch.equal(g1[6].reshape(4, 4), gw) and torch.equal(d1, d2)
    assert float(depth.abs().max()) > 0 and float(gw[2].abs().max()) > 0 and float(d1[1].abs().max()) > 0
