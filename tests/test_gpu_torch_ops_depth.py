"""The libtorch route of the fastgs depth modes (lfs::fastgs_forward_wrapper_depth / lfs::fastgs_backward_wrapper_depth of include/lfs_gsplat_torch.hpp, next to the
untouched fast_gs::rasterization::*): the backend library defines them (CPU, no GPU), and on the GPU they give the bits of the ctypes route."""
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
    for name in ("lfs::fastgs_forward_wrapper_depth(", "lfs::fastgs_backward_wrapper_depth(", "lfs::fastgs_forward_wrapper_ex(", "fast_gs::rasterization::forward_wrapper(",
                 "fast_gs::rasterization::backward_wrapper("):
        assert name in defined, name
    header = open(os.path.join(ROOT, "include", "lfs_gsplat_torch.hpp")).read()
    assert "fastgs_forward_wrapper_depth(" in header and "fastgs_backward_wrapper_depth(" in header


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
        image, alpha, depth, prim, inst, n_inst = m.fastgs_forward_wrapper_depth(*a, cam, *fr, True, kind == "invdepth")
        g1 = m.fastgs_backward_wrapper_depth(none, gi, ga, gd, alpha, a[0], a[1], a[2], a[5], prim, inst, a[6], cam, *fr, n_inst)
        w2c_g = a[6].clone().requires_grad_(True)
        g1w = m.fastgs_backward_wrapper_depth(none, gi, ga, gd, alpha, a[0], a[1], a[2], a[5], prim, inst, w2c_g, cam, *fr, n_inst)
        s = fastgs.FastGSSettings(cam, *fr, True, kind)
        img2, al2, d2, pws, iws, n2 = fastgs.forward_wrapper_depth(*a, s)
        g2 = fastgs.backward_wrapper(None, gi, ga, img2, al2, a[0], a[1], a[2], a[4], a[5], pws, iws, a[6], s, n2, grad_depth=gd)
        gw = torch.empty(4, 4, device=DEV)
        g2w = fastgs.backward_wrapper(None, gi, ga, img2, al2, a[0], a[1], a[2], a[4], a[5], pws, iws, a[6], s, n2, grad_depth=gd, grad_w2c=gw)
        ref_img = m.fastgs_forward_wrapper_ex(*a, cam, *fr, True)[0]
    assert n_inst == n2 and torch.equal(image, img2) and torch.equal(alpha, al2) and torch.equal(depth, d2) and torch.equal(image, ref_img)
    assert float(depth.abs().max()) > 0 and (g1[6] is None or g1[6].numel() == 0)     # no camera gradient unless w2c asks for one
    for p, q in zip(g1[:6], g2):
        assert torch.equal(p.reshape(q.shape), q)
    for p, q in zip(g1w[:6], g2w):
        assert torch.equal(p.reshape(q.shape), q)
    assert torch.equal(g1w[6].reshape(4, 4), gw) and float(gw[2].abs().max()) > 0
