"""The background colour on the MI355X (bodies: tests/background_reference.py, shared with tests/test_emulated_background.py): lfs_background_compose and
lfs_background_compose_bwd against the float32 model and torch bit for bit at every size, group combination and alignment with NaN guards; the fastgs trainer step
with a colour against fast_rasterize + autograd (MSE, L1 + D-SSIM, segment mode); the defaults against the step without the arguments, bit for bit; RGBA targets;
the 3DGUT route's fused forms against their autograd twin; lfs::background_compose through the pybind module.

Measured on the MI355X (printed by the tests): the coloured fastgs step against autograd - |dloss| 6e-8 .. 2.4e-7 against the bound 1e-6, rel_l2 of the six gradient
groups 4e-8 .. 4.3e-7 against 1e-4; the 3DGUT route's fused forms against the autograd twin - |dloss| <= 1.5e-8 against 1e-4."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import background_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("bg", ref.COLOURS, ids=["black", "white", "colour"])
def test_kernels_sizes_groups_in_place_alignment(lfs, bg):
    ref.check_kernels(DEV, bg)


def test_wrapper_refusals(lfs):
    ref.check_wrapper_refusals(DEV)


def test_one_launch_at_1080p(lfs):
    """the size of a training image (2025 blocks, the vector form): both groups in one launch and the backward, every pixel against the float32 model"""
    import torch
    from lichtfeld_studio_amd import ops
    H, W = 1080, 1920
    image, alpha, target, u8, v, v_in = [torch.from_numpy(a).to(DEV) for a in ref.inputs(H, W)]
    shown, t_out = ops.background_compose(ref.BG, image, alpha, None, target, u8)
    out = ops.background_compose_bwd(ref.BG, v, v_in)
    image, alpha, target, u8, v, v_in = ref.inputs(H, W)
    assert np.array_equal(ref.bits(shown.cpu().numpy()), ref.bits(ref.model_compose(image, alpha, ref.BG)))
    assert np.array_equal(ref.bits(t_out.cpu().numpy()), ref.bits(ref.model_target(target, u8, ref.BG)))
    assert np.array_equal(ref.bits(out.cpu().numpy()[0]), ref.bits(ref.model_bwd(v, ref.BG, v_in)))


@pytest.mark.parametrize("loss,segment", [("mse", False), ("l1_ssim", False), ("l1_ssim", True)], ids=["mse", "l1_ssim", "l1_ssim_segment"])
def test_fastgs_step_with_a_colour_matches_autograd(lfs, loss, segment):
    ref.check_fastgs_step_matches_autograd(DEV, loss, segment)


def test_defaults_are_the_parents(lfs):
    ref.check_defaults_are_the_parents(lfs.capi, DEV)


@pytest.mark.parametrize("bg", [ref.BG, (0.0, 0.0, 0.0)], ids=["colour", "black"])
def test_rgba_step(lfs, bg):
    ref.check_rgba_step(DEV, bg)


def test_preload_alphas(lfs, tmp_path):
    ref.check_preload_alphas(DEV, tmp_path)


def test_trainer_policy(lfs):
    ref.check_trainer_policy(DEV)


@pytest.mark.parametrize("one_call", [False, True], ids=["default_form", "one_call"])
def test_3dgut_route_fused_matches_autograd(lfs, one_call):
    ref.check_gut_route(DEV, one_call)


def test_3dgut_route_random_colour_per_step(lfs):
    ref.check_gut_route(DEV, False, (0.0, 0.0, 0.0), "random")


def test_3dgut_route_rgba(lfs):
    ref.check_gut_route_rgba(DEV)


def test_evaluate_composites_the_ground_truth(lfs):
    import torch
    from lichtfeld_studio_amd import evaluate, scenes
    from lichtfeld_studio_amd.trainer import GutTrainer
    dev = torch.device(DEV)
    sc = scenes.syn_a(n=2000, sh_degree=1)
    tr = GutTrainer(sc, dev, iterations=100, rasterizer="fastgs")
    gt = scenes.target_image(sc.height, sc.width).to(dev)
    plane = torch.from_numpy(ref.disc_alpha(sc.height, sc.width)).to(dev)
    a = ref.alpha_of(plane)
    bg = torch.tensor(ref.BG, device=dev)
    m1 = evaluate.evaluate(tr.model, [tr.camera(0)], [gt], background=bg, alphas=[plane])
    m2 = evaluate.evaluate(tr.model, [tr.camera(0)], [a * gt + (1.0 - a) * bg.view(3, 1, 1)], background=bg)
    m3 = evaluate.evaluate(tr.model, [tr.camera(0)], [gt], background=bg)
    assert m1.psnr == m2.psnr and m1.ssim == m2.ssim and m1.psnr != m3.psnr
    with pytest.raises(ValueError):
        evaluate.evaluate(tr.model, [tr.camera(0)], [gt], alphas=[plane, plane])


def test_libtorch_wrapper_equals_the_python_one(lfs):
    import torch
    try:
        from lichtfeld_studio_amd import _lfs_torch_ops as m
    except ImportError:
        pytest.skip("_lfs_torch_ops.so not built (python lichtfeld-studio_amd/build.py --torch-ops)")
    from lichtfeld_studio_amd import ops
    for (H, W) in ((7, 67), (16, 64)):
        image, alpha, target, u8, v, v_in = [torch.from_numpy(a).to(DEV) for a in ref.inputs(H, W)]
        want_s, want_t = ops.background_compose(ref.BG, image, alpha, None, target, u8)
        got_s, got_t = m.background_compose(list(ref.BG), image, alpha, target, u8, False)
        assert torch.equal(got_s, want_s) and torch.equal(got_t, want_t) and got_s.data_ptr() != image.data_ptr()
        only_s, none_t = m.background_compose(list(ref.BG), image, alpha)
        assert torch.equal(only_s, want_s) and none_t is None
        none_s, only_t = m.background_compose(list(ref.BG), None, None, target, u8)
        assert none_s is None and torch.equal(only_t, want_t)
        want_b = ops.background_compose_bwd(ref.BG, v, v_in)
        assert torch.equal(m.background_compose_bwd(list(ref.BG), v, v_in), want_b)
        assert torch.equal(m.background_compose_bwd(list(ref.BG), v), ops.background_compose_bwd(ref.BG, v))
        work = image.clone()
        same, _ = m.background_compose(list(ref.BG), work, alpha, None, None, True)
        assert same.data_ptr() == work.data_ptr() and torch.equal(work, want_s)
        acc = v_in.clone()
        assert m.background_compose_bwd(list(ref.BG), v, acc, True).data_ptr() == acc.data_ptr() and torch.equal(acc, want_b)
    with pytest.raises(RuntimeError):
        m.background_compose(list(ref.BG), image, None)
    with pytest.raises(RuntimeError):
        m.background_compose([0.1, float("nan"), 0.2], image, alpha)
    with pytest.raises(RuntimeError):
        m.background_compose(list(ref.BG), image.cpu(), alpha.cpu())
