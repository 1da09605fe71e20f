"""GPU: masked training through GutTrainer (DESIGN.md §8 "Masked training") - the fused 3DGUT step against the autograd form, the fastgs step against
fast_rasterize under autograd with the autograd mirror of the masked loss, the direction of the opacity penalty, and the unmasked step left alone."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def n(t):
    return t.detach().cpu().double().numpy()


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _half_mask(H, W):
    """PreparedMask: the left half counts, the right half is ignored (sums by lfs_mask_prepare)"""
    from lichtfeld_studio_amd import losses
    m = torch.zeros(H, W, dtype=torch.uint8)
    m[:, :W // 2] = 255
    return losses.prepare_mask(m.to(DEV), W, H)


def test_masked_l1_ssim_trainers_agree_and_train(lfs):
    """3DGUT rasterizer, l1_ssim, mask_mode "ignore", a half-image mask: the fused trainer (cxx_views: the masked loss kernels) and fused_l2=False (autograd over
    masked_photometric_loss) - the bounds of test_l1_ssim_trainers_agree_and_train."""
    from lichtfeld_studio_amd import scenes
    from lichtfeld_studio_amd.trainer import GutTrainer
    sc = scenes.syn_a(n=3000, sh_degree=1)
    a = GutTrainer(sc, torch.device(DEV), iterations=200, fused_l2=True, loss="l1_ssim", mask_mode="ignore")
    b = GutTrainer(sc, torch.device(DEV), iterations=200, fused_l2=False, loss="l1_ssim", mask_mode="ignore")
    target = torch.rand(3, sc.height, sc.width, generator=torch.Generator().manual_seed(1)).to(DEV) * 0.5
    mask = _half_mask(sc.height, sc.width)
    la = [float(a.train_step([target], views=[0], masks=[mask])) for _ in range(30)]
    lb = [float(b.train_step([target], views=[0], masks=[mask])) for _ in range(30)]
    assert a.last_plan.path == "cxx_views" and b.last_plan.path == "autograd"
    print("fused", la[0], la[-1], "autograd", lb[0], lb[-1])
    assert abs(la[0] - lb[0]) < 1e-5 and abs(la[-1] - lb[-1]) < 1e-3
    assert la[-1] < 0.97 * la[0] and lb[-1] < 0.97 * lb[0]
    # the mask matters: the unmasked loss of the same first step is another number
    c = GutTrainer(sc, torch.device(DEV), iterations=200, fused_l2=True, loss="l1_ssim")
    assert abs(float(c.train_step([target], views=[0])) - la[0]) > 1e-4


def test_fastgs_segment_step_matches_autograd(lfs):
    """fastgs rasterizer, one view, segment mode: the gradients of render_and_backward (masked loss kernel, its v_alpha in place of the zero alpha gradient) against
    fast_rasterize under autograd with masked_photometric_loss plus the alpha term - the bounds of test_fastgs_trainer_step_matches_autograd."""
    from lichtfeld_studio_amd import fastgs, losses, scenes
    from lichtfeld_studio_amd.trainer import GutTrainer
    dev = torch.device(DEV)
    sc = scenes.syn_a(n=4000, sh_degree=2)
    w_a = 0.5
    tr = GutTrainer(sc, dev, iterations=100, rasterizer="fastgs", loss="l1_ssim", mask_mode="segment", mask_alpha_weight=w_a)
    target = scenes.target_image(sc.height, sc.width).to(dev)
    mask = _half_mask(sc.height, sc.width)
    ref = fastgs.fast_rasterize(tr.camera(0), tr.model, torch.zeros(3, device=dev))
    m = mask.mask_u8.float()
    loss_ref = losses.masked_photometric_loss(ref.image, target, mask, tr.lambda_dssim) + w_a * ((255.0 - m) * ref.alpha.reshape(m.shape)).sum() / (255.0 * m.numel())
    loss_ref.backward()
    ref_grads = [p.grad.clone() for p in tr.model.parameters()]
    for p in tr.model.parameters():
        p.grad = None
    loss = tr.train_step([target], views=[0], masks=[mask])
    assert tr.last_plan.path == "fastgs"
    assert abs(float(loss) - float(loss_ref)) < 1e-6
    for name, g, r in zip(["means", "sh0", "shN", "raw_scales", "raw_quats", "raw_opacities"], tr.bucket.views, ref_grads):
        assert rel_l2(n(g), n(r).reshape(n(g).shape)) < 1e-4, name


def test_segment_mode_lowers_the_opacity_outside_the_mask(lfs):
    """Direction only: after 30 segment-mode steps the mean rendered alpha over M == 0 is lower than at step 0 and lower than the ignore-mode twin's."""
    from lichtfeld_studio_amd import fastgs, scenes
    from lichtfeld_studio_amd.trainer import GutTrainer
    dev = torch.device(DEV)
    sc = scenes.syn_a(n=3000, sh_degree=1)
    target = scenes.target_image(sc.height, sc.width).to(dev)
    mask = _half_mask(sc.height, sc.width)
    outside = mask.mask_u8 == 0

    def alpha_outside(tr):
        with torch.no_grad():
            out = fastgs.fast_rasterize(tr.camera(0), tr.model, torch.zeros(3, device=dev))
        return float(out.alpha.reshape(outside.shape)[outside].mean())

    seg = GutTrainer(sc, dev, iterations=100, rasterizer="fastgs", loss="l1_ssim", mask_mode="segment", mask_alpha_weight=1.0)
    ign = GutTrainer(sc, dev, iterations=100, rasterizer="fastgs", loss="l1_ssim", mask_mode="ignore")
    a0 = alpha_outside(seg)
    for _ in range(30):
        seg.train_step([target], views=[0], masks=[mask])
        ign.train_step([target], views=[0], masks=[mask])
    a_seg, a_ign = alpha_outside(seg), alpha_outside(ign)
    print("alpha outside the mask: start", a0, "segment", a_seg, "ignore", a_ign)
    assert a_seg < a0 and a_seg < a_ign


@pytest.mark.parametrize("rasterizer", ["gut", "fastgs"])
def test_a_step_without_a_mask_is_the_unmasked_step(lfs, rasterizer):
    from lichtfeld_studio_amd import scenes
    from lichtfeld_studio_amd.trainer import GutTrainer
    dev = torch.device(DEV)
    sc = scenes.syn_a(n=3000, sh_degree=1)
    target = scenes.target_image(sc.height, sc.width).to(dev)
    a = GutTrainer(sc, dev, iterations=100, rasterizer=rasterizer, loss="l1_ssim", mask_mode="ignore")
    b = GutTrainer(sc, dev, iterations=100, rasterizer=rasterizer, loss="l1_ssim")
    for step in range(3):
        la, lb = float(a.train_step([target], views=[0], masks=[None])), float(b.train_step([target], views=[0]))
        assert a.last_plan == b.last_plan
        # the same kernels on the same inputs; their float atomics arrive in any order, so two runs of ONE trainer differ in the last bits as well
        assert abs(la - lb) < (1e-6 if step == 0 else 1e-5)
    assert a._masks is None
