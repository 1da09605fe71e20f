"""GPU: depth-supervised training through GutTrainer: the fastgs step with a depth target against fast_rasterize under autograd, the direction of the
depth loss on a scene started from perturbed means, the step without depths left bit for bit alone, the refused combinations and the weight schedule.
Scene: tests/test_oracle_fastgs._scene (3000 Gaussians, 160 x 112, one camera) turned into a trainer Scene."""
import math

import numpy as np
import pytest
import torch

from gpu_util import n, rel_l2
from test_gpu_fastgs_antialiased import _deterministic
from test_oracle_fastgs import _scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CFG = dict(N=3000, W=160, H=112, seed=0, deg=1)


def _trainer_scene(sc, means=None):
    from lichtfeld_studio_amd.scenes import Scene
    f32 = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32)
    K = torch.tensor([[[sc["fx"], 0, sc["cx"]], [0, sc["fy"], sc["cy"]], [0, 0, 1]]], dtype=torch.float32)
    return Scene("depth-test", sc["W"], sc["H"], 1, f32(sc["means"] if means is None else means), f32(sc["rot_raw"]), f32(sc["scales_raw"]), f32(sc["opac_raw"]),
                 f32(sc["sh0"]), f32(sc["sh_rest"][:, :3]), f32(sc["w2c"])[None], K)


def _render(tr, kind):
    """(image, alpha, accumulated depth map) of the trainer's model at view 0"""
    from lichtfeld_studio_amd import fastgs
    from lichtfeld_studio_amd.rasterizer import RenderMode
    with torch.no_grad():
        r = fastgs.fast_rasterize(tr.camera(0), tr.model, torch.zeros(3, device=DEV), render_mode=RenderMode.RGB_D, depth_kind=kind)
    return r.image, r.alpha, r.depth


def _ground_truth(kind):
    """targets rendered from the ground-truth scene: (image, PreparedDepth of its accumulated depth map - uncovered pixels carry 0 and are invalid)"""
    from lichtfeld_studio_amd import losses
    from lichtfeld_studio_amd.trainer import GutTrainer
    gt = GutTrainer(_trainer_scene(_scene(**CFG)), torch.device(DEV), iterations=100, rasterizer="fastgs")
    image, _, depth = _render(gt, kind)
    return image.contiguous(), losses.prepare_depth(depth)


def _perturbed():
    sc = _scene(**CFG)
    rng = np.random.default_rng(77)
    ray = sc["means"] - sc["cam_pos"][None, :]
    ray /= np.linalg.norm(ray, axis=1, keepdims=True)
    return _trainer_scene(sc, sc["means"] + 0.02 * rng.standard_normal(sc["means"].shape) + ray * (0.25 * rng.standard_normal((len(ray), 1))))


def _depth_l1(tr, pd, kind):
    _, _, d = _render(tr, kind)
    valid = ~torch.isnan(pd.target)
    return float((d[0] - pd.target)[valid].abs().mean())


@pytest.mark.parametrize("kind", ["invdepth", "depth"])
def test_depth_step_matches_autograd(lfs, kind):
    """GutTrainer(depth_loss=kind).train_step(depths=...) against fast_rasterize(RGB_D) + torch autograd: the bounds of test_fastgs_trainer_step_matches_autograd"""
    from lichtfeld_studio_amd import fastgs
    from lichtfeld_studio_amd.rasterizer import RenderMode
    from lichtfeld_studio_amd.trainer import GutTrainer
    dev = torch.device(DEV)
    target, pd = _ground_truth(kind)
    w = (0.7, 0.01)
    tr = GutTrainer(_perturbed(), dev, iterations=100, rasterizer="fastgs", depth_loss=kind, depth_weight=w)
    ref = fastgs.fast_rasterize(tr.camera(0), tr.model, torch.zeros(3, device=dev), render_mode=RenderMode.RGB_D, depth_kind=kind)
    valid = ~torch.isnan(pd.target)
    l1 = ((ref.depth[0] - torch.where(valid, pd.target, torch.zeros_like(pd.target))).abs() * valid).sum() / max(float(valid.sum()), 1.0)
    loss_ref = torch.nn.functional.mse_loss(ref.image, target) + w[0] * l1
    loss_ref.backward()
    ref_grads = [p.grad.clone() for p in tr.model.parameters()]
    for p in tr.model.parameters():
        p.grad = None
    loss = tr.train_step([target], views=[0], depths=[pd])
    print(f"{kind}: loss {float(loss):.8f}, autograd {float(loss_ref):.8f}, depth term {float(w[0] * l1):.6f}")
    assert tr.last_plan.path == "fastgs" and abs(float(loss) - float(loss_ref)) < 1e-6 and float(w[0] * l1) > 1e-4
    for name, g, r in zip(["means", "sh0", "shN", "raw_scales", "raw_quats", "raw_opacities"], tr.bucket.views, ref_grads):
        e = rel_l2(n(g), n(r).reshape(n(g).shape))
        print(f"{kind} {name}: rel-L2 {e:.2e} (< 1e-4)")
        assert e < 1e-4, name


def test_depth_loss_lowers_the_depth_error(lfs):
    """60 steps from perturbed means against targets rendered from the ground truth: the depth L1 after the run with depth_loss="invdepth" is lower than the twin
    trainer's without it (the amount is printed, the direction asserted)."""
    from lichtfeld_studio_amd.trainer import GutTrainer
    dev = torch.device(DEV)
    target, pd = _ground_truth("invdepth")
    a = GutTrainer(_perturbed(), dev, iterations=60, rasterizer="fastgs", depth_loss="invdepth")
    b = GutTrainer(_perturbed(), dev, iterations=60, rasterizer="fastgs")
    start = _depth_l1(a, pd, "invdepth")
    for _ in range(60):
        a.train_step([target], views=[0], depths=[pd])
        b.train_step([target], views=[0])
    ea, eb = _depth_l1(a, pd, "invdepth"), _depth_l1(b, pd, "invdepth")
    print(f"inverse-depth L1 against the targets: start {start:.6f}, after 60 steps with the depth loss {ea:.6f}, without {eb:.6f}: ratio {ea / eb:.4f} (< 1)")
    assert ea / eb < 1.0 and ea < start


def test_steps_without_depths_are_the_old_steps_and_the_refused_combinations_raise(lfs):
    from lichtfeld_studio_amd.trainer import GutTrainer
    dev = torch.device(DEV)
    sc = _perturbed()
    target, pd = _ground_truth("invdepth")
    with _deterministic(lfs):
        plain = GutTrainer(sc, dev, iterations=100, rasterizer="fastgs")
        off = GutTrainer(sc, dev, iterations=100, rasterizer="fastgs", depth_loss="none")
        unused = GutTrainer(sc, dev, iterations=100, rasterizer="fastgs", depth_loss="invdepth")
        for _ in range(5):
            la, lb, lc = plain.train_step([target], views=[0]), off.train_step([target], views=[0], depths=None), unused.train_step([target], views=[0], depths=[None])
            assert abs(float(la) - float(lb)) < 2e-6 and abs(float(la) - float(lc)) < 2e-6   # (the loss kernel's blocks add with float atomics: the value, not its bits)
        for p, q, r in zip(plain.model.parameters(), off.model.parameters(), unused.model.parameters()):
            assert torch.equal(p, q) and torch.equal(p, r)
        assert plain.last_plan == off.last_plan == unused.last_plan
        used = GutTrainer(sc, dev, iterations=100, rasterizer="fastgs", depth_loss="invdepth")
        for _ in range(5):
            used.train_step([target], views=[0], depths=[pd])
        assert not torch.equal(used.model.means, plain.model.means)
    with pytest.raises(ValueError, match="not wired into the 3DGUT route"):
        GutTrainer(sc, dev, iterations=100, rasterizer="gut", depth_loss="invdepth")
    with pytest.raises(ValueError, match="one rank"):
        GutTrainer(sc, dev, iterations=100, rasterizer="fastgs", depth_loss="depth", world=2)
    with pytest.raises(ValueError, match="Invalid depth loss"):
        GutTrainer(sc, dev, iterations=100, rasterizer="fastgs", depth_loss="median")
    with pytest.raises(ValueError, match="both > 0"):
        GutTrainer(sc, dev, iterations=100, rasterizer="fastgs", depth_loss="depth", depth_weight=(1.0, 0.0))
    with pytest.raises(ValueError, match="needs GutTrainer\\(depth_loss="):
        plain.train_step([target], views=[0], depths=[pd])
    with pytest.raises(ValueError, match="parallel to targets"):
        used.train_step([target], views=[0], depths=[pd, pd])
    # the schedule: first and last weights are the configured ones, log-linear between
    s = GutTrainer(sc, dev, iterations=101, rasterizer="fastgs", depth_loss="invdepth", depth_weight=(0.8, 0.02))
    assert s.depth_weight_at(1) == pytest.approx(0.8, rel=1e-12) and s.depth_weight_at(101) == pytest.approx(0.02, rel=1e-12) and s.depth_weight_at(500) == pytest.approx(0.02, rel=1e-12)
    assert s.depth_weight_at(51) == pytest.approx(math.sqrt(0.8 * 0.02), rel=1e-12)
    d = GutTrainer(sc, dev, iterations=100, rasterizer="fastgs", depth_loss="invdepth")
    assert d.depth_weight == (1.0, 0.01)
