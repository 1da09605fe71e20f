"""GPU: GutTrainer(contribution_prune_at=..., contribution_threshold=...): the RadSplat prune on the blending-weight statistic inside a training run.

Scene: the 3000 Gaussians of tests/test_gpu_depth_training.py (CFG: 160 x 112) seen by two cameras 0.1 apart, plus - built in the frame of camera 0 -
  * a WALL 1.5 in front of the camera: three coplanar layers (z = 1.5, 1.55, 1.6) of 21 x 15 Gaussians of opacity 0.99 on a 0.05 grid, scales 0.04 / 0.045 / 0.05 (the
    later layers slightly larger). A pixel under the wall meets four or more of them per layer at alpha >= 0.69: T < 0.01 behind the first layer, < 1e-4 inside the
    second or third - the pixels terminate INSIDE the wall;
  * 200 HIDDEN Gaussians (scale 0.01, opacity 0.9) at z = 2.5 behind the wall's centre, within +-10 x +-7 px of it; their 1/255 extent is 2 px and the wall reaches
    +-23 x +-16 px (the second camera moves the two against each other by 2 px): every pixel they cover has terminated before the walk reaches them, in both views.
Opacity-based pruning keeps the 200 (opacity 0.9); no training ray blends them."""
import numpy as np
import pytest
import torch

from test_gpu_depth_training import CFG
from test_gpu_fastgs_antialiased import _deterministic
from test_oracle_fastgs import _scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_HIDDEN = 200
PRUNE_AT = 20


def _hidden_scene(baseline=0.1, zh=2.5):
    """-> (trainer Scene with two views, the world-space means of the 200 hidden Gaussians)"""
    from lichtfeld_studio_amd.scenes import Scene
    sc = _scene(**CFG)
    R, t = sc["w2c"][:3, :3], sc["w2c"][:3, 3]
    to_world = lambda p_cam: (p_cam - t[None, :]) @ R          # R^T (p - t), row vectors
    gx, gy = np.meshgrid(np.arange(-10, 11) * 0.05, np.arange(-7, 8) * 0.05)
    wall_cam, wall_scale = [], []
    for z, s in ((1.5, 0.04), (1.55, 0.045), (1.6, 0.05)):
        wall_cam.append(np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, z)], 1))
        wall_scale.append(np.full(gx.size, s))
    wall_cam, wall_scale = np.concatenate(wall_cam), np.concatenate(wall_scale)
    rng = np.random.default_rng(21)
    hid_cam = np.stack([rng.uniform(-10, 10, N_HIDDEN) / sc["fx"] * zh, rng.uniform(-7, 7, N_HIDDEN) / sc["fy"] * zh, np.full(N_HIDDEN, zh)], 1)
    hidden_world = to_world(hid_cam)
    n_new = len(wall_cam) + N_HIDDEN
    logit = lambda p: np.log(p / (1 - p))
    means = np.concatenate([sc["means"], to_world(wall_cam), hidden_world])
    scales = np.concatenate([sc["scales_raw"], np.log(np.repeat(np.concatenate([wall_scale, np.full(N_HIDDEN, 0.01)])[:, None], 3, 1))])
    rot = np.concatenate([sc["rot_raw"], np.tile([1.0, 0, 0, 0], (n_new, 1))])
    opac = np.concatenate([sc["opac_raw"], np.full(len(wall_cam), logit(0.99)), np.full(N_HIDDEN, logit(0.9))])
    sh0 = np.concatenate([sc["sh0"], rng.standard_normal((n_new, 1, 3)) * 0.5])
    shN = np.concatenate([sc["sh_rest"][:, :3], np.zeros((n_new, 3, 3))])
    w2c = np.stack([sc["w2c"], sc["w2c"]])
    w2c[1, 0, 3] += baseline
    f32 = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32)
    K = torch.tensor([[sc["fx"], 0, sc["cx"]], [0, sc["fy"], sc["cy"]], [0, 0, 1]], dtype=torch.float32).repeat(2, 1, 1)
    return Scene("hidden-test", sc["W"], sc["H"], 1, f32(means), f32(rot), f32(scales), f32(opac), f32(sh0), f32(shN), f32(w2c), K), f32(hidden_world)


def _targets(scene):
    from lichtfeld_studio_amd import scenes
    return [scenes.target_image(scene.height, scene.width, seed=43 + v).to(DEV) for v in range(2)]


def _state(tr):
    """every parameter and both Adam moments of every group, as clones"""
    out = []
    for p in tr.model.parameters():
        st = tr.optimizer.state.get(id(p))
        out += [p.detach().clone()] + ([st["exp_avg"].clone(), st["exp_avg_sq"].clone()] if st is not None else [])
    return out


def _rows_present(means, wanted):
    """bool [len(wanted)]: is row wanted[k] (bit for bit) among the rows of means"""
    return torch.tensor([bool((means == w).all(dim=1).any()) for w in wanted.to(means.device)])


def _step(tr, targets):
    v = tr.iteration % 2
    return tr.train_step([targets[v]], views=[v])


def test_prune_removes_the_hidden_gaussians_and_training_goes_on(lfs):
    from lichtfeld_studio_amd.trainer import GutTrainer
    dev = torch.device(DEV)
    scene, hidden = _hidden_scene()
    targets = _targets(scene)
    with _deterministic(lfs):
        on = GutTrainer(scene, dev, iterations=100, rasterizer="fastgs", contribution_prune_at=(PRUNE_AT,), contribution_threshold=0.01)
        off = GutTrainer(scene, dev, iterations=100, rasterizer="fastgs")
        n0 = scene.means.shape[0]
        # 1. off means unchanged: through iteration 19 the twin without the option holds the same bits
        for _ in range(PRUNE_AT - 1):
            _step(on, targets)
            _step(off, targets)
        assert on.iteration == off.iteration == PRUNE_AT - 1
        a, b = _state(on), _state(off)
        assert len(a) == len(b) >= 16      # (six parameters, two moments for each group the optimizer has stepped)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        # the hidden rows as they stand before the prune (training moved them: they are identified by their means in the twin, which holds the same bits)
        assert on.contribution_log == []
        _step(on, targets)
        _step(off, targets)
        hidden_now = off.model.means.detach()[n0 - N_HIDDEN:]
        # 2. iteration 20 pruned: at least the 200, and all of the 200
        n1 = on.model.means.shape[0]
        print(f"N {n0} -> {n1}; log {on.contribution_log}")
        assert on.contribution_log == [(PRUNE_AT, n0, n1)] and n1 <= n0 - N_HIDDEN
        assert not _rows_present(on.model.means.detach(), hidden_now).any()
        assert off.model.means.shape[0] == n0
        # 3. every parameter and both moments of every group follow
        for x in _state(on):
            assert x.shape[0] == n1
        # 4. ten more steps
        for _ in range(10):
            loss = _step(on, targets)
            assert torch.isfinite(loss).all()
        assert on.model.means.shape[0] == n1 and on.contribution_log == [(PRUNE_AT, n0, n1)]
        # (5. is test_zero_row_prune_leaves_the_image_of_the_scene_as_built_alone; the same prune on THIS twin, trained for 30 steps towards noise targets, is printed:
        # 4 pixels change by 1.3e-5 / 1.6e-5 there - a few small Gaussians deep in the scene have become pure terminators, the caveat of DESIGN.md 8m)
        for d, same, n_rows in _zero_row_prune_changes(off):
            print(f"after 30 steps: threshold -> 0+ prune of {n_rows} rows: max image change {d:.3e}, bit-identical {same}")


def _zero_row_prune_changes(tr):
    """remove the rows with max_w == 0 over both views (threshold -> 0+: no float below 1e-30 is a blending weight, w >= 1e-4 / 255) from the trainer's model ->
    per view (max abs image change, bit-identical, rows removed)"""
    from lichtfeld_studio_amd import fastgs
    from lichtfeld_studio_amd.contribution import compute_contribution, prune_mask
    cams = [tr.camera(v) for v in range(2)]
    stats = compute_contribution(tr.model, cams)
    mask = prune_mask(stats, threshold=1e-30)
    assert torch.equal(mask, stats.max_w == 0) and int(mask.sum()) >= N_HIDDEN
    n_before = tr.model.means.shape[0]
    bg = torch.zeros(3, device=DEV)
    with torch.no_grad():
        before = [fastgs.fast_rasterize(c, tr.model, bg).image.clone() for c in cams]
        tr._remove_gaussians(mask)
        after = [fastgs.fast_rasterize(c, tr.model, bg).image for c in cams]
    assert tr.model.means.shape[0] == n_before - int(mask.sum())
    return [(float((x - y).abs().max()), torch.equal(x, y), int(mask.sum())) for x, y in zip(before, after)]


def test_zero_row_prune_leaves_the_image_of_the_scene_as_built_alone(lfs):
    """5. Removing the rows with max_w == 0 does not change the image: at most 1e-6 per pixel, expected bit-identical. In general it may change it: a row is also empty
    when its Gaussian only ever TERMINATES pixels, and without it those pixels run on with the transmittance they had. It holds for THIS scene, as built, only: here no
    pruned Gaussian passes the alpha test at a live pixel. Its empty rows are the Gaussians behind the cameras or outside both frusta, and Gaussians - the 200 hidden ones
    among them - whose whole footprint lies where every pixel died in front of them. For a Gaussian to terminate without ever being blended, every live pixel of its
    footprint must have T (1 - alpha) < 1e-4 <= T; at the rim of the footprint (alpha ~ 1/255) that is T in [1e-4, 1.004e-4], so live pixels may meet only its core - no
    Gaussian of the scene as built is in that position in both views (checked here, not provable in general). It does NOT hold for any model: the twin of the test above,
    after 30 steps towards noise targets, has a few such Gaussians (4 pixels change by 1.3e-5 and 1.6e-5; printed there)."""
    from lichtfeld_studio_amd.trainer import GutTrainer
    scene, _ = _hidden_scene()
    tr = GutTrainer(scene, torch.device(DEV), iterations=100, rasterizer="fastgs")
    for d, same, n_rows in _zero_row_prune_changes(tr):
        print(f"scene as built: threshold -> 0+ prune of {n_rows} rows: max image change {d:.3e}, bit-identical {same}")
        assert d <= 1e-6


def test_hidden_gaussians_survive_an_opacity_prune_but_not_this_one(lfs):
    """the statistic of the untrained scene: the 200 rows are empty although their opacity is 0.9 and the preprocess puts them on tiles; the wall's front layer is not"""
    from lichtfeld_studio_amd.contribution import compute_contribution, prune_mask
    from lichtfeld_studio_amd.trainer import GutTrainer
    scene, _ = _hidden_scene()
    tr = GutTrainer(scene, torch.device(DEV), iterations=100, rasterizer="fastgs")
    stats = compute_contribution(tr.model, [tr.camera(v) for v in range(2)])
    n0 = scene.means.shape[0]
    assert stats.views == 2
    assert not bool(stats.max_w[n0 - N_HIDDEN:].any()) and not bool(stats.n_pix[n0 - N_HIDDEN:].any())
    assert bool((torch.sigmoid(tr.model.raw_opacities.detach()[n0 - N_HIDDEN:]) > 0.89).all())
    front = slice(CFG["N"], CFG["N"] + 315)
    assert bool((stats.max_w[front] > 0.05).all())      # (its neighbours of equal depth and lower index stand in front of it: well below 0.99, well above the threshold)
    mask = prune_mask(stats, threshold=0.01)
    assert bool(mask[n0 - N_HIDDEN:].all()) and not bool(mask[front].any())
    k = prune_mask(stats, keep=n0 - N_HIDDEN)
    assert int(k.sum()) == N_HIDDEN


@pytest.mark.parametrize("kw", [dict(strategy="default"), dict(filter3d=True, antialiasing=True), dict(visible_adam=True)], ids=["adc", "filter3d", "visible_adam"])
def test_prune_with_the_other_options(lfs, kw):
    """3. with ADC the strategy's accumulators (densification_info) follow; 6. with filter3d the filter tensor has the new N; 7. with visible_adam the next step runs"""
    from lichtfeld_studio_amd.trainer import GutTrainer
    scene, _ = _hidden_scene()
    targets = _targets(scene)
    tr = GutTrainer(scene, torch.device(DEV), iterations=100, rasterizer="fastgs", contribution_prune_at=(3,), contribution_threshold=0.01, **kw)
    n0 = scene.means.shape[0]
    for _ in range(3):
        _step(tr, targets)
    n1 = tr.model.means.shape[0]
    assert tr.contribution_log == [(3, n0, n1)] and n1 <= n0 - N_HIDDEN
    if "strategy" in kw:
        assert tr.densification_info is not None and tr.densification_info.shape == (2, n1)
    if kw.get("filter3d"):
        assert tr.filter3d_var is not None and tr.filter3d_var.shape == (n1,)
    for _ in range(2):
        loss = _step(tr, targets)
        assert torch.isfinite(loss).all()
    for x in _state(tr):
        assert x.shape[0] == n1
    if "strategy" in kw:
        assert tr.densification_info.shape == (2, n1)
    if kw.get("visible_adam"):
        assert tr._vis_bits is not None and tr._vis_bits.numel() == (n1 + 31) // 32


def test_refused_combinations(lfs):
    from lichtfeld_studio_amd.trainer import GutTrainer
    scene, _ = _hidden_scene()
    dev = torch.device(DEV)
    base = dict(iterations=100, rasterizer="fastgs", contribution_prune_at=(20,))
    for bad, word in [(dict(rasterizer="gut"), "3DGUT"), (dict(world=2), "one rank"), (dict(strategy="mcmc"), "mcmc"), (dict(one_call=True), "one_call"),
                      (dict(contribution_prune_at=(0,)), "outside"), (dict(contribution_prune_at=(20, 101)), "outside"), (dict(contribution_threshold=0.0), "(0, 1)"),
                      (dict(contribution_threshold=1.0), "(0, 1)")]:
        with pytest.raises(ValueError, match=word.replace("(", r"\(").replace(")", r"\)")):
            GutTrainer(scene, dev, **{**base, **bad})
    tr = GutTrainer(scene, dev, iterations=100, rasterizer="fastgs")      # the empty default: no prune iterations, nothing refused
    assert tr.contribution_prune_at == frozenset() and tr.contribution_log == []


def test_prune_inside_three_steps_on_a_small_scene(lfs):
    """257 Gaussians at 96 x 80, two views, a fifth of them behind both cameras - small enough to run on the wavefront emulator as well
    (tests/test_emulated_fastgs_contribution.py): the prune at the end of iteration 2 removes at least the 52 nobody sees, every row follows, step 3 runs"""
    from lichtfeld_studio_amd.scenes import Scene
    from lichtfeld_studio_amd.trainer import GutTrainer
    from test_gpu_fastgs_contribution import _named_scene, _second_view
    sc = _named_scene("n257")
    f32 = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32)
    K = torch.tensor([[sc["fx"], 0, sc["cx"]], [0, sc["fy"], sc["cy"]], [0, 0, 1]], dtype=torch.float32).repeat(2, 1, 1)
    scene = Scene("small-prune-test", sc["W"], sc["H"], 1, f32(sc["means"]), f32(sc["rot_raw"]), f32(sc["scales_raw"]), f32(sc["opac_raw"]), f32(sc["sh0"]),
                  f32(sc["sh_rest"][:, :3]), f32(np.stack([sc["w2c"], _second_view(sc)["w2c"]])), K)
    targets = _targets(scene)
    tr = GutTrainer(scene, DEV, iterations=100, rasterizer="fastgs", contribution_prune_at=(2,), contribution_threshold=0.01)
    behind = tr.model.means.detach()[4::5].clone()
    for _ in range(2):
        _step(tr, targets)
    n1 = tr.model.means.shape[0]
    assert tr.contribution_log == [(2, 257, n1)] and 0 < n1 <= 257 - 52
    assert not _rows_present(tr.model.means.detach(), behind).any()      # (their gradients are zero: they are where they started)
    loss = _step(tr, targets)
    assert torch.isfinite(loss).all()
    for x in _state(tr):
        assert x.shape[0] == n1
