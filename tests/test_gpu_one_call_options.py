"""GPU: GutTrainer(one_call=True) - L1 + D-SSIM, MCMC between refinements and iteration <= 1000 through the one-call step (lfs_gut_train_step_opt: loss kernels on the
workspace's render, the noise and the shN freeze inside the fused tail) - against the default trainer, whose steps for those configurations keep gradient tensors
(lfs_gut_view_forward / _backward_sh / _backward_finish, lfs_add_noise, FusedAdam): bit for bit in the deterministic accumulation mode (debug bit 16), within the split
form's own run-to-run noise with float atomics, at the headline size, and without a host synchronisation."""
import pytest
import torch

from gpu_util import atomic_noise_bar, noise_check, rel_l2, n

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ["means", "sh0", "shN", "raw_scales", "raw_quats", "raw_opacities"]


def _scene(n_gauss=6000):
    """scenes.syn_a (one camera) with two more cameras nearby: the round-robin schedule then renders another view on every step, and the tail prepares ITS colours"""
    import numpy as np
    from gpu_util import small_rotation_viewmat
    from lichtfeld_studio_amd import scenes
    sc = scenes.syn_a(n=n_gauss, sh_degree=2)
    more = [torch.from_numpy(small_rotation_viewmat(np.random.default_rng(s), a, 0.1)) for s, a in ((3, 0.06), (4, 0.1))]
    sc.viewmats = torch.cat([sc.viewmats, torch.stack(more)], 0).contiguous()
    sc.Ks = sc.Ks.repeat(3, 1, 1).contiguous()
    return sc


def _kw(kind, n_gauss):
    from lichtfeld_studio_amd import strategies
    if kind == "mcmc":
        return dict(loss="l1_ssim", strategy="mcmc", opt_params=strategies.OptimizationParameters(iterations=30000, max_cap=n_gauss, scale_reg=0.01, opacity_reg=0.01))
    return dict(loss=kind)


def _pair(sc, kind, start, **extra):
    from lichtfeld_studio_amd.trainer import GutTrainer
    kw = _kw(kind, sc.means.shape[0])
    a, b = GutTrainer(sc, DEV, iterations=30000, one_call=True, **kw, **extra), GutTrainer(sc, DEV, iterations=30000, **kw, **extra)
    a.iteration = b.iteration = start
    return a, b


def _same_state(a, b, tag):
    for name, pa, pb in zip(NAMES, a.model.parameters(), b.model.parameters()):
        pa, pb = pa.detach(), pb.detach()
        assert pa.shape == pb.shape and torch.equal(pa, pb), (tag, name, float((pa - pb).abs().max()))
        sa, sb = a.optimizer.state[id(getattr(a.model, name))], b.optimizer.state[id(getattr(b.model, name))]
        assert sa["step_count"] == sb["step_count"], (tag, name, sa["step_count"], sb["step_count"])
        assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]), (tag, name)


# kind, first iteration - 1, the form the one-call trainer must take on each of the five steps (path, freeze_shN), the default trainer's paths
CASES = {
    "l1_ssim": ("l1_ssim", 1598, [("cxx_all", False)] * 5, ["cxx_views"] * 5),
    # the refining iteration 1600 lies inside the run: relocation rewrites rows and moments first - the split form for that step, the one-call form again after it
    "l1_ssim_mcmc": ("mcmc", 1597, [("cxx_all", False), ("cxx_all", False), ("cxx_views", False), ("cxx_all", False), ("cxx_all", False)], ["cxx_views"] * 5),
    "mse_across_1000": ("mse", 998, [("cxx_all", True), ("cxx_all", True), ("cxx_all", False), ("cxx_all", False), ("cxx_all", False)],
                        ["cxx_views", "cxx_views", "cxx_all", "cxx_all", "cxx_all"]),
    "l1_ssim_across_1000": ("l1_ssim", 998, [("cxx_all", True), ("cxx_all", True), ("cxx_all", False), ("cxx_all", False), ("cxx_all", False)], ["cxx_views"] * 5),
}


@pytest.mark.parametrize("case", list(CASES))
def test_one_call_trainer_is_bit_identical_to_the_default_trainer(lfs, case):
    kind, start, want_a, want_b = CASES[case]
    sc = _scene()
    target = torch.rand(3, sc.height, sc.width, generator=torch.Generator().manual_seed(5)).to(DEV) * 0.7
    lib = lfs.load_library()
    try:
        lib.lfs_set_debug_flags(16)
        a, b = _pair(sc, kind, start)
        for step in range(5):     # no `views`: the round-robin schedule rotates over the scene's views and names the next one
            la, lb = a.train_step([target]), b.train_step([target])
            assert (a.last_plan.path, a.last_plan.freeze_shN) == want_a[step], (case, step, a.last_plan)
            assert b.last_plan.path == want_b[step] and not b.last_plan.freeze_shN, (case, step, b.last_plan)
            assert a.last_n_isects == b.last_n_isects > 0, (case, step)
            # (the loss value is a float-atomic sum of partials in either form: tests/test_gpu_gut_step.py:103 compares it the same way)
            print(case, step, "loss", float(la), float(lb))
            noise_check(f"one-call vs split loss value {case} step {step}", abs(float(la) - float(lb)), 1e-5 * abs(float(lb)))
            assert float(la) > 0
            _same_state(a, b, (case, step))
        torch.cuda.synchronize()
    finally:
        lib.lfs_set_debug_flags(0)
    assert a.model.active_sh_degree == b.model.active_sh_degree
    assert a._gut_step.colour_launches_saved >= 1, "no step found its SH colours prepared by the step before"
    assert a._gut_step.retries <= 2


def test_one_call_trainer_within_the_split_forms_own_noise_with_float_atomics(lfs):
    """Debug bit 16 off: the rasterizer backward accumulates with float atomics, and two runs of the SAME form differ. The one-call form must lie within the noise
    of the split form: per parameter, the relative L2 distance to one split run after five steps against atomic_noise_bar over three split runs."""
    from lichtfeld_studio_amd.trainer import GutTrainer
    sc = _scene()
    target = torch.rand(3, sc.height, sc.width, generator=torch.Generator().manual_seed(5)).to(DEV) * 0.7
    kw = _kw("mcmc", 6000)

    def run(one_call):
        tr = GutTrainer(sc, DEV, iterations=30000, one_call=one_call, **kw)
        tr.iteration = 1600          # five steps between two refinements
        for _ in range(5):
            tr.train_step([target])
            assert tr.last_plan.path == ("cxx_all" if one_call else "cxx_views")
        torch.cuda.synchronize()
        return [n(p) for p in tr.model.parameters()]

    split = [run(False) for _ in range(3)]
    new = run(True)
    for k, name in enumerate(NAMES):
        bar = atomic_noise_bar(split[0][k], split[1][k], split[2][k])
        d = rel_l2(new[k], split[0][k])
        noise_check(f"one-call vs split, float atomics: {name}", d, bar)


def test_one_call_l1_ssim_step_at_the_headline_size_is_bit_identical(lfs):
    """1 M Gaussians, 1920 x 1080, SH degree 3 (SYN-B): one L1 + D-SSIM step, deterministic mode."""
    from lichtfeld_studio_amd import scenes
    sc = scenes.syn_b(n=1_000_000, n_views=2)
    assert (sc.width, sc.height) == (1920, 1080) and sc.sh_degree == 3
    target = scenes.target_image(sc.height, sc.width).to(DEV)
    lib = lfs.load_library()
    try:
        lib.lfs_set_debug_flags(16)
        a, b = _pair(sc, "l1_ssim", 3000)
        la, lb = a.train_step([target]), b.train_step([target])
        torch.cuda.synchronize()
    finally:
        lib.lfs_set_debug_flags(0)
    assert a.last_plan.path == "cxx_all" and b.last_plan.path == "cxx_views"
    assert a.last_n_isects == b.last_n_isects > 1_000_000
    noise_check("one-call vs split loss value, headline size", abs(float(la) - float(lb)), 1e-5 * abs(float(lb)))
    _same_state(a, b, "headline")


def test_one_call_l1_ssim_mcmc_step_enqueues_without_a_host_synchronisation(lfs):
    """After a warm-up (module loads, the workspaces, the capacity settled) an L1 + D-SSIM + noise step is enqueued under torch's sync debug mode "error": no
    .item(), no blocking copy, no stream synchronisation - only the spin on the pinned counts the MSE step has as well (not a torch synchronisation)."""
    from lichtfeld_studio_amd.trainer import GutTrainer
    sc = _scene()
    target = torch.rand(3, sc.height, sc.width, generator=torch.Generator().manual_seed(5)).to(DEV) * 0.7
    tr = GutTrainer(sc, DEV, iterations=30000, one_call=True, **_kw("mcmc", 6000))
    tr.iteration = 1600
    for _ in range(3):
        tr.train_step([target])
    torch.cuda.synchronize()
    before = tr.model.means.detach().clone()
    retries = tr._gut_step.retries
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(2):
            loss = tr.train_step([target])
            assert tr.last_plan.path == "cxx_all"
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert tr._gut_step.retries == retries
    assert float(loss) > 0 and not torch.equal(before, tr.model.means.detach())


def test_one_call_switch_leaves_a_degree_4_model_on_the_default_forms(lfs):
    """K = 25 > 16: the fused tail has no instantiation for it, so lfs_gut_train_step_opt would answer LFS_E_UNSUPPORTED for a frozen shN or a noise tensor. The trainer
    does not ask: with one_call=True such a model takes the forms it takes without the switch, and the same steps."""
    from lichtfeld_studio_amd import scenes
    from lichtfeld_studio_amd.trainer import GutTrainer
    sc = scenes.syn_a(n=3000, sh_degree=4)
    target = torch.rand(3, sc.height, sc.width, generator=torch.Generator().manual_seed(5)).to(DEV) * 0.7
    lib = lfs.load_library()
    try:
        lib.lfs_set_debug_flags(16)
        for start in (998, 1600):
            kw = _kw("mcmc", 3000)
            a, b = GutTrainer(sc, DEV, iterations=30000, one_call=True, **kw), GutTrainer(sc, DEV, iterations=30000, **kw)
            a.iteration = b.iteration = start
            for step in range(3):
                a.train_step([target]), b.train_step([target])
                assert a.last_plan == b.last_plan and a.last_plan.path == "cxx_views", (start, step, a.last_plan)
            _same_state(a, b, ("degree 4", start))
        torch.cuda.synchronize()
    finally:
        lib.lfs_set_debug_flags(0)
