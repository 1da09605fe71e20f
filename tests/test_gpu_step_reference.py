"""GPU: the one-call training step on the device - GutStep.train_step (lfs_gut_train_step_opt / lfs_gut_train_step_ex) and GutTrainer(one_call=True) - against
tests/step_reference.py, the float64 PyTorch model of the step that torch.autograd differentiates (written from the reference's sources; see its docstring). The same
per-step checks as tests/test_emulated_step_reference.py (tests/step_reference_checks.py: gradients teacher-forced through the Adam moments at 2e-4 with at most two
flip rows, the loss value at 2e-6, the update within four times the fp32 oracle's own distance from float64 Adam / noise, exact zeros on unlisted rows and clamped
colour channels; every scene guarded by the fp32 oracle passing the same gradient check with no row set aside), here on what the emulator cannot show: v_exp_f32 /
v_rcp_f32, the DPP reductions and the atomics of the real kernels. Deterministic accumulation (debug bit 16) except for the float-atomics case.
Needs oracle/ and tests/golden/ only. The headline size (1 M Gaussians at 1080p) is out of reach of an autograd graph: the largest scene here has 20 000."""
import numpy as np
import pytest
import torch

import step_reference_checks as chk
from gpu_util import atomic_noise_bar, rows_check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GROUPS = ("means", "sh0", "shN", "raw_scales", "raw_quats", "raw_opacities")


class _Run:
    """the six parameters and their moments on the device + one GutStep: what a caller of the C ABI keeps"""

    def __init__(self, sc):
        from lichtfeld_studio_amd.gut_step import GutStep
        self.sc = sc
        self.params = [torch.from_numpy(np.ascontiguousarray(sc[k], np.float32)).to(DEV).contiguous() for k in chk.NAMES]
        self.m = [torch.zeros_like(p) for p in self.params]
        self.v = [torch.zeros_like(p) for p in self.params]
        self.vms = torch.from_numpy(np.stack(sc["vms"])).to(DEV).contiguous()
        self.K = torch.from_numpy(sc["K"]).to(DEV).contiguous()
        self.bg = None if sc["bg"] is None else torch.from_numpy(sc["bg"]).to(DEV)
        self.target = torch.from_numpy(sc["target"]).to(DEV).contiguous()
        self.noise = [torch.from_numpy(x).to(DEV).contiguous() for x in sc["noise"]]
        self.loss = torch.zeros(1, device=DEV)
        self.gs = GutStep(DEV)

    def state(self):
        torch.cuda.synchronize()
        return dict(params=[p.cpu().numpy().copy() for p in self.params], m=[x.cpu().numpy().copy() for x in self.m], v=[x.cpu().numpy().copy() for x in self.v])

    def load(self, st):
        for dst, src in zip(self.params + self.m + self.v, st["params"] + st["m"] + st["v"]):
            dst.copy_(torch.from_numpy(src))
        self.gs.colors_for = None

    def step(self, it, loss, freeze, noise, last=False):
        sc = self.sc
        adam = {}
        for k, name in enumerate(GROUPS):
            if freeze and k == 2:
                continue
            lr, b1, b2, eps, bc1, bc2 = chk.adam_scalars(k, it + 1)
            adam[name] = dict(exp_avg=self.m[k], exp_avg_sq=self.v[k], lr=lr, beta1=b1, beta2=b2, eps=eps, bc1_rcp=bc1, bc2_sqrt_rcp=bc2)
        extra = {}
        if loss != "mse" or freeze or noise:
            extra = dict(loss=loss, lambda_dssim=chk.LAMBDA, freeze_shN=bool(freeze))
            if noise:
                extra.update(noise=self.noise[it], noise_lr=chk.NOISE_LR)
        n = self.gs.train_step(self.params, adam, sc["degree"], sc["W"], sc["H"], self.vms[it % 3], self.K, self.bg, self.target, chk.WEIGHT, self.loss,
                               chk.SCALE_REG, chk.OPACITY_REG, fused_tail=True, next_viewmat=None if last else self.vms[(it + 1) % 3], **extra)
        torch.cuda.synchronize()
        return n, float(self.loss)


def _check_run(lfs, oracle_mod, sc, steps, loss, freeze, noise, label):
    lib = lfs.load_library()
    try:
        lib.lfs_set_debug_flags(16)
        run = _Run(sc)
        before = run.state()
        for it in range(steps):
            n, loss_value = run.step(it, loss, freeze, noise, last=it == steps - 1)
            after = run.state()
            assert n > 0
            chk.check_step(oracle_mod, label, sc, it, before, after, loss_value, loss, bool(freeze), sc["noise"][it] if noise else None)
            before = after
    finally:
        lib.lfs_set_debug_flags(0)
    assert run.gs.colour_launches_saved == steps - 1, "the steps after the first did not render with the colours the previous tail handed over"


@pytest.mark.parametrize("loss,freeze,noise,K,degree,N", [("mse", 0, False, 16, 3, 3000), ("l1_ssim", 1, True, 4, 1, 3000), ("l1_ssim", 0, True, 16, 3, 3000),
                                                          ("mse", 1, True, 4, 1, 65), ("l1_ssim", 0, False, 16, 3, 65)])
def test_device_step_against_the_float64_autograd_model(lfs, oracle_mod, loss, freeze, noise, K, degree, N):
    sc = chk.make_scene(2000 * K + N, N, K, degree)
    _check_run(lfs, oracle_mod, sc, 3, loss, freeze, noise, f"gpu {loss} freeze={freeze} noise={noise} K={K} N={N}")


def test_device_step_on_a_ragged_image_without_background(lfs, oracle_mod):
    sc = chk.make_scene(11, 3000, 16, 3, W=203, H=117, background=False)
    _check_run(lfs, oracle_mod, sc, 3, "l1_ssim", 0, True, "gpu ragged")


def test_device_step_on_a_dense_scene_with_early_termination(lfs, oracle_mod):
    sc = chk.make_scene(19, 1500, 16, 3, W=128, H=128, spread=0.4, smin=0.05, smax=0.3)
    _check_run(lfs, oracle_mod, sc, 3, "l1_ssim", 0, True, "gpu dense")


def test_device_step_on_20000_gaussians(lfs, oracle_mod):
    sc = chk.make_scene(13, 20000, 16, 3, W=203, H=117, smin=0.01, smax=0.06)
    _check_run(lfs, oracle_mod, sc, 2, "l1_ssim", 0, True, "gpu 20000")


def test_device_step_with_float_atomics(lfs, oracle_mod):
    """Debug bit 16 off: the rasterizer backward accumulates with float atomics and two runs of the same step differ. One draw against the reference: the fp32 bar of the
    deterministic mode plus the noise of a draw, gpu_util.atomic_noise_bar over three draws of the same step (triangle inequality: draw - reference = (draw - the
    exact fp32 sum) + (fp32 - float64))."""
    sc = chk.make_scene(2000 * 16 + 3000, 3000, 16, 3)
    run = _Run(sc)
    start = run.state()
    draws = []
    for _ in range(3):
        run.load(start)
        _, loss_value = run.step(0, "l1_ssim", 0, True, last=True)
        draws.append((run.state(), loss_value))
    rec = [[chk.recovered_gradients(start, d[0], k) for k in range(6)] for d in draws]

    def grad_check(name, what, a, ref):
        k, j = chk.NAMES.index(name), ("g", "g2").index(what)
        bar = chk.GRAD_BAR + atomic_noise_bar(*[rec[i][k][j] for i in range(3)])
        total, flips, rest = rows_check(a, ref, bar=bar, max_flips=chk.MAX_FLIPS)
        print(f"float atomics {name} {what}: {total:.3e} ({flips} rows set aside -> {rest:.3e}) / bar {bar:.3e}")
        assert rest < bar, (name, what, total, flips, rest, bar)

    chk.check_step(oracle_mod, "gpu float atomics", sc, 0, start, draws[0][0], draws[0][1], "l1_ssim", False, sc["noise"][0], grad_check=grad_check)


@pytest.mark.parametrize("kind,start", [("mcmc", 1600), ("l1_ssim", 998)])
def test_one_call_trainer_against_the_float64_autograd_model(lfs, oracle_mod, kind, start):
    """GutTrainer(one_call=True): its own learning rates and schedule, the MCMC strategy's noise draw (start 1600: between two refinements) and, across iteration 1000,
    the frozen shN (start 998: two frozen steps, then one that updates it) - the scalars and the noise the trainer handed to the step are the ones the check uses."""
    from lichtfeld_studio_amd import scenes, strategies
    from lichtfeld_studio_amd.trainer import GutTrainer
    d = chk.make_scene(77, 3000, 16, 3)
    d["bg"] = np.zeros(3, np.float32)   # (the trainer's background)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    sc = scenes.Scene("step-reference", d["W"], d["H"], 3, t(d["means"]), t(d["raw_quats"]), t(d["raw_scales"]), t(d["raw_opac"]), t(d["sh0"]), t(d["shN"]),
                      t(np.stack(d["vms"])), t(np.stack([d["K"]] * 3)))
    kw = dict(loss="l1_ssim")
    if kind == "mcmc":
        kw.update(strategy="mcmc", opt_params=strategies.OptimizationParameters(iterations=30000, max_cap=3000, scale_reg=0.01, opacity_reg=0.01))
    target = t(d["target"]).to(DEV)
    lib = lfs.load_library()
    try:
        lib.lfs_set_debug_flags(16)
        tr = GutTrainer(sc, DEV, iterations=30000, one_call=True, **kw)
        tr.iteration = start
        names = ("means", "sh0", "shN", "raw_scales", "raw_quats", "raw_opacities")
        seen = {}
        prepare = tr.optimizer.prepare_inline
        tr.optimizer.prepare_inline = lambda p: seen.setdefault(id(p), prepare(p))
        if tr.strategy is not None:
            draw = tr.strategy.draw_noise
            tr.strategy.draw_noise = lambda: seen.setdefault("noise", draw())

        def state():
            torch.cuda.synchronize()
            ps = [getattr(tr.model, n_) for n_ in names]
            st = [tr.optimizer._state(p) for p in ps]
            return dict(params=[p.detach().cpu().numpy().copy() for p in ps], m=[s["exp_avg"].cpu().numpy().copy() for s in st], v=[s["exp_avg_sq"].cpu().numpy().copy() for s in st])

        before = state()
        for it in range(3):
            seen.clear()
            loss_value = float(tr.train_step([target], views=[it % 3], next_views=[(it + 1) % 3]))
            assert tr.last_plan.path == "cxx_all"
            after = state()
            freeze = tr.last_plan.freeze_shN
            assert freeze == (kind == "l1_ssim" and start + it + 1 <= 1000)

            def adam(k):
                s = seen[id(getattr(tr.model, names[k]))]
                return (s["lr"], s["beta1"], s["beta2"], s["eps"], s["bc1_rcp"], s["bc2_sqrt_rcp"])

            noise, noise_lr = (None, 0.0) if "noise" not in seen else (seen["noise"][0].cpu().numpy(), float(seen["noise"][1]))
            assert (noise is not None) == (kind == "mcmc")
            chk.check_step(oracle_mod, f"trainer {kind}", d, it, before, after, loss_value, "l1_ssim", freeze, noise, adam=adam, noise_lr=noise_lr, lam=tr.lambda_dssim,
                           scale_reg=tr.scale_reg, opacity_reg=tr.opacity_reg)
            before = after
    finally:
        lib.lfs_set_debug_flags(0)
    assert tr._gut_step.colour_launches_saved == 2
