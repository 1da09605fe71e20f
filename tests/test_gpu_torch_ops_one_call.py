"""lfs::GutTrainStep::step_opt (include/lfs_gut_train_step.hpp: the one-call training step with the reference's own loss, the MCMC noise and the shN freeze, for a
libtorch C++ caller) through the pybind module, against gut_step.GutStep.train_step with the same options: both enqueue lfs_gut_train_step_opt, so in the deterministic
accumulation mode parameters and moments agree BIT FOR BIT - including a first attempt that overflows its deliberately small workspace and is re-run with the same
noise. And step() itself is what it was: equal to step_opt with default options and to the Python driver's fused-tail step."""
import pytest
import torch

from gpu_util import noise_check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ["means", "sh0", "shN", "raw_scales", "raw_quats", "raw_opacities"]
KEYS = ("lr", "beta1", "beta2", "eps", "bc1_rcp", "bc2_sqrt_rcp")


def _mod():
    import lichtfeld_studio_amd  # noqa: F401
    from lichtfeld_studio_amd import _lfs_torch_ops as m
    return m


class _State:
    """six parameter tensors + a FusedAdam over them (the bookkeeping a trainer keeps around either driver)"""

    def __init__(self, sc):
        from lichtfeld_studio_amd.trainer import GutTrainer
        self.tr = GutTrainer(sc, DEV, iterations=7000)
        self.params = [p.detach() for p in self.tr.model.parameters()]
        self.opt = self.tr.optimizer

    def adam(self, freeze):
        return {k: self.opt.prepare_inline(getattr(self.tr.model, k)) for k in NAMES if not (freeze and k == "shN")}

    def after(self, it):
        self.opt._inline_done.clear()


def _run(m, lfs, loss, freeze, noise_on, use_cxx, steps=3, capacity=1000):
    from lichtfeld_studio_amd import scenes
    from lichtfeld_studio_amd.gut_step import GutStep
    sc = scenes.syn_a(n=5000, sh_degree=2)
    target = torch.rand(3, sc.height, sc.width, generator=torch.Generator().manual_seed(13)).to(DEV) * 0.7
    st = _State(sc)
    scn = st.tr.scene
    gen = torch.Generator(device=DEV).manual_seed(7)
    loss_t = torch.zeros(1, device=DEV)
    cxx = m.GutTrainStep(16, capacity) if use_cxx else None      # 1000 entries: the first attempt cannot fit
    py = None if use_cxx else GutStep(DEV, initial_capacity=capacity)
    vm, Km, deg = scn.viewmats[0], scn.Ks[0], 2
    losses = []
    for it in range(steps):
        noise = torch.randn(5000, 3, device=DEV, generator=gen) if noise_on else None
        ad = st.adam(freeze)
        if use_cxx:
            order = [ad.get(k) for k in NAMES]
            blank = [0.0] * 6
            n_isects = cxx.step_opt(st.params, [None if d is None else d["exp_avg"] for d in order], [None if d is None else d["exp_avg_sq"] for d in order],
                                    [blank if d is None else [d[k] for k in KEYS] for d in order], deg, vm, Km, sc.width, sc.height, st.tr.bg, target, 1.0, loss_t, 0.01, 0.01,
                                    next_viewmat=vm, loss_kind=1 if loss == "l1_ssim" else 0, lambda_dssim=0.2, freeze_shN=freeze, noise=noise, noise_lr=0.5)
        else:
            n_isects = py.train_step(st.params, ad, deg, sc.width, sc.height, vm, Km, st.tr.bg, target, 1.0, loss_t, 0.01, 0.01, fused_tail=True, next_viewmat=vm,
                                     loss=loss, lambda_dssim=0.2, freeze_shN=freeze, noise=noise, noise_lr=0.5)
        st.after(it)
        losses.append(float(loss_t))
    torch.cuda.synchronize()
    retries = cxx.retries() if use_cxx else py.retries
    saved = cxx.colour_launches_saved() if use_cxx else py.colour_launches_saved
    return st, losses, n_isects, retries, saved


@pytest.mark.parametrize("loss,freeze,noise", [("l1_ssim", False, True), ("l1_ssim", True, False), ("mse", True, True), ("mse", False, False)])
def test_step_opt_equals_the_python_driver_bit_for_bit(lfs, loss, freeze, noise):
    m = _mod()
    assert hasattr(m.GutTrainStep, "step_opt")
    lib = lfs.load_library()
    try:
        lib.lfs_set_debug_flags(16)
        a, la, na, ra, sa = _run(m, lfs, loss, freeze, noise, use_cxx=False)
        b, lb, nb, rb, sb = _run(m, lfs, loss, freeze, noise, use_cxx=True)
    finally:
        lib.lfs_set_debug_flags(0)
    assert ra >= 1 and rb >= 1 and na == nb > 0
    assert sa == sb == 2          # the second and third step found their colours prepared, in both drivers
    for x, y in zip(la, lb):
        noise_check(f"step_opt loss value {loss}", abs(x - y), 1e-5 * abs(x))
        assert x > 0
    for name, pa, pb in zip(NAMES, a.params, b.params):
        assert torch.equal(pa, pb), (name, float((pa - pb).abs().max()))
        sa_, sb_ = a.opt._state(getattr(a.tr.model, name)), b.opt._state(getattr(b.tr.model, name))
        assert torch.equal(sa_["exp_avg"], sb_["exp_avg"]) and torch.equal(sa_["exp_avg_sq"], sb_["exp_avg_sq"]), name
        if freeze and name == "shN":
            assert not sa_["exp_avg"].any() and torch.equal(pa, a.tr.scene.shN)
        else:
            assert sa_["exp_avg"].any(), name


def test_step_is_unchanged_and_equals_step_opt_with_default_options(lfs):
    m = _mod()
    from lichtfeld_studio_amd import scenes
    from lichtfeld_studio_amd.gut_step import GutStep
    sc = scenes.syn_a(n=5000, sh_degree=2)
    target = torch.rand(3, sc.height, sc.width, generator=torch.Generator().manual_seed(13)).to(DEV) * 0.7
    lib = lfs.load_library()
    outs = []
    try:
        lib.lfs_set_debug_flags(16)
        for form in ("py", "step", "step_opt"):
            st = _State(sc)
            scn = st.tr.scene
            loss_t = torch.zeros(1, device=DEV)
            drv = GutStep(DEV, initial_capacity=1000) if form == "py" else m.GutTrainStep(16, 1000)
            for it in range(3):
                ad = st.adam(False)
                lists = ([ad[k]["exp_avg"] for k in NAMES], [ad[k]["exp_avg_sq"] for k in NAMES], [[ad[k][j] for j in KEYS] for k in NAMES])
                if form == "py":
                    drv.train_step(st.params, ad, 2, sc.width, sc.height, scn.viewmats[0], scn.Ks[0], st.tr.bg, target, 1.0, loss_t, 0.0, 0.0, fused_tail=True)
                elif form == "step":
                    drv.step(st.params, *lists, 2, scn.viewmats[0], scn.Ks[0], sc.width, sc.height, st.tr.bg, target, 1.0, loss_t, 0.0, 0.0)
                else:
                    drv.step_opt(st.params, *lists, 2, scn.viewmats[0], scn.Ks[0], sc.width, sc.height, st.tr.bg, target, 1.0, loss_t)
                st.after(it)
            torch.cuda.synchronize()
            outs.append((st, float(loss_t)))
    finally:
        lib.lfs_set_debug_flags(0)
    ref = outs[0]
    for st, l in outs[1:]:
        noise_check("GutTrainStep loss value", abs(l - ref[1]), 1e-5 * ref[1])
        for name, pa, pb in zip(NAMES, ref[0].params, st.params):
            assert torch.equal(pa, pb), name
            sa_, sb_ = ref[0].opt._state(getattr(ref[0].tr.model, name)), st.opt._state(getattr(st.tr.model, name))
            assert torch.equal(sa_["exp_avg"], sb_["exp_avg"]) and torch.equal(sa_["exp_avg_sq"], sb_["exp_avg_sq"]), name
