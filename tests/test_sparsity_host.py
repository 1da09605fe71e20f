"""CPU: the host side of the ADMM sparsity optimiser (lichtfeld_studio_amd/sparsity.py, trainer.py) - the schedule predicates against the header's inequalities
(sparsity_optimizer.hpp:102-117), the float32 prune count, and the step forms the trainer plans during the sparsification phase. No kernel is launched."""
import dataclasses

import numpy as np
import pytest
import torch

import sparsity_reference as ref


@pytest.mark.parametrize("base,steps,every", [(20, 20, 5), (30000, 15000, 50), (7, 3, 1), (10, 10, 50)])
def test_schedule_predicates_are_the_headers_inequalities(lfs, base, steps, every):
    from lichtfeld_studio_amd.sparsity import ADMMSparsityOptimizer, Config
    sp = ADMMSparsityOptimizer(Config(sparsify_steps=steps, update_every=every, start_iteration=base))
    assert not sp.is_initialized()
    its = range(base - 2, base + steps + 3) if steps < 1000 else list(range(base - 2, base + 3)) + list(range(base + steps - 120, base + steps + 3))
    for it in its:
        assert sp.should_update(it) == ref.should_update(it, base, steps, every), it
        assert sp.should_apply_loss(it) == ref.should_apply_loss(it, base, steps), it
        assert sp.should_prune(it) == ref.should_prune(it, base, steps), it
    # spelled out once: the loss from the first iteration of the phase, the first update one period later, none at the end, the prune after the last loss
    assert sp.should_apply_loss(base) and not sp.should_update(base) and not sp.should_apply_loss(base - 1)
    assert not sp.should_apply_loss(base + steps) and not sp.should_update(base + steps) and sp.should_prune(base + steps)
    assert not sp.should_prune(base + steps - 1) and not sp.should_prune(base + steps + 1)


def test_config_defaults_are_the_references(lfs):
    from lichtfeld_studio_amd.sparsity import ADMMSparsityOptimizer, Config
    assert dataclasses.asdict(Config()) == dict(sparsify_steps=15000, init_rho=0.0005, prune_ratio=0.6, update_every=50, start_iteration=30000)
    assert ADMMSparsityOptimizer().config == Config() and ADMMSparsityOptimizer.Config is Config


def test_num_to_prune_is_the_truncated_float32_product(lfs):
    from lichtfeld_studio_amd.sparsity import ADMMSparsityOptimizer, Config, num_to_prune
    for ratio in (0.6, 0.25, 0.5, 0.9, 0.1):
        sp = ADMMSparsityOptimizer(Config(prune_ratio=ratio))
        differing = None
        for n in list(range(1, 3000)) + [10 ** 6, 10 ** 6 + 5, 3_000_000] + list(range(7_000_000, 7_000_020)):
            want = int(np.float32(ratio) * np.float32(n))
            assert want == ref.num_to_prune_f32(ratio, n)
            assert num_to_prune(ratio, n) == want
            assert sp.get_num_to_prune(torch.empty(n, device="meta")) == want
            if differing is None and want != int(ratio * n):
                differing = n
        if ratio == 0.6:
            # the default ratio: 0.6 n has the fraction .2 .4 .6 .8 or none; once the product passes 2^22 a float holds halves only and .6 / .8 round UP to the
            # next integer, which the truncated double product never reaches (7 000 001 -> 4 200 001 against 4 200 000)
            assert differing is not None and differing >= 7_000_000
            assert num_to_prune(ratio, differing) == int(ratio * differing) + 1 == ref.num_to_prune_f64(ratio, differing) + 1
    assert ADMMSparsityOptimizer().get_num_to_prune(None) == 0 and ADMMSparsityOptimizer().get_num_to_prune(torch.empty(0)) == 0


def test_the_plan_keeps_an_opacity_gradient_tensor_during_the_phase_and_is_unchanged_outside_it(lfs):
    """one view, one rank, MSE, no strategy, iteration > 1000: the all-inline one-call step everywhere - except where the ADMM term applies"""
    from lichtfeld_studio_amd import scenes
    from lichtfeld_studio_amd.trainer import GutTrainer
    sc = scenes.syn_a(n=64, sh_degree=1)
    base, steps = 1005, 6
    for one_call in (False, True):
        on = GutTrainer(sc, torch.device("cpu"), iterations=base, one_call=one_call, enable_sparsity=True, sparsify_steps=steps, sparsity_update_every=2)
        off = GutTrainer(sc, torch.device("cpu"), iterations=base, one_call=one_call)
        assert on.total_iterations == base + steps and off.total_iterations == base and off.sparsity is None
        for it in range(base - 3, base + steps + 3):
            on.iteration = off.iteration = it
            p_on, p_off = on._plan(1), off._plan(1)
            assert p_off.path == "cxx_all" and p_off.inline_all
            if base <= it < base + steps:
                assert not p_on.inline_all and p_on.path != "cxx_all", it
                assert p_on.path in ("cxx_views", "batch_views", "py_views")
            else:
                assert p_on == p_off, it
    # the other rasterizer and the autograd form carry the gradient tensor anyway: the same plan with and without the phase
    for kw in (dict(rasterizer="fastgs"), dict(fused_l2=False)):
        on = GutTrainer(sc, torch.device("cpu"), iterations=base, enable_sparsity=True, sparsify_steps=steps, **kw)
        off = GutTrainer(sc, torch.device("cpu"), iterations=base, **kw)
        for it in range(base - 1, base + steps + 1):
            on.iteration = off.iteration = it
            assert on._plan(1) == off._plan(1) and on._plan(1).path in ("fastgs", "autograd")


def test_a_trainer_without_the_switch_allocates_nothing_and_the_strategy_limit_follows_the_total(lfs):
    from lichtfeld_studio_amd import scenes
    from lichtfeld_studio_amd.trainer import GutTrainer
    sc = scenes.syn_a(n=64, sh_degree=1)
    off = GutTrainer(sc, torch.device("cpu"), iterations=30, sparsify_steps=10, init_rho=0.1, prune_ratio=0.5, sparsity_update_every=5)
    assert off.sparsity is None and off.total_iterations == 30
    on = GutTrainer(sc, torch.device("cpu"), iterations=30, strategy="mcmc", enable_sparsity=True, sparsify_steps=10, init_rho=0.1, prune_ratio=0.5,
                    sparsity_update_every=5)
    assert on.sparsity.u is None and on.sparsity.z is None and not on.sparsity.is_initialized()          # lazily, on first use
    assert on.sparsity.config.start_iteration == 30 and on.sparsity.config.update_every == 5
    assert on.strategy.params.iterations == 30 and on.strategy.step_limit == 40                          # the optimizer steps through the phase
    assert on.scheduler.gamma == pytest.approx(0.01 ** (1.0 / 30))                                       # the schedule stays the base run's
    plain = GutTrainer(sc, torch.device("cpu"), iterations=30, strategy="mcmc")
    assert plain.strategy.step_limit == 30
