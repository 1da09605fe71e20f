"""CPU: ADC on the 3DGUT route needs a step form with a gradient-tensor finish pass - that pass computes densification_info. trainer.plan_step keeps
strategy="default" out of every form without one (the one-call step and the inline-Adam forms) for every combination of its other inputs; GutTrainer relies on it."""
import itertools


def test_plan_step_keeps_adc_out_of_every_form_without_a_finish_pass():
    import lichtfeld_studio_amd  # noqa: F401
    from lichtfeld_studio_amd.trainer import plan_step
    seen = set()
    for (loss, n_views, world, force, iteration, refining, has_shN, fused_opt, bilateral, cxx_step, batch_views, factored_sh, one_call, masked, inline_shN, inline_all) in \
            itertools.product(("mse", "l1_ssim"), (1, 2), (1, 2), (False, True), (500, 1000, 1001, 3000), (False, True), (False, True), (False, True), (False, True),
                              (False, True), (False, True), (False, True), (False, True), (False, True), (False, True), (False, True)):
        kw = dict(rasterizer="gut", fused_l2=True, world=world, force_collectives=force, sh_sharded=False, shard_rows=0, n_views=n_views, loss=loss, strategy="default",
                  refining=refining, iteration=iteration, has_shN=has_shN, optimizer_fused=fused_opt, bilateral=bilateral, inline_shN_adam=inline_shN,
                  inline_all_adam=inline_all, cxx_step=cxx_step, batch_views=batch_views, factored_sh=factored_sh, one_call=one_call, masked=masked)
        if factored_sh and (world > 1 or force) and not cxx_step:
            continue                                       # (plan_step raises: GutTrainer rejects that configuration up front)
        plan = plan_step(**kw)
        seen.add(plan.path)
        assert plan.path in ("cxx_views", "cxx_factored", "batch_views", "py_views"), (kw, plan)
        assert not plan.inline_all and not plan.inline_shN and not plan.inline_shard, (kw, plan)   # ("inline_all", "inline_shN", "inline_shard": no gradient tensor)
    assert seen == {"cxx_views", "cxx_factored", "batch_views", "py_views"}


def test_plan_step_for_adc_is_the_plan_without_the_inline_switches():
    """the rows the trainer test relies on: one view on one rank -> cxx_views (cxx_step) or py_views; two views -> batch_views or py_views; forced collectives with
    the factored exchange -> cxx_factored"""
    import lichtfeld_studio_amd  # noqa: F401
    from lichtfeld_studio_amd.trainer import plan_step
    base = dict(rasterizer="gut", fused_l2=True, world=1, force_collectives=False, sh_sharded=False, shard_rows=0, n_views=1, loss="l1_ssim", strategy="default",
                refining=False, iteration=3000, has_shN=True, optimizer_fused=True, bilateral=False)
    assert plan_step(**base).path == "cxx_views"
    assert plan_step(**dict(base, cxx_step=False)).path == "py_views"
    assert plan_step(**dict(base, n_views=2)).path == "batch_views"
    assert plan_step(**dict(base, n_views=2, batch_views=False)).path == "py_views"
    assert plan_step(**dict(base, force_collectives=True, factored_sh=True)).path == "cxx_factored"
    assert plan_step(**dict(base, one_call=True)).path == "cxx_views"
    assert plan_step(**dict(base, rasterizer="fastgs")).path == "fastgs" and plan_step(**dict(base, fused_l2=False)).path == "autograd"
