"""trainer.plan_step with one_call=True (GutTrainer(one_call=True)): over the same product of inputs as tests/test_host_logic.py's table, the one-call form is chosen
exactly under the documented conditions, and with the keyword off every row is what it is without the keyword."""
import itertools


def _rows():
    for (world, force, sharded, n_views, loss, strategy, refining, iteration, has_shN, fused, bilateral, i_shN, i_all, cxx, batch) in itertools.product(
            (1, 2, 8), (False, True), (False, True), (1, 8), ("mse", "l1_ssim"), (None, "mcmc", "default"), (False, True), (500, 1000, 1001, 7000), (False, True),
            (False, True), (False, True), (False, True), (False, True), (False, True), (False, True)):
        if refining and strategy is None:
            continue
        yield dict(rasterizer="gut", fused_l2=True, world=world, force_collectives=force, sh_sharded=sharded, shard_rows=1000 if sharded else 0, n_views=n_views,
                   loss=loss, strategy=strategy, refining=refining, iteration=iteration, has_shN=has_shN, optimizer_fused=fused, bilateral=bilateral,
                   inline_shN_adam=i_shN, inline_all_adam=i_all, cxx_step=cxx, batch_views=batch)


def test_one_call_rows_of_the_step_plan_table():
    import lichtfeld_studio_amd  # noqa: F401
    from lichtfeld_studio_amd.trainer import plan_step
    n = chosen = 0
    for kw in _rows():
        off = plan_step(**kw)
        assert plan_step(**kw, one_call=False) == off and not off.freeze_shN
        on = plan_step(**kw, one_call=True)
        n += 1
        want = (kw["world"] == 1 and not kw["force_collectives"] and not kw["sh_sharded"] and kw["n_views"] == 1 and kw["optimizer_fused"] and kw["has_shN"]
                and kw["cxx_step"] and not kw["bilateral"] and kw["loss"] in ("mse", "l1_ssim")
                and (kw["strategy"] is None or (kw["strategy"] == "mcmc" and not kw["refining"])))
        if want:
            chosen += 1
            assert on.path == "cxx_all" and on.inline_all and not on.multi and not on.inline_shard
            assert on.freeze_shN == (kw["iteration"] <= 1000) and on.inline_shN == (kw["iteration"] > 1000)
            assert on.skip_deferred == off.skip_deferred
        else:
            assert on == off, kw        # everything else keeps its form
        if kw["refining"] or kw["bilateral"] or kw["n_views"] > 1 or kw["world"] > 1 or kw["force_collectives"] or kw["strategy"] == "default":
            assert on == off and not on.freeze_shN
            if on.path == "cxx_all":    # (only the parent's own MSE row can still be the one-call form here - never a refining / bilateral / several-view / multi-rank step)
                assert not (kw["refining"] or kw["bilateral"] or kw["n_views"] > 1 or kw["world"] > 1 or kw["force_collectives"] or kw["strategy"] is not None)
    assert n > 20000 and chosen == 2 * 2 * 4 * 2 * 2 * 2   # loss x (no strategy | MCMC between refinements) x iteration x the three A/B switches that do not matter


def test_one_call_documented_rows():
    import lichtfeld_studio_amd  # noqa: F401
    from lichtfeld_studio_amd.trainer import plan_step
    base = dict(rasterizer="gut", fused_l2=True, world=1, force_collectives=False, sh_sharded=False, shard_rows=0, n_views=1, loss="l1_ssim", strategy="mcmc", refining=False,
                iteration=3000, has_shN=True, optimizer_fused=True, bilateral=False)
    assert plan_step(**base).path == "cxx_views"                                            # the reference's configuration today
    p = plan_step(**base, one_call=True)
    assert p.path == "cxx_all" and p.inline_all and not p.freeze_shN                        # ... as one call
    assert plan_step(**dict(base, refining=True), one_call=True) == plan_step(**dict(base, refining=True))       # relocation / growth: the split form
    assert plan_step(**dict(base, iteration=500), one_call=True).freeze_shN                 # shN frozen for the first 1000 iterations
    assert plan_step(**dict(base, iteration=1000), one_call=True).freeze_shN and not plan_step(**dict(base, iteration=1001), one_call=True).freeze_shN
    assert plan_step(**dict(base, strategy="default"), one_call=True).path != "cxx_all"     # ADC stays on the split forms
    assert plan_step(**dict(base, bilateral=True), one_call=True).path == "cxx_views"
    assert plan_step(**dict(base, n_views=8), one_call=True).path == "batch_views"
    assert plan_step(**dict(base, world=8), one_call=True).path == "cxx_views"
    for other in ("fastgs",):
        assert plan_step(**dict(base, rasterizer=other), one_call=True).path == "fastgs"
    assert plan_step(**dict(base, fused_l2=False), one_call=True).path == "autograd"
    assert plan_step(**dict(base, cxx_step=False), one_call=True).path == "py_views"
