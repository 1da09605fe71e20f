"""GPU: the sparsification phase of GutTrainer (enable_sparsity; trainer.cpp:331-360, :707-714, :745-754, :776-784) on a SYN-A-style scene of 2000 Gaussians,
64 x 64, 4 views: 20 base iterations, 20 sparsification iterations with a state update every 5, then the prune to half. Both rasterizers, with and without the
MCMC strategy, next to a twin trainer without the phase; both backwards run in their deterministic accumulation mode (debug bit 4: integer atomics in two passes,
raster.hip and fastgs_blend.hip), without which two trainers built alike differ in the last bits of every gradient."""
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ["means", "sh0", "shN", "raw_scales", "raw_quats", "raw_opacities"]
BASE, STEPS, EVERY, RATIO, N0 = 20, 20, 5, 0.5, 2000
SH_INTERVAL = 15      # the SH schedule would raise the degree at iterations 15 and 30: the second one lies in the phase and must not happen


def _scene():
    from lichtfeld_studio_amd import scenes
    sc = scenes.syn_a(n=N0, sh_degree=2)
    viewmats = torch.eye(4).repeat(4, 1, 1)
    viewmats[:, 0, 3] = torch.tensor([0.0, 0.3, -0.3, 0.15])
    viewmats[:, 1, 3] = torch.tensor([0.0, -0.2, 0.2, 0.1])
    Ks = torch.tensor([[50.0, 0, 32], [0, 50.0, 32], [0, 0, 1]]).repeat(4, 1, 1)
    return dataclasses.replace(sc, width=64, height=64, viewmats=viewmats, Ks=Ks, extra={"active_sh_degree": 0})


def _targets(sc):
    g = torch.Generator().manual_seed(11)
    return [(torch.rand(3, sc.height, sc.width, generator=g) * 0.7).to(DEV) for _ in range(4)]


def _trainer(rasterizer, strategy, **kw):
    from lichtfeld_studio_amd import strategies
    from lichtfeld_studio_amd.trainer import GutTrainer
    op = None
    if strategy is not None:
        op = strategies.OptimizationParameters.for_strategy(strategy, iterations=BASE, sh_degree_interval=SH_INTERVAL)
    tr = GutTrainer(_scene(), torch.device(DEV), iterations=BASE, rasterizer=rasterizer, strategy=strategy, opt_params=op, **kw)
    tr.sh_degree_interval = SH_INTERVAL
    return tr


def _step(tr, targets):
    v = (tr.iteration) % 4
    return tr.train_step([targets[v]], views=[v])


def _state(tr):
    out = {}
    for name, p in zip(NAMES, tr.model.parameters()):
        st = tr.optimizer.state.get(id(p))
        out[name] = (p.detach().clone(), None if st is None else st["exp_avg"].clone(), None if st is None else st["exp_avg_sq"].clone())
    return out


SPARSE = dict(enable_sparsity=True, sparsify_steps=STEPS, sparsity_update_every=EVERY, prune_ratio=RATIO, init_rho=0.0005)


@pytest.mark.parametrize("strategy", [None, "mcmc"])
@pytest.mark.parametrize("rasterizer", ["gut", "fastgs"])
def test_base_phase_sparsification_and_prune(lfs, rasterizer, strategy):
    from lichtfeld_studio_amd import sparsity
    lib = lfs.load_library()
    targets = _targets(_scene())
    try:
        lib.lfs_set_debug_flags(16)
        on = _trainer(rasterizer, strategy, **SPARSE)
        assert on.total_iterations == BASE + STEPS and on.sparsity is not None
        sp = on.sparsity
        captured, terms = {}, []
        real_mask, real_add = sp.get_prune_mask, sp.add_loss_and_grad

        def recording_mask(raw):
            captured["state"] = _state(on)
            captured["mask"] = real_mask(raw)
            return captured["mask"]

        def recording_add(raw, grad_view, loss_acc, scale=1.0):
            before, loss_before = grad_view.detach().clone(), loss_acc.detach().clone()
            real_add(raw, grad_view, loss_acc, scale)
            terms.append((on.iteration, raw.detach().clone(), before, grad_view.detach().clone(), float(loss_acc) - float(loss_before), scale))
        sp.get_prune_mask, sp.add_loss_and_grad = recording_mask, recording_add

        updates, counts, degrees = [], {}, {}
        for it in range(1, BASE + STEPS + 1):
            u_before = None if sp.u is None else sp.u.clone()
            _step(on, targets)
            assert on.iteration == it
            if it < BASE:
                assert sp.u is None and not sp.is_initialized() and not terms
            elif it == BASE:
                assert sp.is_initialized() and not bool(sp.u.any())       # initialised lazily, on first use: u = 0
            if u_before is not None and sp.u is not None and not torch.equal(u_before, sp.u):
                updates.append(it)
            counts[it], degrees[it] = on.model.means.shape[0], on.model.active_sh_degree
            if BASE <= it < BASE + STEPS:
                assert on.last_plan.path != "cxx_all" and not on.last_plan.inline_all
                # the opacity gradient of this step carries the operator's own output, once, and the loss its value
                assert len(terms) == it - BASE + 1 and terms[-1][0] == it
                _, raw, g_before, g_after, loss_delta, scale = terms[-1]
                assert scale == 1.0
                if it == BASE or it == BASE + 7:
                    term, tl = torch.zeros(N0, device=DEV), torch.zeros(1, device=DEV)
                    sparsity.admm_loss_grad(raw, sp.z, sp.u, 0.0005, 1.0, term, False, tl)       # (no update between the term and here on these iterations)
                    assert bool((term != 0).any())
                    big = torch.maximum(g_before.reshape(-1).abs(), term.abs())
                    ulp = torch.nextafter(big, torch.full_like(big, float("inf"))) - big
                    err = (g_after.reshape(-1).double() - (g_before.reshape(-1).double() + term.double())).abs()
                    assert bool((err <= ulp.double()).all())
                    assert loss_delta == pytest.approx(float(tl), rel=1e-3, abs=1e-7) and float(tl) > 0
        torch.cuda.synchronize()
    finally:
        lib.lfs_set_debug_flags(0)

    assert len(terms) == STEPS
    assert updates == [BASE + 5, BASE + 10, BASE + 15], updates
    assert all(counts[it] == N0 for it in range(1, BASE + STEPS)) and counts[BASE + STEPS] == N0 - int(np.float32(RATIO) * np.float32(N0)) == 1000
    assert degrees[SH_INTERVAL - 1] == 0 and degrees[SH_INTERVAL] == 1                            # the schedule ran in the base phase ...
    assert all(degrees[it] == degrees[BASE + 1] == 1 for it in range(BASE + 1, BASE + STEPS + 1))  # ... and stopped: iteration 30 would have raised it
    assert on.sparsity is None                                                                     # dropped after the prune

    # the prune: the 1000 largest raw opacities of the model as it stood after the last optimizer step, all six tensors and both Adam moments cut alike
    before, mask = captured["state"], captured["mask"]
    raw = before["raw_opacities"][0].reshape(-1)
    assert mask.dtype == torch.bool and int(mask.sum()) == 1000
    order = torch.sort(raw, stable=True)[1]
    want = torch.zeros(N0, dtype=torch.bool, device=DEV)
    want[order[:1000]] = True
    assert torch.equal(mask, want)
    assert float(raw[mask].max()) <= float(raw[~mask].min())
    keep = (~mask).nonzero().squeeze(-1)
    after = _state(on)
    for name in NAMES:
        for k, (a, b) in enumerate(zip(after[name], before[name])):
            assert (a is None) == (b is None), (name, k)
            if a is not None:
                assert a.shape[0] == 1000 and torch.equal(a, b.index_select(0, keep)), (name, k)
    assert on.bucket.views[0].shape[0] == 1000
    # and the pruned model trains on
    loss = _step(on, targets)
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and on.model.means.shape[0] == 1000


def _max_param_difference(a, b):
    return max(float((pa.detach() - pb.detach()).abs().max()) for pa, pb in zip(a.model.parameters(), b.model.parameters()))


@pytest.mark.parametrize("strategy", [None, "mcmc"])
@pytest.mark.parametrize("rasterizer", ["gut", "fastgs"])
def test_a_twin_without_sparsity_is_the_same_trainer_up_to_the_phase(lfs, rasterizer, strategy):
    """Bit-identical through iteration 19; at iteration 20 the opacity gradients differ by the operator's own output, within 1 ulp of the larger addend; after
    iteration 21 the raw opacities differ, because the optimizer does step in the phase."""
    from lichtfeld_studio_amd import sparsity
    lib = lfs.load_library()
    targets = _targets(_scene())
    try:
        lib.lfs_set_debug_flags(16)
        on, off = _trainer(rasterizer, strategy, **SPARSE), _trainer(rasterizer, strategy)
        sp = on.sparsity
        first_difference, worst = None, 0.0
        for it in range(1, BASE):
            _step(on, targets), _step(off, targets)
            d = _max_param_difference(on, off)
            worst = max(worst, d)
            if d > 0 and first_difference is None:
                first_difference = it
        print(f"{rasterizer} {strategy}: twins through iteration {BASE - 1}: first difference at iteration {first_difference}, max |difference| {worst:.3e}")
        assert first_difference is None
        for name, a, b in zip(NAMES, on.model.parameters(), off.model.parameters()):
            assert torch.equal(a, b), name
        raw_before = on.model.raw_opacities.detach().clone()
        _step(on, targets), _step(off, targets)                      # iteration 20: the first of the phase
        term = torch.zeros(N0, device=DEV)
        sparsity.admm_loss_grad(raw_before, sp.z, sp.u, 0.0005, 1.0, term, False, None)
        g_on, g_off = on.bucket.views[5].reshape(-1).double(), off.bucket.views[5].reshape(-1).double()
        assert bool((term != 0).any())
        big = torch.maximum(g_off.abs(), term.double().abs()).float()
        ulp = torch.nextafter(big, torch.full_like(big, float("inf"))) - big
        err = (g_on - (g_off + term.double())).abs()
        print(f"{rasterizer} {strategy}: max |g_on - (g_off + term)| / ulp {float((err / ulp.double()).max()):.3f}")
        assert bool((err <= ulp.double()).all())
        if strategy is None:    # (a twin with a strategy does not step its optimizer at ITS last iteration, this one)
            for name, a, b in zip(NAMES, on.model.parameters(), off.model.parameters()):
                assert torch.equal(a, b) == (name != "raw_opacities"), name    # the term touches the opacities and nothing else
        _step(on, targets), _step(off, targets)
        _step(on, targets), _step(off, targets)
        torch.cuda.synchronize()
    finally:
        lib.lfs_set_debug_flags(0)
    assert not torch.equal(on.model.raw_opacities, off.model.raw_opacities)


@pytest.mark.parametrize("rasterizer", ["gut", "fastgs"])
def test_the_new_arguments_without_the_switch_change_nothing(lfs, rasterizer):
    """That the switched-off arguments allocate nothing and leave every plan unchanged is held on the CPU by tests/test_sparsity_host.py; here the bits."""
    lib = lfs.load_library()
    targets = _targets(_scene())
    try:
        lib.lfs_set_debug_flags(16)
        a = _trainer(rasterizer, None)
        b = _trainer(rasterizer, None, enable_sparsity=False, sparsify_steps=7, init_rho=0.3, prune_ratio=0.9, sparsity_update_every=2)
        assert b.sparsity is None
        for _ in range(BASE + 4):
            _step(a, targets), _step(b, targets)
            assert a.last_plan == b.last_plan
        torch.cuda.synchronize()
    finally:
        lib.lfs_set_debug_flags(0)
    print(f"{rasterizer}: with and without the arguments after {BASE + 4} iterations: max |difference| {_max_param_difference(a, b):.3e}")
    for name, pa, pb in zip(NAMES, a.model.parameters(), b.model.parameters()):
        assert torch.equal(pa, pb), name
        sa, sb = a.optimizer.state[id(pa)], b.optimizer.state[id(pb)]
        assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]), name
    assert a.model.means.shape[0] == N0 and a.model.active_sh_degree == b.model.active_sh_degree


def test_train_colmap_tool_carries_a_run_through_the_phase_and_saves_the_pruned_model(lfs, tmp_path):
    """tools/train_colmap.py --enable-sparsity: base run, sparsification, prune; the model of the base run is saved at --iterations, the pruned one at the end."""
    import json
    import os
    import subprocess
    import sys

    from lichtfeld_studio_amd import loader
    from test_gpu_dataprep import _synthetic_colmap
    base, _, xyz, _ = _synthetic_colmap(str(tmp_path), n_views=8, n_pts=6002)      # every second point goes into the cloud: N = 3001
    out = str(tmp_path / "run")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "train_colmap.py"), "-d", base, "-i", "40", "--strategy", "mcmc", "--sh-degree", "1", "-o", out,
                        "--enable-sparsity", "--sparsify-steps", "30", "--init-rho", "0.001", "--prune-ratio", "0.6"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    N = len(xyz)
    left = N - int(np.float32(0.6) * np.float32(N))
    assert res["iterations"] == 70 and res["base_iterations"] == 40 and res["gaussians"] == left == 1201
    assert res["ply"].endswith("splat_70.ply") and os.path.exists(os.path.join(out, "splat_40.ply"))
    assert loader.load_ply(res["ply"], DEV).means.shape[0] == left
    assert loader.load_ply(os.path.join(out, "splat_40.ply"), DEV).means.shape[0] == N
