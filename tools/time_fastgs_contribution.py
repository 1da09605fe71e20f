#!/usr/bin/env python3
"""What the contribution statistic of the fastgs (EWA) rasterizer costs (lfs_fastgs_view_contribution), on SYN-B (1 M Gaussians, 1920 x 1080, SH degree 3).
One process; after a warm-up of every form, `--rounds` rounds alternate between the forms. Per form, the median over the rounds and the round-to-round spread (max - min) of

  (i)   step_ms        one GutTrainer(rasterizer="fastgs") train_step of the DEFAULT configuration, between device events - with this checkout's library and, with
                       --parent-lib PATH, with the parent commit's liblfs_gsplat.so loaded into the same process (each library drives a trainer of its own; the two
                       alternate round by round). Acceptance: this library's median is not above the parent's by more than the parent's own spread.
  (ii)  pass_us        on one fixed view: the blend forward ("fastgs_blend_fwd" scope of lfs_fastgs_view_render), the blend backward ("fastgs_blend_bwd" of
                       lfs_fastgs_view_backward) and the contribution pass ("fastgs_contribution"), from the library's event profiler; with the number of (pixel,
                       Gaussian) pairs the contribution pass reduces
  (iii) with --colmap DIR (a stand-in scene of tools/make_synthetic_colmap.py): 100 training steps with GutTrainer(contribution_prune_at=(50,)), each timed on its own -
                       the prune is iteration 50's time above the median step, and its share of the 100 steps; then N and the training-view PSNR before and after a
                       prune of the trained model at thresholds 0.01 and 0.05 (reported: no claim about image quality is made from a stand-in scene)

(ii) and (iii) are reported, not gated.

    python tools/time_fastgs_contribution.py [--out profiles/r18/fastgs_contribution.json] [--parent-lib /path/to/parent/liblfs_gsplat.so] [--colmap DIR] [--rounds 7] [--calls 20]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18", "fastgs_contribution.json"))
    ap.add_argument("--parent-lib", default=None, help="liblfs_gsplat.so built from the parent commit: its default step alternates with this checkout's")
    ap.add_argument("--colmap", default=None, help="a COLMAP directory (tools/make_synthetic_colmap.py): the whole-prune timing and the N / PSNR table")
    ap.add_argument("--images", default="images")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--n", type=int, default=1_000_000)
    args = ap.parse_args()
    import torch

    import lichtfeld_studio_amd as lfs
    from lichtfeld_studio_amd import capi, contribution, fastgs, ops, scenes
    from lichtfeld_studio_amd.trainer import GutTrainer
    if not torch.cuda.is_available():
        raise SystemExit("time_fastgs_contribution.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    libs = {"this": lfs.load_library()}
    if args.parent_lib:   # a second library in the same process: capi hands out whichever one is current (capi._LIB), every call of the package asks it
        saved, exports = os.environ.get("LFS_GSPLAT_LIB"), list(capi.EXPORTS)
        os.environ["LFS_GSPLAT_LIB"], capi._LIB = os.path.abspath(args.parent_lib), None
        capi.EXPORTS[:] = [e for e in exports if e != "lfs_fastgs_view_contribution"]   # (the parent does not have the entry this tool is about)
        try:
            libs["parent"] = capi.load_library()
        finally:
            capi.EXPORTS[:] = exports
            capi._LIB = libs["this"]
            if saved is None:
                del os.environ["LFS_GSPLAT_LIB"]
            else:
                os.environ["LFS_GSPLAT_LIB"] = saved
        assert libs["parent"] is not libs["this"]

    def use(name):
        capi._LIB = libs[name]

    sc = scenes.syn_b(n=args.n, n_views=4).to(dev)
    target = scenes.target_image(sc.height, sc.width).to(dev)
    trainers = {}
    for name in libs:
        use(name)
        trainers[name] = GutTrainer(sc, dev, iterations=30000, rasterizer="fastgs")
    use("this")

    # (ii): one forward on fixed inputs; render, backward and contribution calls on its workspaces
    tr0 = trainers["this"]
    st = tr0._fastgs_settings(0)
    means, sh0, shN, raw_scales, raw_quats, raw_opac = [p.detach().clone().contiguous() for p in tr0.model.parameters()]   # (copies: the trainers go on updating theirs)
    w2c = sc.viewmats[0].contiguous()
    N = means.shape[0]
    image, alpha, pws, iws, n_inst = fastgs.forward_wrapper(means, raw_scales, raw_quats, raw_opac, sh0, shN, w2c, st)
    gi, ga = torch.randn_like(image), torch.zeros_like(alpha)
    grads = fastgs.backward_wrapper(None, gi, ga, image, alpha, means, raw_scales, raw_quats, sh0, shN, pws, iws, w2c, st, n_inst)
    stats_buf = contribution.new_stats_buffer(N, dev)

    def render():   # (the whole forward on workspaces of its own: a render is not repeatable on a workspace - the scatter consumes the preprocess's cursors; the scope is the blend)
        fastgs.forward_wrapper(means, raw_scales, raw_quats, raw_opac, sh0, shN, w2c, st)

    def backward():
        fastgs.backward_wrapper(None, gi, ga, image, alpha, means, raw_scales, raw_quats, sh0, shN, pws, iws, w2c, st, n_inst, out=grads)

    def contrib():
        ops.fastgs_view_contribution(pws, iws, n_inst, N, st.width, st.height, stats_buf)

    passes = {"fastgs_blend_fwd": render, "fastgs_blend_bwd": backward, "fastgs_contribution": contrib}

    def window(fn, calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / calls   # ms per call

    def scope_us(scope, calls):
        capi.profile_enable(True)
        try:
            capi.profile_collect()
            for _ in range(calls):
                passes[scope]()
            torch.cuda.synchronize()
            got = capi.profile_collect()
        finally:
            capi.profile_enable(False)
        return 1e3 * got[scope][0] / got[scope][1]

    def step(name):
        use(name)
        try:
            tr = trainers[name]
            tr.train_step([target], views=[tr.iteration % 4])
        finally:
            use("this")

    for name in libs:
        window(lambda: step(name), args.warmup)
    for scope in passes:
        scope_us(scope, args.warmup)
    step_ms = {name: [] for name in libs}
    pass_us = {scope: [] for scope in passes}
    for _ in range(args.rounds):
        for name in libs:
            step_ms[name].append(window(lambda: step(name), args.calls))
        for scope in passes:
            pass_us[scope].append(scope_us(scope, args.calls))

    def stats(v):
        return {"rounds": [round(x, 3) for x in v], "median": round(statistics.median(v), 3), "spread": round(max(v) - min(v), 3)}
    # the size of the pass's work: the (pixel, Gaussian) pairs it reduces and the Gaussians whose rows it updates
    stats_buf.zero_()
    contrib()
    torch.cuda.synchronize()
    _, n_pix, _ = contribution.unpack_stats(stats_buf)
    out = {"scene": "SYN-B", "gaussians": N, "size": [sc.width, sc.height], "sh_degree": 3, "rounds": args.rounds, "calls_per_round": args.calls, "warmup_calls": args.warmup,
           "libraries": {name: lib.lfs_version().decode() for name, lib in libs.items()}, "device": torch.cuda.get_device_name(0), "n_instances": n_inst,
           "blended_pixel_pairs": int(n_pix.sum()), "gaussians_blended": int((n_pix > 0).sum()),
           "default_step_ms": {name: stats(v) for name, v in step_ms.items()}, "pass_us": {scope: stats(v) for scope, v in pass_us.items()}}
    c, b, f = (out["pass_us"][k]["median"] for k in ("fastgs_contribution", "fastgs_blend_bwd", "fastgs_blend_fwd"))
    out["contribution_over_blend_bwd"] = round(c / b, 3)
    out["contribution_over_blend_fwd"] = round(c / f, 3)
    if "parent" in libs:
        t, p = out["default_step_ms"]["this"], out["default_step_ms"]["parent"]
        out["default_step_minus_parent_ms"] = round(t["median"] - p["median"], 3)
        out["default_step_within_parent_spread"] = bool(t["median"] - p["median"] <= p["spread"])
    try:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import kernel_resources
        out["kernel_resources"] = {k: v for k, v in sorted(kernel_resources.kernels(capi.library_path()).items()) if "fg_contrib" in k or "fg_blend_fwd" in k}
    except Exception as e:   # the static table is a convenience here: tests/test_kernel_resources_fastgs_contribution.py is the check
        out["kernel_resources_error"] = repr(e)

    if args.colmap:
        from lichtfeld_studio_amd import evaluate, loader
        from lichtfeld_studio_amd.rasterizer import SplatModel
        del trainers, tr0
        torch.cuda.empty_cache()
        scene, ds, scene_scale = loader.colmap_scene(args.colmap, args.images, split="all", device=dev)
        targets = loader.preload(ds, dev)
        tr = GutTrainer(scene, dev, iterations=100, loss="l1_ssim", rasterizer="fastgs", scene_scale=scene_scale, contribution_prune_at=(50,), contribution_threshold=0.01)
        times = []
        for it in range(100):
            v = it % len(ds)
            torch.cuda.synchronize(); t0 = time.time()
            tr.train_step([targets[v]], views=[v])
            torch.cuda.synchronize(); times.append(time.time() - t0)
        med = statistics.median(times)
        prune_s = times[49] - med
        cams = [tr.camera(v) for v in range(len(ds))]
        table = []
        st_all = contribution.compute_contribution(tr.model, cams)
        before = evaluate.evaluate(tr.model, cams, targets).psnr
        for thr in (0.01, 0.05):
            keep = contribution.prune_mask(st_all, threshold=thr).logical_not().nonzero().squeeze(-1)
            with torch.no_grad():
                pruned = SplatModel(*[p.detach().index_select(0, keep).contiguous() for p in tr.model.parameters()], tr.model.max_sh_degree, tr.model.active_sh_degree)
            table.append({"threshold": thr, "n_before": int(tr.model.means.shape[0]), "n_after": int(keep.numel()), "psnr_train_views_before": round(before, 4),
                          "psnr_train_views_after": round(evaluate.evaluate(pruned, cams, targets).psnr, 4)})
        out["whole_prune"] = {"scene": os.path.basename(os.path.normpath(args.colmap)), "views": len(ds), "size": [scene.width, scene.height], "log": tr.contribution_log,
                              "median_step_s": round(med, 5), "prune_s": round(prune_s, 4), "steps_100_s": round(sum(times), 4), "prune_share_of_100_steps": round(prune_s / sum(times), 4),
                              "thresholds_on_the_100_step_model": table, "note": "a synthetic stand-in after 100 steps: not measured on real data"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
