#!/usr/bin/env python3
"""What the absgrad mode of the fastgs (EWA) rasterizer (LFS_FASTGS_ABSGRAD) costs, on SYN-B (1 M Gaussians, 1920 x 1080, SH degree 3). One process; after a
warm-up of every form, `--rounds` rounds alternate between the forms. Per form, the median over the rounds and the round-to-round spread (max - min) of

  (i)   step_ms         one GutTrainer(rasterizer="fastgs") train_step of the DEFAULT mode, between device events - with this checkout's library and, with
                        --parent-lib PATH, with the parent commit's liblfs_gsplat.so loaded into the same process (each library drives a trainer of its own; the two
                        alternate round by round). Acceptance: this library's median is not above the parent's by more than the parent's own spread.
  (ii)  blend_bwd_us    the blend backward of one lfs_fastgs_view_backward with densification_info set, on a default workspace (fg_blend_bwd_kernel) and on an absgrad
                        workspace (fg_blend_bwd_abs_kernel): the "fastgs_blend_bwd" scope of the library's event profiler
  (iii) densify_abs_us  fg_densify_abs_kernel alone: the "fastgs_densify_abs" scope of the same absgrad backward calls

(ii) and (iii) are reported, not gated.

    python tools/time_fastgs_absgrad.py [--out profiles/r14/fastgs_absgrad.json] [--parent-lib /path/to/parent/liblfs_gsplat.so] [--rounds 7] [--calls 20] [--warmup 10]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "fastgs_absgrad.json"))
    ap.add_argument("--parent-lib", default=None, help="liblfs_gsplat.so built from the parent commit: its default step alternates with this checkout's")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--n", type=int, default=1_000_000)
    args = ap.parse_args()
    import torch

    import lichtfeld_studio_amd as lfs
    from lichtfeld_studio_amd import capi, fastgs, scenes
    from lichtfeld_studio_amd.trainer import GutTrainer
    if not torch.cuda.is_available():
        raise SystemExit("time_fastgs_absgrad.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    libs = {"this": lfs.load_library()}
    if args.parent_lib:   # a second library in the same process: capi hands out whichever one is current (capi._LIB), every call of the package asks it
        saved = os.environ.get("LFS_GSPLAT_LIB")
        os.environ["LFS_GSPLAT_LIB"], capi._LIB = os.path.abspath(args.parent_lib), None
        libs["parent"] = capi.load_library()
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

    # (ii), (iii): one forward per form on fixed inputs, then backward calls with densification_info on its workspace
    tr0 = trainers["this"]
    s = tr0._fastgs_settings(0)
    means, sh0, shN, raw_scales, raw_quats, raw_opac = [p.detach().clone().contiguous() for p in tr0.model.parameters()]   # (copies: the trainers go on updating theirs)
    w2c = sc.viewmats[0].contiguous()
    N = means.shape[0]
    forms = ("default", "absgrad")
    state = {}
    for m in forms:
        st = fastgs.FastGSSettings(s.cam_position, s.active_sh_bases, s.width, s.height, s.focal_x, s.focal_y, s.center_x, s.center_y, s.near_plane, s.far_plane,
                                   absgrad=(m == "absgrad"))
        image, alpha, p, i, n_inst = fastgs.forward_wrapper(means, raw_scales, raw_quats, raw_opac, sh0, shN, w2c, st)
        gi, ga = torch.randn_like(image), torch.zeros_like(alpha)
        dens = torch.zeros(2, N, device=dev)
        state[m] = dict(st=st, image=image, alpha=alpha, pws=p, iws=i, n_inst=n_inst, gi=gi, ga=ga, dens=dens, out=None)
        state[m]["out"] = fastgs.backward_wrapper(dens, gi, ga, image, alpha, means, raw_scales, raw_quats, sh0, shN, p, i, w2c, st, n_inst)

    def backward(m):
        d = state[m]
        fastgs.backward_wrapper(d["dens"], d["gi"], d["ga"], d["image"], d["alpha"], means, raw_scales, raw_quats, sh0, shN, d["pws"], d["iws"], w2c, d["st"], d["n_inst"],
                                out=d["out"])

    def window(fn, calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / calls   # ms per call

    def scopes_us(m, calls):
        """{scope: us per call} of `calls` backward calls of form m (the scopes of the blend backward and, absgrad only, of the densification kernel)"""
        capi.profile_enable(True)
        try:
            capi.profile_collect()
            for _ in range(calls):
                backward(m)
            torch.cuda.synchronize()
            got = capi.profile_collect()
        finally:
            capi.profile_enable(False)
        return {k: 1e3 * got[k][0] / got[k][1] for k in ("fastgs_blend_bwd", "fastgs_densify_abs") if k in got}

    def step(name):
        use(name)
        try:
            tr = trainers[name]
            tr.train_step([target], views=[tr.iteration % 4])
        finally:
            use("this")

    for name in libs:
        window(lambda: step(name), args.warmup)
    for m in forms:
        scopes_us(m, args.warmup)
    step_ms = {name: [] for name in libs}
    blend_us = {m: [] for m in forms}
    densify_us = []
    for _ in range(args.rounds):
        for name in libs:
            step_ms[name].append(window(lambda: step(name), args.calls))
        for m in forms:
            got = scopes_us(m, args.calls)
            blend_us[m].append(got["fastgs_blend_bwd"])
            if m == "absgrad":
                densify_us.append(got["fastgs_densify_abs"])
            else:
                assert "fastgs_densify_abs" not in got

    def stats(v):
        return {"rounds": [round(x, 3) for x in v], "median": round(statistics.median(v), 3), "spread": round(max(v) - min(v), 3)}
    out = {"scene": "SYN-B", "gaussians": N, "size": [sc.width, sc.height], "sh_degree": 3, "rounds": args.rounds, "calls_per_round": args.calls, "warmup_calls": args.warmup,
           "libraries": {name: lib.lfs_version().decode() for name, lib in libs.items()}, "device": torch.cuda.get_device_name(0),
           "default_step_ms": {name: stats(v) for name, v in step_ms.items()},
           "blend_bwd_us": {m: stats(v) for m, v in blend_us.items()}, "densify_abs_us": stats(densify_us), "n_instances": state["default"]["n_inst"]}
    d, a = out["blend_bwd_us"]["default"]["median"], out["blend_bwd_us"]["absgrad"]["median"]
    out["abs_blend_bwd_over_default_percent"] = round(100.0 * (a / d - 1.0), 2)
    if "parent" in libs:
        t, p = out["default_step_ms"]["this"], out["default_step_ms"]["parent"]
        out["default_step_minus_parent_ms"] = round(t["median"] - p["median"], 3)
        out["default_step_within_parent_spread"] = bool(t["median"] - p["median"] <= p["spread"])
    try:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import kernel_resources
        out["kernel_resources"] = {k: v for k, v in sorted(kernel_resources.kernels(capi.library_path()).items()) if "fg_blend_bwd" in k or "fg_densify" in k}
    except Exception as e:   # the static table is a convenience here: tests/test_kernel_resources_fastgs_absgrad.py is the check
        out["kernel_resources_error"] = repr(e)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
