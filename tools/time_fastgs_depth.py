#!/usr/bin/env python3
"""Same-process A/B of the default mode and the depth mode (inverse depth) of the fastgs (EWA) rasterizer on SYN-B (1 M Gaussians, 1920 x 1080, SH degree 3) - the
method of tools/time_fastgs_aa.py: after a warm-up of each form, `--rounds` rounds alternate between the modes. Per mode, the median over the rounds and the
round-to-round spread (max - min) of

  blend_fwd_us    the blending forward: the "fastgs_blend_fwd" scope of the library's event profiler inside lfs_fastgs_view_render without / with a depth plane
  blend_bwd_us    the blending backward: the "fastgs_blend_bwd" scope inside lfs_fastgs_view_backward without / with grad_depth (nine / ten reduced values per instance)
  step_ms         one GutTrainer(rasterizer="fastgs") train_step, between device events; the depth mode's step carries a depth target for its view
                  (depth_loss="invdepth": the depth forward and backward and the fused depth loss)

The tool runs on a tree without the depth entry points too and then times the default mode only: that run is the baseline the default mode's step is held to
(not slower than the baseline by more than the baseline's own round-to-round spread; --baseline FILE puts both numbers and the verdict into the output).
The depth mode's cost is reported, not gated. VGPRs / scratch / occupancy of the instantiations come from tools/kernel_resources.py.

    python tools/time_fastgs_depth.py [--out profiles/r12/fastgs_depth.json] [--baseline parent.json] [--rounds 7] [--calls 20] [--warmup 10]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12", "fastgs_depth.json"))
    ap.add_argument("--baseline", default=None, help="the output of this tool on the parent commit")
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
        raise SystemExit("time_fastgs_depth.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    lib = lfs.load_library()
    has_depth = hasattr(lib, "lfs_fastgs_view_render")
    modes = ["default"] + (["invdepth"] if has_depth else [])
    sc = scenes.syn_b(n=args.n, n_views=4).to(dev)
    target = scenes.target_image(sc.height, sc.width).to(dev)
    trainers = {m: GutTrainer(sc, dev, iterations=30000, rasterizer="fastgs", **({"depth_loss": "invdepth"} if m == "invdepth" else {})) for m in modes}

    tr0 = trainers["default"]
    s = tr0._fastgs_settings(0)
    means, sh0, shN, raw_scales, raw_quats, raw_opac = [p.detach().clone().contiguous() for p in tr0.model.parameters()]   # (copies: the trainers go on updating theirs)
    w2c = sc.viewmats[0].contiguous()
    frame = (s.cam_position, s.active_sh_bases, s.width, s.height, s.focal_x, s.focal_y, s.center_x, s.center_y, s.near_plane, s.far_plane)

    # one forward per mode on fixed inputs; forward and backward are then repeated on that state
    state = {}
    for m in modes:
        st = fastgs.FastGSSettings(*frame) if m == "default" else fastgs.FastGSSettings(*frame, False, "invdepth")
        state[m] = dict(st=st)

    def forward(mode):
        d = state[mode]
        if mode == "default":
            d["image"], d["alpha"], d["pws"], d["iws"], d["n_inst"] = fastgs.forward_wrapper(means, raw_scales, raw_quats, raw_opac, sh0, shN, w2c, d["st"])
        else:
            d["image"], d["alpha"], d["depth"], d["pws"], d["iws"], d["n_inst"] = fastgs.forward_wrapper_depth(means, raw_scales, raw_quats, raw_opac, sh0, shN, w2c, d["st"])

    def backward(mode):
        d = state[mode]
        kw = {} if mode == "default" else {"grad_depth": d["gd"]}
        d["out"] = fastgs.backward_wrapper(None, d["gi"], d["ga"], d["image"], d["alpha"], means, raw_scales, raw_quats, sh0, shN, d["pws"], d["iws"], w2c, d["st"], d["n_inst"],
                                           out=d.get("out"), **kw)

    depths = {}
    for m in modes:
        forward(m)
        d = state[m]
        d["gi"], d["ga"] = torch.randn_like(d["image"]), torch.zeros_like(d["alpha"])
        if m != "default":
            from lichtfeld_studio_amd import losses
            d["gd"] = torch.randn_like(d["depth"])
            # the step's depth targets: the scene's own inverse depth, rendered per view, off by 5 % (so that the loss has a gradient everywhere it is valid)
            for v in range(4):
                sv = trainers[m]._fastgs_settings(v)
                sv.depth = "invdepth"
                dep = fastgs.forward_wrapper_depth(means, raw_scales, raw_quats, raw_opac, sh0, shN, sc.viewmats[v].contiguous(), sv)[2]
                depths[v] = losses.prepare_depth(dep * 1.05)
        backward(m)

    def window(fn, calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / calls   # ms per call

    def scope_us(name, fn, calls):
        capi.profile_filter(name)
        capi.profile_enable(True)
        try:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            ms, count = capi.profile_collect()[name]
        finally:
            capi.profile_enable(False)
            capi.profile_filter(None)
        return 1e3 * ms / count

    def step(m):
        tr = trainers[m]
        v = tr.iteration % 4
        if m == "default":
            tr.train_step([target], views=[v])
        else:
            tr.train_step([target], views=[v], depths=[depths[v]])

    for m in modes:
        scope_us("fastgs_blend_fwd", lambda: forward(m), args.warmup)
        scope_us("fastgs_blend_bwd", lambda: backward(m), args.warmup)
        window(lambda: step(m), args.warmup)
    keys = ("blend_fwd_us", "blend_bwd_us", "step_ms")
    rounds = {m: {k: [] for k in keys} for m in modes}
    for _ in range(args.rounds):
        for m in modes:
            rounds[m]["blend_fwd_us"].append(scope_us("fastgs_blend_fwd", lambda: forward(m), args.calls))
            rounds[m]["blend_bwd_us"].append(scope_us("fastgs_blend_bwd", lambda: backward(m), args.calls))
            rounds[m]["step_ms"].append(window(lambda: step(m), args.calls))
    N = means.shape[0]
    out = {"scene": "SYN-B", "gaussians": N, "size": [sc.width, sc.height], "sh_degree": 3, "rounds": args.rounds, "calls_per_round": args.calls, "warmup_calls": args.warmup,
           "library": lib.lfs_version().decode(), "device": torch.cuda.get_device_name(0), "n_instances": int(state["default"]["n_inst"]), "modes": {}}
    for m in modes:
        out["modes"][m] = {k: {"rounds": [round(x, 3) for x in v], "median": round(statistics.median(v), 3), "spread": round(max(v) - min(v), 3)} for k, v in rounds[m].items()}
    if args.baseline:
        base = json.load(open(args.baseline))
        b, d = base["modes"]["default"]["step_ms"], out["modes"]["default"]["step_ms"]
        out["baseline"] = {"library": base["library"], "default": base["modes"]["default"]}
        out["default_step_minus_baseline_ms"] = round(d["median"] - b["median"], 3)
        out["default_step_within_baseline_spread"] = bool(d["median"] - b["median"] <= b["spread"])
    try:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import kernel_resources
        out["kernel_resources"] = {k: v for k, v in sorted(kernel_resources.kernels(capi.library_path()).items()) if "fg_blend" in k or "fg_preprocess" in k}
    except Exception as e:   # the static table is a convenience here: tests/test_kernel_resources_fastgs_depth.py is the check
        out["kernel_resources_error"] = repr(e)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
