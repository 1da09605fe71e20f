#!/usr/bin/env python3
"""Same-process A/B of the default and the antialiased mode of the fastgs (EWA) rasterizer on SYN-B (1 M Gaussians, 1920 x 1080, SH degree 3) - the method of
tools/time_masked_loss.py: after a warm-up of each form, `--rounds` rounds alternate between the modes. Per mode, the median over the rounds and the round-to-round
spread (max - min) of

  preprocess_us   one lfs_fastgs_view_preprocess call (memset, the per-primitive kernel, the tile scan, the count read-back, the SH colours), between device events
  prep_bwd_us     the per-primitive stage of the backward: the "fastgs_preprocess_bwd" scope of the library's event profiler (both instantiations of
                  fg_preprocess_bwd_kernel are queued, the one that does not match the workspace's mode word returns at once), blend backward held out (debug bit 1)
  step_ms         one GutTrainer(rasterizer="fastgs") train_step, between device events

On a library without lfs_fastgs_view_preprocess the antialiased mode is left out and the default mode alone is timed: such a run is the baseline the default mode's step is held to
(not slower than the baseline by more than the baseline's own round-to-round spread; --baseline FILE puts both numbers and the verdict into the output).
The antialiased mode's cost is reported, not gated. VGPRs / scratch / occupancy of the instantiations come from tools/kernel_resources.py.

    python tools/time_fastgs_aa.py [--out profiles/r11/fastgs_antialiased.json] [--baseline parent.json] [--rounds 7] [--calls 20] [--warmup 10]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "fastgs_antialiased.json"))
    ap.add_argument("--baseline", default=None, help="the output of this tool on the parent commit")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--n", type=int, default=1_000_000)
    args = ap.parse_args()
    import torch

    import lichtfeld_studio_amd as lfs
    from lichtfeld_studio_amd import capi, fastgs, scenes
    from lichtfeld_studio_amd.capi import ptr, stream
    from lichtfeld_studio_amd.trainer import GutTrainer
    if not torch.cuda.is_available():
        raise SystemExit("time_fastgs_aa.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    lib = lfs.load_library()
    modes = ["default"] + (["antialiased"] if hasattr(lib, "lfs_fastgs_view_preprocess") else [])
    sc = scenes.syn_b(n=args.n, n_views=4).to(dev)
    target = scenes.target_image(sc.height, sc.width).to(dev)
    trainers = {m: GutTrainer(sc, dev, iterations=30000, rasterizer="fastgs", **({"antialiasing": True} if m == "antialiased" else {})) for m in modes}

    # the raw entry on fixed inputs
    tr0 = trainers["default"]
    s = tr0._fastgs_settings(0)
    means, sh0, shN, raw_scales, raw_quats, raw_opac = [p.detach().clone().contiguous() for p in tr0.model.parameters()]   # (copies: the trainers go on updating theirs)
    w2c, cam = sc.viewmats[0].contiguous(), s.cam_position.reshape(-1)[:3].contiguous()
    N = means.shape[0]
    pws = torch.empty(lib.lfs_fastgs_primitive_workspace_bytes(C.c_uint32(N), C.c_uint32(s.width), C.c_uint32(s.height)), dtype=torch.uint8, device=dev)
    n_dev = torch.zeros(1, dtype=torch.int64, device=dev)
    view = fastgs.view_struct(s, means, raw_scales, raw_quats, raw_opac.reshape(-1), sh0, shN, w2c, cam, pws)

    def preprocess(mode):
        capi.check(lib.lfs_fastgs_view_preprocess(C.byref(view), C.c_uint32(1 if mode == "antialiased" else 0), ptr(n_dev), stream()), "view_preprocess")

    # one forward + backward per mode; the later backward calls keep its accumulator rows (debug bit 1) and run the per-primitive stage only
    state = {}
    for m in modes:
        st = fastgs.FastGSSettings(s.cam_position, s.active_sh_bases, s.width, s.height, s.focal_x, s.focal_y, s.center_x, s.center_y, s.near_plane, s.far_plane,
                                   *((True,) if m == "antialiased" else ()))
        image, alpha, p, i, n_inst = fastgs.forward_wrapper(means, raw_scales, raw_quats, raw_opac, sh0, shN, w2c, st)
        gi, ga = torch.randn_like(image), torch.zeros_like(alpha)
        state[m] = dict(st=st, image=image, alpha=alpha, pws=p, iws=i, n_inst=n_inst, gi=gi, ga=ga, out=None)
        state[m]["out"] = fastgs.backward_wrapper(None, gi, ga, image, alpha, means, raw_scales, raw_quats, sh0, shN, p, i, w2c, st, n_inst)

    def prep_bwd(mode):
        d = state[mode]
        fastgs.backward_wrapper(None, d["gi"], d["ga"], d["image"], d["alpha"], means, raw_scales, raw_quats, sh0, shN, d["pws"], d["iws"], w2c, d["st"], d["n_inst"],
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

    def scope_us(mode, calls):
        lib.lfs_fastgs_set_debug_flags(2)
        capi.profile_filter("fastgs_preprocess_bwd")
        capi.profile_enable(True)
        try:
            for _ in range(calls):
                prep_bwd(mode)
            torch.cuda.synchronize()
            ms, count = capi.profile_collect()["fastgs_preprocess_bwd"]
        finally:
            capi.profile_enable(False)
            capi.profile_filter(None)
            lib.lfs_fastgs_set_debug_flags(0)
        return 1e3 * ms / count

    step = lambda m: trainers[m].train_step([target], views=[trainers[m].iteration % 4])
    for m in modes:
        window(lambda: preprocess(m), args.warmup)
        scope_us(m, args.warmup)
        window(lambda: step(m), args.warmup)
    keys = ("preprocess_us", "prep_bwd_us", "step_ms")
    rounds = {m: {k: [] for k in keys} for m in modes}
    for _ in range(args.rounds):
        for m in modes:
            rounds[m]["preprocess_us"].append(1e3 * window(lambda: preprocess(m), args.calls))
            rounds[m]["prep_bwd_us"].append(scope_us(m, args.calls))
            rounds[m]["step_ms"].append(window(lambda: step(m), args.calls))
    out = {"scene": "SYN-B", "gaussians": N, "size": [sc.width, sc.height], "sh_degree": 3, "rounds": args.rounds, "calls_per_round": args.calls, "warmup_calls": args.warmup,
           "library": lib.lfs_version().decode(), "device": torch.cuda.get_device_name(0), "modes": {}}
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
        out["kernel_resources"] = {k: v for k, v in sorted(kernel_resources.kernels(capi.library_path()).items()) if "fg_preprocess" in k}
    except Exception as e:   # the static table is a convenience here: tests/test_kernel_resources.py is the check
        out["kernel_resources_error"] = repr(e)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
