#!/usr/bin/env python3
"""Same-process A/B of the default and the filtered mode (the 3D smoothing filter) of the fastgs (EWA) rasterizer on SYN-B (1 M Gaussians,
1920 x 1080, SH degree 3) - the method of tools/time_fastgs_aa.py: after a warm-up of each form, `--rounds` rounds alternate between the modes. Per mode, the median
over the rounds and the round-to-round spread (max - min) of

  preprocess_us   one lfs_fastgs_view_preprocess[_ex] call (memset, the per-primitive kernel, the tile scan, the count read-back, the SH colours), between device events
  prep_bwd_us     the per-primitive stage of the backward: the "fastgs_preprocess_bwd" scope of the library's event profiler, blend backward held out (debug bit 1)
  step_ms         one GutTrainer(rasterizer="fastgs") train_step, between device events (the filtered trainer with filter3d_every past the run: the recomputation is
                  timed on its own below, not inside the step)

and, once, `filter3d_compute_ms`: lfs_filter3d_compute over all N Gaussians and --cameras cameras on a ring around the scene (median and spread over the rounds),
with its share of 100 default steps.

On a library without lfs_fastgs_view_preprocess_ex the filtered mode and the filter computation are left out and the default mode alone is timed: such a run (this
file copied into a checkout of the parent commit) is the baseline the default mode's step is held to - not slower than the baseline by more than the baseline's own
round-to-round spread; --baseline FILE puts both numbers and the verdict into the output. The filtered mode's cost is reported, not gated.

    python tools/time_fastgs_filter3d.py [--out profiles/r13/fastgs_filter3d.json] [--baseline parent.json] [--rounds 7] [--calls 20] [--warmup 10] [--cameras 200]
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def ring_cameras(torch, centre, radius, count, width, height, focal):
    """viewmats [count,4,4] and Ks [count,3,3] of cameras on a horizontal ring around `centre`, looking at it"""
    vms, Ks = [], []
    for k in range(count):
        a = 2 * math.pi * k / count
        eye = centre + torch.tensor([radius * math.sin(a), 0.1 * radius * math.cos(3 * a), -radius * math.cos(a)], dtype=torch.float64)
        f = centre - eye
        f = f / f.norm()
        r = torch.linalg.cross(torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64), f)
        r = r / r.norm()
        d = torch.linalg.cross(f, r)
        w = torch.eye(4, dtype=torch.float64)
        w[:3, :3] = torch.stack([r, d, f])
        w[:3, 3] = -w[:3, :3] @ eye
        vms.append(w)
        Ks.append(torch.tensor([[focal, 0, width / 2], [0, focal, height / 2], [0, 0, 1]], dtype=torch.float64))
    return torch.stack(vms).float(), torch.stack(Ks).float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "fastgs_filter3d.json"))
    ap.add_argument("--baseline", default=None, help="the output of this tool on the parent commit")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--cameras", type=int, default=200)
    args = ap.parse_args()
    import torch

    import lichtfeld_studio_amd as lfs
    from lichtfeld_studio_amd import capi, fastgs, scenes
    from lichtfeld_studio_amd.capi import ptr, stream
    from lichtfeld_studio_amd.trainer import GutTrainer
    if not torch.cuda.is_available():
        raise SystemExit("time_fastgs_filter3d.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    lib = lfs.load_library()
    have = hasattr(lib, "lfs_fastgs_view_preprocess_ex")
    modes = ["default"] + (["filtered"] if have else [])
    sc = scenes.syn_b(n=args.n, n_views=4).to(dev)
    target = scenes.target_image(sc.height, sc.width).to(dev)
    trainers = {m: GutTrainer(sc, dev, iterations=30000, rasterizer="fastgs", **({"filter3d": True, "filter3d_every": 10 ** 9} if m == "filtered" else {})) for m in modes}

    # the raw entries on fixed inputs
    tr0 = trainers["default"]
    s = tr0._fastgs_settings(0)
    means, sh0, shN, raw_scales, raw_quats, raw_opac = [p.detach().clone().contiguous() for p in tr0.model.parameters()]   # (copies: the trainers go on updating theirs)
    w2c, cam = sc.viewmats[0].contiguous(), s.cam_position.reshape(-1)[:3].contiguous()
    N = means.shape[0]
    pws = torch.empty(lib.lfs_fastgs_primitive_workspace_bytes(C.c_uint32(N), C.c_uint32(s.width), C.c_uint32(s.height)), dtype=torch.uint8, device=dev)
    n_dev = torch.zeros(1, dtype=torch.int64, device=dev)
    view = fastgs.view_struct(s, means, raw_scales, raw_quats, raw_opac.reshape(-1), sh0, shN, w2c, cam, pws)
    fvar, ext, packed_ring = None, None, None
    if have:
        from lichtfeld_studio_amd import filter3d
        fvar = trainers["filtered"].update_filter3d().clone()
        ext = capi.FastgsViewExt(ptr(fvar))
        z = (means @ sc.viewmats[0][:3, :3].T + sc.viewmats[0][:3, 3])[:, 2]
        vm, Ks = ring_cameras(torch, means.double().mean(0).cpu(), float(z.mean()), args.cameras, sc.width, sc.height, float(sc.Ks[0][0, 0]))
        packed_ring = filter3d.pack_cameras(viewmats=vm, Ks=Ks, width=int(sc.width), height=int(sc.height), device=dev)
        ring_out = torch.empty(N, device=dev)

    def preprocess(mode):
        if mode == "filtered":
            capi.check(lib.lfs_fastgs_view_preprocess_ex(C.byref(view), C.c_uint32(0), C.byref(ext), ptr(n_dev), stream()), "view_preprocess_ex")
        else:
            capi.check(lib.lfs_fastgs_view_preprocess(C.byref(view), C.c_uint32(0), ptr(n_dev), stream()), "view_preprocess")

    # one forward + backward per mode; the later backward calls keep its accumulator rows (debug bit 1) and run the per-primitive stage only
    state = {}
    for m in modes:
        st = fastgs.FastGSSettings(s.cam_position, s.active_sh_bases, s.width, s.height, s.focal_x, s.focal_y, s.center_x, s.center_y, s.near_plane, s.far_plane,
                                   *((False, "none", fvar) if m == "filtered" else ()))
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
    compute = (lambda: filter3d.compute_filter3d(means, packed_ring, out=ring_out)) if have else None
    for m in modes:
        window(lambda: preprocess(m), args.warmup)
        scope_us(m, args.warmup)
        window(lambda: step(m), args.warmup)
    if have:
        window(compute, args.warmup)
    keys = ("preprocess_us", "prep_bwd_us", "step_ms")
    rounds = {m: {k: [] for k in keys} for m in modes}
    compute_ms = []
    for _ in range(args.rounds):
        for m in modes:
            rounds[m]["preprocess_us"].append(1e3 * window(lambda: preprocess(m), args.calls))
            rounds[m]["prep_bwd_us"].append(scope_us(m, args.calls))
            rounds[m]["step_ms"].append(window(lambda: step(m), args.calls))
        if have:
            compute_ms.append(window(compute, args.calls))
    out = {"scene": "SYN-B", "gaussians": N, "size": [sc.width, sc.height], "sh_degree": 3, "rounds": args.rounds, "calls_per_round": args.calls, "warmup_calls": args.warmup,
           "library": lib.lfs_version().decode(), "device": torch.cuda.get_device_name(0), "modes": {}}
    for m in modes:
        out["modes"][m] = {k: {"rounds": [round(x, 3) for x in v], "median": round(statistics.median(v), 3), "spread": round(max(v) - min(v), 3)} for k, v in rounds[m].items()}
    if have:
        d, f = out["modes"]["default"], out["modes"]["filtered"]
        out["filtered_step_over_default_percent"] = round(100.0 * (f["step_ms"]["median"] / d["step_ms"]["median"] - 1.0), 2)
        out["filtered_trainer_recomputed_the_filter"] = trainers["filtered"].filter3d_computes
        med = statistics.median(compute_ms)
        out["filter3d_compute_ms"] = {"cameras": args.cameras, "rounds": [round(x, 4) for x in compute_ms], "median": round(med, 4), "spread": round(max(compute_ms) - min(compute_ms), 4),
                                      "percent_of_100_default_steps": round(100.0 * med / (100.0 * d["step_ms"]["median"]), 4)}
    if args.baseline:
        base = json.load(open(args.baseline))
        b, d = base["modes"]["default"]["step_ms"], out["modes"]["default"]["step_ms"]
        out["baseline"] = {"library": base["library"], "default": base["modes"]["default"]}
        out["default_step_minus_baseline_ms"] = round(d["median"] - b["median"], 3)
        out["default_step_within_baseline_spread"] = bool(d["median"] - b["median"] <= b["spread"])
    try:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import kernel_resources
        out["kernel_resources"] = {k: v for k, v in sorted(kernel_resources.kernels(capi.library_path()).items()) if "fg_preprocess" in k or "filter3d" in k}
    except Exception as e:   # the static table is a convenience here: the tests/test_kernel_resources_*.py files are the check
        out["kernel_resources_error"] = repr(e)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
