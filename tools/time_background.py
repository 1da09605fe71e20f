#!/usr/bin/env python3
"""What the background colour of the fastgs (EWA) route costs (lfs_background_compose / lfs_background_compose_bwd). One process; after a warm-up of every
form, `--rounds` rounds alternate between the forms. Per form, the median over the rounds and the round-to-round spread (max - min) of

  (i)   entry_us       at 1920 x 1080, between device events: the compose entry (render group alone, target group alone, both in one launch) and its backward (with and
                       without v_alpha_in), the torch sequence each replaces, and a device-to-device copy that moves the same number of bytes (read + written): the
                       streaming bound. Reported as ratios; there is no threshold.
  (ii)  step_ms        one GutTrainer(rasterizer="fastgs") train_step on SYN-B (1 M Gaussians, 1920 x 1080, SH degree 3) of the DEFAULT configuration - with this
                       checkout's library and, with --parent-lib PATH, with the parent commit's liblfs_gsplat.so loaded into the same process (each library drives a
                       trainer of its own; the two alternate round by round). Acceptance: this library's median is not above the parent's by more than the parent's
                       own spread.
  (iii) step_ms        the same step with background (0.3, 0.6, 0.9), with background_mode "random", and with "random" + an RGBA plane: the cost over the default step.
                       Reported; no threshold.
  (iv)  with --end-to-end: a SYN-A-sized object in the image centre, RGBA targets from its own render; 150 steps from a cloud that fills the image, once with
                       background_mode "random" + alphas, once on a black background with black-composited targets: the mean rendered alpha where the target alpha is 0.
                       Recorded, not asserted.

    python tools/time_background.py [--out profiles/r20/background.json] [--parent-lib /path/to/parent/liblfs_gsplat.so] [--rounds 7] [--calls 20] [--end-to-end]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BG = (0.3, 0.6, 0.9)
NEW_EXPORTS = ("lfs_background_compose", "lfs_background_compose_bwd")


def end_to_end(torch, dev, steps):
    """-> the (iv) record"""
    import math

    from lichtfeld_studio_amd import fastgs, scenes
    from lichtfeld_studio_amd.trainer import GutTrainer
    obj = scenes.syn_a(seed=7, n=4000, sh_degree=1)
    obj.means[:, :2] *= 0.3                                   # the object: the image centre only
    cloud = scenes.syn_a(seed=11, n=4000, sh_degree=1)        # what training starts from: Gaussians all over the image
    cloud.raw_opacities.fill_(math.log(0.3 / 0.7))
    gt_tr = GutTrainer(obj, dev, iterations=steps, rasterizer="fastgs")
    black = torch.zeros(3, device=dev)
    with torch.no_grad():
        gt = fastgs.fast_rasterize(gt_tr.camera(0), gt_tr.model, black)
    a = gt.alpha[0].clamp(0.0, 1.0)
    plane = (a * 255.0 + 0.5).to(torch.uint8)
    af = plane.float() / 255.0
    straight = torch.where(a > 1e-6, gt.image / a.clamp_min(1e-6), torch.zeros_like(gt.image)).clamp(0.0, 1.0)   # un-premultiplied colour
    on_black = af * straight
    outside = plane == 0

    def alpha_outside(tr):
        with torch.no_grad():
            out = fastgs.fast_rasterize(tr.camera(0), tr.model, black)
        return float(out.alpha[0][outside].mean()), float(out.alpha[0][~outside].mean())

    runs = {"random_background_with_alphas": (GutTrainer(cloud, dev, iterations=steps, rasterizer="fastgs", loss="l1_ssim", background_mode="random"), straight, [plane]),
            "black_background_black_composited_targets": (GutTrainer(cloud, dev, iterations=steps, rasterizer="fastgs", loss="l1_ssim"), on_black, None)}
    rec = {"object": "syn_a(seed=7, n=4000, sh_degree=1), x and y of the means scaled by 0.3", "start": "syn_a(seed=11, n=4000, sh_degree=1), opacity 0.3",
           "size": [obj.width, obj.height], "steps": steps, "loss": "l1_ssim", "pixels_with_target_alpha_0": int(outside.sum()), "pixels": int(outside.numel())}
    for name, (tr, target, alphas) in runs.items():
        start = alpha_outside(tr)
        for _ in range(steps):
            tr.train_step([target], views=[0], alphas=alphas)
        end = alpha_outside(tr)
        rec[name] = {"mean_alpha_where_target_alpha_is_0": {"start": round(start[0], 5), "end": round(end[0], 5)},
                     "mean_alpha_elsewhere": {"start": round(start[1], 5), "end": round(end[1], 5)}}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20", "background.json"))
    ap.add_argument("--parent-lib", default=None, help="liblfs_gsplat.so built from the parent commit: its default step alternates with this checkout's")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--end-to-end", action="store_true")
    ap.add_argument("--end-to-end-steps", type=int, default=150)
    args = ap.parse_args()
    import torch

    import lichtfeld_studio_amd as lfs
    from lichtfeld_studio_amd import capi, ops, scenes
    from lichtfeld_studio_amd.trainer import GutTrainer
    if not torch.cuda.is_available():
        raise SystemExit("time_background.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    libs = {"this": lfs.load_library()}
    if args.parent_lib:   # a second library in the same process: capi hands out whichever one is current (capi._LIB), every call of the package asks it
        saved, exports = os.environ.get("LFS_GSPLAT_LIB"), list(capi.EXPORTS)
        os.environ["LFS_GSPLAT_LIB"], capi._LIB = os.path.abspath(args.parent_lib), None
        capi.EXPORTS[:] = [e for e in exports if e not in NEW_EXPORTS]   # (the parent does not have the entries this tool is about)
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

    def window(fn, calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / calls   # ms per call

    def stats(v, digits=3):
        return {"rounds": [round(x, digits) for x in v], "median": round(statistics.median(v), digits), "spread": round(max(v) - min(v), digits)}

    # ---- (i) the two entries at 1080p ---------------------------------------------------------------------------------------------------------------------------------
    H, W = 1080, 1920
    g = torch.Generator(device=dev).manual_seed(1)
    image, target, v = (torch.rand((3, H, W), device=dev, generator=g) for _ in range(3))
    alpha, v_in = torch.rand((1, H, W), device=dev, generator=g), torch.rand((1, H, W), device=dev, generator=g)
    u8 = torch.randint(0, 256, (H, W), device=dev, generator=g, dtype=torch.uint8)
    shown, t_out, v_alpha = torch.empty_like(image), torch.empty_like(target), torch.empty_like(alpha)
    bg_t = torch.tensor(BG, device=dev).view(3, 1, 1)
    plane = 4 * H * W
    nbytes = {"compose_render": 7 * plane, "compose_target": 6 * plane + H * W, "compose_both": 13 * plane + H * W, "bwd": 4 * plane, "bwd_with_v_alpha_in": 5 * plane}
    src, dst = torch.empty(13 * plane // 2 + H * W, dtype=torch.uint8, device=dev), torch.empty(13 * plane // 2 + H * W, dtype=torch.uint8, device=dev)

    def torch_target():
        a = u8.float() / 255.0
        return a * target + (1.0 - a) * bg_t

    forms = {
        "compose_render": (lambda: ops.background_compose(BG, image, alpha, shown), lambda: image + (1.0 - alpha) * bg_t),
        "compose_target": (lambda: ops.background_compose(BG, target_rgb=target, target_alpha=u8, target_out=t_out), torch_target),
        "compose_both": (lambda: ops.background_compose(BG, image, alpha, shown, target, u8, t_out), lambda: (image + (1.0 - alpha) * bg_t, torch_target())),
        "bwd": (lambda: ops.background_compose_bwd(BG, v, None, v_alpha), lambda: -(v * bg_t).sum(0, keepdim=True)),
        "bwd_with_v_alpha_in": (lambda: ops.background_compose_bwd(BG, v, v_in, v_alpha), lambda: v_in - (v * bg_t).sum(0, keepdim=True)),
    }
    timed = {}
    for name, (entry, seq) in forms.items():
        half = nbytes[name] // 2
        timed[name] = {"entry": entry, "torch": seq, "copy": (lambda h=half: dst[:h].copy_(src[:h]))}
    entry_us = {name: {k: [] for k in fs} for name, fs in timed.items()}
    for fs in timed.values():
        for fn in fs.values():
            window(fn, args.warmup)
    for _ in range(args.rounds):
        for name, fs in timed.items():
            for k, fn in fs.items():
                entry_us[name][k].append(1e3 * window(fn, args.calls))
    out = {"device": torch.cuda.get_device_name(0), "libraries": {name: lib.lfs_version().decode() for name, lib in libs.items()}, "rounds": args.rounds,
           "calls_per_round": args.calls, "warmup_calls": args.warmup, "background": list(BG), "entries_1920x1080": {}}
    for name, rec in entry_us.items():
        e = {k: stats(vv, 2) for k, vv in rec.items()}
        med = {k: e[k]["median"] for k in e}
        out["entries_1920x1080"][name] = {"bytes_moved": nbytes[name], "us": e, "entry_GBps": round(nbytes[name] / med["entry"] / 1e3, 1),
                                          "entry_over_copy": round(med["entry"] / med["copy"], 3), "torch_over_entry": round(med["torch"] / med["entry"], 2)}
    del image, target, v, alpha, v_in, u8, shown, t_out, v_alpha, src, dst

    # ---- (ii), (iii) the training step on SYN-B -----------------------------------------------------------------------------------------------------------------------
    sc = scenes.syn_b(n=args.n, n_views=4).to(dev)
    target = scenes.target_image(sc.height, sc.width).to(dev)
    plane_u8 = torch.randint(0, 256, (sc.height, sc.width), device=dev, generator=g, dtype=torch.uint8)
    trainers = {}
    for name in libs:
        use(name)
        trainers[name] = (name, GutTrainer(sc, dev, iterations=30000, rasterizer="fastgs"), None)
    use("this")
    trainers["colour"] = ("this", GutTrainer(sc, dev, iterations=30000, rasterizer="fastgs", background=BG), None)
    trainers["random"] = ("this", GutTrainer(sc, dev, iterations=30000, rasterizer="fastgs", background_mode="random"), None)
    trainers["random_with_alphas"] = ("this", GutTrainer(sc, dev, iterations=30000, rasterizer="fastgs", background_mode="random"), [plane_u8])

    def step(key):
        lib, tr, alphas = trainers[key]
        use(lib)
        try:
            tr.train_step([target], views=[tr.iteration % 4], **({} if alphas is None else {"alphas": alphas}))
        finally:
            use("this")

    for key in trainers:
        window(lambda: step(key), args.warmup)
    step_ms = {key: [] for key in trainers}
    for _ in range(args.rounds):
        for key in trainers:
            step_ms[key].append(window(lambda: step(key), args.calls))
    out["step_SYN-B_fastgs"] = {"gaussians": int(sc.means.shape[0]), "size": [sc.width, sc.height], "sh_degree": 3, "ms": {k: stats(vv) for k, vv in step_ms.items()}}
    ms = out["step_SYN-B_fastgs"]["ms"]
    for key in ("colour", "random", "random_with_alphas"):
        out["step_SYN-B_fastgs"][f"{key}_minus_default_ms"] = round(ms[key]["median"] - ms["this"]["median"], 3)
    if "parent" in libs:
        out["step_SYN-B_fastgs"]["default_step_minus_parent_ms"] = round(ms["this"]["median"] - ms["parent"]["median"], 3)
        out["step_SYN-B_fastgs"]["default_step_within_parent_spread"] = bool(ms["this"]["median"] - ms["parent"]["median"] <= ms["parent"]["spread"])
    del trainers, sc
    if args.end_to_end:
        out["end_to_end"] = end_to_end(torch, dev, args.end_to_end_steps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
