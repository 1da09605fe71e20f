#!/usr/bin/env python3
"""What ADC's densification statistic costs on the 3DGUT route, and how it compares with the EWA route's. One process, on the GPU.

  (i)  finish_us        SYN-B (1 M Gaussians, 1920 x 1080, SH degree 3): the gradient-tensor finish pass of one view, default form (raster_finish_adam_kernel<false>, the
                        "finish_grads" scope of the library's event profiler - byte for byte the parent commit's kernel, tools/code_object_identity.py) against the
                        densifying form (raster_finish_densify_kernel, "finish_densify"), alternating round by round after a warm-up of both. Median over the rounds and
                        round-to-round spread (max - min). Reported, not gated.
  (ii) ratio            syn_a, one view, the same dL/d(render) into both rasterizers: s_i(3DGUT) / s_i(fastgs) over the Gaussians both count as visible - median and
                        10 - 90 % range. Says how far grad_threshold transfers between the two rasterizers. Reported, not asserted.

    python tools/time_gut_densify.py [--out profiles/r16/gut_densify.json] [--rounds 7] [--calls 20] [--warmup 10] [--n 1000000]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16", "gut_densify.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--n", type=int, default=1_000_000)
    args = ap.parse_args()
    import torch

    import lichtfeld_studio_amd as lfs
    from lichtfeld_studio_amd import capi, fastgs, scenes
    from lichtfeld_studio_amd.gut_step import GutStep
    from lichtfeld_studio_amd.trainer import GutTrainer
    if not torch.cuda.is_available():
        raise SystemExit("time_gut_densify.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    lib = lfs.load_library()

    # ---- (i) the two forms of the finish pass on SYN-B --------------------------------------------------------------------------------------------------------------
    sc = scenes.syn_b(n=args.n, n_views=4).to(dev)
    params = [t.contiguous() for t in (sc.means, sc.sh0, sc.shN, sc.raw_scales, sc.raw_quats, sc.raw_opacities)]
    N, W, H = params[0].shape[0], sc.width, sc.height
    vm, Km, bg = sc.viewmats[0].contiguous(), sc.Ks[0].contiguous(), torch.zeros(3, device=dev)
    v_render = torch.randn(H, W, 3, device=dev) * 1e-3
    gs = GutStep(dev)
    grads = [torch.zeros_like(p) for p in params]
    dens = torch.zeros(2, N, device=dev)
    n_isects = gs.view_forward(params, 3, W, H, vm, Km, bg)
    gs.view_backward_sh(params, 3, W, H, vm, Km, bg, grads, False, v_render=v_render)   # leaves the accumulator rows and dL/d(dirs) in the workspace: the finish passes only read them
    forms = {"default": {}, "densify": {"densification_info": dens}}

    def scope_us(form, calls):
        capi.profile_enable(True)
        try:
            capi.profile_collect()
            for _ in range(calls):
                gs.view_backward_finish(params, 3, W, H, vm, Km, bg, grads, False, **forms[form])
            torch.cuda.synchronize()
            got = capi.profile_collect()
        finally:
            capi.profile_enable(False)
        key = "finish_grads" if form == "default" else "finish_densify"
        assert key in got and ("finish_densify" in got) == (form == "densify"), sorted(got)
        return 1e3 * got[key][0] / got[key][1]

    for form in forms:
        scope_us(form, args.warmup)
    finish_us = {form: [] for form in forms}
    for _ in range(args.rounds):
        for form in forms:
            finish_us[form].append(scope_us(form, args.calls))

    def stats(v):
        return {"rounds": [round(x, 3) for x in v], "median": round(statistics.median(v), 3), "spread": round(max(v) - min(v), 3)}
    out = {"library": lib.lfs_version().decode(), "device": torch.cuda.get_device_name(0),
           "finish_pass": {"scene": "SYN-B", "gaussians": N, "size": [W, H], "sh_degree": 3, "n_isects": n_isects, "rounds": args.rounds, "calls_per_round": args.calls,
                           "warmup_calls": args.warmup, "finish_us": {form: stats(v) for form, v in finish_us.items()}}}
    d, e = out["finish_pass"]["finish_us"]["default"], out["finish_pass"]["finish_us"]["densify"]
    out["finish_pass"]["densify_minus_default_us"] = round(e["median"] - d["median"], 3)
    out["finish_pass"]["densify_over_default_percent"] = round(100.0 * (e["median"] / d["median"] - 1.0), 2)
    out["finish_pass"]["above_default_spread"] = bool(e["median"] - d["median"] > d["spread"])
    del gs, grads, dens, params, sc

    # ---- (ii) the statistic of the two rasterizers on one syn_a view, the same dL/d(render) ----------------------------------------------------------------------------
    sa = scenes.syn_a(n=10_000, sh_degree=2)
    tr = GutTrainer(sa, dev, iterations=100, rasterizer="fastgs")
    means, sh0, shN, raw_scales, raw_quats, raw_opac = [p.detach().contiguous() for p in tr.model.parameters()]
    Na, Wa, Ha = means.shape[0], sa.width, sa.height
    v_img = torch.randn(3, Ha, Wa, generator=torch.Generator().manual_seed(11)).to(dev) * 1e-3          # dL/d(image) [3,H,W]
    st = tr._fastgs_settings(0)
    w2c = tr.scene.viewmats[0].contiguous()
    image, alpha, pws, iws, n_inst = fastgs.forward_wrapper(means, raw_scales, raw_quats, raw_opac, sh0, shN, w2c, st)
    d_fg = torch.zeros(2, Na, device=dev)
    fastgs.backward_wrapper(d_fg, v_img.contiguous(), torch.zeros_like(alpha), image, alpha, means, raw_scales, raw_quats, sh0, shN, pws, iws, w2c, st, n_inst)
    g2 = GutStep(dev)
    ps = [means, sh0, shN, raw_scales, raw_quats, raw_opac]
    g2.view_forward(ps, tr.model.get_active_sh_degree(), Wa, Ha, w2c, tr.scene.Ks[0].contiguous(), tr.bg)
    d_gut = torch.zeros(2, Na, device=dev)
    g2.view_backward(ps, tr.model.get_active_sh_degree(), Wa, Ha, w2c, tr.scene.Ks[0].contiguous(), tr.bg, [torch.zeros_like(p) for p in ps], False,
                     v_render=v_img.permute(1, 2, 0).contiguous(), densification_info=d_gut)
    torch.cuda.synchronize()
    both = (d_fg[0] > 0) & (d_gut[0] > 0) & (d_fg[1] > 0)
    r = (d_gut[1][both] / d_fg[1][both]).double().cpu()
    q = torch.quantile(r, torch.tensor([0.1, 0.5, 0.9], dtype=torch.float64))
    thr = 2e-4
    out["cross_rasterizer"] = {"scene": "syn_a", "gaussians": Na, "size": [Wa, Ha], "sh_degree": 2, "v_render_scale": 1e-3,
                               "visible": {"gut": int((d_gut[0] > 0).sum()), "fastgs": int((d_fg[0] > 0).sum()), "both": int(both.sum())},
                               "s_gut_over_s_fastgs": {"p10": round(float(q[0]), 4), "median": round(float(q[1]), 4), "p90": round(float(q[2]), 4)},
                               "above_grad_threshold_2e-4": {"gut": int((d_gut[1] > thr).sum()), "fastgs": int((d_fg[1] > thr).sum()),
                                                             "both": int(((d_gut[1] > thr) & (d_fg[1] > thr)).sum())}}
    try:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import kernel_resources
        out["kernel_resources"] = {k: v for k, v in sorted(kernel_resources.kernels(capi.library_path()).items()) if "raster_finish_adam" in k or "raster_finish_densify" in k}
    except Exception as e:   # the static table is a convenience here: tests/test_kernel_resources_gut_densify.py is the check
        out["kernel_resources_error"] = repr(e)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
