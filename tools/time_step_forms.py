#!/usr/bin/env python3
"""Same-process A/B of GutTrainer(one_call=False | True) for the configurations the one-call step gained with lfs_gut_train_step_opt (bench.py measures the MSE step
and is left alone):

    l1_ssim        L1 + D-SSIM, no strategy, from iteration 3000
    l1_ssim_mcmc   L1 + D-SSIM + MCMC at the cap (max_cap = N: no growth), from iteration 3000; refining iterations run OUTSIDE the timed windows (both forms take the
                   split form there)
    mse_early      the clamped MSE while iteration <= 1000 (shN frozen), from iteration 100

Workload: SYN-B - 1 M Gaussians, 1920 x 1080, SH degree 3, 64 orbit cameras, round-robin views. Per configuration two trainers live side by side; after a warm-up of each,
`--rounds` rounds of `--steps` steps alternate between them (off, on, off, on, ...), each round synchronised at both ends. EVERY round starts from the state the
trainer had after its warm-up (parameters, Adam moments and counts, learning rates, iteration, the strategy's generator: snapshot / restore below): training changes
the scene and with it the work per step, and the two forms compute the same trajectory, so all rounds of a configuration time the same 200 steps. Per form: the median over the rounds of ms / step and the round-to-round spread (max - min). The one-call form counts as a speed-up for a
configuration only where its median beats the split form's by more than the split form's own spread. One JSON document -> --out (default profiles/r07/one_call_options.json).

    python tools/time_step_forms.py [--out FILE] [--n 1000000] [--rounds 5] [--steps 200] [--warmup 40] [--configs l1_ssim,l1_ssim_mcmc,mse_early]
    python tools/time_step_forms.py --only l1_ssim_mcmc:on --steps 60 --warmup 20     # one form alone, e.g. under a kernel trace
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_trainer(scene, dev, config, one_call, n):
    from lichtfeld_studio_amd import strategies
    from lichtfeld_studio_amd.trainer import GutTrainer
    if config == "l1_ssim":
        tr = GutTrainer(scene, dev, iterations=30000, loss="l1_ssim", one_call=one_call)
    elif config == "l1_ssim_mcmc":
        tr = GutTrainer(scene, dev, iterations=30000, loss="l1_ssim", strategy="mcmc", one_call=one_call,
                        opt_params=strategies.OptimizationParameters(iterations=30000, max_cap=n))
    elif config == "mse_early":
        tr = GutTrainer(scene, dev, iterations=30000, loss="mse", one_call=one_call)
    else:
        raise ValueError(config)
    tr.iteration = 100 if config == "mse_early" else 3000
    return tr


def snapshot(tr):
    opt = tr.optimizer
    snap = {"params": [p.detach().clone() for p in tr.model.parameters()], "lr": [g["lr"] for g in opt.param_groups], "iteration": tr.iteration,
            "degree": tr.model.active_sh_degree, "state": {}, "gen": tr.strategy.generator.get_state() if tr.strategy is not None else None}
    for p in tr.model.parameters():
        st = opt._state(p)
        snap["state"][id(p)] = (st["step_count"], st["exp_avg"].clone(), st["exp_avg_sq"].clone())
    return snap


def restore(tr, snap):
    """in place: the tensors keep their identity (MCMC at the cap relocates in place as well)"""
    import torch
    opt = tr.optimizer
    with torch.no_grad():
        for p, q in zip(tr.model.parameters(), snap["params"]):
            p.data.copy_(q)
            count, m, v = snap["state"][id(p)]
            st = opt._state(p)
            st["step_count"] = count
            st["exp_avg"].copy_(m)
            st["exp_avg_sq"].copy_(v)
    for g, lr in zip(opt.param_groups, snap["lr"]):
        g["lr"] = lr
    tr.iteration, tr.model.active_sh_degree = snap["iteration"], snap["degree"]
    if snap["gen"] is not None:
        tr.strategy.generator.set_state(snap["gen"])
    tr._gut_step.colors_for = None   # (the parameters were rewritten behind the step driver's back: colours a tail prepared are void)


def run_steps(tr, target, steps, config):
    """-> (seconds inside the timed windows, timed steps, set of step forms seen). Refining iterations are stepped outside the windows."""
    import torch
    forms = set()
    timed, count = 0.0, 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        st = tr.strategy
        if st is not None and st.is_refining(tr.iteration + 1):
            torch.cuda.synchronize()
            timed += time.perf_counter() - t0
            tr.train_step([target])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            continue
        tr.train_step([target])
        forms.add(tr.last_plan.path + ("+freeze" if tr.last_plan.freeze_shN else ""))
        count += 1
    torch.cuda.synchronize()
    timed += time.perf_counter() - t0
    return timed, count, forms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "one_call_options.json"))
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--configs", default="l1_ssim,l1_ssim_mcmc,mse_early")
    ap.add_argument("--only", default="", help="config:off|on - run that one form alone (no A/B, nothing written)")
    args = ap.parse_args()
    import torch

    import lichtfeld_studio_amd as lfs
    from lichtfeld_studio_amd import scenes
    dev = torch.device("cuda:0")
    scene = scenes.syn_b(n=args.n)
    target = scenes.target_image(scene.height, scene.width).to(dev)
    if args.only:
        config, form = args.only.split(":")
        tr = make_trainer(scene, dev, config, form == "on", args.n)
        run_steps(tr, target, args.warmup, config)
        sec, cnt, forms = run_steps(tr, target, args.steps, config)
        print(json.dumps({"config": config, "one_call": form == "on", "ms_per_step": 1e3 * sec / cnt, "forms": sorted(forms)}))
        return
    out = {"workload": f"SYN-B, {args.n} Gaussians, {scene.width}x{scene.height}, SH degree {scene.sh_degree}", "rounds": args.rounds, "steps_per_round": args.steps,
           "warmup_steps": args.warmup, "library": lfs.load_library().lfs_version().decode(), "device": torch.cuda.get_device_name(0), "configs": {}}
    for config in [c for c in args.configs.split(",") if c]:
        trainers = {"off": make_trainer(scene, dev, config, False, args.n), "on": make_trainer(scene, dev, config, True, args.n)}
        ms, forms = {"off": [], "on": []}, {"off": set(), "on": set()}
        snaps = {}
        for k, tr in trainers.items():
            run_steps(tr, target, args.warmup, config)
            snaps[k] = snapshot(tr)
        for _ in range(args.rounds):
            for k, tr in trainers.items():
                restore(tr, snaps[k])
                sec, cnt, seen = run_steps(tr, target, args.steps, config)
                ms[k].append(1e3 * sec / cnt)
                forms[k] |= seen
        res = {}
        for k in ("off", "on"):
            res[k] = {"ms_per_step_rounds": [round(x, 4) for x in ms[k]], "median_ms": round(statistics.median(ms[k]), 4), "spread_ms": round(max(ms[k]) - min(ms[k]), 4),
                      "img_per_s": round(1e3 / statistics.median(ms[k]), 1), "step_forms": sorted(forms[k]), "retries": trainers[k]._gut_step.retries,
                      "colour_launches_saved": trainers[k]._gut_step.colour_launches_saved}
        gain = res["off"]["median_ms"] - res["on"]["median_ms"]
        res["gain_ms"] = round(gain, 4)
        res["speed_up_accepted"] = bool(gain > res["off"]["spread_ms"])
        out["configs"][config] = res
        print(config, json.dumps(res), flush=True)
        del trainers, snaps
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
