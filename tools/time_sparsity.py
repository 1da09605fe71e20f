#!/usr/bin/env python3
"""Same-process A/B of the ADMM sparsity operators (csrc/sparsity.hip) against the reference's torch expression sequences (sparsity_optimizer.cpp) on the same
tensors, at SYN-B size (1 M Gaussians), and of a whole training step of the sparsification phase with the term on and off:

    state   lfs_admm_update                 |  sigmoid, + u, torch.sort, threshold, (v > thr) * v, u += opa - z        (update_state / prune_z, :83-86, :152-168)
    loss    lfs_admm_loss_grad (accumulate) |  sigmoid, - z, + u, norm, pow, * rho / 2, backward()                     (compute_loss :57-59 + trainer.cpp:713)
    step    GutTrainer(enable_sparsity) inside the phase  |  the same split step form (gradient tensors) without the term  |  the default form outside a phase

The torch forms are timed WITHOUT the host reads the reference wraps around them (`(z == 0).sum().item()`, `loss.item()`): device work against device work.
Per form `--rounds` rounds of `--reps` calls alternate (hip, torch, hip, torch, ...), each round synchronised at both ends; reported: the median over the rounds of
ms per call and the round-to-round spread (max - min). A HIP form counts as a speed-up only where its median beats the torch form's by more than the torch form's
own spread - the rule of tools/time_step_forms.py. One JSON document -> --out (default profiles/r08/sparsity.json).

    python tools/time_sparsity.py [--out FILE] [--n 1000000] [--rounds 7] [--reps 20] [--steps 100] [--warmup 20]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps


def ab(forms, rounds, reps, warmup=3):
    """forms: {name: callable} -> {name: {median_ms, spread_ms, rounds}}; the forms alternate within every round"""
    for fn in forms.values():
        timed(fn, warmup)
    ms = {k: [] for k in forms}
    for _ in range(rounds):
        for k, fn in forms.items():
            ms[k].append(timed(fn, reps))
    return {k: {"ms_rounds": [round(x, 4) for x in v], "median_ms": round(statistics.median(v), 4), "spread_ms": round(max(v) - min(v), 4)} for k, v in ms.items()}


def verdict(res, hip, torch_form):
    gain = res[torch_form]["median_ms"] - res[hip]["median_ms"]
    res["gain_ms"] = round(gain, 4)
    res["speed_up_accepted"] = bool(gain > res[torch_form]["spread_ms"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "sparsity.json"))
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--skip-step", action="store_true", help="operators only")
    args = ap.parse_args()
    import torch

    import lichtfeld_studio_amd as lfs
    from lichtfeld_studio_amd import scenes, sparsity
    from lichtfeld_studio_amd.trainer import GutTrainer
    dev = torch.device("cuda:0")
    scene = scenes.syn_b(n=args.n)
    N, rho, ratio = args.n, 0.0005, 0.6
    k = sparsity.num_to_prune(ratio, N)
    raw = scene.raw_opacities.to(dev).contiguous()
    out = {"workload": f"SYN-B, {N} Gaussians", "rounds": args.rounds, "reps_per_round": args.reps, "prune_ratio": ratio, "k": k,
           "library": lfs.load_library().lfs_version().decode(), "device": torch.cuda.get_device_name(0),
           "note": "torch forms without the reference's host reads ((z == 0).sum().item(), loss.item())"}

    # ---- state update ------------------------------------------------------------------------------------------------
    u_h, z_h = torch.zeros(N, device=dev), torch.empty(N, device=dev)
    st = {"u": torch.zeros(N, device=dev), "z": None}

    def state_hip():
        sparsity.admm_update(raw, u_h, z_h, k)

    def state_torch():
        with torch.no_grad():
            opa = torch.sigmoid(raw).detach().contiguous()
            v = opa + st["u"]
            thr = torch.sort(v.flatten(), 0)[0][k - 1]
            st["z"] = (v > thr) * v
            st["u"] += opa - st["z"]
    out["state"] = verdict(ab({"hip": state_hip, "torch": state_torch}, args.rounds, args.reps), "hip", "torch")
    print("state", json.dumps(out["state"]), flush=True)

    # ---- loss + gradient -----------------------------------------------------------------------------------------------
    z, u = z_h.clone(), u_h.clone()
    g_h, loss_h = torch.zeros(N, device=dev), torch.zeros(1, device=dev)
    raw_t = raw.clone().requires_grad_(True)
    raw_t.grad = torch.zeros_like(raw_t)

    def loss_hip():
        sparsity.admm_loss_grad(raw, z, u, rho, 1.0, g_h, True, loss_h)

    def loss_torch():
        opa = torch.sigmoid(raw_t)
        diff = opa - z.detach() + u.detach()
        loss = 0.5 * rho * torch.pow(torch.norm(diff, 2), 2)
        loss.backward()
    out["loss"] = verdict(ab({"hip": loss_hip, "torch": loss_torch}, args.rounds, args.reps), "hip", "torch")
    print("loss", json.dumps(out["loss"]), flush=True)

    # ---- the select alone against the sort alone ---------------------------------------------------------------------------
    x = (torch.sigmoid(raw) + u).contiguous()
    sel_out = torch.zeros(1, device=dev)
    out["select"] = verdict(ab({"hip": lambda: sparsity.select_kth(x, k, sel_out), "torch": lambda: torch.sort(x, 0)[0][k - 1]}, args.rounds, args.reps), "hip", "torch")
    print("select", json.dumps(out["select"]), flush=True)

    # ---- a whole step of the phase ---------------------------------------------------------------------------------------
    if not args.skip_step:
        target = scenes.target_image(scene.height, scene.width).to(dev)
        base = 3000
        on = GutTrainer(scene, dev, iterations=base, enable_sparsity=True, sparsify_steps=10 ** 9, sparsity_update_every=10 ** 8)
        off = GutTrainer(scene, dev, iterations=30000)
        off.inline_all_adam = False            # the step form the phase takes (gradient tensors), without the term
        default = GutTrainer(scene, dev, iterations=30000)
        trainers = {"term_on": on, "term_off_same_form": off, "default_form": default}
        for tr in trainers.values():
            tr.iteration = base
            for _ in range(args.warmup):
                tr.train_step([target])
        # every round starts from the state the trainer had after its warm-up (tools/time_step_forms.py: training changes the scene and with it the work per step)
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        from time_step_forms import restore, snapshot
        snaps = {name: snapshot(tr) for name, tr in trainers.items()}
        ms, forms = {name: [] for name in trainers}, {}
        for _ in range(args.rounds):
            for name, tr in trainers.items():
                restore(tr, snaps[name])
                ms[name].append(timed(lambda: tr.train_step([target]), args.steps))
                forms[name] = tr.last_plan.path
        res = {name: {"ms_per_step_rounds": [round(v, 4) for v in vals], "median_ms": round(statistics.median(vals), 4), "spread_ms": round(max(vals) - min(vals), 4),
                      "step_form": forms[name]} for name, vals in ms.items()}
        res["term_cost_ms"] = round(res["term_on"]["median_ms"] - res["term_off_same_form"]["median_ms"], 4)
        res["term_cost_resolved"] = bool(abs(res["term_cost_ms"]) > max(res["term_on"]["spread_ms"], res["term_off_same_form"]["spread_ms"]))
        res["phase_step_over_default_ms"] = round(res["term_on"]["median_ms"] - res["default_form"]["median_ms"], 4)
        out["step"] = res
        print("step", json.dumps(res), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
