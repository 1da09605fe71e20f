#!/usr/bin/env python3
"""Visible-only Adam against the dense kernel, in one process on one GPU (results: profiles/r17/visible_adam.json).

    python tools/bench_adam_visible.py --out visible_adam.json [--n 1000000] [--rounds 5] [--window-s 1.0] [--no-trainer]

Kernels: N Gaussians, SH degree 3, all six parameter groups (59 floats per Gaussian). Every round times, for each visible fraction (1.0, 0.5, 0.2, 0.05) and each
mask layout (iid bits; runs of 4096 consecutive Gaussians), a window of lfs_adam_step_multi launches and then a window of lfs_adam_step_multi_visible
launches between device events - the two forms alternate, so drift of the machine hits both. A warm-up and a pilot window per form and mask before the first
round size every window to about --window-s seconds of device time. Reported per configuration: the median over the rounds of the time per launch and the round-to-round spread (max - min) / median, the
bytes model 1652 |V| + N / 8 beside the dense 1652 N, and the visible form's time over (dense time x bytes ratio).

Trainer: a scene of five clusters with one camera in front of each (a view sees a fifth of the Gaussians), 1080p, MSE, no strategy, iteration > 1000: the fastgs
step of GutTrainer as it is by default (shN's Adam inside the SH backward), with that fusion off (all six groups through lfs_adam_step_multi), and with
visible_adam=True, alternating, timed on the host around a device synchronise."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEV = "cuda:0"
FRACTIONS = [1.0, 0.5, 0.2, 0.05]
BYTES_PER_GAUSSIAN = 59 * 28     # 16 B read + 12 B written per element


def pack(mask: torch.Tensor) -> torch.Tensor:
    """bool [N] (device) -> int32 [ceil(N / 32)], bit i of word i // 32"""
    N = mask.shape[0]
    words = (N + 31) // 32
    padded = torch.zeros(words * 32, dtype=torch.int64, device=mask.device)
    padded[:N] = mask.to(torch.int64)
    w = (padded.view(words, 32) << torch.arange(32, device=mask.device)).sum(1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def masks_for(N: int, fraction: float, gen: torch.Generator) -> dict:
    iid = torch.rand(N, generator=gen) < fraction
    runs = (torch.rand((N + 4095) // 4096, generator=gen) < fraction).repeat_interleave(4096)[:N]
    if fraction >= 1.0:
        iid[:], runs[:] = True, True
    return {"iid": iid.to(DEV), "runs4096": runs.to(DEV)}


def spread(xs):
    return (max(xs) - min(xs)) / statistics.median(xs)


def bench_kernels(N: int, rounds: int, window_s: float) -> dict:
    from lichtfeld_studio_amd import ops
    gen = torch.Generator().manual_seed(0)
    shapes = [(N, 3), (N, 1, 3), (N, 15, 3), (N, 3), (N, 4), (N,)]
    lrs = [1.6e-4, 2.5e-3, 1.25e-4, 5e-3, 1e-3, 5e-2]
    mk = lambda s: [(torch.randn(sh, device=DEV) * s) for sh in shapes]
    torch.manual_seed(0)
    p, m, v, g = mk(1.0), [x.abs() for x in mk(0.1)], [x.abs() for x in mk(0.01)], mk(1e-3)
    bc = (1 / (1 - 0.9 ** 1000), 1 / math.sqrt(1 - 0.999 ** 1000))
    entries = [(p[i], m[i], v[i], g[i], lrs[i], 0.9, 0.999, 1e-15, *bc) for i in range(6)]
    configs = []
    for f in FRACTIONS:
        for layout, mask in masks_for(N, f, gen).items():
            configs.append({"fraction": f, "layout": layout, "visible": int(mask.sum()), "bits": pack(mask)})

    def window(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps

    dense = lambda: ops.adam_step_multi(entries)
    for c in configs:       # warm-up: every form on every mask
        c["fn"] = (lambda bits: (lambda: ops.adam_step_multi_visible(entries, bits, N)))(c["bits"])
        for _ in range(3):
            dense(); c["fn"]()
        c["dense_ms"], c["visible_ms"] = [], []
        c["reps"] = max(50, int(math.ceil(window_s * 1e3 / window(c["fn"], 50))))
    dense_reps = max(50, int(math.ceil(window_s * 1e3 / window(dense, 50))))
    torch.cuda.synchronize()
    for _ in range(rounds):
        for c in configs:
            c["dense_ms"].append(window(dense, dense_reps))
            c["visible_ms"].append(window(c["fn"], c["reps"]))
    all_dense = [x for c in configs for x in c["dense_ms"]]
    dense_bytes = BYTES_PER_GAUSSIAN * N
    out = {"N": N, "floats_per_gaussian": 59, "rounds": rounds, "window_s": window_s, "dense_launches_per_window": dense_reps,
           "dense": {"ms_median": statistics.median(all_dense), "spread": spread(all_dense), "bytes": dense_bytes,
                     "GBps": dense_bytes / statistics.median(all_dense) / 1e6, "windows": len(all_dense)},
           "visible": []}
    for c in configs:
        d, w = statistics.median(c["dense_ms"]), statistics.median(c["visible_ms"])
        model = BYTES_PER_GAUSSIAN * c["visible"] + N // 8
        out["visible"].append({"fraction": c["fraction"], "layout": c["layout"], "visible_gaussians": c["visible"], "launches_per_window": c["reps"], "ms_median": w, "spread": spread(c["visible_ms"]),
                               "dense_ms_median_same_rounds": d, "dense_spread_same_rounds": spread(c["dense_ms"]), "time_over_dense": w / d, "ms_per_round": c["visible_ms"], "dense_ms_per_round": c["dense_ms"],
                               "bytes_model": model, "bytes_model_over_dense": model / dense_bytes, "time_over_bytes_model": (w / d) / (model / dense_bytes),
                               "GBps_of_model_bytes": model / w / 1e6})
        print(json.dumps(out["visible"][-1]), flush=True)
    print(json.dumps(out["dense"]), flush=True)
    return out


def five_cluster_scene(n: int, width: int = 1920, height: int = 1080, focal: float = 1200.0):
    """scenes.syn_b's Gaussians in five boxes 100 units apart along x, one camera 10 units in front of each box"""
    import dataclasses
    from lichtfeld_studio_amd import scenes
    sc = scenes._syn_box("five-clusters", 42, n, width, height, focal, 5)
    means = sc.means.clone()
    means[:, 0] += 100.0 * (torch.arange(n) % 5)
    viewmats = torch.stack([scenes.look_at_viewmat((100.0 * c, 0.0, -10.0), (100.0 * c, 0.0, 0.0)) for c in range(5)], 0)
    return dataclasses.replace(sc, means=means, viewmats=viewmats)


def bench_trainer(n: int, rounds: int, steps: int) -> dict:
    from lichtfeld_studio_amd.trainer import GutTrainer
    sc = five_cluster_scene(n)
    gen = torch.Generator().manual_seed(1)
    targets = [(torch.rand(3, sc.height, sc.width, generator=gen) * 0.7).to(DEV) for _ in range(5)]
    forms = {"default (shN's Adam inside the SH backward)": {}, "separate optimizer (lfs_adam_step_multi over six groups)": {"inline": False},
             "visible_adam": {"visible_adam": True}}
    trainers, times = {}, {}
    for name, kw in forms.items():
        tr = GutTrainer(sc, torch.device(DEV), iterations=30000, rasterizer="fastgs", visible_adam=kw.get("visible_adam", False))
        tr.inline_shN_adam = kw.get("inline", True)
        tr.iteration = 1500
        trainers[name], times[name] = tr, []

    def run(tr, k0, count):
        for k in range(k0, k0 + count):
            tr.train_step([targets[k % 5]], views=[k % 5])
        torch.cuda.synchronize()

    k = 0
    for tr in trainers.values():
        run(tr, 0, 10)
    k = 10
    for _ in range(rounds):
        for name, tr in trainers.items():
            t0 = time.perf_counter()
            run(tr, k, steps)
            times[name].append((time.perf_counter() - t0) * 1e3 / steps)
        k += steps
    vis = trainers["visible_adam"]
    bits = vis._vis_bits.to(torch.int64) & 0xFFFFFFFF
    seen = int(sum(bin(int(w)).count("1") for w in bits.cpu().tolist()))
    out = {"scene": f"{n} Gaussians in five clusters, one camera per cluster, {sc.width} x {sc.height}, SH degree 3, MSE, no strategy, iteration > 1000",
           "visible_fraction_of_the_last_view": seen / n, "steps_per_window": steps, "rounds": rounds, "step_ms": {}}
    for name, xs in times.items():
        out["step_ms"][name] = {"median": statistics.median(xs), "spread": spread(xs), "per_round": xs}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=1.0, help="device time of one timed window")
    ap.add_argument("--trainer-steps", type=int, default=800, help="training steps per timed window")
    ap.add_argument("--no-trainer", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_adam_visible.py measures on the GPU: no device found")
    result = {"device": torch.cuda.get_device_name(0), "kernels": bench_kernels(args.n, args.rounds, args.window_s)}
    if not args.no_trainer:
        result["trainer"] = bench_trainer(args.n, args.rounds, args.trainer_steps)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
