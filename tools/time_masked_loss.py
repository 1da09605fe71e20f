#!/usr/bin/env python3
"""Same-process A/B of the unmasked and the masked L1 + D-SSIM entry (lfs_photometric_loss_ex_fwd_bwd | lfs_photometric_loss_masked_fwd_bwd, csrc/ssim.hip) at
1920 x 1080, and the time of lfs_mask_prepare from a 4K (3840 x 2160) source - the method of tools/time_step_forms.py: after a warm-up of each form, `--rounds`
rounds of `--calls` calls alternate between the forms (unmasked, masked, masked + alpha, unmasked, ...), each round between two device events with a synchronise at
both ends. Per form: the median over the rounds of us / call and the round-to-round spread (max - min). Recorded, not gated. The mask adds H * W bytes read in each
of the two launches, which move 3 * 3 * H * W * 4 bytes of derivative maps each way: the masked entry is expected within the unmasked entry's own spread.

    python tools/time_masked_loss.py [--out profiles/r09/masked_loss.json] [--rounds 7] [--calls 200] [--warmup 50]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09", "masked_loss.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    args = ap.parse_args()
    import torch

    import lichtfeld_studio_amd as lfs
    from lichtfeld_studio_amd import losses
    if not torch.cuda.is_available():
        raise SystemExit("time_masked_loss.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    H, W = args.height, args.width
    g = torch.Generator().manual_seed(0)
    render = (torch.rand(H, W, 3, generator=g) * 1.4 - 0.2).to(dev)
    target = torch.rand(3, H, W, generator=g).to(dev)
    alpha = torch.rand(H, W, generator=g).to(dev)
    src = (torch.rand(2160, 3840, generator=g) * 256).to(torch.uint8).to(dev)
    mask = losses.prepare_mask(src, W, H)
    loss = torch.zeros(1, device=dev)

    forms = {
        "unmasked": lambda: losses.loss_fwd_bwd("l1_ssim", render, target, 1.0, loss, chw=False, clamp=True),
        "masked": lambda: losses.loss_fwd_bwd("l1_ssim", render, target, 1.0, loss, chw=False, clamp=True, mask=mask),
        "masked_alpha": lambda: losses.loss_fwd_bwd("l1_ssim", render, target, 1.0, loss, chw=False, clamp=True, mask=mask, alpha=alpha, alpha_weight=1.0),
        "mask_prepare_4k_to_1080p": lambda: losses.prepare_mask(src, W, H),
    }

    def window(fn, calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        return 1e3 * a.elapsed_time(b) / calls   # us per call

    for fn in forms.values():
        window(fn, args.warmup)
    us = {k: [] for k in forms}
    for _ in range(args.rounds):
        for k, fn in forms.items():
            us[k].append(window(fn, args.calls))
    out = {"shape": [H, W], "mask_source": [2160, 3840], "rounds": args.rounds, "calls_per_round": args.calls, "warmup_calls": args.warmup,
           "library": lfs.load_library().lfs_version().decode(), "device": torch.cuda.get_device_name(0), "unit": "us per call (two launches; mask_prepare: memset + one)",
           "mask_bytes_per_launch": H * W, "map_bytes_per_launch": 3 * 3 * H * W * 4, "forms": {}}
    for k, v in us.items():
        out["forms"][k] = {"us_rounds": [round(x, 2) for x in v], "median_us": round(statistics.median(v), 2), "spread_us": round(max(v) - min(v), 2)}
    f = out["forms"]
    out["masked_minus_unmasked_us"] = round(f["masked"]["median_us"] - f["unmasked"]["median_us"], 2)
    out["within_unmasked_spread"] = bool(abs(out["masked_minus_unmasked_us"]) <= f["unmasked"]["spread_us"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
