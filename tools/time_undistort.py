#!/usr/bin/env python3
"""Same-process A/B of the plain image resample (lfs_image_u8_to_chw_f32, csrc/dataprep.hip) and the undistorting one (lfs_image_undistort_u8_to_chw_f32,
csrc/undistort.hip) at 1920 x 1080 -> 1920 x 1080 and 3840 x 2160 -> 1920 x 1080 - the method of tools/time_masked_loss.py: after a warm-up of each form, `--rounds`
rounds of `--calls` calls alternate between the forms, each round between two device events with a synchronise at both ends. Per form: the median over the rounds of
us / call and the round-to-round spread (max - min). Recorded, not gated: this is a once-per-image cost. Both kernels write 3 * 4 + (1) bytes per destination pixel
and read at most 4 texels of 3 bytes; the undistorting one adds the lens model (a few dozen VALU operations per pixel, its coefficients in SGPRs).

    python tools/time_undistort.py [--out profiles/r15/undistort.json] [--rounds 7] [--calls 2000] [--warmup 200]

An existing --out file is extended (the end-to-end PSNR figures of tests/test_gpu_undistort.py live in the same file), not replaced.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "undistort.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    args = ap.parse_args()
    import numpy as np
    import torch

    import lichtfeld_studio_amd as lfs
    from lichtfeld_studio_amd import loader, undistort
    if not torch.cuda.is_available():
        raise SystemExit("time_undistort.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    forms = {}
    for name, (sw, sh), (dw, dh) in [("1080p_to_1080p", (1920, 1080), (1920, 1080)), ("4k_to_1080p", (3840, 2160), (1920, 1080))]:
        src = (torch.rand(sh, sw, 3, generator=g) * 256).to(torch.uint8).to(dev)
        cam = loader.CameraData(1, 4, 0, sw, sh, 0.8 * sw, 0.8 * sw, 0.5 * sw, 0.5 * sh, np.eye(3, dtype=np.float32), np.zeros(3, np.float32),
                                np.asarray([-0.25, 0.08], np.float32), np.asarray([0.004, -0.003], np.float32), np.zeros(0, np.float32), "t.png", "")
        m = undistort.undistorted_camera(cam, sw, sh, dw, dh, 0.0)
        forms[f"plain_{name}"] = lambda src=src, dw=dw, dh=dh: loader.u8_to_chw_f32(src, dw, dh)
        forms[f"undistort_{name}"] = lambda src=src, m=m: loader.undistort_u8_to_chw_f32(src, m)

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
    timing = {"rounds": args.rounds, "calls_per_round": args.calls, "warmup_calls": args.warmup, "library": lfs.load_library().lfs_version().decode(),
              "device": torch.cuda.get_device_name(0), "unit": "us per call (one launch and its output allocations, OPENCV model k1 k2 p1 p2 = -0.25 0.08 0.004 -0.003)",
              "forms": {}}
    for k, v in us.items():
        timing["forms"][k] = {"us_rounds": [round(x, 2) for x in v], "median_us": round(statistics.median(v), 2), "spread_us": round(max(v) - min(v), 2)}
    out = {}
    if os.path.exists(args.out):
        with open(args.out) as fh:
            out = json.load(fh)
    out["timing"] = timing
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(timing))


if __name__ == "__main__":
    main()
