#!/usr/bin/env python3
"""Same-process timing of the scene transform at --n Gaussians (default 1 M), SH degree 3 - the method of tools/time_fastgs_filter3d.py: after a
warm-up of every form, `--rounds` rounds alternate between them; per form the median over the rounds and the round-to-round spread (max - min) of the time of ONE
call (a window of --calls calls between device events):

  hip_out_of_place   lfs_splat_transform_apply into fresh buffers (236 B in, 236 B out per Gaussian)
  hip_in_place       the same with every output == its input
  torch              the equivalent torch sequence on the same tensors: a matmul for the means, the reference's quaternion expression
                     (src/core/splat_data.cpp:356-359), raw_scales + log s, one einsum per band per the [N, K, 3] layout, the results gathered into one shN tensor
  copy               device-to-device copies of the same four tensors (2 x 236 B per Gaussian): the streaming bound of the pass

The acceptance rule (ISSUE: scene transform): hip is faster than torch by more than torch's own round-to-round spread. hip / copy is reported as the distance from the
streaming bound, whatever it is; the bytes per second of every form are computed from the shapes.

    python tools/time_splat_transform.py [--out profiles/r19/splat_transform.json] [--rounds 9] [--calls 20] [--warmup 5] [--n 1000000]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19", "splat_transform.json"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n", type=int, default=1_000_000)
    args = ap.parse_args()
    import numpy as np
    import torch

    import lichtfeld_studio_amd as lfs  # noqa: F401
    from lichtfeld_studio_amd import transform
    if not torch.cuda.is_available():
        raise SystemExit("time_splat_transform.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    N, deg, rows = args.n, 3, 15
    g = torch.Generator(device=dev); g.manual_seed(0)
    means = torch.randn((N, 3), device=dev, generator=g) * 10
    quats = torch.randn((N, 4), device=dev, generator=g)
    scales = torch.randn((N, 3), device=dev, generator=g)
    shN = torch.randn((N, rows, 3), device=dev, generator=g)
    ins = (means, quats, scales, shN)
    outs = tuple(torch.empty_like(t) for t in ins)
    work = tuple(t.clone() for t in ins)                      # the in-place form runs on its own copies (a rotation applied over and over stays bounded)
    w, x, y, z = 0.51, -0.37, 0.64, 0.44
    n = (w * w + x * x + y * y + z * z) ** 0.5
    w, x, y, z = w / n, x / n, y / n, z / n
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    xf = transform.similarity(rotation=R, scale=1.0, translation=[0.5, -1.0, 0.25])
    rec = xf.record(deg)
    sR = torch.tensor(list(rec.sR), device=dev).reshape(3, 3)
    t = torch.tensor(list(rec.t), device=dev)
    q = [float(v) for v in rec.q]
    log_s = float(rec.log_s)
    mats = [torch.tensor(list(getattr(rec, f"m{l}")), device=dev).reshape(2 * l + 1, 2 * l + 1) for l in (1, 2, 3)]

    def hip_out():
        transform.apply(xf, deg, *ins, out=outs)

    def hip_in():
        transform.apply(xf, deg, *work, out="inplace")

    def torch_seq():
        m2 = means @ sR.T + t
        w2, x2, y2, z2 = quats.unbind(1)
        w1, x1, y1, z1 = q
        q2 = torch.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                          w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], 1)
        s2 = scales + log_s
        h2 = torch.cat([torch.einsum("ik,nkc->nic", M, shN[:, l * l - 1:(l + 1) ** 2 - 1, :]) for l, M in enumerate(mats, 1)], 1)
        return m2, q2, s2, h2

    def copy():
        for o, i in zip(outs, ins):
            o.copy_(i)

    forms = {"hip_out_of_place": hip_out, "hip_in_place": hip_in, "torch": torch_seq, "copy": copy}

    # the forms agree before anything is timed (torch's matmul / einsum may fuse and reorder: rounding, not bits)
    hip_out()
    ref = torch_seq()
    for a, b, name in zip(outs, ref, ("means", "quats", "raw_scales", "shN")):
        err = float((a - b).abs().max())
        assert err <= 1e-4 * float(b.abs().max()), (name, err)

    def window(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / args.calls   # us per call

    for fn in forms.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in forms}
    for _ in range(args.rounds):
        for k, fn in forms.items():
            samples[k].append(window(fn))
    bytes_moved = 2 * N * (3 + 4 + 3 + 3 * rows) * 4
    out = {"n": N, "sh_degree": deg, "rounds": args.rounds, "calls_per_window": args.calls, "bytes_per_call": bytes_moved, "device": torch.cuda.get_device_name(0), "forms": {}}
    for k, v in samples.items():
        med = statistics.median(v)
        out["forms"][k] = {"median_us": round(med, 2), "spread_us": round(max(v) - min(v), 2), "min_us": round(min(v), 2), "tb_per_s": round(bytes_moved / med / 1e6, 3),
                           "samples_us": [round(s, 2) for s in v]}
    f = out["forms"]
    slower = max(f["hip_out_of_place"]["median_us"], f["hip_in_place"]["median_us"])
    out["torch_over_hip_out_of_place"] = round(f["torch"]["median_us"] / f["hip_out_of_place"]["median_us"], 3)
    out["hip_out_of_place_over_copy"] = round(f["hip_out_of_place"]["median_us"] / f["copy"]["median_us"], 3)
    out["hip_in_place_over_copy"] = round(f["hip_in_place"]["median_us"] / f["copy"]["median_us"], 3)
    out["accepted"] = bool(f["torch"]["median_us"] - slower > f["torch"]["spread_us"])
    out["rule"] = "torch median - hip median (the slower of the two forms) > torch's round-to-round spread"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "forms"} | {k: (v["median_us"], v["spread_us"]) for k, v in f.items()}))


if __name__ == "__main__":
    main()
