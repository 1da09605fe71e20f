#!/usr/bin/env python
"""SOG export on one MI355X, on record (no threshold): -> profiles/r08/sog_export.json

    python tools/time_sog_export.py [--n 1000000] [--runs 5] [--warmup 2] [--iterations 10] [--out profiles/r08/sog_export.json]

  * lfs_kmeans_assign alone at k = 65 536, D = 45 (hipEvent timing, median of --runs after --warmup): ms, TFLOP/s on the 2 N k D useful flops and the
    fraction of the 155 TF f32-matrix peak; the same for a chunked torch baseline in the same process, (x @ c^T - |c|^2 / 2).argmax(1), and how many labels agree;
  * write_sog end to end (wall clock: most of it is host work - quantisation, WebP) at palette 64 and at 65 536, the bundle's size against the PLY's;
  * one 256 x 256 fastgs view of the model before and after a SOG round trip and the PSNR between the two, at both palette sizes.
The model is SYN-B (scenes.syn_b: 1 M Gaussians, SH degree 3, random coefficients - no structure for a palette to find, so the PSNR is a floor, not a typical value)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

PEAK_F32_MATRIX_TF = 155.0


def _event_ms(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=65536)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "sog_export.json"))
    args = ap.parse_args()

    import lichtfeld_studio_amd  # noqa: F401
    from lichtfeld_studio_amd import evaluate, loader, scenes, sog
    from lichtfeld_studio_amd.fastgs import fast_rasterize
    from lichtfeld_studio_amd.rasterizer import Camera, SplatModel

    dev = torch.device("cuda:0")
    sc = scenes.syn_b(n=args.n, n_views=4).to(dev)
    model = SplatModel(sc.means, sc.sh0, sc.shN, sc.raw_scales, sc.raw_quats, sc.raw_opacities, sc.sh_degree)
    N, D, k = args.n, 45, min(args.k, args.n)
    res = {"device": torch.cuda.get_device_name(0), "N": N, "D": D, "k": k, "runs": args.runs, "warmup": args.warmup, "iterations": args.iterations,
           "timing": "hipEvent pairs around the call, median; write_sog: wall clock around the call, median"}

    # ---- the assignment alone ---------------------------------------------------------------------------------------------------
    x = sc.shN.reshape(N, D).contiguous()
    cen = x[torch.randperm(N, generator=torch.Generator().manual_seed(0))[:k].to(dev)].clone()
    flop = 2.0 * N * k * D
    ms = _event_ms(lambda: sog.kmeans_assign(x, cen), args.runs, args.warmup)
    hip_labels = sog.kmeans_assign(x, cen)
    res["assign_hip"] = {"ms": ms, "median_ms": statistics.median(ms), "tflops": flop / statistics.median(ms) / 1e9,
                         "fraction_of_155TF": flop / statistics.median(ms) / 1e9 / PEAK_F32_MATRIX_TF,
                         "tflops_padded_D48": flop * 48 / 45 / statistics.median(ms) / 1e9}
    print(json.dumps({"assign_hip": res["assign_hip"]}), flush=True)

    chunk = 16384
    half = -0.5 * (cen * cen).sum(1)

    def torch_assign():
        out = torch.empty(N, dtype=torch.int64, device=dev)
        for s in range(0, N, chunk):
            out[s:s + chunk] = torch.addmm(half, x[s:s + chunk], cen.t()).argmax(1)
        return out
    ms = _event_ms(torch_assign, args.runs, args.warmup)
    torch_labels = torch_assign()
    res["assign_torch"] = {"ms": ms, "median_ms": statistics.median(ms), "tflops": flop / statistics.median(ms) / 1e9, "chunk": chunk,
                           "expression": "addmm(-|c|^2/2, x, c^T).argmax(1)", "labels_equal_to_hip": float((torch_labels == hip_labels.long()).float().mean())}
    print(json.dumps({"assign_torch": res["assign_torch"]}), flush=True)
    del torch_labels, hip_labels, cen, x

    # ---- the export end to end, the sizes, the round-trip render -----------------------------------------------------------------------
    cam = Camera(sc.viewmats[:1].contiguous(), torch.tensor([[[300.0, 0, 128], [0, 300.0, 128], [0, 0, 1]]], device=dev), 256, 256)
    bg = torch.zeros(3, device=dev)
    with torch.no_grad():
        before = torch.clamp(fast_rasterize(cam, model, bg).image, 0, 1).clone()
    with tempfile.TemporaryDirectory() as tmp:
        ply = os.path.join(tmp, "splat.ply")
        loader.save_ply(model, ply)
        res["ply_bytes"] = os.path.getsize(ply)
        for palette in (64, k):
            path = os.path.join(tmp, f"splat_{palette}.sog")
            wall = []
            for i in range(args.warmup + args.runs):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                loader.save_sog(model, path, iterations=args.iterations, palette_size=palette)
                torch.cuda.synchronize()
                if i >= args.warmup:
                    wall.append(time.perf_counter() - t0)
                print(json.dumps({"palette": palette, "write_sog_s": time.perf_counter() - t0}), flush=True)
            back = loader.load_sog(path, dev)
            with torch.no_grad():
                after = torch.clamp(fast_rasterize(cam, back, bg).image, 0, 1)
            res[f"palette_{palette}"] = {"write_sog_s": wall, "median_s": statistics.median(wall), "sog_bytes": os.path.getsize(path),
                                         "sog_over_ply": os.path.getsize(path) / res["ply_bytes"], "round_trip_psnr_256x256_fastgs": evaluate.psnr(after, before)}
            print(json.dumps({f"palette_{palette}": res[f"palette_{palette}"]}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
