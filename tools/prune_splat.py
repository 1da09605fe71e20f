#!/usr/bin/env python
"""Prune a trained splat by what its Gaussians contribute to the training images (lichtfeld-studio_amd/contribution.py):

    python tools/prune_splat.py -d /data/garden --images images_4 --ply out/garden/splat_30000.ply --out out/garden/pruned --threshold 0.01 [--save-sog]
    python tools/prune_splat.py -d /data/garden --images images_4 --ply out/garden/splat_30000.ply --out out/garden/pruned --keep 1000000

Loads the PLY and the COLMAP scene, computes every Gaussian's blending-weight statistic over the training views on one MI355X, removes the Gaussians whose maximum
weight over all training rays is below --threshold (RadSplat: 0.01) or keeps the --keep Gaussians of largest summed weight, and writes <out>.ply (and <out>.sog).
Prints one JSON line: N before and after and the PSNR on the training views before and after. The statistic follows the image: a Gaussian that only ever TERMINATES
pixels counts as 0, and without it those pixels run on - the PSNR change printed here is that effect; a few hundred training iterations heal it
(tools/train_colmap.py --contribution-prune-at prunes inside the run instead). All views must share one image size. The file is rendered as it is: a PLY written with
the 3D filter baked in needs no filter here."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    ap.add_argument("-d", "--data-path", required=True, help="COLMAP directory of the scene the splat was trained on")
    ap.add_argument("--ply", required=True, help="the trained splat")
    ap.add_argument("--out", required=True, help="output path; .ply (and .sog) is appended when missing")
    ap.add_argument("--threshold", type=float, default=None, help="remove the Gaussians whose maximum blending weight over all training rays is below this (RadSplat: 0.01)")
    ap.add_argument("--keep", type=int, default=None, help="keep this many Gaussians, those of largest summed blending weight")
    ap.add_argument("--images", default="images")
    ap.add_argument("--test-every", type=int, default=8, help="with --eval-split: every N-th view is held out and takes no part in the statistic")
    ap.add_argument("--eval-split", action="store_true", help="the splat was trained with --eval: use the training views only")
    ap.add_argument("--resize-factor", type=int, default=-1)
    ap.add_argument("--max-width", type=int, default=0)
    ap.add_argument("--text", action="store_true", help="COLMAP text files")
    ap.add_argument("--antialiasing", action="store_true", help="the splat was trained in the antialiased mode: statistic and PSNR renders run in it")
    ap.add_argument("--save-sog", action="store_true", help="also write the compressed .sog bundle")
    ap.add_argument("--sog-iterations", type=int, default=10)
    return ap


def check_args(args) -> None:
    """what the tool refuses, before anything is loaded"""
    if (args.threshold is None) == (args.keep is None):
        raise SystemExit("exactly one of --threshold and --keep is needed")
    if args.threshold is not None and not 0.0 < args.threshold < 1.0:
        raise SystemExit("--threshold must lie in (0, 1): it is compared with a blending weight")
    if args.keep is not None and args.keep < 1:
        raise SystemExit("--keep must be >= 1")
    if not args.ply.lower().endswith(".ply"):
        raise SystemExit("--ply must name a .ply file")


def main():
    args = build_parser().parse_args()
    check_args(args)

    import torch

    import lichtfeld_studio_amd  # noqa: F401
    from lichtfeld_studio_amd import contribution, evaluate, loader
    from lichtfeld_studio_amd.rasterizer import Camera, SplatModel

    dev = torch.device("cuda:0")
    model = loader.load_ply(args.ply, device=dev)
    scene, ds, _ = loader.colmap_scene(args.data_path, args.images, split="train" if args.eval_split else "all", test_every=args.test_every, resize_factor=args.resize_factor,
                                       max_width=args.max_width, text=args.text, device=dev)
    targets = loader.preload(ds, dev)
    cameras = [Camera(scene.viewmats[v:v + 1].contiguous(), scene.Ks[v:v + 1].contiguous(), scene.width, scene.height) for v in range(len(ds))]
    n_before = int(model.means.shape[0])
    psnr_before = evaluate.evaluate(model, cameras, targets, antialiased=args.antialiasing).psnr
    torch.cuda.synchronize(); t0 = time.time()
    stats = contribution.compute_contribution(model, cameras, antialiased=args.antialiasing)
    mask = contribution.prune_mask(stats, threshold=args.threshold) if args.threshold is not None else contribution.prune_mask(stats, keep=args.keep)
    torch.cuda.synchronize(); seconds = time.time() - t0
    keep = mask.logical_not().nonzero().squeeze(-1)
    with torch.no_grad():
        pruned = SplatModel(*[p.detach().index_select(0, keep).contiguous() for p in model.parameters()], model.max_sh_degree, model.active_sh_degree)
    psnr_after = evaluate.evaluate(pruned, cameras, targets, antialiased=args.antialiasing).psnr
    base = args.out[:-4] if args.out.lower().endswith(".ply") else args.out
    os.makedirs(os.path.dirname(os.path.abspath(base)), exist_ok=True)
    loader.save_ply(pruned, base + ".ply")
    out = {"n_before": n_before, "n_after": int(keep.numel()), "never_blended": int((stats.max_w == 0).sum()), "views": stats.views,
           "rule": {"threshold": args.threshold} if args.threshold is not None else {"keep": args.keep},
           "psnr_train_views_before": round(psnr_before, 4), "psnr_train_views_after": round(psnr_after, 4), "statistic_seconds": round(seconds, 3), "ply": base + ".ply",
           "ply_bytes": os.path.getsize(base + ".ply")}
    if args.save_sog:
        loader.save_sog(pruned, base + ".sog", iterations=args.sog_iterations)
        out.update(sog=base + ".sog", sog_bytes=os.path.getsize(base + ".sog"))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
