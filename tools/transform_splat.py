#!/usr/bin/env python
"""Move a trained splat by a similarity and / or cut it to a box (lichtfeld-studio_amd/transform.py):

    python tools/transform_splat.py --ply splat.ply --out upright --rotate x -90 --translate 0 0 1.2 [--save-sog]
    python tools/transform_splat.py --sog scene.sog --out half --scale 0.5 --crop-min -1 -1 0 --crop-max 1 1 2
    python tools/transform_splat.py --ply splat.ply --out moved --matrix m00 m01 ... m33 -d /data/garden --images images_4

The transform is --matrix (16 numbers, row-major, x' = s R x + t) OR any of --rotate AXIS DEG / --scale S / --translate X Y Z, each repeatable; they are applied
in the order they stand on the command line. Means, orientations, log-scales and every SH band the file holds are moved (the view-dependent colour turns with the
scene). --crop-min / --crop-max name a box in the OUTPUT frame; the Gaussians whose mean lies in it are kept (--crop-invert: those outside). Writes <out>.ply (and
<out>.sog with --save-sog) and prints one JSON line. With -d COLMAP_DIR the line also holds the PSNR on the training views before the move and after it with the
cameras moved along (transform_cameras): a similarity leaves it unchanged up to rounding; a crop changes it by what was cut away. Non-uniform scale, shear and
reflections are refused."""
import argparse
import json
import math
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class _Op(argparse.Action):
    """--rotate / --scale / --translate go into ONE list, so that their order on the command line survives"""

    def __call__(self, parser, namespace, values, option_string=None):
        ops = list(getattr(namespace, "ops", None) or [])
        ops.append((self.dest, values))
        namespace.ops = ops


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ply", default=None, help="the splat, as a PLY")
    ap.add_argument("--sog", default=None, help="the splat, as a .sog bundle")
    ap.add_argument("--out", required=True, help="output path; .ply (and .sog) is appended when missing")
    ap.add_argument("--matrix", type=float, nargs=16, default=None, help="row-major 4x4 similarity")
    ap.add_argument("--rotate", nargs=2, action=_Op, metavar=("AXIS", "DEG"), help="rotation about x, y or z by DEG degrees (repeatable)")
    ap.add_argument("--scale", nargs=1, action=_Op, metavar="S", help="uniform scale (repeatable)")
    ap.add_argument("--translate", nargs=3, action=_Op, metavar=("X", "Y", "Z"), help="translation (repeatable)")
    ap.add_argument("--crop-min", type=float, nargs=3, default=None, help="box minimum, in the output frame")
    ap.add_argument("--crop-max", type=float, nargs=3, default=None, help="box maximum, in the output frame")
    ap.add_argument("--crop-invert", action="store_true", help="keep what lies OUTSIDE the box")
    ap.add_argument("--save-sog", action="store_true", help="also write the compressed .sog bundle")
    ap.add_argument("--sog-iterations", type=int, default=10)
    ap.add_argument("-d", "--data-path", default=None, help="COLMAP directory of the scene the splat was trained on: print the PSNR on its views before and after")
    ap.add_argument("--images", default="images")
    ap.add_argument("--resize-factor", type=int, default=-1)
    ap.add_argument("--max-width", type=int, default=0)
    ap.add_argument("--text", action="store_true", help="COLMAP text files")
    ap.add_argument("--antialiasing", action="store_true", help="the splat was trained in the antialiased mode: the PSNR renders run in it")
    ap.set_defaults(ops=None)
    ap._negative_number_matcher = re.compile(r"^-(\d+\.?\d*|\.\d+)([eE][-+]?\d+)?$")   # -1e-05 is a number, not an option (argparse knows -1 and -.5 only)
    return ap


def _number(text, what):
    try:
        v = float(text)
    except ValueError:
        raise SystemExit(f"{what}: {text!r} is not a number")
    if not math.isfinite(v):
        raise SystemExit(f"{what} must be finite")
    return v


def _matmul4(a, b):
    return [[sum(a[i][k] * b[k][j] for k in range(4)) for j in range(4)] for i in range(4)]


def matrix_of(args):
    """the 4x4 (nested lists, float64) the arguments ask for, or None: --matrix, or the --rotate / --scale / --translate operations composed in command-line order"""
    if args.matrix is not None:
        return [list(args.matrix[4 * i:4 * i + 4]) for i in range(4)]
    if not args.ops:
        return None
    m = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    for kind, vals in args.ops:
        op = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
        if kind == "rotate":
            a = math.radians(_number(vals[1], "--rotate DEG"))
            c, s = math.cos(a), math.sin(a)
            i, j = {"x": (1, 2), "y": (2, 0), "z": (0, 1)}[vals[0].lower()]
            op[i][i], op[i][j], op[j][i], op[j][j] = c, -s, s, c
        elif kind == "scale":
            for i in range(3):
                op[i][i] = _number(vals[0], "--scale")
        else:
            for i in range(3):
                op[i][3] = _number(vals[i], "--translate")
        m = _matmul4(op, m)
    return m


def check_args(args) -> None:
    """what the tool refuses, before anything is loaded"""
    if (args.ply is None) == (args.sog is None):
        raise SystemExit("exactly one of --ply and --sog is needed")
    if args.ply is not None and not args.ply.lower().endswith(".ply"):
        raise SystemExit("--ply must name a .ply file")
    if args.sog is not None and not args.sog.lower().endswith(".sog"):
        raise SystemExit("--sog must name a .sog file")
    if args.matrix is not None and args.ops:
        raise SystemExit("give --matrix OR --rotate / --scale / --translate")
    if args.matrix is not None and not all(math.isfinite(v) for v in args.matrix):
        raise SystemExit("--matrix must be finite")
    for kind, vals in args.ops or []:
        if kind == "rotate":
            if vals[0].lower() not in ("x", "y", "z"):
                raise SystemExit("--rotate AXIS must be x, y or z")
            _number(vals[1], "--rotate DEG")
        elif kind == "scale":
            if not _number(vals[0], "--scale") > 0:
                raise SystemExit("--scale must be > 0")
        else:
            for v in vals:
                _number(v, "--translate")
    if (args.crop_min is None) != (args.crop_max is None):
        raise SystemExit("--crop-min and --crop-max are needed together")
    if args.crop_min is not None and not all(math.isfinite(a) and math.isfinite(b) and a < b for a, b in zip(args.crop_min, args.crop_max)):
        raise SystemExit("the crop box needs finite corners with min < max on every axis")
    if args.crop_invert and args.crop_min is None:
        raise SystemExit("--crop-invert needs --crop-min / --crop-max")
    if matrix_of(args) is None and args.crop_min is None:
        raise SystemExit("nothing to do: give a transform (--matrix, --rotate, --scale, --translate) or a crop box")


def main():
    args = build_parser().parse_args()
    check_args(args)

    import numpy as np
    import torch

    import lichtfeld_studio_amd  # noqa: F401
    from lichtfeld_studio_amd import loader, transform

    dev = torch.device("cuda:0")
    m = matrix_of(args)
    xf = transform.similarity(np.array(m, np.float64)) if m is not None else None   # (refuses shear / non-uniform scale / reflections before the file is read)
    model = loader.load_ply(args.ply, device=dev) if args.ply is not None else loader.load_sog(args.sog, device=dev)
    n_before = int(model.means.shape[0])
    out = {"n_before": n_before}
    cameras = targets = None
    if args.data_path is not None:
        from lichtfeld_studio_amd import evaluate
        from lichtfeld_studio_amd.rasterizer import Camera
        scene, ds, _ = loader.colmap_scene(args.data_path, args.images, split="all", resize_factor=args.resize_factor, max_width=args.max_width, text=args.text, device=dev)
        targets = loader.preload(ds, dev)
        cameras = [Camera(scene.viewmats[v:v + 1].contiguous(), scene.Ks[v:v + 1].contiguous(), scene.width, scene.height) for v in range(len(ds))]
        out["psnr_train_views_before"] = round(evaluate.evaluate(model, cameras, targets, antialiased=args.antialiasing).psnr, 4)
    if xf is not None:
        model = transform.transform_model(model, xf, inplace=True)
        out.update(matrix=[[float(v) for v in r] for r in xf.matrix], scale=xf.scale)
    if args.crop_min is not None:
        model = transform.crop(model, args.crop_min, args.crop_max, invert=args.crop_invert)
    out["n_after"] = int(model.means.shape[0])
    if cameras is not None and out["n_after"] > 0:
        if xf is not None:
            moved = transform.transform_cameras(scene.viewmats, xf)
            cameras = [Camera(moved[v:v + 1].contiguous(), scene.Ks[v:v + 1].contiguous(), scene.width, scene.height) for v in range(len(ds))]
        out["psnr_train_views_after"] = round(evaluate.evaluate(model, cameras, targets, antialiased=args.antialiasing).psnr, 4)
    base = args.out[:-4] if args.out.lower().endswith((".ply", ".sog")) else args.out
    os.makedirs(os.path.dirname(os.path.abspath(base)), exist_ok=True)
    loader.save_ply(model, base + ".ply")
    out.update(ply=base + ".ply", ply_bytes=os.path.getsize(base + ".ply"))
    if args.save_sog:
        loader.save_sog(model, base + ".sog", iterations=args.sog_iterations)
        out.update(sog=base + ".sog", sog_bytes=os.path.getsize(base + ".sog"))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
