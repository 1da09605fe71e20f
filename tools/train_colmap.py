#!/usr/bin/env python
"""Train on a COLMAP directory end to end on one MI355X (the reference's `LichtFeld-Studio -d <data> --images images_4 --test-every 8
--eval -i 30000`, eval/benchmark_mipnerf360.sh:37-44, reduced to the data path this repository covers):

    python tools/train_colmap.py -d /data/garden --images images_4 --iterations 30000 --strategy default --eval -o out/garden

COLMAP reader -> point-cloud initialisation -> fastgs (default) or 3DGUT training with the L1 + SSIM loss and the ADC / MCMC strategy ->
[--enable-sparsity: ADMM sparsification phase + prune] -> PSNR / SSIM on the held-out views -> splat PLY (and, with --save-sog, the .sog bundle). Prints one JSON line. All views must share one image size.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    ap.add_argument("-d", "--data-path", required=True)
    ap.add_argument("--images", default="images")
    ap.add_argument("-i", "--iterations", type=int, default=30000)
    ap.add_argument("--strategy", default="default", choices=["default", "mcmc", "none"])
    ap.add_argument("--gut", action="store_true", help="3DGUT rasterizer instead of the default EWA (fastgs) one")
    ap.add_argument("--test-every", type=int, default=8)
    ap.add_argument("--resize-factor", type=int, default=-1)
    ap.add_argument("--max-width", type=int, default=3840)
    ap.add_argument("--sh-degree", type=int, default=3)
    ap.add_argument("--bilateral-grid", action="store_true")
    ap.add_argument("--eval", action="store_true", help="PSNR / SSIM on the held-out views (every --test-every-th); with --depth-loss also saves their renders and depth maps")
    ap.add_argument("-o", "--output-path", default="output")
    ap.add_argument("--text", action="store_true", help="read cameras.txt / images.txt / points3D.txt")
    ap.add_argument("--eval-every", type=int, default=0, help="with --eval: held-out PSNR (the renderer the model trains with) every N iterations -> 'psnr_curve' (the turbulence of an MCMC run)")
    ap.add_argument("--pose-optimization", default="none", choices=["none", "direct", "mlp"],
                    help="learn a correction of every training camera's pose (fastgs rasterizer only; not together with --eval, as in the reference)")
    ap.add_argument("--save-sog", action="store_true", help="also write splat_<iterations>.sog, the compressed bundle web viewers load (the reference's --save-sog)")
    ap.add_argument("--sog-iterations", type=int, default=10, help="k-means iterations of the SOG export (the reference's sog_iterations)")
    ap.add_argument("--sog-palette-size", type=int, default=None, help="entries of the SOG shN palette, up to min(65536, N) (default: the reference's value, 64 from 1024 Gaussians on)")
    ap.add_argument("--enable-sparsity", action="store_true", help="after --iterations, ADMM sparsification for --sparsify-steps more iterations, then prune to (1 - --prune-ratio) of the Gaussians")
    ap.add_argument("--sparsify-steps", type=int, default=15000)
    ap.add_argument("--init-rho", type=float, default=0.0005, help="ADMM penalty parameter")
    ap.add_argument("--prune-ratio", type=float, default=0.6, help="share of the Gaussians the final prune removes")
    ap.add_argument("--mask-mode", default="none", choices=["none", "ignore", "segment"],
                    help="image masks (<data>/<masks folder>/<image name>.png, or the image's own alpha): ignore = masked pixels leave the loss; segment = and the opacity outside the mask is penalised (fastgs rasterizer)")
    ap.add_argument("--masks-folder", default="masks")
    ap.add_argument("--invert-masks", action="store_true", help="the mask files mark what to IGNORE (white = ignored)")
    ap.add_argument("--mask-threshold", type=int, default=-1, help="binarise: mask byte >= N counts fully, below it not at all (default: keep soft values)")
    ap.add_argument("--mask-alpha-weight", type=float, default=1.0, help="weight of the opacity penalty of --mask-mode segment")
    ap.add_argument("--antialiasing", action="store_true", help="antialiased mode of the EWA rasterizer for training and --eval renders (the reference's antialiasing parameter)")
    ap.add_argument("--filter3d", action="store_true", help="the 3D smoothing filter of Mip-Splatting (fastgs rasterizer): a per-Gaussian low-pass sized by the highest rate at which any "
                    "training camera samples the Gaussian; training and --eval renders use it, and the saved PLY / SOG hold the BAKED scales and opacities, so any viewer "
                    "renders what was trained (a baked file is not a resume point: training on from it would apply the filter twice)")
    ap.add_argument("--filter3d-every", type=int, default=100, help="recompute the filter every N iterations (and after every refinement)")
    ap.add_argument("--mip-splatting", action="store_true", help="--filter3d and --antialiasing together: the 3D smoothing filter and the 2D Mip filter")
    ap.add_argument("--absgrad", action="store_true", help="ADC densifies by the per-pixel ABSOLUTE screen-space gradients (AbsGS; fastgs rasterizer, --strategy default): large "
                    "Gaussians over fine texture, whose signed gradients cancel, get split. Without --grad-threshold the threshold becomes 8e-4")
    ap.add_argument("--grad-threshold", type=float, default=None, help="ADC's screen-space gradient threshold for splitting / cloning (default 2e-4; 8e-4 with --absgrad)")
    ap.add_argument("--visible-adam", action="store_true", help="the optimizer updates only the Gaussians the step's views saw (gsplat's visible_adam, the official code's "
                    "sparse_adam; fastgs rasterizer): the others keep parameters and Adam moments untouched, and the step streams only the visible rows")
    ap.add_argument("--contribution-prune-at", type=int, nargs="+", default=[], metavar="ITER",
                    help="contribution pruning (fastgs rasterizer): at the end of each listed iteration, compute every Gaussian's maximum blending weight over ALL training "
                         "views and remove the ones below --contribution-threshold (RadSplat). Training goes on and heals what the prune disturbed")
    ap.add_argument("--contribution-threshold", type=float, default=0.01, help="a Gaussian no training ray weights this much is removed (RadSplat: 0.01)")
    ap.add_argument("--depth-loss", default="none", choices=["none", "invdepth", "depth"],
                    help="depth-regularised training (fastgs rasterizer): L1 between the accumulated inverse depth (invdepth: monocular depth, the Inria convention) or depth of a view "
                         "and <data>/<depths folder>/<image stem>.npy (float32 [H,W]) or .png (16-bit greyscale, value / 65536). With --eval, every held-out render is then saved as "
                         "<output>/renders/val_NNNN.png with its expected-depth map val_NNNN_depth.png beside it (without --depth-loss no renders are saved)")
    ap.add_argument("--depths-folder", default="depths")
    ap.add_argument("--depth-params", default=None, help="depth_params.json: per image {scale, offset}, target = value * scale + offset; a view without an entry or with "
                                                         "scale <= 0 trains without a depth target (default: <data>/sparse/0/depth_params.json when it exists)")
    ap.add_argument("--depth-weight-init", type=float, default=1.0, help="weight of the depth loss at the first iteration")
    ap.add_argument("--depth-weight-final", type=float, default=0.01, help="... and at the last: exponential decay between the two")
    ap.add_argument("--undistort", action="store_true", help="resample every image whose COLMAP camera has lens distortion (SIMPLE_RADIAL, RADIAL, OPENCV, FULL_OPENCV, the fisheye "
                    "models) to a distortion-free pinhole camera of the same size at load, masks and depth targets with it, and train / --eval on that camera (without: the "
                    "distortion parameters are ignored, as if the images had gone through COLMAP's image_undistorter)")
    ap.add_argument("--undistort-alpha", type=float, default=0.0, help="with --undistort: 0 = zoom in until no output pixel is blank, 1 = zoom out until no source pixel is lost "
                    "(OpenCV's getOptimalNewCameraMatrix alpha); above 0 the blank pixels leave the loss (--mask-mode none becomes ignore)")
    ap.add_argument("--background", type=float, nargs=3, default=None, metavar=("R", "G", "B"), help="the colour training renders (and RGBA targets) are composited over, in [0,1] (default black)")
    ap.add_argument("--white-background", action="store_true", help="--background 1 1 1 (the official trainer's --white_background)")
    ap.add_argument("--random-background", action="store_true", help="one random colour per step (seeded, CPU generator; the official trainer's random_background): with "
                    "--alpha-targets, transparent becomes the only consistent explanation of a pixel whose alpha is 0")
    ap.add_argument("--bg-modulation", action="store_true", help="the reference's bg_modulation: a sine-modulated colour mixed into the background for the first three quarters of the run")
    ap.add_argument("--alpha-targets", action="store_true", help="images with an alpha channel (2 or 4 channels) are composited over the step's background colour "
                    "before the loss, and over the evaluation background by --eval")
    return ap


def check_args(args) -> None:
    """the combinations the tool refuses, before anything is loaded"""
    if args.mip_splatting:
        args.filter3d = args.antialiasing = True
    if args.filter3d and args.gut:
        raise SystemExit("--filter3d is not wired into the 3DGUT route. Please disable the 3D filter or disable gut.")
    if args.antialiasing and args.gut:
        raise SystemExit("--antialiasing is not wired into the 3DGUT route. Please disable antialiasing or disable gut.")
    if args.absgrad and args.gut:
        raise SystemExit("--absgrad is not wired into the 3DGUT route. Please disable absgrad or disable gut.")
    if args.absgrad and args.strategy != "default":
        raise SystemExit("--absgrad changes what ADC densifies by: it needs --strategy default.")
    if args.visible_adam and args.gut:
        raise SystemExit("--visible-adam is not wired into the 3DGUT route. Please disable visible-adam or disable gut.")
    if args.visible_adam and args.enable_sparsity:
        raise SystemExit("--visible-adam cannot be combined with --enable-sparsity: the ADMM penalty must reach every opacity.")
    if args.contribution_prune_at:
        if args.gut:
            raise SystemExit("--contribution-prune-at is not wired into the 3DGUT route. Please disable contribution pruning or disable gut.")
        if args.strategy == "mcmc":
            raise SystemExit("--contribution-prune-at cannot be combined with --strategy mcmc: MCMC holds the Gaussian count and would relocate onto the freed rows.")
        bad = [i for i in args.contribution_prune_at if not 1 <= i <= args.iterations]
        if bad:
            raise SystemExit(f"--contribution-prune-at names iterations outside 1..{args.iterations}: {bad}")
        if not 0.0 < args.contribution_threshold < 1.0:
            raise SystemExit("--contribution-threshold must lie in (0, 1): it is compared with a blending weight")
    if args.grad_threshold is not None and not args.grad_threshold > 0:
        raise SystemExit("--grad-threshold must be > 0")
    if args.depth_loss != "none" and args.gut:
        raise SystemExit("--depth-loss is not wired into the 3DGUT route. Please disable the depth loss or disable gut.")
    if args.depth_loss != "none" and not (args.depth_weight_init > 0 and args.depth_weight_final > 0):
        raise SystemExit("--depth-weight-init and --depth-weight-final must be > 0 (the weight is interpolated in the logarithm)")
    if not 0.0 <= args.undistort_alpha <= 1.0:
        raise SystemExit("--undistort-alpha must be in [0, 1]")
    if args.undistort_alpha > 0 and not args.undistort:
        raise SystemExit("--undistort-alpha needs --undistort")
    if args.undistort and args.undistort_alpha > 0 and args.mask_mode == "none":
        args.mask_mode = "ignore"
        print("undistort: --undistort-alpha > 0 leaves blank pixels in the targets; --mask-mode none becomes ignore (they leave the loss)", file=sys.stderr)
    if args.random_background and args.bg_modulation:
        raise SystemExit("--random-background and --bg-modulation both choose the colour of every step: pass one of them.")
    if args.white_background and args.background is not None:
        raise SystemExit("--white-background is --background 1 1 1: pass one of them.")
    if args.white_background:
        args.background = [1.0, 1.0, 1.0]
    if args.background is not None and not all(v == v and 0.0 <= v <= 1.0 for v in args.background):
        raise SystemExit("--background takes three numbers in [0, 1]")
    if args.pose_optimization != "none" and args.eval:   # trainer.cpp:367-370
        raise SystemExit("Evaluating with pose optimization is not supported yet. Please disable pose optimization or evaluation.")


def depth_params_path(args):
    """--depth-params, or the Inria pipeline's default location when that file exists, or None (the files' values are the targets)"""
    if args.depth_params:
        return args.depth_params
    for cand in (os.path.join(args.data_path, "sparse", "0", "depth_params.json"), os.path.join(args.data_path, "depth_params.json")):
        if os.path.isfile(cand):
            return cand
    return None


def main():
    args = build_parser().parse_args()
    check_args(args)

    import lichtfeld_studio_amd  # noqa: F401
    from lichtfeld_studio_amd import evaluate, loader, strategies
    from lichtfeld_studio_amd.rasterizer import Camera
    from lichtfeld_studio_amd.trainer import GutTrainer

    dev = torch.device("cuda:0")
    mcmc = args.strategy == "mcmc"
    op_kw = {"absgrad": True} if args.absgrad else {}
    if args.grad_threshold is not None:
        op_kw["grad_threshold"] = args.grad_threshold
    op = strategies.OptimizationParameters.for_strategy(args.strategy, iterations=args.iterations, **op_kw)   # ADC: stop_refine 15000, no regularisers
    if args.absgrad:
        print(f"absgrad: ADC reads absolute screen-space gradients, grad_threshold {op.grad_threshold:g}" + ("" if args.grad_threshold is not None else " (the default of this mode)"))
    init_scaling, init_opacity = (0.1, 0.5) if mcmc else (1.0, 0.1)        # parameter/{mcmc,default}_optimization_params.json
    t0 = time.time()
    split = "train" if args.eval else "all"
    scene, ds, scene_scale = loader.colmap_scene(args.data_path, args.images, split=split, test_every=args.test_every, resize_factor=args.resize_factor,
                                                 max_width=args.max_width, sh_degree=args.sh_degree, init_scaling=init_scaling, init_opacity=init_opacity,
                                                 text=args.text, device=dev, masks_folder=args.masks_folder, depths_folder=args.depths_folder,
                                                 undistort=args.undistort, undistort_alpha=args.undistort_alpha)
    maps = [ds.undistort_map(k) for k in range(len(ds))]
    if not args.undistort:
        n_dist = sum(1 for i in ds.indices if ds.cameras[i].camera_model_type != 0 or np.any(ds.cameras[i].radial_distortion) or np.any(ds.cameras[i].tangential_distortion))
        if n_dist:
            print(f"warning: {n_dist} of {len(ds)} views have lens distortion, which is being IGNORED (pinhole rendering against distorted images); pass --undistort",
                  file=sys.stderr)
    masks = loader.preload_masks(ds, dev, args.invert_masks, args.mask_threshold) if args.mask_mode != "none" else None
    depths = None
    if args.depth_loss != "none":
        depths = loader.preload_depths(ds, dev, args.depth_loss, loader.load_depth_params(depth_params_path(args)), masks)
        if not any(d is not None for d in depths):
            raise SystemExit(f"--depth-loss {args.depth_loss}: no view has a usable depth target under {os.path.join(args.data_path, args.depths_folder)}")
    alphas = loader.preload_alphas(ds, dev) if args.alpha_targets else None
    if alphas is not None and not any(a is not None for a in alphas):
        raise SystemExit("--alpha-targets: no image of the split has an alpha channel")
    background = tuple(args.background) if args.background is not None else (0.0, 0.0, 0.0)
    background_mode = "random" if args.random_background else "modulated" if args.bg_modulation else "constant"
    targets = loader.preload(ds, dev, workers=os.cpu_count() or 8)          # resident in HBM: 288 GB hold a Mip-NeRF360 scene at full resolution
    t_load = time.time() - t0
    rast = "gut" if args.gut else "fastgs"
    if args.bilateral_grid and rast != "fastgs":
        raise SystemExit("--bilateral-grid needs the fastgs rasterizer")
    tr = GutTrainer(scene, dev, iterations=args.iterations, loss="l1_ssim", strategy=None if args.strategy == "none" else args.strategy, opt_params=op,
                    scene_scale=scene_scale, rasterizer=rast, use_bilateral_grid=args.bilateral_grid, pose_optimization=args.pose_optimization,
                    enable_sparsity=args.enable_sparsity, sparsify_steps=args.sparsify_steps, init_rho=args.init_rho, prune_ratio=args.prune_ratio,
                    mask_mode=args.mask_mode, mask_alpha_weight=args.mask_alpha_weight, antialiasing=args.antialiasing,
                    depth_loss=args.depth_loss, depth_weight=(args.depth_weight_init, args.depth_weight_final),
                    filter3d=args.filter3d, filter3d_every=args.filter3d_every, absgrad=args.absgrad, visible_adam=args.visible_adam,
                    contribution_prune_at=tuple(args.contribution_prune_at), contribution_threshold=args.contribution_threshold,
                    background=background, background_mode=background_mode)
    total = tr.total_iterations                                             # --iterations, plus the sparsification phase

    def export():
        """the model a file is written from: with --filter3d the filter of the CURRENT model folded into scales and opacities (filter3d.bake), the model itself otherwise"""
        if not args.filter3d:
            return tr.model
        from lichtfeld_studio_amd import filter3d
        from lichtfeld_studio_amd.rasterizer import SplatModel
        m = tr.model
        with torch.no_grad():
            scales, opac = filter3d.bake(m, tr.update_filter3d(force=True))
        return SplatModel(m.means.detach(), m.sh0.detach(), m.shN.detach(), scales, m.raw_quats.detach(), opac, m.max_sh_degree, m.active_sh_degree)
    def val_K(val, k, w, h):
        """a held-out view's intrinsics: its undistortion map's destination camera, or the plain pinhole K"""
        m = val.undistort_map(k)
        return loader.intrinsics(val.cameras[val.indices[k]], w, h) if m is None else m.K()
    os.makedirs(args.output_path, exist_ok=True)
    g = torch.Generator().manual_seed(0)
    val_set = None
    if args.eval and args.eval_every > 0:
        cams_all, _ = (loader.read_colmap_cameras_and_images_text if args.text else loader.read_colmap_cameras_and_images)(args.data_path, args.images)
        val = loader.CameraDataset(cams_all, "val", args.test_every, args.resize_factor, args.max_width, undistort=args.undistort, undistort_alpha=args.undistort_alpha)
        vc, vi = [], []
        for k, img in enumerate(loader.preload(val, dev)):
            cam = val.cameras[val.indices[k]]
            h, w = img.shape[1:]
            vc.append(Camera(torch.from_numpy(loader.world_to_view(cam))[None].to(dev), torch.from_numpy(val_K(val, k, w, h))[None].to(dev), w, h))
            vi.append(img)
        val_set = (vc, vi)
    curve = []
    t0 = time.time()
    t_eval = 0.0
    order = []
    for it in range(total):
        if not order:
            order = torch.randperm(len(ds), generator=g).tolist()          # infinite random sampler, one view per step
        v = order.pop()
        tr.train_step([targets[v]], views=[v], masks=None if masks is None else [masks[v]], depths=None if depths is None else [depths[v]],
                      alphas=None if alphas is None else [alphas[v]])
        if args.enable_sparsity and it + 1 == args.iterations:              # the model of the base run, before sparsification touches it
            loader.save_ply(export(), os.path.join(args.output_path, f"splat_{args.iterations}.ply"))
        if val_set is not None and (it + 1) % args.eval_every == 0:
            torch.cuda.synchronize(); te = time.time()
            m = evaluate.evaluate(tr.model, val_set[0], val_set[1], it + 1, rasterizer=rast if args.gut else "fastgs", antialiased=args.antialiasing,
                                  filter3d=tr.update_filter3d(force=True))
            # the same metric on 12 TRAINING views: a held-out PSNR that falls while this one holds is a generalisation gap (Gaussians fitted to the rays the training views
            # sample), both falling is an unstable optimisation
            tsel = list(range(0, len(ds), max(1, len(ds) // 12)))[:12]
            tcams = [tr.camera(v) for v in tsel]
            mt = evaluate.evaluate(tr.model, tcams, [targets[v] for v in tsel], it + 1, rasterizer=rast if args.gut else "fastgs", antialiased=args.antialiasing,
                                  filter3d=tr.update_filter3d(force=True))
            s3 = tr.model.raw_scales.detach()
            asp = (s3.max(-1).values - s3.min(-1).values).exp()
            # projected size of the SMALLEST axis of every Gaussian in pixels at the first training camera (focal length x scale / depth): the share below half a pixel
            cam0 = tr.camera(0)
            with torch.no_grad():
                pc = tr.model.means.detach() @ cam0.world_view_transform[0, :3, :3].T + cam0.world_view_transform[0, :3, 3]
                px = float(cam0.K[0, 0, 0]) * s3.exp().min(-1).values / pc[:, 2].clamp_min(1e-3)
                sub = float(((px < 0.5) & (pc[:, 2] > 0.01)).float().mean())
            curve.append({"iteration": it + 1, "psnr": round(m.psnr, 3), "psnr_train_views": round(mt.psnr, 3), "thin_axis_below_half_pixel": round(sub, 4),
                          "gaussians": int(tr.model.means.shape[0]), "mean_log_scale": round(float(s3.mean()), 3),
                          "median_aspect": round(float(asp.median()), 2), "frac_aspect_ge_10": round(float((asp >= 10).float().mean()), 4)})
            print(json.dumps(curve[-1]), file=sys.stderr, flush=True)
            t_eval += time.time() - te
    torch.cuda.synchronize()
    t_train = time.time() - t0 - t_eval
    out = {"data": args.data_path, "images": len(ds), "size": [scene.width, scene.height], "iterations": total, "rasterizer": rast,
           "strategy": args.strategy, "antialiasing": bool(args.antialiasing), "filter3d": bool(args.filter3d), "absgrad": bool(args.absgrad), "visible_adam": bool(args.visible_adam), "pose_optimization": args.pose_optimization, "gaussians": int(tr.model.means.shape[0]), "load_s": round(t_load, 1), "train_s": round(t_train, 1),
           "iters_per_s": round(total / max(t_train, 1e-9), 1)}
    if masks is not None:
        out.update(mask_mode=args.mask_mode, masked_views=sum(m is not None for m in masks))
    if args.undistort:
        zs = [m.z for m in maps if m is not None]
        out.update(undistort_alpha=args.undistort_alpha, undistorted_views=len(zs), undistort_z=[round(min(zs), 5), round(max(zs), 5)] if zs else None)
    if background_mode != "constant" or background != (0.0, 0.0, 0.0) or alphas is not None:
        out.update(background=list(background), background_mode=background_mode, alpha_views=None if alphas is None else sum(a is not None for a in alphas))
    if depths is not None:
        out.update(depth_loss=args.depth_loss, depth_views=sum(d is not None for d in depths), depth_weight=[args.depth_weight_init, args.depth_weight_final])
    if args.enable_sparsity:
        out.update(base_iterations=args.iterations, sparsify_steps=args.sparsify_steps, prune_ratio=args.prune_ratio, init_rho=args.init_rho)
    if args.eval:
        cams_all, _ = (loader.read_colmap_cameras_and_images_text if args.text else loader.read_colmap_cameras_and_images)(args.data_path, args.images)
        val = loader.CameraDataset(cams_all, "val", args.test_every, args.resize_factor, args.max_width, data_path=args.data_path, masks_folder=args.masks_folder,
                                   undistort=args.undistort, undistort_alpha=args.undistort_alpha)   # the held-out views through the same kind of map
        val_masks = loader.preload_masks(val, dev, args.invert_masks, args.mask_threshold) if args.mask_mode != "none" else None   # PSNR over the masked pixels; SSIM unmasked
        cameras, images = [], []
        for k, img in enumerate(loader.preload(val, dev)):
            cam = val.cameras[val.indices[k]]
            h, w = img.shape[1:]
            cameras.append(Camera(torch.from_numpy(loader.world_to_view(cam))[None].to(dev), torch.from_numpy(val_K(val, k, w, h))[None].to(dev), w, h))
            images.append(img)
        val_alphas = loader.preload_alphas(val, dev) if args.alpha_targets else None
        eval_bg = torch.tensor(background, dtype=torch.float32, device=dev)   # (the base colour: the per-step modes end on it)
        m = evaluate.evaluate(tr.model, cameras, images, total, background=eval_bg, masks=val_masks, antialiased=args.antialiasing,
                              filter3d=tr.update_filter3d(force=True), alphas=val_alphas)
        out.update(psnr=round(m.psnr, 4), ssim=round(m.ssim, 5), val_images=m.n_images)
        if args.depth_loss != "none":   # the held-out renders and, beside each, its expected depth map (D / alpha; grey, scaled to the view's own range)
            from lichtfeld_studio_amd import fastgs
            from lichtfeld_studio_amd.rasterizer import RenderMode
            rdir = os.path.join(args.output_path, "renders")
            os.makedirs(rdir, exist_ok=True)
            for k, cam in enumerate(cameras):
                with torch.no_grad():
                    r = fastgs.fast_rasterize(cam, tr.model, torch.zeros(3, device=dev), antialiased=args.antialiasing, render_mode=RenderMode.RGB_ED, depth_kind=args.depth_loss,
                                              filter3d=tr.filter3d_var)
                rgb = (r.image.clamp(0, 1) * 255.0 + 0.5).to(torch.uint8).permute(1, 2, 0).contiguous().cpu().numpy()
                d = r.depth[0]
                lo, hi = float(d[r.alpha[0] > 0.5].min()) if bool((r.alpha[0] > 0.5).any()) else 0.0, float(d.max())
                grey = (((d - lo) / max(hi - lo, 1e-12)).clamp(0, 1) * 255.0 + 0.5).to(torch.uint8).cpu().numpy()
                loader.write_png(os.path.join(rdir, f"val_{k:04d}.png"), rgb)
                loader.write_png(os.path.join(rdir, f"val_{k:04d}_depth.png"), grey[..., None].repeat(3, axis=2))
            out["renders"] = rdir
        if args.gut:   # the reference's protocol above renders with the EWA rasterizer; this is the renderer the model was trained with
            mg = evaluate.evaluate(tr.model, cameras, images, total, background=eval_bg, rasterizer="gut", masks=val_masks, alphas=val_alphas)
            out.update(psnr_gut=round(mg.psnr, 4), ssim_gut=round(mg.ssim, 5))
    if curve:
        out["psnr_curve"] = curve
    ply = os.path.join(args.output_path, f"splat_{total}.ply")
    loader.save_ply(export(), ply)
    out["ply"] = ply
    if args.filter3d:   # the file above holds the baked parameters (what a viewer renders); the raw ones - the state training would go on from - beside it
        raw_ply = os.path.join(args.output_path, f"splat_{total}_unfiltered.ply")
        loader.save_ply(tr.model, raw_ply)
        out["ply_unfiltered"] = raw_ply
    if args.save_sog:
        sog_path = os.path.join(args.output_path, f"splat_{total}.sog")
        loader.save_sog(export(), sog_path, iterations=args.sog_iterations, palette_size=args.sog_palette_size)
        out.update(sog=sog_path, sog_bytes=os.path.getsize(sog_path), ply_bytes=os.path.getsize(ply))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
