"""Host model of the absgrad densification signal of the fastgs rasterizer (LFS_FASTGS_ABSGRAD), in numpy and independent of the code under test.

For instance (Gaussian i, pixel p) the blend backward forms h = -alpha dL/dalpha, dx = mean2d.x - (j + 0.5), dy = mean2d.y - (i + 0.5); with (A, B, C) = conic_opacity[i].xyz
that pixel's share of dL/dmean2d_i is gx_p = h (A dx + B dy), gy_p = h (B dx + C dy). The model walks every pixel's tile list back to front from the oracle's forward
(mean2d, conic_opacity, color, alpha, n_contrib, offsets, ids) with the reference's rules - power <= 0, alpha = min(opacity exp(power), 0.999) >= 1/255, the last
n_contrib entries of the list only - and returns per Gaussian the signed sums (Sx, Sy), the absolute sums (Gx, Gy) and both densification_info forms,
    [0][i] = 1, [1][i] = sqrt((0.5 W X_i)^2 + (0.5 H Y_i)^2)   for n_touched[i] != 0, zero otherwise,
(X, Y) = (Sx, Sy) for the default mode and (Gx, Gy) for absgrad. It computes in the dtype of the forward it is given (the sums in float64 either way), so the
float32 forward gives the values a float32 implementation with exact sums would produce: the flip-row budget of the GPU tests is checked with it on the CPU.
The signed form must reproduce oracle.fastgs_backward's densification_info (tests/test_fastgs_absgrad_reference.py): that holds the model to something.

The scenes of the absgrad tests live here too, so that the CPU checks, the GPU tests and the emulated tests share them."""
import functools

import numpy as np

TILE = 16


def absgrad_model(fwd, g_image, g_alpha, W, H, depth=None, g_depth=None):
    """fwd: oracle.fastgs_forward(...) -> dict(Gx, Gy, Sx, Sy [N] float64, dens_abs, dens_signed [2,N] float64, instances: how many (i, p) took part).
    depth [N], g_depth [1,H,W]: the backward with a depth gradient - d_i is blended as a fourth colour channel whose image gradient is g_depth."""
    dt = fwd["mean2d"].dtype.type
    N = fwd["mean2d"].shape[0]
    mx, my = fwd["mean2d"][:, 0], fwd["mean2d"][:, 1]
    ca, cb, cc, op = (fwd["conic_opacity"][:, k] for k in range(4))
    col = np.maximum(fwd["color"], dt(0))
    gi = np.asarray(g_image, dt).reshape(3, H * W)
    ga = np.asarray(g_alpha, dt).reshape(H * W)
    alpha_map, n_contrib = fwd["alpha"].reshape(-1), fwd["n_contrib"].reshape(-1)
    offsets, ids = fwd["offsets"], fwd["ids"]
    min_alpha, max_alpha = dt(1.0) / dt(255.0), dt(np.float32(0.999))
    gw = (W + TILE - 1) // TILE
    out = {k: np.zeros(N, np.float64) for k in ("Gx", "Gy", "Sx", "Sy")}
    instances = 0
    for pix in range(W * H):
        nc = int(n_contrib[pix])
        if nc == 0:
            continue
        py, px = divmod(pix, W)
        t = (py // TILE) * gw + px // TILE
        lst = ids[offsets[t]:offsets[t] + nc][::-1]                     # back to front
        dx, dy = mx[lst] - (dt(px) + dt(0.5)), my[lst] - (dt(py) + dt(0.5))
        s = dt(0.5) * (ca[lst] * dx * dx + cc[lst] * dy * dy) + cb[lst] * dx * dy
        with np.errstate(over="ignore"):
            al = np.minimum(op[lst] * np.exp(-s), max_alpha)
        keep = ~(s < 0) & ~(al < min_alpha)
        lst, dx, dy, al = lst[keep], dx[keep], dy[keep], al[keep]
        if len(lst) == 0:
            continue
        t_final = dt(1) - alpha_map[pix]
        oma_rcp = dt(1) / (dt(1) - al)
        tr = t_final * np.cumprod(oma_rcp)                               # transmittance in front of each entry
        wgt = tr * al
        cv = col[lst] @ gi[:, pix]
        if depth is not None:
            cv = cv + np.asarray(depth, dt)[lst] * np.asarray(g_depth, dt).reshape(-1)[pix]
        behind = np.concatenate([[dt(0)], np.cumsum(wgt * cv)[:-1]]).astype(dt)
        dl_dalpha = ga[pix] * t_final * oma_rcp + tr * cv - behind * oma_rcp
        h = -al * dl_dalpha
        gx = (h * (ca[lst] * dx + cb[lst] * dy)).astype(np.float64)
        gy = (h * (cb[lst] * dx + cc[lst] * dy)).astype(np.float64)
        np.add.at(out["Sx"], lst, gx); np.add.at(out["Sy"], lst, gy)
        np.add.at(out["Gx"], lst, np.abs(gx)); np.add.at(out["Gy"], lst, np.abs(gy))
        instances += len(lst)
    vis = fwd["n_touched"] != 0

    def dens(X, Y):
        return np.stack([vis.astype(np.float64), np.where(vis, np.sqrt((0.5 * W * X) ** 2 + (0.5 * H * Y) ** 2), 0.0)])
    out["dens_abs"], out["dens_signed"] = dens(out["Gx"], out["Gy"]), dens(out["Sx"], out["Sy"])
    out["instances"] = instances
    return out


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------------------------------
# 40 x 24: 3 x 2 tiles, both edges partial, 8 x 8 cells cut by the border; 64 x 48: whole tiles. N = the scene sizes of the depth tests.
# Gaussian 0: large and in front of the camera - it covers four or more tiles, so its row is summed across wavefronts. Gaussians 2 .. 9 (N >= 200): an opaque stack at
# one place, which terminates the pixels under it early (the e.y <= last cut). Gaussian 1 (N >= 2): far outside the image, n_touched == 0.
CFGS = [dict(N=1, W=40, H=24, seed=11), dict(N=2, W=64, H=48, seed=12), dict(N=200, W=40, H=24, seed=13), dict(N=3000, W=64, H=48, seed=14)]
SCENE_IDS = lambda i: f"N{CFGS[i]['N']}_{CFGS[i]['W']}x{CFGS[i]['H']}"


def _look(sc, x, y, z):
    """world position of the camera-space point (x, y, z)"""
    w2c = np.asarray(sc["w2c"], np.float64)
    return w2c[:3, :3].T @ (np.array([x, y, z]) - w2c[:3, 3])


@functools.lru_cache(maxsize=None)
def scene(idx):
    """the scene of configuration idx (a dict as tests/test_oracle_fastgs.py's _scene; never modified)"""
    from test_oracle_fastgs import _scene
    c = CFGS[idx]
    sc = _scene(N=c["N"], W=c["W"], H=c["H"], seed=c["seed"], deg=1, spread=0.6)
    N = c["N"]
    sc["means"][0] = _look(sc, 0.05, -0.03, 3.0)
    sc["scales_raw"][0] = np.log([0.5, 0.35, 0.3])
    sc["opac_raw"][0] = 0.5
    if N >= 2:
        sc["means"][1] = _look(sc, 40.0, 0.0, 3.0)
    if N >= 200:
        for k in range(2, 10):
            sc["means"][k] = _look(sc, -0.25, 0.1, 2.0 + 0.05 * k)
            sc["scales_raw"][k] = np.log([0.2, 0.2, 0.2])
            sc["opac_raw"][k] = 6.0
    return sc


def upstream(sc, seed=5):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((3, sc["H"], sc["W"])).astype(np.float32), rng.standard_normal((1, sc["H"], sc["W"])).astype(np.float32)


def oracle_forward(o, sc, dtype):
    return o.fastgs_forward(sc["means"], sc["scales_raw"], sc["rot_raw"], sc["opac_raw"], sc["sh0"], sc["sh_rest"], sc["w2c"], sc["cam_pos"],
                            sc["active_sh_bases"], sc["W"], sc["H"], sc["fx"], sc["fy"], sc["cx"], sc["cy"], dtype=dtype)


_MODELS = {}


def model_of(o, key, sc, g_image, g_alpha, dtype=np.float64, depth=None, g_depth=None):
    """absgrad_model on the oracle's forward of `sc`, computed once per key (callers pass a key that names scene and gradients) and never modified"""
    k = (key, np.dtype(dtype).name)
    if k not in _MODELS:
        _MODELS[k] = absgrad_model(oracle_forward(o, sc, dtype), g_image, g_alpha, sc["W"], sc["H"], depth=depth, g_depth=g_depth)
    return _MODELS[k]


# the forms of the value test beyond the plain one, each on the scene whose render the device produces in that form:
#   "depth": a depth-mode workspace and a backward with grad_depth; "aa": LFS_FASTGS_ANTIALIASED = the default render at the compensated opacity
#   (tests/fastgs_aa_reference.py); "f3d": the 3D filter = the default render of the baked scene (tests/fastgs_filter3d_reference.py)
VARIANTS = ("plain", "depth", "aa", "f3d")
VARIANT_SCENES = (2, 3)   # the indices into CFGS the three extra forms run on


def filter_var_of(sc):
    """[N] filter variances for the "f3d" form: of the size of the squared scales, different per Gaussian (any non-negative operand is valid)"""
    return np.random.default_rng(21).uniform(0.0, 0.01, len(sc["means"])).astype(np.float32)


def g_depth_of(sc, seed=9):
    return np.random.default_rng(seed).standard_normal((1, sc["H"], sc["W"])).astype(np.float32)


def variant_model(o, idx, variant, dtype=np.float64):
    """the model of scene idx in one of VARIANTS with the random upstream gradients (computed once)"""
    sc = scene(idx)
    gi, ga = upstream(sc)
    if variant == "plain":
        return model_of(o, (idx, "random"), sc, gi, ga, dtype)
    if variant == "depth":
        from fastgs_depth_reference import d64
        return model_of(o, (idx, "depth"), sc, gi, ga, dtype, depth=d64(sc["means"], sc["w2c"], "depth")[0], g_depth=g_depth_of(sc))
    if variant == "aa":
        from fastgs_aa_reference import rho64
        rho = rho64(sc["means"], sc["scales_raw"], sc["rot_raw"], sc["w2c"], sc["fx"], sc["fy"], sc["cx"], sc["cy"], sc["W"], sc["H"])
        o64 = rho / (1.0 + np.exp(-np.asarray(sc["opac_raw"], np.float32).astype(np.float64)))
        with np.errstate(divide="ignore"):
            raw2 = np.where(rho > 0, np.log(o64) - np.log1p(-o64), -30.0)
        return model_of(o, (idx, "aa"), dict(sc, opac_raw=raw2), gi, ga, dtype)
    from fastgs_filter3d_reference import baked_scene
    return model_of(o, (idx, "f3d"), baked_scene(sc, filter_var_of(sc).astype(np.float64))[0], gi, ga, dtype)


def single_gaussian_scene(W, H, mean2d, sigma_px=3.0, z=4.0, opacity_raw=0.0):
    """one isotropic Gaussian (conic B = 0 up to rounding) whose projected centre is `mean2d` (pixel coordinates, pixel p covers [p, p + 1)) and whose projected
    standard deviation is about sigma_px: identity camera, the Gaussian on the plane z, degree-0 grey colour"""
    fx = fy = 64.0
    cx, cy = W / 2.0, H / 2.0
    w2c = np.eye(4)
    means = np.array([[(mean2d[0] - cx) * z / fx, (mean2d[1] - cy) * z / fy, z]])
    s = sigma_px * z / fx
    return dict(means=means, scales_raw=np.log(np.full((1, 3), s)), rot_raw=np.array([[1.0, 0, 0, 0]]), opac_raw=np.array([opacity_raw]),
                sh0=np.full((1, 1, 3), 1.0), sh_rest=np.zeros((1, 15, 3)), w2c=w2c, cam_pos=np.zeros(3), active_sh_bases=1, W=W, H=H, fx=fx, fy=fy, cx=cx, cy=cy)

