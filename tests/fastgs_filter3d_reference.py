"""Exact host model of the 3D smoothing filter, independent of the code under test. float64 arithmetic on inputs taken at float32 (what the
device sees), as tests/fastgs_aa_reference.py does.

    camera c sees Gaussian i  iff  z > 0.2 and -0.15 W <= x <= 1.15 W and -0.15 H <= y <= 1.15 H   ((x, y) the pinhole projection in pixels)
    nu_i = max over the seeing cameras of max(fx, fy) / z;  unseen: the smallest nu among the seen;  v_i = variance_scale / nu_i^2  (none seen / C = 0: v = 0)
    s'_k = sqrt(s_k^2 + v),  kappa = prod_k s_k / s'_k,  o' = sigmoid(raw) kappa
    backward: g_k = g'_k (1 - u_k) + S u_k,  u_k = v / (s_k^2 + v),  S = o_eff dL/do_eff,  g_opac = S (1 - sigmoid(raw))

A camera is the dict(w2c [4,4], fx, fy, cx, cy, W, H)."""
import numpy as np

NEAR_Z = 0.2
MARGIN = 0.15


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def project64(means, cam):
    """-> (x, y, z, mag) per Gaussian: pixel coordinates, camera-space depth, and mag = sum_k |r_k m_k| + |t| of the depth row (what its float32 rounding scales with)"""
    m, w = _f32(means), _f32(cam["w2c"])
    p = m @ w[:3, :3].T + w[:3, 3]
    fx, fy, cx, cy = [float(np.float32(cam[k])) for k in ("fx", "fy", "cx", "cy")]
    z = p[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        x, y = fx * p[:, 0] / z + cx, fy * p[:, 1] / z + cy
    mag = np.abs(m * w[2, :3]).sum(1) + abs(w[2, 3])
    return x, y, z, mag


def seen64(means, cam):
    x, y, z, _ = project64(means, cam)
    W, H = float(cam["W"]), float(cam["H"])
    with np.errstate(invalid="ignore"):
        return (z > NEAR_Z) & (x >= -MARGIN * W) & (x <= (1 + MARGIN) * W) & (y >= -MARGIN * H) & (y <= (1 + MARGIN) * H)


def boundary_distance(means, cam):
    """relative distance of every Gaussian to the nearest boundary of the 'seen' test of this camera (z = 0.2 and the four frustum planes; the frustum planes only count
    for points in front of the camera)"""
    x, y, z, _ = project64(means, cam)
    W, H = float(cam["W"]), float(cam["H"])
    dz = np.abs(z - NEAR_Z) / NEAR_Z
    with np.errstate(invalid="ignore"):
        dx = np.minimum(np.abs(x + MARGIN * W), np.abs(x - (1 + MARGIN) * W)) / W
        dy = np.minimum(np.abs(y + MARGIN * H), np.abs(y - (1 + MARGIN) * H)) / H
    front = z > 0
    return np.where(front, np.minimum(dz, np.minimum(dx, dy)), dz)


def nu64(means, cams):
    """-> (nu [N] with 0 for unseen, argmax camera [N] (-1 unseen), seen [C,N], z [C,N], mag [C,N], f [C])"""
    N = len(means)
    nu, arg = np.zeros(N), np.full(N, -1)
    seen, zs, mags, fs = [], [], [], []
    for c, cam in enumerate(cams):
        _, _, z, mag = project64(means, cam)
        s = seen64(means, cam)
        f = max(float(np.float32(cam["fx"])), float(np.float32(cam["fy"])))
        with np.errstate(divide="ignore"):
            rate = np.where(s, f / z, 0.0)
        better = rate > nu
        nu, arg = np.where(better, rate, nu), np.where(better, c, arg)
        seen.append(s); zs.append(z); mags.append(mag); fs.append(f)
    shp = (len(cams), N)
    return nu, arg, np.array(seen).reshape(shp), np.array(zs).reshape(shp), np.array(mags).reshape(shp), np.array(fs)


def filter_var64(means, cams, variance_scale=0.2):
    nu = nu64(means, cams)[0]
    if not (nu > 0).any():
        return np.zeros(len(means))
    nu = np.where(nu > 0, nu, nu[nu > 0].min())
    return float(np.float32(variance_scale)) / nu ** 2


def filter_var_tolerance(means, cams, variance_scale=0.2):
    """the bound on |v_device - v64|, derived: the device's depth is off by |dz| <= 4 * 2^-24 * mag (three products and three sums, each rounded once), nu = f / z by
    nu |dz| / z plus one rounding, v = scale / nu^2 by twice nu's relative error plus the roundings of the square and the quotient: v (2 |dz| / z + 2 ulp), 1 ulp =
    2^-23 relative. The depth error taken is the worst over the cameras that see the Gaussian (whichever of them the device picks as the maximum); an unseen Gaussian
    takes the worst over all seen pairs (the minimum can come from any of them)."""
    nu, _, seen, z, mag, _ = nu64(means, cams)
    v = filter_var64(means, cams, variance_scale)
    if len(cams) == 0 or not seen.any():
        return np.zeros(len(means))
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(seen, 4 * 2.0 ** -24 * mag / np.abs(z), 0.0)
    per = rel.max(0)
    per = np.where(nu > 0, per, rel.max())
    return v * (2 * per + 2 * 2.0 ** -23)


def sigmoid64(raw):
    return 1.0 / (1.0 + np.exp(-_f32(raw)))


def effective64(scales_raw, opac_raw, v):
    """-> (log s' [N,3], kappa [N], u [N,3], o' = sigmoid(raw) kappa [N], logit(o') [N] (-30 where o' = 0))"""
    rs, v = _f32(scales_raw), _f32(v).reshape(-1, 1)
    s2 = np.exp(2 * rs)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(v > 0, v / (s2 + v), 0.0)
        kappa = np.sqrt(np.prod(1.0 - u, axis=1))
        o = sigmoid64(opac_raw).reshape(-1) * kappa
        logit = np.where(o > 0, np.log(o) - np.log1p(-o), -30.0)
    return 0.5 * np.log(s2 + v), kappa, u, o, logit


def baked_scene(sc, v):
    """the scene whose default render is the filtered render of (sc, v)"""
    ls, kappa, u, o, logit = effective64(sc["scales_raw"], sc["opac_raw"], v)
    return dict(sc, scales_raw=ls, opac_raw=logit), kappa, u


def chain64(g_scales_eff, g_opac_eff, sc, v):
    """gradients of the default backward at the baked parameters -> the filtered backward's (grad_scales_raw, grad_opacities_raw, the S u term)
    g_opac_eff = S (1 - o') with o' the baked opacity, so S = g_opac_eff / (1 - o')"""
    _, kappa, u, o, _ = effective64(sc["scales_raw"], sc["opac_raw"], v)
    S = np.asarray(g_opac_eff, np.float64).reshape(-1) / (1.0 - o)
    su = S[:, None] * u
    return np.asarray(g_scales_eff, np.float64) * (1.0 - u) + su, S * (1.0 - sigmoid64(sc["opac_raw"]).reshape(-1)), su


def camera_of_scene(sc):
    return dict(w2c=sc["w2c"], fx=sc["fx"], fy=sc["fy"], cx=sc["cx"], cy=sc["cy"], W=sc["W"], H=sc["H"])


def look_at(eye, target, up=(0.0, 1.0, 0.0)):
    """world-to-camera [4,4] of a camera at `eye` whose +z axis points at `target`"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    f = target - eye; f /= np.linalg.norm(f)
    r = np.cross(np.asarray(up, np.float64), f); r /= np.linalg.norm(r)
    d = np.cross(f, r)
    w = np.eye(4)
    w[:3, :3] = np.stack([r, d, f])
    w[:3, 3] = -w[:3, :3] @ eye
    return w
