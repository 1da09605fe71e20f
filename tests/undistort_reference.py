"""Float64 model of the undistortion resample, numpy only, written from the definitions: the pixel convention (centres at +0.5), the OpenCV
pinhole terms, the OpenCV fisheye polynomial, the validity rule, the single bilinear tap with its 8-bit re-quantisation, the nearest-neighbour pick. It shares no
code with csrc/undistort.hip, csrc/lfs_camera.cuh or lichtfeld-studio_amd/undistort.py. A map `m` is anything with the fields of lfs_undistort_map (the ctypes
struct the kernel receives: the model is evaluated on exactly the numbers the kernel gets)."""
import numpy as np

PINHOLE, FISHEYE = 0, 2


def fisheye_max_angle(k):
    """smallest theta > 0 with d/dtheta (theta + k1 theta^3 + k2 theta^5 + k3 theta^7 + k4 theta^9) = 0; inf when the polynomial grows everywhere"""
    k = [float(v) for v in k[:4]]
    poly = np.polynomial.Polynomial([1.0, 3 * k[0], 5 * k[1], 7 * k[2], 9 * k[3]])   # in theta^2
    roots = [r.real for r in poly.roots() if abs(r.imag) < 1e-12 and r.real > 0]
    return float(np.sqrt(min(roots))) if roots else float("inf")


def distort(m, x, y):
    """normalised undistorted -> (normalised distorted x, y, accepted by the model)"""
    k = [float(v) for v in m.radial]
    if int(m.model) == FISHEYE:
        r = np.hypot(x, y)
        th = np.arctan(r)
        rd = th + k[0] * th ** 3 + k[1] * th ** 5 + k[2] * th ** 7 + k[3] * th ** 9
        s = np.where(r > 0, rd / np.where(r > 0, r, 1.0), 1.0)
        return s * x, s * y, th < float(m.max_angle)
    p1, p2 = float(m.tangential[0]), float(m.tangential[1])
    s1, s2, s3, s4 = [float(v) for v in m.thin]
    r2 = x * x + y * y
    with np.errstate(divide="ignore", invalid="ignore"):
        radial = (1 + k[0] * r2 + k[1] * r2 ** 2 + k[2] * r2 ** 3) / (1 + k[3] * r2 + k[4] * r2 ** 2 + k[5] * r2 ** 3)
    xd = x * radial + 2 * p1 * x * y + p2 * (r2 + 2 * x * x) + s1 * r2 + s2 * r2 ** 2
    yd = y * radial + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y + s3 * r2 + s4 * r2 ** 2
    return xd, yd, radial > 0.8


def source_positions(m):
    """-> (sx, sy, accepted) float64 [dh,dw]: where every destination pixel centre reads the source (continuous coordinates, centres at +0.5)"""
    xs = (np.arange(int(m.dst_width), dtype=np.float64) + 0.5 - float(m.dst_cx)) / float(m.dst_fx)
    ys = (np.arange(int(m.dst_height), dtype=np.float64) + 0.5 - float(m.dst_cy)) / float(m.dst_fy)
    x, y = np.meshgrid(xs, ys)
    xd, yd, ok = distort(m, x, y)
    return xd * float(m.src_fx) + float(m.src_cx), yd * float(m.src_fy) + float(m.src_cy), ok


def border_margin(m, sx, sy):
    """signed distance of the position to the rectangle of source pixel centres [0.5, sw - 0.5] x [0.5, sh - 0.5]: >= 0 inside"""
    with np.errstate(invalid="ignore"):
        mg = np.minimum(np.minimum(sx - 0.5, int(m.src_width) - 0.5 - sx), np.minimum(sy - 0.5, int(m.src_height) - 0.5 - sy))
    return np.where(np.isfinite(mg), mg, -np.inf)


def evaluate(m):
    """-> (sx, sy, valid, margin): valid = the model accepts the pixel and all four bilinear taps are inside the source"""
    sx, sy, ok = source_positions(m)
    mg = border_margin(m, sx, sy)
    return sx, sy, ok & (mg >= 0), mg


def bilinear_u8(src, sx, sy, valid):
    """one bilinear tap of a uint8 [h,w] or [h,w,c] source at the valid positions, re-quantised to 8 bit with round-to-nearest -> int64 [dh,dw(,c)], 0 elsewhere"""
    a = np.asarray(src, np.float64)
    if a.ndim == 2:
        a = a[..., None]
    h, w = a.shape[:2]
    fx, fy = np.where(valid, sx, 0.5) - 0.5, np.where(valid, sy, 0.5) - 0.5
    x0, y0 = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
    ax, ay = (fx - x0)[..., None], (fy - y0)[..., None]
    x0, y0 = np.clip(x0, 0, w - 1), np.clip(y0, 0, h - 1)
    x1, y1 = np.clip(x0 + 1, 0, w - 1), np.clip(y0 + 1, 0, h - 1)
    v = (1 - ay) * ((1 - ax) * a[y0, x0] + ax * a[y0, x1]) + ay * ((1 - ax) * a[y1, x0] + ax * a[y1, x1])
    q = np.clip(np.floor(v + 0.5), 0, 255).astype(np.int64) * valid[..., None]
    return q if np.asarray(src).ndim == 3 else q[..., 0]


def nearest(src, sx, sy, valid):
    """the texel that contains the position; NaN where invalid. Also returns the distance of the position to the nearest texel boundary (rounding boundary)."""
    a = np.asarray(src, np.float64)
    h, w = a.shape
    px, py = np.where(valid, sx, 0.5), np.where(valid, sy, 0.5)
    ix, iy = np.clip(np.floor(px).astype(np.int64), 0, w - 1), np.clip(np.floor(py).astype(np.int64), 0, h - 1)
    dist = np.minimum(np.abs(px - np.round(px)), np.abs(py - np.round(py)))
    return np.where(valid, a[iy, ix], np.nan), dist


def mask_values(src, sx, sy, valid, invert, threshold):
    """the mask entry: tap + quantise, threshold (>= threshold -> 255 else 0; negative keeps soft values), invert, then 0 where invalid; src None -> validity plane"""
    if src is None:
        return valid.astype(np.int64) * 255
    q = bilinear_u8(src, sx, sy, valid)
    if threshold >= 0:
        q = np.where(q >= threshold, 255, 0)
    if invert:
        q = 255 - q
    return q * valid
