"""Undistortion at load, host side: the distortion-free pinhole camera a distorted COLMAP view is resampled to. numpy, float64; nothing here
touches the GPU - the resample itself is csrc/undistort.hip, driven by the lfs_undistort_map this module fills.

The output camera keeps the size (image_target_size) and the principal point of the source, scaled to the output; only the focal lengths change, by a zoom z:

    dst_fx = fx * (dst_w / cam.width) * z        dst_fy = fy * (dst_h / cam.height) * z

Pixel centres are at +0.5 (image_to_chw_kernel, COLMAP). z comes from the image border: the rectangle of source pixel centres, shrunk by the guard GUARD = 1/64 px,
is sampled at every pixel along its four sides (and where the principal point's row / column meets a side), every sample is mapped to normalised undistorted
coordinates by inverting the lens model (Newton iteration to convergence), and per side the innermost and the outermost value of the side's coordinate are taken:

    z_valid = max(el / max(L), er / min(R), et / max(T), eb / min(B))     the smallest zoom at which every output pixel centre lands inside the source
    z_all   = min(el / min(L), er / max(R), et / min(T), eb / max(B))     the largest zoom at which every border sample still lands inside the output
    z       = clamp((1 - alpha) z_valid + alpha z_all, 0.2, 2.0)

with el = (0.5 - dst_cx) / (fx dst_w / cam.width), er the same with dst_w - 0.5, et / eb in y: the normalised positions of the outermost output pixel centres at
z = 1 (at equal source and output sizes these are (0.5 - cx) / fx ... of the source). alpha has the meaning of OpenCV's getOptimalNewCameraMatrix: 0 = no blank
pixels, 1 = no source pixel lost. A border sample the model cannot reach (a fisheye angle beyond the one up to which the polynomial grows, a radial factor <= 0.8,
which the projection itself rejects) counts as infinitely far out: it never limits z_valid and drives z_all into the clamp."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

PINHOLE, FISHEYE = 0, 2       # gsplat::CameraModelType, as CameraData.camera_model_type
GUARD = 1.0 / 64.0            # px
Z_MIN, Z_MAX = 0.2, 2.0
ICD_MIN = 0.8                 # the projection's validity criterion for the radial factor


def _loader_error(msg: str):
    from .loader import LoaderError
    return LoaderError(msg)


@dataclass
class UndistortMap:
    """One view's map: the lens model with the source intrinsics at the size of the source file, and the destination pinhole. struct() is the C mirror."""
    model: int                    # PINHOLE (with distortion) | FISHEYE
    src_width: int
    src_height: int
    dst_width: int
    dst_height: int
    src_fx: float
    src_fy: float
    src_cx: float
    src_cy: float
    radial: np.ndarray            # [6] k1 k2 k3 | k4 k5 k6 (pinhole: numerator | denominator; fisheye: k1..k4, 0, 0)
    tangential: np.ndarray        # [2]
    thin: np.ndarray              # [4]
    max_angle: float              # fisheye: the angle up to which theta * poly(theta^2) grows (inf: everywhere)
    dst_fx: float
    dst_fy: float
    dst_cx: float
    dst_cy: float
    z: float
    z_valid: float
    z_all: float

    def with_source_size(self, width: int, height: int) -> "UndistortMap":
        """the same map for a source plane of another size that shows the same picture (a depth file stored at its own resolution)"""
        import dataclasses
        ax, ay = width / float(self.src_width), height / float(self.src_height)
        return dataclasses.replace(self, src_width=int(width), src_height=int(height), src_fx=self.src_fx * ax, src_fy=self.src_fy * ay, src_cx=self.src_cx * ax,
                                   src_cy=self.src_cy * ay)

    def K(self) -> np.ndarray:
        """the destination intrinsics as loader.intrinsics lays them out"""
        K = np.zeros((3, 3), np.float32)
        K[0, 0], K[1, 1], K[0, 2], K[1, 2], K[2, 2] = self.dst_fx, self.dst_fy, self.dst_cx, self.dst_cy, 1.0
        return K

    def struct(self):
        """lfs_undistort_map"""
        from .capi import UndistortMapStruct
        s = UndistortMapStruct()
        s.model = int(self.model)
        s.src_width, s.src_height, s.dst_width, s.dst_height = int(self.src_width), int(self.src_height), int(self.dst_width), int(self.dst_height)
        s.src_fx, s.src_fy, s.src_cx, s.src_cy = self.src_fx, self.src_fy, self.src_cx, self.src_cy
        for k in range(6):
            s.radial[k] = float(self.radial[k])
        for k in range(2):
            s.tangential[k] = float(self.tangential[k])
        for k in range(4):
            s.thin[k] = float(self.thin[k])
        s.max_angle = float(min(self.max_angle, float(np.finfo(np.float32).max)))
        s.dst_fx, s.dst_fy, s.dst_cx, s.dst_cy = self.dst_fx, self.dst_fy, self.dst_cx, self.dst_cy
        return s


# ---- the lens models, float64 ------------------------------------------------------------------------------------------------------------------------------
def _pinhole_terms(k, p, s, x, y):
    """-> (xd, yd, icD, J) of the OpenCV model at normalised (x, y); J = [[dxd/dx, dxd/dy], [dyd/dx, dyd/dy]]"""
    r2 = x * x + y * y
    num = 1.0 + r2 * (k[0] + r2 * (k[1] + r2 * k[2]))
    den = 1.0 + r2 * (k[3] + r2 * (k[4] + r2 * k[5]))
    d = num / den
    dnum = k[0] + r2 * (2.0 * k[1] + 3.0 * k[2] * r2)
    dden = k[3] + r2 * (2.0 * k[4] + 3.0 * k[5] * r2)
    dd = (dnum * den - num * dden) / (den * den)                  # d(icD) / d(r^2)
    xd = d * x + 2.0 * p[0] * x * y + p[1] * (r2 + 2.0 * x * x) + r2 * (s[0] + r2 * s[1])
    yd = d * y + p[0] * (r2 + 2.0 * y * y) + 2.0 * p[1] * x * y + r2 * (s[2] + r2 * s[3])
    tx, ty = s[0] + 2.0 * s[1] * r2, s[2] + 2.0 * s[3] * r2
    J = ((d + 2.0 * x * x * dd + 2.0 * p[0] * y + 6.0 * p[1] * x + 2.0 * x * tx, 2.0 * x * y * dd + 2.0 * p[0] * x + 2.0 * p[1] * y + 2.0 * y * tx),
         (2.0 * x * y * dd + 2.0 * p[0] * x + 2.0 * p[1] * y + 2.0 * x * ty, d + 2.0 * y * y * dd + 6.0 * p[0] * y + 2.0 * p[1] * x + 2.0 * y * ty))
    return xd, yd, d, J


def _pinhole_inverse(k, p, s, xd, yd, who: str):
    """normalised distorted -> normalised undistorted, Newton to convergence; (x, y, reachable)"""
    x, y = xd.copy(), yd.copy()
    for _ in range(200):
        fx, fy, _, J = _pinhole_terms(k, p, s, x, y)
        fx, fy = fx - xd, fy - yd
        det = J[0][0] * J[1][1] - J[0][1] * J[1][0]
        if not np.all(np.isfinite(det)) or np.any(np.abs(det) < 1e-12):
            raise _loader_error(f"{who}: the distortion model folds inside the image (singular Jacobian at the border)")
        dx, dy = (fx * J[1][1] - fy * J[0][1]) / det, (fy * J[0][0] - fx * J[1][0]) / det
        x, y = x - dx, y - dy
        if max(np.abs(dx).max(), np.abs(dy).max()) < 1e-15:
            break
    fx, fy, icd, _ = _pinhole_terms(k, p, s, x, y)
    if not (np.abs(fx - xd).max() < 1e-10 and np.abs(fy - yd).max() < 1e-10):
        raise _loader_error(f"{who}: the distortion model could not be inverted at the image border (it folds inside the image)")
    return x, y, icd > ICD_MIN


def fisheye_max_angle(k) -> float:
    """the smallest positive angle at which d/dtheta [theta (1 + k1 theta^2 + .. + k4 theta^8)] = 0, inf when there is none"""
    c = [9.0 * k[3], 7.0 * k[2], 5.0 * k[1], 3.0 * k[0], 1.0]     # in t = theta^2, highest power first
    while len(c) > 1 and c[0] == 0.0:
        c = c[1:]
    if len(c) == 1:
        return float("inf")
    roots = np.roots(np.array(c, np.float64))
    t = [r.real for r in roots if abs(r.imag) < 1e-12 * max(1.0, abs(r.real)) and r.real > 0.0]
    return float(np.sqrt(min(t))) if t else float("inf")


def _fisheye_rd(k, th):
    t2 = th * th
    return th * (1.0 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))))


def _fisheye_inverse(k, max_angle, xd, yd):
    rd = np.hypot(xd, yd)
    lim = min(max_angle, np.pi / 2)
    reach = rd < _fisheye_rd(k, lim)
    th = np.where(reach, np.minimum(rd, lim), 0.0)
    for _ in range(200):
        t2 = th * th
        df = 1.0 + t2 * (3.0 * k[0] + t2 * (5.0 * k[1] + t2 * (7.0 * k[2] + t2 * 9.0 * k[3])))
        step = np.where(reach, (_fisheye_rd(k, th) - rd) / np.where(df > 0, df, 1.0), 0.0)
        th = np.clip(th - step, 0.0, lim)
        if np.abs(step).max() < 1e-15:
            break
    reach &= (th < lim) & (np.abs(_fisheye_rd(k, th) - rd) < 1e-10)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        s = np.where(rd > 0, np.tan(th) / np.where(rd > 0, rd, 1.0), 1.0)
    return xd * s, yd * s, reach


def _radial_profile_reaches(k, rd_needed: float) -> bool:
    """r * icD(r^2) grows monotonically from 0 until it has reached the farthest border sample's distorted radius"""
    r = np.linspace(0.0, 8.0 * max(rd_needed, 1e-6), 16385)
    r2 = r * r
    num = 1.0 + r2 * (k[0] + r2 * (k[1] + r2 * k[2]))
    den = 1.0 + r2 * (k[3] + r2 * (k[4] + r2 * k[5]))
    bad = (den <= 0) | (num <= 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = r * num / den
    grows = np.concatenate([[True], np.diff(f) > 0]) & ~bad
    stop = len(r) if grows.all() else int(np.argmin(grows))        # first sample that does not grow
    return bool(stop > 0 and f[stop - 1] >= rd_needed)


def _side(lo: float, hi: float, n: int, through: float) -> np.ndarray:
    """every pixel centre along a side of the guarded rectangle, its two ends, and the principal point's row / column where it crosses the side"""
    v = np.clip(np.arange(n, dtype=np.float64) + 0.5, lo, hi)
    if lo < through < hi:
        v = np.append(v, through)
    return v


def undistorted_camera(cam, src_w: int, src_h: int, dst_w: int, dst_h: int, alpha: float = 0.0) -> Optional[UndistortMap]:
    """cam: a loader.CameraData. -> the view's UndistortMap, or None for a camera without distortion (no radial or tangential term that is not zero, not a
    fisheye): such a view takes the plain resample. LoaderError for a model that folds inside the image."""
    model = int(cam.camera_model_type)
    rad = np.asarray(cam.radial_distortion, np.float64).ravel()
    tan = np.asarray(cam.tangential_distortion, np.float64).ravel()
    if model != FISHEYE and not rad.any() and not tan.any():
        return None
    who = f"camera {cam.camera_id} ({getattr(cam, 'image_name', '')})"
    if model not in (PINHOLE, FISHEYE):
        raise _loader_error(f"{who}: camera model type {model} cannot be undistorted")
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"undistort alpha must be in [0, 1] (got {alpha})")
    if rad.size > (4 if model == FISHEYE else 6) or tan.size > 2:
        raise _loader_error(f"{who}: {rad.size} radial / {tan.size} tangential coefficients")
    k, p, s = np.zeros(6), np.zeros(2), np.zeros(4)
    k[:rad.size], p[:tan.size] = rad, tan
    sx, sy = src_w / float(cam.width), src_h / float(cam.height)
    fx, fy, cx, cy = float(cam.focal_x) * sx, float(cam.focal_y) * sy, float(cam.center_x) * sx, float(cam.center_y) * sy
    dfx0, dfy0 = float(cam.focal_x) * dst_w / float(cam.width), float(cam.focal_y) * dst_h / float(cam.height)
    dcx, dcy = float(cam.center_x) * dst_w / float(cam.width), float(cam.center_y) * dst_h / float(cam.height)
    if not (fx > 0 and fy > 0):
        raise _loader_error(f"{who}: focal lengths must be positive")
    el, er, et, eb = (0.5 - dcx) / dfx0, (dst_w - 0.5 - dcx) / dfx0, (0.5 - dcy) / dfy0, (dst_h - 0.5 - dcy) / dfy0
    if not (el < 0 < er and et < 0 < eb):
        raise _loader_error(f"{who}: the principal point is outside the image")

    x0, x1, y0, y1 = 0.5 + GUARD, src_w - 0.5 - GUARD, 0.5 + GUARD, src_h - 0.5 - GUARD
    xs, ys = _side(x0, x1, src_w, cx), _side(y0, y1, src_h, cy)
    sides = {"L": (np.full_like(ys, x0), ys), "R": (np.full_like(ys, x1), ys), "T": (xs, np.full_like(xs, y0)), "B": (xs, np.full_like(xs, y1))}
    max_angle = fisheye_max_angle(k) if model == FISHEYE else float("inf")
    if model == PINHOLE:
        far = max(float(np.hypot((px - cx) / fx, (py - cy) / fy).max()) for px, py in sides.values())
        if not _radial_profile_reaches(k, far):
            raise _loader_error(f"{who}: the radial distortion is not monotonic inside the image (the model folds)")
    und = {}
    for name, (px, py) in sides.items():
        xd, yd = (px - cx) / fx, (py - cy) / fy
        x, y, reach = _pinhole_inverse(k, p, s, xd, yd, who) if model == PINHOLE else _fisheye_inverse(k, max_angle, xd, yd)
        v = x if name in "LR" else y
        und[name] = np.where(reach, v, -np.inf if name in "LT" else np.inf)
    L, R, T, B = und["L"], und["R"], und["T"], und["B"]
    if not (L.max() < 0 and R.min() > 0 and T.max() < 0 and B.min() > 0):
        raise _loader_error(f"{who}: a side of the image border crosses the principal point after undistortion (the model folds)")
    with np.errstate(divide="ignore"):
        z_valid = max(el / L.max(), er / R.min(), et / T.max(), eb / B.min())
        z_all = min(el / L.min(), er / R.max(), et / T.min(), eb / B.max())
    z = float(np.clip((1.0 - alpha) * z_valid + alpha * z_all, Z_MIN, Z_MAX))
    return UndistortMap(model, int(src_w), int(src_h), int(dst_w), int(dst_h), fx, fy, cx, cy, k, p, s, max_angle, dfx0 * z, dfy0 * z, dcx, dcy, z,
                        float(z_valid), float(z_all))
