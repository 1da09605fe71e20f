"""lichtfeld-studio_amd/undistort.py on the CPU (no GPU, no kernel): the zoom of the undistorted pinhole camera against closed forms for a radial-only lens, the
two guarantees of alpha = 0 and alpha = 1 in a float64 evaluation of the map (tests/undistort_reference.py), the cameras that yield no map, the ones that are
refused, and the clamp."""
import numpy as np
import pytest

import undistort_reference as ref
from test_gpu_undistort import MODELS, SIZES, camera_data


@pytest.fixture(scope="module")
def ud(lfs):
    from lichtfeld_studio_amd import undistort
    return undistort


def _invert_radial(k1, rd):
    """r with r (1 + k1 r^2) = rd, by bisection on the growing branch"""
    lo, hi = 0.0, (np.sqrt(-1.0 / (3.0 * k1)) if k1 < 0 else 10.0)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if mid * (1 + k1 * mid * mid) < rd else (lo, mid)
    return 0.5 * (lo + hi)


@pytest.mark.parametrize("k1", [-0.2, 0.15])
def test_radial_only_zoom_equals_its_closed_form(ud, k1):
    """A radial lens moves points along rays through the principal point. Along a side of the border the undistorted coordinate is x_d r / r_d with r_d smallest
    where the principal point's row (column) meets the side and largest at a corner: for k1 < 0 (r / r_d grows with r_d) the innermost sample of a side is the
    mid-edge and the outermost a corner, for k1 > 0 the other way round."""
    sw, sh = 67, 45
    cam = camera_data((0, [k1], []), sw, sh)
    k1 = float(cam.radial_distortion[0])   # (the coefficient as the loader holds it: float32)
    g = ud.GUARD
    fx, fy, cx, cy = cam.focal_x, cam.focal_y, cam.center_x, cam.center_y
    xl, xr, yt, yb = (0.5 + g - cx) / fx, (sw - 0.5 - g - cx) / fx, (0.5 + g - cy) / fy, (sh - 0.5 - g - cy) / fy

    def und(xd, yd):   # undistorted (x, y) of a distorted normalised point
        rd = np.hypot(xd, yd)
        s = _invert_radial(k1, rd) / rd
        return xd * s, yd * s
    mid = {"L": und(xl, 0.0)[0], "R": und(xr, 0.0)[0], "T": und(0.0, yt)[1], "B": und(0.0, yb)[1]}
    corner = {"L": [und(xl, yt)[0], und(xl, yb)[0]], "R": [und(xr, yt)[0], und(xr, yb)[0]], "T": [und(xl, yt)[1], und(xr, yt)[1]], "B": [und(xl, yb)[1], und(xr, yb)[1]]}
    e = {"L": (0.5 - cx) / fx, "R": (sw - 0.5 - cx) / fx, "T": (0.5 - cy) / fy, "B": (sh - 0.5 - cy) / fy}
    inner = {s: mid[s] if k1 < 0 else min(corner[s], key=abs) for s in "LRTB"}
    outer = {s: max(corner[s], key=abs) if k1 < 0 else mid[s] for s in "LRTB"}
    z_valid = max(e[s] / inner[s] for s in "LRTB")
    z_all = min(e[s] / outer[s] for s in "LRTB")
    m = ud.undistorted_camera(cam, sw, sh, sw, sh, 0.0)
    assert m.z_valid == pytest.approx(z_valid, rel=1e-9) and m.z_all == pytest.approx(z_all, rel=1e-9)
    assert m.z == pytest.approx(z_valid, rel=1e-12) and m.z_all < m.z_valid
    assert (m.dst_fx, m.dst_fy, m.dst_cx, m.dst_cy) == pytest.approx((fx * m.z, fy * m.z, cx, cy), rel=1e-12)
    half = ud.undistorted_camera(cam, sw, sh, sw, sh, 0.5)
    assert half.z == pytest.approx(0.5 * (z_valid + z_all), rel=1e-9)
    # a smaller output: the principal point scales with it, the focal lengths with it and z
    small = ud.undistorted_camera(cam, sw, sh, 33, 22, 0.0)
    assert (small.dst_cx, small.dst_cy) == pytest.approx((cx * 33 / sw, cy * 22 / sh), rel=1e-12)
    assert (small.dst_fx, small.dst_fy) == pytest.approx((fx * 33 / sw * small.z, fy * 22 / sh * small.z), rel=1e-12)
    assert (small.src_fx, small.src_cx, small.src_width) == (pytest.approx(fx), pytest.approx(cx), sw)


@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("size", SIZES)
def test_alpha_0_covers_every_output_pixel_and_alpha_1_keeps_every_source_pixel(ud, model, size):
    (sw, sh), (dw, dh) = size
    cam = camera_data(model, sw, sh)
    m0 = ud.undistorted_camera(cam, sw, sh, dw, dh, 0.0)
    assert ud.Z_MIN < m0.z < ud.Z_MAX and m0.z == m0.z_valid
    _, _, valid, margin = ref.evaluate(m0)
    assert valid.all() and margin.min() >= ud.GUARD / 2, margin.min()
    m1 = ud.undistorted_camera(cam, sw, sh, dw, dh, 1.0)
    assert m1.z == m1.z_all < m0.z
    # every source border sample, mapped to the output camera by inverting the model numerically (dense search over the output plane is not needed: the model
    # is evaluated forward on a fine grid of the output rectangle's border and must stay OUTSIDE the guarded source rectangle's interior there)
    t = np.linspace(0.0, 1.0, 4001)
    bx = np.concatenate([t * (dw - 1) + 0.5, t * (dw - 1) + 0.5, np.full_like(t, 0.5), np.full_like(t, dw - 0.5)])
    by = np.concatenate([np.full_like(t, 0.5), np.full_like(t, dh - 0.5), t * (dh - 1) + 0.5, t * (dh - 1) + 0.5])
    xd, yd, _ = ref.distort(m1, (bx - m1.dst_cx) / m1.dst_fx, (by - m1.dst_cy) / m1.dst_fy)
    sx, sy = xd * m1.src_fx + m1.src_cx, yd * m1.src_fy + m1.src_cy
    g = ud.GUARD
    inside = (sx > 0.5 + g + 1e-9) & (sx < sw - 0.5 - g - 1e-9) & (sy > 0.5 + g + 1e-9) & (sy < sh - 0.5 - g - 1e-9)
    assert not inside.any(), "the outermost output pixel centres read at or beyond the source border: the whole source projects inside the output"


def test_cameras_without_distortion_yield_no_map(ud):
    assert ud.undistorted_camera(camera_data((0, [], []), 67, 45), 67, 45, 67, 45) is None
    assert ud.undistorted_camera(camera_data((0, [0.0, 0.0], [0.0, 0.0]), 67, 45), 67, 45, 33, 22, 0.7) is None
    assert ud.undistorted_camera(camera_data((2, [], []), 67, 45), 67, 45, 67, 45) is not None   # an ideal fisheye is still not a pinhole


def test_a_folding_camera_is_refused_by_name(ud, lfs):
    from lichtfeld_studio_amd.loader import LoaderError
    with pytest.raises(LoaderError, match="camera 7"):   # r (1 - 1.2 r^2) peaks at r = 0.53: the border (r_d up to 0.75) cannot be reached
        ud.undistorted_camera(camera_data((0, [-1.2], []), 67, 45, cam_id=7), 67, 45, 67, 45)
    with pytest.raises(LoaderError, match="camera 8"):   # r (1 + 0.5 r^2 - r^4) peaks at 0.728 (r = 0.79), the farthest corner is at r_d = 0.78
        ud.undistorted_camera(camera_data((0, [0.5, -1.0], []), 67, 45, cam_id=8), 67, 45, 67, 45)
    with pytest.raises(ValueError):
        ud.undistorted_camera(camera_data("opencv", 67, 45), 67, 45, 67, 45, alpha=1.5)


def test_the_clamp_engages_for_a_170_degree_fisheye(ud):
    """an equidistant fisheye whose horizontal field of view is 170 degrees: tan(85 deg) = 11.4 cannot be covered by a pinhole of the same size"""
    from lichtfeld_studio_amd import loader
    sw, sh = 67, 45
    f = (sw / 2.0) / np.radians(85.0)
    cam = loader.CameraData(3, 5, 2, sw, sh, f, f, sw / 2.0, sh / 2.0, np.eye(3, dtype=np.float32), np.zeros(3, np.float32), np.zeros(4, np.float32),
                            np.zeros(0, np.float32), np.zeros(0, np.float32), "f.png", "/nonexistent/f.png")
    m = ud.undistorted_camera(cam, sw, sh, sw, sh, 0.0)
    assert ud.Z_MIN < m.z == m.z_valid < 1.0      # no blank pixels: the (shorter) vertical field of view decides, 0.974 / tan(0.974 rad)
    assert m.z_valid == pytest.approx(((sh / 2.0 - 0.5) / f) / np.tan((sh / 2.0 - 0.5 - ud.GUARD) / f), rel=1e-9)
    m = ud.undistorted_camera(cam, sw, sh, sw, sh, 1.0)
    assert m.z_all < ud.Z_MIN and m.z == ud.Z_MIN   # the corners are beyond 90 degrees (infinitely far out), the mid-edges at tan(85 deg)
    # beyond the invertible angle: the border counts as infinitely far out, z_all runs into the clamp
    cam.radial_distortion = np.asarray([-0.2, 0.0, 0.0, 0.0], np.float32)   # theta (1 - 0.2 theta^2) peaks at theta = 1.29 < 85 degrees
    m = ud.undistorted_camera(cam, sw, sh, sw, sh, 1.0)
    assert m.max_angle == pytest.approx(np.sqrt(1 / 0.6), rel=1e-6) and m.z_all == 0.0 and m.z == ud.Z_MIN
    assert ref.fisheye_max_angle(cam.radial_distortion) == pytest.approx(m.max_angle, rel=1e-9)


def test_the_struct_mirrors_the_map(ud):
    m = ud.undistorted_camera(camera_data("full_opencv", 130, 70), 130, 70, 65, 35, 0.5)
    s = m.struct()
    assert (s.model, s.src_width, s.src_height, s.dst_width, s.dst_height) == (0, 130, 70, 65, 35)
    assert list(s.radial) == [np.float32(v) for v in m.radial] and list(s.tangential) == [np.float32(v) for v in m.tangential] and list(s.thin) == [0.0] * 4
    assert (s.dst_fx, s.dst_fy, s.dst_cx, s.dst_cy) == tuple(np.float32(v) for v in (m.dst_fx, m.dst_fy, m.dst_cx, m.dst_cy))
    assert np.array_equal(m.K(), np.array([[s.dst_fx, 0, s.dst_cx], [0, s.dst_fy, s.dst_cy], [0, 0, 1]], np.float32))


def test_the_tool_refuses_alpha_without_the_flag_and_switches_the_mask_mode(capsys):
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("train_colmap_for_undistort", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "train_colmap.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    parse = lambda *a: tool.build_parser().parse_args(["-d", "x", *a])
    args = parse()
    tool.check_args(args)
    assert (args.undistort, args.undistort_alpha, args.mask_mode) == (False, 0.0, "none")
    for bad in (["--undistort-alpha", "0.5"], ["--undistort", "--undistort-alpha", "1.5"], ["--undistort", "--undistort-alpha", "-0.1"]):
        with pytest.raises(SystemExit):
            tool.check_args(parse(*bad))
    args = parse("--undistort")
    tool.check_args(args)
    assert args.mask_mode == "none"            # alpha = 0: no blank pixels, nothing to mask
    args = parse("--undistort", "--undistort-alpha", "0.5")
    tool.check_args(args)
    assert args.mask_mode == "ignore" and "becomes ignore" in capsys.readouterr().err
    args = parse("--undistort", "--undistort-alpha", "0.5", "--mask-mode", "segment")
    tool.check_args(args)
    assert args.mask_mode == "segment"
