"""GPU parity of the undistortion stage (csrc/undistort.hip: lfs_image_undistort_u8_to_chw_f32, lfs_mask_undistort_prepare, lfs_plane_undistort_nearest_f32) against
the float64 model of tests/undistort_reference.py, the loader wiring around it, and one end-to-end check against the project's own distorted-camera renderer.
The same kernel bodies run on the wavefront emulator in tests/test_emulated_undistort.py.

Bounds (none of them taken from what the kernel gives):
  * image / mask values: where kernel and model both call the pixel valid, at most one 8-bit step apart - a position error e moves a bilinear value of 8-bit
    data by at most 2 e 255 levels, and fp32 positions at these sizes (coordinates < 130, 24-bit mantissa, a few dozen operations) are good to well under 1e-3 px,
    i.e. < 0.51 level before rounding: the rounded values differ by at most 1. At most 0.5 % of those pixels may differ at all.
  * validity: kernel and model may disagree only where the float64 position is within 1e-3 px of the source border, and on at most 0.5 % of the pixels.
  * nearest-neighbour plane: kernel and model may pick different texels only where the float64 position is within 1e-3 px of a texel (rounding) boundary, and on
    at most 0.5 % of the pixels.
  * the mask entry's two sums equal numpy's integer sums of its own output, exactly; invalid pixels are exactly 0 (NaN for the plane)."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import undistort_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SIZES = [((67, 45), (67, 45)), ((67, 45), (33, 22)), ((130, 70), (65, 35)), ((64, 4), (64, 4))]   # (sw, sh) -> (dw, dh); the last is exactly one block
MODELS = {
    "simple_radial_barrel": (0, [-0.2], []),
    "simple_radial_pincushion": (0, [0.15], []),
    "opencv": (0, [-0.25, 0.08], [0.004, -0.003]),
    "full_opencv": (0, [-0.22, 0.06, -0.01, 0.04, 0.01, 0.002], [0.003, -0.002]),   # k4..k6: the rational denominator
    "opencv_fisheye": (2, [-0.03, 0.01, -0.004, 0.001], []),
}
ALPHAS = [0.0, 0.5, 1.0]
CASES = [(s, m, a) for s in range(len(SIZES)) for m in MODELS for a in ALPHAS]
POSITION_EPS = 1e-3   # px
CAP = 0.005           # share of the pixels


def camera_data(model, sw, sh, cam_id=1):
    """a loader.CameraData: fx = 0.8 sw, fy = 0.82 sw, the principal point off the centre"""
    from lichtfeld_studio_amd import loader
    kind, radial, tangential = MODELS[model] if isinstance(model, str) else model
    return loader.CameraData(cam_id, 4, kind, sw, sh, 0.8 * sw, 0.82 * sw, 0.53 * sw, 0.46 * sh, np.eye(3, dtype=np.float32), np.zeros(3, np.float32),
                             np.asarray(radial, np.float32), np.asarray(tangential, np.float32), np.zeros(0, np.float32), f"cam{cam_id}.png", f"/nonexistent/cam{cam_id}.png")


@functools.lru_cache(maxsize=None)
def case(si, model, alpha):
    """the map, the float64 model's evaluation of it and the seeded noise sources: computed once per case, shared by the tests, never written to"""
    from lichtfeld_studio_amd import undistort
    (sw, sh), (dw, dh) = SIZES[si]
    m = undistort.undistorted_camera(camera_data(model, sw, sh), sw, sh, dw, dh, alpha)
    sx, sy, valid, margin = ref.evaluate(m.struct())
    rng = np.random.RandomState(100 * si + 10 * list(MODELS).index(model) + int(alpha * 2))
    rgb = rng.randint(0, 256, size=(sh, sw, 3)).astype(np.uint8)
    plane = rng.randint(0, 256, size=(sh, sw)).astype(np.uint8)
    depth = rng.rand(sh, sw).astype(np.float32) + 0.5
    out = dict(map=m, sx=sx, sy=sy, valid=valid, margin=margin, rgb=rgb, plane=plane, depth=depth)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _check_validity(got_valid, c, what):
    """-> the pixels both call valid. Disagreement only within POSITION_EPS of the source border, on at most CAP of the pixels."""
    assert set(np.unique(got_valid)) <= {0, 255}, what
    got = got_valid == 255
    differ = got != c["valid"]
    print(f"{what}: {int(c['valid'].sum())} of {got.size} pixels valid in the model, validity differs at {int(differ.sum())}")
    assert np.all(np.abs(c["margin"][differ]) < POSITION_EPS), (what, c["margin"][differ])
    assert differ.sum() <= CAP * got.size, (what, int(differ.sum()))
    return got & c["valid"]


def _check_values(got, want, both, what):
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))[both]
    print(f"{what}: {int((d > 0).sum())} of {d.size} jointly valid values differ, max {int(d.max()) if d.size else 0} level(s)")
    assert d.size == 0 or d.max() <= 1, (what, int(d.max()))
    assert (d > 0).sum() <= CAP * d.size, (what, int((d > 0).sum()), d.size)


@pytest.mark.parametrize("si,model,alpha", CASES)
def test_image_matches_the_f64_model(lfs, si, model, alpha):
    from lichtfeld_studio_amd import loader
    c = case(si, model, alpha)
    img, valid = loader.undistort_u8_to_chw_f32(torch.from_numpy(c["rgb"].copy()).to(DEV), c["map"])
    img, valid = img.cpu().numpy(), valid.cpu().numpy()
    (dw, dh) = SIZES[si][1]
    assert img.shape == (3, dh, dw) and valid.shape == (dh, dw)
    both = _check_validity(valid, c, "image")
    levels = np.rint(img.astype(np.float64) * 255.0).astype(np.int64)
    assert np.array_equal(img, (levels / 255.0).astype(np.float32)), "every value is an 8-bit level / 255"
    assert np.all(img[:, valid == 0] == 0.0), "invalid pixels are exactly 0"
    want = ref.bilinear_u8(c["rgb"], c["sx"], c["sy"], c["valid"])
    _check_values(levels.transpose(1, 2, 0), want, both[..., None].repeat(3, -1), "image")
    if alpha == 0.0:
        assert valid.min() == 255, "alpha = 0: no blank pixel"


@pytest.mark.parametrize("si,model,alpha", CASES)
def test_mask_entry_matches_the_f64_model_and_its_sums_are_exact(lfs, si, model, alpha):
    from lichtfeld_studio_amd import loader
    c = case(si, model, alpha)
    (dw, dh) = SIZES[si][1]
    _, valid = loader.undistort_u8_to_chw_f32(torch.from_numpy(c["rgb"].copy()).to(DEV), c["map"])
    src = torch.from_numpy(c["plane"].copy()).to(DEV)
    for invert, threshold in [(False, -1), (True, -1), (False, 128), (True, 128)]:
        pm = loader.undistort_mask(src, c["map"], invert, threshold)
        got, sums = pm.mask_u8.cpu().numpy(), pm.sums.cpu().numpy()
        crop = got[5:dh - 5, 5:dw - 5] if (dh > 10 and dw > 10) else got
        assert sums.tolist() == [int(got.astype(np.int64).sum()), int(crop.astype(np.int64).sum())], (invert, threshold)
        assert np.all(got[valid.cpu().numpy() == 0] == 0), "blank pixels stay 0, inverted or not"
        want = ref.mask_values(c["plane"], c["sx"], c["sy"], c["valid"], invert, threshold)
        both = (valid.cpu().numpy() == 255) & c["valid"]
        if threshold < 0:
            _check_values(got, want, both, f"mask invert={invert}")
        else:   # a binarised value may flip only where the soft value is within one level of the threshold
            soft = ref.bilinear_u8(c["plane"], c["sx"], c["sy"], c["valid"])
            flip = (got != want) & both
            assert np.all(np.abs(soft[flip] - threshold) <= 1) and flip.sum() <= CAP * both.sum(), (invert, threshold, int(flip.sum()))
            assert set(np.unique(got)) <= {0, 255}
    # no mask file: the validity plane of the image entry, bit for bit, with its sums
    pm = loader.undistort_mask(None, c["map"], True, 77, device=DEV)
    got, sums = pm.mask_u8.cpu().numpy(), pm.sums.cpu().numpy()
    assert np.array_equal(got, valid.cpu().numpy())
    crop = got[5:dh - 5, 5:dw - 5] if (dh > 10 and dw > 10) else got
    assert sums.tolist() == [int(got.astype(np.int64).sum()), int(crop.astype(np.int64).sum())]


@pytest.mark.parametrize("si,model,alpha", CASES)
def test_plane_entry_picks_the_models_texel(lfs, si, model, alpha):
    from lichtfeld_studio_amd import loader
    c = case(si, model, alpha)
    _, valid = loader.undistort_u8_to_chw_f32(torch.from_numpy(c["rgb"].copy()).to(DEV), c["map"])
    valid = valid.cpu().numpy() == 255
    got = loader.undistort_plane_nearest(torch.from_numpy(c["depth"].copy()).to(DEV), c["map"]).cpu().numpy()
    assert np.array_equal(np.isnan(got), ~valid), "NaN exactly where the image entry calls the pixel invalid"
    want, dist = ref.nearest(c["depth"], c["sx"], c["sy"], c["valid"])
    both = valid & c["valid"]
    differ = both & (got != want.astype(np.float32))
    print(f"plane: {int(differ.sum())} of {int(both.sum())} picks differ")
    assert np.all(dist[differ] < POSITION_EPS), dist[differ]
    assert differ.sum() <= CAP * got.size


def test_a_depth_file_of_another_size_goes_through_the_same_map(lfs):
    """preload_depths hands the plane entry a file at its own resolution: the map's source intrinsics are scaled to it"""
    from lichtfeld_studio_amd import loader
    c = case(0, "opencv", 0.5)
    m2 = c["map"].with_source_size(134, 90)
    sx, sy, valid, _ = ref.evaluate(m2.struct())
    depth = np.random.RandomState(5).rand(90, 134).astype(np.float32)
    got = loader.undistort_plane_nearest(torch.from_numpy(depth).to(DEV), c["map"]).cpu().numpy()
    want, dist = ref.nearest(depth, sx, sy, valid)
    ok = valid & ~np.isnan(got)
    assert (np.isnan(got) != ~valid).sum() <= CAP * got.size
    differ = ok & (got != want.astype(np.float32))
    assert np.all(dist[differ] < POSITION_EPS) and differ.sum() <= CAP * got.size


def test_entry_points_refuse_bad_arguments_before_any_launch(lfs):
    from lichtfeld_studio_amd import capi
    lib = capi.load_library()
    c = case(0, "opencv", 0.0)
    good = c["map"].struct()
    src = torch.from_numpy(c["rgb"].copy()).to(DEV)
    plane = torch.from_numpy(c["plane"].copy()).to(DEV)
    depth = torch.from_numpy(c["depth"].copy()).to(DEV)
    dw, dh = good.dst_width, good.dst_height
    img = torch.full((3, dh, dw), -7.0, device=DEV)
    val = torch.full((dh, dw), 9, dtype=torch.uint8, device=DEV)
    msk = torch.full((dh, dw), 9, dtype=torch.uint8, device=DEV)
    sums = torch.full((2,), -5, dtype=torch.int64, device=DEV)
    out = torch.full((dh, dw), -7.0, device=DEV)
    p, st = capi.ptr, capi.stream()

    def bad_maps():
        for field, value in [("src_width", 0), ("src_height", 0), ("dst_width", 0), ("dst_height", 0), ("src_fx", 0.0), ("src_fy", -1.0), ("dst_fx", 0.0),
                             ("dst_fy", float("nan")), ("model", 1), ("src_width", 1 << 30)]:
            s = c["map"].struct()
            setattr(s, field, value)
            yield field, s
        s = case(0, "opencv_fisheye", 0.0)["map"].struct()
        s.max_angle = 0.0
        yield "max_angle", s

    E = -1
    for field, s in bad_maps():
        assert lib.lfs_image_undistort_u8_to_chw_f32(C.byref(s), p(src), p(img), p(val), st) == E, field
        assert lib.lfs_mask_undistort_prepare(C.byref(s), p(plane), p(msk), C.c_uint32(0), C.c_int32(-1), p(sums), st) == E, field
        assert lib.lfs_plane_undistort_nearest_f32(C.byref(s), p(depth), p(out), st) == E, field
    assert lib.lfs_image_undistort_u8_to_chw_f32(None, p(src), p(img), p(val), st) == E
    assert lib.lfs_image_undistort_u8_to_chw_f32(C.byref(good), None, p(img), p(val), st) == E
    assert lib.lfs_image_undistort_u8_to_chw_f32(C.byref(good), p(src), None, p(val), st) == E
    assert lib.lfs_image_undistort_u8_to_chw_f32(C.byref(good), p(src), p(img), None, st) == E
    assert lib.lfs_mask_undistort_prepare(None, p(plane), p(msk), C.c_uint32(0), C.c_int32(-1), p(sums), st) == E
    assert lib.lfs_mask_undistort_prepare(C.byref(good), p(plane), None, C.c_uint32(0), C.c_int32(-1), p(sums), st) == E
    assert lib.lfs_mask_undistort_prepare(C.byref(good), p(plane), p(msk), C.c_uint32(0), C.c_int32(-1), None, st) == E
    assert lib.lfs_plane_undistort_nearest_f32(None, p(depth), p(out), st) == E
    assert lib.lfs_plane_undistort_nearest_f32(C.byref(good), None, p(out), st) == E
    assert lib.lfs_plane_undistort_nearest_f32(C.byref(good), p(depth), None, st) == E
    torch.cuda.synchronize()
    assert bool((img == -7.0).all()) and bool((val == 9).all()) and bool((msk == 9).all()) and bool((out == -7.0).all()) and sums.tolist() == [-5, -5]


# ---- the loader around the kernels ---------------------------------------------------------------------------------------------------------------------------
def _small_colmap(tmp):
    from test_gpu_dataprep import _synthetic_colmap
    return _synthetic_colmap(str(tmp), W=64, H=48, n_views=3, n_pts=300)[0]


def _add_masks(base):
    from lichtfeld_studio_amd import loader
    os.makedirs(os.path.join(base, "masks"), exist_ok=True)
    rng = np.random.RandomState(3)
    for name in sorted(os.listdir(os.path.join(base, "images"))):
        loader.write_png(os.path.join(base, "masks", name + ".png"), rng.randint(0, 256, size=(48, 64, 1)).astype(np.uint8).repeat(3, -1))


def test_a_pinhole_dataset_is_untouched_by_the_option(lfs, tmp_path):
    """undistort=True on cameras without distortion: the old entry points, bit for bit"""
    from lichtfeld_studio_amd import loader
    base = _small_colmap(tmp_path)
    _add_masks(base)
    res = []
    for on in (False, True):
        scene, ds, _ = loader.colmap_scene(base, "images", split="all", sh_degree=1, device=DEV, undistort=on, undistort_alpha=0.5 if on else 0.0)
        assert all(ds.undistort_map(k) is None for k in range(len(ds)))
        targets, valids = loader.preload(ds, DEV, return_valid=True)
        assert valids == [None] * len(ds)
        res.append((scene.Ks.cpu(), targets, loader.preload_masks(ds, DEV, False, 100)))
    (K0, t0, m0), (K1, t1, m1) = res
    assert torch.equal(K0, K1) and len(t0) == len(t1) == 3
    for a, b in zip(t0, t1):
        assert torch.equal(a, b)
    for a, b in zip(m0, m1):
        assert a is not None and torch.equal(a.mask_u8, b.mask_u8) and torch.equal(a.sums, b.sums)


OPENCV_PARAMS = [-0.25, 0.08, 0.004, -0.003]   # k1 k2 p1 p2


def _distort_colmap(base):
    """rewrite cameras.bin of a pinhole COLMAP directory as the OPENCV model (id 4) with distortion; the images stay what they are"""
    from oracle import colmap_io as oc
    from lichtfeld_studio_amd import loader
    cam = loader.read_colmap_cameras_and_images(base, "images")[0][0]
    oc.write_cameras_bin(os.path.join(base, "sparse", "0", "cameras.bin"),
                         [(1, 4, cam.width, cam.height, [float(cam.focal_x), float(cam.focal_y), float(cam.center_x), float(cam.center_y), *OPENCV_PARAMS])])


def test_a_distorted_dataset_without_the_option_loads_as_before_and_with_it_through_the_maps(lfs, tmp_path):
    from lichtfeld_studio_amd import loader
    base = _small_colmap(tmp_path)
    _distort_colmap(base)
    scene, ds, _ = loader.colmap_scene(base, "images", split="all", sh_degree=1, device=DEV)
    assert not ds.undistort and ds.undistort_map(0) is None
    targets = loader.preload(ds, DEV)
    for k, tgt in enumerate(targets):   # what the parent commit computes: the plain resample and the plain pinhole K
        cam = ds.cameras[ds.indices[k]]
        assert len(cam.radial_distortion) == 2 and len(cam.tangential_distortion) == 2
        assert torch.equal(tgt, loader.u8_to_chw_f32(torch.from_numpy(loader.decode_rgb8(cam.image_path)).to(DEV)))
        assert np.array_equal(scene.Ks[k].cpu().numpy(), loader.intrinsics(cam, 64, 48))
    assert loader.preload_masks(ds, DEV) == [None] * len(ds)
    # with the option: every view has a map, Scene.Ks holds its destination intrinsics, preload goes through the new entry
    scene_u, ds_u, _ = loader.colmap_scene(base, "images", split="all", sh_degree=1, device=DEV, undistort=True, undistort_alpha=0.5)
    tu, valids = loader.preload(ds_u, DEV, return_valid=True)
    masks = loader.preload_masks(ds_u, DEV)
    for k in range(len(ds_u)):
        m = ds_u.undistort_map(k)
        assert m is not None and m.z_valid > m.z > m.z_all
        assert np.array_equal(scene_u.Ks[k].cpu().numpy(), m.K()) and not np.array_equal(m.K(), loader.intrinsics(ds_u.cameras[ds_u.indices[k]], 64, 48))
        img, valid = loader.undistort_u8_to_chw_f32(torch.from_numpy(loader.decode_rgb8(ds_u.cameras[ds_u.indices[k]].image_path)).to(DEV), m)
        assert torch.equal(tu[k], img) and torch.equal(valids[k], valid) and 0 < int((valid == 0).sum()) < valid.numel()
        assert torch.equal(masks[k].mask_u8, valid), "alpha > 0 and no mask file: the validity plane is the mask"
        cam, one = ds_u.get(k, DEV)
        assert torch.equal(one, img)
    ds_0 = loader.CameraDataset(ds_u.cameras, "all", undistort=True, undistort_alpha=0.0, data_path=base)
    assert loader.preload_masks(ds_0, DEV) == [None] * len(ds_0), "alpha = 0 and no mask file: every pixel is covered, the view stays unmasked"


# ---- end to end (GPU only: the 3DGUT renderer is the witness) ------------------------------------------------------------------------------------------------
def _psnr(a, b, where=None):
    d = (np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2
    return float(10.0 * np.log10(1.0 / (d.mean() if where is None else d[:, where].mean())))


def _distorted_camera(cam, W, H):
    from lichtfeld_studio_amd.rasterizer import Camera
    k1, k2, p1, p2 = OPENCV_PARAMS
    return Camera(cam.world_view_transform, cam.K, W, H, radial_distortion=torch.tensor([[k1, k2]], device=DEV), tangential_distortion=torch.tensor([[p1, p2]], device=DEV))


def _render_u8(camera, tr):
    from lichtfeld_studio_amd.rasterizer import rasterize
    with torch.no_grad():
        img = rasterize(camera, tr.model, tr.bg, 1.0, False, False).image
    return (img.clamp(0, 1).permute(1, 2, 0) * 255 + 0.5).to(torch.uint8).contiguous()


def test_undistorting_a_distorted_render_gives_the_pinhole_render(lfs):
    """The project's own distorted-camera renderer (the 3DGUT rasterizer with OPENCV coefficients) draws a fixed scene; the 8-bit image is undistorted at alpha = 0
    and compared with the pinhole render of the same scene at the map's destination intrinsics. The PSNR is not fixed in advance: it must lie within 0.1 dB of
    the PSNR the float64 model's undistortion of the SAME 8-bit input reaches (the kernel is held to the model, not to itself), and undistorting must beat not
    undistorting. LFS_UNDISTORT_REPORT=<file>: both values are written there as JSON (profiles/r15/undistort.json)."""
    from lichtfeld_studio_amd import loader, scenes, undistort
    from lichtfeld_studio_amd.rasterizer import Camera
    from lichtfeld_studio_amd.trainer import GutTrainer
    W, H = 96, 64
    sc = scenes._syn_box("SYN-U", 11, 400, W, H, 72.0, 1, sh_degree=1)
    sc.raw_scales += float(np.log(8.0))
    tr = GutTrainer(sc, torch.device(DEV), iterations=10)
    cam = tr.camera(0)
    K = cam.K[0].cpu().numpy()
    k1, k2, p1, p2 = OPENCV_PARAMS
    cd = loader.CameraData(1, 4, 0, W, H, float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), np.eye(3, dtype=np.float32), np.zeros(3, np.float32),
                           np.asarray([k1, k2], np.float32), np.asarray([p1, p2], np.float32), np.zeros(0, np.float32), "v.png", "/nonexistent/v.png")
    u8 = _render_u8(_distorted_camera(cam, W, H), tr)
    m = undistort.undistorted_camera(cd, W, H, W, H, 0.0)
    got, valid = loader.undistort_u8_to_chw_f32(u8, m)
    assert int(valid.min()) == 255
    pin = _render_u8(Camera(cam.world_view_transform, torch.from_numpy(m.K())[None].to(DEV), W, H), tr).permute(2, 0, 1).cpu().numpy() / 255.0
    sx, sy, ok, _ = ref.evaluate(m.struct())
    model = ref.bilinear_u8(u8.cpu().numpy(), sx, sy, ok).transpose(2, 0, 1) / 255.0
    psnr_kernel, psnr_model = _psnr(got.cpu().numpy(), pin), _psnr(model, pin)
    psnr_raw = _psnr(u8.permute(2, 0, 1).cpu().numpy() / 255.0, pin)
    print(f"undistorted vs pinhole render: kernel {psnr_kernel:.3f} dB, float64 model {psnr_model:.3f} dB; not undistorted {psnr_raw:.3f} dB; z {m.z:.4f}")
    path = os.environ.get("LFS_UNDISTORT_REPORT")
    if path:   # (the file is shared with tools/time_undistort.py: extended, not replaced)
        report = json.load(open(path)) if os.path.exists(path) else {}
        report["end_to_end"] = {"psnr_kernel_db": round(psnr_kernel, 4), "psnr_f64_model_db": round(psnr_model, 4), "psnr_not_undistorted_db": round(psnr_raw, 4),
                                "z": round(m.z, 6), "size": [W, H], "gaussians": 400, "opencv_k1_k2_p1_p2": OPENCV_PARAMS,
                                "what": "distorted 3DGUT render, 8 bit, undistorted at alpha = 0, against the pinhole 3DGUT render at the map's destination intrinsics"}
        with open(path, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")
    assert abs(psnr_kernel - psnr_model) < 0.1, (psnr_kernel, psnr_model)
    assert psnr_kernel > psnr_raw, (psnr_kernel, psnr_raw)


def _distorted_colmap(tmp_path, W=96, H=64, V=6):
    """a COLMAP directory (OPENCV camera model) whose images the 3DGUT renderer drew through that lens -> its path"""
    from oracle import colmap_io as oc
    from scipy.spatial.transform import Rotation
    from lichtfeld_studio_amd import loader, scenes
    from lichtfeld_studio_amd.trainer import GutTrainer
    sc = scenes._syn_box("SYN-UD", 7, 1500, W, H, 72.0, V, sh_degree=1)
    sc.raw_scales += float(np.log(8.0))
    src = GutTrainer(sc, torch.device(DEV), iterations=10)
    base = str(tmp_path / "scene")
    os.makedirs(os.path.join(base, "sparse", "0"))
    os.makedirs(os.path.join(base, "images"))
    images = []
    for v in range(V):
        loader.write_png(os.path.join(base, "images", f"v{v:02d}.png"), _render_u8(_distorted_camera(src.camera(v), W, H), src).cpu().numpy())
        mat = sc.viewmats[v].double().cpu().numpy()
        q = Rotation.from_matrix(mat[:3, :3]).as_quat()
        images.append((v + 1, [q[3], q[0], q[1], q[2]], list(mat[:3, 3]), 1, f"v{v:02d}.png"))
    K = sc.Ks[0]
    oc.write_cameras_bin(os.path.join(base, "sparse", "0", "cameras.bin"), [(1, 4, W, H, [float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), *OPENCV_PARAMS])])
    oc.write_images_bin(os.path.join(base, "sparse", "0", "images.bin"), images)
    xyz = sc.means.cpu().numpy()[::2]
    rgb = np.clip((sc.sh0[::2, 0].cpu().numpy() * 0.28209479177387814 + 0.5) * 255, 0, 255).astype(np.uint8)
    oc.write_points3d_bin(os.path.join(base, "sparse", "0", "points3D.bin"), xyz, rgb)
    return base


def test_training_on_a_distorted_colmap_directory_with_undistortion(lfs, tmp_path):
    """a COLMAP directory whose images were taken through an OPENCV lens (the 3DGUT renderer draws them) -> colmap_scene(undistort=True) -> a few fastgs steps:
    finite, decreasing loss"""
    from lichtfeld_studio_amd import loader
    from lichtfeld_studio_amd.trainer import GutTrainer
    W, H, V = 96, 64, 6
    base = _distorted_colmap(tmp_path, W, H, V)
    scene, ds, scale = loader.colmap_scene(base, "images", split="all", sh_degree=1, device=DEV, undistort=True)
    assert all(ds.undistort_map(k) is not None for k in range(V)) and (scene.width, scene.height) == (W, H)
    targets, valids = loader.preload(ds, DEV, return_valid=True)
    assert all(int(v.min()) == 255 for v in valids)
    tr = GutTrainer(scene, torch.device(DEV), iterations=200, rasterizer="fastgs", loss="l1_ssim")
    losses = [float(tr.train_step([targets[k % V]], views=[k % V])) for k in range(60)]
    assert np.isfinite(losses).all() and np.mean(losses[-V:]) < np.mean(losses[:V]), (losses[:V], losses[-V:])


def _run_tool(base, out, *extra):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "train_colmap.py"), "-d", base, "--strategy", "none", "--sh-degree", "1", "--test-every", "3", "-o", out,
                        *extra], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1]), r.stderr


def test_the_tool_undistorts_training_and_held_out_views(lfs, tmp_path):
    """tools/train_colmap.py --undistort --undistort-alpha 0.5 --eval: blank pixels leave the loss (the mask mode is switched and said so), the held-out views go
    through the same kind of map, the JSON reports the undistorted views and the range of z"""
    res, err = _run_tool(_distorted_colmap(tmp_path), str(tmp_path / "run"), "-i", "20", "--eval", "--undistort", "--undistort-alpha", "0.5")
    assert "--mask-mode none becomes ignore" in err and "IGNORED" not in err
    assert res["undistorted_views"] == res["images"] == 4 and res["val_images"] == 2 and res["undistort_alpha"] == 0.5 and res["mask_mode"] == "ignore"
    assert res["masked_views"] == 4, "no mask files: every view's validity plane is its mask"
    lo, hi = res["undistort_z"]
    assert 0.2 < lo <= hi < 1.0 and np.isfinite(res["psnr"])


def test_the_tool_warns_when_it_ignores_distortion(lfs, tmp_path):
    res, err = _run_tool(_distorted_colmap(tmp_path), str(tmp_path / "run"), "-i", "2")
    assert "have lens distortion, which is being IGNORED" in err and "--undistort" in err
    assert "undistorted_views" not in res and "mask_mode" not in res
