"""CPU: the host side of masked training - the alpha-channel decoder of liblfs_io and its Pillow fallback, mask discovery, the planner's masked rows, the
configurations GutTrainer refuses, and the masked PSNR."""
import itertools
import os
import struct
import zlib

import numpy as np
import pytest
import torch


def _png(path, arr, color_type, depth):
    """arr [h,w,samples] (uint8 or uint16) -> a non-interlaced PNG of the given colour type, filter 0 on every row"""
    h, w, _ = arr.shape
    raw = b"".join(b"\x00" + (arr[y].astype(">u2") if depth == 16 else arr[y].astype(np.uint8)).tobytes() for y in range(h))

    def chunk(kind, body):
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, color_type, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))


def _pixels(h, w, samples, depth, seed):
    rng = np.random.RandomState(seed)
    return rng.randint(0, 1 << depth, size=(h, w, samples)).astype(np.uint16 if depth == 16 else np.uint8)


@pytest.mark.parametrize("depth", [8, 16])
@pytest.mark.parametrize("color_type,samples", [(6, 4), (4, 2)])
def test_alpha_channel_native_and_pillow(lfs, tmp_path, color_type, samples, depth):
    from lichtfeld_studio_amd import loader
    px = _pixels(13, 17, samples, depth, seed=color_type * 100 + depth)
    path = str(tmp_path / "a.png")
    _png(path, px, color_type, depth)
    want = (px[..., -1] >> 8).astype(np.uint8) if depth == 16 else px[..., -1]   # 16 bit: the high byte, as the RGB path reduces its samples
    got = loader.decode_mask8(path, alpha=True)
    assert got.dtype == np.uint8 and got.shape == (13, 17) and np.array_equal(got, want)
    assert np.array_equal(loader._pillow_alpha8(path), want)   # the fallback, on a file the native decoder takes: the same bytes
    # the RGB path of the same file is untouched by the alpha
    rgb = loader.decode_rgb8(path)
    assert rgb.shape == (13, 17, 3)
    assert loader.get_image_info(path)[2] == samples


def test_alpha_of_files_without_one_is_unsupported(lfs, tmp_path):
    import ctypes as C

    from PIL import Image

    from lichtfeld_studio_amd import loader
    rgb = _pixels(9, 11, 3, 8, 1)
    jpg, png = str(tmp_path / "a.jpg"), str(tmp_path / "rgb.png")
    Image.fromarray(rgb).save(jpg)
    loader.write_png(png, rgb)
    lib = loader.io_library()
    for path in (jpg, png):
        data, w, h = C.POINTER(C.c_uint8)(), C.c_int32(), C.c_int32()
        assert lib.lfs_image_load_alpha8(os.fsencode(path), C.byref(data), C.byref(w), C.byref(h)) == loader.IO_E_UNSUPPORTED
        with pytest.raises(loader.LoaderError):
            loader.decode_mask8(path, alpha=True)
    # a mask FILE is read through its first channel, whatever the format
    assert np.array_equal(loader.decode_mask8(png), rgb[..., 0])


def test_mask_discovery_order_alpha_fallback_and_size_check(lfs, tmp_path):
    from lichtfeld_studio_amd import loader
    data = tmp_path / "scene"
    (data / "images").mkdir(parents=True)
    (data / "masks").mkdir()
    rgb = _pixels(8, 10, 3, 8, 2)
    img = str(data / "images" / "frame_01.jpg.png")   # (a double extension: the three candidate names are all different)
    loader.write_png(img, rgb)
    assert loader.find_mask(img, str(data)) is None   # no file, no alpha
    m = _pixels(8, 10, 1, 8, 3)
    # <image file name>.png, <stem>.png, <stem><image ext>: a .jpg image keeps the three names apart; the later candidate is found until an earlier one exists
    img2 = str(data / "images" / "view.jpg")
    from PIL import Image
    Image.fromarray(rgb).save(img2)
    cands = [str(data / "masks" / c) for c in ("view.jpg.png", "view.png", "view.jpg")]
    Image.fromarray(m[..., 0]).save(cands[2], format="JPEG")
    assert loader.find_mask(img2, str(data)) == (cands[2], False)
    _png(cands[1], m, 0, 8)
    assert loader.find_mask(img2, str(data)) == (cands[1], False)
    _png(cands[0], m, 0, 8)
    assert loader.find_mask(img2, str(data)) == (cands[0], False)
    assert np.array_equal(loader.load_mask8(img2, (cands[0], False)), m[..., 0])
    _png(str(data / "masks" / "frame_01.jpg.png.png"), m, 0, 8)
    assert loader.find_mask(img, str(data)) == (str(data / "masks" / "frame_01.jpg.png.png"), False)
    assert loader.find_mask(img, str(data), masks_folder="other") is None     # another folder: nothing there, and the image has no alpha
    # the image's own alpha when no file is found
    rgba = _pixels(8, 10, 4, 8, 4)
    img3 = str(data / "images" / "obj.png")
    _png(img3, rgba, 6, 8)
    assert loader.find_mask(img3, str(data)) == (img3, True)
    assert np.array_equal(loader.load_mask8(img3, (img3, True)), rgba[..., 3])
    # a mask of another size than its image's source size
    _png(str(data / "masks" / "obj.png"), _pixels(4, 5, 1, 8, 5), 0, 8)
    src = loader.find_mask(img3, str(data))
    assert src == (str(data / "masks" / "obj.png"), False)
    with pytest.raises(loader.LoaderError):
        loader.load_mask8(img3, src)
    # the dataset carries the source per camera
    z = np.zeros(0, np.float32)
    cams = [loader.CameraData(1, 1, 0, 10, 8, 1.0, 1.0, 5.0, 4.0, np.eye(3, dtype=np.float32), np.zeros(3, np.float32), z, z, z, os.path.basename(p), p)
            for p in (img2, img3, img)]
    ds = loader.CameraDataset(cams, "all", data_path=str(data))
    assert ds.masks_folder == "masks" and [ds.mask_source(i) for i in range(len(ds))] == [loader.find_mask(c.image_path, str(data)) for c in cams]


def test_masked_plans_never_take_the_one_call_form(lfs):
    from lichtfeld_studio_amd.trainer import plan_step
    base = dict(rasterizer="gut", fused_l2=True, world=1, force_collectives=False, sh_sharded=False, shard_rows=0, n_views=1, loss="mse", strategy=None, refining=False,
                iteration=3000, has_shN=True, optimizer_fused=True, bilateral=False)
    assert plan_step(**base).path == "cxx_all" and plan_step(**dict(base, masked=True)).path == "cxx_views"
    assert plan_step(**dict(base, loss="l1_ssim", one_call=True)).path == "cxx_all"
    assert plan_step(**dict(base, loss="l1_ssim", one_call=True, masked=True)).path == "cxx_views"
    seen = 0
    for loss, strategy, refining, iteration, one_call, bilateral, n_views, cxx_step, world in itertools.product(
            ("mse", "l1_ssim"), (None, "mcmc"), (False, True), (500, 3000), (False, True), (False, True), (1, 2), (False, True), (1, 2)):
        kw = dict(base, loss=loss, strategy=strategy, refining=refining, iteration=iteration, one_call=one_call, bilateral=bilateral, n_views=n_views, cxx_step=cxx_step,
                  world=world)
        plain, masked = plan_step(**kw), plan_step(**dict(kw, masked=True))
        assert plan_step(**dict(kw, masked=False)) == plain          # the default is the keyword off
        assert masked.path != "cxx_all" and not masked.inline_all
        if plain.path == "cxx_all":
            seen += 1
        elif not plain.inline_all:
            assert masked == plain                                     # a step that was no one-call / all-inline form keeps its plan
    assert seen > 0
    assert plan_step(**dict(base, rasterizer="fastgs", masked=True)) == plan_step(**dict(base, rasterizer="fastgs"))
    assert plan_step(**dict(base, fused_l2=False, masked=True)).path == "autograd"


def test_configurations_masked_training_refuses(lfs):
    from lichtfeld_studio_amd import losses, scenes
    from lichtfeld_studio_amd.trainer import GutTrainer
    sc = scenes.syn_a(n=50, sh_degree=1)
    cpu = torch.device("cpu")
    with pytest.raises(ValueError, match="mask mode"):
        GutTrainer(sc, cpu, mask_mode="sometimes")
    with pytest.raises(ValueError, match="segment.*3DGUT"):
        GutTrainer(sc, cpu, rasterizer="gut", fused_l2=True, loss="l1_ssim", mask_mode="segment")
    with pytest.raises(ValueError, match="l1_ssim"):
        GutTrainer(sc, cpu, rasterizer="fastgs", loss="mse", mask_mode="segment")
    GutTrainer(sc, cpu, rasterizer="fastgs", loss="l1_ssim", mask_mode="segment")
    mask = losses.PreparedMask(torch.full((sc.height, sc.width), 255, dtype=torch.uint8), torch.tensor([1, 1]))
    target = torch.zeros(3, sc.height, sc.width)
    tr = GutTrainer(sc, cpu, loss="l1_ssim")
    with pytest.raises(ValueError, match="mask_mode"):
        tr.train_step([target], views=[0], masks=[mask])
    # several views on one rank plan to batch_views, cxx_step off plans to py_views: neither carries a mask
    tr = GutTrainer(sc, cpu, loss="l1_ssim", mask_mode="ignore", views_per_rank=2)
    tr._cxx_supported = lambda: True
    with pytest.raises(ValueError, match="batch_views"):
        tr.train_step([target, target], views=[0, 0], masks=[mask, None])
    tr = GutTrainer(sc, cpu, loss="l1_ssim", mask_mode="ignore")
    tr.cxx_step = False
    with pytest.raises(ValueError, match="py_views"):
        tr.train_step([target], views=[0], masks=[mask])
    with pytest.raises(ValueError, match="parallel"):
        tr.train_step([target], views=[0], masks=[mask, mask])


def test_masked_psnr_against_numpy(lfs):
    from lichtfeld_studio_amd import evaluate, losses
    rng = np.random.RandomState(7)
    p, t = rng.rand(3, 12, 15).astype(np.float32), rng.rand(3, 12, 15).astype(np.float32)
    m = rng.randint(0, 256, size=(12, 15)).astype(np.uint8)
    mse = (m[None].astype(np.float64) * (p.astype(np.float64) - t) ** 2).sum() / (3 * m.astype(np.float64).sum())
    want = 20 * np.log10(1 / np.sqrt(mse))
    got = evaluate.psnr(torch.from_numpy(p), torch.from_numpy(t), mask=torch.from_numpy(m))
    assert abs(got - want) < 1e-4
    pm = losses.PreparedMask(torch.from_numpy(m), torch.tensor([int(m.sum()), 0]))
    assert evaluate.psnr(torch.from_numpy(p)[None], torch.from_numpy(t)[None], mask=pm) == got
    full = evaluate.psnr(torch.from_numpy(p), torch.from_numpy(t), mask=torch.full((12, 15), 255, dtype=torch.uint8))
    assert abs(full - evaluate.psnr(torch.from_numpy(p), torch.from_numpy(t))) < 1e-4
    assert abs(got - full) > 1e-3
    with pytest.raises(ValueError):
        evaluate.psnr(torch.from_numpy(p), torch.from_numpy(t), mask=torch.zeros(3, 3))
