"""CPU: the host side of depth supervision - lfs_image_load_gray16 of liblfs_io.so on 16-bit PNGs written here with zlib + struct, the depth file
discovery and depth_params.json handling of loader.py, and the argument parsing of tools/train_colmap.py. No GPU, no device library."""
import importlib.util
import json
import os
import struct
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _chunk(kind: bytes, body: bytes) -> bytes:
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)


def _write_png(path, samples, bit_depth=16, colour_type=0, filters=None):
    """a non-interlaced PNG from an integer array [h,w] (greyscale) or [h,w,c]; filters: one PNG filter type per row (default 0), applied here"""
    a = np.asarray(samples)
    h, w = a.shape[:2]
    ch = 1 if a.ndim == 2 else a.shape[2]
    bps = bit_depth // 8
    rows = a.reshape(h, w * ch).astype(">u2" if bps == 2 else np.uint8).view(np.uint8).reshape(h, w * ch * bps)
    bpp = ch * bps
    raw, prev = bytearray(), np.zeros(rows.shape[1], np.int32)
    for y in range(h):
        cur = rows[y].astype(np.int32)
        ft = 0 if filters is None else filters[y % len(filters)]
        left = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]])
        ul = np.concatenate([np.zeros(bpp, np.int32), prev[:-bpp]])
        if ft == 0:
            pred = np.zeros_like(cur)
        elif ft == 1:
            pred = left
        elif ft == 2:
            pred = prev
        elif ft == 3:
            pred = (left + prev) >> 1
        else:
            p = left + prev - ul
            pa, pb, pc = np.abs(p - left), np.abs(p - prev), np.abs(p - ul)
            pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, prev, ul))
        raw += bytes([ft]) + ((cur - pred) & 0xFF).astype(np.uint8).tobytes()
        prev = cur
    ihdr = struct.pack(">IIBBBBB", w, h, bit_depth, colour_type, 0, 0, 0)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(bytes(raw))) + _chunk(b"IEND", b""))


def test_gray16_keeps_both_bytes(lfs, tmp_path):
    from lichtfeld_studio_amd import loader
    edge = np.array([[0, 1, 255, 256, 65535], [65535, 256, 255, 1, 0], [0x1234, 0xFF00, 0x00FF, 0x8000, 0x7FFF]], np.uint16)
    p = str(tmp_path / "edge.png")
    _write_png(p, edge)
    got = loader.decode_gray16(p)
    assert got.dtype == np.uint16 and got.shape == (3, 5) and np.array_equal(got, edge)
    # every scanline filter, an odd size, every low byte
    rng = np.random.RandomState(0)
    big = rng.randint(0, 65536, size=(11, 37)).astype(np.uint16)
    big[0, :] = np.arange(37) * 7 + 250                                # values around the byte boundary
    q = str(tmp_path / "big.png")
    _write_png(q, big, filters=[0, 1, 2, 3, 4])
    assert np.array_equal(loader.decode_gray16(q), big)
    assert np.array_equal(loader.load_depth(q), (big.astype(np.float64) / 65536.0).astype(np.float32))
    # the 8-bit path is what it was: the high byte, replicated to RGB
    rgb = loader.decode_rgb8(q)
    assert rgb.shape == (11, 37, 3) and np.array_equal(rgb[..., 0], (big >> 8).astype(np.uint8)) and np.array_equal(rgb[..., 0], rgb[..., 2])
    # not a 16-bit greyscale file: refused, not reduced
    for name, arr, depth, ct in (("g8.png", (big >> 8).astype(np.uint8), 8, 0), ("rgb16.png", np.stack([big] * 3, -1), 16, 2), ("ga16.png", np.stack([big] * 2, -1), 16, 4)):
        r = str(tmp_path / name)
        _write_png(r, arr, depth, ct)
        assert loader.decode_rgb8(r).shape == (11, 37, 3)             # (a valid PNG for the 8-bit decoder)
        with pytest.raises(loader.LoaderError):
            loader.decode_gray16(r)
    with pytest.raises(loader.LoaderError):
        loader.decode_gray16(str(tmp_path / "missing.png"))
    with open(str(tmp_path / "cut.png"), "wb") as f:
        f.write(open(p, "rb").read()[:40])
    with pytest.raises(loader.LoaderError):
        loader.decode_gray16(str(tmp_path / "cut.png"))


def test_find_depth_and_depth_params(lfs, tmp_path):
    from lichtfeld_studio_amd import loader
    data = tmp_path / "scene"
    (data / "depths").mkdir(parents=True)
    (data / "images").mkdir()
    img = lambda n: str(data / "images" / n)
    a = (np.arange(12, dtype=np.float32).reshape(3, 4) + 1) / 8
    np.save(str(data / "depths" / "a.npy"), a)
    _write_png(str(data / "depths" / "b.png"), np.full((3, 4), 32768, np.uint16))
    np.save(str(data / "depths" / "c.npy"), a)
    _write_png(str(data / "depths" / "c.png"), np.full((3, 4), 1, np.uint16))
    assert loader.find_depth(img("a.jpg"), str(data)) == str(data / "depths" / "a.npy")
    assert loader.find_depth(img("b.JPG"), str(data)) == str(data / "depths" / "b.png")
    assert loader.find_depth(img("c.png"), str(data)) == str(data / "depths" / "c.npy")          # the float file wins
    assert loader.find_depth(img("d.jpg"), str(data)) is None
    assert loader.find_depth(img("a.jpg"), str(data), "nowhere") is None and loader.find_depth(img("a.jpg"), None) is None and loader.find_depth(img("a.jpg"), str(data), None) is None
    assert np.array_equal(loader.load_depth(str(data / "depths" / "a.npy")), a) and float(loader.load_depth(str(data / "depths" / "b.png"))[0, 0]) == 0.5
    for shape in ((1, 3, 4), (3, 4, 1), (1, 1, 4), (1, 3, 1), (1, 1, 1)):     # a channel axis of one is dropped, a spatial axis of one is kept
        np.save(str(data / "depths" / "chan.npy"), np.arange(np.prod(shape), dtype=np.float32).reshape(shape))
        got = loader.load_depth(str(data / "depths" / "chan.npy"))
        want = shape[1:] if shape[0] == 1 else shape[:2]
        assert got.shape == want and np.array_equal(got.reshape(-1), np.arange(np.prod(shape), dtype=np.float32)), (shape, got.shape)
    np.save(str(data / "depths" / "bad.npy"), np.zeros((2, 3, 4), np.float32))
    with pytest.raises(loader.LoaderError):
        loader.load_depth(str(data / "depths" / "bad.npy"))
    # depth_params.json: t = v * scale + offset; no entry or scale <= 0 -> no target
    pj = str(data / "depth_params.json")
    with open(pj, "w") as f:
        json.dump({"a": {"scale": 2.0, "offset": 0.25, "med_scale": 1.0}, "b": {"scale": 0.0, "offset": 0.0}, "c": {"scale": -1.0, "offset": 3.0}, "junk": 5}, f)
    params = loader.load_depth_params(pj)
    assert params == {"a": (2.0, 0.25), "b": (0.0, 0.0), "c": (-1.0, 3.0)}
    assert loader.load_depth_params(None) is None and loader.load_depth_params(str(data / "none.json")) is None
    assert np.array_equal(loader.depth_target(str(data / "depths" / "a.npy"), "a", params), a * 2.0 + 0.25)
    assert loader.depth_target(str(data / "depths" / "b.png"), "b", params) is None
    assert loader.depth_target(str(data / "depths" / "c.npy"), "c", params) is None
    assert loader.depth_target(str(data / "depths" / "a.npy"), "zzz", params) is None
    assert np.array_equal(loader.depth_target(str(data / "depths" / "a.npy"), "zzz", None), a)  # no table: the file's values are the target
    # the dataset hands the source on
    z3, z0 = np.zeros(3, np.float32), np.zeros(0, np.float32)
    cams = [loader.CameraData(0, 1, 0, 4, 3, 1.0, 1.0, 2.0, 1.5, np.eye(3, dtype=np.float32), z3, z0, z0, z0, n, img(n)) for n in ("a.jpg", "d.jpg")]
    ds = loader.CameraDataset(cams, "all", data_path=str(data))
    assert ds.depth_source(0) == str(data / "depths" / "a.npy") and ds.depth_source(1) is None
    assert loader.CameraDataset(cams, "all", data_path=str(data), depths_folder=None).depth_source(0) is None


def _tool():
    spec = importlib.util.spec_from_file_location("train_colmap_tool", os.path.join(ROOT, "tools", "train_colmap.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_colmap_depth_arguments(tmp_path):
    tool = _tool()
    ap = tool.build_parser()
    a = ap.parse_args(["-d", "x"])
    assert a.depth_loss == "none" and a.depths_folder == "depths" and a.depth_params is None and (a.depth_weight_init, a.depth_weight_final) == (1.0, 0.01)
    tool.check_args(a)
    a = ap.parse_args(["-d", "x", "--depths-folder", "mono", "--depth-loss", "invdepth", "--depth-weight-init", "0.5", "--depth-weight-final", "0.002", "--depth-params", "p.json"])
    assert (a.depths_folder, a.depth_loss, a.depth_weight_init, a.depth_weight_final, a.depth_params) == ("mono", "invdepth", 0.5, 0.002, "p.json")
    tool.check_args(a)
    assert tool.depth_params_path(a) == "p.json"
    assert ap.parse_args(["-d", "x", "--depth-loss", "depth"]).depth_loss == "depth"
    with pytest.raises(SystemExit):
        ap.parse_args(["-d", "x", "--depth-loss", "median"])
    with pytest.raises(SystemExit, match="not wired into the 3DGUT route"):
        tool.check_args(ap.parse_args(["-d", "x", "--depth-loss", "invdepth", "--gut"]))
    with pytest.raises(SystemExit, match="must be > 0"):
        tool.check_args(ap.parse_args(["-d", "x", "--depth-loss", "invdepth", "--depth-weight-final", "0"]))
    with pytest.raises(SystemExit, match="--antialiasing is not wired into the 3DGUT route"):
        tool.check_args(ap.parse_args(["-d", "x", "--antialiasing", "--gut"]))               # (the earlier refusals are where they were)
    # the default location of depth_params.json
    d = tmp_path / "s"
    (d / "sparse" / "0").mkdir(parents=True)
    a = ap.parse_args(["-d", str(d), "--depth-loss", "invdepth"])
    assert tool.depth_params_path(a) is None
    (d / "sparse" / "0" / "depth_params.json").write_text("{}")
    assert tool.depth_params_path(a) == str(d / "sparse" / "0" / "depth_params.json")
