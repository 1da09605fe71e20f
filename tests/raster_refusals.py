"""What the eight C entries of the 3DGUT rasterizer's host layer refuse, and with which code: the forward, the five backwards, lfs_gut_finish_grads and
lfs_gut_finish_adam (csrc/raster.hip), called through ctypes as a foreign caller would. One body, two runners: tests/test_emulated_raster_refusals.py (the library
built as host code, tests/emul_util.py) and tests/test_gpu_raster.py (the real library).

Scene: 8 Gaussians in front of one pinhole camera, 16x16 image, tile 16, three channels, global shutter; the tile lists come from the package's own intersection
operators. A valid call of every entry returns 0. Then each row below changes ONE argument of that valid call, must return the listed code, and must leave every
output buffer - the workspace included - at the sentinel it was filled with: a call is refused before anything is launched or cleared, so the bogus sizes of some
rows (2^26 Gaussians, 2^29 intersections) need no allocation."""
import ctypes as C

import torch

DEV = "cuda:0"
N, W, H, TILE = 8, 16, 16, 16
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
SENTINEL_BYTE = 0x5A

_SCENE = [("means", "ptr"), ("quats", "ptr"), ("scales", "ptr"), ("colors", "ptr"), ("opacities", "ptr"), ("backgrounds", "ptr")]
_LISTS = [("tile_offsets", "ptr"), ("flatten_ids", "ptr"), ("n_isects", "i64")]
_GRADS = [("v_means", "ptr"), ("v_quats", "ptr"), ("v_scales", "ptr"), ("v_colors", "ptr"), ("v_opacities", "ptr")]
_WS = [("workspace", "ptr"), ("workspace_bytes", "size"), ("stream", "stream")]
_REFERENCE_FORM = [("N", "u32"), ("channels", "u32"), *_SCENE, ("masks", "ptr"), ("cams", "cams"), ("tile_size", "u32"), ("ut_params", "ut"), *_LISTS]
_EXTENSION_FORM = [("N", "u32"), *_SCENE, ("cams", "cams"), ("tile_size", "u32"), *_LISTS]
_BWD = [*_REFERENCE_FORM, ("render_alphas", "ptr"), ("last_ids", "ptr"), ("v_render_colors", "ptr"), ("v_render_alphas", "ptr"), *_GRADS, *_WS]
# entry -> (parameters in the order of include/lfs_gsplat.h, the outputs among them)
ENTRIES = {
    "fwd": ("lfs_rasterize_to_pixels_from_world_3dgs_fwd", [*_REFERENCE_FORM, ("render_colors", "ptr"), ("render_alphas", "ptr"), ("last_ids", "ptr"), *_WS],
            ["render_colors", "render_alphas", "last_ids", "workspace"]),
    "bwd": ("lfs_rasterize_to_pixels_from_world_3dgs_bwd", _BWD, [n for n, _ in _GRADS] + ["workspace"]),
    "bwd_prepared": ("lfs_rasterize_to_pixels_from_world_3dgs_bwd_prepared", _BWD, [n for n, _ in _GRADS] + ["workspace"]),
    "mse": ("lfs_rasterize_to_pixels_from_world_3dgs_bwd_prepared_mse",
            [*_EXTENSION_FORM, ("render_colors", "ptr"), ("render_alphas", "ptr"), ("last_ids", "ptr"), ("target_chw", "ptr"), ("weight", "f32"), ("loss", "ptr"), *_GRADS, *_WS],
            ["loss"] + [n for n, _ in _GRADS] + ["workspace"]),
    "mse_acc": ("lfs_rasterize_to_pixels_from_world_3dgs_bwd_prepared_mse_acc",
                [*_EXTENSION_FORM, ("render_colors", "ptr"), ("render_alphas", "ptr"), ("last_ids", "ptr"), ("target_chw", "ptr"), ("weight", "f32"), *_WS], ["workspace"]),
    "acc": ("lfs_rasterize_to_pixels_from_world_3dgs_bwd_prepared_acc",
            [*_EXTENSION_FORM, ("render_alphas", "ptr"), ("last_ids", "ptr"), ("v_render_colors", "ptr"), ("v_render_alphas", "ptr"), *_WS], ["workspace"]),
    "finish_grads": ("lfs_gut_finish_grads",
                     [("N", "u32"), ("means", "ptr"), ("raw_quats", "ptr"), ("quats", "ptr"), ("scales", "ptr"), ("opacities", "ptr"), ("scale_reg", "f32"), ("opacity_reg", "f32"),
                      ("accumulate", "int"), ("g_means", "ptr"), ("g_raw_scales", "ptr"), ("g_raw_quats", "ptr"), ("g_raw_opacities", "ptr"), ("v_colors", "ptr"), ("loss", "ptr"), *_WS],
                     ["g_means", "g_raw_scales", "g_raw_quats", "g_raw_opacities", "v_colors", "loss", "workspace"]),
    "finish_adam": ("lfs_gut_finish_adam",
                    [("N", "u32"), ("means", "ptr"), ("raw_scales", "ptr"), ("raw_quats", "ptr"), ("raw_opacities", "ptr"), ("quats", "ptr"), ("scales", "ptr"), ("opacities", "ptr"),
                     ("v_dirs", "ptr"), ("exp_avg", "ptrs"), ("exp_avg_sq", "ptrs"), ("scalars", "floats"), ("scale_reg", "f32"), ("opacity_reg", "f32"), ("loss", "ptr"), *_WS],
                    ["means", "raw_scales", "raw_quats", "raw_opacities", "exp_avg", "exp_avg_sq", "loss", "workspace"]),
}
RASTER = ["fwd", "bwd", "bwd_prepared", "mse", "mse_acc", "acc"]
MSE_FORMS = ["mse", "mse_acc"]


def cam(**fields):   # a row that changes fields of the camera block
    return {"cams": ("edit", fields)}


# (entries, what changes, expected code). "BELOW": one byte less than the entry needs.
ROWS = [
    (RASTER, "cams NULL", {"cams": None}, INVALID),
    (RASTER, "C = 0", cam(C=0), INVALID),
    (RASTER, "viewmats0 NULL", cam(viewmats0=None), INVALID),
    (RASTER, "Ks NULL", cam(Ks=None), INVALID),
    (RASTER, "camera_model = ORTHO", cam(camera_model=1), UNSUPPORTED),
    (RASTER, "tile_size 4", {"tile_size": 4}, UNSUPPORTED),
    (RASTER, "tile_size 12", {"tile_size": 12}, UNSUPPORTED),
    (RASTER, "tile_size 72", {"tile_size": 72}, UNSUPPORTED),
    (RASTER, "C * N = 2^26", {"N": 1 << 26}, UNSUPPORTED),
    (RASTER, "n_isects = -1", {"n_isects": -1}, INVALID),
    (RASTER, "n_isects = 2^31", {"n_isects": 1 << 31}, INVALID),
    (RASTER, "n_isects = 2^29", {"n_isects": 1 << 29}, UNSUPPORTED),
    (RASTER, "workspace NULL", {"workspace": None}, INVALID),
    (RASTER, "workspace_bytes one below lfs_rasterize_workspace_bytes", {"workspace_bytes": "BELOW"}, WORKSPACE),
    (RASTER, "means NULL", {"means": None}, INVALID),
    (RASTER, "flatten_ids NULL with lists present", {"flatten_ids": None}, INVALID),
    (RASTER, "tile_offsets NULL", {"tile_offsets": None}, INVALID),
    (["fwd", "bwd", "bwd_prepared"], "channels 0", {"channels": 0}, UNSUPPORTED),
    (["fwd", "bwd", "bwd_prepared"], "channels 5", {"channels": 5}, UNSUPPORTED),
    (["fwd"], "render_colors NULL", {"render_colors": None}, INVALID),
    (["fwd"], "render_alphas NULL", {"render_alphas": None}, INVALID),
    (["fwd"], "last_ids NULL", {"last_ids": None}, INVALID),
    (["bwd", "bwd_prepared"], "v_means NULL", {"v_means": None}, INVALID),
    (["bwd", "bwd_prepared"], "render_alphas NULL", {"render_alphas": None}, INVALID),
    (["bwd", "bwd_prepared"], "last_ids NULL", {"last_ids": None}, INVALID),
    (["bwd", "bwd_prepared"], "v_render_colors NULL", {"v_render_colors": None}, INVALID),
    (["bwd", "bwd_prepared"], "N = 0", {"N": 0}, 0),
    (MSE_FORMS, "n_isects = 0", {"n_isects": 0}, UNSUPPORTED),
    (MSE_FORMS, "target_chw NULL", {"target_chw": None}, INVALID),
    (MSE_FORMS, "render_colors NULL", {"render_colors": None}, INVALID),
    (["mse"], "loss NULL", {"loss": None}, INVALID),
    (MSE_FORMS, "C = 2", cam(C=2), INVALID),
    (["acc"], "v_render_colors NULL", {"v_render_colors": None}, INVALID),
    (["acc"], "C = 2", cam(C=2), WORKSPACE),   # (a two-camera workspace is larger: the size check comes before "rows only: one camera"; the MSE forms check the camera count first)
    (["finish_grads"], "N = 0", {"N": 0}, 0),
    (["finish_grads"], "v_colors NULL", {"v_colors": None}, INVALID),
    (["finish_grads"], "workspace NULL", {"workspace": None}, INVALID),
    (["finish_grads"], "workspace_bytes one below the offset of the culling records", {"workspace_bytes": "BELOW"}, WORKSPACE),
    (["finish_adam"], "v_dirs NULL", {"v_dirs": None}, INVALID),
    (["finish_adam"], "exp_avg[2] NULL", {"exp_avg": ("null_at", 2)}, INVALID),
    (["finish_adam"], "workspace_bytes one below the offset of the culling records", {"workspace_bytes": "BELOW"}, WORKSPACE),
]


def _call(lib, capi, entry, values):
    """one call of `entry` with `values`; every ctypes object stays referenced until it returns"""
    symbol, params, _ = ENTRIES[entry]
    args, keep = [], []
    for name, kind in params:
        v = values.get(name)
        if kind == "ptr":
            args.append(C.c_void_p(v.data_ptr()) if v is not None else None)
        elif kind == "ptrs":
            arr = (C.c_void_p * len(v))(*[t.data_ptr() if t is not None else None for t in v])
            keep.append(arr); args.append(arr)
        elif kind == "floats":
            arr = (C.c_float * len(v))(*v)
            keep.append(arr); args.append(arr)
        elif kind == "cams":
            args.append(C.byref(v) if v is not None else None)
        elif kind == "ut":
            keep.append(capi.ut_struct(None)); args.append(C.byref(keep[-1]))
        elif kind == "stream":
            args.append(capi.stream())
        else:
            args.append({"u32": C.c_uint32, "i64": C.c_int64, "f32": C.c_float, "int": C.c_int, "size": C.c_size_t}[kind](v))
    fn = getattr(lib, symbol)
    fn.restype = C.c_int
    return fn(*args)


def _sentinel_like(t):
    return torch.full_like(t.view(torch.uint8), SENTINEL_BYTE).view(t.dtype)


def _untouched(t):
    return bool((t.view(torch.uint8) == SENTINEL_BYTE).all())


def run_all():
    """-> number of refused calls checked"""
    from lichtfeld_studio_amd import capi, ops
    lib = capi.load_library()
    g = torch.Generator(device="cpu").manual_seed(5)
    f32 = lambda *s: torch.rand(*s, generator=g, dtype=torch.float32)
    means = torch.cat([f32(N, 2) * 1.6 - 0.8, f32(N, 1) + 2.5], 1).to(DEV)
    raw_quats = (f32(N, 4) - 0.5).to(DEV)
    quats = torch.nn.functional.normalize(raw_quats, dim=-1).contiguous()
    raw_scales = (f32(N, 3) - 2.0).to(DEV)
    scales = raw_scales.exp()
    raw_opacities = (f32(N) * 2 - 0.5).to(DEV)
    opac = torch.sigmoid(raw_opacities)
    colors, opacities = f32(1, N, 3).to(DEV), opac[None].contiguous()
    bg = f32(1, 3).to(DEV)
    vm = torch.eye(4, device=DEV)[None].contiguous()
    K = torch.tensor([[[14.0, 0, 8], [0, 14.0, 8], [0, 0, 1]]], device=DEV)
    radii, m2, depths, _, _ = ops.projection_ut_3dgs_fused(means, quats, scales, opac, vm, None, K, W, H, 0.3, 0.01, 1e4, 0.0, False, capi.CameraModelType.PINHOLE)
    _, ids, flat = ops.intersect_tile(m2, radii, depths, None, None, 1, TILE, 1, 1, True)
    offs = ops.intersect_offset(ids, 1, 1, 1)
    n_isects = int(flat.shape[0])
    assert n_isects >= N // 2, "degenerate scene"
    cams = capi.cameras_struct(vm, None, K, W, H, capi.CameraModelType.PINHOLE, capi.ShutterType.GLOBAL)
    ws_bytes = lib.lfs_rasterize_workspace_bytes(C.c_uint32(1), C.c_uint32(N), C.c_uint32(3), C.c_uint32(W), C.c_uint32(H), C.c_uint32(TILE), C.c_int64(n_isects))
    # the finish entries read the workspace up to its culling records: behind the accumulator rows (16 floats per Gaussian) and the 256 loss slots, 256-byte aligned
    rows_bytes = lib.lfs_rasterize_workspace_acc_offset(C.c_uint32(1), C.c_uint32(N)) + ((4 * (16 * N + 256) + 255) & ~255)
    assert 0 < rows_bytes < ws_bytes
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=DEV)
    base = dict(N=N, channels=3, means=means, quats=quats, scales=scales, colors=colors, opacities=opacities, backgrounds=bg, masks=None, cams=cams, tile_size=TILE,
                tile_offsets=offs, flatten_ids=flat, n_isects=n_isects, render_colors=z(1, H, W, 3), render_alphas=z(1, H, W, 1), last_ids=z(1, H, W, dtype=torch.int32),
                v_render_colors=f32(1, H, W, 3).to(DEV), v_render_alphas=f32(1, H, W, 1).to(DEV), v_means=z(N, 3), v_quats=z(N, 4), v_scales=z(N, 3), v_colors=z(1, N, 3),
                v_opacities=z(1, N), target_chw=f32(3, H, W).to(DEV), weight=1.0, loss=z(1), workspace=z(ws_bytes, dtype=torch.uint8), workspace_bytes=ws_bytes)
    finish = dict(N=N, means=means.clone(), raw_scales=raw_scales.clone(), raw_quats=raw_quats.clone(), raw_opacities=raw_opacities.clone(), quats=quats, scales=scales,
                  opacities=opac, scale_reg=0.01, opacity_reg=0.01, accumulate=0, g_means=z(N, 3), g_raw_scales=z(N, 3), g_raw_quats=z(N, 4), g_raw_opacities=z(N),
                  v_colors=z(N, 3), v_dirs=z(N, 3), loss=z(1), exp_avg=[z(N, 3), z(N, 3), z(N, 4), z(N)], exp_avg_sq=[z(N, 3), z(N, 3), z(N, 4), z(N)],
                  scalars=[1e-3, 0.9, 0.999, 1e-15, 10.0, 31.6] * 4, workspace=base["workspace"], workspace_bytes=rows_bytes)
    valid = {e: (finish if e.startswith("finish") else base) for e in ENTRIES}
    needs = {e: (rows_bytes if e.startswith("finish") else ws_bytes) for e in ENTRIES}

    # every entry accepts its valid call (in an order in which each finds what it reads: the forward's outputs, the prepared workspace, the accumulator rows)
    for entry in ["fwd", "bwd", "bwd_prepared", "mse", "mse_acc", "finish_grads", "acc", "finish_adam"]:
        assert _call(lib, capi, entry, valid[entry]) == 0, entry
    torch.cuda.synchronize()
    assert float(base["render_alphas"].max()) > 0.05, "degenerate scene"
    # v_render_alphas NULL is a valid call: it stands for zeros
    got = {}
    for key, v_ra in (("null", None), ("zeros", torch.zeros_like(base["v_render_alphas"]))):
        vals = dict(base, v_render_alphas=v_ra, **{n: torch.zeros_like(base[n]) for n, _ in _GRADS})
        assert _call(lib, capi, "bwd", vals) == 0
        torch.cuda.synchronize()
        got[key] = [vals[n] for n, _ in _GRADS]
    for a, b in zip(got["null"], got["zeros"]):   # two runs of the same sums: equal up to the order of the float atomics
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-6)

    checked = 0
    for entries, what, change, code in ROWS:
        for entry in entries:
            _, _, outputs = ENTRIES[entry]
            vals = dict(valid[entry])
            for name in outputs:   # fresh outputs, filled with the sentinel
                v = vals[name]
                vals[name] = [_sentinel_like(t) for t in v] if isinstance(v, list) else _sentinel_like(v)
            for name, new in change.items():
                if new == "BELOW":
                    new = needs[entry] - 1
                elif isinstance(new, tuple) and new[0] == "edit":
                    edited = type(vals["cams"]).from_buffer_copy(vals["cams"])
                    for k, fv in new[1].items():
                        setattr(edited, k, fv)
                    new = edited
                elif isinstance(new, tuple) and new[0] == "null_at":
                    new = [None if i == new[1] else t for i, t in enumerate(vals[name])]
                vals[name] = new
            rc = _call(lib, capi, entry, vals)
            torch.cuda.synchronize()
            print(f"raster refusals: {entry:13s} {what:60s} -> {rc} (expected {code})")
            assert rc == code, (entry, what, rc, code)
            for name in outputs:
                v = vals[name]
                for t in (v if isinstance(v, list) else [v]):
                    assert t is None or _untouched(t), (entry, what, name)
            checked += 1
    return checked
