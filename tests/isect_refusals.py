"""What the intersection stage's C entries (csrc/intersect.hip) and, through lfs_gut_view_forward, the training step's front end (csrc/gut_step.hip) refuse, and
with which code - called through ctypes as a foreign caller would. One body, two runners: tests/test_emulated_isect_refusals.py (the library built as host code,
tests/emul_util.py) and tests/test_gpu_intersect.py (the real library).

Scene: one camera, 8 Gaussians, tile 16, a 2 x 2 tile grid - random means in a 32 x 32 image, radii 1..9; the intersection workspace is 1280 bytes. A valid count and
a valid emit return 0. Then each row below changes ONE argument of the valid call and must return the listed code. A refused call (code != 0) must leave every
output and the workspace as they were - the outputs at the sentinel they were filled with, the workspace at the sentinel (count) or at what the valid count left
there (emit): a call is refused before anything is launched, copied or cleared, so the bogus sizes of some rows (2^30 cameras, 2^31 intersections) need no allocation.
Rows with code 0 are valid calls; what they may write is listed with them."""
import ctypes as C

import torch

DEV = "cuda:0"
N, TILE, TW, TH, W, H = 8, 16, 2, 2, 32, 32
T = TW * TH
WS_BYTES = 1280
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
SENTINEL_BYTE = 0x5A

_GRID = [("C", "u32"), ("N", "u32"), ("means2d", "ptr"), ("radii", "ptr")]
_TILES = [("tile_size", "u32"), ("tile_width", "u32"), ("tile_height", "u32")]
_WS = [("workspace", "ptr"), ("workspace_bytes", "size"), ("stream", "stream")]
# entry -> (parameters in the order of include/lfs_gsplat.h, the outputs among them)
ENTRIES = {
    "count": ("lfs_intersect_tile_count_ex",
              [*_GRID, *_TILES, ("tiles_per_gauss", "ptr"), ("n_isects", "ptr"), ("max_tile_isects", "ptr"), ("tile_offsets", "ptr"), ("flags", "u32"), ("stamp_out", "ptr"),
               ("stamp", "i64"), *_WS],
              ["tiles_per_gauss", "n_isects", "max_tile_isects", "tile_offsets", "stamp_out"]),
    "emit": ("lfs_intersect_tile_emit_ex",
             [*_GRID, ("depths", "ptr"), *_TILES, ("sort", "int"), ("n_isects", "i64"), ("tiles_per_gauss", "ptr"), ("isect_ids", "ptr"), ("flatten_ids", "ptr"),
              ("tile_offsets", "ptr"), ("scratch", "ptr"), ("max_tile_isects", "i64"), *_WS],
             ["isect_ids", "flatten_ids", "tile_offsets", "scratch"]),
}

# (entry, what changes, expected code, the outputs a VALID row may write - everything else stays at the sentinel). "BELOW": one byte less than the entry needs.
EVERYTHING = "everything"
ROWS = [
    ("count", "n_isects NULL", {"n_isects": None}, INVALID, None),
    ("count", "workspace NULL", {"workspace": None}, INVALID, None),
    ("count", "tile_size 0", {"tile_size": 0}, INVALID, None),
    ("count", "tile_width 0", {"tile_width": 0}, INVALID, None),
    ("count", "tile_height 0", {"tile_height": 0}, INVALID, None),
    ("count", "C = 0", {"C": 0}, INVALID, None),
    ("count", "C = 2^30", {"C": 1 << 30}, UNSUPPORTED, None),
    ("count", "workspace_bytes one below", {"workspace_bytes": "BELOW"}, WORKSPACE, None),
    ("count", "means2d NULL", {"means2d": None}, INVALID, None),
    ("count", "radii NULL", {"radii": None}, INVALID, None),
    ("count", "tiles_per_gauss NULL", {"tiles_per_gauss": None}, INVALID, None),
    ("count", "N = 0", {"N": 0}, 0, EVERYTHING),   # (valid: it writes counts, offsets and workspace)
    ("emit", "workspace NULL", {"workspace": None}, INVALID, None),
    ("emit", "C = 0", {"C": 0}, INVALID, None),
    ("emit", "tile_size 0", {"tile_size": 0}, INVALID, None),
    ("emit", "workspace_bytes one below", {"workspace_bytes": "BELOW"}, WORKSPACE, None),
    ("emit", "n_isects = 2^31", {"n_isects": 1 << 31}, UNSUPPORTED, None),
    ("emit", "means2d NULL", {"means2d": None}, INVALID, None),
    ("emit", "radii NULL", {"radii": None}, INVALID, None),
    ("emit", "depths NULL", {"depths": None}, INVALID, None),
    ("emit", "isect_ids NULL", {"isect_ids": None}, INVALID, None),
    ("emit", "flatten_ids NULL", {"flatten_ids": None}, INVALID, None),
    ("emit", "sort = 0 with tiles_per_gauss NULL", {"sort": 0, "tiles_per_gauss": None}, INVALID, None),
    ("emit", "tile_width 0", {"tile_width": 0}, INVALID, None),     # (the count has always refused a zero tile grid; the emit used to launch grids of T = 0)
    ("emit", "tile_height 0", {"tile_height": 0}, INVALID, None),
    ("emit", "n_isects = 0", {"n_isects": 0}, 0, ["tile_offsets"]),
    ("emit", "n_isects = -1", {"n_isects": -1}, 0, ["tile_offsets"]),
    ("emit", "scratch NULL", {"scratch": None}, 0, EVERYTHING),     # (valid: the one-pass scatter)
    ("emit", "tile_offsets NULL", {"tile_offsets": None}, 0, EVERYTHING),
    ("emit", "sort = 0", {"sort": 0}, 0, EVERYTHING),
]

# the training step's entries, through lfs_gut_view_forward on the same scene: (what changes, expected code). Nothing may be written.
STEP_ROWS = [
    ("capacity = 0", {"capacity": 0}, INVALID),
    ("workspace_bytes one below lfs_gut_step_layout_for(...).bytes", {"workspace_bytes": "BELOW"}, WORKSPACE),
    ("tile_size 12", {"tile_size": 12}, INVALID),   # (no rasterizer cell kernels for it: the step cannot lay its workspace out)
    ("K = 33", {"K": 33}, INVALID),
]


def _call(lib, capi, entry, values):
    symbol, params, _ = ENTRIES[entry]
    args = []
    for name, kind in params:
        v = values.get(name)
        if kind == "ptr":
            args.append(C.c_void_p(v.data_ptr()) if v is not None else None)
        elif kind == "stream":
            args.append(capi.stream())
        else:
            args.append({"u32": C.c_uint32, "i64": C.c_int64, "int": C.c_int, "size": C.c_size_t}[kind](v))
    fn = getattr(lib, symbol)
    fn.restype = C.c_int
    return fn(*args)


def _sentinel(nbytes):
    return torch.full((nbytes,), SENTINEL_BYTE, dtype=torch.uint8, device=DEV)


def _sentinel_like(t):
    return torch.full_like(t.view(torch.uint8), SENTINEL_BYTE).view(t.dtype)


def _untouched(t):
    return bool((t.view(torch.uint8) == SENTINEL_BYTE).all())


class _Verdict:
    """collect = None: a failed expectation is an assertion error. A list: it is appended instead (the table run against another build of the library)."""

    def __init__(self, collect):
        self.collect = collect

    def expect(self, ok, *what):
        if self.collect is None:
            assert ok, what
        elif not ok:
            self.collect.append(what)


def _step_rows(lib, capi, verdict):
    from lichtfeld_studio_amd.gut_step import StepArgs, StepLayout
    g = torch.Generator(device="cpu").manual_seed(11)
    f32 = lambda *s: torch.rand(*s, generator=g, dtype=torch.float32)
    K = 4
    t = dict(means=torch.cat([f32(N, 2) * 1.6 - 0.8, f32(N, 1) + 2.5], 1), sh0=f32(N, 1, 3), shN=f32(N, K - 1, 3) - 0.5, raw_scales=f32(N, 3) - 2.0,
             raw_quats=f32(N, 4) - 0.5, raw_opacities=f32(N) * 2 - 0.5, viewmat=torch.eye(4), Kmat=torch.tensor([[28.0, 0, 16], [0, 28.0, 16], [0, 0, 1]]))
    t = {k: v.contiguous().to(DEV) for k, v in t.items()}
    capacity = 4 * T * N
    lay = StepLayout()
    assert lib.lfs_gut_step_layout_for(C.c_uint32(N), C.c_uint32(W), C.c_uint32(H), C.c_uint32(TILE), C.c_int64(capacity), C.byref(lay)) == 0
    fn = lib.lfs_gut_view_forward
    fn.restype = C.c_int

    def call(ws, **change):
        a = StepArgs()
        a.N, a.K, a.sh_degree, a.image_width, a.image_height, a.tile_size = N, change.get("K", K), 1, W, H, change.get("tile_size", TILE)
        for k in ("means", "sh0", "shN", "raw_scales", "raw_quats", "raw_opacities", "viewmat", "Kmat"):
            setattr(a, k, t[k].data_ptr())
        nbytes = lay.bytes - 1 if change.get("workspace_bytes") == "BELOW" else lay.bytes
        rc = fn(C.byref(a), C.c_int64(change.get("capacity", capacity)), C.c_int64(1024), C.c_void_p(ws.data_ptr()), C.c_size_t(nbytes), None, C.c_int64(1), capi.stream())
        torch.cuda.synchronize()
        return rc

    ws = _sentinel(lay.bytes)
    assert call(ws) == 0, "lfs_gut_view_forward: the valid call"
    counts = ws[lay.counts:lay.counts + 24].view(torch.int64)
    assert int(counts[0]) >= N // 2 and int(counts[2]) == 1, "degenerate scene"
    checked = 0
    for what, change, code in STEP_ROWS:
        ws = _sentinel(lay.bytes)
        rc = call(ws, **change)
        print(f"isect refusals: view_forward {what:62s} -> {rc} (expected {code})")
        verdict.expect(rc == code, "view_forward", what, "code", rc, code)
        verdict.expect(_untouched(ws), "view_forward", what, "wrote", "workspace")
        checked += 1
    return checked


def run_all(collect=None):
    """-> number of rows checked"""
    from lichtfeld_studio_amd import capi
    lib = capi.load_library()
    verdict = _Verdict(collect)
    lib.lfs_intersect_tile_workspace_bytes.restype = C.c_size_t
    assert lib.lfs_intersect_tile_workspace_bytes(C.c_uint32(1), C.c_uint32(N), C.c_uint32(TW), C.c_uint32(TH)) == WS_BYTES
    g = torch.Generator(device="cpu").manual_seed(7)
    means2d = (torch.rand(1, N, 2, generator=g) * 32).to(DEV)
    radii = torch.randint(1, 10, (1, N, 2), generator=g, dtype=torch.int32).to(DEV)
    depths = (torch.rand(1, N, generator=g) + 1).to(DEV)
    z = lambda n, dtype: torch.zeros(n, dtype=dtype, device=DEV)
    count = dict(C=1, N=N, means2d=means2d, radii=radii, tile_size=TILE, tile_width=TW, tile_height=TH, tiles_per_gauss=z(N, torch.int32), n_isects=z(1, torch.int64),
                 max_tile_isects=z(1, torch.int64), tile_offsets=z(T, torch.int32), flags=0, stamp_out=z(1, torch.int64), stamp=3, workspace=_sentinel(WS_BYTES),
                 workspace_bytes=WS_BYTES)
    assert _call(lib, capi, "count", count) == 0
    torch.cuda.synchronize()
    n_isects = int(count["n_isects"][0])
    assert n_isects >= N and int(count["tiles_per_gauss"].sum()) == n_isects and int(count["stamp_out"][0]) == 3, "degenerate scene"
    counted = count["workspace"].clone()   # what every emit row finds in the workspace
    emit = dict(C=1, N=N, means2d=means2d, radii=radii, depths=depths, tile_size=TILE, tile_width=TW, tile_height=TH, sort=1, n_isects=n_isects,
                tiles_per_gauss=count["tiles_per_gauss"], isect_ids=z(n_isects, torch.int64), flatten_ids=z(n_isects, torch.int32), tile_offsets=z(T, torch.int32),
                scratch=z(n_isects, torch.int64), max_tile_isects=int(count["max_tile_isects"][0]), workspace=counted.clone(), workspace_bytes=WS_BYTES)
    assert _call(lib, capi, "emit", emit) == 0
    torch.cuda.synchronize()
    assert torch.equal(emit["tile_offsets"], count["tile_offsets"]) and sorted(emit["flatten_ids"].tolist()) == sorted(
        i for i, n in enumerate(count["tiles_per_gauss"].tolist()) for _ in range(n))
    valid = {"count": count, "emit": emit}

    checked = 0
    for entry, what, change, code, may_write in ROWS:
        _, _, outputs = ENTRIES[entry]
        vals = dict(valid[entry])
        for name in outputs:
            vals[name] = _sentinel_like(vals[name])
        before = _sentinel(WS_BYTES) if entry == "count" else counted.clone()
        vals["workspace"] = before.clone()
        for name, new in change.items():
            vals[name] = WS_BYTES - 1 if new == "BELOW" else new
        rc = _call(lib, capi, entry, vals)
        torch.cuda.synchronize()
        print(f"isect refusals: {entry:5s} {what:40s} -> {rc} (expected {code})")
        verdict.expect(rc == code, entry, what, "code", rc, code)
        if may_write != EVERYTHING:
            for name in outputs:
                if vals[name] is not None and name not in (may_write or []):
                    verdict.expect(_untouched(vals[name]), entry, what, "wrote", name)
            if vals["workspace"] is not None:
                verdict.expect(torch.equal(vals["workspace"], before), entry, what, "wrote", "workspace")
        if may_write == ["tile_offsets"]:
            verdict.expect(torch.equal(vals["tile_offsets"], count["tile_offsets"]), entry, what, "tile_offsets not written")
        checked += 1
    return checked + _step_rows(lib, capi, verdict)
