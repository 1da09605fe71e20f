"""tests/isect_refusals.py on the CPU: the product library compiled as host code on the wavefront emulator, "cuda:0" served by CPU tensors (the fixture pattern of
tests/test_emulated_raster_refusals.py). The refusals are host code, so what holds here holds for the real library, which tests/test_gpu_intersect.py runs the same
body on. Also here, because it is host code as well: the byte layout of the intersection workspace and of the training step's workspace, against recorded values."""
import ctypes as C
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import emul_util  # noqa: E402
import isect_refusals  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _emulated_library_and_cpu_tensors():
    assert emul_util.available(), "no clang++ to build the emulated library"
    import lichtfeld_studio_amd.ops  # noqa: F401  (before installed(): the loader hooks of every imported module of the package get patched)
    with emul_util.installed(), emul_util.cuda_requests_served_by_the_cpu():
        yield


def test_every_refused_intersection_call_returns_its_code_and_writes_nothing():
    from lichtfeld_studio_amd import capi
    assert capi.load_library() is emul_util.library()
    assert isect_refusals.run_all() == len(isect_refusals.ROWS) + len(isect_refusals.STEP_ROWS)


# lfs_gut_step_layout_for(N, W, H, 16, capacity) and lfs_intersect_tile_workspace_bytes(1, N, ceil(W / 16), ceil(H / 16)) as the build BEFORE the workspace layout became
# a table of byte offsets (csrc/lfs_step_internal.h: isect_layout) returned them - recorded from that build, not from this one
LAYOUT_FIELDS = ("bytes", "render", "alpha", "last_ids", "radii", "means2d", "depths", "colors", "quats", "scales", "opacities", "tile_offsets", "flatten_ids", "isect_ids",
                 "counts", "abort_flag")
RECORDED = {
    # (N, W, H, capacity): (the sixteen layout fields in the order above, the intersection workspace's bytes)
    (1, 16, 16, 1): ((12544, 6912, 9984, 11008, 768, 1024, 1280, 1792, 0, 256, 512, 3072, 3840, 3584, 12288, 12032), 1280),
    (3000, 256, 256, 100000): ((7241216, 5929984, 6716416, 6978560, 96256, 120320, 144384, 168448, 0, 48128, 84224, 242944, 1044480, 244480, 7240960, 7240704), 3840),
    (1000000, 1920, 1080, 12000000): ((905707264, 864234752, 889117952, 897412352, 32000000, 40000000, 48000000, 56000000, 0, 16000000, 28000000, 80066048, 176102912,
                                       80102912, 905707008, 905706752), 102912),
}


@pytest.mark.parametrize("shape", sorted(RECORDED))
def test_the_workspace_layouts_are_the_recorded_ones(shape):
    from lichtfeld_studio_amd.gut_step import StepLayout
    lib = emul_util.library()
    n, w, h, capacity = shape
    fields, isect_bytes = RECORDED[shape]
    lay = StepLayout()
    assert lib.lfs_gut_step_layout_for(C.c_uint32(n), C.c_uint32(w), C.c_uint32(h), C.c_uint32(16), C.c_int64(capacity), C.byref(lay)) == 0
    assert tuple(int(getattr(lay, k)) for k in LAYOUT_FIELDS) == fields
    assert int(lib.lfs_intersect_tile_workspace_bytes(C.c_uint32(1), C.c_uint32(n), C.c_uint32((w + 15) // 16), C.c_uint32((h + 15) // 16))) == isect_bytes
