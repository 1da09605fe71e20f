"""tests/raster_refusals.py on the CPU: the product library compiled as host code on the wavefront emulator, "cuda:0" served by CPU tensors (the fixture pattern of
tests/test_emulated_fastgs_absgrad.py). The refusals are host code, so what holds here holds for the real library, which tests/test_gpu_raster.py runs the same body on."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import emul_util  # noqa: E402
import raster_refusals  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _emulated_library_and_cpu_tensors():
    assert emul_util.available(), "no clang++ to build the emulated library"
    import lichtfeld_studio_amd.ops  # noqa: F401  (before installed(): the loader hooks of every imported module of the package get patched)
    with emul_util.installed(), emul_util.cuda_requests_served_by_the_cpu():
        yield


def test_every_refused_rasterizer_call_returns_its_code_and_writes_nothing():
    from lichtfeld_studio_amd import capi
    assert capi.load_library() is emul_util.library()
    assert raster_refusals.run_all() == sum(len(entries) for entries, _, _, _ in raster_refusals.ROWS)
