"""The C-ABI test bodies of tests/test_gpu_fastgs_w2c.py (identity at SH degree 0, the SH term, no disturbance / full write / determinism, edges) on the CPU: the
product library compiled as host code on the wavefront emulator, "cuda:0" served by CPU tensors (the fixture pattern of tests/test_emulated_gpu_suite.py). Same
inputs, same float64 expectations, same bounds. What this holds without a GPU is the kernels' logic - above all that no lane of fg_preprocess_bwd_kernel<true>
leaves before the workgroup sum (rows past N, invisible primitives), the wave64 butterfly, the LDS hand-over and the partial-row reduction at ragged sizes."""
import ctypes as C
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import emul_util  # noqa: E402
import test_gpu_fastgs_w2c as gpu_tests  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _emulated_library_and_cpu_tensors():
    if not emul_util.available():
        pytest.skip("no clang++ to build the emulated library")
    with emul_util.installed() as lib, emul_util.cuda_requests_served_by_the_cpu():
        lib.lfs_fastgs_w2c_workspace_bytes.restype = C.c_size_t
        yield


test_emulated__grad_w2c_is_the_sum_of_dcam_times_mean_at_sh_degree_0 = gpu_tests.test_grad_w2c_is_the_sum_of_dcam_times_mean_at_sh_degree_0
test_emulated__grad_w2c_leaves_out_the_sh_colour_term = gpu_tests.test_grad_w2c_leaves_out_the_sh_colour_term
test_emulated__w2c_entry_point_disturbs_nothing_writes_fully_and_is_deterministic = gpu_tests.test_w2c_entry_point_disturbs_nothing_writes_fully_and_is_deterministic
test_emulated__grad_w2c_edges_empty_scene_nothing_visible_and_return_codes = gpu_tests.test_grad_w2c_edges_empty_scene_nothing_visible_and_return_codes


def test_the_emulated_library_served_these_tests():
    import lichtfeld_studio_amd  # noqa: F401
    from lichtfeld_studio_amd import fastgs
    assert fastgs.load_library() is emul_util.library()
    assert emul_util.library().lfs_version().decode().endswith("src-unknown")
