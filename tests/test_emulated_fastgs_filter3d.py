"""Cases 1-7 of tests/test_gpu_fastgs_filter3d.py on the CPU: the product library compiled as host code on the wavefront emulator, "cuda:0" served by CPU tensors
(the pattern of tests/test_emulated_fastgs_antialiased.py). Same scenes, same float64 host model, same oracle calls, same bounds. What this holds without a GPU
is the kernels' logic: lfs_filter3d_compute (the camera loop, the seen test, the integer minimum and the second pass), the filtered forms of the per-primitive
forward and backward in every combination (antialiased, depth, grad_w2c), the order of the cuts, the mode word and the library's memory of filtered workspaces, and
the argument checks of the _ex entries. csrc/filter3d.hip is part of the emulated build like every file of build.SOURCES. (The deterministic accumulation mode the
tests ask for is dropped by the emulated library: its wavefronts run one after the other, the float sums are reproducible as they are.)"""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import emul_util  # noqa: E402
import test_gpu_fastgs_filter3d as gpu_tests  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _emulated_library_and_cpu_tensors():
    if not emul_util.available():
        pytest.skip("no clang++ to build the emulated library")
    import lichtfeld_studio_amd.fastgs  # noqa: F401  (before installed(): the loader hooks of every imported module of the package get patched)
    import lichtfeld_studio_amd.filter3d  # noqa: F401
    gpu_tests._expected_grads.cache_clear()
    with emul_util.installed(), emul_util.cuda_requests_served_by_the_cpu():
        yield
    gpu_tests._expected_grads.cache_clear()   # (results of the emulated library: a later -m gpu run in the same process computes its own)


test_emulated__the_camera_set_exercises_the_kernel = gpu_tests.test_the_camera_set_exercises_the_kernel
test_emulated__filter3d_compute_matches_the_host_model = gpu_tests.test_filter3d_compute_matches_the_host_model
test_emulated__filter3d_compute_edges = gpu_tests.test_filter3d_compute_edges
test_emulated__filtered_forward_is_the_default_forward_at_the_baked_parameters = gpu_tests.test_filtered_forward_is_the_default_forward_at_the_baked_parameters
test_emulated__filtered_backward_is_the_composition = gpu_tests.test_filtered_backward_is_the_composition
test_emulated__filter_with_antialiasing = gpu_tests.test_filter_with_antialiasing
test_emulated__filter_with_depth = gpu_tests.test_filter_with_depth
test_emulated__filtered_pose_gradient = gpu_tests.test_filtered_pose_gradient
test_emulated__filtered_cuts = gpu_tests.test_filtered_cuts
test_emulated__the_old_entries_and_the_ex_entries_without_a_filter_agree_bit_for_bit = gpu_tests.test_the_old_entries_and_the_ex_entries_without_a_filter_agree_bit_for_bit
test_emulated__a_backward_that_disagrees_with_the_forward_about_the_filter_is_refused = gpu_tests.test_a_backward_that_disagrees_with_the_forward_about_the_filter_is_refused


def test_the_emulated_library_served_these_tests():
    from lichtfeld_studio_amd import fastgs, filter3d
    assert fastgs.load_library() is emul_util.library() and filter3d.load_library() is emul_util.library()
    assert emul_util.library().lfs_version().decode().endswith("src-unknown")
