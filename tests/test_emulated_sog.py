"""The test bodies of tests/test_gpu_sog.py on the CPU: the product library compiled as host code on the wavefront emulator, "cuda:0" served by CPU tensors
(the fixture pattern of tests/test_emulated_gpu_suite.py). Same inputs, same numpy models, same bounds. What this holds without a GPU is the kernels' logic:
the MFMA operand and accumulator lane maps of the assignment (the emulator's v_mfma_f32_16x16x4_f32 is the fmaf chain the hardware computes), the fragment-order
pre-pass, padding of k and D, the (score, index) fold between the lane groups, both binary searches of the 1-D rule, the fixed-order f64 tree of the update and
the two-stage min / max of the Morton codes, at ragged sizes."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import emul_util  # noqa: E402
import test_gpu_sog as gpu_tests  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _emulated_library_and_cpu_tensors():
    if not emul_util.available():
        pytest.skip("no clang++ to build the emulated library")
    import lichtfeld_studio_amd.sog  # noqa: F401  (before installed(): the loader hooks of every imported module of the package get patched)
    with emul_util.installed(), emul_util.cuda_requests_served_by_the_cpu():
        yield


test_emulated__morton_codes_are_bit_equal_to_the_model_and_the_order_is_stable = gpu_tests.test_morton_codes_are_bit_equal_to_the_model_and_the_order_is_stable
test_emulated__morton_of_identical_points_takes_the_cube_clamp = gpu_tests.test_morton_of_identical_points_takes_the_cube_clamp
test_emulated__assignment_is_within_the_f32_score_bound_of_the_fp64_nearest = gpu_tests.test_assignment_is_within_the_f32_score_bound_of_the_fp64_nearest
test_emulated__assignment_gives_exact_ties_to_the_lowest_index = gpu_tests.test_assignment_gives_exact_ties_to_the_lowest_index
test_emulated__assignment_1d_is_the_first_strict_minimum = gpu_tests.test_assignment_1d_is_the_first_strict_minimum
test_emulated__update_is_the_segment_mean_keeps_empty_clusters_and_repeats_bit_for_bit = gpu_tests.test_update_is_the_segment_mean_keeps_empty_clusters_and_repeats_bit_for_bit
test_emulated__kmeans_1d_returns_the_labels_of_the_centroids_before_the_last_update = gpu_tests.test_kmeans_1d_returns_the_labels_of_the_centroids_before_the_last_update
test_emulated__kmeans_1d_with_no_more_points_than_clusters_returns_the_sorted_data = gpu_tests.test_kmeans_1d_with_no_more_points_than_clusters_returns_the_sorted_data
test_emulated__kmeans_inertia_does_not_increase = gpu_tests.test_kmeans_inertia_does_not_increase
test_emulated__kmeans_with_the_same_generator_seed_is_bit_identical = gpu_tests.test_kmeans_with_the_same_generator_seed_is_bit_identical
test_emulated__kmeans_with_no_more_points_than_clusters_returns_the_data = gpu_tests.test_kmeans_with_no_more_points_than_clusters_returns_the_data
test_emulated__entry_points_refuse_bad_arguments_before_any_launch = gpu_tests.test_entry_points_refuse_bad_arguments_before_any_launch


def test_the_emulated_library_served_these_tests():
    from lichtfeld_studio_amd import sog
    assert sog.load_library() is emul_util.library()
    assert emul_util.library().lfs_version().decode().endswith("src-unknown")
