"""The test bodies of tests/test_gpu_sparsity.py on the CPU: the product library compiled as host code on the wavefront emulator, "cuda:0" served by CPU tensors
(the fixture pattern of tests/test_emulated_sog.py). Same inputs, same numpy models, same bounds. What this holds without a GPU is the kernels' logic: the
order-preserving key and its inverse, the digit masks and the (prefix, residual rank) hand-over of the four select passes, the wave scan of the pick kernel,
the v values stored by the first pass, the fixed-order loss tree, the block scan and the carry of the ordered mask pass, at ragged sizes."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import emul_util  # noqa: E402
import test_gpu_sparsity as gpu_tests  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _emulated_library_and_cpu_tensors():
    if not emul_util.available():
        pytest.skip("no clang++ to build the emulated library")
    import lichtfeld_studio_amd.sparsity  # noqa: F401  (before installed(): the loader hooks of every imported module of the package get patched)
    with emul_util.installed(), emul_util.cuda_requests_served_by_the_cpu():
        yield


test_emulated__select_is_the_kth_of_the_sorted_array = gpu_tests.test_select_is_the_kth_of_the_sorted_array
test_emulated__select_repeats_bit_for_bit = gpu_tests.test_select_repeats_bit_for_bit
test_emulated__update_uses_the_sigmoid_of_activations_fwd_bit_for_bit = gpu_tests.test_update_uses_the_sigmoid_of_activations_fwd_bit_for_bit
test_emulated__three_successive_updates_match_the_f32_model = gpu_tests.test_three_successive_updates_match_the_f32_model
test_emulated__update_zeroes_every_value_tied_at_the_threshold = gpu_tests.test_update_zeroes_every_value_tied_at_the_threshold
test_emulated__loss_and_gradient_are_within_the_f32_bounds_of_the_f64_model = gpu_tests.test_loss_and_gradient_are_within_the_f32_bounds_of_the_f64_model
test_emulated__prune_mask_takes_the_lowest_values_and_breaks_ties_by_index = gpu_tests.test_prune_mask_takes_the_lowest_values_and_breaks_ties_by_index
test_emulated__prune_mask_of_equal_values_prunes_the_first_half = gpu_tests.test_prune_mask_of_equal_values_prunes_the_first_half
test_emulated__all_four_operators_past_the_grid_cap = gpu_tests.test_all_four_operators_past_the_grid_cap
test_emulated__entry_points_refuse_bad_arguments_before_any_launch = gpu_tests.test_entry_points_refuse_bad_arguments_before_any_launch


def test_the_emulated_library_served_these_tests():
    from lichtfeld_studio_amd import sparsity
    assert sparsity.load_library() is emul_util.library()
    assert emul_util.library().lfs_version().decode().endswith("src-unknown")
