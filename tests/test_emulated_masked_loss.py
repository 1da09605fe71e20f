"""The test bodies of tests/test_gpu_masked_loss.py on the CPU: the product library compiled as host code on the wavefront emulator, "cuda:0" served by CPU
tensors (the fixture pattern of tests/test_emulated_sparsity.py). Same inputs, same float64 model, same bounds. What this holds without a GPU is the kernels'
logic: the per-pixel weights and the crop, the normalisers derived from the device-side sums, the empty-mask and empty-crop cases, the pre-multiplied
derivative maps and their exact zeros, the alpha term, the integer sums of lfs_mask_prepare at ragged sizes, and the argument checks."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import emul_util  # noqa: E402
import test_gpu_masked_loss as gpu_tests  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _emulated_library_and_cpu_tensors():
    if not emul_util.available():
        pytest.skip("no clang++ to build the emulated library")
    import lichtfeld_studio_amd.loader  # noqa: F401  (before installed(): the loader hooks of every imported module of the package get patched)
    import lichtfeld_studio_amd.losses  # noqa: F401
    with emul_util.installed(), emul_util.cuda_requests_served_by_the_cpu():
        yield


test_emulated__masked_l1_ssim_value_and_gradient_match_the_f64_model = gpu_tests.test_masked_l1_ssim_value_and_gradient_match_the_f64_model
test_emulated__full_mask_agrees_with_the_unmasked_entry = gpu_tests.test_full_mask_agrees_with_the_unmasked_entry
test_emulated__gradient_is_local_to_the_mask = gpu_tests.test_gradient_is_local_to_the_mask
test_emulated__alpha_penalty_outside_the_mask = gpu_tests.test_alpha_penalty_outside_the_mask
test_emulated__masked_mse_matches_the_f64_model = gpu_tests.test_masked_mse_matches_the_f64_model
test_emulated__mask_prepare_sums_copy_threshold_and_invert = gpu_tests.test_mask_prepare_sums_copy_threshold_and_invert
test_emulated__mask_prepare_resamples_as_the_image_path_does = gpu_tests.test_mask_prepare_resamples_as_the_image_path_does
test_emulated__masked_entry_points_refuse_bad_arguments_before_any_launch = gpu_tests.test_masked_entry_points_refuse_bad_arguments_before_any_launch


def test_the_emulated_library_served_these_tests():
    from lichtfeld_studio_amd import losses
    assert losses.load_library() is emul_util.library()
    assert emul_util.library().lfs_version().decode().endswith("src-unknown")
