"""The test bodies of tests/test_gpu_depth_loss.py on the CPU: the product library compiled as host code on the wavefront emulator, "cuda:0" served by CPU tensors
(the fixture pattern of tests/test_emulated_masked_loss.py). Same inputs, same float64 model, same bounds. What this holds without a GPU is the kernels' logic: the
validity rule and its sentinel, the exact integer sum, the normaliser max(sum m, 1), the sign and the exact zeros of the gradient, and the argument checks."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import emul_util  # noqa: E402
import test_gpu_depth_loss as gpu_tests  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _emulated_library_and_cpu_tensors():
    if not emul_util.available():
        pytest.skip("no clang++ to build the emulated library")
    import lichtfeld_studio_amd.losses  # noqa: F401  (before installed(): the loader hooks of every imported module of the package get patched)
    with emul_util.installed(), emul_util.cuda_requests_served_by_the_cpu():
        yield


test_emulated__depth_l1_value_and_gradient_match_the_f64_model = gpu_tests.test_depth_l1_value_and_gradient_match_the_f64_model
test_emulated__depth_loss_ignores_the_map_where_the_target_is_invalid_and_prepare_is_idempotent = gpu_tests.test_depth_loss_ignores_the_map_where_the_target_is_invalid_and_prepare_is_idempotent
test_emulated__depth_entry_points_refuse_bad_arguments_before_any_launch = gpu_tests.test_depth_entry_points_refuse_bad_arguments_before_any_launch


def test_the_emulated_library_served_these_tests():
    from lichtfeld_studio_amd import losses
    assert losses.load_library() is emul_util.library()
    assert emul_util.library().lfs_version().decode().endswith("src-unknown")
