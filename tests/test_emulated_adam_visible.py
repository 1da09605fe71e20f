"""The operator bodies of tests/test_gpu_adam_visible.py on the CPU: the product library compiled as host code on the wavefront emulator, "cuda:0" served by CPU
tensors (the fixture pattern of tests/test_emulated_sparsity.py). Same inputs, same bit-equality assertions. What this holds without a GPU is the kernels' logic:
the ballot and the two word stores of the visibility kernel with their tail word, the compaction of a block's set bits (k-th set bit, the shuffle that hands a lane
its row), the all-visible 16-byte span, the 16-byte accesses of the narrow rows that straddle two Gaussians, the unaligned views, and the refusals. The two sizes
past the workgroup cap stay on the GPU: 4 and 26 million element updates per mask are minutes under emulation."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import emul_util  # noqa: E402
import test_gpu_adam_visible as gpu_tests  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _emulated_library_and_cpu_tensors():
    if not emul_util.available():
        pytest.skip("no clang++ to build the emulated library")
    with emul_util.installed(), emul_util.cuda_requests_served_by_the_cpu():
        yield


test_emulated__visible_rows_equal_the_dense_kernel_and_the_rest_is_untouched = gpu_tests.test_visible_rows_equal_the_dense_kernel_and_the_rest_is_untouched
test_emulated__visible_rows_on_unaligned_views_take_the_scalar_path = gpu_tests.test_visible_rows_on_unaligned_views_take_the_scalar_path
test_emulated__bits_are_the_backwards_visibility_count = gpu_tests.test_bits_are_the_backwards_visibility_count
test_emulated__entry_points_refuse_bad_arguments_before_any_launch = gpu_tests.test_entry_points_refuse_bad_arguments_before_any_launch


def test_the_emulated_library_served_these_tests():
    from lichtfeld_studio_amd import ops
    assert ops.load_library() is emul_util.library()
    assert emul_util.library().lfs_version().decode().endswith("src-unknown")
