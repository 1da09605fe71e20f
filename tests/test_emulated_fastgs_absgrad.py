"""tests/test_gpu_fastgs_absgrad.py on the CPU: the product library compiled as host code on the wavefront emulator, "cuda:0" served by CPU tensors (the fixture
pattern of tests/test_emulated_fastgs_depth.py). Same scenes, same float64 host model, same bounds. What this holds without a GPU is the kernels' logic: the two
absolute sums of the abs form of the blend backward over exactly the instances of the other sums, their way through the twelve-value reduction (the compiler-generated
branch the -DLFS_RED_ADDTID=0 library shares) into slots 10 / 11, fg_densify_abs_kernel, the flag's way through the mode word and the host's memory of the workspace,
and the Python layers. (The deterministic accumulation mode the tests ask for is dropped by the emulated library: its wavefronts run one after the other, the float
sums are reproducible as they are - so the bit comparisons hold here too.) GPU-only: the libtorch route (the emulator has no libtorch build)."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import emul_util  # noqa: E402
import test_gpu_fastgs_absgrad as gpu_tests  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _emulated_library_and_cpu_tensors():
    if not emul_util.available():
        pytest.skip("no clang++ to build the emulated library")
    import lichtfeld_studio_amd.fastgs  # noqa: F401  (before installed(): the loader hooks of every imported module of the package get patched)
    import lichtfeld_studio_amd.losses  # noqa: F401
    with emul_util.installed(), emul_util.cuda_requests_served_by_the_cpu():
        yield


test_emulated__absgrad_densification_info_matches_the_float64_model = gpu_tests.test_absgrad_densification_info_matches_the_float64_model
test_emulated__a_gaussian_whose_signed_gradient_cancels_is_seen_by_absgrad = gpu_tests.test_a_gaussian_whose_signed_gradient_cancels_is_seen_by_absgrad
test_emulated__without_cancellation_the_absolute_sum_is_the_signed_one = gpu_tests.test_without_cancellation_the_absolute_sum_is_the_signed_one
test_emulated__gradients_and_render_are_bit_identical_with_and_without_the_flag = gpu_tests.test_gradients_and_render_are_bit_identical_with_and_without_the_flag
test_emulated__flag_values_accumulation_and_the_optimizer_fused_backward = gpu_tests.test_flag_values_accumulation_and_the_optimizer_fused_backward
test_emulated__trainer_densifies_by_absolute_gradients = gpu_tests.test_trainer_densifies_by_absolute_gradients


def test_the_emulated_library_served_these_tests():
    from lichtfeld_studio_amd import fastgs
    assert fastgs.load_library() is emul_util.library()
    assert emul_util.library().lfs_version().decode().endswith("src-unknown")
