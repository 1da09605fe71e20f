"""The test bodies of tests/test_gpu_mcmc_relocate.py on the CPU: the product library compiled as host code on the wavefront emulator, "cuda:0" served by CPU
tensors (the pattern of tests/test_emulated_sog.py). Same inputs, same host model, same assertions. What this holds without a GPU is the logic of the six
relocation kernels: the carry of the block scan across chunks of 256 block sums, the ragged last thread and last block, the strict cdf > target rule at its
edges, the count clamp and the copy / zeroing rules. What it cannot hold is the device's expf (the margin of the general-weights tier is there for it)."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import emul_util  # noqa: E402
import test_gpu_mcmc_relocate as gpu_tests  # noqa: E402

# sizes of the exact tier that are NOT taken, each with the reason (the GPU run keeps every size)
NOT_TAKEN = {}


@pytest.fixture(scope="module", autouse=True)
def _emulated_library_and_cpu_tensors():
    if not emul_util.available():
        pytest.skip("no clang++ to build the emulated library")
    with emul_util.installed(), emul_util.cuda_requests_served_by_the_cpu():
        yield


@pytest.mark.parametrize("N", [s for s in gpu_tests.EXACT_SIZES if s not in NOT_TAKEN])
def test_emulated__exact_weights_give_the_models_sources_bit_for_bit(N):
    gpu_tests.exact_tier(N)


test_emulated__general_weights_sources_exact_and_values_within_the_relocation_bars = gpu_tests.test_general_weights_sources_exact_and_values_within_the_relocation_bars
test_emulated__targets_on_block_boundaries_never_draw_a_dead_source = gpu_tests.test_targets_on_block_boundaries_never_draw_a_dead_source
test_emulated__a_source_drawn_130_times_is_relocated_with_n_max = gpu_tests.test_a_source_drawn_130_times_is_relocated_with_n_max
test_emulated__nothing_alive_changes_nothing = gpu_tests.test_nothing_alive_changes_nothing
test_emulated__optional_pointers_do_not_change_the_result = gpu_tests.test_optional_pointers_do_not_change_the_result
test_emulated__bad_arguments_are_refused_before_any_launch = gpu_tests.test_bad_arguments_are_refused_before_any_launch


def test_the_emulated_library_served_these_tests():
    from lichtfeld_studio_amd import capi
    assert capi.load_library() is emul_util.library()
    assert emul_util.library().lfs_version().decode().endswith("src-unknown")
