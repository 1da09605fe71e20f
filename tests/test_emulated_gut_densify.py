"""tests/test_gpu_gut_densify.py on the CPU: the product library compiled as host code on the wavefront emulator, "cuda:0" served by CPU tensors (the fixture pattern of
tests/test_emulated_fastgs_absgrad.py). Same scenes, same float64 formula, same bounds. What this holds without a GPU is the logic of the densifying finish pass - its
operand loads in the emulated branch of the shared body, the statistic's arithmetic, the store guard of the tail lanes, the per-view accumulation - and the way of
densification_info through the four _ex entries, gut_step.py, fused.py and the trainer's step forms. (The deterministic accumulation mode the tests ask for is dropped by
the emulated library: its wavefronts run one after the other, the float sums are reproducible as they are - so the bit comparisons hold here too.) The entry tests run
on a 700-Gaussian scene here. GPU-only: the N = 6000 cases, the 40-step trainer runs (a minute and a half here; one step of the trainer through the forced factored
form is kept) and the export lookup on the shipped library, which tests/test_capi_symbols.py does on this side."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import emul_util  # noqa: E402
import test_gpu_gut_densify as gpu_tests  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _emulated_library_and_cpu_tensors():
    if not emul_util.available():
        pytest.skip("no clang++ to build the emulated library")
    import lichtfeld_studio_amd.fused  # noqa: F401  (before installed(): the loader hooks of every imported module of the package get patched)
    import lichtfeld_studio_amd.gut_step  # noqa: F401
    import lichtfeld_studio_amd.losses  # noqa: F401
    with emul_util.installed(), emul_util.cuda_requests_served_by_the_cpu():
        yield


@pytest.mark.parametrize("n,view", [(1, 0), (63, 0), (65, 0), (257, 0), (257, 1)])
def test_emulated__statistic_matches_the_float64_formula_and_the_gradients_keep_their_bits(lfs, n, view):
    gpu_tests.test_statistic_matches_the_float64_formula_and_the_gradients_keep_their_bits(lfs, n, view)


test_emulated__statistic_is_positive_somewhere_on_the_single_gaussian_scene = gpu_tests.test_statistic_is_positive_somewhere_on_the_single_gaussian_scene


def test_emulated__accumulating_call_adds_the_views_own_statistic(lfs):
    gpu_tests.test_accumulating_call_adds_the_views_own_statistic(lfs, 65)


def test_emulated__combined_entry_and_its_halves_give_the_bits_of_the_rows_entry(lfs):
    gpu_tests.test_combined_entry_and_its_halves_give_the_bits_of_the_rows_entry(lfs, n=700)


def test_emulated__operator_route_gives_the_same_bits_and_refuses_without_the_fused_finish(lfs):
    gpu_tests.test_operator_route_gives_the_same_bits_and_refuses_without_the_fused_finish(lfs, n=700)


test_emulated__forced_collectives_statistic_of_one_step_equals_the_unforced_one = gpu_tests.test_forced_collectives_statistic_of_one_step_equals_the_unforced_one
test_emulated__combinations_without_a_finish_pass_still_raise = gpu_tests.test_combinations_without_a_finish_pass_still_raise


def test_the_emulated_library_served_these_tests():
    from lichtfeld_studio_amd import gut_step
    assert gut_step.load_library() is emul_util.library()
    assert emul_util.library().lfs_version().decode().endswith("src-unknown")
