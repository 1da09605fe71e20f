"""tests/test_gpu_fastgs_contribution.py on the CPU: the product library compiled as host code on the wavefront emulator, "cuda:0" served by CPU tensors (the fixture
pattern of tests/test_emulated_gut_densify.py). Same scenes (N <= 306), same twin renders, same bounds. What this holds without a GPU is the kernel's logic: the walk
and the transmittance recurrence against the forward's, the blended / terminating split, the two wave reductions (DPP rows, readlane across them) and the ballot count, lanes outside the image, the three
integer updates of a row and their accumulation over calls, the refusals, the folding of contribution.compute_contribution, and the trainer's prune hook on one small scene (the 4145-Gaussian
trainer runs stay on the GPU). What it cannot hold is the ISA side
(the atomics as the hardware executes them, v_exp_f32): the GPU file. The two are not compared with each other."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import emul_util  # noqa: E402
import test_gpu_contribution_training as trainer_tests  # noqa: E402
import test_gpu_fastgs_contribution as gpu_tests  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _emulated_library_and_cpu_tensors():
    if not emul_util.available():
        pytest.skip("no clang++ to build the emulated library")
    import lichtfeld_studio_amd.contribution  # noqa: F401  (before installed(): the loader hooks of every imported module of the package get patched)
    import lichtfeld_studio_amd.losses  # noqa: F401
    with emul_util.installed(), emul_util.cuda_requests_served_by_the_cpu():
        yield


test_emulated__statistic_equals_the_per_pixel_weight_map_of_the_twin_render = gpu_tests.test_statistic_equals_the_per_pixel_weight_map_of_the_twin_render
test_emulated__weights_of_a_view_sum_to_its_alpha_map = gpu_tests.test_weights_of_a_view_sum_to_its_alpha_map
test_emulated__weights_stay_below_the_alpha_clamp = gpu_tests.test_weights_stay_below_the_alpha_clamp
test_emulated__gaussians_behind_the_point_of_termination_have_an_empty_row = gpu_tests.test_gaussians_behind_the_point_of_termination_have_an_empty_row
test_emulated__gaussians_outside_the_frustum_have_an_empty_row = gpu_tests.test_gaussians_outside_the_frustum_have_an_empty_row
test_emulated__rows_are_bit_reproducible_and_independent_of_the_order_of_views = gpu_tests.test_rows_are_bit_reproducible_and_independent_of_the_order_of_views
test_emulated__entry_refuses_before_any_launch_and_leaves_the_rows_untouched = gpu_tests.test_entry_refuses_before_any_launch_and_leaves_the_rows_untouched
test_emulated__a_camera_that_looks_away_has_no_instances_and_changes_nothing = gpu_tests.test_a_camera_that_looks_away_has_no_instances_and_changes_nothing
test_emulated__the_call_leaves_image_and_alpha_of_the_render_as_they_were = gpu_tests.test_the_call_leaves_image_and_alpha_of_the_render_as_they_were
test_emulated__compute_contribution_folds_without_changing_a_bit = gpu_tests.test_compute_contribution_folds_without_changing_a_bit

test_emulated__prune_inside_three_steps_on_a_small_scene = trainer_tests.test_prune_inside_three_steps_on_a_small_scene   # the trainer's hook, one small scene


def test_the_emulated_library_served_these_tests():
    from lichtfeld_studio_amd import ops
    assert ops.load_library() is emul_util.library()
    assert emul_util.library().lfs_version().decode().endswith("src-unknown")
