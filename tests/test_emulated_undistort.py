"""The test bodies of tests/test_gpu_undistort.py on the CPU: the product library compiled as host code on the wavefront emulator, "cuda:0" served by CPU tensors
(the fixture pattern of tests/test_emulated_masked_loss.py). Same cases, same float64 model, same bounds. What this holds without a GPU is the kernels' logic: the
pixel convention, both lens models through the header's functions, the validity rule, the tap and its re-quantisation, threshold / invert / blank pixels, the integer
sums at ragged sizes and in the one-block case, the nearest-neighbour pick, the argument checks, and the loader's choice between the old and the new entry points."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import emul_util  # noqa: E402
import test_gpu_undistort as gpu_tests  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _emulated_library_and_cpu_tensors():
    if not emul_util.available():
        pytest.skip("no clang++ to build the emulated library")
    import lichtfeld_studio_amd.loader  # noqa: F401  (before installed(): the loader hooks of every imported module of the package get patched)
    import lichtfeld_studio_amd.losses  # noqa: F401
    with emul_util.installed(), emul_util.cuda_requests_served_by_the_cpu():
        yield


test_emulated__image_matches_the_f64_model = gpu_tests.test_image_matches_the_f64_model
test_emulated__mask_entry_matches_the_f64_model_and_its_sums_are_exact = gpu_tests.test_mask_entry_matches_the_f64_model_and_its_sums_are_exact
test_emulated__plane_entry_picks_the_models_texel = gpu_tests.test_plane_entry_picks_the_models_texel
test_emulated__a_depth_file_of_another_size_goes_through_the_same_map = gpu_tests.test_a_depth_file_of_another_size_goes_through_the_same_map
test_emulated__entry_points_refuse_bad_arguments_before_any_launch = gpu_tests.test_entry_points_refuse_bad_arguments_before_any_launch
test_emulated__a_pinhole_dataset_is_untouched_by_the_option = gpu_tests.test_a_pinhole_dataset_is_untouched_by_the_option
test_emulated__a_distorted_dataset_without_the_option_loads_as_before_and_with_it_through_the_maps = \
    gpu_tests.test_a_distorted_dataset_without_the_option_loads_as_before_and_with_it_through_the_maps


def test_the_emulated_library_served_these_tests():
    from lichtfeld_studio_amd import losses
    assert losses.load_library() is emul_util.library()
    assert emul_util.library().lfs_version().decode().endswith("src-unknown")
