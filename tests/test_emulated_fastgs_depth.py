"""tests/test_gpu_fastgs_depth.py on the CPU: the product library compiled as host code on the wavefront emulator, "cuda:0" served by CPU tensors (the fixture
pattern of tests/test_emulated_fastgs_antialiased.py). Same scenes, same float64 host model, same oracle calls, same bounds. What this holds without a GPU is the
kernels' logic: d_i in the record and the mode word, the extra accumulator of the forward over exactly the colour's instances, depth as a fourth blended channel of
the backward and its tenth reduced value, dL/dz in grad_means and in row 2 of grad_w2c for both kinds, the host-side flag memory behind the two depth entry points,
and the argument checks. (The deterministic accumulation mode the tests ask for is dropped by the emulated library: its wavefronts run one after the other, the
float sums are reproducible as they are.) One case is GPU-only for that reason, the 3000-Gaussian scene of the linearity test: the 1e-6 bound budgets the roundings
of one backward whose rows are accumulated exactly, which is what the deterministic mode provides; the emulated library adds the cells' sums in float32, and at
N = 3000 (the scene with the most cells per Gaussian) those extra roundings put the most ill-conditioned tensor at the bound - rot_raw 1.01e-6 emulated, 5.9e-7 on
the GPU. The other two scenes of that test run here."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import emul_util  # noqa: E402
import test_gpu_fastgs_depth as gpu_tests  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _emulated_library_and_cpu_tensors():
    if not emul_util.available():
        pytest.skip("no clang++ to build the emulated library")
    import lichtfeld_studio_amd.fastgs  # noqa: F401  (before installed(): the loader hooks of every imported module of the package get patched)
    import lichtfeld_studio_amd.losses  # noqa: F401
    with emul_util.installed(), emul_util.cuda_requests_served_by_the_cpu():
        yield


test_emulated__depth_forward_is_the_colour_forward_of_the_twin = gpu_tests.test_depth_forward_is_the_colour_forward_of_the_twin
test_emulated__depth_only_backward_is_the_twins_colour_backward = gpu_tests.test_depth_only_backward_is_the_twins_colour_backward



@pytest.mark.parametrize("idx,kind", [c for c in gpu_tests.LINEARITY_CASES if gpu_tests.CFGS[c[0]]["N"] != 3000], ids=gpu_tests.CASE_IDS)
def test_emulated__depth_backward_is_linear_in_its_three_gradients(lfs, idx, kind):
    gpu_tests.test_depth_backward_is_linear_in_its_three_gradients(lfs, idx, kind)


test_emulated__depth_camera_gradient = gpu_tests.test_depth_camera_gradient
test_emulated__default_mode_is_untouched_by_the_depth_modes = gpu_tests.test_default_mode_is_untouched_by_the_depth_modes
test_emulated__fast_rasterize_render_modes_and_autograd = gpu_tests.test_fast_rasterize_render_modes_and_autograd
test_emulated__adam_is_refused_with_grad_w2c_and_with_grad_depth = gpu_tests.test_adam_is_refused_with_grad_w2c_and_with_grad_depth


def test_the_emulated_library_served_these_tests():
    from lichtfeld_studio_amd import fastgs
    assert fastgs.load_library() is emul_util.library()
    assert emul_util.library().lfs_version().decode().endswith("src-unknown")
