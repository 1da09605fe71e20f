"""Cases 1-5 of tests/test_gpu_fastgs_antialiased.py on the CPU: the product library compiled as host code on the wavefront emulator, "cuda:0" served by CPU
tensors (the fixture pattern of tests/test_emulated_masked_loss.py). Same scenes, same float64 host model, same oracle calls, same bounds. What this holds without
a GPU is the kernels' logic: the compensation and the order of the cuts in the forward, the rho term of the per-primitive backward in both W2C forms, the mode word
of the workspace and the two backward instantiations picking by it, and the argument checks of lfs_fastgs_view_preprocess. (The deterministic accumulation mode the
tests ask for is dropped by the emulated library: its wavefronts run one after the other, the float sums are reproducible as they are.)"""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import emul_util  # noqa: E402
import test_gpu_fastgs_antialiased as gpu_tests  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _emulated_library_and_cpu_tensors():
    if not emul_util.available():
        pytest.skip("no clang++ to build the emulated library")
    import lichtfeld_studio_amd.fastgs  # noqa: F401  (before installed(): the loader hooks of every imported module of the package get patched)
    gpu_tests._expected_grads.cache_clear()
    with emul_util.installed(), emul_util.cuda_requests_served_by_the_cpu():
        yield
    gpu_tests._expected_grads.cache_clear()   # (results of the emulated library: a later -m gpu run in the same process computes its own)


test_emulated__antialiased_forward_is_the_default_forward_at_the_compensated_opacity = gpu_tests.test_antialiased_forward_is_the_default_forward_at_the_compensated_opacity
test_emulated__antialiased_backward_is_the_composition = gpu_tests.test_antialiased_backward_is_the_composition
test_emulated__antialiased_cuts = gpu_tests.test_antialiased_cuts
test_emulated__default_mode_is_untouched = gpu_tests.test_default_mode_is_untouched
test_emulated__antialiased_pose_gradient = gpu_tests.test_antialiased_pose_gradient


def test_the_emulated_library_served_these_tests():
    from lichtfeld_studio_amd import fastgs
    assert fastgs.load_library() is emul_util.library()
    assert emul_util.library().lfs_version().decode().endswith("src-unknown")
