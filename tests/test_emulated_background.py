"""The background colour without a GPU (bodies: tests/background_reference.py, shared with tests/test_gpu_background.py).

First what needs no kernel: the policy (background.py: the reference's modulation table, the mix weights, the random and the jittered colours, GutTrainer's
validation), the refusals of the two entries before any launch through the BUILT library, the training tool's refusals. Then csrc/background.hip compiled as host
code on the wavefront emulator ("cuda:0" served by CPU tensors, the pattern of tests/test_emulated_splat_transform.py): both kernels in both forms against the float32
model bit for bit at every size, on 16-byte- and 4-byte-aligned buffers with NaN guards, in and out of place; the wrapper's refusals; preload_alphas; and the fastgs
trainer step with a colour and with RGBA planes on a small scene."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import background_reference as ref  # noqa: E402
import emul_util  # noqa: E402

DEV = "cuda:0"


# ---- host only -------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_policy_modulation_table_and_mix_weights(lfs):
    ref.check_policy_table()


def test_policy_random_and_jitter(lfs):
    ref.check_policy_random_and_jitter()


def test_entries_refuse_before_any_launch(lfs):
    ref.check_entry_refusals(lfs)


def test_tool_refuses_bad_background_arguments_without_loading_the_package():
    code = (
        "import sys; sys.path.insert(0, %r); import train_colmap as t\n"
        "def refused(argv):\n"
        "    try:\n"
        "        t.check_args(t.build_parser().parse_args(['-d', 'x'] + argv))\n"
        "    except SystemExit as e:\n"
        "        return isinstance(e.code, str)\n"
        "    return False\n"
        "assert refused(['--random-background', '--bg-modulation'])\n"
        "assert refused(['--white-background', '--background', '0', '0', '0'])\n"
        "assert refused(['--background', '0.5', '1.5', '0']) and refused(['--background', '0.5', 'nan', '0']) and refused(['--background', '-0.1', '0', '0'])\n"
        "for ok in ([], ['--white-background', '--alpha-targets'], ['--background', '0.2', '0.4', '0.6', '--random-background'], ['--bg-modulation', '--gut']):\n"
        "    assert not refused(ok), ok\n"
        "a = t.build_parser().parse_args(['-d', 'x', '--white-background']); t.check_args(a); assert a.background == [1.0, 1.0, 1.0]\n"
        "assert 'lichtfeld_studio_amd' not in sys.modules\n"
        "print('ok')\n") % os.path.join(os.path.dirname(HERE), "tools")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]


# ---- the kernels on the wavefront emulator -----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emulated():
    if not emul_util.available():
        pytest.skip("no clang++ to build the emulated library")
    import lichtfeld_studio_amd.fastgs  # noqa: F401  (before installed(): the loader hooks of every imported module of the package get patched)
    import lichtfeld_studio_amd.loader  # noqa: F401
    import lichtfeld_studio_amd.evaluate  # noqa: F401
    with emul_util.installed(), emul_util.cuda_requests_served_by_the_cpu():
        yield


@pytest.mark.parametrize("bg", ref.COLOURS, ids=["black", "white", "colour"])
def test_emulated__kernels_sizes_groups_in_place_alignment(emulated, bg):
    ref.check_kernels(DEV, bg)


def test_emulated__wrapper_refusals(emulated):
    ref.check_wrapper_refusals(DEV)


def test_emulated__trainer_policy(emulated):
    ref.check_trainer_policy(DEV)


def test_emulated__preload_alphas(emulated, tmp_path):
    ref.check_preload_alphas(DEV, tmp_path)


@pytest.mark.parametrize("loss,segment", [("mse", False), ("l1_ssim", True)], ids=["mse", "l1_ssim_segment"])
def test_emulated__fastgs_step_matches_autograd(emulated, loss, segment):
    ref.check_fastgs_step_matches_autograd(DEV, loss, segment, n=300, sh_degree=1)


@pytest.mark.parametrize("bg", [ref.BG, (0.0, 0.0, 0.0)], ids=["colour", "black"])
def test_emulated__rgba_step(emulated, bg):
    ref.check_rgba_step(DEV, bg, n=300, sh_degree=1)


def test_emulated__defaults_are_the_parents(emulated, lfs):
    ref.check_defaults_are_the_parents(sys.modules["lichtfeld_studio_amd.capi"], DEV, n=300, sh_degree=1)


def test_the_emulated_library_served_these_tests(emulated):
    from lichtfeld_studio_amd import ops
    assert ops.load_library() is emul_util.library()
    assert emul_util.library().lfs_version().decode().endswith("src-unknown")
