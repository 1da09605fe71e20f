"""The scene transform without a GPU (bodies: tests/splat_transform_reference.py, shared with tests/test_gpu_splat_transform.py).

First the pure host functions through the BUILT library: lfs_sh_rotation_matrices (orthogonality, the defining identity, the homomorphism), every refusal and the
accepted scales of lfs_splat_transform_from_matrix, the identity record, the refusals of lfs_splat_transform_apply before any launch, transform_cameras, and the
argument refusals of tools/transform_splat.py. Then csrc/splat_transform.hip compiled as host code on the wavefront emulator ("cuda:0" served by CPU tensors, the
pattern of tests/test_emulated_fastgs_filter3d.py): the kernels against the float32 model bit for bit and the float64 model within the derived bounds at every size
and SH layout, in and out of place, on 16-byte- and 4-byte-aligned buffers with NaN guards; round trips; skipped pairs; transform_model and crop; and the render
invariance through the emulated fastgs rasterizer, with the reference's behaviour (shN left alone) shown to fail it."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import emul_util  # noqa: E402
import splat_transform_reference as ref  # noqa: E402

DEV = "cuda:0"


# ---- the built library's host functions ----------------------------------------------------------------------------------------------------------------------------
def test_band_matrices(lfs):
    ref.check_band_matrices(lfs)


def test_from_matrix_refusals_scales_identity_inverse(lfs):
    ref.check_from_matrix(lfs)


def test_apply_refuses_before_any_launch(lfs):
    ref.check_entry_refusals(lfs)


def test_transform_cameras(lfs):
    ref.check_transform_cameras()


def test_tool_refuses_bad_arguments_without_loading_torch():
    import subprocess
    code = (
        "import sys; sys.path.insert(0, %r); import transform_splat as t\n"
        "def refused(argv):\n"
        "    try:\n"
        "        t.check_args(t.build_parser().parse_args(argv))\n"
        "    except SystemExit as e:\n"
        "        return isinstance(e.code, str)\n"
        "    return False\n"
        "io = ['--ply', 'a.ply', '--out', 'b']\n"
        "assert refused(io), 'neither a transform nor a crop'\n"
        "assert refused(['--out', 'b', '--scale', '2']), 'no input'\n"
        "assert refused(['--ply', 'a.ply', '--sog', 'a.sog', '--out', 'b', '--scale', '2']), 'two inputs'\n"
        "assert refused(['--ply', 'a.txt', '--out', 'b', '--scale', '2'])\n"
        "assert refused(io + ['--scale', '0']) and refused(io + ['--scale', '-1']) and refused(io + ['--scale', 'nan'])\n"
        "assert refused(io + ['--matrix'] + ['1'] * 16 + ['--scale', '2']), 'a matrix and parts'\n"
        "assert refused(io + ['--matrix'] + ['1'] * 15 + ['nan'])\n"
        "assert refused(io + ['--rotate', 'w', '30']) and refused(io + ['--rotate', 'x', 'inf'])\n"
        "assert refused(io + ['--crop-min', '0', '0', '0']), 'half a box'\n"
        "assert refused(io + ['--crop-min', '0', '0', '0', '--crop-max', '1', '-1', '1']), 'an empty box'\n"
        "assert refused(io + ['--crop-invert', '--scale', '2']), 'invert without a box'\n"
        "for ok in (['--scale', '2'], ['--rotate', 'x', '90', '--rotate', 'z', '-30', '--translate', '1', '2', '3'], ['--matrix'] + ['1'] * 16,\n"
        "           ['--crop-min', '0', '0', '0', '--crop-max', '1', '1', '1', '--crop-invert']):\n"
        "    assert not refused(io + ok), ok\n"
        "m = t.matrix_of(t.build_parser().parse_args(io + ['--rotate', 'z', '90', '--scale', '2', '--translate', '1', '0', '0']))\n"
        "assert [[round(v, 12) for v in r] for r in m] == [[0, -2, 0, 1], [2, 0, 0, 0], [0, 0, 2, 0], [0, 0, 0, 1]], m\n"
        "a = t.build_parser().parse_args(io + ['--matrix'] + ['-1e-05'] * 15 + ['1'] + ['--crop-min', '-1e-3', '-2.5', '-.5', '--crop-max', '1', '1', '1'])\n"
        "assert a.matrix[0] == -1e-05 and a.crop_min == [-1e-3, -2.5, -0.5]\n"
        "assert 'torch' not in sys.modules\n"
        "print('ok')\n") % os.path.join(os.path.dirname(HERE), "tools")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]


# ---- the kernels on the wavefront emulator ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emulated():
    if not emul_util.available():
        pytest.skip("no clang++ to build the emulated library")
    import lichtfeld_studio_amd.fastgs  # noqa: F401  (before installed(): the loader hooks of every imported module of the package get patched)
    import lichtfeld_studio_amd.transform  # noqa: F401
    with emul_util.installed(), emul_util.cuda_requests_served_by_the_cpu():
        yield


def test_emulated__kernel_sizes_layouts_in_place_alignment(emulated):
    ref.check_kernel_sizes(DEV)


def test_emulated__other_transforms(emulated):
    ref.check_transforms(DEV)


def test_emulated__round_trip(emulated):
    ref.check_round_trip(DEV)


def test_emulated__skipped_pairs(emulated):
    ref.check_skipped_pairs(DEV)


def test_emulated__transform_model(emulated):
    ref.check_transform_model(DEV)


def test_emulated__crop(emulated):
    ref.check_crop(DEV)


def test_emulated__render_invariance_fastgs(emulated):
    ref.check_render_invariance(DEV, "fastgs")


def test_the_emulated_library_served_these_tests(emulated):
    from lichtfeld_studio_amd import transform
    assert transform.load_library() is emul_util.library()
    assert emul_util.library().lfs_version().decode().endswith("src-unknown")
