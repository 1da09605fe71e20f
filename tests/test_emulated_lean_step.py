"""The lean fused-tail training step (csrc/gut_step.hip: FwdLean - no activation round trip, no key write-back in the per-tile sort, no tiles_per_gauss) compiled as
HOST code on the wavefront emulator (tests/emul), at the smaller sizes of tests/test_gpu_lean_step.py: the cases and the comparisons are tests/lean_step_util.py's. The deterministic accumulation mode is compiled out here; the emulator runs one lane after the other, so every sum has
one order and the comparisons are exact, the loss value included. The workspace starts as 0xFF bytes (NaN) and is replaced by such a block between the steps of the
overflow case: a part of it the step reads before it writes it shows."""
import ctypes as C
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
CSRC = os.path.join(ROOT, "lichtfeld-studio_amd", "csrc")
sys.path.insert(0, HERE)

import lean_step_util as lean  # noqa: E402


@pytest.fixture(scope="module")
def be(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ to build the emulated kernels")
    out = str(tmp_path_factory.mktemp("emul") / "liblfs_lean_emul.so")
    srcs = [os.path.join(CSRC, f) for f in ("intersect.hip", "raster.hip", "projection_ut.hip", "sh.hip", "gut_step.hip")]
    cmd = [CLANG, "-x", "c++", "-std=c++17", "-O1", "-DLFS_EMULATE", "-fPIC", "-shared", "-ffp-contract=on", "-I" + os.path.join(HERE, "emul"), "-Wno-unused-value",
           "-Wno-unknown-attributes", *srcs, os.path.join(HERE, "emul", "emul_stubs.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return lean.Backend(C.CDLL(out))


@pytest.mark.parametrize("N,degree", [(37, 3), (37, 1), (130, 3)])
def test_tail_recomputes_the_activations_bit_for_bit(be, N, degree):
    lean.check_activations(be, N, degree)


@pytest.mark.parametrize("mode", ["freeze", "noise"])
def test_tail_recomputes_the_activations_with_frozen_shN_and_with_noise(be, mode):
    lean.check_activations(be, 37, 3, mode=mode)


def test_next_colours_of_the_lean_tail(be):
    lean.check_next_colours(be, 37, 3)


@pytest.mark.parametrize("N", [1, 63, 1000])
def test_accumulator_rows_and_loss_slots_are_clear_for_every_step(be, N):
    lean.check_clear(be, N)


def test_accumulator_clear_around_an_overflowing_attempt(be):
    lean.check_clear(be, 63, overflow=True)


def test_accumulator_clear_step_by_step(be):
    """(the device test's form for float atomics: step k + 1 of the three-pass form from the fused run's state after step k - exact here for every row)"""
    lean.check_clear_with_float_atomics(be, 63)


@pytest.mark.parametrize("equal_depths", [False, True])
@pytest.mark.parametrize("n_stack", [1, 1024, 1025, 4096, 4097])
def test_sort_without_key_write_back(be, n_stack, equal_depths):
    lean.check_sort(be, n_stack, equal_depths)
