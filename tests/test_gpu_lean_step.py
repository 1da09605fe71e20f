"""GPU: the lean fused-tail training step (csrc/gut_step.hip: FwdLean) computes what the step computed before it left out the work its result does not need.
  1  the activated quaternions / scales / opacities are recomputed by gut_tail_kernel (csrc/lfs_activations.cuh) instead of stored by the projection kernel and read
     back: against lfs_gut_train_step, whose three passes read the stored values - also at the rows where that arithmetic branches
  2  the backward's accumulator clear: no stale row, no stale loss slot from the step before (written for the clear as a rider of the scan launch, which was
     measured and taken out again - profiles/r20/lean_step; the cases hold whatever clears the rows)
  3  the per-tile sort writes no keys: the lists are those of lfs_intersect_tile_count / _emit
Deterministic accumulation (debug bit 4) on, every comparison on the bytes, the loss value included (fewer wavefronts than loss slots at these image sizes:
lean_step_util.assert_same_loss) - but for the means under noise, which have no bitwise reference in the library (lean_step_util.check_activations); the cases and comparisons are tests/lean_step_util.py's, shared with the emulator's
tests/test_emulated_lean_step.py; one case of 2 also runs with float atomics, on the kernels a training run uses."""
import pytest

import lean_step_util as lean

pytestmark = pytest.mark.gpu


@pytest.fixture()
def be(lfs):
    import torch
    from lichtfeld_studio_amd.capi import stream
    lib = lfs.load_library()
    lib.lfs_set_debug_flags(16)
    try:
        yield lean.Backend(lib, torch=torch, device="cuda:0", stream=stream)
        torch.cuda.synchronize()
    finally:
        lib.lfs_set_debug_flags(0)


@pytest.mark.parametrize("degree", [3, 1])
@pytest.mark.parametrize("N", [37, 130, 4099])
def test_tail_recomputes_the_activations_bit_for_bit(be, N, degree):
    """N below one wavefront, ragged, several workgroups; a 40 x 24 image (partial tiles); two steps over two views (the second on the colours the first tail left)"""
    lean.check_activations(be, N, degree)


@pytest.mark.parametrize("mode", ["freeze", "noise"])
def test_tail_recomputes_the_activations_with_frozen_shN_and_with_noise(be, mode):
    lean.check_activations(be, 130, 3, mode=mode)


def test_next_colours_of_the_lean_tail(be):
    lean.check_next_colours(be, 130, 3)


@pytest.mark.parametrize("N", [1, 63, 1000, 4099])
def test_accumulator_rows_and_loss_slots_are_clear_for_every_step(be, N):
    lean.check_clear(be, N)


def test_accumulator_clear_around_an_overflowing_attempt(be):
    lean.check_clear(be, 1000, overflow=True)


@pytest.mark.parametrize("N", [63, 4099])
def test_accumulator_clear_with_float_atomics(be, N):
    be.lib.lfs_set_debug_flags(0)   # (the fixture puts the deterministic mode back off as well)
    lean.check_clear_with_float_atomics(be, N)


@pytest.mark.parametrize("equal_depths", [False, True])
@pytest.mark.parametrize("n_stack", [1, 1024, 1025, 4096, 4097])
def test_sort_without_key_write_back(be, n_stack, equal_depths):
    lean.check_sort(be, n_stack, equal_depths)
