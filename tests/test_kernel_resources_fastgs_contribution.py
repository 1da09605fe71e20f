"""Static check of the contribution kernel (no GPU; tools/kernel_resources.py on the shipped code object): fgs::fg_contrib_kernel is in the library, does not spill - no
scratch, no AGPRs - uses no LDS (the two wave reductions are cross-lane moves, the records arrive through the scalar unit) and keeps the 8 waves per SIMD of the forward
whose walk it repeats (11 VGPRs; the forward has 15)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "lichtfeld-studio_amd", "liblfs_gsplat.so")
KERNEL = "fgs::fg_contrib_kernel"


@pytest.fixture(scope="module")
def table():
    if not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("library not built / no llvm-readelf")
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.kernels(LIB)


def test_kernel_is_shipped_without_scratch_lds_or_spills(table):
    assert KERNEL in table, [n for n in table if "contrib" in n]
    print(f"{KERNEL}: {table[KERNEL]}")
    assert table[KERNEL]["scratch_bytes"] == 0 and table[KERNEL]["agprs"] == 0 and table[KERNEL]["lds_bytes"] == 0, table[KERNEL]
    assert table[KERNEL]["max_workgroup"] == 64      # one wavefront per 8x8 cell
    assert len([k for k in table if "contrib" in k]) == 1


def test_kernel_keeps_full_occupancy(table):
    assert table[KERNEL]["vgprs"] <= 64 and table[KERNEL]["waves_per_simd"] == 8, table[KERNEL]


def test_the_blend_kernels_are_still_there(table):
    assert "fgs::fg_blend_fwd_kernel<false>" in table and "fgs::fg_blend_fwd_kernel<true>" in table and "fgs::fg_cull_kernel" in table
