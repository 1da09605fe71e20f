"""Static check of the visible-only Adam kernels (no GPU; tools/kernel_resources.py on the shipped code object): both exist, neither spills - no scratch, no AGPRs -
neither uses LDS (the compaction hands rows over with a shuffle), and both keep the full 8 waves per SIMD of a streaming kernel: the Adam kernel asks for them in
its launch bounds (62 VGPRs; 71 and 7 waves without), the visibility kernel needs 6 VGPRs."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "lichtfeld-studio_amd", "liblfs_gsplat.so")
KERNELS = ["adamv::adam_multi_visible_kernel", "adamv::visibility_kernel"]


@pytest.fixture(scope="module")
def table():
    if not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("library not built / no llvm-readelf")
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.kernels(LIB)


def test_both_kernels_exist_without_scratch_or_spills(table):
    for k in KERNELS:
        assert k in table, (k, [n for n in table if "adam" in n])
        print(f"{k}: {table[k]}")
        assert table[k]["scratch_bytes"] == 0 and table[k]["agprs"] == 0 and table[k]["lds_bytes"] == 0, (k, table[k])
    assert len([k for k in table if k.startswith("adamv::")]) == len(KERNELS)


def test_both_kernels_keep_full_occupancy(table):
    for k in KERNELS:
        assert table[k]["waves_per_simd"] == 8, (k, table[k])


def test_the_dense_kernels_are_still_there(table):
    assert "adam_kernel" in table and "adam_multi_kernel" in table
