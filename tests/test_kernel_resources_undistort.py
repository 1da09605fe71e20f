"""Static check of the undistortion kernels (no GPU; tools/kernel_resources.py on the shipped code object): the one templated body exists once per payload - image,
mask, plane - and none of the three spills: no scratch, no AGPRs. The camera block is a by-value kernel argument, so its coefficients cost SGPRs, not VGPRs: every
form keeps the full 8 waves per SIMD; only the mask form uses LDS (the 32 bytes of its block sums)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "lichtfeld-studio_amd", "liblfs_gsplat.so")
KERNELS = [f"ud::undistort_kernel<ud::{p}>" for p in ("ImagePayload", "MaskPayload", "PlanePayload")]


@pytest.fixture(scope="module")
def table():
    if not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("library not built / no llvm-readelf")
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.kernels(LIB)


def test_the_three_forms_exist_without_scratch_or_spills(table):
    for k in KERNELS:
        assert k in table, (k, [n for n in table if "undistort" in n])
        print(f"{k}: {table[k]}")
        assert table[k]["scratch_bytes"] == 0 and table[k]["agprs"] == 0, (k, table[k])
    assert len([k for k in table if "undistort_kernel<" in k]) == len(KERNELS)


def test_the_three_forms_keep_full_occupancy(table):
    for k in KERNELS:
        assert table[k]["waves_per_simd"] == 8, (k, table[k])
        assert table[k]["lds_bytes"] == (32 if "MaskPayload" in k else 0), (k, table[k])
