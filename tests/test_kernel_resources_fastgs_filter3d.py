"""Static check of the filtered forms of the fastgs per-primitive kernels and of the filter-variance kernels (no GPU; tools/kernel_resources.py on the shipped code
object): every filtered form exists under its own name, none has scratch or AGPRs, and each keeps (at least) the waves per SIMD of its unfiltered form. The unfiltered
forms themselves are held to the parent commit's registers by tests/test_kernel_resources_fastgs_depth.py, which this change leaves alone."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "lichtfeld-studio_amd", "liblfs_gsplat.so")
B = ("false", "true")
FORWARD = [f"fgs::fg_preprocess_f3d_kernel<{lds}, {aa}, {d}>" for lds in B for aa in B for d in (0, 1, 2)]
BACKWARD = [f"fgs::fg_preprocess_bwd_f3d_kernel<{w2c}, {aa}, {d}>" for w2c in B for aa in B for d in (0, 1, 2)]
COMPUTE = ["f3d::filter3d_nu_kernel", "f3d::filter3d_finish_kernel"]


@pytest.fixture(scope="module")
def table():
    if not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("library not built / no llvm-readelf")
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.kernels(LIB)


def test_every_filtered_form_exists_without_scratch_or_agprs(table):
    for k in FORWARD + BACKWARD + COMPUTE:
        assert k in table, k
        assert table[k]["scratch_bytes"] == 0 and table[k]["agprs"] == 0, (k, table[k])
    assert len([k for k in table if "_f3d_kernel<" in k]) == len(FORWARD) + len(BACKWARD)


def test_filtered_forms_keep_the_occupancy_of_their_unfiltered_forms(table):
    """one more dword read and a few VALU instructions per primitive. (The filtered forward forms are capped at 96 SGPRs - csrc/fastgs_prep.hip - so those with the LDS
    histogram come out one wave ABOVE their unfiltered forms in the tool's model; no form may come out below.)"""
    for k in FORWARD + BACKWARD:
        base = k.replace("_f3d_kernel", "_kernel")
        print(f"{k}: vgprs {table[k]['vgprs']} sgprs {table[k]['sgprs']} waves {table[k]['waves_per_simd']} | unfiltered {table[base]['vgprs']} {table[base]['sgprs']} {table[base]['waves_per_simd']}")
        assert table[k]["waves_per_simd"] >= table[base]["waves_per_simd"], (k, table[k], table[base])
        assert table[k]["lds_bytes"] == table[base]["lds_bytes"], (k, table[k], table[base])
    for k in BACKWARD:
        assert table[k]["waves_per_simd"] == table[k.replace("_f3d_kernel", "_kernel")]["waves_per_simd"]
    for k in COMPUTE:
        assert table[k]["waves_per_simd"] == 8 and table[k]["lds_bytes"] == 0, (k, table[k])
