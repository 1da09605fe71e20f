"""Static check of the abs forms of the fastgs blend backward and of the absgrad densification kernel (no GPU; tools/kernel_resources.py on the shipped code object):
every fgs::fg_* kernel is free of scratch and AGPRs, the abs forms exist under their own names with the LDS block and the waves per SIMD of their default forms, and
fg_densify_abs_kernel exists. The default forms themselves are held to the parent commit's registers by tests/test_kernel_resources_fastgs_depth.py and
tests/test_kernel_resources_fastgs_filter3d.py, which this change leaves alone."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "lichtfeld-studio_amd", "liblfs_gsplat.so")
ABS = [f"fgs::fg_blend_bwd_abs_kernel<{acc}, {depth}>" for acc in (0, 1, 2) for depth in ("false", "true")]


@pytest.fixture(scope="module")
def table():
    if not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("library not built / no llvm-readelf")
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.kernels(LIB)


def test_no_fastgs_kernel_has_scratch_or_agprs(table):
    fg = [k for k in table if k.startswith("fgs::fg_")]
    assert len(fg) >= 60, len(fg)
    for k in fg:
        assert table[k]["scratch_bytes"] == 0 and table[k]["agprs"] == 0, (k, table[k])


def test_abs_forms_keep_the_lds_block_and_the_occupancy_of_their_default_forms(table):
    assert "fgs::fg_densify_abs_kernel" in table and table["fgs::fg_densify_abs_kernel"]["lds_bytes"] == 0
    assert sorted(k for k in table if "fg_blend_bwd_abs_kernel<" in k) == sorted(ABS)
    for k in ABS:
        base = k.replace("_abs_kernel", "_kernel")
        print(f"{k}: vgprs {table[k]['vgprs']} sgprs {table[k]['sgprs']} waves {table[k]['waves_per_simd']} | default form {table[base]['vgprs']} {table[base]['sgprs']} {table[base]['waves_per_simd']}")
        assert table[k]["lds_bytes"] == 4608 and table[base]["lds_bytes"] == 4608, (k, table[k], table[base])
        assert table[k]["waves_per_simd"] == table[base]["waves_per_simd"], (k, table[k], table[base])
