"""Static check of the fastgs blend and per-primitive kernels after the depth forms were added (no GPU; tools/kernel_resources.py on the shipped code objects):
no instantiation spills, and the default instantiations - the ones every step without depth runs - keep the register counts of the commit before the depth modes,
read from that commit's code object with the same tool and written down here. A depth form that leaks into the default path shows up HERE as a changed count."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "lichtfeld-studio_amd", "liblfs_gsplat.so")

# (VGPRs, LDS bytes) of the parent commit's instantiations -> the names they have now (the new template arguments: no depth)
PARENT = {
    "fgs::fg_blend_fwd_kernel<false>": (15, 0),
    "fgs::fg_blend_bwd_kernel<0, false>": (32, 4608), "fgs::fg_blend_bwd_kernel<1, false>": (32, 4608), "fgs::fg_blend_bwd_kernel<2, false>": (34, 4608),
    "fgs::fg_preprocess_kernel<false, false, 0>": (60, 0), "fgs::fg_preprocess_kernel<false, true, 0>": (60, 0),
    "fgs::fg_preprocess_kernel<true, false, 0>": (60, 0), "fgs::fg_preprocess_kernel<true, true, 0>": (60, 0),
    "fgs::fg_preprocess_bwd_kernel<false, false, 0>": (111, 0), "fgs::fg_preprocess_bwd_kernel<false, true, 0>": (124, 0),
    "fgs::fg_preprocess_bwd_kernel<true, false, 0>": (118, 192), "fgs::fg_preprocess_bwd_kernel<true, true, 0>": (124, 192),
    "fgs::fg_cull_kernel": (45, 18432), "fgs::fg_det_resolve_kernel": (7, 0),
}
DEPTH_FORMS = (["fgs::fg_blend_fwd_kernel<true>"] + [f"fgs::fg_blend_bwd_kernel<{acc}, true>" for acc in (0, 1, 2)]
               + [f"fgs::fg_preprocess_kernel<{lds}, {aa}, {d}>" for lds in ("false", "true") for aa in ("false", "true") for d in (1, 2)]
               + [f"fgs::fg_preprocess_bwd_kernel<{w2c}, {aa}, {d}>" for w2c in ("false", "true") for aa in ("false", "true") for d in (1, 2)])


@pytest.fixture(scope="module")
def table():
    if not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("library not built / no llvm-readelf")
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return {k: v for k, v in mod.kernels(LIB).items() if k.startswith("fgs::fg_")}


def test_no_instantiation_of_the_fastgs_kernels_spills(table):
    assert len(table) >= len(PARENT) + len(DEPTH_FORMS), sorted(table)
    for k in list(PARENT) + DEPTH_FORMS:
        assert k in table, k
    for k, v in table.items():
        assert v["scratch_bytes"] == 0 and v["agprs"] == 0, (k, v)


def test_default_instantiations_keep_the_parents_registers(table):
    for k, (vgprs, lds) in PARENT.items():
        assert (table[k]["vgprs"], table[k]["lds_bytes"]) == (vgprs, lds), (k, table[k])


def test_depth_forms_keep_the_occupancy_of_their_default_forms(table):
    """one more accumulator in the forward, one more reduced value in the backward (the same LDS block), one more term in the per-primitive backward"""
    assert table["fgs::fg_blend_fwd_kernel<true>"]["waves_per_simd"] == table["fgs::fg_blend_fwd_kernel<false>"]["waves_per_simd"] == 8
    for acc in (0, 1, 2):
        d, p = table[f"fgs::fg_blend_bwd_kernel<{acc}, true>"], table[f"fgs::fg_blend_bwd_kernel<{acc}, false>"]
        assert d["waves_per_simd"] == p["waves_per_simd"] == 8 and d["lds_bytes"] == p["lds_bytes"] and d["vgprs"] <= p["vgprs"] + 2, (acc, d, p)
    for k in DEPTH_FORMS:
        if "preprocess" in k:
            base = k.rsplit(",", 1)[0] + ", 0>"
            assert table[k]["waves_per_simd"] == table[base]["waves_per_simd"], (k, table[k], table[base])
