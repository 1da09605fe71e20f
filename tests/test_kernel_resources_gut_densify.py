"""CPU: the densifying form of the gradient-tensor finish pass in the shipped code object (tools/kernel_resources.py on lichtfeld-studio_amd/liblfs_gsplat.so). It is
a kernel under its own name - raster_finish_densify_kernel, in a code object of its own (csrc/raster_densify.hip) - next to the two default forms, which keep their
names; it spills nothing, uses no AGPRs, and keeps the occupancy floor tests/test_kernel_resources.py sets for this pass (4 wavefronts per SIMD)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "lichtfeld-studio_amd", "liblfs_gsplat.so")
NEW = "raster_finish_densify_kernel"


@pytest.fixture(scope="module")
def table():
    if not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("library not built / no llvm-readelf")
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.kernels(LIB)


def test_densifying_finish_pass_is_a_kernel_of_its_own_without_scratch_or_agprs(table):
    assert NEW in table, sorted(k for k in table if "finish" in k)
    for k in ("raster_finish_adam_kernel<true>", "raster_finish_adam_kernel<false>"):
        assert k in table, k
    for k in (NEW, "raster_finish_adam_kernel<false>"):
        v = table[k]
        print(f"{k:36s} vgprs {v['vgprs']:3d} agprs {v['agprs']} sgprs {v['sgprs']:3d} scratch {v['scratch_bytes']} lds {v['lds_bytes']} waves/SIMD {v['waves_per_simd']}")
    v = table[NEW]
    assert v["scratch_bytes"] == 0 and v["agprs"] == 0, v
    assert v["lds_bytes"] == table["raster_finish_adam_kernel<false>"]["lds_bytes"], v     # the same wave-private row hand-over, nothing else
    assert v["waves_per_simd"] >= 4, v
