"""Static check of the scene-transform kernels (no GPU; tools/kernel_resources.py on the shipped code object): every form exists under its own name, none has scratch
or AGPRs, the SH kernel's LDS tile is the 24 KB the host code sizes its tiles by (six blocks per CU), and the register counts leave the streaming pass the occupancy
it was measured with."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "lichtfeld-studio_amd", "liblfs_gsplat.so")
SH = [f"st::st_sh_kernel<{deg}, {vec}>" for deg in range(5) for vec in ("false", "true")]


@pytest.fixture(scope="module")
def table():
    if not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("library not built / no llvm-readelf")
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.kernels(LIB)


def test_every_form_exists_without_scratch_or_agprs(table):
    for k in SH + ["st::st_geom_kernel"]:
        assert k in table, k
        print(k, table[k])
        assert table[k]["scratch_bytes"] == 0 and table[k]["agprs"] == 0, (k, table[k])
    assert len([k for k in table if k.startswith("st::")]) == len(SH) + 1


def test_lds_tile_and_occupancy(table):
    for k in SH:
        assert table[k]["lds_bytes"] == 24576 and table[k]["max_workgroup"] == 256, (k, table[k])
        # six 4-wave blocks per CU by LDS = 6 waves per SIMD. Degrees 0-3 (the measured configuration is degree 3) must stay LDS-limited; degree 4 holds two
        # 9-coefficient vectors per packed channel pair and may be register-limited one step below (20 waves per CU, each lane with four 16-byte loads in flight)
        deg = int(k.split("<")[1].split(",")[0])
        assert table[k]["waves_per_simd"] >= (6 if deg <= 3 else 5), (k, table[k])
    g = table["st::st_geom_kernel"]
    assert g["lds_bytes"] == 0 and g["waves_per_simd"] == 8, g
