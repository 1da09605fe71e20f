"""Static check of the background-compose kernels (no GPU; tools/kernel_resources.py on the shipped code object): both kernels exist in both forms under their own
names, none has scratch, AGPRs or LDS, and the register counts allow 8 waves per SIMD - the bar st_geom_kernel is held to."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "lichtfeld-studio_amd", "liblfs_gsplat.so")
FORMS = [f"bgc::{k}<{vec}>" for k in ("compose_kernel", "compose_bwd_kernel") for vec in ("false", "true")]


@pytest.fixture(scope="module")
def table():
    if not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("library not built / no llvm-readelf")
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.kernels(LIB)


def test_every_form_exists_without_scratch_agprs_or_lds(table):
    for k in FORMS:
        assert k in table, k
        print(k, table[k])
        assert table[k]["scratch_bytes"] == 0 and table[k]["agprs"] == 0 and table[k]["lds_bytes"] == 0, (k, table[k])
        assert table[k]["max_workgroup"] == 256, (k, table[k])
    assert len([k for k in table if k.startswith("bgc::")]) == len(FORMS)


def test_eight_waves_per_simd(table):
    for k in FORMS:
        assert table[k]["waves_per_simd"] == 8, (k, table[k])
