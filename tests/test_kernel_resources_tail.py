"""Static check (no GPU) of every gut_tail_kernel instantiation in the shipped gfx950 code object - the fused tail of the one-call training step, with its FREEZE
(shN frozen) and NOISE (MCMC noise) variants: no scratch, no AGPRs, and no fewer wavefronts per SIMD than the instantiation the MSE benchmark step runs
(gut_tail_kernel<16, true>, i.e. <LPG 16, NEXT, no FREEZE, no NOISE>). Read from the AMDGPU metadata of lichtfeld-studio_amd/liblfs_gsplat.so (tools/kernel_resources.py)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "lichtfeld-studio_amd", "liblfs_gsplat.so")
SHIPPED = "gut_tail_kernel<16, true, false, false>"


@pytest.fixture(scope="module")
def tails():
    if not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("library not built / no llvm-readelf")
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return {k: v for k, v in mod.kernels(LIB).items() if k.startswith("gut_tail_kernel<")}


def test_every_variant_is_instantiated(tails):
    want = {f"gut_tail_kernel<{lpg}, {nxt}, {fr}, {nz}>" for lpg in (4, 16) for nxt in ("false", "true") for fr in ("false", "true") for nz in ("false", "true")}
    assert set(tails) == want, sorted(set(tails) ^ want)


def test_no_variant_spills_or_falls_below_the_shipped_occupancy(tails):
    assert SHIPPED in tails, sorted(tails)
    floor = tails[SHIPPED]["waves_per_simd"]
    assert floor >= 2
    for k, v in sorted(tails.items()):
        print(k, v)
        assert v["scratch_bytes"] == 0 and v["agprs"] == 0, (k, v)
        assert v["waves_per_simd"] >= floor, (k, v, floor)
        assert v["vgprs"] <= 256 and v["lds_bytes"] <= 64 * 1024, (k, v)
