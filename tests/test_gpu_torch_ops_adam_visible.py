"""lfs::adam_step_multi_visible of the libtorch layer (csrc/torch_ops.cpp) through its pybind module: the same bits as ops.adam_step_multi_visible (both call
lfs_adam_step_multi_visible), the version counters of the updated tensors bumped, and c10::Error for what the wrapper refuses."""
import math

import pytest
import torch

DEV = "cuda:0"
BC = (1 / (1 - 0.9 ** 5), 1 / math.sqrt(1 - 0.999 ** 5))


def _mod():
    import lichtfeld_studio_amd  # noqa: F401
    try:
        from lichtfeld_studio_amd import _lfs_torch_ops as m
    except ImportError:
        pytest.skip("_lfs_torch_ops.so not built (python lichtfeld-studio_amd/build.py --torch-ops)")
    return m


def test_module_has_the_entry_and_refuses_cpu_tensors():
    m = _mod()
    assert hasattr(m, "adam_step_multi_visible")
    x = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        m.adam_step_multi_visible([x], [x.clone()], [x.clone()], [x.clone()], [[1e-3, 0.9, 0.999, 1e-15, *BC]], torch.zeros(1, dtype=torch.int32), 4)


@pytest.mark.gpu
def test_wrapper_equals_the_python_mirror(lfs):
    m = _mod()
    from lichtfeld_studio_amd import ops
    N = 1000
    g = torch.Generator().manual_seed(3)
    shapes = [(N, 3), (N, 15, 3), (N,)]
    mk = lambda s=1.0: [(torch.randn(sh, generator=g) * s).to(DEV) for sh in shapes]
    p, mo, v, gr = mk(), [x.abs() for x in mk(0.1)], [x.abs() for x in mk(0.01)], mk()
    p2, m2, v2 = [[x.clone() for x in row] for row in (p, mo, v)]
    bits = torch.randint(-2 ** 31, 2 ** 31 - 1, ((N + 31) // 32,), generator=g, dtype=torch.int64).to(torch.int32).to(DEV)
    bits[-1] &= (1 << (N % 32)) - 1
    sc = [[1e-3 * (i + 1), 0.9, 0.999, 1e-15, *BC] for i in range(3)]
    versions = [x._version for x in p + mo + v]
    m.adam_step_multi_visible(p, mo, v, gr, sc, bits, N)
    ops.adam_step_multi_visible([(p2[i], m2[i], v2[i], gr[i], *sc[i]) for i in range(3)], bits, N)
    for a, b in zip(p + mo + v, p2 + m2 + v2):
        assert torch.equal(a, b)
    assert all(x._version > old for x, old in zip(p + mo + v, versions))
    with pytest.raises(RuntimeError, match="leading dimension"):
        m.adam_step_multi_visible(p, mo, v, gr, sc, bits, N + 1)
    with pytest.raises(RuntimeError, match="int32"):
        m.adam_step_multi_visible(p, mo, v, gr, sc, bits.to(torch.int64), N)
