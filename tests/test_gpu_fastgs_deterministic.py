"""GPU: the deterministic accumulation mode of the fastgs blend backward (lfs_set_debug_flags bit 4; fg_blend_bwd_kernel<1> / <2> + fg_det_resolve_kernel in
csrc/fastgs_blend.hip). With the bit set two backward calls on the same forward give the same bits in all six gradients - which the float-atomic default does
not - and those gradients are the default's up to the default's own run-to-run noise. The int64 accumulator rows live in the primitive workspace, which grows
with the bit; a backward that is handed a workspace sized without it refuses before it launches anything."""
import pytest
import torch

from gpu_util import atomic_noise_bar, n, noise_check, rel_l2
from test_gpu_fastgs_w2c import _State
from test_oracle_fastgs import _scene

pytestmark = pytest.mark.gpu
NAMES = ["means", "scales_raw", "rotations_raw", "opacities_raw", "sh0", "sh_rest"]
# one wavefront's worth, a ragged image with several tiles and thousands of instances per Gaussian row, and degree 1 (the colour slots feed the SH backward)
CASES = [dict(N=1, W=80, H=64, seed=4, deg=0), dict(N=65, W=80, H=64, seed=3, deg=0), dict(N=2000, W=203, H=117, seed=1, deg=1)]


@pytest.mark.parametrize("cfg", CASES, ids=lambda c: f"N{c['N']}")
def test_two_backwards_give_the_same_bits_and_the_float_atomic_sums_within_their_noise(lfs, cfg):
    lib = lfs.load_library()
    sc = _scene(**cfg)
    draws = [_State(sc).backward() for _ in range(3)]          # default mode: three draws of the float-atomic sums (their spread sets the bar below)
    lib.lfs_set_debug_flags(16)
    try:
        st = _State(sc)                                          # (the forward sizes the workspace: with the bit set)
        a, b = st.backward(), st.backward()
        c = _State(sc).backward()                                # ... and a second forward of the same scene
        torch.cuda.synchronize()
    finally:
        lib.lfs_set_debug_flags(0)
    touched = 0
    for k, name in enumerate(NAMES):
        if a[k] is None or a[k].numel() == 0:
            continue
        assert torch.isfinite(a[k]).all(), name
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), name
        touched += int(bool((a[k] != 0).any()))
        if float(draws[0][k].abs().max()) > 0:
            noise_check(f"fastgs deterministic vs float atomics, N={cfg['N']}, {name}", rel_l2(n(a[k]), n(draws[0][k])), atomic_noise_bar(*[d[k] for d in draws]))
    assert touched >= 5


def test_a_workspace_sized_without_the_bit_is_refused(lfs):
    from lichtfeld_studio_amd.capi import LfsError
    lib = lfs.load_library()
    st = _State(_scene(N=65, W=80, H=64, seed=3, deg=0))        # forward without the bit
    small = int(st.pws.numel())
    lib.lfs_set_debug_flags(16)
    try:
        assert lib.lfs_fastgs_primitive_workspace_bytes(65, 80, 64) >= small + 65 * 16 * 8
        with pytest.raises(LfsError):
            st.backward()
    finally:
        lib.lfs_set_debug_flags(0)
    assert lib.lfs_fastgs_primitive_workspace_bytes(65, 80, 64) == small
    g = st.backward()                                           # the default mode still takes it
    torch.cuda.synchronize()
    assert torch.isfinite(g[0]).all()
