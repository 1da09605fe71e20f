"""GPU: every form of the spherical-harmonics kernels (csrc/sh.hip, csrc/lfs_sh.cuh) against the float64 model of tests/sh_reference.py, band by band, through the
C entries (ctypes: outputs are pre-filled with NaN or a known pattern and followed by guard rows). The cases, the bounds and the assertions are those of
tests/test_emulated_sh_forms.py - the same check functions, here on device memory and the product library:
  (a) lfs_spherical_harmonics_fwd / _bwd over the whole (degree, K) table, masks given or NULL, v_dirs wanted or not;
  (b) lfs_sh_model_fwd / _bwd, accumulate off (into NaN) and on (into a pattern), v_means added to a pattern;
  (c) lfs_sh_model_bwd_adam = (b) + lfs_adam_step on shN, bit for bit, two chained steps;
  (d) lfs_sh_model_bwd_adam_all: accumulator rows with NaN around dL/dcolour, the float4 load and its three-dword fallback, v_dirs written, Adam on sh0 and shN;
  (e) lfs_sh_model_fwd_views / _bwd_views against the model summed over the views: view strides, accumulate, v_shN = NULL, inline Adam, radii = colors = NULL;
  (f) n = 1, 63, 64, 65, 129 for one case of each lane-group class, in forms (a), (b) and (e).
Each case is a few launches over at most 333 Gaussians."""
import ctypes as C

import numpy as np
import pytest
import torch

import sh_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_TORCH = {np.dtype(np.float32): torch.float32, np.dtype(np.int32): torch.int32, np.dtype(np.uint8): torch.uint8}


class DeviceBackend:
    """device memory behind sh_reference.Backend: a handle is a torch tensor viewing a byte buffer at the wanted alignment"""
    def __init__(self, lib, stream):
        self.lib, self.stream = lib, stream

    def raw(self, nbytes):
        return torch.zeros(nbytes, dtype=torch.uint8, device=DEV)

    def addr(self, h):
        return h.data_ptr()

    def view(self, raw, start, arr):
        v = raw[start:start + arr.nbytes].view(_TORCH[arr.dtype]).reshape(arr.shape)
        v.copy_(torch.from_numpy(np.array(arr, copy=True)))
        return v

    def ptr(self, h):
        return None if h is None else C.c_void_p(h.data_ptr())

    def host(self, h):
        return h.cpu().numpy()


@pytest.fixture
def B(lfs):
    from lichtfeld_studio_amd.capi import load_library, stream
    return R.Backend(DeviceBackend(load_library(), stream()))


@pytest.mark.parametrize("degree,K", R.TABLE + R.FWD_ONLY)
@pytest.mark.parametrize("masks,want_dirs", [(True, True), (False, True), (True, False)])
def test_op_form(B, degree, K, masks, want_dirs):
    R.check_op(B, degree, K, R.N, masks, want_dirs)


@pytest.mark.parametrize("degree,K", R.TABLE)
@pytest.mark.parametrize("all_visible", [False, True])
def test_model_form(B, degree, K, all_visible):
    R.check_model(B, degree, K, R.N, all_visible)


@pytest.mark.parametrize("degree,K", R.ADAM_TABLE)
def test_bwd_adam_is_bwd_then_adam_step(B, degree, K):
    R.check_bwd_adam(B, degree, K, 65)


@pytest.mark.parametrize("degree,K", R.ADAM_TABLE + [(3, 16)])
@pytest.mark.parametrize("n", [65, R.N])
def test_bwd_adam_all(B, degree, K, n):
    R.check_bwd_adam_all(B, degree, K, n)


@pytest.mark.parametrize("degree,K", R.VIEWS_TABLE)
@pytest.mark.parametrize("V,pad", [(1, 0), (1, 7), (3, 0), (3, 7)])
def test_views(B, degree, K, V, pad):
    R.check_views(B, degree, K, V, pad)


def test_views_inline_adam(B):
    R.check_views_adam(B)


@pytest.mark.parametrize("degree,K", R.LPG_CASES)
@pytest.mark.parametrize("n", R.SIZES)
def test_size_sweep(B, degree, K, n):
    R.check_op(B, degree, K, n)
    R.check_model(B, degree, K, n)
    R.check_views(B, degree, K, 3, 7, n)
