"""CPU: the host side of the 3D smoothing filter (lichtfeld-studio_amd/filter3d.py) - `bake` against the float64 model, a baked model through save_ply / load_ply,
the packed camera layout and the trainer's recompute schedule as pure host logic. No kernel runs."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import fastgs_filter3d_reference as ref
from test_oracle_fastgs import _scene


def _inputs(N=500, seed=3):
    sc = _scene(N=N, seed=seed)
    v = ref.filter_var64(sc["means"], [ref.camera_of_scene(sc)]).astype(np.float32)
    v[::7] = 0.0                                                          # rows without a filter
    return sc, v


def test_bake_matches_the_float64_model(lfs):
    from lichtfeld_studio_amd import filter3d
    sc, v = _inputs()
    rs, ro = torch.tensor(sc["scales_raw"], dtype=torch.float32), torch.tensor(sc["opac_raw"], dtype=torch.float32).reshape(-1, 1)
    bs, bo = filter3d.bake((rs, ro), torch.tensor(v))
    ls, kappa, u, o, logit = ref.effective64(sc["scales_raw"], sc["opac_raw"], v)
    assert bs.dtype == torch.float32 and bs.shape == rs.shape and bo.shape == ro.shape
    # float32 results of float64 arithmetic: within one rounding of the model (2^-24 relative), plus the model's own few float64 ulps
    assert np.abs(bs.numpy().astype(np.float64) - ls).max() <= 2.0 ** -24 * np.abs(ls).max() + 1e-12
    assert np.abs(bo.numpy().astype(np.float64).reshape(-1) - logit).max() <= 2.0 ** -24 * np.abs(logit).max() + 1e-12
    assert (kappa < 0.9).mean() > 0.1 and np.abs(bs.numpy() - sc["scales_raw"]).max() > 1e-2
    zero = v == 0
    assert zero.any() and torch.equal(bs[zero], rs[zero]) and torch.equal(bo[zero], ro[zero])      # v = 0 rows: the raw values themselves
    # the round trip through the activations: exp(2 bs) = exp(2 rs) + v and sigmoid(bo) = sigmoid(ro) kappa
    assert np.allclose(np.exp(2 * bs.numpy().astype(np.float64)), np.exp(2 * rs.numpy().astype(np.float64)) + v[:, None], rtol=1e-6)
    assert np.allclose(1 / (1 + np.exp(-bo.numpy().astype(np.float64).reshape(-1))), o, rtol=1e-6)
    # extremes: nothing overflows, a scale far below the filter takes the opacity to zero without a NaN
    xs, xo = filter3d.bake((torch.tensor([[40.0, 0.0, -40.0], [50.0, 50.0, 50.0]]), torch.tensor([[2.0], [-3.0]])), torch.tensor([1e-3, 1e-3]))
    assert bool(torch.isfinite(xs).all()) and float(xs[0, 0]) == 40.0 and abs(float(xs[0, 2]) - 0.5 * np.log(1e-3)) < 1e-5
    assert not bool(torch.isnan(xo).any()) and float(xo[0]) < -30 and abs(float(xo[1]) + 3.0) < 1e-6
    with pytest.raises(filter3d.LfsError):
        filter3d.bake((rs, ro), torch.tensor(v[:-1]))


def test_a_baked_ply_loads_as_the_baked_model(lfs, tmp_path):
    from lichtfeld_studio_amd import filter3d, loader
    from lichtfeld_studio_amd.rasterizer import SplatModel
    sc, v = _inputs(N=200)
    f = lambda k, shape=None: torch.tensor(sc[k], dtype=torch.float32).reshape(shape) if shape else torch.tensor(sc[k], dtype=torch.float32)
    model = SplatModel(f("means"), f("sh0"), f("sh_rest"), f("scales_raw"), f("rot_raw"), f("opac_raw", (-1, 1)), 3)
    bs, bo = filter3d.bake(model, torch.tensor(v))
    path = str(tmp_path / "baked.ply")
    loader.save_ply(SplatModel(model.means, model.sh0, model.shN, bs, model.raw_quats, bo, 3), path)
    back = loader.load_ply(path, device="cpu")
    assert torch.equal(back.raw_scales, bs) and torch.equal(back.raw_opacities.reshape(-1), bo.reshape(-1)) and torch.equal(back.means, model.means)
    assert not torch.equal(back.raw_scales, model.raw_scales)


def test_pack_cameras_layout(lfs):
    from lichtfeld_studio_amd import filter3d
    from lichtfeld_studio_amd.capi import Filter3dCamera
    assert C.sizeof(Filter3dCamera) == 4 * filter3d.CAMERA_DWORDS == 72
    vm = torch.arange(32, dtype=torch.float32).reshape(2, 4, 4)
    Ks = torch.tensor([[[60.0, 0, 31.5], [0, 66.0, 24.5], [0, 0, 1]], [[75.0, 0, 36.0], [0, 82.5, 24.0], [0, 0, 1]]])
    p = filter3d.pack_cameras(viewmats=vm, Ks=Ks, width=[64, 72], height=48)
    assert p.dtype == torch.int32 and p.shape == (2, 18) and p.is_contiguous()
    cams = (Filter3dCamera * 2).from_buffer_copy(p.numpy().tobytes())
    for c in range(2):
        assert list(cams[c].w2c) == [float(16 * c + k) for k in range(12)]
        assert (cams[c].fx, cams[c].fy, cams[c].cx, cams[c].cy) == tuple(float(x) for x in (Ks[c, 0, 0], Ks[c, 1, 1], Ks[c, 0, 2], Ks[c, 1, 2]))
        assert (cams[c].width, cams[c].height) == ((64, 72)[c], 48)
    assert filter3d.pack_cameras([]).shape == (0, 18)


def test_recompute_schedule():
    """before the first step; the step after one that changed the model; otherwise every `every` steps counted from the last computation"""
    import lichtfeld_studio_amd  # noqa: F401
    from lichtfeld_studio_amd.filter3d import Filter3dSchedule

    def run(every, changed_at, steps):
        s, computed = Filter3dSchedule(every), []
        for it in range(1, steps + 1):
            if s.due():
                s.computed()
                computed.append(it)
            s.step_done(model_changed=it in changed_at)
        return computed

    assert run(4, (), 13) == [1, 5, 9, 13]
    assert run(100, (), 50) == [1]
    assert run(100, (6, 20), 30) == [1, 7, 21]
    assert run(4, (6,), 16) == [1, 5, 7, 11, 15]                          # the count restarts at the recomputation a change forced
    assert run(1, (), 4) == [1, 2, 3, 4]
    with pytest.raises(ValueError):
        Filter3dSchedule(0)
