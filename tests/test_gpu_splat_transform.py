"""The scene transform on the MI355X (bodies: tests/splat_transform_reference.py, shared with tests/test_emulated_splat_transform.py): lfs_splat_transform_apply
against the float32 model bit for bit and the float64 model within the derived bounds at every size and SH layout, in and out of place, on 16-byte- and
4-byte-aligned buffers with NaN guards; round trips; skipped pairs; transform_model and crop; render invariance through BOTH rasterizers (fastgs and 3DGUT), with the
reference's behaviour (shN left alone) shown to fail it; lfs::splat_transform through the pybind module; one round trip of tools/transform_splat.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import splat_transform_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_kernel_sizes_layouts_in_place_alignment(lfs):
    ref.check_kernel_sizes(DEV)


def test_other_transforms(lfs):
    ref.check_transforms(DEV)


def test_round_trip(lfs):
    ref.check_round_trip(DEV)


def test_skipped_pairs(lfs):
    ref.check_skipped_pairs(DEV)


def test_transform_model(lfs):
    ref.check_transform_model(DEV)


def test_crop(lfs):
    ref.check_crop(DEV)


def test_render_invariance_fastgs(lfs):
    ref.check_render_invariance(DEV, "fastgs")


def test_render_invariance_3dgut(lfs):
    ref.check_render_invariance(DEV, "gut")


def test_one_million_rows_in_place(lfs):
    """one launch at the size of a real scene (grid > 2^13 blocks, offsets past 2^27 bytes): bit-equality with the float32 model on a sample of rows, in place"""
    import torch
    from lichtfeld_studio_amd import transform
    N = 1_000_003
    g = torch.Generator(device=DEV); g.manual_seed(5)
    shN = torch.rand((N, 15, 3), device=DEV, generator=g) * 4 - 2
    means, quats, scales = torch.randn((N, 3), device=DEV, generator=g) * 100, torch.randn((N, 4), device=DEV, generator=g), torch.randn((N, 3), device=DEV, generator=g)
    rows = torch.cat([torch.arange(0, 300), torch.arange(N // 2 - 150, N // 2 + 150), torch.arange(N - 300, N)]).to(DEV)
    before = [t[rows].cpu().numpy() for t in (means, quats, scales, shN)]
    xf = transform.similarity(ref.GENERIC)
    transform.apply(xf, 3, means, quats, scales, shN, out="inplace")
    want = ref.model32(xf.record(3), *before)
    for t, w in zip((means, quats, scales, shN), want):
        assert np.array_equal(ref.bits(t[rows].cpu().numpy()), ref.bits(w))
    assert bool(torch.isfinite(shN).all()) and bool(torch.isfinite(means).all())


def test_libtorch_wrapper_equals_transform_model(lfs):
    import torch
    try:
        from lichtfeld_studio_amd import _lfs_torch_ops as m
    except ImportError:
        pytest.skip("_lfs_torch_ops.so not built (python lichtfeld-studio_amd/build.py --torch-ops)")
    from lichtfeld_studio_amd import transform
    from lichtfeld_studio_amd.rasterizer import SplatModel
    xf = transform.similarity(ref.GENERIC)
    matrix = [float(v) for v in ref.GENERIC.reshape(-1)]
    for deg, rows in ((3, 15), (4, 24), (0, 0), (2, 10)):
        a = [torch.from_numpy(x).to(DEV) for x in ref.inputs(257, rows, 40 + deg)]
        model = SplatModel(a[0], torch.zeros((257, 1, 3), device=DEV), a[3], a[2], a[1], torch.zeros((257, 1), device=DEV), deg)
        want = transform.transform_model(model, xf)
        got = m.splat_transform(a[0], a[1], a[2], a[3], matrix, False)
        for g, w in zip(got, (want.means, want.raw_quats, want.raw_scales, want.shN)):
            assert g.shape == w.shape and np.array_equal(ref.bits(g.cpu().numpy()), ref.bits(w.cpu().numpy()))
        assert all(g.data_ptr() != x.data_ptr() or x.numel() == 0 for g, x in zip(got, a))
        same = m.splat_transform(a[0], a[1], a[2], a[3], matrix, True)                  # in place: the same tensors, overwritten
        for g, x, w in zip(same, a, (want.means, want.raw_quats, want.raw_scales, want.shN)):
            assert g.data_ptr() == x.data_ptr() and np.array_equal(ref.bits(x.cpu().numpy()), ref.bits(w.cpu().numpy()))
    only = m.splat_transform(None, None, None, torch.from_numpy(ref.inputs(65, 15, 1)[3]).to(DEV), matrix, False)
    assert only[0] is None and only[1] is None and only[2] is None and only[3].shape == (65, 15, 3)
    with pytest.raises(RuntimeError):
        m.splat_transform(a[0], a[1], a[2], a[3], [float(v) for v in np.diag([1.0, 2.0, 1.0, 1.0]).reshape(-1)], False)     # non-uniform scale: refused, not averaged
    with pytest.raises(RuntimeError):
        m.splat_transform(a[0].cpu(), None, None, None, matrix, False)


def test_tool_round_trip(lfs, tmp_path):
    """tools/transform_splat.py on a 300-Gaussian PLY: out, then back with the inverse matrix - the file returns within the round-trip bounds; a crop in the output frame"""
    import torch
    from lichtfeld_studio_amd import loader, transform
    from lichtfeld_studio_amd.rasterizer import SplatModel
    means, quats, scales, shN = ref.inputs(300, 15, 50)
    means = (means / 100).astype(np.float32)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(DEV)
    rng = np.random.default_rng(1)
    model = SplatModel(t(means), t(rng.normal(size=(300, 1, 3))), t(shN), t(scales), t(quats), t(rng.normal(size=(300, 1))), 3)
    src = str(tmp_path / "in.ply")
    loader.save_ply(model, src)
    tool = os.path.join(os.path.dirname(HERE), "tools", "transform_splat.py")

    def run(*argv):
        r = subprocess.run([sys.executable, tool, *argv], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        return json.loads(r.stdout.strip().splitlines()[-1])

    a = run("--ply", src, "--out", str(tmp_path / "moved"), "--rotate", "x", "90", "--rotate", "z", "-30", "--scale", "2", "--translate", "1", "2", "3")
    assert (a["n_before"], a["n_after"]) == (300, 300) and abs(a["scale"] - 2.0) < 1e-12
    xf = transform.similarity(np.array(a["matrix"]))
    moved = loader.load_ply(a["ply"], device=DEV)
    source = loader.load_ply(src, device=DEV)                                             # (save_ply stores the NORMALISED rotation, as the reference's writer does)
    want = transform.transform_model(source, xf)
    want.raw_quats = torch.nn.functional.normalize(want.raw_quats, dim=-1)
    for g, w in zip(moved.parameters(), want.parameters()):
        assert np.array_equal(ref.bits(g.detach().cpu().numpy()), ref.bits(w.detach().cpu().numpy()))
    inv = [repr(float(v)) for v in xf.inverse().matrix.reshape(-1)]
    b = run("--ply", a["ply"], "--out", str(tmp_path / "back.ply"), "--matrix", *inv)
    back = loader.load_ply(b["ply"], device=DEV)
    a0 = [p.detach().cpu().numpy() for p in (source.means, source.raw_quats, source.raw_scales, source.shN)]
    a1 = [p.detach().cpu().numpy() for p in (moved.means, moved.raw_quats, moved.raw_scales, moved.shN)]
    bounds = ref.round_trip_bounds(xf, xf.inverse(), 3, a0, a1)
    # the two files hold unit quaternions: each normalisation rounds within 4 u (sum of four squares, root, quotient) and removes a norm that the un-normalised product
    # of two rounded unit quaternions has off 1 by at most 4 u more
    bounds[1] = bounds[1] + 12 * ref.U
    for g, w, bound in zip((back.means, back.raw_quats, back.raw_scales, back.shN), a0, bounds):
        assert (np.abs(g.detach().cpu().numpy().astype(np.float64) - w) <= bound).all()
    assert torch.equal(back.sh0, moved.sh0) and torch.equal(back.raw_opacities, moved.raw_opacities)
    x2 = want.means.detach().cpu().numpy().astype(np.float64)
    lo, hi = np.median(x2, 0) - 0.5, np.median(x2, 0) + 0.5
    keep = ((x2 >= lo) & (x2 <= hi)).all(1)
    c = run("--ply", src, "--out", str(tmp_path / "cut"), "--matrix", *[repr(float(v)) for v in xf.matrix.reshape(-1)], "--crop-min", *[repr(float(v)) for v in lo], "--crop-max",
            *[repr(float(v)) for v in hi], "--save-sog")
    assert c["n_after"] == int(keep.sum()) and 0 < c["n_after"] < 300 and os.path.getsize(c["sog"]) > 0
    r = subprocess.run([sys.executable, tool, "--ply", src, "--out", str(tmp_path / "x")], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "nothing to do" in r.stderr
