"""CPU: the SOG container (lichtfeld_studio_amd/sog.py write_sog / read_sog) on the emulated library - bundle contents, meta.json, image sizes, and the round
trip against a decode written here from the format description (tests/sog_reference.py), not from the product's reader."""
import json
import os
import sys
import zipfile

import numpy as np
import pytest
import torch

pytest.importorskip("PIL")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import emul_util  # noqa: E402
import sog_reference as ref  # noqa: E402

SQRT2 = 1.41421356237


@pytest.fixture(scope="module", autouse=True)
def _emulated_library():
    if not emul_util.available():
        pytest.skip("no clang++ to build the emulated library")
    import lichtfeld_studio_amd.sog  # noqa: F401  (before installed(): its loader hooks get patched with the others)
    with emul_util.installed():
        yield


def _model(N, degree, seed):
    from lichtfeld_studio_amd.rasterizer import SplatModel
    rng = np.random.default_rng(seed)
    coeffs = (degree + 1) ** 2 - 1
    means = (rng.standard_normal((N, 3)) * np.array([5.0, 1.0, 20.0])).astype(np.float32)
    sh0 = rng.standard_normal((N, 1, 3)).astype(np.float32)
    # channel c of every higher-order coefficient sits around 10 (c + 1), coefficient j adds 0.3 j, eight groups of Gaussians differ by 0.05 g:
    # a writer or reader that swaps (j, c) puts values of the wrong colour into a channel
    group = rng.integers(0, 8, N)
    shN = (10.0 * (np.arange(3)[None, None, :] + 1) + 0.3 * np.arange(coeffs)[None, :, None] + 0.05 * group[:, None, None]
           + 0.002 * rng.standard_normal((N, coeffs, 3))).astype(np.float32)
    scales = (rng.standard_normal((N, 3)) - 3.0).astype(np.float32)
    quats = rng.standard_normal((N, 4)).astype(np.float32)
    quats[0] = 0.0                                         # becomes the identity
    quats[1] = [0.0, 0.0, -2.0, 0.0]                       # largest component negative: the sign flips
    opac = (2.0 * rng.standard_normal(N)).astype(np.float32)
    t = lambda a: torch.from_numpy(a)
    return SplatModel(t(means), t(sh0), t(shN), t(scales), t(quats), t(opac), degree)


def _np(model):
    return [p.detach().numpy() for p in model.parameters()]


def _unit(q):
    q = np.asarray(q, np.float64)
    length = np.linalg.norm(q, axis=1, keepdims=True)
    return np.where(length > 0, q / np.where(length > 0, length, 1), np.array([1.0, 0, 0, 0]))


def _check_round_trip(model, path, palette_size, degree):
    from lichtfeld_studio_amd import sog
    N = model.means.shape[0]
    coeffs = (degree + 1) ** 2 - 1
    meta_written = sog.write_sog(model, path, iterations=3, palette_size=palette_size)
    meta, images, names = ref.open_bundle(path)
    assert meta == json.loads(json.dumps(meta_written))
    expected = ["means_l.webp", "means_u.webp", "quats.webp", "scales.webp", "sh0.webp"] + (["shN_centroids.webp", "shN_labels.webp"] if degree else []) + ["meta.json"]
    assert sorted(names) == sorted(expected)
    width, height = ref.texture_size(N)
    assert (meta["version"], meta["count"], meta["width"], meta["height"]) == (2, N, width, height)
    assert width % 4 == 0 and height % 4 == 0 and width * height >= N and width == int(np.ceil(np.sqrt(N) / 4)) * 4
    for nme in ("means_l.webp", "means_u.webp", "quats.webp", "scales.webp", "sh0.webp"):
        assert images[nme].shape == (height, width, 4), nme
    assert meta["means"]["files"] == ["means_l.webp", "means_u.webp"] and meta["scales"]["files"] == ["scales.webp"]
    assert meta["quats"]["files"] == ["quats.webp"] and meta["sh0"]["files"] == ["sh0.webp"]
    assert len(meta["means"]["mins"]) == 3 and len(meta["means"]["maxs"]) == 3
    assert 1 <= len(meta["scales"]["codebook"]) <= 256 and 1 <= len(meta["sh0"]["codebook"]) <= 256

    means, sh0, shN, scales, quats, opac = _np(model)
    order = np.argsort(ref.morton_codes(means), kind="stable")            # pixel i holds Gaussian order[i]
    back = sog.read_sog(path, device="cpu")
    r_means, r_sh0, r_shN, r_scales, r_quats, r_opac = _np(back)
    assert back.max_sh_degree == degree and r_means.shape == (N, 3) and r_shN.shape == (N, coeffs, 3)
    px = lambda nme: images[nme].reshape(-1, 4)[:N]

    # means: log space, one 16-bit step per axis
    mlog = ref.log_transform(means)
    mins, maxs = np.array(meta["means"]["mins"]), np.array(meta["means"]["maxs"])
    np.testing.assert_allclose(mins, mlog.min(0), atol=1e-6)
    np.testing.assert_allclose(maxs, mlog.max(0), atol=1e-6)
    q16 = px("means_l.webp")[:, :3].astype(np.int64) | (px("means_u.webp")[:, :3].astype(np.int64) << 8)
    dlog = q16 / 65535.0 * (maxs - mins) + mins
    assert (np.abs(dlog - mlog[order]) <= (maxs - mins) / 65535 + 1e-6).all()
    np.testing.assert_allclose(r_means, np.sign(dlog) * (np.exp(np.abs(dlog)) - 1), rtol=1e-5, atol=1e-6)
    assert (px("means_l.webp")[:, 3] == 255).all() and (px("means_u.webp")[:, 3] == 255).all()

    # quaternions, up to sign: the three STORED components within sqrt(2) / 255 plus f32 rounding (all four: test_quaternion_round_trip_every_component below);
    # the stored bytes are the truncated value or the next one up
    q, r = _unit(quats[order]), r_quats.astype(np.float64)
    r = r * np.where(np.abs(r - q).max(1) <= np.abs(r + q).max(1), 1.0, -1.0)[:, None]
    stored = np.ones((N, 4), bool)
    stored[np.arange(N), np.abs(q).argmax(1)] = False
    assert (np.abs(r - q)[stored] <= SQRT2 / 255 + 1e-6).all(), np.abs(r - q)[stored].max()
    qb = px("quats.webp")[:, :3].astype(np.int64)
    others = np.array([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]])[np.abs(q).argmax(1)]
    flipped = q * np.sign(q[np.arange(N), np.abs(q).argmax(1)])[:, None]
    exact = (np.take_along_axis(flipped, others, 1) * SQRT2 * 0.5 + 0.5) * 255
    assert ((qb >= np.floor(exact - 1e-3)) & (qb <= np.floor(exact + 1e-3) + 1)).all()
    qa = px("quats.webp")[:, 3]
    np.testing.assert_array_equal(qa, 252 + np.abs(q).argmax(1))
    assert (r_quats[np.arange(N), qa.astype(np.int64) - 252] > 0).all()

    # raw scales and sh0: exactly the codebook entry of the stored label
    np.testing.assert_array_equal(r_scales, np.array(meta["scales"]["codebook"], np.float32)[px("scales.webp")[:, :3]])
    np.testing.assert_array_equal(r_sh0.reshape(N, 3), np.array(meta["sh0"]["codebook"], np.float32)[px("sh0.webp")[:, :3]])
    assert (np.diff(meta["scales"]["codebook"]) >= 0).all() and (np.diff(meta["sh0"]["codebook"]) >= 0).all()
    assert np.abs(r_scales - scales[order]).mean() < 0.05 and np.abs(r_sh0.reshape(N, 3) - sh0.reshape(N, 3)[order]).mean() < 0.05   # (a 256-entry codebook over ~6 units)
    assert (px("scales.webp")[:, 3] == 255).all()

    # opacity
    sig = 1 / (1 + np.exp(-opac[order].astype(np.float64)))
    stored = px("sh0.webp")[:, 3] / 255.0
    assert (stored <= sig + 1e-6).all() and (sig - stored <= 1 / 255 + 1e-6).all()          # truncated, never rounded up
    assert (np.abs(1 / (1 + np.exp(-r_opac.astype(np.float64))) - sig) <= 1 / 255 + 1e-6).all()

    if not degree:
        assert "shN" not in meta
        return meta
    sm = meta["shN"]
    palette = sm["palette_size"]
    assert (sm["bands"], sm["coeffs"]) == (degree, coeffs) and sm["files"] == ["shN_centroids.webp", "shN_labels.webp"] and 1 <= len(sm["codebook"]) <= 256
    assert images["shN_centroids.webp"].shape == (-(-palette // 64), 64 * coeffs, 4) and images["shN_labels.webp"].shape == (height, width, 4)
    lab = px("shN_labels.webp")
    labels = lab[:, 0].astype(np.int64) | (lab[:, 1].astype(np.int64) << 8)
    assert labels.max() < palette and (lab[:, 2] == 0).all() and (lab[:, 3] == 255).all()
    cpx = images["shN_centroids.webp"].reshape(-1, 4)
    cb = np.array(sm["codebook"], np.float32)
    centroids = cb[cpx[:palette * coeffs, :3]].reshape(palette, coeffs, 3)   # pixel i * coeffs + j, channel c -> coefficient j of colour c of centroid i
    np.testing.assert_array_equal(r_shN, centroids[labels])
    return meta, r_shN, shN[order]


def test_bundle_round_trip_at_sh_degree_3(tmp_path):
    meta, r_shN, shN = _check_round_trip(_model(500, 3, 1), str(tmp_path / "splat.sog"), 128, 3)
    assert meta["shN"]["palette_size"] == 128                                  # an explicit palette size is honoured
    # (j, c) in the right places: colour c sits around 10 (c + 1) + 0.3 j; palette and codebook cost a few hundredths
    assert np.abs(r_shN - shN).max() < 0.25, np.abs(r_shN - shN).max()
    for c in range(3):
        assert abs(r_shN[:, :, c].mean() - (10 * (c + 1) + 0.3 * 7 + 0.05 * 3.5)) < 0.1


def test_bundle_round_trip_at_sh_degree_0_with_fewer_values_than_codebook_entries(tmp_path):
    from lichtfeld_studio_amd import sog
    model = _model(40, 0, 2)
    meta = _check_round_trip(model, str(tmp_path / "small.sog"), None, 0)
    assert len(meta["scales"]["codebook"]) == 120                              # 3 N <= 256 values: each is its own entry and decodes exactly
    back = sog.read_sog(str(tmp_path / "small.sog"), device="cpu")
    order = np.argsort(ref.morton_codes(model.means.numpy()), kind="stable")
    np.testing.assert_array_equal(back.raw_scales.detach().numpy(), model.raw_scales.numpy()[order])
    np.testing.assert_array_equal(back.sh0.detach().numpy(), model.sh0.numpy()[order])


@pytest.mark.parametrize("N,seed", [(500, 1), (40, 2)])
def test_quaternion_round_trip_every_component(tmp_path, N, seed):
    """Every component of the decoded quaternion within sqrt(2) / 255 plus rounding of the original, compared up to sign - the reconstructed fourth component
    included. Plain truncation of the three stored bytes (the reference's encoder) does not give that: the fourth component, sqrt(1 - v0^2 - v1^2 - v2^2) in the
    decoder, collects the three one-sided truncation errors (measured with truncation on these models: 0.01112, 34 of 500 above the bound; 0.00628, 1 of 40).
    sog._pack_quats therefore picks each byte from {truncated, truncated + 1} by the decoded error; the decode here is the product's reader, which follows the
    reference reader's arithmetic."""
    from lichtfeld_studio_amd import sog
    model = _model(N, 0, seed)
    sog.write_sog(model, str(tmp_path / "q.sog"), iterations=1)
    order = np.argsort(ref.morton_codes(model.means.numpy()), kind="stable")
    q, r = _unit(model.raw_quats.numpy()[order]), sog.read_sog(str(tmp_path / "q.sog"), device="cpu").raw_quats.detach().numpy().astype(np.float64)
    err = np.minimum(np.abs(r - q).max(1), np.abs(r + q).max(1))
    print(f"quaternion round trip N = {N}: max component error {err.max():.5f} against sqrt(2) / 255 = {SQRT2 / 255:.5f}; above: {(err > SQRT2 / 255 + 1e-6).sum()} of {N}")
    assert (err <= SQRT2 / 255 + 1e-6).all(), err.max()


def test_default_palette_size_reproduces_the_reference_expression(tmp_path):
    from lichtfeld_studio_amd import sog
    assert sog.default_palette_size(2000) == 64 and sog.default_palette_size(1024) == 64 and sog.default_palette_size(1023) == 1 and sog.default_palette_size(500) == 1
    assert sog.default_palette_size(3_000_000) == 64
    meta = sog.write_sog(_model(500, 3, 3), str(tmp_path / "a.sog"), iterations=1)
    assert meta["shN"]["palette_size"] == 1
    meta = sog.write_sog(_model(2000, 1, 4), str(tmp_path / "b.sog"), iterations=1)
    assert meta["shN"]["palette_size"] == 64 and (meta["shN"]["bands"], meta["shN"]["coeffs"]) == (1, 3)
    assert ref.open_bundle(str(tmp_path / "b.sog"))[1]["shN_centroids.webp"].shape == (1, 64 * 3, 4)
    from lichtfeld_studio_amd.capi import LfsError
    with pytest.raises(LfsError):
        sog.write_sog(_model(40, 1, 5), str(tmp_path / "c.sog"), palette_size=41)


def test_loose_files_hold_the_same_images(tmp_path):
    from PIL import Image
    from lichtfeld_studio_amd import loader, sog
    model = _model(500, 3, 1)
    loader.save_sog(model, str(tmp_path / "bundle.sog"), iterations=2, palette_size=32)
    os.makedirs(tmp_path / "loose")
    loader.save_sog(model, str(tmp_path / "loose" / "meta.json"), iterations=2, palette_size=32)
    meta, images, names = ref.open_bundle(str(tmp_path / "bundle.sog"))
    assert sorted(os.listdir(tmp_path / "loose")) == sorted(names)
    assert json.load(open(tmp_path / "loose" / "meta.json")) == meta
    for nme, img in images.items():
        with Image.open(tmp_path / "loose" / nme) as im:
            np.testing.assert_array_equal(np.asarray(im.convert("RGBA")), img)
    a, b = loader.load_sog(str(tmp_path / "bundle.sog"), device="cpu"), loader.load_sog(str(tmp_path / "loose" / "meta.json"), device="cpu")
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.equal(p, q)
    assert zipfile.is_zipfile(tmp_path / "bundle.sog") and not zipfile.is_zipfile(tmp_path / "loose" / "meta.json")
