"""GPU: the SOG export operators (lichtfeld_studio_amd/sog.py over csrc/sog.hip) - Morton codes, the MFMA assignment, the 1-D assignment, the segmented-mean
update and the two Lloyd loops - against the independent numpy models of tests/sog_reference.py. Fixed seeds; every body also runs on the emulated library
(tests/test_emulated_sog.py). The reference's CUDA kernels have no CPU build here, so there are no reference goldens.

Bounds (derived, not measured):
  assignment  d2(x, c_label) - min_c d2(x, c) <= 8 (D + 2) u (|x|^2 + max_c |c|^2), u = 2^-24: each score is an f32 fmaf chain of D products on a pre-rounded
              -|c|^2 / 2, |s^ - s| <= 2 (D + 2) u (|x|^2 + |c|^2) by the standard dot-product bound; the chosen and the best score may each be off by that much,
              and d2 = |x|^2 - 2 s.
  update      |centroid - fp64 mean| <= 32 u max|x| (excludes a plain sequential f32 sum over 10^4 values)."""
import numpy as np
import pytest
import torch

import sog_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _n(x):
    return x.detach().cpu().numpy()


# ---- 1. Morton -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 63, 1000])
def test_morton_codes_are_bit_equal_to_the_model_and_the_order_is_stable(N):
    from lichtfeld_studio_amd import sog
    rng = np.random.default_rng(100 + N)
    means = rng.uniform(0.0, 1.0, (N, 3)).astype(np.float32) * np.array([1.0, 0.5, 0.25], np.float32)
    if N >= 3:
        means[0] = 0.0
        means[1] = 1.0                     # the maximum corner of a cube of edge 1: 2 097 151 on every axis
        means[2] = means[N // 2]           # equal codes: the order must fall back on the index
    codes = sog.morton_encode(_t(means))
    assert codes.dtype == torch.int64 and tuple(codes.shape) == (N,)
    expect = ref.morton_codes(means)
    np.testing.assert_array_equal(_n(codes), expect)
    if N >= 3:
        assert int(codes[1]) == -1 and int(codes[0]) == -(1 << 63)      # all 63 bits set / none, + INT64_MIN
    order = _n(sog.morton_sort_indices(codes))
    np.testing.assert_array_equal(order, np.argsort(expect, kind="stable"))


@pytest.mark.parametrize("N", [1, 63, 1000])
def test_morton_of_identical_points_takes_the_cube_clamp(N):
    from lichtfeld_studio_amd import sog
    means = np.tile(np.array([[0.3, -7.0, 11.5]], np.float32), (N, 1))
    codes = sog.morton_encode(_t(means))
    np.testing.assert_array_equal(_n(codes), ref.morton_codes(means))
    assert (_n(codes) == -(1 << 63)).all()
    np.testing.assert_array_equal(_n(sog.morton_sort_indices(codes)), np.arange(N))


# ---- 2. assignment ---------------------------------------------------------------------------------------------------
ASSIGN_SHAPES = [(1, 1, 1), (17, 3, 9), (257, 17, 24), (1000, 300, 45), (1000, 64, 45), (300, 1000, 45), (100, 20, 64)]


def _assign_inputs(N, k, D):
    rng = np.random.default_rng(1000 * N + 10 * k + D)
    data = rng.standard_normal((N, D)).astype(np.float32)
    cen = (0.7 * rng.standard_normal((k, D))).astype(np.float32)
    m = min(N, k) // 2
    cen[:m] = data[:m] + np.float32(0.05) * rng.standard_normal((m, D)).astype(np.float32)    # some centroids sit next to points, as in a running k-means
    return data, cen


@pytest.mark.parametrize("N,k,D", ASSIGN_SHAPES)
def test_assignment_is_within_the_f32_score_bound_of_the_fp64_nearest(N, k, D):
    from lichtfeld_studio_amd import sog
    data, cen = _assign_inputs(N, k, D)
    # the checker itself, on the CPU: the fp64 argmin satisfies the bound on these inputs
    exact = ref.squared_distances(data, cen).argmin(1)
    e0, b0 = ref.assignment_excess_and_bound(data, cen, exact)
    assert (e0 <= b0).all() and (b0 > 0).all()
    labels = sog.kmeans_assign(_t(data), _t(cen))
    assert labels.dtype == torch.int32 and tuple(labels.shape) == (N,)
    lab = _n(labels)
    assert lab.min() >= 0 and lab.max() < k
    excess, bound = ref.assignment_excess_and_bound(data, cen, lab)
    print(f"assign ({N},{k},{D}): max excess {excess.max():.3e}, min bound {bound.min():.3e}, labels != fp64 argmin: {(lab != exact).sum()}")
    assert (excess <= bound).all(), (excess.max(), bound.min())          # no point excluded
    again = sog.kmeans_assign(_t(data), _t(cen))
    assert torch.equal(labels, again)


@pytest.mark.parametrize("N,k,D", [(257, 17, 24), (1000, 64, 45)])
def test_assignment_gives_exact_ties_to_the_lowest_index(N, k, D):
    """every centroid row twice: rows c and c + k score bit-identically, so every label must stay below k - within a lane, between the lane groups and
    (k = 64: the copies sit in the next 64-centroid chunk) across chunks"""
    from lichtfeld_studio_amd import sog
    data, cen = _assign_inputs(N, k, D)
    labels = _n(sog.kmeans_assign(_t(data), _t(np.concatenate([cen, cen]))))
    single = _n(sog.kmeans_assign(_t(data), _t(cen)))
    assert labels.max() < k
    np.testing.assert_array_equal(labels, single)


# ---- 3. 1-D assignment -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 256])
@pytest.mark.parametrize("n", [1, 255, 5000])
def test_assignment_1d_is_the_first_strict_minimum(n, k):
    from lichtfeld_studio_amd import sog
    rng = np.random.default_rng(7 * n + k)
    # centroids on a 1/64 grid: duplicates occur by themselves at k = 256 and midpoints are exact in f32
    cen = np.sort(np.round(rng.standard_normal(k) * 64) / 64).astype(np.float32)
    if k == 2 and n == 255:
        cen[1] = cen[0]                                                   # both entries equal
    if k == 256:
        assert (np.diff(cen) == 0).any()
    mids = ((cen[:-1].astype(np.float64) + cen[1:]) / 2).astype(np.float32)
    special = np.concatenate([mids, cen, [cen[0] - 1, cen[-1] + 1, 1e6, -1e6, 3e7, -3e7, 0.0]]).astype(np.float32)   # far points: many centroids share one rounded distance
    data = rng.standard_normal(n).astype(np.float32) * 1.5
    m = min(n, special.shape[0])
    data[:m] = special[rng.permutation(special.shape[0])[:m]] if n > 1 else mids[:1]
    labels = sog.kmeans_assign_1d(_t(data), _t(cen))
    assert labels.dtype == torch.int32
    np.testing.assert_array_equal(_n(labels), ref.assign_1d(data, cen))


# ---- 4. update -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,k,D", [(1000, 300, 45), (30000, 256, 1)])
def test_update_is_the_segment_mean_keeps_empty_clusters_and_repeats_bit_for_bit(N, k, D):
    from lichtfeld_studio_amd import sog
    rng = np.random.default_rng(N + k + D)
    data = (rng.standard_normal((N, D)) + 1.0).astype(np.float32)       # a common offset: the sums grow, a sequential f32 sum would lose digits
    empty = np.array([3, k // 2, k - 1])
    allowed = np.setdiff1d(np.arange(k), empty)
    labels = allowed[rng.integers(0, allowed.shape[0], N)]
    if N >= 20000:
        labels[rng.permutation(N)[:12000]] = 7                            # one cluster of >= 10^4 points
        assert (labels == 7).sum() >= 10000
    labels = labels.astype(np.int32)
    start = rng.standard_normal((k, D)).astype(np.float32)
    mean, counts = ref.segment_means(data, labels, k)
    assert (counts[empty] == 0).all() and (counts == 0).sum() >= 3
    cen = _t(start.copy())
    sog.kmeans_update(_t(data), _t(labels), cen)
    got = _n(cen)
    filled = counts > 0
    err = np.abs(got[filled].astype(np.float64) - mean[filled]).max()
    bound = 32 * U * np.abs(data).max()
    print(f"update ({N},{k},{D}): max error {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    np.testing.assert_array_equal(got[~filled].view(np.uint32), start[~filled].view(np.uint32))
    cen2 = _t(start.copy())
    sog.kmeans_update(_t(data), _t(labels), cen2)
    assert torch.equal(cen, cen2)


# ---- 5. kmeans_1d ----------------------------------------------------------------------------------------------------
def test_kmeans_1d_returns_the_labels_of_the_centroids_before_the_last_update():
    from lichtfeld_studio_amd import sog
    rng = np.random.default_rng(5)
    data = np.concatenate([rng.standard_normal(3000), 4 + 0.3 * rng.standard_normal(2000)]).astype(np.float32)
    c2, l2 = sog.kmeans_1d(_t(data), 256, iterations=2)
    c3, l3 = sog.kmeans_1d(_t(data), 256, iterations=3)
    assert tuple(c3.shape) == (256, 1) and l3.dtype == torch.int32 and tuple(l3.shape) == (5000,)
    np.testing.assert_array_equal(_n(l3), ref.assign_1d(data, _n(c2).reshape(-1)))
    assert (np.diff(_n(c3).reshape(-1)) >= 0).all() and (np.diff(_n(c2).reshape(-1)) >= 0).all()
    # the centroid of a non-empty cluster is its mean
    mean, counts = ref.segment_means(data[:, None], _n(l3), 256)
    filled = counts > 0
    assert np.abs(_n(c3).reshape(-1)[filled] - mean[filled, 0]).max() <= 32 * U * np.abs(data).max()


def test_kmeans_1d_with_no_more_points_than_clusters_returns_the_sorted_data():
    from lichtfeld_studio_amd import sog
    data = np.random.default_rng(6).standard_normal(100).astype(np.float32)
    c, l = sog.kmeans_1d(_t(data), 256, iterations=3)
    np.testing.assert_array_equal(_n(c).reshape(-1), np.sort(data))
    np.testing.assert_array_equal(_n(l), np.arange(100, dtype=np.int32))


# ---- 6. kmeans -------------------------------------------------------------------------------------------------------
def _clustered(N, D, seed):
    rng = np.random.default_rng(seed)
    centres = 2.0 * rng.standard_normal((40, D))
    return (centres[rng.integers(0, 40, N)] + 0.5 * rng.standard_normal((N, D))).astype(np.float32)


def test_kmeans_inertia_does_not_increase():
    """labels of run i (iterations = i) are the assignment to the centroids run i - 1 returned: J(l_i, c_{i-1}) >= J(l_i, c_i) >= J(l_{i+1}, c_i)"""
    from lichtfeld_studio_amd import sog
    data = _clustered(2000, 45, 11)
    init = data[np.random.default_rng(12).permutation(2000)[:64]].copy()
    prev_c, inertias = init, []
    for i in range(1, 6):
        c, l = sog.kmeans(_t(data), 64, iterations=i, tolerance=0.0, init=_t(init))
        assert tuple(c.shape) == (64, 45) and l.dtype == torch.int32 and tuple(l.shape) == (2000,)
        inertias.append(ref.inertia(data, prev_c, _n(l)))
        prev_c = _n(c)
    print("kmeans inertia per iteration:", inertias)
    for a, b in zip(inertias, inertias[1:]):
        assert b <= a * (1 + 1e-5), inertias
    assert inertias[-1] < 0.9 * inertias[0]


@pytest.mark.parametrize("k", [64, 300])
def test_kmeans_with_the_same_generator_seed_is_bit_identical(k):
    """k = 64: k-means++; k = 300: distinct random points"""
    from lichtfeld_studio_amd import sog
    data = _t(_clustered(2000, 45, 13))
    runs = [sog.kmeans(data, k, iterations=2, generator=torch.Generator().manual_seed(7)) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    other = sog.kmeans(data, k, iterations=2, generator=torch.Generator().manual_seed(8))
    assert not torch.equal(runs[0][0], other[0])


def test_kmeans_with_no_more_points_than_clusters_returns_the_data():
    from lichtfeld_studio_amd import sog
    data = _t(_clustered(50, 45, 14))
    c, l = sog.kmeans(data, 64, iterations=3)
    assert torch.equal(c, data) and c.data_ptr() != data.data_ptr()
    np.testing.assert_array_equal(_n(l), np.arange(50, dtype=np.int32))


def test_entry_points_refuse_bad_arguments_before_any_launch():
    import ctypes as C
    from lichtfeld_studio_amd import sog
    from lichtfeld_studio_amd.capi import LfsError
    lib = sog.load_library()
    x = _t(np.zeros((4, 3), np.float32))
    lab = torch.zeros(4, dtype=torch.int32, device=x.device)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=x.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert lib.lfs_kmeans_assign(C.c_int64(4), C.c_uint32(0), C.c_uint32(3), p(x), p(x), p(lab), p(ws), C.c_size_t(ws.numel()), None) == -1
    assert lib.lfs_kmeans_assign(C.c_int64(4), C.c_uint32(65537), C.c_uint32(3), p(x), p(x), p(lab), p(ws), C.c_size_t(ws.numel()), None) == -2
    assert lib.lfs_kmeans_assign(C.c_int64(4), C.c_uint32(4), C.c_uint32(65), p(x), p(x), p(lab), p(ws), C.c_size_t(ws.numel()), None) == -2
    assert lib.lfs_kmeans_assign(C.c_int64(4), C.c_uint32(4), C.c_uint32(3), p(x), p(x), p(lab), p(ws), C.c_size_t(16), None) == -3
    assert lib.lfs_kmeans_assign(C.c_int64(4), C.c_uint32(4), C.c_uint32(3), None, p(x), p(lab), p(ws), C.c_size_t(ws.numel()), None) == -1
    assert lib.lfs_morton_encode(C.c_int64(4), p(x), None, p(ws), C.c_size_t(ws.numel()), None) == -1
    assert lib.lfs_morton_encode(C.c_int64(4), p(x), p(ws), p(ws), C.c_size_t(8), None) == -3
    assert lib.lfs_kmeans_assign_1d(C.c_int64(4), C.c_uint32(0), p(x), p(x), p(lab), None) == -1
    assert lib.lfs_kmeans_update(C.c_int64(4), C.c_uint32(2), C.c_uint32(65), p(x), p(lab), p(lab), p(x), None) == -2
    assert lib.lfs_kmeans_update(C.c_int64(4), C.c_uint32(2), C.c_uint32(3), p(x), None, p(lab), p(x), None) == -1
    with pytest.raises(LfsError):
        sog.kmeans_assign(x, _t(np.zeros((2, 4), np.float32)))
    with pytest.raises(LfsError):
        sog.morton_encode(_t(np.zeros((4, 2), np.float32)))
