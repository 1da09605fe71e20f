"""The models the scene transform (csrc/splat_transform.hip, lichtfeld-studio_amd/transform.py) is held to, the cases, and the checks themselves -
written once with the device as an argument, so that tests/test_emulated_splat_transform.py (the kernels as host code on the wavefront emulator) and
tests/test_gpu_splat_transform.py (the MI355X) run the SAME bodies.

FLOAT64 MODEL. x' = s R x + t, q' = q_R (x) q, raw' = raw + log s, and per colour channel and band a'_l = M_l a_l with M_l from THIS module's own construction: a
least-squares fit A_l M = B_l, A = Y_l(d_j), B = Y_l(R^T d_j) over 96 Fibonacci-sphere directions (numpy lstsq; the library fits over 64 directions through the normal
equations with constants from closed forms - here the decimal constants of Sloan's paper, taken as float64), so that for every unit d
sum_k a'_k Y_k(d) = sum_k a_k Y_k(R^T d): the scene rotated by R, seen along R d, shows the colour d showed before.

FLOAT32 MODEL. The arithmetic lfs_gsplat.h fixes for lfs_splat_transform_apply, restated in numpy float32 on the float32 record the library built (numpy's float32
operations are IEEE single operations, un-fused): the kernel's result must equal it bit for bit.

BOUNDS against the float64 model, u = 2^-24 (half an ulp, relative):
  SH element i of band l   (2l+3) u sum_k |M_ik| |a_k|      a dot product of 2l+1 terms (2l+1 products, 2l additions, each within u of the partial sums, which the
                                                           absolute sum bounds) plus one rounding of every matrix entry
  means                    5 u (sum_j |sR_ij| |x_j| + |t_i|)   three products, three sums, one rounding of each entry of sR and t: 4 + 1
  quaternions              5 u sum |q_R| |q|  per component  four products, three sums, the rounding of q_R
  log-scales               exactly fl(raw + log_s), log_s = fl32(log s)
ROUND TRIP (xf, then xf.inverse()): the second pass's bound on its own inputs plus the first pass's bound carried through the second pass's linear map in absolute
value - "twice those bounds" with each pass's magnitudes; for the log-scales one rounding per addition, u (|raw + log_s| + |raw|), plus |fl32(log s) + fl32(log 1/s)|."""
import ctypes as C
import functools

import numpy as np

U = 2.0 ** -24
SIZES = (1, 63, 64, 65, 85, 129, 255, 256, 257, 1000)      # 85 / 129: one past a tile of the SH kernel at degree 4 (84 rows) and at degrees 1-3 (128)
# (rows of shN held, degree rotated): every held degree with all of its bands; rotated degree below the held one (pass-through rows); row counts that belong to no degree
SH_CASES = [(0, 0), (3, 1), (8, 2), (15, 3), (24, 4), (15, 0), (15, 1), (15, 2), (24, 3), (24, 1), (10, 2), (17, 3)]
GUARD = 3


# ---- the basis in float64 (Sloan, "Efficient Spherical Harmonic Evaluation", JCGT 2013), the coefficient order and signs of sh_basis (csrc/lfs_sh.cuh) -------------
def basis64(d):
    d = np.asarray(d, np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    b = [None] * 25
    b[0] = np.full(x.shape, 0.2820947917738781)
    c1 = 0.48860251190292
    b[1], b[2], b[3] = -c1 * y, c1 * z, -c1 * x
    z2 = z * z
    t0B = -1.092548430592079 * z
    fC1, fS1 = x * x - y * y, 2.0 * x * y
    c2 = 0.5462742152960395
    b[4], b[5], b[6], b[7], b[8] = c2 * fS1, t0B * y, 0.9461746957575601 * z2 - 0.3153915652525201, t0B * x, c2 * fC1
    t0C = -2.285228997322329 * z2 + 0.4570457994644658
    t1B = 1.445305721320277 * z
    fC2, fS2 = x * fC1 - y * fS1, x * fS1 + y * fC1
    c3 = -0.5900435899266435
    b[9], b[10], b[11] = c3 * fS2, t1B * fS1, t0C * y
    b[12] = z * (1.865881662950577 * z2 - 1.119528997770346)
    b[13], b[14], b[15] = t0C * x, t1B * fC1, c3 * fC2
    t0D = z * (-4.683325804901025 * z2 + 2.007139630671868)
    t1C = 3.31161143515146 * z2 - 0.47308734787878
    t2B = -1.770130769779931 * z
    fC3, fS3 = x * fC2 - y * fS2, x * fS2 + y * fC2
    c4 = 0.6258357354491763
    b[16], b[17], b[18], b[19] = c4 * fS3, t2B * fS2, t1C * fS1, t0D * y
    b[20] = 1.984313483298443 * z * b[12] - 1.006230589874905 * b[6]
    b[21], b[22], b[23], b[24] = t0D * x, t1C * fC1, t2B * fC2, c4 * fC3
    return np.stack(b, -1)


def fibonacci_sphere(n):
    i = np.arange(n) + 0.5
    ph, th = np.arccos(1.0 - 2.0 * i / n), np.pi * (1.0 + 5.0 ** 0.5) * i
    return np.stack([np.cos(th) * np.sin(ph), np.sin(th) * np.sin(ph), np.cos(ph)], 1)


def band_matrices64(R, degree=4):
    """[M_1 .. M_degree], this module's own construction"""
    R = np.asarray(R, np.float64)
    d = fibonacci_sphere(96)
    A, B = basis64(d), basis64(d @ R)          # row j of d @ R is (R^T d_j)^T
    return [np.linalg.lstsq(A[:, l * l:(l + 1) ** 2], B[:, l * l:(l + 1) ** 2], rcond=None)[0] for l in range(1, degree + 1)]


def quat_to_rotmat(q):
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def rotmat_to_quat64(R):
    """wxyz, w >= 0 (through the eigenvector of the largest eigenvalue of the symmetric 4x4 of Bar-Itzhack - not Shepperd's branches, which the library uses)"""
    R = np.asarray(R, np.float64)
    K = np.array([[R[0, 0] - R[1, 1] - R[2, 2], 0, 0, 0], [R[0, 1] + R[1, 0], R[1, 1] - R[0, 0] - R[2, 2], 0, 0],
                  [R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], R[2, 2] - R[0, 0] - R[1, 1], 0],
                  [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], R[0, 0] + R[1, 1] + R[2, 2]]]) / 3.0
    w, v = np.linalg.eigh(K, UPLO="L")
    x, y, z, qw = v[:, np.argmax(w)]
    q = np.array([qw, x, y, z])
    return q if q[0] >= 0 else -q


def random_rotations(n, seed):
    rng = np.random.default_rng(seed)
    return [quat_to_rotmat(rng.normal(size=4)) for _ in range(n)]


def axis_aligned_rotations():
    """the 24 proper signed permutation matrices"""
    import itertools
    out = []
    for p in itertools.permutations(range(3)):
        for sg in itertools.product((1.0, -1.0), repeat=3):
            R = np.zeros((3, 3))
            for i in range(3):
                R[i, p[i]] = sg[i]
            if np.linalg.det(R) > 0:
                out.append(R)
    assert len(out) == 24
    return out


def matrix4(s, R, t):
    m = np.eye(4)
    m[:3, :3] = s * np.asarray(R, np.float64)
    m[:3, 3] = t
    return m


def decompose64(m):
    """(s, R, t) of a similarity 4x4 in float64, R the polar factor"""
    m = np.asarray(m, np.float64)
    s = float(np.cbrt(np.linalg.det(m[:3, :3])))
    u, _, vt = np.linalg.svd(m[:3, :3])
    return s, u @ vt, m[:3, 3].copy()


# ---- the float64 model and the bounds ------------------------------------------------------------------------------------------------------------------------
def hamilton64(a, b):
    """a (x) b, a [4] or [N,4], b [N,4], wxyz"""
    w1, x1, y1, z1 = np.moveaxis(np.asarray(a, np.float64), -1, 0)
    w2, x2, y2, z2 = np.moveaxis(np.asarray(b, np.float64), -1, 0)
    return np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                     w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], -1)


def hamilton_abs(a, b):
    a, b = np.abs(np.asarray(a, np.float64)), np.abs(np.asarray(b, np.float64))
    w1, x1, y1, z1 = np.moveaxis(a, -1, 0)
    w2, x2, y2, z2 = np.moveaxis(b, -1, 0)
    return np.stack([w1 * w2 + x1 * x2 + y1 * y2 + z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 + z1 * y2, w1 * y2 + x1 * z2 + y1 * w2 + z1 * x2,
                     w1 * z2 + x1 * y2 + y1 * x2 + z1 * w2], -1)


def sh_apply64(mats, shN, degree):
    """shN [N,K,3] float64 -> bands 1..degree multiplied by mats, further rows unchanged"""
    out = np.array(shN, np.float64)
    for l in range(1, degree + 1):
        a, b = l * l - 1, (l + 1) ** 2 - 1
        out[:, a:b, :] = np.einsum("ik,nkc->nic", mats[l - 1], np.asarray(shN, np.float64)[:, a:b, :])
    return out


def sh_abs(mats, shN, degree):
    """sum_k |M_ik| |a_k| per element (0 on the pass-through rows), and the per-band factor (2l+3)"""
    mag = np.zeros(np.shape(shN), np.float64)
    fac = np.zeros(np.shape(shN), np.float64)
    for l in range(1, degree + 1):
        a, b = l * l - 1, (l + 1) ** 2 - 1
        mag[:, a:b, :] = np.einsum("ik,nkc->nic", np.abs(mats[l - 1]), np.abs(np.asarray(shN, np.float64)[:, a:b, :]))
        fac[:, a:b, :] = 2 * l + 3
    return mag, fac


class Model64:
    """the float64 model of one transform (matrix m [4,4]) at SH degree `degree`"""

    def __init__(self, m, degree, q_like=None):
        """q_like: the record's quaternion - at w = 0 (a rotation by pi) both signs are 'w >= 0'; the model takes the library's"""
        self.s, self.R, self.t = decompose64(m)
        self.degree = degree
        self.mats = band_matrices64(self.R, 4)
        self.qR = rotmat_to_quat64(self.R)
        if q_like is not None and abs(self.qR[0]) < 1e-6 and float(np.dot(self.qR, np.asarray(q_like, np.float64))) < 0:
            self.qR = -self.qR
        self.sR = self.s * self.R

    def means(self, x):
        x = np.asarray(x, np.float64)
        return x @ self.sR.T + self.t, 5 * U * (np.abs(x) @ np.abs(self.sR).T + np.abs(self.t))

    def quats(self, q):
        return hamilton64(self.qR, q), 5 * U * hamilton_abs(self.qR, q)

    def scales_exact(self, raw, log_s32):
        """fl(raw + log_s) with the record's log_s, which must itself be log s rounded once (one more ulp where the library's s = cbrt(det) is a last float64 bit off)"""
        assert abs(float(log_s32) - np.log(self.s)) <= U * abs(np.log(self.s)) + 1e-15
        return (np.asarray(raw, np.float32) + np.float32(log_s32)).astype(np.float32)

    def shN(self, a):
        mag, fac = sh_abs(self.mats, a, self.degree)
        return sh_apply64(self.mats, a, self.degree), fac * U * mag


# ---- the float32 model: lfs_splat_transform_apply's arithmetic on the library's record ---------------------------------------------------------------------------
def record_arrays(rec):
    f = lambda a: np.array(list(a), np.float32)
    return dict(sR=f(rec.sR).reshape(3, 3), t=f(rec.t), q=f(rec.q), log_s=np.float32(rec.log_s), sh_degree=int(rec.sh_degree),
                mats=[f(rec.m1).reshape(3, 3), f(rec.m2).reshape(5, 5), f(rec.m3).reshape(7, 7), f(rec.m4).reshape(9, 9)])


def model32(rec, means=None, quats=None, raw_scales=None, shN=None):
    r = record_arrays(rec)
    out = [None, None, None, None]
    if means is not None:
        x, y, z = (np.asarray(means, np.float32)[:, j] for j in range(3))
        out[0] = np.stack([((r["sR"][i, 0] * x + r["sR"][i, 1] * y) + r["sR"][i, 2] * z) + r["t"][i] for i in range(3)], 1)
    if quats is not None:
        w1, x1, y1, z1 = r["q"]
        w2, x2, y2, z2 = (np.asarray(quats, np.float32)[:, j] for j in range(4))
        out[1] = np.stack([((w1 * w2 - x1 * x2) - y1 * y2) - z1 * z2, ((w1 * x2 + x1 * w2) + y1 * z2) - z1 * y2, ((w1 * y2 - x1 * z2) + y1 * w2) + z1 * x2,
                           ((w1 * z2 + x1 * y2) - y1 * x2) + z1 * w2], 1)
    if raw_scales is not None:
        out[2] = np.asarray(raw_scales, np.float32) + r["log_s"]
    if shN is not None:
        a = np.asarray(shN, np.float32)
        o = a.copy()
        for l in range(1, r["sh_degree"] + 1):
            M, lo = r["mats"][l - 1], l * l - 1
            for i in range(2 * l + 1):
                acc = M[i, 0] * a[:, lo, :]
                for k in range(1, 2 * l + 1):
                    acc = acc + M[i, k] * a[:, lo + k, :]
                o[:, lo + i, :] = acc
        out[3] = o
    assert all(v is None or v.dtype == np.float32 for v in out)
    return out


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------------------------
def inputs(N, rows, seed=0):
    """means up to 1e3, raw quaternions of norm 1e-3 .. 1e3, log-scales, coefficients +-2"""
    rng = np.random.default_rng(1000 * seed + 7 * N + rows)
    means = (rng.uniform(-1, 1, (N, 3)) * 10.0 ** rng.uniform(-2, 3, (N, 1))).astype(np.float32)
    q = rng.normal(size=(N, 4))
    quats = (q / np.linalg.norm(q, axis=1, keepdims=True) * 10.0 ** rng.uniform(-3, 3, (N, 1))).astype(np.float32)
    scales = rng.uniform(-8, 3, (N, 3)).astype(np.float32)
    shN = rng.uniform(-2, 2, (N, rows, 3)).astype(np.float32)
    return means, quats, scales, shN


GENERIC = matrix4(1.7, quat_to_rotmat([0.51, -0.37, 0.64, 0.44]), [3.25, -110.5, 0.0625])


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


# ---- host functions (CPU, through the built library) ---------------------------------------------------------------------------------------------------------------
def check_band_matrices(lfs):
    from lichtfeld_studio_amd import transform
    rots = random_rotations(200, seed=11) + axis_aligned_rotations() + [np.eye(3)]
    dirs = np.random.default_rng(5).normal(size=(50, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    coeff = np.random.default_rng(6).normal(size=25)
    worst = dict(orth=0.0, identity=0.0, product=0.0)
    mats = [transform.sh_rotation_matrices(R, 4) for R in rots]
    for R, Ms in zip(rots, mats):
        assert [m.shape for m in Ms] == [(3, 3), (5, 5), (7, 7), (9, 9)]
        moved = coeff.copy()
        for l, M in enumerate(Ms, 1):
            worst["orth"] = max(worst["orth"], np.abs(M @ M.T - np.eye(2 * l + 1)).max())
            moved[l * l:(l + 1) ** 2] = M @ coeff[l * l:(l + 1) ** 2]
        # sum_k a'_k Y_k(d) = sum_k a_k Y_k(R^T d)   (rows of dirs @ R are (R^T d)^T)
        worst["identity"] = max(worst["identity"], np.abs(basis64(dirs) @ moved - basis64(dirs @ R) @ coeff).max())
    for i in range(0, 200, 2):
        Ms = transform.sh_rotation_matrices(rots[i] @ rots[i + 1], 4)
        for l in range(4):
            worst["product"] = max(worst["product"], np.abs(Ms[l] - mats[i][l] @ mats[i + 1][l]).max())
    print("band matrices:", worst)
    assert worst["orth"] <= 1e-12 and worst["identity"] <= 1e-12 and worst["product"] <= 1e-12, worst
    for l, M in enumerate(mats[-1], 1):
        assert np.array_equal(M, np.eye(2 * l + 1))
    # against this module's own construction
    for R in rots[:20]:
        for a, b in zip(transform.sh_rotation_matrices(R, 4), band_matrices64(R)):
            assert np.abs(a - b).max() <= 1e-12
    assert len(transform.sh_rotation_matrices(rots[0], 2)) == 2 and transform.sh_rotation_matrices(rots[0], 0) == []
    import pytest
    with pytest.raises(lfs.capi.LfsError):
        transform.sh_rotation_matrices(rots[0], 5)


def refused_matrices():
    """(name, 4x4, sh_degree): every refusal of lfs_splat_transform_from_matrix with a minimal matrix"""
    e = np.eye(4)
    def put(i, j, v):
        m = e.copy(); m[i, j] = v; return m
    return [("nan", put(0, 3, np.nan), 0), ("inf", put(1, 1, np.inf), 0), ("last row w", put(3, 3, 2.0), 0), ("last row x", put(3, 0, 1e-30), 0),
            ("zero scale", np.diag([0.0, 0.0, 0.0, 1.0]), 0), ("negative scale", np.diag([-1.0, -1.0, -1.0, 1.0]), 0), ("reflection", np.diag([1.0, 1.0, -1.0, 1.0]), 0),
            ("non-uniform scale", np.diag([1.0, 1.0, 1.0 + 1e-4, 1.0]), 0), ("shear", put(0, 1, 1e-4), 0), ("degree", e.copy(), 5)]


def check_from_matrix(lfs):
    import pytest
    from lichtfeld_studio_amd import transform
    from lichtfeld_studio_amd.capi import LfsError, SplatTransformStruct
    lib = lfs.load_library()
    assert C.sizeof(SplatTransformStruct) == 728
    for name, m, deg in refused_matrices():
        rec = SplatTransformStruct()
        m = np.ascontiguousarray(m, np.float64)
        assert lib.lfs_splat_transform_from_matrix(m.ctypes.data_as(C.c_void_p), C.c_uint32(deg), C.byref(rec)) == -1, name
        if deg <= 4:
            with pytest.raises(LfsError):
                transform.similarity(m)
    assert lib.lfs_splat_transform_from_matrix(None, C.c_uint32(0), C.byref(SplatTransformStruct())) == -1
    # just inside the similarity test: accepted
    transform.similarity(np.diag([1.0, 1.0, 1.0 + 1e-6, 1.0]))
    R = quat_to_rotmat([0.3, 0.5, -0.2, 0.79])
    for s in (1e-3, 1.0, 1e3):
        xf = transform.similarity(rotation=R, scale=s, translation=[1.0, -2.0, 3.0])
        r = record_arrays(xf.record(4))
        assert np.abs(r["sR"] - s * R).max() <= U * 2 * s and abs(float(r["log_s"]) - np.log(s)) <= U * abs(np.log(s)) + 1e-15 and r["sh_degree"] == 4
        q = rotmat_to_quat64(R)
        assert r["q"][0] >= 0 and np.abs(r["q"] - q).max() <= 2 * U and abs(np.linalg.norm(r["q"].astype(np.float64)) - 1) <= 4 * U
        for a, b in zip(r["mats"], band_matrices64(R)):
            assert np.array_equal(a, b.astype(np.float32)) or np.abs(a - b).max() <= U   # float64 values within 1e-12 round to the same float32, or to its neighbour at a tie
        assert np.array_equal(r["t"], np.array([1, -2, 3], np.float32))
    # quaternion input == matrix input; Shepperd's other three branches (rotations by pi about the axes: w = 0)
    assert np.allclose(transform.similarity(rotation=[0.3, 0.5, -0.2, 0.79]).matrix, transform.similarity(rotation=R).matrix, atol=1e-15)
    for R2 in axis_aligned_rotations():
        r = record_arrays(transform.similarity(rotation=R2).record(0))
        assert r["q"][0] >= 0 and np.abs(quat_to_rotmat(r["q"]) - R2).max() <= 4 * U
    # the identity: the identity record, bit for bit
    for deg in range(5):
        rec = transform.similarity(np.eye(4)).record(deg)
        want = SplatTransformStruct()
        for i in (0, 4, 8):
            want.sR[i] = 1.0
        want.q[0] = 1.0
        want.sh_degree = deg
        for name, n in (("m1", 3), ("m2", 5), ("m3", 7), ("m4", 9)):
            for i in range(n):
                getattr(want, name)[i * n + i] = 1.0
        assert bytes(rec) == bytes(want)
    # inverse and composition in float64
    xf = transform.similarity(GENERIC)
    assert np.abs((xf @ xf.inverse()).matrix - np.eye(4)).max() <= 1e-12 and np.abs((xf.inverse() @ xf).matrix - np.eye(4)).max() <= 1e-12
    s, R, t = decompose64(GENERIC)
    assert abs(xf.scale - s) <= 1e-15 * s and np.abs(xf.rotation - R).max() <= 1e-15 and np.array_equal(xf.translation, t)
    # a matrix off a similarity by less than the tolerance is re-orthonormalised before anything is derived from it
    skew = GENERIC.copy(); skew[:3, :3] = skew[:3, :3] @ (np.eye(3) + 3e-6 * np.array([[0, 1, 0], [1, 0, 0], [0, 0, 0.0]]))
    r = record_arrays(transform.similarity(skew).record(4))
    Rr = r["sR"].astype(np.float64) / np.exp(np.float64(r["log_s"]))
    assert np.abs(Rr @ Rr.T - np.eye(3)).max() <= 8 * U
    assert np.abs(r["mats"][3].astype(np.float64) @ r["mats"][3].astype(np.float64).T - np.eye(9)).max() <= 16 * U


# ---- the kernel (emulated and on the GPU) ----------------------------------------------------------------------------------------------------------------------------
def _guarded(torch, dev, arr, misalign):
    """a NaN-filled flat buffer with GUARD rows (+ one float when misaligned) in front and GUARD rows behind a view of arr's shape -> (buffer, view)"""
    n = int(np.prod(arr.shape))
    row = int(np.prod(arr.shape[1:])) if arr.ndim > 1 else 1
    front = GUARD * row
    front += (-front) % 4
    if misalign:
        front += 1
    buf = torch.full((front + n + GUARD * row,), float("nan"), dtype=torch.float32, device=dev)
    return buf, buf[front:front + n].view(*arr.shape), front


def _guards_intact(buf, front, n):
    import torch
    return bool(torch.isnan(buf[:front]).all()) and bool(torch.isnan(buf[front + n:]).all())


def run_apply(dev, xf, degree, arrays, inplace, misalign=False):
    """arrays: (means, quats, scales, shN) numpy or None each -> numpy results through transform.apply on guarded buffers; asserts that the guards survive"""
    import torch
    from lichtfeld_studio_amd import transform
    ins, outs, keep = [], [], []
    for a in arrays:
        if a is None:
            ins.append(None); outs.append(None); continue
        buf_i, view_i, front_i = _guarded(torch, dev, a, misalign)
        view_i.copy_(torch.from_numpy(a).to(dev))
        if inplace:
            buf_o, view_o, front_o = buf_i, view_i, front_i
        else:
            buf_o, view_o, front_o = _guarded(torch, dev, a, misalign)
        ins.append(view_i); outs.append(view_o); keep.append((buf_i, front_i, buf_o, front_o, a.size, a))
    got = transform.apply(xf, degree, *ins, out="inplace" if inplace else tuple(outs))
    if dev != "cpu":
        torch.cuda.synchronize()
    for buf_i, front_i, buf_o, front_o, n, a in keep:
        assert _guards_intact(buf_i, front_i, n) and _guards_intact(buf_o, front_o, n), "a guard row was written"
        if not inplace:
            assert np.array_equal(bits(buf_i[front_i:front_i + n].cpu().numpy()), bits(a).reshape(-1)), "an input was written"
    return [None if g is None else g.cpu().numpy() for g in got]


def _assert_within(got, want64, bound, what):
    err = np.abs(np.asarray(got, np.float64) - want64)
    bad = err > bound
    assert not bad.any(), (what, float((err / np.maximum(bound, 1e-300)).max()), int(bad.sum()))


def check_kernel_case(dev, N, rows, degree, inplace, misalign, m=None, seed=0):
    """one launch: bit-equality with the float32 model and the float64 bounds"""
    from lichtfeld_studio_amd import transform
    xf = transform.similarity(GENERIC if m is None else m)
    means, quats, scales, shN = inputs(N, rows, seed)
    got = run_apply(dev, xf, degree, (means, quats, scales, shN), inplace, misalign)
    want = model32(xf.record(degree), means, quats, scales, shN)
    for g, w, name in zip(got, want, ("means", "quats", "raw_scales", "shN")):
        assert g.shape == w.shape and np.array_equal(bits(g), bits(w)), (name, N, rows, degree, inplace, misalign, int((bits(g) != bits(w)).sum()))
    rec = record_arrays(xf.record(degree))
    m64 = Model64(xf.matrix, degree, q_like=rec["q"])
    _assert_within(got[0], *m64.means(means), "means")
    _assert_within(got[1], *m64.quats(quats), "quats")
    assert np.array_equal(bits(got[2]), bits(m64.scales_exact(scales, rec["log_s"])))
    if rows:
        _assert_within(got[3], *m64.shN(shN), "shN")
        if rows > (degree + 1) ** 2 - 1:
            assert np.array_equal(bits(got[3][:, (degree + 1) ** 2 - 1:]), bits(shN[:, (degree + 1) ** 2 - 1:])), "pass-through rows"


def check_kernel_sizes(dev):
    for N in SIZES:
        for rows, degree in SH_CASES:
            # every (size, case) out of place on aligned buffers; in place and the 4-byte-aligned path alternate over the table so that every case and every size meets both
            check_kernel_case(dev, N, rows, degree, inplace=False, misalign=False)
    for i, N in enumerate(SIZES):
        for j, (rows, degree) in enumerate(SH_CASES):
            check_kernel_case(dev, N, rows, degree, inplace=True, misalign=bool((i + j) & 1), seed=1)
            if (i + j) % 3 == 0:
                check_kernel_case(dev, N, rows, degree, inplace=False, misalign=True, seed=2)


def check_transforms(dev):
    """other transforms than GENERIC at one ragged size: identity (every bit unchanged), pure scales, axis-aligned rotations, a rotation by pi (w = 0)"""
    from lichtfeld_studio_amd import transform
    means, quats, scales, shN = inputs(257, 24, 3)
    got = run_apply(dev, transform.similarity(np.eye(4)), 4, (means, quats, scales, shN), False)
    for g, a in zip(got, (means, quats, scales, shN)):
        assert np.array_equal(bits(g), bits(a))
    for m in [matrix4(1e-3, np.eye(3), [0, 0, 0]), matrix4(1e3, quat_to_rotmat([0.1, 0.9, -0.3, 0.2]), [-5e2, 1, 7]), matrix4(1.0, axis_aligned_rotations()[7], [1, 2, 3]),
              matrix4(0.5, quat_to_rotmat([0, 0.6, 0.8, 0]), [0.5, 0.25, -4])]:
        check_kernel_case(dev, 257, 24, 4, False, False, m=m, seed=4)
        check_kernel_case(dev, 65, 15, 3, True, False, m=m, seed=5)


def round_trip_bounds(xf, inv, degree, a0, a1):
    """bounds on |inverse(forward(a0)) - a0| for (means, quats, raw_scales, shN); a1 = the forward pass's results (the second pass's inputs)"""
    f, b = Model64(xf.matrix, degree, record_arrays(xf.record(0))["q"]), Model64(inv.matrix, degree, record_arrays(inv.record(0))["q"])
    out = [b.means(a1[0])[1] + f.means(a0[0])[1] @ np.abs(b.sR).T,                      # the second pass's bound on its inputs + the first's through |s' R'|
           b.quats(a1[1])[1] + hamilton_abs(b.qR, f.quats(a0[1])[1])]
    ls, li = np.float64(np.float32(np.log(f.s))), np.float64(np.float32(np.log(b.s)))
    raw = np.asarray(a0[2], np.float64)
    out.append(U * (np.abs(raw + ls) + np.abs(raw)) + (1 + U) * abs(ls + li))
    e1 = f.shN(a0[3])[1]
    carried = np.zeros_like(e1)
    for l in range(1, degree + 1):
        lo, hi = l * l - 1, (l + 1) ** 2 - 1
        carried[:, lo:hi, :] = np.einsum("ik,nkc->nic", np.abs(b.mats[l - 1]), e1[:, lo:hi, :])
    out.append(b.shN(a1[3])[1] + carried)
    return out


def check_round_trip(dev):
    from lichtfeld_studio_amd import transform
    for m, N, rows, degree in [(GENERIC, 257, 15, 3), (matrix4(0.5, quat_to_rotmat([0.2, -0.7, 0.1, 0.6]), [10, -20, 5]), 1000, 24, 4), (matrix4(2.0, axis_aligned_rotations()[5], [0, 1, 0]), 65, 8, 2)]:
        xf = transform.similarity(m)
        inv = xf.inverse()
        a0 = inputs(N, rows, 9)
        a1 = run_apply(dev, xf, degree, a0, False)
        a2 = run_apply(dev, inv, degree, tuple(a1), True)
        for got, want, bound, name in zip(a2, a0, round_trip_bounds(xf, inv, degree, a0, a1), ("means", "quats", "raw_scales", "shN")):
            _assert_within(got, np.asarray(want, np.float64), bound, name + " round trip")


def check_skipped_pairs(dev):
    from lichtfeld_studio_amd import transform
    xf = transform.similarity(GENERIC)
    means, quats, scales, shN = inputs(130, 15, 12)
    full = model32(xf.record(3), means, quats, scales, shN)
    for mask in [(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 0, 1, 0), (0, 1, 0, 1), (0, 0, 0, 0)]:
        arrays = tuple(a if k else None for a, k in zip((means, quats, scales, shN), mask))
        for inplace in (False, True):
            got = run_apply(dev, xf, 3, arrays, inplace)
            for g, w, k in zip(got, full, mask):
                assert (g is None) if not k else np.array_equal(bits(g), bits(w))


def check_entry_refusals(lfs):
    """LFS_E_INVALID before any launch: the pointers are host memory no kernel could read, and a launch without a device would not come back as -1"""
    from lichtfeld_studio_amd import transform
    from lichtfeld_studio_amd.capi import SplatTransformStruct
    lib = lfs.load_library()
    buf = (C.c_float * 4096)()
    p = C.cast(buf, C.c_void_p)
    rec = transform.similarity(GENERIC).record(3)
    call = lambda N, r, a, rows, b: lib.lfs_splat_transform_apply(C.c_uint32(N), r, a[0], a[1], a[2], a[3], C.c_uint32(rows), b[0], b[1], b[2], b[3], None)
    none = (None, None, None, None)
    for k in range(4):                                       # a half-NULL pair, either half
        only = tuple(p if j == k else None for j in range(4))
        assert call(8, C.byref(rec), only, 15, none) == -1 and call(8, C.byref(rec), none, 15, only) == -1
    assert call(8, C.byref(rec), (None, None, None, p), 14, (None, None, None, p)) == -1       # degree 3 needs 15 rows
    assert call(8, C.byref(rec), (None, None, None, p), 0, (None, None, None, p)) == -1
    bad = SplatTransformStruct.from_buffer_copy(bytes(rec)); bad.sh_degree = 5
    assert call(8, C.byref(bad), (None, None, None, p), 35, (None, None, None, p)) == -1        # sh_degree > 4
    assert call(8, None, (p, None, None, None), 0, (p, None, None, None)) == -1                 # NULL record
    assert call(8, C.byref(rec), (None, None, None, p), 512, (None, None, None, p)) == -2       # LFS_E_UNSUPPORTED: rows beyond the LDS tile
    assert call(0, C.byref(rec), (p, p, p, p), 15, (p, p, p, p)) == 0                           # N == 0: LFS_OK, nothing launched
    assert call(8, C.byref(rec), none, 0, none) == 0                                            # every pair skipped: nothing to launch
    assert not any(buf)


# ---- render invariance -------------------------------------------------------------------------------------------------------------------------------------------------
W_IMG, H_IMG = 64, 48


@functools.lru_cache(maxsize=None)
def render_scene(n=2000, seed=3):
    """~2000 Gaussians in front of two cameras, every depth in [2, 6] for both, shN amplitudes ~0.5 -> dict of numpy arrays"""
    rng = np.random.default_rng(seed)
    means = np.stack([rng.uniform(-1.4, 1.4, n), rng.uniform(-1.0, 1.0, n), rng.uniform(-1.4, 1.4, n)], 1).astype(np.float32)
    q = rng.normal(size=(n, 4)).astype(np.float32)
    scales = np.log(rng.uniform(0.03, 0.12, (n, 3))).astype(np.float32)
    opac = rng.uniform(-1.0, 2.0, (n, 1)).astype(np.float32)
    sh0 = rng.uniform(-0.5, 1.5, (n, 1, 3)).astype(np.float32)
    shN = (rng.normal(size=(n, 15, 3)) * 0.5).astype(np.float32)
    cams = []
    for eye in ([0.0, 0.0, -4.0], [1.2, 0.5, -3.9]):
        eye = np.array(eye)
        f = -eye / np.linalg.norm(eye)
        r = np.cross([0.0, 1.0, 0.0], f); r /= np.linalg.norm(r)
        w = np.eye(4); w[:3, :3] = np.stack([r, np.cross(f, r), f]); w[:3, 3] = -w[:3, :3] @ eye
        cams.append(w)
    cams = np.stack(cams)
    z = means.astype(np.float64) @ cams[:, 2, :3].T + cams[:, 2, 3]
    assert z.min() >= 2.0 and z.max() <= 6.0, (z.min(), z.max())
    K = np.array([[60.0, 0, W_IMG / 2], [0, 60.0, H_IMG / 2], [0, 0, 1]])
    return dict(means=means, quats=q, scales=scales, opac=opac, sh0=sh0, shN=shN, viewmats=cams, K=K)


RENDER_TRANSFORMS = [matrix4(s, quat_to_rotmat([0.35, 0.61, -0.48, 0.52]), t) for s, t in ((0.5, [1.0, -2.0, 0.5]), (1.0, [-3.0, 0.25, 2.0]), (2.0, [0.5, 4.0, -1.0]))]


def _model(torch, dev, sc, **over):
    from lichtfeld_studio_amd.rasterizer import SplatModel
    a = dict(sc, **over)
    t = lambda k: torch.from_numpy(np.ascontiguousarray(a[k], np.float32)).to(dev)
    return SplatModel(t("means"), t("sh0"), t("shN"), t("scales"), t("quats"), t("opac"), 3)


def render_errors(dev, route, m):
    """-> (e_kernel, e_twin, e_ref): mean absolute differences to render(model, cam), summed over the two views' means / 2"""
    import torch
    from lichtfeld_studio_amd import fastgs, transform
    from lichtfeld_studio_amd.rasterizer import Camera, rasterize
    sc = render_scene()
    xf = transform.similarity(m)
    model = _model(torch, dev, sc)
    m64 = Model64(xf.matrix, 3)
    twin = _model(torch, dev, sc, means=m64.means(sc["means"])[0], quats=m64.quats(sc["quats"])[0], scales=sc["scales"].astype(np.float64) + np.log(m64.s),
                  shN=m64.shN(sc["shN"])[0])
    moved = transform.transform_model(model, xf)
    ref = transform.transform_model(model, xf, rotate_sh=False)
    assert torch.equal(ref.shN, model.shN) and torch.equal(ref.means, moved.means) and torch.equal(ref.raw_quats, moved.raw_quats)
    vm = torch.from_numpy(sc["viewmats"]).to(torch.float32).to(dev)
    vm2 = transform.transform_cameras(vm, xf)
    K = torch.from_numpy(sc["K"]).to(torch.float32).to(dev).reshape(1, 3, 3)
    bg = torch.zeros(3, device=dev)
    render = (lambda c, mo: fastgs.fast_rasterize(c, mo, bg).image) if route == "fastgs" else (lambda c, mo: rasterize(c, mo, bg).image)
    e = np.zeros(3)
    with torch.no_grad():
        for v in range(2):
            c0 = Camera(vm[v:v + 1].contiguous(), K, W_IMG, H_IMG)
            c1 = Camera(vm2[v:v + 1].contiguous(), K, W_IMG, H_IMG)
            base = render(c0, model).double()
            assert float(base.mean()) > 0.05
            for i, mo in enumerate((moved, twin, ref)):
                e[i] += float((render(c1, mo).double() - base).abs().mean()) / 2
    return tuple(e)


def check_render_invariance(dev, route, scales=(0.5, 1.0, 2.0)):
    for m in RENDER_TRANSFORMS:
        s = decompose64(m)[0]
        if not any(abs(s - a) < 1e-9 for a in scales):
            continue
        e_kernel, e_twin, e_ref = render_errors(dev, route, m)
        print(f"render invariance [{route}] s={s}: e_kernel {e_kernel:.3e} e_twin {e_twin:.3e} e_ref {e_ref:.3e}")
        assert e_kernel <= 2 * e_twin + 4.0 / (255 * H_IMG * W_IMG), (route, s, e_kernel, e_twin)
        assert e_ref >= 20 * e_twin + 1e-3, (route, s, e_ref, e_twin)


# ---- crop -----------------------------------------------------------------------------------------------------------------------------------------------------------------
def check_crop(dev):
    import torch
    from lichtfeld_studio_amd import transform
    from lichtfeld_studio_amd.rasterizer import SplatModel
    rng = np.random.default_rng(21)
    n = 500
    means = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
    lo, hi = np.array([-1.0, -0.5, -1.5]), np.array([0.75, 1.0, 0.5])
    w2b = np.linalg.inv(matrix4(1.0, quat_to_rotmat([0.8, 0.1, -0.5, 0.3]), [0.2, -0.1, 0.3]))
    # points chosen off the faces: those within 1e-4 of a face of either box are pushed out of the table
    def dist(p):
        return np.minimum(np.abs(p - lo), np.abs(p - hi)).min(1)
    pb = means.astype(np.float64) @ w2b[:3, :3].T + w2b[:3, 3]
    ok = (dist(means.astype(np.float64)) > 1e-4) & (dist(pb) > 1e-4)
    means = means[ok]; pb = pb[ok]; n = len(means)
    assert n > 450
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    ids = np.arange(n, dtype=np.float32)
    model = SplatModel(t(means), t(np.tile(ids[:, None, None], (1, 1, 3))), t(rng.normal(size=(n, 3, 3))), t(rng.normal(size=(n, 3))), t(rng.normal(size=(n, 4))),
                       t(ids[:, None]), 1, 0)
    m64 = means.astype(np.float64)
    for mask, kw in [(((m64 >= lo) & (m64 <= hi)).all(1), {}), (((pb >= lo) & (pb <= hi)).all(1), dict(world_to_box=w2b))]:
        assert 10 < mask.sum() < n - 10
        for invert in (False, True):
            want = np.nonzero(~mask if invert else mask)[0]
            out = transform.crop(model, lo, hi, invert=invert, **kw)
            assert np.array_equal(out.raw_opacities.cpu().numpy().reshape(-1), ids[want])      # which, and in order
            assert np.array_equal(out.sh0.cpu().numpy()[:, 0, 0], ids[want]) and np.array_equal(bits(out.means.cpu().numpy()), bits(means[want]))
            assert out.shN.shape == (len(want), 3, 3) and out.raw_quats.shape == (len(want), 4) and out.raw_scales.shape == (len(want), 3)
            assert (out.max_sh_degree, out.active_sh_degree) == (1, 0) and all(p.is_contiguous() for p in out.parameters())
    empty = transform.crop(model, [10, 10, 10], [11, 11, 11])
    assert [tuple(p.shape) for p in empty.parameters()] == [(0, 3), (0, 1, 3), (0, 3, 3), (0, 3), (0, 4), (0, 1)]
    assert transform.crop(model, [10, 10, 10], [11, 11, 11], invert=True).means.shape[0] == n
    moved = transform.transform_model(empty, transform.similarity(GENERIC))                      # N = 0 goes through the entry
    assert moved.means.shape == (0, 3) and moved.shN.shape == (0, 3, 3)


def check_transform_model(dev):
    """transform_model: every band the model HOLDS is carried whatever the active degree; in place returns the same object; sh0 / opacities untouched"""
    import torch
    from lichtfeld_studio_amd import transform
    from lichtfeld_studio_amd.rasterizer import SplatModel
    xf = transform.similarity(GENERIC)
    for deg, rows in ((0, 0), (1, 3), (3, 15), (4, 24)):
        means, quats, scales, shN = inputs(257, rows, 30 + deg)
        t = lambda a: torch.from_numpy(a).to(dev)
        sh0, opac = np.full((257, 1, 3), 0.25, np.float32), np.full((257, 1), -1.5, np.float32)
        model = SplatModel(t(means), t(sh0), t(shN), t(scales), t(quats), t(opac), deg, 0)
        want = model32(xf.record(deg), means, quats, scales, shN if rows else None)
        out = transform.transform_model(model, xf)
        assert out is not model and (out.max_sh_degree, out.active_sh_degree) == (deg, 0)
        got = [out.means, out.raw_quats, out.raw_scales] + ([out.shN] if rows else [])
        for g, w in zip(got, want):
            assert np.array_equal(bits(g.cpu().numpy()), bits(w))
        assert out.shN.shape == (257, rows, 3) and torch.equal(out.sh0, model.sh0) and torch.equal(out.raw_opacities, model.raw_opacities)
        assert np.array_equal(bits(model.means.cpu().numpy()), bits(means))                       # the source is untouched
        same = transform.transform_model(model, xf, inplace=True)
        assert same is model
        for g, w in zip([model.means, model.raw_quats, model.raw_scales] + ([model.shN] if rows else []), want):
            assert np.array_equal(bits(g.cpu().numpy()), bits(w))


def check_transform_cameras():
    """the moved camera sees the moved point where the camera saw the point, s times as far"""
    from lichtfeld_studio_amd import transform
    sc = render_scene()
    for m in RENDER_TRANSFORMS:
        xf = transform.similarity(m)
        s, R, t = decompose64(m)
        vm2 = transform.transform_cameras(sc["viewmats"], xf)
        x = sc["means"].astype(np.float64)
        x2 = x @ (s * R).T + t
        for v in range(2):
            p = x @ sc["viewmats"][v, :3, :3].T + sc["viewmats"][v, :3, 3]
            p2 = x2 @ vm2[v, :3, :3].T + vm2[v, :3, 3]
            assert np.abs(p2 - s * p).max() <= 1e-12 * s
            assert np.abs(vm2[v, :3, :3] @ vm2[v, :3, :3].T - np.eye(3)).max() <= 1e-14 and np.array_equal(vm2[v, 3], [0, 0, 0, 1])
