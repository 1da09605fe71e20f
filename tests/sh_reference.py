"""The float64 model of the spherical-harmonics kernel family (csrc/sh.hip, csrc/lfs_sh.cuh), the rows every form is run on, the error bounds, and the
checks themselves - written once against a small `backend` (where arrays live, which library is called), so that tests/test_emulated_sh_forms.py (the kernels
as host code on the wavefront emulator) and tests/test_gpu_sh_forms.py (the MI355X) run the SAME cases through the SAME assertions.

TRUTH: oracle.spherical_harmonics_fwd / _bwd(dtype=np.float64) on the float32 inputs promoted to float64 (the oracle is pinned to the reference by the committed
goldens), and around it the model form in float64: dirs = means - campos with campos = -R^T t from the float32 view matrix, mask = all(radii > 0),
coeffs = cat(sh0, shN), colors = max(sh + 0.5, 0); the backward takes the clamp from the `colors` array HANDED TO THE KERNEL (the entry's contract), so a colour
within rounding of 0 cannot flip a decision. Multi-view: the sum over the views in float64.

ROWS (master(), n = 333; the size sweep truncates the same rows):
  0..224    band-isolating: coefficients zero except band k = row % 25, so the colour is b_k c and v_dirs is s_k grad b_k alone. 333 rows cannot hold the full
            cross 25 bands x 16 directions x channel patterns: band k takes the nine directions (3 k + j) % 16, j < 9, of directions() (+-x, +-y, +-z, the two poles
            with |x|, |y| ~ 1e-7, eight generic ones of different lengths) - nine consecutive indices modulo 16 always hold axis AND generic directions - and the
            channel pattern (one channel / another channel / all three) cycles with the row. Amplitudes of +-4 drive some channels of the model form below -0.5:
            their stored colour is exactly 0 and the expected gradient of those rows is exactly 0.
  225..296  dense randn coefficients; the eight generic directions at norms 1e-3, 1, 1e3 in turn (all 24 combinations). In three of them (NAN_ROWS) the stored bands k >= Kd are NaN: bands above the
            evaluated degree take part in nothing, and a use shows.
  297..308  clamp rows: the degree-0 term alone (sh0 = -3) drives channels below -0.5, the stored colour is exactly 0.
  309..320  colours above 0 and below 1e-3 (degree-0 term only).
  321..332  dense; row ZERO_V is visible in every view and all three of its dL/dcolour values are exactly 0.
  ZERO_ROW  (op form only) direction exactly (0,0,0): the reference yields NaN there, nothing is asserted for that row, the other 63 rows of its workgroup
            stay within their bounds.
About a third of the rows is masked out / invisible, by a hash of the row index (not aligned to 64), differently in each of the three views.
The model form's cameras are rigid motions with signed-permutation rotations and short-mantissa translations: campos is exact in float32 and in float64, so
means - campos is the same number for the kernel and the model up to ONE rounding of the subtraction and the 1e-3 rows do not measure cancellation noise.

BOUNDS (no fixed atol), eps32 = 2^-23:
  forward, per row and channel      G_F eps32 S,                   S = sum_{k<Kd} |b_k| |coeff_k| (+ 0.5 in the model form)
  v_coeffs / v_sh0 / v_shN, element G_C eps32 |b_k| |v|
  v_dirs, per row                   G_D eps32 (1/|d|) sum_{1<=k<Kd} |grad b_k| (|coeff_k| . |v|)    (grad b_k BEFORE the tangent-plane projection; the dot over the
                                    channels with absolute values: where coeff_k . v cancels, its rounding error does not)
b_k and grad b_k come from basis64() below (numpy float64; test_emulated_sh_forms.py pins it to the oracle). The factors are FOUR times the largest ratio of
|oracle(float32) - oracle(float64)| to these scales over the whole case table (measure_G(), which never runs a kernel): the float32 oracle is the reference's
arithmetic; the margin is there because the kernel sums a Gaussian's bands with a lane butterfly while the oracle sums serially. A scale of 0 means: exactly 0."""
import ctypes as C
import functools

import numpy as np

EPS32 = float(np.finfo(np.float32).eps)

# measured by measure_G() (largest |oracle32 - oracle64| / scale over TABLE + FWD_ONLY, op and model form, all three views) | what the tests use: four times that
G_F_MEASURED, G_F = 5.014, 4 * 5.014
G_C_MEASURED, G_C = 11.18, 4 * 11.18
G_D_MEASURED, G_D = 3.710, 4 * 3.710

TABLE = [(0, 1), (1, 4), (2, 9), (3, 16), (4, 25),                                                 # K = (degree + 1)^2
         (0, 4), (0, 16), (1, 9), (1, 16), (2, 16), (2, 25), (3, 25), (1, 32), (4, 32)]           # storage wider than the evaluated degree, across LPG classes
FWD_ONLY = [(3, 40)]                                                                               # the forward op accepts K > 32
ADAM_TABLE = [(1, 4), (2, 9), (3, 25), (4, 25)]
VIEWS_TABLE = [(0, 1), (1, 4), (3, 16), (4, 25), (2, 25)]
LPG_CASES = [(0, 1), (1, 4), (3, 16), (4, 25)]                                                     # one case per lane-group class 1, 4, 16, 32
SIZES = (1, 63, 64, 65, 129)
N = 333
KMAX = 40
ZERO_ROW = 77
ZERO_V = 325
NAN_ROWS = (230, 260, 290)
GUARD = 64

_AX = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1e-7, 1e-7, 1), (-1e-7, 1e-7, -1)]
# eight generic directions (normalised below) and the lengths the band-isolating rows use them at. They were picked from 30000 random candidates for being far,
# in all three views and at every length used, from the zero sets of the 25 basis functions, where b_k is a difference of nearly equal terms and NO float32 evaluation
# is accurate relative to |b_k| (which the bounds are relative to): with randn directions the measured factors are ~600 and the bounds say nothing
_GEN = [((-0.779, 0.6, 0.184), 1.0), ((-0.299, 0.918, -0.259), 2.0), ((0.593, 0.805, -0.033), 0.5), ((-0.928, -0.249, -0.278), 3.0),
        ((-0.847, -0.182, 0.499), 0.25), ((-0.124, 0.851, 0.51), 1.5), ((-0.756, 0.382, -0.532), 6.0), ((-0.46, -0.544, -0.702), 0.2)]


def directions():
    """the 16 directions of the band-isolating rows: axes, poles, the generic ones at their lengths"""
    return np.array(_AX + [tuple(s * c / np.linalg.norm(d) for c in d) for d, s in _GEN], np.float64)


_AMPL = (4.0, -4.0, 0.7, -1.3)

# world -> camera [4,4] of the three views: signed-permutation rotations (det +1, none symmetric) and translations with a few mantissa bits
_ROT = [np.array([[0, 1, 0], [0, 0, 1], [1, 0, 0]]), np.array([[0, 0, -1], [1, 0, 0], [0, -1, 0]]), np.array([[-1, 0, 0], [0, 0, 1], [0, 1, 0]])]
_TRN = [(3.75, 1.75, 2.0), (-3.0, 3.5, 3.5), (4.0, 1.0, 0.5)]


# ---- the basis in numpy float64 (Sloan, "Efficient Spherical Harmonic Evaluation", JCGT 2013; the constants as the float32 values every implementation holds) ----
def _f(v):
    return float(np.float32(v))


def basis64(x, y, z):
    """unit direction components (arrays) -> b [..., 25]"""
    x, y, z = (np.asarray(a, np.float64) for a in (x, y, z))
    b = [None] * 25
    b[0] = np.full(x.shape, _f(0.2820947917738781))
    c1 = _f(0.48860251190292)
    b[1], b[2], b[3] = -c1 * y, c1 * z, -c1 * x
    z2 = z * z
    t0B = _f(-1.092548430592079) * z
    fC1, fS1 = x * x - y * y, 2.0 * x * y
    c2 = _f(0.5462742152960395)
    b[4], b[5], b[6], b[7], b[8] = c2 * fS1, t0B * y, _f(0.9461746957575601) * z2 - _f(0.3153915652525201), t0B * x, c2 * fC1
    t0C = _f(-2.285228997322329) * z2 + _f(0.4570457994644658)
    t1B = _f(1.445305721320277) * z
    fC2, fS2 = x * fC1 - y * fS1, x * fS1 + y * fC1
    c3 = _f(-0.5900435899266435)
    b[9], b[10], b[11] = c3 * fS2, t1B * fS1, t0C * y
    b[12] = z * (_f(1.865881662950577) * z2 - _f(1.119528997770346))
    b[13], b[14], b[15] = t0C * x, t1B * fC1, c3 * fC2
    t0D = z * (_f(-4.683325804901025) * z2 + _f(2.007139630671868))
    t1C = _f(3.31161143515146) * z2 - _f(0.47308734787878)
    t2B = _f(-1.770130769779931) * z
    fC3, fS3 = x * fC2 - y * fS2, x * fS2 + y * fC2
    c4 = _f(0.6258357354491763)
    b[16], b[17], b[18], b[19] = c4 * fS3, t2B * fS2, t1C * fS1, t0D * y
    b[20] = _f(1.984313483298443) * z * b[12] - _f(1.006230589874905) * b[6]
    b[21], b[22], b[23], b[24] = t0D * x, t1C * fC1, t2B * fC2, c4 * fC3
    return np.stack(b, -1)


def basis_grad64(x, y, z):
    """-> d b / d (x, y, z) [..., 25, 3] of the polynomial above, NOT projected on the tangent plane: central differences, exact to ~1e-10 for a quartic"""
    x, y, z = (np.asarray(a, np.float64) for a in (x, y, z))
    h = 1e-6
    return np.stack([(basis64(x + h, y, z) - basis64(x - h, y, z)) / (2 * h), (basis64(x, y + h, z) - basis64(x, y - h, z)) / (2 * h),
                     (basis64(x, y, z + h) - basis64(x, y, z - h)) / (2 * h)], -1)


def fibonacci_sphere(M=2000):
    """M unit directions of the spherical Fibonacci lattice (equal-area bands in z, golden-angle steps in azimuth): no randomness, weight 4 pi / M each"""
    i = np.arange(M, dtype=np.float64)
    z = 1.0 - (2.0 * i + 1.0) / M
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    r = np.sqrt(1.0 - z * z)
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], -1)


# ---- the rows ----
def _visible(i, v):
    return ((i * 2654435761 + v * 40503 + 12345) >> 8) % 3 != 0


@functools.lru_cache(maxsize=None)
def master():
    rng = np.random.default_rng(20240)
    dirs = np.zeros((N, 3), np.float64)
    coef = np.zeros((N, KMAX, 3), np.float32)
    DIRECTIONS = directions()
    for i in range(225):
        k = i % 25
        dirs[i] = DIRECTIONS[(3 * k + i // 25) % 16]
        a, pat = _AMPL[(i // 3) % 4], i % 3
        coef[i, k] = [(a, 0, 0), (0, a, 0), (a, -0.5 * a, 0.3 * a)][pat]
    dense = list(range(225, 297)) + list(range(321, 333))
    for j, i in enumerate(dense):
        d = DIRECTIONS[8 + j % 8]
        dirs[i] = d / np.linalg.norm(d) * (1e-3, 1.0, 1e3)[j % 3]
        coef[i] = rng.standard_normal((KMAX, 3))
    for j, i in enumerate(range(297, 309)):   # the degree-0 term alone below -0.5 in one, two or three channels
        dirs[i] = DIRECTIONS[8 + j % 8]
        coef[i] = 0.1 * rng.standard_normal((KMAX, 3))
        coef[i, 0] = [(-3, 1, 1), (1, -3, -3), (-3, -3, -3)][j % 3]
    for j, i in enumerate(range(309, 321)):   # 0 < colour < 1e-3
        dirs[i] = DIRECTIONS[8 + j % 8]
        coef[i, 0] = (-0.5 + 1e-4 * (1 + (j + np.arange(3)) % 9)) / _f(0.2820947917738781)
    vis = np.array([[_visible(i, v) for i in range(N)] for v in range(3)])
    vis[:, ZERO_V] = True
    vis[0, ZERO_ROW] = True
    vmats = np.zeros((3, 4, 4), np.float32)
    for v in range(3):
        vmats[v, :3, :3], vmats[v, :3, 3], vmats[v, 3, 3] = _ROT[v], _TRN[v], 1.0
    means = (campos64(vmats[0]) + dirs).astype(np.float32)
    dirs32 = dirs.astype(np.float32)
    v_colors = rng.standard_normal((3, N, 3)).astype(np.float32)
    v_colors[:, ZERO_V] = 0.0
    bad = [(0, 4), (2, 0), (0, 0), (-1, 3)]
    radii = np.array([[(3, 5) if vis[v, i] else bad[i % 4] for i in range(N)] for v in range(3)], np.int32)
    for a in (dirs32, coef, vis, vmats, means, v_colors, radii):
        a.setflags(write=False)
    return dict(dirs=dirs32, coef=coef, vis=vis, viewmats=vmats, means=means, v_colors=v_colors, radii=radii)


def campos64(vm):
    vm = np.asarray(vm, np.float64)
    return -vm[:3, :3].T @ vm[:3, 3]


def op_dirs(n):
    d = master()["dirs"][:n].copy()
    if n > ZERO_ROW:
        d[ZERO_ROW] = 0.0
    return d


# ---- truth and scales ----
def _oracle():
    import oracle
    oracle.lib()
    return oracle


def _scales(degree, dirs, coeffs, mask, v):
    """dirs / coeffs / v float64, mask bool -> S [n,3], |b_k| [n,K] (0 for k >= Kd and masked rows), v_dirs scale [n] (without v: only the first two)"""
    Kd = (degree + 1) ** 2
    n, K = coeffs.shape[:2]
    with np.errstate(all="ignore"):
        nrm = np.linalg.norm(dirs, axis=-1)
        u = dirs / nrm[:, None] if degree >= 1 else dirs
        b = np.zeros((n, K))
        b[:, :Kd] = np.abs(basis64(u[:, 0], u[:, 1], u[:, 2]))[:, :Kd]
        b[~mask] = 0.0
        S = np.einsum("nk,nkc->nc", b[:, :Kd], np.abs(coeffs[:, :Kd]))
        if v is None:
            return S, b, None
        gn = np.linalg.norm(basis_grad64(u[:, 0], u[:, 1], u[:, 2]), axis=-1)[:, :Kd]
        sk = np.einsum("nkc,nc->nk", np.abs(coeffs[:, :Kd]), np.abs(v))   # |coeff_k| . |v|: the rounding error of a dot product scales with the magnitudes of its terms
        D = (gn[:, 1:] * sk[:, 1:]).sum(-1) / nrm if degree >= 1 else np.zeros(n)
        D = np.where(mask, D, 0.0)
    return S, b, D


def op_truth(degree, dirs, coeffs, mask, v=None, dtype=np.float64):
    """-> dict(colors, S) and with v also (v_coeffs, Sc [n,K,3], v_dirs, D). Masked rows: 0 everywhere. dtype=np.float32: the reference's arithmetic (measure_G)"""
    o = _oracle()
    n = dirs.shape[0]
    mask = np.ones(n, bool) if mask is None else np.asarray(mask, bool)
    d64, c64 = np.asarray(dirs, np.float64), np.asarray(coeffs, np.float64)
    with np.errstate(all="ignore"):
        out = dict(colors=np.asarray(o.spherical_harmonics_fwd(degree, np.asarray(dirs, dtype), np.asarray(coeffs, dtype), mask, dtype=dtype), np.float64))
        v64 = None if v is None else np.asarray(v, np.float64)
        S, b, D = _scales(degree, d64, c64, mask, v64)
        out["S"] = S
        if v is not None:
            vc, vd = o.spherical_harmonics_bwd(degree, np.asarray(dirs, dtype), np.asarray(coeffs, dtype), mask, np.asarray(v, dtype), True, dtype=dtype)
            out.update(v_coeffs=np.asarray(vc, np.float64), v_dirs=np.asarray(vd, np.float64), Sc=b[:, :, None] * np.abs(v64)[:, None, :], D=D)
    return out


def model_dirs(means, vm, dtype=np.float64):
    if dtype == np.float64:
        return np.asarray(means, np.float64) - campos64(vm)
    vm = np.asarray(vm, np.float32)   # the kernel's campos_of, in float32 (exact for these cameras)
    cp = -np.array([vm[0, c] * vm[0, 3] + vm[1, c] * vm[1, 3] + vm[2, c] * vm[2, 3] for c in range(3)], np.float32)
    return np.asarray(means, np.float32) - cp


def model_fwd_truth(degree, means, vm, sh0, shN, radii, dtype=np.float64):
    """-> dict(colors = max(sh + 0.5, 0) [0.5 for invisible rows], S (+ 0.5), mask, dirs, coeffs)"""
    coeffs = np.concatenate([sh0.reshape(-1, 1, 3), shN.reshape(sh0.shape[0], -1, 3)], 1)
    mask = (np.asarray(radii) > 0).all(-1)
    dirs = model_dirs(means, vm, dtype)
    t = op_truth(degree, dirs, coeffs, mask, None, dtype)
    sh = t["colors"] if dtype == np.float64 else (t["colors"].astype(np.float32) + np.float32(0.5)).astype(np.float64) - 0.5   # (float32: the + 0.5 rounds too)
    return dict(colors=np.maximum(sh + 0.5, 0.0), S=t["S"] + 0.5, mask=mask, dirs=dirs, coeffs=coeffs)


def model_bwd_truth(degree, means, vm, sh0, shN, radii, colors_stored, v_colors, dtype=np.float64):
    """-> dict(v_coeffs [n,K,3], Sc, v_dirs [n,3], D, mask): the clamp is read off the colours handed to the kernel"""
    f = model_fwd_truth(degree, means, vm, sh0, shN, radii, dtype)
    v = np.where(np.asarray(colors_stored) > 0, np.asarray(v_colors, np.float64), 0.0)
    t = op_truth(degree, f["dirs"], f["coeffs"], f["mask"], v.astype(dtype), dtype)
    t["mask"] = f["mask"]
    return t


def coeffs_for(degree, K, n):
    """the master rows cut to [n, K, 3]; in NAN_ROWS the bands k >= Kd, which no form may use, are NaN"""
    c = master()["coef"][:n, :K].copy()
    for i in NAN_ROWS:
        if i < n:
            c[i, (degree + 1) ** 2:] = np.nan
    return c


def model_case(degree, K, n):
    m, cf = master(), coeffs_for(degree, K, n)
    return dict(means=m["means"][:n], sh0=np.ascontiguousarray(cf[:, :1]), shN=np.ascontiguousarray(cf[:, 1:]), viewmats=m["viewmats"],
                radii=m["radii"][:, :n], vis=m["vis"][:, :n], v_colors=m["v_colors"][:, :n])


def stored_colors(degree, c, view=0, radii=None):
    """the float64 model's colours rounded to float32: what the backward tests hand to the kernels as `colors`"""
    return model_fwd_truth(degree, c["means"], c["viewmats"][view], c["sh0"], c["shN"], c["radii"][view] if radii is None else radii)["colors"].astype(np.float32)


def measure_G():
    """-> (G_F, G_C, G_D) measured: max |oracle(float32) - oracle(float64)| / scale over the whole case table, op form and model form (all views). No kernel runs."""
    m = master()
    g = [0.0, 0.0, 0.0]

    def take(i, a32, a64, scale, rows):
        with np.errstate(all="ignore"):
            err = np.abs(a32 - a64)[rows]
            sc = scale[rows] * EPS32
            assert not (err[sc == 0] != 0).any(), "the float32 oracle is not exactly 0 where the scale is 0"
            r = err[sc > 0] / sc[sc > 0]
        if r.size:
            g[i] = max(g[i], float(r.max()))

    for degree, K in TABLE + FWD_ONLY:
        coeffs, mask, v = coeffs_for(degree, K, N), m["vis"][0], m["v_colors"][0]
        dirs = op_dirs(N)
        rows = np.ones(N, bool); rows[ZERO_ROW] = False
        a, b = op_truth(degree, dirs, coeffs, None, v, np.float32), op_truth(degree, dirs, coeffs, None, v, np.float64)   # (every row: the masked runs see a subset)
        take(0, a["colors"], b["colors"], b["S"], rows)
        take(1, a["v_coeffs"], b["v_coeffs"], b["Sc"], rows)
        take(2, a["v_dirs"], b["v_dirs"], np.repeat(b["D"][:, None], 3, 1), rows)
        c = model_case(degree, K, N)
        for view in range(3):
            col = stored_colors(degree, c, view, np.full((N, 2), 2, np.int32))
            args = (degree, c["means"], c["viewmats"][view], c["sh0"], c["shN"], np.full((N, 2), 2, np.int32))   # (every Gaussian visible)
            fa, fb = model_fwd_truth(*args, np.float32), model_fwd_truth(*args, np.float64)
            take(0, fa["colors"], fb["colors"], fb["S"], fb["mask"])
            a, b = model_bwd_truth(*args, col, c["v_colors"][view], np.float32), model_bwd_truth(*args, col, c["v_colors"][view], np.float64)
            take(1, a["v_coeffs"], b["v_coeffs"], b["Sc"], np.ones(N, bool))
            take(2, a["v_dirs"], b["v_dirs"], np.repeat(b["D"][:, None], 3, 1), np.ones(N, bool))
    return tuple(g)


# At a direction that is exactly +-x or +-y the normalisation is exact (|d| = 1), every coordinate is 0 or +-1, and every basis value is 0, a float32 constant or its
# negative - except b_20 = 1.984 z b_12 - 1.006 b_6 = -(1.006... x (-0.3153...)), ONE rounded product. One more rounding for b_k v (or b_k c: a band-isolating row's
# colour is that one term plus exact zeros) makes two half-ulps: |error| <= 2 x eps32/2 x |b_k| |v|, and 1 % on top for the second-order term. A last-digit change of
# a constant of the degree-4 recurrence (5 eps32 on 1.00623...) is four times that.
EQUATORIAL = 1.01


def equatorial(dirs):
    d = np.asarray(dirs)
    return (d[:, 2] == 0) & (((np.abs(d[:, 0]) == 1) & (d[:, 1] == 0)) | ((np.abs(d[:, 1]) == 1) & (d[:, 0] == 0)))


# ---- comparing ----
def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    """float32 arrays equal bit for bit; +0 / -0 and two NaNs count as equal (a sum that starts from +0 cannot return -0, a store can)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | ((a == 0) & (b == 0)) | (np.isnan(a) & np.isnan(b))).all())


def assert_same(what, a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = ~((bits(a) == bits(b)) | ((a == 0) & (b == 0)) | (np.isnan(a) & np.isnan(b)))
    assert not bad.any(), f"{what}: {int(bad.sum())} elements differ, first at {tuple(np.argwhere(bad)[0])}: {a[bad][0]!r} vs {b[bad][0]!r}"


def assert_kept(what, got, before, where=None):
    """the elements selected by `where` (all: None) still hold the bits they were filled with (-0 and NaN payloads included)"""
    g, b = bits(got), bits(before)
    bad = (g != b) if where is None else ((g != b) & np.broadcast_to(where, g.shape))
    assert not bad.any(), f"{what}: {int(bad.sum())} elements that must keep their bits changed, first at {tuple(np.argwhere(bad)[0])}"


def assert_within(what, got, want, bound, rows=None):
    """|got - want| <= bound element-wise (bound 0: equal, and then -0 == +0); rows: bool [n] of the rows that are asserted at all"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    bound = np.broadcast_to(np.asarray(bound, np.float64), want.shape)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    sel = np.ones(want.shape, bool) if rows is None else np.broadcast_to(np.asarray(rows).reshape((-1,) + (1,) * (want.ndim - 1)), want.shape)
    with np.errstate(all="ignore"):
        err = np.abs(got - want)
        bad = sel & ~(err <= bound)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        with np.errstate(all="ignore"):
            worst = float(np.nanmax(np.where(bad & (bound > 0), err / bound, 0.0)))
        raise AssertionError(f"{what}: {int(bad.sum())} elements out of bound, first at {i}: got {got[i]!r}, float64 model {want[i]!r}, bound {bound[i]:.3e}; "
                             f"worst error / bound {worst:.2f}")


def pattern(shape, salt=0):
    """a known float32 pattern for outputs that are added to or must survive: mixed signs and sizes, every fifth element -0.0 (x + 0 turns it into +0)"""
    i = np.arange(int(np.prod(shape)), dtype=np.int64) + salt
    p = (((i * 37) % 1013) / 64.0 - 7.0).astype(np.float32)
    p[i % 5 == 0] = -0.0
    return p.reshape(shape)


# ---- backends: where the arrays live ----
class HostBackend:
    """the emulated kernels: they run on host memory, a numpy array IS the device buffer"""
    def __init__(self, lib):
        self.lib, self.stream = lib, None

    def raw(self, nbytes):
        return np.zeros(nbytes, np.uint8)

    def addr(self, h):
        return h.ctypes.data

    def view(self, raw, start, arr):
        v = raw[start:start + arr.nbytes].view(arr.dtype).reshape(arr.shape)
        v[...] = arr
        return v

    def ptr(self, h):
        return None if h is None else C.c_void_p(h.ctypes.data)

    def host(self, h):
        return np.array(h, copy=True)


class Backend:
    """what the checks need on top of one of the two: upload (optionally at a chosen misalignment), outputs with guard rows, the call itself"""
    def __init__(self, impl):
        self.impl, self.lib, self.stream = impl, impl.lib, impl.stream
        self._guards, self._keep = [], []

    def up(self, arr, misalign=0):
        """a device copy of an array whose first byte sits `misalign` floats after a 16-byte boundary"""
        arr = np.ascontiguousarray(arr)
        raw = self.impl.raw(arr.nbytes + 32)
        start = (4 * misalign - self.impl.addr(raw)) % 16
        h = self.impl.view(raw, start, arr)
        self._keep.append((raw, h))   # (a pointer handed to ctypes holds no reference: alive until done())
        return h

    def out(self, fill):
        """an output tensor pre-filled with `fill` (array), followed by GUARD rows of a pattern that must come back untouched (check with done())"""
        fill = np.ascontiguousarray(fill, np.float32)
        row = fill.shape[1:]
        guard = (123456.0 + np.arange(GUARD * int(np.prod(row, dtype=np.int64)), dtype=np.float32)).reshape((GUARD,) + row)
        h = self.up(np.concatenate([fill, guard], 0))
        self._guards.append((h, fill.shape[0], guard))
        return h

    def get(self, h):
        a = self.impl.host(h)
        for g, rows, _ in self._guards:
            if g is h:
                return a[:rows]
        return a

    def done(self):
        for h, rows, guard in self._guards:
            assert_kept("guard rows after an output", self.impl.host(h)[rows:], guard)
        self._guards, self._keep = [], []

    def p(self, h):
        return self.impl.ptr(h)

    def call(self, name, *args):
        rc = getattr(self.lib, name)(*args, self.stream)
        assert rc == 0, (name, rc)


u32, i32, f32 = C.c_uint32, C.c_int, C.c_float


def _nan(shape):
    return np.full(shape, np.nan, np.float32)


def adam_scalars(step):
    lr, b1, b2, eps = 2.5e-3, 0.9, 0.999, 1e-15
    return [np.float32(x) for x in (lr, b1, b2, eps, 1.0 / (1.0 - b1 ** step), 1.0 / np.sqrt(1.0 - b2 ** step))]


def _adam_step(B, p, m, v, g, count, sc):
    B.call("lfs_adam_step", B.p(p), B.p(m), B.p(v), B.p(g), C.c_int64(count), *[f32(float(x)) for x in sc])


# ---- (a) the op form ----
def check_op(B, degree, K, n=N, masks=True, want_dirs=True):
    m = master()
    dirs, coeffs, v = op_dirs(n), coeffs_for(degree, K, n), m["v_colors"][0, :n]
    mask = m["vis"][0, :n] if masks else None
    rows = np.ones(n, bool)
    if n > ZERO_ROW:
        rows[ZERO_ROW] = False
    t = op_truth(degree, dirs, coeffs, mask, v)
    on = np.ones(n, bool) if mask is None else mask
    d_dirs, d_coeffs, d_v = B.up(dirs), B.up(coeffs), B.up(v)
    d_mask = None if mask is None else B.up(mask.astype(np.uint8))
    colors = B.out(_nan((n, 3)))
    B.call("lfs_spherical_harmonics_fwd", u32(n), u32(K), u32(degree), B.p(d_dirs), B.p(d_coeffs), B.p(d_mask), B.p(colors))
    got = B.get(colors)
    assert_within("colors", got, t["colors"], G_F * EPS32 * t["S"], rows)
    assert (got[~on] == 0).all(), "colours of masked rows are not exactly 0"
    eq = equatorial(dirs) & rows
    assert_within("colors of band-isolating rows on the equatorial axes", got, t["colors"], EQUATORIAL * EPS32 * t["S"], eq & (np.arange(n) < 225))
    if K <= 32:
        v_coeffs, v_dirs = B.out(_nan((n, K, 3))), B.out(_nan((n, 3))) if want_dirs else None
        B.call("lfs_spherical_harmonics_bwd", u32(n), u32(K), u32(degree), B.p(d_dirs), B.p(d_coeffs), B.p(d_mask), B.p(d_v), B.p(v_coeffs), B.p(v_dirs))
        got = B.get(v_coeffs)
        assert_within("v_coeffs", got, t["v_coeffs"], G_C * EPS32 * t["Sc"], rows)
        assert_within("v_coeffs on the equatorial axes", got, t["v_coeffs"], EQUATORIAL * EPS32 * t["Sc"], eq)
        assert (got[~on] == 0).all() and (got[rows][:, (degree + 1) ** 2:] == 0).all(), "v_coeffs of masked rows / of bands k >= Kd are not exactly 0 (FULLY written)"
        if want_dirs:
            got = B.get(v_dirs)
            assert_within("v_dirs", got, t["v_dirs"], G_D * EPS32 * t["D"][:, None], rows)
            assert (got[~on] == 0).all(), "v_dirs of masked rows are not exactly 0"
    B.done()


# ---- (b) the model form, one view ----
def _model_device(B, c, view=0, radii=None):
    r = c["radii"][view] if radii is None else radii
    return dict(means=B.up(c["means"]), vm=B.up(c["viewmats"][view]), sh0=B.up(c["sh0"]), shN=B.up(c["shN"]) if c["shN"].size else None, radii=B.up(r))


def run_model_bwd(B, degree, K, n, c, d, colors, v_colors, accumulate, fill_sh0, fill_shN, fill_means):
    """lfs_sh_model_bwd -> (v_sh0, v_shN, v_means) as numpy; fills are the arrays the outputs hold before the call"""
    o0, oN, om = B.out(fill_sh0), (B.out(fill_shN) if K > 1 else None), B.out(fill_means)
    B.call("lfs_sh_model_bwd", u32(n), u32(K), u32(degree), B.p(d["means"]), B.p(d["vm"]), B.p(d["sh0"]), B.p(d["shN"]), B.p(d["radii"]), B.p(B.up(colors)),
           B.p(B.up(v_colors)), i32(accumulate), B.p(o0), B.p(oN), B.p(om))
    return B.get(o0), (B.get(oN) if K > 1 else np.zeros((n, 0, 3), np.float32)), B.get(om)


def check_model(B, degree, K, n=N, all_visible=False):
    c = model_case(degree, K, n)
    radii = np.full((n, 2), 2, np.int32) if all_visible else c["radii"][0]
    d = _model_device(B, c, 0, radii)
    f = model_fwd_truth(degree, c["means"], c["viewmats"][0], c["sh0"], c["shN"], radii)
    on, Kd = f["mask"], (degree + 1) ** 2
    colors = B.out(_nan((n, 3)))
    B.call("lfs_sh_model_fwd", u32(n), u32(K), u32(degree), B.p(d["means"]), B.p(d["vm"]), B.p(d["sh0"]), B.p(d["shN"]), B.p(d["radii"]), B.p(colors))
    got = B.get(colors)
    assert_within("model colors", got, f["colors"], G_F * EPS32 * f["S"])
    assert (got[~on] == 0.5).all(), "colours of invisible Gaussians are not exactly clamp(0 + 0.5)"
    stored = f["colors"].astype(np.float32)
    v = c["v_colors"][0]
    t = model_bwd_truth(degree, c["means"], c["viewmats"][0], c["sh0"], c["shN"], radii, stored, v)
    bc, bd = G_C * EPS32 * t["Sc"], G_D * EPS32 * t["D"][:, None]
    live = on[:, None, None] & (np.arange(K) < Kd)[None, :, None]     # the elements of v_coeffs a visible Gaussian's evaluated bands own
    moved = on[:, None] & (degree >= 1)                               # the rows of v_means that are added to
    # accumulate = 0 into NaN
    pm = pattern((n, 3), 5)
    g0, gN, gm = run_model_bwd(B, degree, K, n, c, d, stored, v, 0, _nan((n, 1, 3)), _nan((n, K - 1, 3)), pm)
    got = np.concatenate([g0, gN], 1)
    assert_within("v_sh0 | v_shN (accumulate = 0)", got, t["v_coeffs"], bc)
    assert (got[~np.broadcast_to(live, got.shape)] == 0).all(), "accumulate = 0 must write 0 for invisible Gaussians and bands k >= Kd"
    want = pm.astype(np.float64) + t["v_dirs"]
    assert_within("v_means", gm, want, bd + EPS32 * np.abs(want), on if degree >= 1 else np.zeros(n, bool))
    assert_kept("v_means of invisible rows / at degree 0", gm, pm, ~np.broadcast_to(moved, gm.shape))
    # accumulate = 1 into a pattern
    p0, pN = pattern((n, 1, 3), 1), pattern((n, K - 1, 3), 2)
    a0, aN, am = run_model_bwd(B, degree, K, n, c, d, stored, v, 1, p0, pN, pm)
    got, pat = np.concatenate([a0, aN], 1), np.concatenate([p0, pN], 1)
    want = pat.astype(np.float64) + t["v_coeffs"]
    assert_kept("v_sh0 | v_shN of invisible Gaussians and bands k >= Kd (accumulate = 1)", got, pat, ~np.broadcast_to(live, got.shape))
    assert_within("v_sh0 | v_shN (accumulate = 1)", np.where(live, got, 0), np.where(live, want, 0), np.where(live, bc + EPS32 * np.abs(want), 0))
    assert_same("v_means does not depend on accumulate", am, gm)
    B.done()
    return t


# ---- (c) lfs_sh_model_bwd_adam = (b) + lfs_adam_step on shN, bit for bit, two chained steps ----
def check_bwd_adam(B, degree, K, n=65):
    c = model_case(degree, K, n)
    stored, v = stored_colors(degree, c), c["v_colors"][0]
    shN_a, shN_b = c["shN"].copy(), c["shN"].copy()
    m_a = m_b = 0.01 * pattern(c["shN"].shape, 3)
    q_a = q_b = np.abs(0.001 * pattern(c["shN"].shape, 4))
    vm_a = vm_b = pattern((n, 3), 6)
    for step in (1, 2):
        sc = adam_scalars(step)
        # the separate kernels
        ca = dict(c, shN=shN_a)
        d = _model_device(B, ca)
        g0, gN, vm_a = run_model_bwd(B, degree, K, n, ca, d, stored, v, 0, _nan((n, 1, 3)), _nan((n, K - 1, 3)), vm_a)
        hp, hm, hq = d["shN"], B.up(m_a), B.up(q_a)
        _adam_step(B, hp, hm, hq, B.up(gN), gN.size, sc)
        shN_a, m_a, q_a = B.get(hp), B.get(hm), B.get(hq)
        # one kernel
        d = _model_device(B, dict(c, shN=shN_b))
        o0, om, hm, hq = B.out(_nan((n, 1, 3))), B.out(vm_b), B.up(m_b), B.up(q_b)
        B.call("lfs_sh_model_bwd_adam", u32(n), u32(K), u32(degree), B.p(d["means"]), B.p(d["vm"]), B.p(d["sh0"]), B.p(d["shN"]), B.p(d["radii"]), B.p(B.up(stored)),
               B.p(B.up(v)), B.p(o0), B.p(om), B.p(hm), B.p(hq), *[f32(float(x)) for x in sc])
        shN_b, m_b, q_b, vm_b = B.get(d["shN"]), B.get(hm), B.get(hq), B.get(om)
        for what, x, y in (("shN", shN_b, shN_a), ("exp_avg", m_b, m_a), ("exp_avg_sq", q_b, q_a), ("v_sh0", B.get(o0), g0), ("v_means", vm_b, vm_a)):
            assert_same(f"step {step}: {what} (inline Adam vs lfs_sh_model_bwd + lfs_adam_step)", x, y)
        B.done()
    assert not same_bits(shN_a, c["shN"]), "the two steps changed nothing"


# ---- (d) lfs_sh_model_bwd_adam_all: accumulator rows, the float4 load and its fallback, dirs_store, Adam on sh0 and shN ----
def check_bwd_adam_all(B, degree, K, n=N):
    c = model_case(degree, K, n)
    stored, v, on = stored_colors(degree, c), c["v_colors"][0], c["vis"][0]
    acc = _nan((n, 16))
    acc[:, 13:] = v
    mom = [0.01 * pattern(c["sh0"].shape, 7), np.abs(0.001 * pattern(c["sh0"].shape, 8)), 0.01 * pattern(c["shN"].shape, 3), np.abs(0.001 * pattern(c["shN"].shape, 4))]
    sc0, scN = adam_scalars(3), adam_scalars(5)
    # the separate kernels: (b) from a zero v_means, then lfs_adam_step on sh0 and on shN
    d = _model_device(B, c)
    g0, gN, gm = run_model_bwd(B, degree, K, n, c, d, stored, v, 0, _nan((n, 1, 3)), _nan((n, K - 1, 3)), np.zeros((n, 3), np.float32))
    hm = [B.up(x) for x in mom]
    _adam_step(B, d["sh0"], hm[0], hm[1], B.up(g0), g0.size, sc0)
    _adam_step(B, d["shN"], hm[2], hm[3], B.up(gN), gN.size, scN)
    want = [B.get(d["sh0"]), B.get(d["shN"])] + [B.get(h) for h in hm]
    res = []
    for misalign in (0, 1):   # 16-byte-aligned rows: one float4 load per Gaussian; one float into a larger buffer: three dword loads
        d = _model_device(B, c)
        hm = [B.up(x) for x in mom]
        h_acc = B.up(acc, misalign=misalign)
        assert (B.impl.addr(h_acc) % 16 == 0) == (misalign == 0)
        vd = B.out(_nan((n, 3)))
        B.call("lfs_sh_model_bwd_adam_all", u32(n), u32(K), u32(degree), B.p(d["means"]), B.p(d["vm"]), B.p(d["sh0"]), B.p(d["shN"]), B.p(d["radii"]), B.p(B.up(stored)),
               B.p(h_acc), B.p(vd), B.p(hm[0]), B.p(hm[1]), (C.c_float * 6)(*[float(x) for x in sc0]), B.p(hm[2]), B.p(hm[3]), (C.c_float * 6)(*[float(x) for x in scN]))
        got = [B.get(d["sh0"]), B.get(d["shN"])] + [B.get(h) for h in hm]
        for what, x, y in zip(("sh0", "shN", "sh0 exp_avg", "sh0 exp_avg_sq", "shN exp_avg", "shN exp_avg_sq"), got, want):
            assert_same(f"{what} (all-inline vs lfs_sh_model_bwd + lfs_adam_step, accumulator rows {'aligned' if not misalign else 'one float off'})", x, y)
        gvd = B.get(vd)
        assert not np.isnan(gvd).any(), "v_dirs is not fully written"
        assert (gvd[~on] == 0).all(), "v_dirs of invisible Gaussians is not exactly 0"
        assert_same("v_dirs (written) vs the v_means increment of lfs_sh_model_bwd from zero", gvd, gm)
        res.append(got + [gvd])
        B.done()
    for x, y in zip(*res):
        assert_same("float4 path vs three-dword fallback", x, y)


# ---- (e) the multi-view forms ----
def views_case(degree, K, n, V, stride):
    """per-view operands [V, stride, ...]: rows n.. of a view hold what must never be used (visible radii, NaN gradients)"""
    c = model_case(degree, K, n)
    radii = np.full((V, stride, 2), 7, np.int32)
    radii[:, :n] = c["radii"][:V]
    v_colors = _nan((V, stride, 3))
    v_colors[:, :n] = c["v_colors"][:V]
    return c, radii, v_colors


def views_truth(degree, c, V, colors_stored, v_colors):
    """sum over the views in float64 -> (v_coeffs, sum of Sc, v_dirs, sum of D)"""
    n = c["means"].shape[0]
    ts = [model_bwd_truth(degree, c["means"], c["viewmats"][w], c["sh0"], c["shN"], c["radii"][w], colors_stored[w, :n], v_colors[w, :n]) for w in range(V)]
    return tuple(sum(t[k] for t in ts) for k in ("v_coeffs", "Sc", "v_dirs", "D"))


def run_bwd_views(B, degree, K, n, V, stride, c, shN, radii, colors, v_colors, accumulate, fill_sh0, fill_shN, fill_means, adam=None):
    """lfs_sh_model_bwd_views -> (v_sh0, v_shN | None, v_means[, shN, exp_avg, exp_avg_sq]); fill_shN None: v_shN = NULL"""
    h_shN = B.up(shN) if K > 1 else None
    o0, oN, om = B.out(fill_sh0), (B.out(fill_shN) if fill_shN is not None and K > 1 else None), B.out(fill_means)
    hm, hq, sc = (B.up(adam[0]), B.up(adam[1]), adam[2]) if adam else (None, None, [0.0] * 6)
    B.call("lfs_sh_model_bwd_views", u32(n), u32(K), u32(degree), u32(V), u32(stride), B.p(B.up(c["means"])), B.p(B.up(c["viewmats"][:V])), B.p(B.up(c["sh0"])), B.p(h_shN),
           B.p(None if radii is None else B.up(radii)), B.p(None if colors is None else B.up(colors)), B.p(B.up(v_colors)), i32(accumulate), B.p(o0), B.p(oN), B.p(om),
           B.p(hm), B.p(hq), *[f32(float(x)) for x in sc])
    out = (B.get(o0), None if oN is None else B.get(oN), B.get(om))
    return out + ((B.get(h_shN), B.get(hm), B.get(hq)) if adam else ())


def check_views(B, degree, K, V, pad, n=N):
    stride, Kd = n + pad, (degree + 1) ** 2
    c, radii, v_colors = views_case(degree, K, n, V, stride)
    # forward
    fill = pattern((V, stride, 3), 9)
    colors = B.out(fill.reshape(V * stride, 3))
    B.call("lfs_sh_model_fwd_views", u32(n), u32(K), u32(degree), u32(V), u32(stride), B.p(B.up(c["means"])), B.p(B.up(c["viewmats"][:V])), B.p(B.up(c["sh0"])),
           B.p(B.up(c["shN"]) if K > 1 else None), B.p(B.up(radii)), B.p(colors))
    got = B.get(colors).reshape(V, stride, 3)
    stored = np.ones((V, stride, 3), np.float32)
    for w in range(V):
        f = model_fwd_truth(degree, c["means"], c["viewmats"][w], c["sh0"], c["shN"], c["radii"][w])
        assert_within(f"colors of view {w}", got[w, :n], f["colors"], G_F * EPS32 * f["S"])
        stored[w, :n] = f["colors"]
    assert_kept("rows n.. of every view of colors", got[:, n:], fill[:, n:])
    # backward against the float64 model summed over the views; the bound scales with the number of views
    vc, Sc, vd, D = views_truth(degree, c, V, stored, v_colors)
    bc, bd = V * G_C * EPS32 * Sc, V * G_D * EPS32 * D[:, None]
    pm, p0, pN = pattern((n, 3), 5), pattern((n, 1, 3), 1), pattern((n, K - 1, 3), 2)
    g0, gN, gm = run_bwd_views(B, degree, K, n, V, stride, c, c["shN"], radii, stored, v_colors, 0, _nan((n, 1, 3)), _nan((n, K - 1, 3)), pm)
    got = got0 = np.concatenate([g0, gN], 1) if K > 1 else g0
    assert_within("views: v_sh0 | v_shN (accumulate = 0)", got, vc, bc)
    assert (got[:, Kd:] == 0).all(), "bands k >= Kd are not exactly 0"
    want = pm.astype(np.float64) + vd
    if degree >= 1:
        assert_within("views: v_means", gm, want, bd + V * EPS32 * np.abs(want))
    else:
        assert_kept("views: v_means at degree 0", gm, pm)
    a0, aN, am = run_bwd_views(B, degree, K, n, V, stride, c, c["shN"], radii, stored, v_colors, 1, p0, pN, pm)
    got, pat = (np.concatenate([a0, aN], 1), np.concatenate([p0, pN], 1)) if K > 1 else (a0, p0)
    want = pat.astype(np.float64) + vc
    assert_within("views: v_sh0 | v_shN (accumulate = 1)", got, want, bc + EPS32 * np.abs(want))
    assert_same("views: v_means does not depend on accumulate", am, gm)
    # v_shN = NULL: nothing written for it, nothing else changes
    n0, nN, nm = run_bwd_views(B, degree, K, n, V, stride, c, c["shN"], radii, stored, v_colors, 0, _nan((n, 1, 3)), None, pm)
    assert nN is None
    assert_same("views: v_sh0 with v_shN = NULL", n0, g0)
    assert_same("views: v_means with v_shN = NULL", nm, gm)
    # radii = colors = NULL: dL/dcolour rows arrive masked by visibility and clamp
    vis = (radii > 0).all(-1)
    masked = np.where(vis[:, :, None] & (stored > 0), v_colors, np.float32(0)).astype(np.float32)
    masked[:, n:] = np.nan
    m0, mN, mm = run_bwd_views(B, degree, K, n, V, stride, c, c["shN"], None, None, masked, 0, _nan((n, 1, 3)), _nan((n, K - 1, 3)), pm)
    assert_same("views: v_sh0, pre-masked rows vs radii / colors", m0, g0)
    if K > 1:
        assert_same("views: v_shN, pre-masked rows vs radii / colors", mN, gN)
    assert_same("views: v_means, pre-masked rows vs radii / colors", mm, gm)
    if n > ZERO_V:
        assert vis[:, ZERO_V].all() and (v_colors[:, ZERO_V] == 0).all()
        assert (got0[ZERO_V] == 0).all() and same_bits(gm[ZERO_V], pm[ZERO_V]), "a visible Gaussian with dL/dcolour = 0 got a gradient"
    B.done()


def check_views_adam(B, degree=4, K=25, V=3, pad=7, n=N):
    """the inline-Adam form against the stored-gradient form + lfs_adam_step, bit for bit"""
    stride = n + pad
    c, radii, v_colors = views_case(degree, K, n, V, stride)
    stored = np.ones((V, stride, 3), np.float32)
    for w in range(V):
        stored[w, :n] = stored_colors(degree, c, w)
    pm, sc = pattern((n, 3), 5), adam_scalars(2)
    m, q = 0.01 * pattern(c["shN"].shape, 3), np.abs(0.001 * pattern(c["shN"].shape, 4))
    g0, gN, gm = run_bwd_views(B, degree, K, n, V, stride, c, c["shN"], radii, stored, v_colors, 0, _nan((n, 1, 3)), _nan((n, K - 1, 3)), pm)
    hp, hm, hq = B.up(c["shN"]), B.up(m), B.up(q)
    _adam_step(B, hp, hm, hq, B.up(gN), gN.size, sc)
    a0, aN, am, shN, m2, q2 = run_bwd_views(B, degree, K, n, V, stride, c, c["shN"], radii, stored, v_colors, 0, _nan((n, 1, 3)), None, pm, adam=(m, q, sc))
    for what, x, y in (("shN", shN, B.get(hp)), ("exp_avg", m2, B.get(hm)), ("exp_avg_sq", q2, B.get(hq)), ("v_sh0", a0, g0), ("v_means", am, gm)):
        assert_same(f"views, inline Adam vs stored gradient + lfs_adam_step: {what}", x, y)
    B.done()
