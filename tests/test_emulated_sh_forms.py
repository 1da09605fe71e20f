"""Every form of the spherical-harmonics kernels (csrc/sh.hip) as host code on the wavefront emulator, held to the float64 model of tests/sh_reference.py band by
band: the op form, the model form, the two inline-Adam forms, the multi-view forms and the size sweep - the cases and assertions of tests/test_gpu_sh_forms.py,
through the same check functions - in both builds of the lane-group sum (ds_bpermute butterfly / LFS_SH_DPP_SUM). Also here, CPU only: the truth itself
(the oracle's float64 basis is orthonormal on a fixed lattice of directions; the numpy basis behind the bounds equals the oracle's) and the measured factors
of the bounds."""
import ctypes as C
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

import sh_reference as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
CSRC = os.path.join(ROOT, "lichtfeld-studio_amd", "csrc")


def _build(out, defines):
    """tests/test_emulated_sh.py's recipe, plus adam.hip (lfs_adam_step, what the inline-Adam forms are compared with; compiled un-fused like the product's)"""
    cmd = [CLANG, "-x", "c++", "-std=c++17", "-O1", "-DLFS_EMULATE", *defines, "-fPIC", "-shared", "-ffp-contract=off", "-I" + os.path.join(HERE, "emul"),
           "-Wno-unused-value", "-Wno-unknown-attributes", os.path.join(CSRC, "sh.hip"), os.path.join(CSRC, "adam.hip"), os.path.join(HERE, "emul", "emul_stubs.cpp"),
           "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return C.CDLL(out)


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ to build the emulated kernels")
    d = tmp_path_factory.mktemp("emul_sh_forms")
    return {"bpermute": _build(str(d / "a.so"), []), "dpp": _build(str(d / "b.so"), ["-DLFS_SH_DPP_SUM"])}


@pytest.fixture(params=["bpermute", "dpp"])
def B(request, libs):
    return R.Backend(R.HostBackend(libs[request.param]))


# ---- the truth and the bounds (no kernel) ----
def test_float64_basis_of_the_oracle_is_orthonormal_on_a_fixed_lattice(oracle_mod):
    """The Gram matrix of the oracle's 25 float64 basis functions over 2000 spherical-Fibonacci directions, each weighted 4 pi / 2000, is the identity. The basis is
    read off the oracle's forward (unit coefficient in band k). A wrong constant shared by the kernels and the oracle fails here.
    Accuracy the sample allows, worked out in the test: q = the lattice's largest error over ALL monomials x^a y^b z^c of degree <= 8, whose integrals over the
    sphere are known in closed form; b_j b_k is a polynomial of degree <= 8 whose monomial coefficients sum, in absolute value, to at most L_j L_k (L_k: that sum
    for b_k, recovered by a least-squares fit of the 35 monomials of degree <= 4 to the numpy basis, which the next test pins to the oracle), so
    |Gram_jk - delta_jk| <= L_j L_k q (+ 1e-6 for the float32-rounded constants). With M = 2000: q ~ 1.1e-4, the bound is 1e-5 .. 6e-3 depending on the pair."""
    M = 2000
    d = R.fibonacci_sphere(M)
    q = 0.0
    for a, b, c in itertools.product(range(9), repeat=3):
        if a + b + c <= 8:
            exact = 0.0 if (a % 2 or b % 2 or c % 2) else 2 * math.gamma((a + 1) / 2) * math.gamma((b + 1) / 2) * math.gamma((c + 1) / 2) / math.gamma((a + b + c + 3) / 2)
            q = max(q, abs((d[:, 0] ** a * d[:, 1] ** b * d[:, 2] ** c).sum() * 4 * np.pi / M - exact))
    mono = [m for m in itertools.product(range(5), repeat=3) if sum(m) <= 4]
    P = np.random.default_rng(0).uniform(-1, 1, (400, 3))
    A = np.stack([P[:, 0] ** a * P[:, 1] ** b * P[:, 2] ** c for a, b, c in mono], 1)
    Bv = R.basis64(P[:, 0], P[:, 1], P[:, 2])
    co = np.linalg.lstsq(A, Bv, rcond=None)[0]
    assert np.abs(A @ co - Bv).max() < 1e-12
    L = np.abs(co).sum(0)
    basis = np.zeros((M, 25))
    for k0 in range(0, 25, 3):
        coeffs = np.zeros((M, 25, 3))
        for c in range(min(3, 25 - k0)):
            coeffs[:, k0 + c, c] = 1.0
        col = oracle_mod.spherical_harmonics_fwd(4, d, coeffs, None, dtype=np.float64)
        basis[:, k0:k0 + 3] = col[:, :min(3, 25 - k0)]
    err = np.abs(basis.T @ basis * (4.0 * np.pi / M) - np.eye(25))
    tol = np.outer(L, L) * q + 1e-6
    print(f"orthonormality: q = {q:.2e}, max |Gram - I| = {err.max():.2e}, largest error / bound {(err / tol).max():.3f}, bounds {tol.min():.1e} .. {tol.max():.1e}")
    assert q < 2e-4 and (err <= tol).all()


def test_numpy_basis_behind_the_bounds_is_the_oracles(oracle_mod):
    """basis64 (values) and basis_grad64 projected on the tangent plane (gradient) against the oracle's float64 forward / backward on every direction of the table"""
    m = R.master()
    d = m["dirs"].astype(np.float64)
    rng = np.random.default_rng(1)
    coeffs, v = rng.standard_normal((R.N, 25, 3)), rng.standard_normal((R.N, 3))
    nrm = np.linalg.norm(d, axis=1)
    u = d / nrm[:, None]
    b, g = R.basis64(u[:, 0], u[:, 1], u[:, 2]), R.basis_grad64(u[:, 0], u[:, 1], u[:, 2])
    col = oracle_mod.spherical_harmonics_fwd(4, d, coeffs, None, dtype=np.float64)
    np.testing.assert_allclose(np.einsum("nk,nkc->nc", b, coeffs), col, rtol=1e-12, atol=1e-13)
    _, vd = oracle_mod.spherical_harmonics_bwd(4, d, coeffs, None, v, True, dtype=np.float64)
    raw = np.einsum("nkj,nk->nj", g, np.einsum("nkc,nc->nk", coeffs, v))
    mine = (raw - (raw * u).sum(1, keepdims=True) * u) / nrm[:, None]
    np.testing.assert_allclose(mine, vd, rtol=1e-7, atol=1e-8 * np.abs(vd).max())


def test_recorded_factors_are_the_measured_ones():
    """G_*_MEASURED in sh_reference.py = measure_G() (float32 oracle against float64 oracle over the whole table; deterministic: the oracle is built un-fused), and the
    factors the tests use are four times that"""
    gf, gc, gd = R.measure_G()
    print(f"measured G_F = {gf:.3f}, G_C = {gc:.3f}, G_D = {gd:.3f}")
    for name, measured, recorded, used in (("G_F", gf, R.G_F_MEASURED, R.G_F), ("G_C", gc, R.G_C_MEASURED, R.G_C), ("G_D", gd, R.G_D_MEASURED, R.G_D)):
        assert abs(measured - recorded) <= 0.01 * recorded, (name, measured, recorded)
        assert used == 4.0 * recorded, name


def test_case_table_holds_what_it_promises():
    m = R.master()
    assert m["dirs"].shape == (R.N, 3) and 0.25 < 1 - m["vis"].mean() < 0.4 and not (m["vis"][0, :64].all() or m["vis"][0, 64:128].all())
    nrm = np.linalg.norm(m["dirs"].astype(np.float64), axis=1)
    assert nrm.min() < 2e-3 and nrm.max() > 500
    generic = np.abs(m["dirs"][:225].astype(np.float64)).min(1) > 1e-2
    for k in range(25):   # every band meets axis / pole directions and generic ones
        assert 0 < generic[k::25].sum() < 9
    assert R.equatorial(m["dirs"])[20:225:25].any(), "band 20 (the degree-4 recurrence) on an equatorial axis"
    c = R.model_case(4, 25, R.N)
    col = R.stored_colors(4, c)
    on = c["vis"][0]
    assert ((col[:225] == 0).any(1) & on[:225]).sum() >= 10, "band-isolating rows with a channel clamped to exactly 0"
    assert (col[297:309] == 0).any(1)[on[297:309]].all() and ((col[309:321] > 0) & (col[309:321] < 1e-3))[on[309:321]].all()
    assert on[297:309].sum() >= 6 and on[309:321].sum() >= 6


# ---- the forms ----
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
