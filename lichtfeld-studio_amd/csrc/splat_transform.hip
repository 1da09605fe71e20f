// Scene transform: move a splat by a similarity x' = s R x + t - means, orientations, log-scales and the view-dependent colour. The reference's
// SplatData::transform (src/core/splat_data.cpp:288-384) moves the first three and leaves shN alone, so after a rotation every highlight stays where the OLD world
// frame had it; here band l of every colour channel is multiplied by the (2l+1)-square matrix M_l(R) of the real spherical harmonics in the coefficient order and
// signs of sh_basis (lfs_sh.cuh): sum_k (M a)_k Y_k(d) = sum_k a_k Y_k(R^T d). sh0 and the opacities are invariant.
//
// Host part (no GPU): lfs_sh_rotation_matrices fits M_l over 64 fixed directions in float64 (A_l M = B_l, A = Y_l(d_j), B = Y_l(R^T d_j), normal equations: A^T A is
// within a few per cent of (64 / 4 pi) I, so nothing is lost by squaring), lfs_splat_transform_from_matrix decomposes a 4x4, refuses what is not a proper similarity and
// fills the float32 record the kernels take.
//
// Device part, two streaming kernels: the record is a BY-VALUE kernel argument, every lane uses the same 182 dwords, so they arrive as scalar loads from the kernarg
// segment and enter the VALU as SGPR operands (the camera idiom of filter3d.hip). st_geom_kernel: one lane per Gaussian (40 of the 236 bytes). st_sh_kernel: a
// Gaussian's shN row is 3 * shN_rows floats with the channels interleaved, 180 bytes at degree 3 - a lane reading its own row would stride by that. A block instead
// stages up to 128 whole rows through LDS with coalesced loads (16-byte ones where the pointers allow), lane g then rotates row g in LDS (row stride odd: W | 1 words, every
// lane its own bank), and after a second barrier the tile goes back out with coalesced stores. Every global read of a tile precedes the first barrier and every write
// follows the second, tiles are disjoint: in place (out == in) is safe. -ffp-contract=off: the arithmetic below is what a float32 host model repeats bit for bit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/lfs_gsplat.h"

static_assert(sizeof(lfs_splat_transform) == 728, "the ctypes mirror (capi.py: SplatTransformStruct) is laid out by hand");

namespace lfs {
namespace st {

// ---- host: the basis in float64 (Sloan, JCGT 2013; constants from their closed forms, not from the float32 literals of lfs_sh.cuh) ----------------------------
static void basis64(const double x, const double y, const double z, double* b) {
    const double rpi = 1.0 / sqrt(M_PI);
    b[0] = 0.5 * rpi;
    const double c1 = 0.5 * sqrt(3.0) * rpi;
    b[1] = -c1 * y; b[2] = c1 * z; b[3] = -c1 * x;
    const double z2 = z * z;
    const double k15 = sqrt(15.0) * rpi, k5 = sqrt(5.0) * rpi;
    const double t0B = -0.5 * k15 * z;
    const double fC1 = x * x - y * y, fS1 = 2.0 * x * y;
    const double c2 = 0.25 * k15;
    b[4] = c2 * fS1; b[5] = t0B * y; b[6] = 0.75 * k5 * z2 - 0.25 * k5; b[7] = t0B * x; b[8] = c2 * fC1;
    const double k21 = sqrt(21.0 / (32.0 * M_PI));
    const double t0C = -5.0 * k21 * z2 + k21;
    const double t1B = 0.25 * sqrt(105.0) * rpi * z;
    const double fC2 = x * fC1 - y * fS1, fS2 = x * fS1 + y * fC1;
    const double c3 = -0.25 * sqrt(35.0 / (2.0 * M_PI));
    const double k7 = 0.25 * sqrt(7.0) * rpi;
    b[9] = c3 * fS2; b[10] = t1B * fS1; b[11] = t0C * y;
    b[12] = z * (5.0 * k7 * z2 - 3.0 * k7);
    b[13] = t0C * x; b[14] = t1B * fC1; b[15] = c3 * fC2;
    const double k41 = 0.75 * sqrt(5.0 / (2.0 * M_PI)), k42 = 0.375 * k5;
    const double t0D = z * (-7.0 * k41 * z2 + 3.0 * k41);
    const double t1C = 7.0 * k42 * z2 - k42;
    const double t2B = -0.75 * sqrt(35.0 / (2.0 * M_PI)) * z;
    const double fC3 = x * fC2 - y * fS2, fS3 = x * fS2 + y * fC2;
    const double c4 = 0.1875 * sqrt(35.0) * rpi;
    b[16] = c4 * fS3; b[17] = t2B * fS2; b[18] = t1C * fS1; b[19] = t0D * y;
    b[20] = 0.25 * sqrt(63.0) * z * b[12] - (9.0 / (4.0 * sqrt(5.0))) * b[6];
    b[21] = t0D * x; b[22] = t1C * fC1; b[23] = t2B * fC2; b[24] = c4 * fC3;
}

constexpr int FIT_DIRS = 64;

// G X = H for the n x n system G and n right-hand sides (row-major, n <= 9), Gaussian elimination with partial pivoting; X overwrites H
static bool solve(int n, double* G, double* H) {
    for (int c = 0; c < n; ++c) {
        int p = c;
        for (int r = c + 1; r < n; ++r) if (fabs(G[r * n + c]) > fabs(G[p * n + c])) p = r;
        if (!(fabs(G[p * n + c]) > 0.0)) return false;
        if (p != c) for (int k = 0; k < n; ++k) { double u = G[c * n + k]; G[c * n + k] = G[p * n + k]; G[p * n + k] = u; u = H[c * n + k]; H[c * n + k] = H[p * n + k]; H[p * n + k] = u; }
        for (int r = c + 1; r < n; ++r) {
            const double f = G[r * n + c] / G[c * n + c];
            for (int k = c; k < n; ++k) G[r * n + k] -= f * G[c * n + k];
            for (int k = 0; k < n; ++k) H[r * n + k] -= f * H[c * n + k];
        }
    }
    for (int r = n - 1; r >= 0; --r)
        for (int k = 0; k < n; ++k) {
            double v = H[r * n + k];
            for (int c = r + 1; c < n; ++c) v -= G[r * n + c] * H[c * n + k];
            H[r * n + k] = v / G[r * n + r];
        }
    return true;
}

static bool is_identity3(const double* R) {
    for (int i = 0; i < 9; ++i) if (R[i] != ((i % 4 == 0) ? 1.0 : 0.0)) return false;
    return true;
}

static int rotation_matrices(const double* R, uint32_t degree, double* out) {
    if (!R || degree > 4 || (degree > 0 && !out)) return LFS_E_INVALID;
    for (int i = 0; i < 9; ++i) if (!isfinite(R[i])) return LFS_E_INVALID;
    if (is_identity3(R)) {   // exactly, not to rounding: the identity transform must leave every coefficient's bits alone
        for (uint32_t l = 1; l <= degree; ++l) {
            const int n = 2 * int(l) + 1;
            for (int i = 0; i < n * n; ++i) out[i] = (i % (n + 1) == 0) ? 1.0 : 0.0;
            out += n * n;
        }
        return LFS_OK;
    }
    double a[FIT_DIRS][25], b[FIT_DIRS][25];
    for (int j = 0; j < FIT_DIRS; ++j) {   // a Fibonacci sphere
        const double u = (j + 0.5) / FIT_DIRS, ph = acos(1.0 - 2.0 * u), th = M_PI * (1.0 + sqrt(5.0)) * (j + 0.5);
        const double d[3] = {cos(th) * sin(ph), sin(th) * sin(ph), cos(ph)};
        const double e[3] = {R[0] * d[0] + R[3] * d[1] + R[6] * d[2], R[1] * d[0] + R[4] * d[1] + R[7] * d[2], R[2] * d[0] + R[5] * d[1] + R[8] * d[2]};   // R^T d
        basis64(d[0], d[1], d[2], a[j]);
        basis64(e[0], e[1], e[2], b[j]);
    }
    for (uint32_t l = 1; l <= degree; ++l) {
        const int n = 2 * int(l) + 1, o = int(l * l);
        double G[81], H[81];
        for (int r = 0; r < n; ++r)
            for (int c = 0; c < n; ++c) {
                double g = 0.0, h = 0.0;
                for (int j = 0; j < FIT_DIRS; ++j) { g += a[j][o + r] * a[j][o + c]; h += a[j][o + r] * b[j][o + c]; }
                G[r * n + c] = g; H[r * n + c] = h;
            }
        if (!solve(n, G, H)) return LFS_E_INVALID;
        for (int i = 0; i < n * n; ++i) out[i] = H[i];
        out += n * n;
    }
    return LFS_OK;
}

static double det3(const double* a) {
    return a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) + a[2] * (a[3] * a[7] - a[4] * a[6]);
}

// ---- device ---------------------------------------------------------------------------------------------------------------------------------------------------
constexpr uint32_t GEOM_THREADS = 256;
constexpr uint32_t SH_THREADS = 256;     // four waves stage a tile; the first SH_TILE lanes rotate one row each
constexpr uint32_t SH_TILE = 128;        // rows per block at most
constexpr uint32_t SH_BATCH = 4;         // 16-byte loads a lane has in flight before it turns to LDS
constexpr uint32_t LDS_FLOATS = 6144;    // 24 KB: six blocks (24 waves) per CU
constexpr uint32_t MAX_WPAD = LDS_FLOATS / 4;

__global__ void __launch_bounds__(GEOM_THREADS) st_geom_kernel(const uint32_t N, const lfs_splat_transform xf, const float* means, const float* quats, const float* raw_scales,
                                                               float* means_o, float* quats_o, float* raw_scales_o) {
    const size_t i = size_t(blockIdx.x) * GEOM_THREADS + threadIdx.x;
    if (i >= N) return;
    if (means) {
        const float x = means[3 * i], y = means[3 * i + 1], z = means[3 * i + 2];
        const float ox = ((xf.sR[0] * x + xf.sR[1] * y) + xf.sR[2] * z) + xf.t[0];
        const float oy = ((xf.sR[3] * x + xf.sR[4] * y) + xf.sR[5] * z) + xf.t[1];
        const float oz = ((xf.sR[6] * x + xf.sR[7] * y) + xf.sR[8] * z) + xf.t[2];
        means_o[3 * i] = ox; means_o[3 * i + 1] = oy; means_o[3 * i + 2] = oz;
    }
    if (quats) {   // q_R (x) q on the raw quaternion, the reference's term order (splat_data.cpp:356-359)
        const float w1 = xf.q[0], x1 = xf.q[1], y1 = xf.q[2], z1 = xf.q[3];
        const float w2 = quats[4 * i], x2 = quats[4 * i + 1], y2 = quats[4 * i + 2], z2 = quats[4 * i + 3];
        const float ow = ((w1 * w2 - x1 * x2) - y1 * y2) - z1 * z2;
        const float ox = ((w1 * x2 + x1 * w2) + y1 * z2) - z1 * y2;
        const float oy = ((w1 * y2 - x1 * z2) + y1 * w2) + z1 * x2;
        const float oz = ((w1 * z2 + x1 * y2) - y1 * x2) + z1 * w2;
        quats_o[4 * i] = ow; quats_o[4 * i + 1] = ox; quats_o[4 * i + 2] = oy; quats_o[4 * i + 3] = oz;
    }
    if (raw_scales) {
        const float a = raw_scales[3 * i], b = raw_scales[3 * i + 1], c = raw_scales[3 * i + 2];
        raw_scales_o[3 * i] = a + xf.log_s; raw_scales_o[3 * i + 1] = b + xf.log_s; raw_scales_o[3 * i + 2] = c + xf.log_s;
    }
}

// band L of the three channels of one LDS row: a'_i = sum_k M[i][k] a_k, ascending k, left to right
template <int L>
__device__ __forceinline__ void rotate_band(const float* __restrict__ M, float* __restrict__ row) {
    constexpr int n = 2 * L + 1;
    float* const band = row + 3 * (L * L - 1);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float a[n], o[n];
#pragma unroll
        for (int k = 0; k < n; ++k) a[k] = band[3 * k + ch];
#pragma unroll
        for (int i = 0; i < n; ++i) {
            float acc = M[i * n] * a[0];
#pragma unroll
            for (int k = 1; k < n; ++k) acc = acc + M[i * n + k] * a[k];
            o[i] = acc;
        }
#pragma unroll
        for (int i = 0; i < n; ++i) band[3 * i + ch] = o[i];
    }
}

// W = 3 * shN_rows floats per row; tile rows; pad = Wpad - W in {0, 1}. VEC: both pointers 16-byte aligned (tile is a multiple of 4 rows: so is every tile's base)
template <int DEG, bool VEC>
__global__ void __launch_bounds__(SH_THREADS) st_sh_kernel(const uint32_t N, const lfs_splat_transform xf, const float* shN, float* shN_o, const uint32_t W, const uint32_t tile) {
    __shared__ float lds[LDS_FLOATS];
    const uint32_t pad = (W & 1u) ^ 1u, Wpad = W + pad;
    const uint32_t g0 = blockIdx.x * tile;
    const uint32_t n = min(tile, N - g0);
    const uint32_t total = n * W;               // <= tile * Wpad <= LDS_FLOATS
    const size_t base = size_t(g0) * W;
    const float* const src = shN + base;
    float* const dst = shN_o + base;
    const uint32_t nvec = VEC ? total / 4u : 0u;
    for (uint32_t v0 = threadIdx.x; v0 < nvec; v0 += SH_BATCH * SH_THREADS) {   // SH_BATCH loads issued back to back, then their LDS stores
        float4 q[SH_BATCH];
#pragma unroll
        for (uint32_t j = 0; j < SH_BATCH; ++j) {
            const uint32_t v = v0 + j * SH_THREADS;   // (past the end: the tile's last vector once more, not stored - no branch between the loads)
            q[j] = *reinterpret_cast<const float4*>(src + 4u * (v < nvec ? v : nvec - 1u));
        }
#pragma unroll
        for (uint32_t j = 0; j < SH_BATCH; ++j) {
            const uint32_t v = v0 + j * SH_THREADS;
            if (v >= nvec) continue;
            if (!pad) {
                *reinterpret_cast<float4*>(lds + 4u * v) = q[j];
            } else {
                const uint32_t f = 4u * v, g = f / W;
                uint32_t c = f - g * W, li = f + g;
                const float e[4] = {q[j].x, q[j].y, q[j].z, q[j].w};
#pragma unroll
                for (int k = 0; k < 4; ++k) { lds[li] = e[k]; ++li; if (++c == W) { c = 0; ++li; } }
            }
        }
    }
    for (uint32_t f = 4u * nvec + threadIdx.x; f < total; f += SH_THREADS) lds[pad ? f + f / W : f] = src[f];
    __syncthreads();
    if (DEG > 0 && threadIdx.x < n) {
        float* const row = lds + threadIdx.x * Wpad;
        rotate_band<1>(xf.m1, row);
        if (DEG >= 2) rotate_band<2>(xf.m2, row);
        if (DEG >= 3) rotate_band<3>(xf.m3, row);
        if (DEG >= 4) rotate_band<4>(xf.m4, row);
    }
    __syncthreads();
    for (uint32_t v = threadIdx.x; v < nvec; v += SH_THREADS) {
        float4 q;
        if (!pad) {
            q = *reinterpret_cast<const float4*>(lds + 4u * v);
        } else {
            const uint32_t f = 4u * v, g = f / W;
            uint32_t c = f - g * W, li = f + g;
            float e[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) { e[j] = lds[li]; ++li; if (++c == W) { c = 0; ++li; } }
            q = make_float4(e[0], e[1], e[2], e[3]);
        }
        *reinterpret_cast<float4*>(dst + 4u * v) = q;
    }
    for (uint32_t f = 4u * nvec + threadIdx.x; f < total; f += SH_THREADS) dst[f] = lds[pad ? f + f / W : f];
}

template <int DEG>
static void launch_sh(bool vec, uint32_t blocks, hipStream_t s, uint32_t N, const lfs_splat_transform& xf, const float* shN, float* shN_o, uint32_t W, uint32_t tile) {
    if (vec) hipLaunchKernelGGL((st_sh_kernel<DEG, true>), dim3(blocks), dim3(SH_THREADS), 0, s, N, xf, shN, shN_o, W, tile);
    else hipLaunchKernelGGL((st_sh_kernel<DEG, false>), dim3(blocks), dim3(SH_THREADS), 0, s, N, xf, shN, shN_o, W, tile);
}

} // namespace st
} // namespace lfs

using namespace lfs;

extern "C" int lfs_sh_rotation_matrices(const double* R, uint32_t degree, double* out) { return st::rotation_matrices(R, degree, out); }

extern "C" int lfs_splat_transform_from_matrix(const double* m, uint32_t sh_degree, lfs_splat_transform* out) {
    if (!m || !out || sh_degree > 4) return LFS_E_INVALID;
    for (int i = 0; i < 16; ++i) if (!isfinite(m[i])) return LFS_E_INVALID;
    if (m[12] != 0.0 || m[13] != 0.0 || m[14] != 0.0 || m[15] != 1.0) return LFS_E_INVALID;
    const double A[9] = {m[0], m[1], m[2], m[4], m[5], m[6], m[8], m[9], m[10]};
    const double det = st::det3(A);
    if (!(det > 0.0) || !isfinite(det)) return LFS_E_INVALID;          // s <= 0, a reflection
    const double s = cbrt(det);
    if (!(s > 0.0) || !isfinite(s)) return LFS_E_INVALID;
    double R[9];
    for (int i = 0; i < 9; ++i) R[i] = A[i] / s;
    for (int i = 0; i < 3; ++i)                                          // a similarity: A^T A = s^2 I
        for (int j = 0; j < 3; ++j) {
            const double g = R[i] * R[j] + R[3 + i] * R[3 + j] + R[6 + i] * R[6 + j];
            if (!(fabs(g - (i == j ? 1.0 : 0.0)) <= 1e-5)) return LFS_E_INVALID;
        }
    for (int it = 0; it < 5 && !st::is_identity3(R); ++it) {            // the nearest rotation: Newton's iteration for the polar factor, R <- (R + R^-T) / 2
        const double d = st::det3(R);
        const double C[9] = {R[4] * R[8] - R[5] * R[7], R[5] * R[6] - R[3] * R[8], R[3] * R[7] - R[4] * R[6],
                             R[2] * R[7] - R[1] * R[8], R[0] * R[8] - R[2] * R[6], R[1] * R[6] - R[0] * R[7],
                             R[1] * R[5] - R[2] * R[4], R[2] * R[3] - R[0] * R[5], R[0] * R[4] - R[1] * R[3]};   // the cofactor matrix = det R^-T
        for (int i = 0; i < 9; ++i) R[i] = 0.5 * (R[i] + C[i] / d);
    }
    lfs_splat_transform x;
    for (int i = 0; i < 9; ++i) x.sR[i] = float(s * R[i]);
    x.t[0] = float(m[3]); x.t[1] = float(m[7]); x.t[2] = float(m[11]);
    // Shepperd's method: the largest of w, x, y, z is taken from the diagonal, the others from the off-diagonal sums
    const double tr = R[0] + R[4] + R[8];
    double q[4];
    if (tr >= R[0] && tr >= R[4] && tr >= R[8]) {
        q[0] = 1.0 + tr; q[1] = R[7] - R[5]; q[2] = R[2] - R[6]; q[3] = R[3] - R[1];
    } else if (R[0] >= R[4] && R[0] >= R[8]) {
        q[0] = R[7] - R[5]; q[1] = 1.0 + R[0] - R[4] - R[8]; q[2] = R[1] + R[3]; q[3] = R[2] + R[6];
    } else if (R[4] >= R[8]) {
        q[0] = R[2] - R[6]; q[1] = R[1] + R[3]; q[2] = 1.0 - R[0] + R[4] - R[8]; q[3] = R[5] + R[7];
    } else {
        q[0] = R[3] - R[1]; q[1] = R[2] + R[6]; q[2] = R[5] + R[7]; q[3] = 1.0 - R[0] - R[4] + R[8];
    }
    const double qn = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]) * (q[0] < 0.0 ? -1.0 : 1.0);
    for (int i = 0; i < 4; ++i) x.q[i] = float(q[i] / qn + 0.0);      // (+ 0.0: no -0 components)
    x.log_s = float(log(s));
    x.sh_degree = sh_degree;
    double M[164];
    const int rc = st::rotation_matrices(R, 4, M);                       // all four bands, whatever sh_degree rotates: the record depends on the degree in one field only
    if (rc != LFS_OK) return rc;
    for (int i = 0; i < 9; ++i) x.m1[i] = float(M[i]);
    for (int i = 0; i < 25; ++i) x.m2[i] = float(M[9 + i]);
    for (int i = 0; i < 49; ++i) x.m3[i] = float(M[34 + i]);
    for (int i = 0; i < 81; ++i) x.m4[i] = float(M[83 + i]);
    *out = x;
    return LFS_OK;
}

extern "C" int lfs_splat_transform_apply(uint32_t N, const lfs_splat_transform* xf, const float* means, const float* quats, const float* raw_scales, const float* shN,
                                         uint32_t shN_rows, float* means_o, float* quats_o, float* raw_scales_o, float* shN_o, lfs_stream_t stream) {
    if (!xf || xf->sh_degree > 4) return LFS_E_INVALID;
    if (N == 0) return LFS_OK;
    if (!means != !means_o || !quats != !quats_o || !raw_scales != !raw_scales_o || !shN != !shN_o) return LFS_E_INVALID;   // a pair is given or skipped as a whole
    const uint32_t deg = xf->sh_degree;
    if (shN && shN_rows < (deg + 1) * (deg + 1) - 1) return LFS_E_INVALID;
    const uint64_t W64 = 3ull * shN_rows;
    if (shN && (W64 | 1ull) > st::MAX_WPAD) return LFS_E_UNSUPPORTED;   // 511 rows: far beyond any degree a splat file holds
    hipStream_t s = (hipStream_t)stream;
    bool launched = false;
    if (means || quats || raw_scales) {
        launched = true;
        const uint32_t blocks = (N + st::GEOM_THREADS - 1) / st::GEOM_THREADS;
        hipLaunchKernelGGL(st::st_geom_kernel, dim3(blocks), dim3(st::GEOM_THREADS), 0, s, N, *xf, means, quats, raw_scales, means_o, quats_o, raw_scales_o);
    }
    if (shN && shN_rows > 0 && !(deg == 0 && shN == shN_o)) {
        launched = true;
        const uint32_t W = uint32_t(W64), Wpad = W | 1u;
        uint32_t tile = st::LDS_FLOATS / Wpad;
        tile = (tile > st::SH_TILE ? st::SH_TILE : tile) & ~3u;         // >= 4 by the check above
        const uint32_t blocks = (N + tile - 1) / tile;
        const bool vec = ((reinterpret_cast<uintptr_t>(shN) | reinterpret_cast<uintptr_t>(shN_o)) & 15u) == 0;
        switch (deg) {
            case 0: st::launch_sh<0>(vec, blocks, s, N, *xf, shN, shN_o, W, tile); break;
            case 1: st::launch_sh<1>(vec, blocks, s, N, *xf, shN, shN_o, W, tile); break;
            case 2: st::launch_sh<2>(vec, blocks, s, N, *xf, shN, shN_o, W, tile); break;
            case 3: st::launch_sh<3>(vec, blocks, s, N, *xf, shN, shN_o, W, tile); break;
            default: st::launch_sh<4>(vec, blocks, s, N, *xf, shN, shN_o, W, tile); break;
        }
    }
    return launched ? (int)hipGetLastError() : LFS_OK;
}
