// SOG export kernels: Morton codes of the means, Lloyd's assignment (dense and 1-D) and the segmented-mean centroid update.
// Reference behaviour: kernels/morton_encoding.cu:11-97 (codes, bounding cube), kernels/kmeans.cu:18-122 (assignment, 1-D assignment,
// centroid update); the host loops around them live in sog.py. None of the kernels uses a float atomic: every result has the same bits on every run.
//
// CDNA4 design.
//  * Assignment is argmax_c (x.c - |c|^2 / 2), a dense [k x D] x [D x N] contraction: v_mfma_f32_16x16x4_f32 (exact f32 fmaf chains). Centroids are the A
//    operand, points the B operand, so the accumulator lane of column lane & 15 holds 4 centroid scores of ONE point and the running (best, index) pair
//    is lane-private until one exchange between the four lane groups at the very end. A wave keeps 4 point tiles (64 points) as B fragments in registers
//    for the whole kernel: each centroid fragment read from LDS feeds 4 independent accumulators (40-cycle dependent latency against 32-cycle issue).
//    A pre-pass writes the centroids once in FRAGMENT order (one 64-float line per [16 centroids x 4 dims] MFMA operand, D zero-padded, k padded to the
//    64-centroid chunk with -inf scores) together with -|c|^2 / 2; the main kernel's staging is then a straight float4 copy whose LDS writes and fragment
//    reads are both lane-linear (conflict-free without padding), prefetched into registers one chunk ahead of the MFMA loop.
//  * The update gets the points grouped by label (order / seg_start from a stable sort on the caller's side): one workgroup per cluster sums its rows in
//    a fixed order in f64 and writes sum / count; an empty cluster writes nothing (kmeans.cu:119-121).
//  * Morton: per-block min / max partials, one block folds them into (min, cube), then one thread per point.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/lfs_gsplat.h"
#include "lfs_prof.h"

namespace lfs {
namespace sog {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int THREADS = 256;
constexpr uint32_t MORTON_MAX_PARTIALS = 1024;
constexpr int AS_PT = 4;                    // 16-point tiles per wave (B fragments resident in registers)
constexpr int AS_CT = 4;                    // 16-centroid tiles per staged chunk
constexpr int AS_CHUNK = 16 * AS_CT;        // centroids per chunk
constexpr int AS_POINTS = (THREADS / 64) * 16 * AS_PT;   // points per workgroup
constexpr uint32_t K_MAX = 65536, D_MAX = 64;

__host__ __device__ inline uint32_t ksteps_for(uint32_t D) { return 4u * ((D + 15u) / 16u); }   // MFMA k-steps: D zero-padded to 16 / 32 / 48 / 64
__host__ __device__ inline uint32_t padded_k(uint32_t k) { return (k + AS_CHUNK - 1u) / AS_CHUNK * AS_CHUNK; }

// ---- Morton ---------------------------------------------------------------------------------------------------------
struct MinMax3 { float lo[3], hi[3]; };

__device__ __forceinline__ void mm_init(MinMax3& m) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { m.lo[a] = INFINITY; m.hi[a] = -INFINITY; }
}

// min / max over the workgroup; the result is valid in thread 0. min and max are exact, so the order of the fold does not matter.
__device__ __forceinline__ void mm_block_reduce(MinMax3& m) {
    __shared__ float s_mm[THREADS / 64][6];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            m.lo[a] = fminf(m.lo[a], __shfl_xor(m.lo[a], off));
            m.hi[a] = fmaxf(m.hi[a], __shfl_xor(m.hi[a], off));
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { s_mm[wave][a] = m.lo[a]; s_mm[wave][3 + a] = m.hi[a]; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < THREADS / 64; ++w) {
#pragma unroll
            for (int a = 0; a < 3; ++a) { m.lo[a] = fminf(m.lo[a], s_mm[w][a]); m.hi[a] = fmaxf(m.hi[a], s_mm[w][3 + a]); }
        }
    }
}

__global__ void __launch_bounds__(THREADS) morton_minmax_kernel(int64_t N, const float* __restrict__ means, float* __restrict__ partial) {
    MinMax3 m; mm_init(m);
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < N; i += (int64_t)gridDim.x * THREADS) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { const float v = means[3 * i + a]; m.lo[a] = fminf(m.lo[a], v); m.hi[a] = fmaxf(m.hi[a], v); }
    }
    mm_block_reduce(m);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { partial[6 * blockIdx.x + a] = m.lo[a]; partial[6 * blockIdx.x + 3 + a] = m.hi[a]; }
    }
}

// bounds = (min x, min y, min z, cube): morton_encoding.cu:66-72
__global__ void __launch_bounds__(THREADS) morton_bounds_kernel(uint32_t P, const float* __restrict__ partial, float* __restrict__ bounds) {
    MinMax3 m; mm_init(m);
    for (uint32_t i = threadIdx.x; i < P; i += THREADS) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { m.lo[a] = fminf(m.lo[a], partial[6 * i + a]); m.hi[a] = fmaxf(m.hi[a], partial[6 * i + 3 + a]); }
    }
    mm_block_reduce(m);
    if (threadIdx.x == 0) {
        const float cube = fmaxf(fmaxf(m.hi[0] - m.lo[0], m.hi[1] - m.lo[1]), m.hi[2] - m.lo[2]);
        bounds[0] = m.lo[0]; bounds[1] = m.lo[1]; bounds[2] = m.lo[2];
        bounds[3] = fmaxf(cube, 1e-7f);
    }
}

__device__ __forceinline__ uint64_t split_by_3(uint32_t a) {
    uint64_t x = a & 0x1fffffu;
    x = (x | x << 32) & 0x1f00000000ffffull;
    x = (x | x << 16) & 0x1f0000ff0000ffull;
    x = (x | x << 8) & 0x100f00f00f00f00full;
    x = (x | x << 4) & 0x10c30c30c30c30c3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}

__global__ void __launch_bounds__(THREADS) morton_encode_kernel(int64_t N, const float* __restrict__ means, const float* __restrict__ bounds, int64_t* __restrict__ codes) {
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= N) return;
    const double size = (double)bounds[3];
    uint32_t q[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float rel = means[3 * i + a] - bounds[a];       // f32 subtraction, then f64 (morton_encoding.cu:38-40)
        const double normalized = (double)rel / size;
        q[a] = (uint32_t)(normalized * 2097151.0);
    }
    const uint64_t code = split_by_3(q[0]) | (split_by_3(q[1]) << 1) | (split_by_3(q[2]) << 2);
    codes[i] = (int64_t)(code ^ 0x8000000000000000ull);       // + INT64_MIN (the code has 63 bits)
}

// ---- dense assignment --------------------------------------------------------------------------------------------------
// frag: [KP / 16][KS][64] with element (q * 16 + r) of line (tile, kk) = centroid 16 * tile + r, dimension 4 * kk + q;  hn[KP] = -|c|^2 / 2 (-inf past k)
__global__ void __launch_bounds__(THREADS) kmeans_prep_kernel(uint32_t k, uint32_t D, uint32_t KP, uint32_t KS, const float* __restrict__ centroids,
                                                              float* __restrict__ frag, float* __restrict__ hn) {
    const uint32_t DP = 4 * KS;
    const uint32_t e = blockIdx.x * THREADS + threadIdx.x;
    if (e >= KP * DP) return;
    const uint32_t c = e / DP, d = e % DP;
    const bool real = c < k;
    frag[((size_t)(c >> 4) * KS + (d >> 2)) * 64 + (d & 3) * 16 + (c & 15)] = (real && d < D) ? centroids[(size_t)c * D + d] : 0.f;
    if (d == 0) {
        float s = 0.f;
        if (real) for (uint32_t j = 0; j < D; ++j) { const float v = centroids[(size_t)c * D + j]; s = fmaf(v, v, s); }
        hn[c] = real ? -0.5f * s : -INFINITY;
    }
}

template <int KS>
__global__ void __launch_bounds__(THREADS) kmeans_assign_kernel(int64_t N, uint32_t k, uint32_t D, uint32_t nchunks, const float* __restrict__ data,
                                                                const float* __restrict__ frag, const float* __restrict__ hn, int32_t* __restrict__ labels) {
    constexpr int V4 = KS / 4;                       // float4 per thread and chunk: AS_CT * KS * 64 floats over 256 threads
    __shared__ __attribute__((aligned(16))) float s_a[AS_CT * KS * 64];
    __shared__ __attribute__((aligned(16))) float s_hn[AS_CHUNK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, q = lane >> 4;
    const int64_t pbase = ((int64_t)blockIdx.x * (THREADS / 64) + wave) * (16 * AS_PT);

    float b[AS_PT][KS];                              // B fragments: point pbase + 16 * pt + col, dimension 4 * kk + q
#pragma unroll
    for (int pt = 0; pt < AS_PT; ++pt) {
        const int64_t p = pbase + 16 * pt + col;
        const float* row = data + (size_t)(p < N ? p : 0) * D;
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) {
            const uint32_t d = 4 * kk + q;
            b[pt][kk] = (p < N && d < D) ? row[d] : 0.f;
        }
    }
    float best[AS_PT]; int bidx[AS_PT];
#pragma unroll
    for (int pt = 0; pt < AS_PT; ++pt) { best[pt] = -INFINITY; bidx[pt] = 0x7fffffff; }

    const f32x4* g4 = reinterpret_cast<const f32x4*>(frag);     // (ext-vector values: they stay in registers where HIP's float4 struct array did not)
    f32x4 pre[V4]; float pre_hn = 0.f;
#pragma unroll
    for (int i = 0; i < V4; ++i) pre[i] = g4[i * THREADS + tid];
    if (tid < AS_CHUNK) pre_hn = hn[tid];

    for (uint32_t ch = 0; ch < nchunks; ++ch) {
        __syncthreads();                             // every wave is done with the previous chunk
#pragma unroll
        for (int i = 0; i < V4; ++i) reinterpret_cast<f32x4*>(s_a)[i * THREADS + tid] = pre[i];
        if (tid < AS_CHUNK) s_hn[tid] = pre_hn;
        __syncthreads();
        if (ch + 1 < nchunks) {                      // the next chunk travels while this one is multiplied
#pragma unroll
            for (int i = 0; i < V4; ++i) pre[i] = g4[(size_t)(ch + 1) * (AS_CT * KS * 16) + i * THREADS + tid];
            if (tid < AS_CHUNK) pre_hn = hn[(ch + 1) * AS_CHUNK + tid];
        }
#pragma unroll
        for (int ct = 0; ct < AS_CT; ++ct) {
            const f32x4 h = *reinterpret_cast<const f32x4*>(s_hn + 16 * ct + 4 * q);
            f32x4 acc[AS_PT];
#pragma unroll
            for (int pt = 0; pt < AS_PT; ++pt) acc[pt] = h;
#pragma unroll
            for (int kk = 0; kk < KS; ++kk) {
                const float a = s_a[(ct * KS + kk) * 64 + lane];
#pragma unroll
                for (int pt = 0; pt < AS_PT; ++pt) acc[pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[pt][kk], acc[pt], 0, 0, 0);
            }
            const int i0 = (int)(ch * AS_CHUNK) + 16 * ct + 4 * q;   // ascending within the lane: a strict > keeps the lowest index of equal scores
#pragma unroll
            for (int pt = 0; pt < AS_PT; ++pt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float v = acc[pt][r];
                    if (v > best[pt]) { best[pt] = v; bidx[pt] = i0 + r; }
                }
            }
        }
    }
    // the four lane groups hold disjoint centroid rows of the same 16 points: fold (score, index) pairs, lowest index among equal scores
#pragma unroll
    for (int pt = 0; pt < AS_PT; ++pt) {
#pragma unroll
        for (int m = 16; m <= 32; m <<= 1) {
            const float ov = __shfl_xor(best[pt], m);
            const int oi = __shfl_xor(bidx[pt], m);
            if (ov > best[pt] || (ov == best[pt] && oi < bidx[pt])) { best[pt] = ov; bidx[pt] = oi; }
        }
        const int64_t p = pbase + 16 * pt + col;
        if (q == 0 && p < N) labels[p] = (uint32_t)bidx[pt] < k ? bidx[pt] : 0;   // (nothing compared greater than -inf: NaN data)
    }
}

// ---- 1-D assignment: first index that minimises fabsf(p - c) under a strict < (kmeans.cu:58-83) ----------------------------
// c ascending. j = first index with c[j] >= p. fl(p - c[i]) is non-increasing in i left of j and non-decreasing from j on, so the minimum is
// min(dl, dr) with dl = |p - c[j-1]|, dr = |p - c[j]|; rounding can make several indices LEFT of j share the value dl (and duplicates do), the linear
// scan keeps the first of them: a second search for the first i with |p - c[i]| <= dl. On the right the first index of the minimum is j itself.
__global__ void __launch_bounds__(THREADS) kmeans_assign_1d_kernel(int64_t n, int k, const float* __restrict__ data, const float* __restrict__ c,
                                                                   int32_t* __restrict__ labels) {
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const float p = data[i];
    int lo = 0, hi = k;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (c[mid] < p) lo = mid + 1; else hi = mid; }
    const int j = lo;
    int ans = 0;
    if (j > 0) {
        const float dl = fabsf(p - c[j - 1]);
        const float dr = j < k ? fabsf(p - c[j]) : INFINITY;
        if (dr < dl) ans = j;
        else {
            lo = 0; hi = j - 1;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (fabsf(p - c[mid]) <= dl) hi = mid; else lo = mid + 1; }
            ans = lo;
        }
    }
    labels[i] = ans;
}

// ---- centroid update: mean of the rows order[seg[c] .. seg[c+1]) -------------------------------------------------------------------
// Thread t sums dimension t % DP2 of every G-th row (G = 256 / DP2, DP2 = D rounded up to a power of two) in f64, the G partials are folded by a fixed
// tree in LDS. Bounds come from device memory, so they are clamped here: no value of order / seg_start can make the kernel leave data[N, D].
__global__ void __launch_bounds__(THREADS) kmeans_update_kernel(int64_t N, uint32_t D, uint32_t DP2, const float* __restrict__ data, const int32_t* __restrict__ order,
                                                                const int32_t* __restrict__ seg, float* __restrict__ centroids) {
    __shared__ double s_sum[THREADS];
    const uint32_t c = blockIdx.x, t = threadIdx.x;
    int64_t beg = seg[c], end = seg[c + 1];
    beg = beg < 0 ? 0 : (beg > N ? N : beg);
    end = end < beg ? beg : (end > N ? N : end);
    if (end <= beg) return;                          // an empty cluster keeps its centroid (uniform over the workgroup)
    const uint32_t d = t & (DP2 - 1), g = t / DP2, G = THREADS / DP2;
    double acc = 0.0;
    if (d < D) {
        for (int64_t i = beg + g; i < end; i += G) {
            const int64_t row = order[i];
            if (row >= 0 && row < N) acc += (double)data[(size_t)row * D + d];
        }
    }
    s_sum[t] = acc;
    __syncthreads();
    for (uint32_t stride = THREADS / 2; stride >= DP2; stride >>= 1) {
        if (t < stride) s_sum[t] += s_sum[t + stride];
        __syncthreads();
    }
    if (t < D) centroids[(size_t)c * D + t] = (float)(s_sum[t] / (double)(end - beg));
}

static inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }
static inline uint32_t morton_partials(int64_t N) {
    const int64_t blocks = (N + THREADS - 1) / THREADS;
    return (uint32_t)(blocks < 1 ? 1 : (blocks > (int64_t)MORTON_MAX_PARTIALS ? (int64_t)MORTON_MAX_PARTIALS : blocks));
}
static inline bool grid_ok(int64_t n) { return n >= 0 && (n + THREADS - 1) / THREADS <= 0x7fffffffll; }

} // namespace sog
} // namespace lfs

using namespace lfs::sog;

extern "C" size_t lfs_morton_workspace_bytes(int64_t N) {
    if (N < 0) return 0;
    return align256(((size_t)morton_partials(N) * 6 + 4) * sizeof(float));
}

extern "C" int lfs_morton_encode(int64_t N, const float* means, int64_t* codes, void* workspace, size_t workspace_bytes, lfs_stream_t stream) {
    if (N < 0 || !grid_ok(N)) return LFS_E_INVALID;
    if (N == 0) return LFS_OK;
    if (!means || !codes || !workspace || ((uintptr_t)workspace & 15)) return LFS_E_INVALID;
    if (workspace_bytes < lfs_morton_workspace_bytes(N)) return LFS_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t P = morton_partials(N);
    float* partial = (float*)workspace;
    float* bounds = partial + (size_t)P * 6;
    lfs::ProfScope prof("morton_encode", s);
    hipLaunchKernelGGL(morton_minmax_kernel, dim3(P), dim3(THREADS), 0, s, N, means, partial);
    hipLaunchKernelGGL(morton_bounds_kernel, dim3(1), dim3(THREADS), 0, s, P, (const float*)partial, bounds);
    hipLaunchKernelGGL(morton_encode_kernel, dim3((uint32_t)((N + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, N, means, (const float*)bounds, codes);
    return (int)hipGetLastError();
}

extern "C" size_t lfs_kmeans_assign_workspace_bytes(uint32_t k, uint32_t D) {
    if (k < 1 || k > K_MAX || D < 1 || D > D_MAX) return 0;
    return align256((size_t)padded_k(k) * (4 * ksteps_for(D) + 1) * sizeof(float));
}

extern "C" int lfs_kmeans_assign(int64_t N, uint32_t k, uint32_t D, const float* data, const float* centroids, int32_t* labels,
                                 void* workspace, size_t workspace_bytes, lfs_stream_t stream) {
    if (N < 0 || !grid_ok(N) || k < 1 || D < 1) return LFS_E_INVALID;
    if (k > K_MAX || D > D_MAX) return LFS_E_UNSUPPORTED;
    if (N == 0) return LFS_OK;
    if (!data || !centroids || !labels || !workspace || ((uintptr_t)workspace & 15)) return LFS_E_INVALID;
    if (workspace_bytes < lfs_kmeans_assign_workspace_bytes(k, D)) return LFS_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t KS = ksteps_for(D), KP = padded_k(k), nchunks = KP / AS_CHUNK;
    float* frag = (float*)workspace;
    float* hn = frag + (size_t)KP * 4 * KS;
    hipLaunchKernelGGL(kmeans_prep_kernel, dim3((KP * 4 * KS + THREADS - 1) / THREADS), dim3(THREADS), 0, s, k, D, KP, KS, centroids, frag, hn);
    const dim3 grid((uint32_t)((N + AS_POINTS - 1) / AS_POINTS));
    lfs::ProfScope prof("kmeans_assign", s);
    switch (KS) {
    case 4: hipLaunchKernelGGL(kmeans_assign_kernel<4>, grid, dim3(THREADS), 0, s, N, k, D, nchunks, data, (const float*)frag, (const float*)hn, labels); break;
    case 8: hipLaunchKernelGGL(kmeans_assign_kernel<8>, grid, dim3(THREADS), 0, s, N, k, D, nchunks, data, (const float*)frag, (const float*)hn, labels); break;
    case 12: hipLaunchKernelGGL(kmeans_assign_kernel<12>, grid, dim3(THREADS), 0, s, N, k, D, nchunks, data, (const float*)frag, (const float*)hn, labels); break;
    default: hipLaunchKernelGGL(kmeans_assign_kernel<16>, grid, dim3(THREADS), 0, s, N, k, D, nchunks, data, (const float*)frag, (const float*)hn, labels); break;
    }
    return (int)hipGetLastError();
}

extern "C" int lfs_kmeans_assign_1d(int64_t n, uint32_t k, const float* data, const float* sorted_centroids, int32_t* labels, lfs_stream_t stream) {
    if (n < 0 || !grid_ok(n) || k < 1 || k > 0x40000000u) return LFS_E_INVALID;
    if (n == 0) return LFS_OK;
    if (!data || !sorted_centroids || !labels) return LFS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    lfs::ProfScope prof("kmeans_assign_1d", s);
    hipLaunchKernelGGL(kmeans_assign_1d_kernel, dim3((uint32_t)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, n, (int)k, data, sorted_centroids, labels);
    return (int)hipGetLastError();
}

extern "C" int lfs_kmeans_update(int64_t N, uint32_t k, uint32_t D, const float* data, const int32_t* order, const int32_t* seg_start, float* centroids,
                                 lfs_stream_t stream) {
    if (N < 0 || N > 0x7fffffffll || k < 1 || D < 1) return LFS_E_INVALID;
    if (k > K_MAX || D > D_MAX) return LFS_E_UNSUPPORTED;
    if (!seg_start || !centroids || (N > 0 && (!data || !order))) return LFS_E_INVALID;
    if (N == 0) return LFS_OK;
    uint32_t DP2 = 1;
    while (DP2 < D) DP2 <<= 1;
    hipStream_t s = (hipStream_t)stream;
    lfs::ProfScope prof("kmeans_update", s);
    hipLaunchKernelGGL(kmeans_update_kernel, dim3(k), dim3(THREADS), 0, s, N, D, DP2, data, order, seg_start, centroids);
    return (int)hipGetLastError();
}
