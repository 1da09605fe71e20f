// Visible-only Adam (gsplat's SelectiveAdam, the official 3DGS code's sparse_adam): the update of adam.hip for the Gaussians a step's views saw, and nothing -
// no load, no store - for the rest. A translation unit of its own: adam.hip's code object keeps every byte.
//
// Visibility is one bit per Gaussian: bit i of a uint32 array of lfs_visibility_words(N) words, bits >= N zero. At 1 M Gaussians that is 125 KB, which stays in
// cache. lfs_fastgs_view_visibility writes it from the n_touched column of a view's primitive workspace (one lane per Gaussian, one ballot per wave, every wave
// owns its two words: no atomics); lfs_adam_step_multi_visible consumes it, one launch for all parameter groups.
//
// Two row classes, by the tensor's row width n_elements / N:
//   wide rows (shN: 9 / 24 / 45 / 72 floats; anything above 4): a wave takes a block of 64 Gaussians, reads the block's two mask words at a wave-uniform address,
//     compacts the set bits (lane r learns the position of the r-th set bit) and spreads the (visible Gaussian, element) pairs over its lanes: every lane
//     works at any visibility, and a row of an invisible Gaussian is never addressed. A block with all 64 bits set is one contiguous span and moves 16 bytes
//     per lane as adam.hip does.
//   narrow rows (1, 3, 4 floats): the flat 16-byte accesses of adam_range, skipped when none of the four elements belongs to a visible Gaussian, with a
//     per-element select otherwise (a 16-byte access may straddle into an invisible neighbour's row: its elements are stored back as they were loaded).
// Pointers that are not 16-byte aligned take the 4-byte accesses. No LDS, no scratch. Compiled with -ffp-contract=off: adam_elem rounds as in adam.hip.
#include <hip/hip_runtime.h>
#include "../../include/lfs_gsplat.h"
#include "lfs_prof.h"
#include "lfs_adam.cuh"
#include "lfs_fastgs.cuh"

namespace lfs {
namespace adamv {

constexpr uint32_t WIDE_MIN = 5;          // rows of at least this many floats take the compaction path ...
constexpr uint32_t WIDE_MAX = 1u << 20;   // ... up to here (64 rows stay inside 32-bit element counts); wider ones take the flat path with a run-time width

__global__ void __launch_bounds__(256) visibility_kernel(const uint32_t N, const uint32_t* __restrict__ n_touched, uint32_t* __restrict__ bits, const int accumulate) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;     // (< 2^32: the grid has ceil(N / 256) workgroups)
    const uint64_t b = __ballot(i < N && n_touched[i] != 0u);
    const uint32_t lane = threadIdx.x & 63u;
    if (lane < 2u) {                                          // lanes 0 and 1 store the wave's two words
        const uint32_t w = (i >> 6) * 2u + lane, half = uint32_t(b >> (32u * lane));
        if (w < (N + 31u) / 32u) bits[w] = accumulate ? (bits[w] | half) : half;
    }
}

struct Multi {
    lfs_adam_tensor t[LFS_ADAM_MAX_TENSORS];
    uint32_t width[LFS_ADAM_MAX_TENSORS];
    int32_t block_begin[LFS_ADAM_MAX_TENSORS + 1]; // workgroup ranges per tensor
    const uint32_t* bits;
    uint32_t N;
    int32_t n;
};

__device__ __forceinline__ bool aligned16(const lfs_adam_tensor& t) {
    return ((reinterpret_cast<uintptr_t>(t.param) | reinterpret_cast<uintptr_t>(t.exp_avg) | reinterpret_cast<uintptr_t>(t.exp_avg_sq) |
             reinterpret_cast<uintptr_t>(t.grad)) & 15) == 0;
}

// one element, kept unless its Gaussian is visible (the arithmetic runs on copies: a NaN gradient of an invisible row stays in a dead register)
__device__ __forceinline__ void adam_elem_if(const bool vis, float& p, float& m, float& v, const float g, const AdamScalars& s) {
    float pp = p, mm = m, vv = v;
    adam_elem(pp, mm, vv, g, s);
    if (vis) { p = pp; m = mm; v = vv; }
}

// narrow rows. W: the row width (0: a run-time width, w)
template <int W>
__device__ __forceinline__ void rows_flat(const lfs_adam_tensor& t, const AdamScalars& s, const uint64_t w, const uint32_t* __restrict__ bits,
                                          const int64_t worker, const int64_t n_workers) {
    const uint64_t width = W ? uint64_t(W) : w;
    const auto vis = [&](const int64_t e) { const uint64_t g = uint64_t(e) / width; return ((bits[g >> 5] >> (g & 31u)) & 1u) != 0u; };   // g < N: e < N * width
    const int64_t n = t.n_elements;
    if (aligned16(t)) {
        const int64_t n4 = n >> 2;
        for (int64_t i = worker; i < n4; i += n_workers) {
            const bool v0 = vis(4 * i), v1 = vis(4 * i + 1), v2 = vis(4 * i + 2), v3 = vis(4 * i + 3);
            if (!(v0 || v1 || v2 || v3)) continue;
            float4 p = reinterpret_cast<float4*>(t.param)[i];
            float4 m = reinterpret_cast<float4*>(t.exp_avg)[i];
            float4 v = reinterpret_cast<float4*>(t.exp_avg_sq)[i];
            const float4 g = reinterpret_cast<const float4*>(t.grad)[i];
            adam_elem_if(v0, p.x, m.x, v.x, g.x, s); adam_elem_if(v1, p.y, m.y, v.y, g.y, s);
            adam_elem_if(v2, p.z, m.z, v.z, g.z, s); adam_elem_if(v3, p.w, m.w, v.w, g.w, s);
            reinterpret_cast<float4*>(t.param)[i] = p;
            reinterpret_cast<float4*>(t.exp_avg)[i] = m;
            reinterpret_cast<float4*>(t.exp_avg_sq)[i] = v;
        }
        for (int64_t i = (n4 << 2) + worker; i < n; i += n_workers)
            if (vis(i)) adam_elem(t.param[i], t.exp_avg[i], t.exp_avg_sq[i], t.grad[i], s);
    } else {
        for (int64_t i = worker; i < n; i += n_workers)
            if (vis(i)) adam_elem(t.param[i], t.exp_avg[i], t.exp_avg_sq[i], t.grad[i], s);
    }
}

// position of the k-th (from 0) set bit of m; k < popcount(m)
__device__ __forceinline__ uint32_t kth_set_bit(const uint64_t m, uint32_t k) {
    uint32_t pos = 0;
#pragma unroll
    for (uint32_t step = 32; step != 0; step >>= 1) {
        const uint32_t c = uint32_t(__popcll((m >> pos) & ((1ull << step) - 1ull)));
        if (k >= c) { k -= c; pos += step; }
    }
    return pos;
}

// wide rows: wave `wave` of `n_waves` takes the blocks of 64 Gaussians wave, wave + n_waves, ... (both wave-uniform)
__device__ __forceinline__ void rows_wide(const lfs_adam_tensor& t, const AdamScalars& s, const uint32_t w, const uint32_t* __restrict__ bits, const uint32_t N,
                                          const uint32_t wave, const uint32_t n_waves, const uint32_t lane) {
    const uint32_t n_blocks = (N + 63u) / 64u, n_words = (N + 31u) / 32u;
    const bool aligned = aligned16(t);
    for (uint32_t b = wave; b < n_blocks; b += n_waves) {
        uint64_t mask = bits[2u * b];
        if (2u * b + 1u < n_words) mask |= uint64_t(bits[2u * b + 1u]) << 32;
        const uint32_t rows = N - 64u * b;                      // (of the last block: fewer than 64; a bit at or past N addresses nothing)
        if (rows < 64u) mask &= (1ull << rows) - 1ull;
        if (mask == 0ull) continue;
        const int64_t first = int64_t(b) * 64 * w;              // the block's first element
        if (aligned && mask == ~0ull) {                         // 64 visible rows: one span of 16 w float4, 256-byte aligned
            float4* const p4 = reinterpret_cast<float4*>(t.param + first);
            float4* const m4 = reinterpret_cast<float4*>(t.exp_avg + first);
            float4* const v4 = reinterpret_cast<float4*>(t.exp_avg_sq + first);
            const float4* const g4 = reinterpret_cast<const float4*>(t.grad + first);
            for (uint32_t i = lane; i < 16u * w; i += 64u) {
                float4 p = p4[i], m = m4[i], v = v4[i];
                const float4 g = g4[i];
                adam_elem(p.x, m.x, v.x, g.x, s); adam_elem(p.y, m.y, v.y, g.y, s);
                adam_elem(p.z, m.z, v.z, g.z, s); adam_elem(p.w, m.w, v.w, g.w, s);
                p4[i] = p; m4[i] = m; v4[i] = v;
            }
            continue;
        }
        const uint32_t total = uint32_t(__popcll(mask)) * w;    // (visible Gaussian, element) pairs of the block
        const uint32_t pos = kth_set_bit(mask, lane);           // lane r: the row of the r-th visible Gaussian (meaningless past the count, never asked for)
        for (uint32_t base = 0; base < total; base += 64u) {
            const uint32_t item = base + lane, k = item / w, c = item - k * w;
            const uint32_t row = uint32_t(__shfl(int(pos), int(k & 63u)));   // (every lane takes part; k < 64 wherever item < total)
            if (item < total) {
                const int64_t e = first + int64_t(row) * w + c;
                adam_elem(t.param[e], t.exp_avg[e], t.exp_avg_sq[e], t.grad[e], s);
            }
        }
    }
}

__global__ void __launch_bounds__(256, 8) adam_multi_visible_kernel(const Multi a) {   // (8 waves per SIMD: 64 VGPRs, as the streaming kernels of adam.hip)
    int ti = 0;
#pragma unroll
    for (int k = 1; k < LFS_ADAM_MAX_TENSORS; ++k) if (k < a.n && int32_t(blockIdx.x) >= a.block_begin[k]) ti = k;
    const lfs_adam_tensor& t = a.t[ti];
    const AdamScalars s{t.lr, t.beta1, t.beta2, t.eps, t.bias_correction1_rcp, t.bias_correction2_sqrt_rcp};
    const uint32_t w = a.width[ti];
    const uint32_t block = uint32_t(int32_t(blockIdx.x) - a.block_begin[ti]), n_blocks = uint32_t(a.block_begin[ti + 1] - a.block_begin[ti]);
    if (w >= WIDE_MIN && w <= WIDE_MAX) {
        const uint32_t wave = uint32_t(__builtin_amdgcn_readfirstlane(block * 4u + (threadIdx.x >> 6)));
        rows_wide(t, s, w, a.bits, a.N, wave, n_blocks * 4u, threadIdx.x & 63u);
        return;
    }
    const int64_t worker = int64_t(block) * 256 + threadIdx.x, n_workers = int64_t(n_blocks) * 256;
    switch (w) {
    case 1: rows_flat<1>(t, s, 1, a.bits, worker, n_workers); break;
    case 3: rows_flat<3>(t, s, 3, a.bits, worker, n_workers); break;
    case 4: rows_flat<4>(t, s, 4, a.bits, worker, n_workers); break;
    default: rows_flat<0>(t, s, w, a.bits, worker, n_workers); break;
    }
}

} // namespace adamv
} // namespace lfs

extern "C" uint32_t lfs_visibility_words(uint32_t N) { return N / 32u + (N % 32u != 0u ? 1u : 0u); }

extern "C" int lfs_fastgs_view_visibility(const lfs_fastgs_view* view, uint32_t* bits, int accumulate, lfs_stream_t stream) {
    if (!view) return LFS_E_INVALID;
    const uint32_t N = view->N;
    if (N == 0) return LFS_OK;
    if (!view->primitive_workspace || !bits || view->width == 0 || view->height == 0) return LFS_E_INVALID;
    const lfs::fgs::PrimWs w = lfs::fgs::prim_ws(view->primitive_workspace, N, view->width, view->height);
    if (view->primitive_workspace_bytes < w.bytes) return LFS_E_WORKSPACE;
    lfs::ProfScope prof("fastgs_visibility", (hipStream_t)stream);
    hipLaunchKernelGGL(lfs::adamv::visibility_kernel, dim3(N / 256u + (N % 256u != 0u ? 1u : 0u)), dim3(256), 0, (hipStream_t)stream, N, w.n_touched, bits,
                       accumulate != 0 ? 1 : 0);
    return (int)hipGetLastError();
}

extern "C" int lfs_adam_step_multi_visible(const lfs_adam_tensor* tensors, int32_t n_tensors, const uint32_t* visible_bits, uint32_t N, lfs_stream_t stream) {
    if (n_tensors == 0) return LFS_OK;
    if (!tensors || n_tensors < 0 || n_tensors > LFS_ADAM_MAX_TENSORS) return LFS_E_INVALID;
    if (N > 0 && !visible_bits) return LFS_E_INVALID;
    int64_t total = 0;
    for (int i = 0; i < n_tensors; ++i) {
        const lfs_adam_tensor& t = tensors[i];
        if (t.n_elements <= 0) continue;
        if (!t.param || !t.exp_avg || !t.exp_avg_sq || !t.grad) return LFS_E_INVALID;
        if (N == 0 || t.n_elements % int64_t(N) != 0 || t.n_elements / int64_t(N) > int64_t(UINT32_MAX)) return LFS_E_INVALID;
        total += t.n_elements;
    }
    if (total == 0) return LFS_OK;
    lfs::adamv::Multi a;
    a.n = 0; a.block_begin[0] = 0; a.bits = visible_bits; a.N = N;
    // share ~2048 workgroups (adam_blocks' cap: eight per CU, what 64 VGPRs keep resident) between the tensors in proportion to their size, as lfs_adam_step_multi
    // does; a workgroup of a wide tensor is four waves = four blocks of 64 rows per trip
    for (int i = 0; i < n_tensors; ++i) {
        const lfs_adam_tensor& t = tensors[i];
        if (t.n_elements <= 0) continue;
        const uint32_t w = uint32_t(t.n_elements / int64_t(N));
        const bool wide = w >= lfs::adamv::WIDE_MIN && w <= lfs::adamv::WIDE_MAX;
        int64_t b = (t.n_elements * 2048 + total - 1) / total;
        const int64_t bmax = wide ? ((int64_t(N) + 63) / 64 + 3) / 4 : (t.n_elements / 4 + 255) / 256;
        if (b > bmax) b = bmax;
        if (b < 1) b = 1;
        a.t[a.n] = t;
        a.width[a.n] = w;
        a.block_begin[a.n + 1] = a.block_begin[a.n] + int32_t(b);
        ++a.n;
    }
    lfs::ProfScope prof("adam_multi_visible", (hipStream_t)stream);
    hipLaunchKernelGGL(lfs::adamv::adam_multi_visible_kernel, dim3(a.block_begin[a.n]), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
