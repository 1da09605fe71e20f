// ADMM sparsity optimisation (the reference's src/training/components/sparsity_optimizer.cpp: prune_z, update_state, compute_loss + backward, get_prune_mask)
// as fixed-size device passes: no sort, no host read, no float atomic - the same bits on every run.
//
//  * select: the k-th smallest of N floats by a 4-pass most-significant-digit radix SELECT over an order-preserving 32-bit key (torch.sort's order: -0 == +0,
//    any NaN above +inf). A pass counts the 8-bit digit of the keys that still match the digits chosen so far in a per-workgroup LDS histogram and flushes the
//    non-empty bins with integer atomics; a one-wave kernel then scans the 256 bins, picks the digit that holds the rank and leaves (prefix, residual rank) in the
//    workspace for the next pass. 4 x N key reads against the ~2 x 4 x N reads + writes of a radix sort, and nothing but one float comes out.
//  * update: v = sigmoid(raw) + u is written to the workspace by the FIRST histogram pass (so the select runs over the very values that are thresholded
//    afterwards), then one pass writes z = v > thr ? v : 0 and u += sigmoid(raw) - z.
//  * loss + gradient: one pass; the sum of d^2 goes thread -> wave (xor tree) -> workgroup -> a second one-workgroup kernel, all in a fixed order.
//  * prune mask: select on the RAW opacities, then one workgroup walks the array in order and hands the ties at the boundary value to the lowest indices.
//
// Grids are sized for the device (256 CUs x 4 resident workgroups), not for N: every streaming kernel is a grid-stride loop over at most MAX_BLOCKS workgroups.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/lfs_gsplat.h"
#include "lfs_math.cuh"
#include "lfs_prof.h"

namespace lfs {
namespace sparsity {

constexpr int THREADS = 256;
constexpr uint32_t MAX_BLOCKS = 1024;
constexpr int PASSES = 4, BINS = 256;
constexpr int MASK_ITEMS = 4;                                   // elements per thread and round of the ordered mask pass
// select workspace: hist[PASSES][BINS] u32 | state[64] u32 (0: key prefix, 1: residual rank, 2: key of the result, 3: rank of the result among equal keys)
constexpr size_t HIST_BYTES = (size_t)PASSES * BINS * sizeof(uint32_t);
constexpr size_t SELECT_BYTES = HIST_BYTES + 256;
constexpr size_t THR_BYTES = 256;                               // the selected value (one float), on a line of its own

// order-preserving key of torch.sort's order on floats: negative values bit-flipped, non-negative ones get the sign bit; -0 is +0; a NaN of either sign keeps its
// payload and sorts above +inf
LFS_DI uint32_t order_key(float x) {
    uint32_t b = __float_as_uint(x);
    if ((b & 0x7fffffffu) > 0x7f800000u) return b | 0x80000000u;
    if (b == 0x80000000u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
LFS_DI float key_value(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// FROM_RAW: the value is sigmoid(raw[i]) + u[i], stored to vbuf[i] on the way (pass 0 of the ADMM update); otherwise x[i]
template <bool FROM_RAW>
__global__ void __launch_bounds__(THREADS) select_hist_kernel(int64_t N, const float* __restrict__ x, const float* __restrict__ u, float* __restrict__ vbuf, int pass,
                                                              const uint32_t* __restrict__ state, uint32_t* __restrict__ hist) {
    __shared__ uint32_t s_hist[BINS];
    s_hist[threadIdx.x] = 0u;
    __syncthreads();
    const int shift = 24 - 8 * pass;
    const uint32_t himask = pass == 0 ? 0u : 0xffffffffu << (shift + 8);
    const uint32_t prefix = pass == 0 ? 0u : state[0];
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < N; i += (int64_t)gridDim.x * THREADS) {
        float v;
        if (FROM_RAW) { v = sigmoid(x[i]) + u[i]; vbuf[i] = v; }
        else v = x[i];
        const uint32_t key = order_key(v);
        if ((key & himask) == prefix) atomicAdd(&s_hist[(key >> shift) & 0xffu], 1u);
    }
    __syncthreads();
    const uint32_t c = s_hist[threadIdx.x];
    if (c) atomicAdd(&hist[pass * BINS + threadIdx.x], c);
}

// one wave: lane l owns bins 4 l .. 4 l + 3. The lane whose bins hold the rank extends the prefix by its digit and leaves the rank within that digit.
__global__ void __launch_bounds__(64) select_pick_kernel(int pass, uint32_t k, uint32_t* __restrict__ state, const uint32_t* __restrict__ hist, float* __restrict__ out_value) {
    const int lane = threadIdx.x;
    const uint32_t rank = pass == 0 ? k : state[1];
    const uint32_t prefix = pass == 0 ? 0u : state[0];
    uint32_t c[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] = hist[pass * BINS + 4 * lane + j];
    const uint32_t s = c[0] + c[1] + c[2] + c[3];
    uint32_t incl = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(incl, d);
        if (lane >= d) incl += t;
    }
    const uint32_t excl = incl - s;
    if (excl < rank && rank <= incl) {             // exactly one lane: the bins of a pass hold every key the previous digit's bin held, and 1 <= rank <= that count
        uint32_t r = rank - excl;
        int j = 0;
        while (j < 3 && r > c[j]) { r -= c[j]; ++j; }
        const uint32_t p = prefix | ((uint32_t)(4 * lane + j) << (24 - 8 * pass));
        state[0] = p;
        state[1] = r;
        if (pass == PASSES - 1) {
            state[2] = p;
            state[3] = r;
            out_value[0] = key_value(p);
        }
    }
}

// z = v > thr ? v : 0 ; u = u + (opa - z)   (sparsity_optimizer.cpp:83-86, :167); zero_all: prune_z's index == 0 -> z = 0
__global__ void __launch_bounds__(THREADS) admm_apply_kernel(int64_t N, const float* __restrict__ raw, float* __restrict__ u, float* __restrict__ z,
                                                             const float* __restrict__ vbuf, const float* __restrict__ thr_p, const bool zero_all) {
    const float thr = zero_all ? 0.f : thr_p[0];
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < N; i += (int64_t)gridDim.x * THREADS) {
        const float opa = sigmoid(raw[i]);
        float zz = 0.f;
        if (!zero_all) { const float v = vbuf[i]; zz = v > thr ? v : 0.f; }
        z[i] = zz;
        u[i] = u[i] + (opa - zz);
    }
}

// d = (opa - z) + u ; g (+)= ((scale rho) d) opa (1 - opa) ; partial[block] = sum d^2 in the order thread (grid stride) -> wave xor tree -> the four waves
template <bool ACCUM>
__global__ void __launch_bounds__(THREADS) admm_loss_grad_kernel(int64_t N, const float* __restrict__ raw, const float* __restrict__ z, const float* __restrict__ u,
                                                                 const float sr, float* __restrict__ g, float* __restrict__ partial) {
    __shared__ float s_part[THREADS / 64];
    float acc = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < N; i += (int64_t)gridDim.x * THREADS) {
        float om;                                  // 1 - opa, accurate where opa rounds towards 1 (a plain 1.f - opa has lost most of its bits there)
        const float opa = sigmoid(raw[i], om);
        const float d = (opa - z[i]) + u[i];
        acc += d * d;
        const float gi = sr * d * opa * om;
        if (ACCUM) g[i] += gi; else g[i] = gi;
    }
    if (partial == nullptr) return;                // (uniform over the grid)
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]);
}

// loss += factor * sum(partial[0 .. P))   one workgroup: strided per-thread sums, then the same tree
__global__ void __launch_bounds__(THREADS) admm_loss_fold_kernel(uint32_t P, const float* __restrict__ partial, const float factor, float* __restrict__ loss) {
    __shared__ float s_part[THREADS / 64];
    float acc = 0.f;
    for (uint32_t i = threadIdx.x; i < P; i += THREADS) acc += partial[i];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) loss[0] += factor * ((s_part[0] + s_part[1]) + (s_part[2] + s_part[3]));
}

// mask[i] = key(raw[i]) < key(thr), or == and among the first `need` of the equal ones in index order. ONE workgroup walks the array in order
// (THREADS x MASK_ITEMS elements per round, the ties counted by a block scan plus the carry of the rounds before): it runs once per training run.
__global__ void __launch_bounds__(THREADS) prune_mask_kernel(int64_t N, const float* __restrict__ raw, const uint32_t* __restrict__ state, uint8_t* __restrict__ mask) {
    __shared__ uint32_t s_wave[THREADS / 64];
    const uint32_t thr_key = state[2], need = state[3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t carry = 0u;
    for (int64_t base = 0; base < N; base += (int64_t)THREADS * MASK_ITEMS) {
        const int64_t i0 = base + (int64_t)threadIdx.x * MASK_ITEMS;
        bool lt[MASK_ITEMS], tie[MASK_ITEMS];
        uint32_t c = 0u;
#pragma unroll
        for (int j = 0; j < MASK_ITEMS; ++j) {
            const bool valid = i0 + j < N;
            const uint32_t key = valid ? order_key(raw[i0 + j]) : 0u;
            lt[j] = valid && key < thr_key;
            tie[j] = valid && key == thr_key;
            c += tie[j] ? 1u : 0u;
        }
        uint32_t incl = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t t = __shfl_up(incl, d);
            if (lane >= d) incl += t;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        uint32_t before = carry, total = 0u;
#pragma unroll
        for (int w = 0; w < THREADS / 64; ++w) { if (w < wave) before += s_wave[w]; total += s_wave[w]; }
        uint32_t seen = before + incl - c;         // equal keys at lower indices
#pragma unroll
        for (int j = 0; j < MASK_ITEMS; ++j) {
            if (i0 + j < N) mask[i0 + j] = (lt[j] || (tie[j] && seen < need)) ? 1 : 0;
            if (tie[j]) ++seen;
        }
        carry += total;
        __syncthreads();                           // s_wave is rewritten by the next round
    }
}

static inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }
static inline bool count_ok(int64_t N) { return N >= 0 && N <= 0x7fffffffll; }      // ranks and bin counts are 32-bit
static inline uint32_t blocks_for(int64_t N) {
    const int64_t b = (N + THREADS - 1) / THREADS;
    return (uint32_t)(b < 1 ? 1 : (b > (int64_t)MAX_BLOCKS ? (int64_t)MAX_BLOCKS : b));
}

// the select, enqueued: `first_from_raw` makes pass 0 compute and store v = sigmoid(x) + u. ws = SELECT_BYTES, out_value = device float.
static void enqueue_select(hipStream_t s, int64_t N, uint32_t k, const float* x, const float* u, float* vbuf, bool first_from_raw, void* ws, float* out_value) {
    uint32_t* hist = (uint32_t*)ws;
    uint32_t* state = (uint32_t*)((char*)ws + HIST_BYTES);
    (void)hipMemsetAsync(ws, 0, SELECT_BYTES, s);
    const dim3 grid(blocks_for(N)), block(THREADS);
    for (int pass = 0; pass < PASSES; ++pass) {
        if (pass == 0 && first_from_raw)
            hipLaunchKernelGGL(select_hist_kernel<true>, grid, block, 0, s, N, x, u, vbuf, pass, (const uint32_t*)state, hist);
        else
            hipLaunchKernelGGL(select_hist_kernel<false>, grid, block, 0, s, N, first_from_raw ? (const float*)vbuf : x, (const float*)nullptr, (float*)nullptr, pass,
                               (const uint32_t*)state, hist);
        hipLaunchKernelGGL(select_pick_kernel, dim3(1), dim3(64), 0, s, pass, k, state, (const uint32_t*)hist, out_value);
    }
}

} // namespace sparsity
} // namespace lfs

using namespace lfs::sparsity;

extern "C" size_t lfs_select_kth_workspace_bytes(int64_t N) { return count_ok(N) ? SELECT_BYTES : 0; }

extern "C" int lfs_select_kth_f32(const float* x, int64_t N, int64_t k, float* out_value, void* workspace, size_t workspace_bytes, lfs_stream_t stream) {
    if (!count_ok(N)) return LFS_E_INVALID;
    if (N == 0) return LFS_OK;
    if (k < 1 || k > N || !x || !out_value || !workspace || ((uintptr_t)workspace & 15)) return LFS_E_INVALID;
    if (workspace_bytes < lfs_select_kth_workspace_bytes(N)) return LFS_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    lfs::ProfScope prof("select_kth", s);
    enqueue_select(s, N, (uint32_t)k, x, nullptr, nullptr, false, workspace, out_value);
    return (int)hipGetLastError();
}

extern "C" size_t lfs_admm_update_workspace_bytes(int64_t N) { return count_ok(N) ? SELECT_BYTES + THR_BYTES + align256((size_t)N * sizeof(float)) : 0; }

extern "C" int lfs_admm_update(const float* raw_opacities, float* u, float* z, int64_t N, int64_t k, void* workspace, size_t workspace_bytes, lfs_stream_t stream) {
    if (!count_ok(N)) return LFS_E_INVALID;
    if (N == 0) return LFS_OK;
    if (k < 0 || k > N || !raw_opacities || !u || !z || !workspace || ((uintptr_t)workspace & 15)) return LFS_E_INVALID;
    if (workspace_bytes < lfs_admm_update_workspace_bytes(N)) return LFS_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    float* thr = (float*)((char*)workspace + SELECT_BYTES);
    float* vbuf = (float*)((char*)workspace + SELECT_BYTES + THR_BYTES);
    lfs::ProfScope prof("admm_update", s);
    if (k > 0) enqueue_select(s, N, (uint32_t)k, raw_opacities, u, vbuf, true, workspace, thr);
    hipLaunchKernelGGL(admm_apply_kernel, dim3(blocks_for(N)), dim3(THREADS), 0, s, N, raw_opacities, u, z, (const float*)vbuf, (const float*)thr, k == 0);
    return (int)hipGetLastError();
}

extern "C" size_t lfs_admm_loss_grad_workspace_bytes(int64_t N) { return count_ok(N) ? align256((size_t)MAX_BLOCKS * sizeof(float)) : 0; }

extern "C" int lfs_admm_loss_grad(const float* raw_opacities, const float* z, const float* u, int64_t N, float rho, float scale, float* g_raw_opacities, int accumulate,
                                  float* loss, void* workspace, size_t workspace_bytes, lfs_stream_t stream) {
    if (!count_ok(N)) return LFS_E_INVALID;
    if (N == 0) return LFS_OK;
    if (!raw_opacities || !z || !u || !g_raw_opacities) return LFS_E_INVALID;
    if (loss) {
        if (!workspace || ((uintptr_t)workspace & 15)) return LFS_E_INVALID;
        if (workspace_bytes < lfs_admm_loss_grad_workspace_bytes(N)) return LFS_E_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    const uint32_t P = blocks_for(N);
    float* partial = loss ? (float*)workspace : nullptr;
    const float sr = scale * rho;
    lfs::ProfScope prof("admm_loss_grad", s);
    if (accumulate) hipLaunchKernelGGL(admm_loss_grad_kernel<true>, dim3(P), dim3(THREADS), 0, s, N, raw_opacities, z, u, sr, g_raw_opacities, partial);
    else hipLaunchKernelGGL(admm_loss_grad_kernel<false>, dim3(P), dim3(THREADS), 0, s, N, raw_opacities, z, u, sr, g_raw_opacities, partial);
    if (loss) hipLaunchKernelGGL(admm_loss_fold_kernel, dim3(1), dim3(THREADS), 0, s, P, (const float*)partial, scale * 0.5f * rho, loss);
    return (int)hipGetLastError();
}

extern "C" size_t lfs_admm_prune_mask_workspace_bytes(int64_t N) { return count_ok(N) ? SELECT_BYTES + THR_BYTES : 0; }

// The reference takes topk(sigmoid(raw), n_prune, largest = false) (sparsity_optimizer.cpp:110-123). sigmoid is monotone (non-decreasing also after rounding), so the
// n_prune smallest RAW opacities are n_prune smallest activated ones: selecting on the raw values is one of the results topk may return, and the only difference is
// which of several equal activated opacities go - which topk leaves unspecified as well.
extern "C" int lfs_admm_prune_mask(const float* raw_opacities, int64_t N, int64_t n_prune, uint8_t* mask_u8, void* workspace, size_t workspace_bytes, lfs_stream_t stream) {
    if (!count_ok(N)) return LFS_E_INVALID;
    if (N == 0) return LFS_OK;
    if (n_prune < 0 || n_prune > N || !raw_opacities || !mask_u8 || !workspace || ((uintptr_t)workspace & 15)) return LFS_E_INVALID;
    if (workspace_bytes < lfs_admm_prune_mask_workspace_bytes(N)) return LFS_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (n_prune == 0) return (int)hipMemsetAsync(mask_u8, 0, (size_t)N, s);
    float* thr = (float*)((char*)workspace + SELECT_BYTES);
    const uint32_t* state = (const uint32_t*)((char*)workspace + HIST_BYTES);
    lfs::ProfScope prof("admm_prune_mask", s);
    enqueue_select(s, N, (uint32_t)n_prune, raw_opacities, nullptr, nullptr, false, workspace, thr);
    hipLaunchKernelGGL(prune_mask_kernel, dim3(1), dim3(THREADS), 0, s, N, raw_opacities, state, mask_u8);
    return (int)hipGetLastError();
}
