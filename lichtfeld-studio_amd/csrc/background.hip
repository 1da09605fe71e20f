// Background colour on the EWA route: the compose stage between the fastgs forward and the loss, its backward, and the RGBA target.
//   render group   shown_c  = image_c + (1 - alpha) * bg_c                       (fast_rasterizer.cpp:60-66, the expression of fastgs.fast_rasterize)
//   target group   out_c    = a * t_c + (1 - a) * bg_c,  a = (float)u8 / 255     (a == 0: out = bg exactly; a == 255: out = t exactly)
//   backward       v_alpha  = [v_alpha_in] - ((v_0 bg_0 + v_1 bg_1) + v_2 bg_2)  (dL/d(image) is v_shown itself: nothing is copied)
// The colour is three floats BY VALUE in the args struct: kernel arguments, read through the scalar unit - no device tensor, no host read. The planes are contiguous,
// so the kernels index the flattened H*W plane. Two forms of each kernel, chosen on the host (as st_sh_kernel<deg, vec> is):
//   VEC     every plane base involved is 16-byte aligned (the tensor bases are and H*W % 4 == 0; the u8 plane's base 4-byte aligned): a lane takes 4 consecutive pixels
//           with one 16-byte access per float plane and one 4-byte load for the four alpha bytes;
//   scalar  otherwise: a lane takes 4 pixels one block width apart (pixel = 1024 block + 256 k + lane, k = 0..3) so that every 4-byte access of a wave is coalesced,
//           each with its own bounds test (the ragged end needs no separate tail).
// A pixel is read and written by the same lane and by no other: shown == image and v_alpha == v_alpha_in are safe. 256 threads, no LDS, no atomics, no scratch.
// -ffp-contract=off: the arithmetic below is what a float32 host model repeats bit for bit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/lfs_gsplat.h"

static_assert(sizeof(lfs_background_compose_args) == 72, "the ctypes mirror (capi.py: BackgroundComposeArgs) is laid out by hand");
static_assert(sizeof(lfs_background_compose_bwd_args) == 48, "the ctypes mirror (capi.py: BackgroundComposeBwdArgs) is laid out by hand");

namespace lfs {
namespace bgc {

constexpr uint32_t THREADS = 256, PER_LANE = 4, PER_BLOCK = THREADS * PER_LANE;

struct Color { float r, g, b; };

__device__ __forceinline__ float over(const float x, const float alpha, const float bg) { return x + (1.0f - alpha) * bg; }
__device__ __forceinline__ float mix(const float t, const float a, const float bg) { return a * t + (1.0f - a) * bg; }

__device__ __forceinline__ float4 over4(const float4 x, const float4 al, const float bg) {
    return make_float4(over(x.x, al.x, bg), over(x.y, al.y, bg), over(x.z, al.z, bg), over(x.w, al.w, bg));
}
__device__ __forceinline__ float4 mix4(const float4 t, const float4 a, const float bg) {
    return make_float4(mix(t.x, a.x, bg), mix(t.y, a.y, bg), mix(t.z, a.z, bg), mix(t.w, a.w, bg));
}

// n = H*W (< 2^31). Either group's pointers may be NULL (wave-uniform tests on kernel arguments).
template <bool VEC>
__global__ void __launch_bounds__(THREADS) compose_kernel(const uint32_t n, const Color bg, const float* image, const float* alpha, float* shown,
                                                          const float* target_rgb, const uint8_t* target_alpha, float* target_out) {
    const float c[3] = {bg.r, bg.g, bg.b};
    if (VEC) {
        const uint32_t p = (blockIdx.x * THREADS + threadIdx.x) * PER_LANE;   // n % 4 == 0: a quad is inside or outside as a whole
        if (p >= n) return;
        if (image) {
            const float4 al = *reinterpret_cast<const float4*>(alpha + p);
            float4 x[3];   // every load before the first store: shown may be image, and the compiler must not be made to order them plane by plane
#pragma unroll
            for (uint32_t k = 0; k < 3; ++k) x[k] = *reinterpret_cast<const float4*>(image + (size_t)k * n + p);
#pragma unroll
            for (uint32_t k = 0; k < 3; ++k) *reinterpret_cast<float4*>(shown + (size_t)k * n + p) = over4(x[k], al, c[k]);
        }
        if (target_rgb) {
            const uint32_t u = *reinterpret_cast<const uint32_t*>(target_alpha + p);   // little-endian: byte j is pixel p + j
            const float4 a = make_float4((float)(u & 255u) / 255.0f, (float)((u >> 8) & 255u) / 255.0f, (float)((u >> 16) & 255u) / 255.0f, (float)(u >> 24) / 255.0f);
            float4 t[3];
#pragma unroll
            for (uint32_t k = 0; k < 3; ++k) t[k] = *reinterpret_cast<const float4*>(target_rgb + (size_t)k * n + p);
#pragma unroll
            for (uint32_t k = 0; k < 3; ++k) *reinterpret_cast<float4*>(target_out + (size_t)k * n + p) = mix4(t[k], a, c[k]);
        }
    } else {
        const uint32_t p0 = blockIdx.x * PER_BLOCK + threadIdx.x;
#pragma unroll
        for (uint32_t j = 0; j < PER_LANE; ++j) {
            const uint32_t p = p0 + j * THREADS;
            if (p >= n) break;
            if (image) {
                const float al = alpha[p];
#pragma unroll
                for (uint32_t k = 0; k < 3; ++k) shown[(size_t)k * n + p] = over(image[(size_t)k * n + p], al, c[k]);
            }
            if (target_rgb) {
                const float a = (float)target_alpha[p] / 255.0f;
#pragma unroll
                for (uint32_t k = 0; k < 3; ++k) target_out[(size_t)k * n + p] = mix(target_rgb[(size_t)k * n + p], a, c[k]);
            }
        }
    }
}

__device__ __forceinline__ float dot_bg(const float v0, const float v1, const float v2, const Color bg) { return (v0 * bg.r + v1 * bg.g) + v2 * bg.b; }

template <bool VEC>
__global__ void __launch_bounds__(THREADS) compose_bwd_kernel(const uint32_t n, const Color bg, const float* v_shown, const float* v_alpha_in, float* v_alpha) {
    if (VEC) {
        const uint32_t p = (blockIdx.x * THREADS + threadIdx.x) * PER_LANE;
        if (p >= n) return;
        const float4 a = *reinterpret_cast<const float4*>(v_shown + p), b = *reinterpret_cast<const float4*>(v_shown + (size_t)n + p),
                     c = *reinterpret_cast<const float4*>(v_shown + 2 * (size_t)n + p);
        const float4 d = make_float4(dot_bg(a.x, b.x, c.x, bg), dot_bg(a.y, b.y, c.y, bg), dot_bg(a.z, b.z, c.z, bg), dot_bg(a.w, b.w, c.w, bg));
        float4 o;
        if (v_alpha_in) {
            const float4 i = *reinterpret_cast<const float4*>(v_alpha_in + p);
            o = make_float4(i.x - d.x, i.y - d.y, i.z - d.z, i.w - d.w);
        } else {
            o = make_float4(-d.x, -d.y, -d.z, -d.w);
        }
        *reinterpret_cast<float4*>(v_alpha + p) = o;
    } else {
        const uint32_t p0 = blockIdx.x * PER_BLOCK + threadIdx.x;
#pragma unroll
        for (uint32_t j = 0; j < PER_LANE; ++j) {
            const uint32_t p = p0 + j * THREADS;
            if (p >= n) break;
            const float d = dot_bg(v_shown[p], v_shown[(size_t)n + p], v_shown[2 * (size_t)n + p], bg);
            v_alpha[p] = v_alpha_in ? v_alpha_in[p] - d : -d;
        }
    }
}

static bool aligned(const void* p, const uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// -> H*W, or 0 when the extents or the colour are refused
static uint32_t checked_extent(const uint32_t h, const uint32_t w, const float* bg) {
    if (h == 0 || w == 0) return 0;
    const uint64_t n = (uint64_t)h * w;
    if (n >= (1ull << 31)) return 0;
    for (int i = 0; i < 3; ++i) if (!isfinite(bg[i])) return 0;
    return (uint32_t)n;
}

} // namespace bgc
} // namespace lfs

using namespace lfs;

extern "C" int lfs_background_compose(const lfs_background_compose_args* a, lfs_stream_t stream) {
    if (!a) return LFS_E_INVALID;
    const uint32_t n = bgc::checked_extent(a->height, a->width, a->bg);
    if (n == 0) return LFS_E_INVALID;
    const bool render = a->image || a->alpha || a->shown, target = a->target_rgb || a->target_alpha || a->target_out;
    if (!render && !target) return LFS_E_INVALID;
    if (render && !(a->image && a->alpha && a->shown)) return LFS_E_INVALID;                    // half a group
    if (target && !(a->target_rgb && a->target_alpha && a->target_out)) return LFS_E_INVALID;
    if (target && a->target_out == a->target_rgb) return LFS_E_INVALID;                         // the resident image is reused every epoch
    bool vec = (n % 4u) == 0;
    if (render) vec = vec && bgc::aligned(a->image, 16) && bgc::aligned(a->alpha, 16) && bgc::aligned(a->shown, 16);
    if (target) vec = vec && bgc::aligned(a->target_rgb, 16) && bgc::aligned(a->target_alpha, 4) && bgc::aligned(a->target_out, 16);
    const bgc::Color bg = {a->bg[0], a->bg[1], a->bg[2]};
    const uint32_t blocks = (n + bgc::PER_BLOCK - 1) / bgc::PER_BLOCK;
    hipStream_t s = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL((bgc::compose_kernel<true>), dim3(blocks), dim3(bgc::THREADS), 0, s, n, bg, a->image, a->alpha, a->shown, a->target_rgb, a->target_alpha, a->target_out);
    else hipLaunchKernelGGL((bgc::compose_kernel<false>), dim3(blocks), dim3(bgc::THREADS), 0, s, n, bg, a->image, a->alpha, a->shown, a->target_rgb, a->target_alpha, a->target_out);
    return (int)hipGetLastError();
}

extern "C" int lfs_background_compose_bwd(const lfs_background_compose_bwd_args* a, lfs_stream_t stream) {
    if (!a) return LFS_E_INVALID;
    const uint32_t n = bgc::checked_extent(a->height, a->width, a->bg);
    if (n == 0 || !a->v_shown || !a->v_alpha) return LFS_E_INVALID;
    const bool vec = (n % 4u) == 0 && bgc::aligned(a->v_shown, 16) && bgc::aligned(a->v_alpha, 16) && (!a->v_alpha_in || bgc::aligned(a->v_alpha_in, 16));
    const bgc::Color bg = {a->bg[0], a->bg[1], a->bg[2]};
    const uint32_t blocks = (n + bgc::PER_BLOCK - 1) / bgc::PER_BLOCK;
    hipStream_t s = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL((bgc::compose_bwd_kernel<true>), dim3(blocks), dim3(bgc::THREADS), 0, s, n, bg, a->v_shown, a->v_alpha_in, a->v_alpha);
    else hipLaunchKernelGGL((bgc::compose_bwd_kernel<false>), dim3(blocks), dim3(bgc::THREADS), 0, s, n, bg, a->v_shown, a->v_alpha_in, a->v_alpha);
    return (int)hipGetLastError();
}
