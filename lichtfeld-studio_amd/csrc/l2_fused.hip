// Fused L2 glue (extensions, not in gsplat/Ops.h): the element-wise libtorch work the reference's trainer wraps
// around the operators, as single HBM passes.
//   * activations fwd / bwd: gs::SplatData::get_rotation / get_scaling / get_opacity
//     (src/core/splat_data.cpp:267-286: normalize, exp, sigmoid) and their autograd backward;
//   * photometric MSE of the clamped render against a CHW target with its gradient in the rasterizer's HWC
//     layout (the rasterizer-only loss of SURVEY.md §8d; rasterizer.cpp:399 clamps the image to [0,1]).
// All of it is HBM-bound streaming: one thread per Gaussian / pixel, 16-byte accesses where the layout allows.
#include "lfs_math.cuh"
#include "lfs_prof.h"
#include "../../include/lfs_gsplat.h"

namespace lfs {

__global__ void __launch_bounds__(256) activations_fwd_kernel(
    const uint32_t N, const float* __restrict__ raw_quats, const float* __restrict__ raw_scales, const float* __restrict__ raw_opacities,
    float* __restrict__ quats, float* __restrict__ scales, float* __restrict__ opacities) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= N) return;
    const float4 q = reinterpret_cast<const float4*>(raw_quats)[g];
    // torch::nn::functional::normalize: x / max(||x||_2, 1e-12)
    const float den = fmaxf(sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w), 1e-12f);
    reinterpret_cast<float4*>(quats)[g] = make_float4(q.x / den, q.y / den, q.z / den, q.w / den); // true divisions, as ATen
#pragma unroll
    for (int k = 0; k < 3; ++k) scales[3 * g + k] = expf(raw_scales[3 * g + k]);
    opacities[g] = sigmoid(raw_opacities[g]);
}

// grads w.r.t. the raw parameters from grads w.r.t. the activated ones. ACCUM adds to the outputs.
template <bool ACCUM>
__global__ void __launch_bounds__(256) activations_bwd_kernel(
    const uint32_t N, const float* __restrict__ raw_quats, const float* __restrict__ scales, const float* __restrict__ opacities,
    const float* __restrict__ v_quats, const float* __restrict__ v_scales, const float* __restrict__ v_opacities,
    const float v_scale_reg, const float v_opacity_reg,
    float* __restrict__ g_raw_quats, float* __restrict__ g_raw_scales, float* __restrict__ g_raw_opacities) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= N) return;
    const float4 q = reinterpret_cast<const float4*>(raw_quats)[g];
    const float4 v = reinterpret_cast<const float4*>(v_quats)[g];
    const float nrm = sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
    float4 gq;
    if (nrm > 1e-12f) { // y = x / n : dx = (v - (v.y) y) / n
        const float inv = 1.f / nrm;
        const float4 y = make_float4(q.x * inv, q.y * inv, q.z * inv, q.w * inv);
        const float d = v.x * y.x + v.y * y.y + v.z * y.z + v.w * y.w;
        gq = make_float4((v.x - d * y.x) * inv, (v.y - d * y.y) * inv, (v.z - d * y.z) * inv, (v.w - d * y.w) * inv);
    } else { // clamped denominator: y = x / 1e-12
        gq = make_float4(v.x * 1e12f, v.y * 1e12f, v.z * 1e12f, v.w * 1e12f);
    }
    float4* gqo = reinterpret_cast<float4*>(g_raw_quats) + g;
    if (ACCUM) { const float4 o = *gqo; gq = make_float4(o.x + gq.x, o.y + gq.y, o.z + gq.z, o.w + gq.w); }
    *gqo = gq;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float gs = (v_scales[3 * g + k] + v_scale_reg) * scales[3 * g + k];
        if (ACCUM) g_raw_scales[3 * g + k] += gs; else g_raw_scales[3 * g + k] = gs;
    }
    const float o = opacities[g];
    const float go = (v_opacities[g] + v_opacity_reg) * o * (1.f - o);
    if (ACCUM) g_raw_opacities[g] += go; else g_raw_opacities[g] = go;
}

// loss += sum((clamp(x,0,1) - t)^2) * inv_numel * weight; v_render = 2 (clamp(x) - t) * inv_numel * weight where 0 <= x <= 1
// (torch::clamp passes the gradient on the closed interval). render HWC, target CHW.
// CHW = true: render / v_render are [3,H,W] and NOT clamped (the fastgs path: fast_rasterizer.cpp hands the image on as is)
// MASKED (lfs_mse_loss_masked_fwd_bwd): every pixel weighted by its mask byte M_p, normalised by 3 * sum(M) read from the device (`scale` is unused:
// the factor is wscale / S_img, a double division rounded to float once, 0 under an empty mask). A compile-time switch of one shared body.
template <bool CHW, bool MASKED>
__device__ __forceinline__ void mse_loss_body(
    const uint32_t H, const uint32_t W, const float* render, const float* target, float scale, float* v_render, float* loss, const bool clamp,
    const uint8_t* mask, const long long* sums, const double wscale, const uint32_t p0, const uint32_t stride) {
    const uint32_t P = H * W;
    float acc = 0.f;
    if constexpr (MASKED) scale = sums[0] > 0 ? float(wscale / double(sums[0])) : 0.f;
    for (uint32_t p = p0; p < P; p += stride) {
        float m = 1.f;
        if constexpr (MASKED) m = float(mask[p]);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const size_t ri = CHW ? size_t(c) * P + p : 3 * size_t(p) + c;
            const float x = render[ri];
            const float d = (clamp ? fminf(fmaxf(x, 0.f), 1.f) : x) - target[size_t(c) * P + p];
            if constexpr (MASKED) {
                acc += m * (d * d);
                v_render[ri] = (m != 0.f && (!clamp || (x >= 0.f && x <= 1.f))) ? 2.f * d * (m * scale) : 0.f;
            } else {
                acc += d * d;
                v_render[ri] = (!clamp || (x >= 0.f && x <= 1.f)) ? 2.f * d * scale : 0.f;
            }
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
    __shared__ float part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(loss, (part[0] + part[1] + part[2] + part[3]) * scale);
}

template <bool CHW>
__global__ void __launch_bounds__(256) mse_loss_kernel(
    const uint32_t H, const uint32_t W, const float* __restrict__ render, const float* __restrict__ target,
    const float scale, float* __restrict__ v_render, float* __restrict__ loss, const bool clamp = !CHW) {
    mse_loss_body<CHW, false>(H, W, render, target, scale, v_render, loss, clamp, nullptr, nullptr, 0.0, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}

template <bool CHW>
__global__ void __launch_bounds__(256) mse_loss_masked_kernel(
    const uint32_t H, const uint32_t W, const float* __restrict__ render, const float* __restrict__ target, const uint8_t* __restrict__ mask,
    const long long* __restrict__ sums, const double wscale, float* __restrict__ v_render, float* __restrict__ loss, const bool clamp) {
    mse_loss_body<CHW, true>(H, W, render, target, 0.f, v_render, loss, clamp, mask, sums, wscale, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}

// Depth supervision (lfs_depth_prepare / lfs_depth_l1_loss_fwd_bwd). A target is valid where it is finite and > 0; the prepared plane carries NaN elsewhere, so the
// loss kernel needs no validity plane. sums[0] = sum_p valid_p M_p (M_p the mask byte, 255 without a mask) = 255 sum_p m_p: integer wave sums and one 64-bit integer
// atomic per block, as mask_prepare_kernel - exact, the same on every run.
// (in and out may be the same plane - preparing in place is part of the contract - so neither is __restrict__; every thread touches its own element only)
__global__ void __launch_bounds__(256) depth_prepare_kernel(const uint32_t P, const float* in, const uint8_t* __restrict__ mask, float* out,
                                                            unsigned long long* __restrict__ sums) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned int m = 0;
    if (p < P) {
        const float t = in[p];
        const bool valid = t > 0.f && t < __builtin_inff();   // (NaN fails both)
        out[p] = valid ? t : __builtin_nanf("");
        m = valid ? (mask ? (unsigned int)mask[p] : 255u) : 0u;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m += __shfl_xor(m, d, 64);
    __shared__ unsigned int part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned int v = part[0] + part[1] + part[2] + part[3];
        if (v) atomicAdd(&sums[0], (unsigned long long)v);
    }
}

// loss_acc += weight sum_p m_p |D_p - t_p| / max(sum m, 1), grad_depth_p = weight m_p sign(D_p - t_p) / max(sum m, 1), m_p = valid_p M_p / 255. With S = sums[0] =
// 255 sum m the common factor is scale = weight / max(S, 255) per unit of M_p (a double division rounded to float once, the same value in every thread); the block
// sums and the atomic are those of mse_loss_body.
__global__ void __launch_bounds__(256) depth_l1_loss_kernel(const uint32_t P, const float* __restrict__ depth, const float* __restrict__ target, const uint8_t* __restrict__ mask,
                                                            const long long* __restrict__ sums, const double weight, float* __restrict__ g_depth, float* __restrict__ loss) {
    const long long S = sums[0];
    const float scale = float(weight / double(S > 255 ? S : 255));
    float acc = 0.f;
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < P; p += gridDim.x * blockDim.x) {
        const float t = target[p];
        float m = mask ? float(mask[p]) : 255.f;
        if (!(t > 0.f)) m = 0.f;                                  // the sentinel of depth_prepare_kernel (NaN), or a target that was never prepared
        const float d = m != 0.f ? depth[p] - t : 0.f;
        acc += m * fabsf(d);
        g_depth[p] = d > 0.f ? m * scale : d < 0.f ? -(m * scale) : 0.f;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
    __shared__ float part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(loss, (part[0] + part[1] + part[2] + part[3]) * scale);
}

} // namespace lfs

extern "C" int lfs_activations_fwd(uint32_t N, const float* raw_quats, const float* raw_scales, const float* raw_opacities,
                                   float* quats, float* scales, float* opacities, lfs_stream_t stream) {
    if (N == 0) return LFS_OK;
    if (!raw_quats || !raw_scales || !raw_opacities || !quats || !scales || !opacities) return LFS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    lfs::ProfScope prof("activations_fwd", s);
    hipLaunchKernelGGL(lfs::activations_fwd_kernel, dim3((N + 255) / 256), dim3(256), 0, s, N, raw_quats, raw_scales, raw_opacities, quats, scales, opacities);
    return (int)hipGetLastError();
}

extern "C" int lfs_activations_bwd(uint32_t N, const float* raw_quats, const float* scales, const float* opacities,
                                   const float* v_quats, const float* v_scales, const float* v_opacities, float scale_reg, float opacity_reg, int accumulate,
                                   float* g_raw_quats, float* g_raw_scales, float* g_raw_opacities, lfs_stream_t stream) {
    if (N == 0) return LFS_OK;
    if (!raw_quats || !scales || !opacities || !v_quats || !v_scales || !v_opacities || !g_raw_quats || !g_raw_scales || !g_raw_opacities) return LFS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    lfs::ProfScope prof("activations_bwd", s);
    const dim3 grid((N + 255) / 256), block(256);
    // regularisers of trainer.cpp:132-158: scale_reg * mean(scales) (mean over 3N values) and opacity_reg * mean(opacities)
    const float vs = scale_reg / (3.f * float(N)), vo = opacity_reg / float(N);
    if (accumulate) hipLaunchKernelGGL(lfs::activations_bwd_kernel<true>, grid, block, 0, s, N, raw_quats, scales, opacities, v_quats, v_scales, v_opacities, vs, vo, g_raw_quats, g_raw_scales, g_raw_opacities);
    else hipLaunchKernelGGL(lfs::activations_bwd_kernel<false>, grid, block, 0, s, N, raw_quats, scales, opacities, v_quats, v_scales, v_opacities, vs, vo, g_raw_quats, g_raw_scales, g_raw_opacities);
    return (int)hipGetLastError();
}

extern "C" int lfs_mse_loss_fwd_bwd(uint32_t H, uint32_t W, const float* render_hwc, const float* target_chw, float weight,
                                    float* v_render_hwc, float* loss, lfs_stream_t stream) {
    if (H == 0 || W == 0) return LFS_OK;
    if (!render_hwc || !target_chw || !v_render_hwc || !loss) return LFS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    lfs::ProfScope prof("mse_loss", s);
    const uint32_t P = H * W;
    const uint32_t blocks = (P + 255) / 256 < 2048 ? (P + 255) / 256 : 2048;
    hipLaunchKernelGGL(lfs::mse_loss_kernel<false>, dim3(blocks), dim3(256), 0, s, H, W, render_hwc, target_chw, weight / float(3u * P), v_render_hwc, loss);
    return (int)hipGetLastError();
}

extern "C" int lfs_mse_loss_chw_fwd_bwd(uint32_t H, uint32_t W, const float* render_chw, const float* target_chw, float weight,
                                        float* v_render_chw, float* loss, lfs_stream_t stream) {
    if (H == 0 || W == 0) return LFS_OK;
    if (!render_chw || !target_chw || !v_render_chw || !loss) return LFS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    lfs::ProfScope prof("mse_loss", s);
    const uint32_t P = H * W;
    const uint32_t blocks = (P + 255) / 256 < 2048 ? (P + 255) / 256 : 2048;
    hipLaunchKernelGGL(lfs::mse_loss_kernel<true>, dim3(blocks), dim3(256), 0, s, H, W, render_chw, target_chw, weight / float(3u * P), v_render_chw, loss);
    return (int)hipGetLastError();
}

// general form (see lfs_photometric_loss_ex_fwd_bwd)
extern "C" int lfs_mse_loss_ex_fwd_bwd(uint32_t H, uint32_t W, const float* render, uint32_t render_is_chw, uint32_t clamp_render, const float* target_chw, float weight,
                                       float* v_render, float* loss, lfs_stream_t stream) {
    if (H == 0 || W == 0) return LFS_OK;
    if (!render || !target_chw || !v_render || !loss) return LFS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    lfs::ProfScope prof("mse_loss", s);
    const uint32_t P = H * W;
    const uint32_t blocks = (P + 255) / 256 < 2048 ? (P + 255) / 256 : 2048;
    if (render_is_chw) hipLaunchKernelGGL(lfs::mse_loss_kernel<true>, dim3(blocks), dim3(256), 0, s, H, W, render, target_chw, weight / float(3u * P), v_render, loss, clamp_render != 0);
    else hipLaunchKernelGGL(lfs::mse_loss_kernel<false>, dim3(blocks), dim3(256), 0, s, H, W, render, target_chw, weight / float(3u * P), v_render, loss, clamp_render != 0);
    return (int)hipGetLastError();
}

// masked form: *loss += weight * sum_c sum_p M_p (r - t)^2 / (3 sum_p M_p); the normaliser comes from mask_sums[0] on the device
extern "C" int lfs_mse_loss_masked_fwd_bwd(uint32_t H, uint32_t W, const float* render, uint32_t render_is_chw, uint32_t clamp_render, const float* target_chw,
                                           const uint8_t* mask_u8, const int64_t* mask_sums, float weight, float* v_render, float* loss, lfs_stream_t stream) {
    if (H == 0 || W == 0) return LFS_OK;
    if (!render || !target_chw || !v_render || !loss || !mask_u8 || !mask_sums) return LFS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    lfs::ProfScope prof("mse_loss_masked", s);
    const uint32_t P = H * W;
    const uint32_t blocks = (P + 255) / 256 < 2048 ? (P + 255) / 256 : 2048;
    const double wscale = double(weight) / 3.0;
    if (render_is_chw) hipLaunchKernelGGL(lfs::mse_loss_masked_kernel<true>, dim3(blocks), dim3(256), 0, s, H, W, render, target_chw, mask_u8, (const long long*)mask_sums, wscale, v_render, loss, clamp_render != 0);
    else hipLaunchKernelGGL(lfs::mse_loss_masked_kernel<false>, dim3(blocks), dim3(256), 0, s, H, W, render, target_chw, mask_u8, (const long long*)mask_sums, wscale, v_render, loss, clamp_render != 0);
    return (int)hipGetLastError();
}

extern "C" int lfs_depth_prepare(uint32_t H, uint32_t W, const float* target_in, const uint8_t* weights_u8, float* target_out, int64_t* sums, lfs_stream_t stream) {
    if (!sums || uint64_t(H) * W >= (1ull << 31) || (H != 0 && W != 0 && (!target_in || !target_out))) return LFS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(sums, 0, sizeof(int64_t), s); // the sum is written, not accumulated
    if (e != hipSuccess) return (int)e;
    if (H == 0 || W == 0) return LFS_OK;
    lfs::ProfScope prof("depth_prepare", s);
    const uint32_t P = H * W;
    hipLaunchKernelGGL(lfs::depth_prepare_kernel, dim3((P + 255) / 256), dim3(256), 0, s, P, target_in, weights_u8, target_out, (unsigned long long*)sums);
    return (int)hipGetLastError();
}

extern "C" int lfs_depth_l1_loss_fwd_bwd(uint32_t H, uint32_t W, const float* depth, const float* target, const uint8_t* weights_u8, const int64_t* sums, float weight,
                                         float* grad_depth, float* loss_acc, lfs_stream_t stream) {
    if (H == 0 || W == 0) return LFS_OK;
    if (!depth || !target || !sums || !grad_depth || !loss_acc || uint64_t(H) * W >= (1ull << 31)) return LFS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    lfs::ProfScope prof("depth_l1_loss", s);
    const uint32_t P = H * W;
    const uint32_t blocks = (P + 255) / 256 < 2048 ? (P + 255) / 256 : 2048;
    hipLaunchKernelGGL(lfs::depth_l1_loss_kernel, dim3(blocks), dim3(256), 0, s, P, depth, target, weights_u8, (const long long*)sums, double(weight), grad_depth, loss_acc);
    return (int)hipGetLastError();
}
