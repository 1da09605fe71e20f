// The 3D smoothing filter of Mip-Splatting (Yu et al., CVPR 2024, section 4.1) for the fastgs (EWA) rasterizer: the per-Gaussian filter variance
//   v_i = variance_scale / nu_i^2,   nu_i = max over the training cameras that see i of max(fx, fy) / z_ic
// - the highest rate (pixels per world unit) at which any training camera samples Gaussian i. The per-primitive kernels of fastgs_prep.hip apply it
// (s'^2 = s^2 + v, opacity * prod s / s'); this file only computes v, once per change of the model, from ALL cameras.
// A camera sees i iff z > 0.2 and the pinhole projection lies within the image grown by 15 % on every side (the margin the EWA Jacobian is clamped with).
// A Gaussian no camera sees takes the smallest nu among the seen ones; none seen at all (or C == 0): v = 0 everywhere.
//
// Pass 1, one thread per Gaussian with its mean in registers: the camera index is the loop counter, the same for every lane, so the 18-dword camera record arrives
// through the scalar unit and enters the VALU as SGPR operands (the idiom of knn_mean_distance_kernel, dataprep.hip). nu (0 = unseen) goes to filter_var[i]; the
// minimum over the seen ones is an unsigned atomicMin on the float's bits (positive floats order like their bits): no float atomics, the result does not depend
// on the order of arrival. Pass 2 turns nu into v and patches the unseen rows. Streaming kernels: -ffp-contract=off like the rest of the per-primitive code.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/lfs_gsplat.h"

namespace lfs {
namespace f3d {

constexpr float NEAR_Z = 0.2f;
constexpr float MARGIN = 0.15f;
constexpr uint32_t THREADS = 256;
constexpr uint32_t NONE_SEEN = 0xFFFFFFFFu;   // the workspace word before any seen Gaussian arrived (above the bits of every finite float)

__global__ void __launch_bounds__(THREADS) filter3d_nu_kernel(const uint32_t N, const float* __restrict__ means, const uint32_t C,
                                                              const lfs_filter3d_camera* __restrict__ cams, float* __restrict__ nu_o, uint32_t* __restrict__ nu_min_bits) {
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    const bool live = i < N;
    const uint32_t ic = live ? i : N - 1;   // (no lane leaves before the loop: the camera loads stay uniform)
    const float mx = means[3 * size_t(ic)], my = means[3 * size_t(ic) + 1], mz = means[3 * size_t(ic) + 2];
    float nu = 0.f;
    for (uint32_t c = 0; c < C; ++c) {
        const lfs_filter3d_camera cam = cams[c];
        const float z = ((cam.w2c[8] * mx + cam.w2c[9] * my) + cam.w2c[10] * mz) + cam.w2c[11];
        const float xc = ((cam.w2c[0] * mx + cam.w2c[1] * my) + cam.w2c[2] * mz) + cam.w2c[3];
        const float yc = ((cam.w2c[4] * mx + cam.w2c[5] * my) + cam.w2c[6] * mz) + cam.w2c[7];
        const float w = float(cam.width), h = float(cam.height);
        const float x = cam.fx * xc / z + cam.cx, y = cam.fy * yc / z + cam.cy;
        const bool seen = z > NEAR_Z && x >= -MARGIN * w && x <= (1.f + MARGIN) * w && y >= -MARGIN * h && y <= (1.f + MARGIN) * h;
        const float rate = fmaxf(cam.fx, cam.fy) / z;
        nu = seen ? fmaxf(nu, rate) : nu;
    }
    if (live) nu_o[i] = nu;
    uint32_t bits = (live && nu > 0.f) ? __float_as_uint(nu) : NONE_SEEN;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) bits = min(bits, __shfl_xor(bits, m, 64));
    if ((threadIdx.x & 63u) == 0u && bits != NONE_SEEN) atomicMin(nu_min_bits, bits);
}

__global__ void __launch_bounds__(THREADS) filter3d_finish_kernel(const uint32_t N, const float variance_scale, const uint32_t* __restrict__ nu_min_bits,
                                                                  float* __restrict__ filter_var) {
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= N) return;
    const uint32_t min_bits = *nu_min_bits;
    float v = 0.f;
    if (min_bits != NONE_SEEN) {
        const float own = filter_var[i];
        const float nu = own > 0.f ? own : __uint_as_float(min_bits);
        v = variance_scale / (nu * nu);
    }
    filter_var[i] = v;
}

} // namespace f3d
} // namespace lfs

using namespace lfs;

static_assert(sizeof(lfs_filter3d_camera) == 72, "the ctypes mirror (capi.py) and the packed tensor of filter3d.py are laid out by hand");

extern "C" size_t lfs_filter3d_workspace_bytes(void) { return 256; }   // one word is used

extern "C" int lfs_filter3d_compute(uint32_t N, const float* means, uint32_t C, const lfs_filter3d_camera* cameras, float variance_scale, float* filter_var,
                                    void* workspace, size_t workspace_bytes, lfs_stream_t stream) {
    if (N == 0) return LFS_OK;
    if (!means || !filter_var || (C > 0 && !cameras) || !(variance_scale >= 0.f)) return LFS_E_INVALID;
    if (!workspace || workspace_bytes < 4) return LFS_E_WORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) % 4 != 0) return LFS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    uint32_t* const nu_min_bits = static_cast<uint32_t*>(workspace);
    const hipError_t e = hipMemsetAsync(nu_min_bits, 0xFF, 4, s);   // the 32-bit word = NONE_SEEN
    if (e != hipSuccess) return (int)e;
    const uint32_t blocks = (N + f3d::THREADS - 1) / f3d::THREADS;
    hipLaunchKernelGGL(f3d::filter3d_nu_kernel, dim3(blocks), dim3(f3d::THREADS), 0, s, N, means, C, cameras, filter_var, nu_min_bits);
    hipLaunchKernelGGL(f3d::filter3d_finish_kernel, dim3(blocks), dim3(f3d::THREADS), 0, s, N, variance_scale, nu_min_bits, filter_var);
    return (int)hipGetLastError();
}
