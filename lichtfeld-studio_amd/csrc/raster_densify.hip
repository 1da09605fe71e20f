// The densifying form of the gradient-tensor finish pass: raster_finish_adam_kernel<false> (raster.hip) over the shared body (lfs_raster_finish_body.cuh),
// plus ADC's densification statistic of the view - in a translation unit of its own, so that raster.hip's code object keeps every byte. Compiled with raster.hip's
// flags (build.py): the shared body's arithmetic is pinned contraction-free, the gradients are the default form's bit for bit (tests/test_gpu_gut_densify.py).
// Host builds on the wavefront emulator (LFS_EMULATE) have no code objects to keep apart: there raster.hip includes this file, so that every emulated build that holds
// raster.hip holds this form too, and the file compiled on its own is empty.
#if !defined(LFS_EMULATE) || defined(LFS_RASTER_DENSIFY_INLINE)
#include "lfs_prof.h"
#include "lfs_raster_finish.cuh"

namespace lfs {

// raster_finish_adam_kernel<false> + ADC's densification statistic of the view (lfs_raster_finish_body.cuh, DENSIFY): radii [N,2] of the view, dens [2,N] read-modify-written.
// (means / raw_quats are only read: the body's stores to them are in its Adam half.)
__global__ void __launch_bounds__(FINISH_BLOCK) raster_finish_densify_kernel(
    const uint32_t N, float* __restrict__ means, float* __restrict__ raw_quats,
    const float* __restrict__ quats, const float* __restrict__ scales, const float* __restrict__ opacities,
    const CamDev* __restrict__ cams, const float* __restrict__ acc, const float* __restrict__ v_dirs, const FinishAdam ad, const FinishGrads gr,
    const float* __restrict__ loss_slots, float* __restrict__ loss, const int32_t* __restrict__ radii, float* __restrict__ dens) {
    constexpr bool ADAM = false, DENSIFY = true;
    constexpr float* raw_scales = nullptr; constexpr float* raw_opacities = nullptr; constexpr const int32_t* abort_flag = nullptr;
#include "lfs_raster_finish_body.cuh"
}

int finish_densify_launch(uint32_t N, const float* means, const float* raw_quats, const float* quats, const float* scales, const float* opacities, const CamDev* cams,
                          const float* acc, const float* v_dirs, const FinishAdam& ad, const FinishGrads& gr, const float* loss_slots, float* loss, const int32_t* radii,
                          float* dens, hipStream_t s) {
    lfs::ProfScope prof("finish_densify", s);
    hipLaunchKernelGGL(raster_finish_densify_kernel, dim3((N + FINISH_BLOCK - 1) / FINISH_BLOCK), dim3(FINISH_BLOCK), 0, s, N, const_cast<float*>(means), const_cast<float*>(raw_quats), quats, scales, opacities, cams, acc,
                       v_dirs, ad, gr, loss_slots, loss, radii, dens);
    return (int)hipGetLastError();
}

} // namespace lfs
#endif
