// gs::SplatData's activations for ONE Gaussian (the arithmetic of activations_fwd_kernel, l2_fused.hip): quaternion x / max(|x|, 1e-12), scale exp, opacity sigmoid.
// Shared by projection_ut_kernel<ACT> (projection_ut.hip), which projects the activated values, and by phase 3 of the training step's fused tail (raster.hip:
// gut_tail_kernel), which has the raw quaternion, scales and opacity in registers already and recomputes the activated ones there - the fused-tail step then neither
// stores them (32 B per Gaussian) nor reads them back. projection_ut.hip is compiled without floating-point contraction and raster.hip with it, so the arithmetic is
// pinned contraction-free HERE, as lfs_mcmc_noise.cuh does: both call sites produce the same bits, and the projection keeps the ones it had.
#pragma once
#include "lfs_math.cuh"

namespace lfs {

LFS_DI void splat_activations(const float4 raw_quat, const float (&raw_scale)[3], const float raw_opacity, float4& quat, float (&scale)[3], float& opacity) {
#pragma clang fp contract(off)
    const float den = fmaxf(sqrtf(raw_quat.x * raw_quat.x + raw_quat.y * raw_quat.y + raw_quat.z * raw_quat.z + raw_quat.w * raw_quat.w), 1e-12f);
    quat = make_float4(raw_quat.x / den, raw_quat.y / den, raw_quat.z / den, raw_quat.w / den);
    scale[0] = expf(raw_scale[0]); scale[1] = expf(raw_scale[1]); scale[2] = expf(raw_scale[2]);
    opacity = 1.f / (1.f + expf(-raw_opacity));
}

} // namespace lfs
