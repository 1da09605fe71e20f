// The SGLD noise of the MCMC strategy (gsplat::add_noise, RelocationCUDA.cu:88-144; "3D Gaussian Splatting as Markov Chain Monte Carlo", Eq. 9) for ONE Gaussian:
//   mean += current_lr * sigmoid(-100 (opacity - 0.005)) * (R diag(exp(2 raw_scale)) R^T) noise
// Shared by add_noise_kernel (mcmc.hip) and by phase 3 of the training step's fused tail (raster.hip: gut_tail_kernel<.., NOISE>), which has the raw scales, the raw
// quaternion and the raw opacity in registers already. mcmc.hip is compiled without floating-point contraction and raster.hip with it, so the arithmetic is pinned
// contraction-free HERE, statement by statement (the rotation matrix and the matrix-vector product are written out instead of calling lfs_math.cuh's helpers, whose
// bodies would take the including file's setting): both call sites produce the same bits, and lfs_add_noise keeps the ones it had.
#pragma once
#include "lfs_math.cuh"

namespace lfs {

LFS_DI void mcmc_add_noise(float (&mean)[3], const float (&raw_scale)[3], const float4 raw_quat /* (w, x, y, z) as stored */, const float raw_opacity,
                           const float (&noise)[3], const float current_lr) {
#pragma clang fp contract(off)
    const float s2[3] = {__expf(2.f * raw_scale[0]), __expf(2.f * raw_scale[1]), __expf(2.f * raw_scale[2])};
    // quat_to_rotmat(w, x, y, z, cap = 1e12f)
    float w = raw_quat.x, x = raw_quat.y, y = raw_quat.z, z = raw_quat.w;
    float inv = 1.f / sqrtf(x * x + y * y + z * z + w * w);
    if (!(inv < 1e12f)) inv = 1e12f;
    x *= inv; y *= inv; z *= inv; w *= inv;
    const float x2 = x * x, y2 = y * y, z2 = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    float R[3][3];
    R[0][0] = 1.f - 2.f * (y2 + z2); R[1][0] = 2.f * (xy + wz); R[2][0] = 2.f * (xz - wy);
    R[0][1] = 2.f * (xy - wz); R[1][1] = 1.f - 2.f * (x2 + z2); R[2][1] = 2.f * (yz + wx);
    R[0][2] = 2.f * (xz + wy); R[1][2] = 2.f * (yz - wx); R[2][2] = 1.f - 2.f * (x2 + y2);
    // covariance = R diag(s2) R^T ; transformed noise = covariance * noise
    float cov[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            cov[r][c] = R[r][0] * s2[0] * R[c][0] + R[r][1] * s2[1] * R[c][1] + R[r][2] * s2[2] * R[c][2];
    const float tn[3] = {cov[0][0] * noise[0] + cov[0][1] * noise[1] + cov[0][2] * noise[2],
                         cov[1][0] * noise[0] + cov[1][1] * noise[1] + cov[1][2] * noise[2],
                         cov[2][0] * noise[0] + cov[2][1] * noise[1] + cov[2][2] * noise[2]};
    const float opacity = 1.f / (1.f + __expf(-raw_opacity));
    const float op_sigmoid = 1.f / (1.f + __expf(100.f * opacity - 0.5f));
    const float nf = current_lr * op_sigmoid;
    mean[0] += nf * tn[0]; mean[1] += nf * tn[1]; mean[2] += nf * tn[2];
}

} // namespace lfs
