// The finish pass over the rasterizer's accumulator rows (one camera, global shutter): the geometry vjp every finish form shares, and the body of the one-round-trip
// pass behind raster_finish_adam_kernel<true / false> (raster.hip) and raster_finish_densify_kernel (raster_densify.hip). The densifying form lives in a translation
// unit - and so in a code object - of its own: raster.hip's code object keeps every byte (kernel descriptors hold the distance to their code, so ONE more kernel in a
// code object changes the descriptors of all the others; tools/code_object_identity.py).
#pragma once
#include "lfs_camera.cuh"
#include "lfs_raster_common.cuh"
#include "lfs_adam.cuh"

namespace lfs {

constexpr uint32_t LOSS_SLOTS = 256; // fused MSE: the wavefronts' partial sums are spread over this many addresses (one hot address costs ~0.08 ms)

// dL/d(mean, quaternion, scale) of ONE Gaussian under ONE camera from its accumulator sums A = dL/d(record matrix), G = dL/dg - the vjp tail of Bwd.cu:318-333 through
// M = S^-1 R^T (global shutter: record matrix M Rinv, g = M (o - mu)). Shared by raster_finish_kernel, raster_finish_adam_kernel and gut_tail_kernel, which are held to
// each other bit for bit (tests/test_gpu_gut_step.py): the arithmetic is pinned contraction-free here, helpers included (lfs_math.cuh's take the including file's default and
// this file allows contraction - round 6: a third inlined copy of the fused form came out one ulp off in dL/dmeans, the compiler fuses a*b + c*d differently per context).
// ADDS to vm / vq / vs (the operator form sums over cameras).
template <bool UNIFORM_ORIGIN>
LFS_DI void finish_geometry(const float4 q, const float (&is)[3], const float (&A_in)[9], const f3 G_in, const f3 mu, const CamDev& cam, float (&vm)[3], float (&vq)[4], float (&vs)[3]) {
#pragma clang fp contract(off)
    m3 R;
    float qw = q.x, qx = q.y, qy = q.z, qz = q.w;
    const float qinv = 1.f / sqrtf(qx * qx + qy * qy + qz * qz + qw * qw);
    qx *= qinv; qy *= qinv; qz *= qinv; qw *= qinv;
    {   // quat_to_rotmat
        const float x2 = qx * qx, y2 = qy * qy, z2 = qz * qz, xy = qx * qy, xz = qx * qz, yz = qy * qz, wx = qw * qx, wy = qw * qy, wz = qw * qz;
        R.m[0][0] = 1.f - 2.f * (y2 + z2); R.m[1][0] = 2.f * (xy + wz); R.m[2][0] = 2.f * (xz - wy);
        R.m[0][1] = 2.f * (xy - wz); R.m[1][1] = 1.f - 2.f * (x2 + z2); R.m[2][1] = 2.f * (yz + wx);
        R.m[0][2] = 2.f * (xz + wy); R.m[1][2] = 2.f * (yz - wx); R.m[2][2] = 1.f - 2.f * (x2 + y2);
    }
    m3 M;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) M.m[r][c] = is[r] * R.m[c][r];
#if LFS_ACC_SYM
    if (UNIFORM_ORIGIN) { // the symmetric row (lfs_raster_common.cuh, LFS_ACC_SYM): A_in = B'' (xx, yy, xz, yz, xy, zz) | sum a'', every slot times REC_UNSCALE by the caller; G_in: empty slots
        const float omx = cam.origin.x - mu.x, omy = cam.origin.y - mu.y, omz = cam.origin.z - mu.z;
        const f3 gv{M.m[0][0] * omx + M.m[0][1] * omy + M.m[0][2] * omz, M.m[1][0] * omx + M.m[1][1] * omy + M.m[1][2] * omz, M.m[2][0] * omx + M.m[2][1] * omy + M.m[2][2] * omz};
        m3 U;
        rot_frame_f32(gv, U);
        float Bp[3][3];   // B'' = sum a'' (x) w'', two factors of c in it: the second REC_UNSCALE here
        Bp[0][0] = A_in[0] * REC_UNSCALE; Bp[1][1] = A_in[1] * REC_UNSCALE; Bp[2][2] = A_in[5] * REC_UNSCALE;
        Bp[0][2] = Bp[2][0] = A_in[2] * REC_UNSCALE; Bp[1][2] = Bp[2][1] = A_in[3] * REC_UNSCALE; Bp[0][1] = Bp[1][0] = A_in[4] * REC_UNSCALE;
        float T[3][3], B[3][3];   // B = U^T B'' U: the sums in the Gaussian's own frame
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) T[k][c] = Bp[k][0] * U.m[0][c] + Bp[k][1] * U.m[1][c] + Bp[k][2] * U.m[2][c];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) B[r][c] = U.m[0][r] * T[0][c] + U.m[1][r] * T[1][c] + U.m[2][r] * T[2][c];
        const float as[3] = {U.m[0][0] * A_in[6] + U.m[1][0] * A_in[7] + U.m[2][0] * A_in[8], U.m[0][1] * A_in[6] + U.m[1][1] * A_in[7] + U.m[2][1] * A_in[8],
                             U.m[0][2] * A_in[6] + U.m[1][2] * A_in[7] + U.m[2][2] * A_in[8]};   // sum a = -dL/dg
        // mean: g = M (o - mu)  ->  dL/dmu = -M^T dL/dg = M^T sum a
        vm[0] += M.m[0][0] * as[0] + M.m[1][0] * as[1] + M.m[2][0] * as[2];
        vm[1] += M.m[0][1] * as[0] + M.m[1][1] * as[1] + M.m[2][1] * as[2];
        vm[2] += M.m[0][2] * as[0] + M.m[1][2] * as[1] + M.m[2][2] * as[2];
        // dL/dM = -B M^-T = -B S R^T. Scales: dL/ds_c = -(1 / s_c^2) (dL/dM R)_cc = B_cc / s_c - a sum of like-signed terms, where dL/dA . M + dL/dg . g cancelled to 1e-6.
        // Rotation: dL/dR[r][c] = dL/dM[c][r] / s_c = -(1 / s_c) sum_k B[c][k] s_k R[r][k]
        const float sk[3] = {1.f / is[0], 1.f / is[1], 1.f / is[2]};
        float g[3][3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) g[r][c] = -is[c] * (B[c][0] * sk[0] * R.m[r][0] + B[c][1] * sk[1] * R.m[r][1] + B[c][2] * sk[2] * R.m[r][2]);
        {   // quat_to_rotmat_vjp on the normalised quaternion
            const float vw = 2.f * (qx * (g[2][1] - g[1][2]) + qy * (g[0][2] - g[2][0]) + qz * (g[1][0] - g[0][1]));
            const float vx = 2.f * (-2.f * qx * (g[1][1] + g[2][2]) + qy * (g[1][0] + g[0][1]) + qz * (g[2][0] + g[0][2]) + qw * (g[2][1] - g[1][2]));
            const float vy = 2.f * (qx * (g[1][0] + g[0][1]) - 2.f * qy * (g[0][0] + g[2][2]) + qz * (g[2][1] + g[1][2]) + qw * (g[0][2] - g[2][0]));
            const float vz = 2.f * (qx * (g[2][0] + g[0][2]) + qy * (g[2][1] + g[1][2]) - 2.f * qz * (g[0][0] + g[1][1]) + qw * (g[1][0] - g[0][1]));
            const float dq = vw * qw + vx * qx + vy * qy + vz * qz;
            vq[0] += (vw - dq * qw) * qinv; vq[1] += (vx - dq * qx) * qinv; vq[2] += (vy - dq * qy) * qinv; vq[3] += (vz - dq * qz) * qinv;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) vs[c] += B[c][c] * is[c];
        return;
    }
    const float (&A)[9] = A_in; const f3 G = G_in;
#elif LFS_REC_ROT
    float Au[9]; f3 Gu = G_in;
#pragma unroll
    for (int k = 0; k < 9; ++k) Au[k] = A_in[k];
    if (UNIFORM_ORIGIN) { // the sums were accumulated in the record's rotated frame (lfs_raster_common.cuh, LFS_REC_ROT): dL/dA = U^T dL/dA'', dL/dg = U^T dL/dg''
        const float omx = cam.origin.x - mu.x, omy = cam.origin.y - mu.y, omz = cam.origin.z - mu.z;
        const f3 g{M.m[0][0] * omx + M.m[0][1] * omy + M.m[0][2] * omz, M.m[1][0] * omx + M.m[1][1] * omy + M.m[1][2] * omz, M.m[2][0] * omx + M.m[2][1] * omy + M.m[2][2] * omz};
        RotFrame F;
        rot_frame(g, F);   // (the record's frame, bit for bit: lfs_raster_common.cuh)
#pragma unroll
        for (int c = 0; c < 3; ++c) rot_apply_t(F, A_in[c], A_in[3 + c], A_in[6 + c], Au[c], Au[3 + c], Au[6 + c]);
        rot_apply_t(F, G_in.y, G_in.z, G_in.x, Gu.x, Gu.y, Gu.z);   // slots 9 .. 11 arrive as (z, x, y) (raster_bwd_kernel)
    }
    const float (&A)[9] = Au; const f3 G = Gu;
#else
    const float (&A)[9] = A_in; const f3 G = G_in;
#endif
    // dL/dM (math rows r, cols c). Global shutter: the record matrix was M Rinv, so dL/dM = dL/d(M Rinv) Rinv^T
    m3 vM;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (UNIFORM_ORIGIN) {
                const m3& Ri = cam.Rinv;
                vM.m[r][c] = A[3 * r] * Ri.m[c][0] + A[3 * r + 1] * Ri.m[c][1] + A[3 * r + 2] * Ri.m[c][2];
            } else vM.m[r][c] = A[3 * r + c];
        }
    if (UNIFORM_ORIGIN) {
        const float gv[3] = {G.x, G.y, G.z}, ov[3] = {cam.origin.x - mu.x, cam.origin.y - mu.y, cam.origin.z - mu.z};
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) vM.m[r][c] += gv[r] * ov[c];
    }
    // mean: gro = M (o - mu)  ->  dL/dmu = -M^T G
    vm[0] -= M.m[0][0] * G.x + M.m[1][0] * G.y + M.m[2][0] * G.z;
    vm[1] -= M.m[0][1] * G.x + M.m[1][1] * G.y + M.m[2][1] * G.z;
    vm[2] -= M.m[0][2] * G.x + M.m[1][2] * G.y + M.m[2][2] * G.z;
    // M = S^-1 R^T, i.e. P = M^T = R S^-1 with dL/dP = (dL/dM)^T:  dL/dR[r][c] = dL/dP[r][c] / s_c ;  dL/ds_c = -(1/s_c^2) sum_r R[r][c] dL/dP[r][c]
    float g[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) g[r][c] = vM.m[c][r] * is[c];
    {   // quat_to_rotmat_vjp on the normalised quaternion
        const float vw = 2.f * (qx * (g[2][1] - g[1][2]) + qy * (g[0][2] - g[2][0]) + qz * (g[1][0] - g[0][1]));
        const float vx = 2.f * (-2.f * qx * (g[1][1] + g[2][2]) + qy * (g[1][0] + g[0][1]) + qz * (g[2][0] + g[0][2]) + qw * (g[2][1] - g[1][2]));
        const float vy = 2.f * (qx * (g[1][0] + g[0][1]) - 2.f * qy * (g[0][0] + g[2][2]) + qz * (g[2][1] + g[1][2]) + qw * (g[0][2] - g[2][0]));
        const float vz = 2.f * (qx * (g[2][0] + g[0][2]) + qy * (g[2][1] + g[1][2]) - 2.f * qz * (g[0][0] + g[1][1]) + qw * (g[1][0] - g[0][1]));
        const float dq = vw * qw + vx * qx + vy * qy + vz * qz;
        vq[0] += (vw - dq * qw) * qinv; vq[1] += (vx - dq * qx) * qinv; vq[2] += (vy - dq * qy) * qinv; vq[3] += (vz - dq * qz) * qinv;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
        vs[c] += -is[c] * is[c] * (R.m[0][c] * vM.m[c][0] + R.m[1][c] * vM.m[c][1] + R.m[2][c] * vM.m[c][2]);
}

// The all-inline training step (ONE camera, global shutter, one view per step on one rank): raster_finish_kernel + the activation backward
// (l2_fused.hip: normalize / exp / sigmoid vjp + the MCMC regularisers) + the Adam updates of means, raw scales, raw quaternions and raw
// opacities (adam.hip) in ONE pass over the Gaussians - no gradient tensor is written or re-read. acc row: dL/dA (9) | -dL/dg (3) | dL/dopacity |
// dL/dcolour (3: consumed by lfs_sh_model_bwd_adam_all, which hands back dL/d(dirs) in v_dirs). Same operations in the same order as
// the three separate kernels (the activation and Adam arithmetic is un-fused there: pinned with fp contract(off) here).
struct FinishAdam { float* m[4]; float* v[4]; AdamScalars s[4]; float scale_reg, opacity_reg; }; // order: means, raw_scales, raw_quats, raw_opacities
// ADAM = false (multi-GPU / multi-view / non-MSE steps, which need gradient TENSORS): the same pass up to the raw-parameter gradients, written (or added,
// `accumulate`) to g_* instead of being consumed - raster_finish_kernel + activations_bwd_kernel + the copy of dL/dmeans in one launch; dL/dcolour goes
// to v_colors for the SH backward, which adds dL/d(dirs) onto g_means afterwards. *loss += the fused MSE (as raster_finish_kernel).
struct FinishGrads { float* g_means; float* g_scales; float* g_quats; float* g_opac; float* v_colors; int accumulate; };
constexpr int FINISH_BLOCK = 256;   // threads per workgroup of raster_finish_adam_kernel
// the fused-loss fold reads LOSS_SLOTS = 256 partial sums with the first four wavefronts of workgroup 0 and adds wave_sum[0..3]: smaller workgroups would drop slots
static_assert(FINISH_BLOCK >= 256 && FINISH_BLOCK % 64 == 0 && FINISH_BLOCK <= 1024, "FINISH_BLOCK: 256, 320, ..., 1024");
// DENSIFY (gradient-tensor form only; raster_finish_densify_kernel): ADC's statistic of THIS view from what the pass holds in registers anyway -
//   v = the rasterizer's part of dL/dmean of this view (vm below: before + dL/d(dirs), before the bucket is added, selected to 0 by `any`)
//   g_c = Rinv^T v, z = (Rinv^T (mu - origin)).z, s = sqrt((g_c.x z W / (2 fx))^2 + (g_c.y z H / (2 fy))^2)   - a lateral shift dX at depth z moves the pixel by fx dX / z,
//   so dL/dX * z * W / (2 fx) is what dL/dmean2d.x * 0.5 * W is on the EWA route (kernels_backward.cuh:233-236): grad_threshold keeps its meaning
//   visible = radii.x > 0 && radii.y > 0;  dens[0][i] += visible, dens[1][i] += visible ? s : 0   (default_strategy.cpp reads row 1 / row 0)
// One lane owns one Gaussian: the read-modify-write of the two rows is plain loads and stores, the loads (radii pair 8 B, two floats) issued with everything else.
// The pass itself is lfs_raster_finish_body.cuh.

// raster_densify.hip: raster_finish_adam_kernel<false> + ADC's statistic of the view (lfs_raster_finish_body.cuh, DENSIFY) - the launch over N > 0 Gaussians; the caller
// (gut_finish_grads_impl, raster.hip) has checked the operands. -> hipGetLastError()
int finish_densify_launch(uint32_t N, const float* means, const float* raw_quats, const float* quats, const float* scales, const float* opacities, const CamDev* cams,
                          const float* acc, const float* v_dirs, const FinishAdam& ad, const FinishGrads& gr, const float* loss_slots, float* loss, const int32_t* radii,
                          float* dens, hipStream_t s);

} // namespace lfs
