// The reference's default training rasterizer ("fastgs", EWA splatting) — per-primitive stages:
// fused activation + covariance + EWA projection + SH colour + exact tile counting (replaces preprocess_cu,
// fastgs/rasterization/include/kernels_forward.cuh:19-205), instance emission (create_instances_cu :224-330, here a
// scatter straight into per-tile buckets, as intersect.hip does) and the per-primitive backward (preprocess_backward_cu,
// kernels_backward.cuh:19-233, incl. convert_sh_to_color_backward kernel_utils.cuh:38-106 and densification_info).
// Streaming, HBM-bound kernels: compiled with -ffp-contract=off so that the tile-membership test rounds like the oracle.
#include <mutex>
#include "lfs_fastgs.cuh"
#include "lfs_prof.h"
#include "lfs_tilelists.cuh"
#include "../../include/lfs_gsplat.h"

namespace lfs {
namespace fgs {

// kernel_utils.cuh:108-148 — does the maximum of the Gaussian over the pixel-index rectangle [rx0, rx0+w-1] x [ry0, ry0+h-1]
// reach the power threshold? (mean already shifted by -0.5)
LFS_DI bool will_contribute(float mx, float my, float ca, float cb, float cc, float rx0, float ry0, float w, float h, float power_threshold) {
    const float rx1 = rx0 + w - 1.f, ry1 = ry0 + h - 1.f;
    const float x_min_diff = rx0 - mx, y_min_diff = ry0 - my;
    const float x_left = x_min_diff > 0.f ? 1.f : 0.f, y_above = y_min_diff > 0.f ? 1.f : 0.f;
    const float not_in_x = x_left + (mx > rx1 ? 1.f : 0.f), not_in_y = y_above + (my > ry1 ? 1.f : 0.f);
    if (not_in_x + not_in_y == 0.f) return true;
    const float ccx = x_left > 0.f ? rx0 : rx1, ccy = y_above > 0.f ? ry0 : ry1;
    const float dfx = mx - ccx, dfy = my - ccy;
    const float dx = copysignf(w - 1.f, x_min_diff), dy = copysignf(h - 1.f, y_min_diff);
    const float tx = not_in_y * __saturatef((dx * ca * dfx + dx * cb * dfy) / (dx * ca * dx));
    const float ty = not_in_x * __saturatef((dy * cb * dfx + dy * cc * dfy) / (dy * cc * dy));
    const float px = ccx + tx * dx, py = ccy + ty * dy;
    const float ddx = mx - px, ddy = my - py;
    return 0.5f * (ca * ddx * ddx + cc * ddy * ddy) + cb * ddx * ddy <= power_threshold;
}

struct Cov { // what forward and backward both need of a primitive's geometry
    float depth, x, y, var[3], R[3][3], RS[3][3], cov[3][3], qr, qx, qy, qz, qn;
    float qxx, qyy, qzz, qxy, qxz, qyz, qrx, qry, qrz;
    float tx, ty, j11, j13, j22, j23, jw1[3], jw2[3], jc1[3], jc2[3], a, b, c;
    float a0, c0; // (a, c) before the dilation: the antialiased mode's compensation needs both determinants
};
// FILTER3D: var3 = the activated variances s_k^2 + v the caller formed (the 3D smoothing filter); the raw scales are not read
template <bool FILTER3D = false>
LFS_DI void ewa(const Frame& f, const float* __restrict__ m, const float* __restrict__ rs, const float4 q, Cov& o, const float* var3 = nullptr) {
    const float* r1 = f.w2c; const float* r2 = f.w2c + 4; const float* r3 = f.w2c + 8;
    o.depth = r3[0] * m[0] + r3[1] * m[1] + r3[2] * m[2] + r3[3];
    o.x = (r1[0] * m[0] + r1[1] * m[1] + r1[2] * m[2] + r1[3]) / o.depth;
    o.y = (r2[0] * m[0] + r2[1] * m[1] + r2[2] * m[2] + r2[3]) / o.depth;
    if constexpr (FILTER3D) { o.var[0] = var3[0]; o.var[1] = var3[1]; o.var[2] = var3[2]; }
    else { o.var[0] = expf(2.f * rs[0]); o.var[1] = expf(2.f * rs[1]); o.var[2] = expf(2.f * rs[2]); }
    o.qr = q.x; o.qx = q.y; o.qy = q.z; o.qz = q.w;
    o.qn = o.qr * o.qr + o.qx * o.qx + o.qy * o.qy + o.qz * o.qz;
    o.qxx = 2.f * o.qx * o.qx / o.qn; o.qyy = 2.f * o.qy * o.qy / o.qn; o.qzz = 2.f * o.qz * o.qz / o.qn;
    o.qxy = 2.f * o.qx * o.qy / o.qn; o.qxz = 2.f * o.qx * o.qz / o.qn; o.qyz = 2.f * o.qy * o.qz / o.qn;
    o.qrx = 2.f * o.qr * o.qx / o.qn; o.qry = 2.f * o.qr * o.qy / o.qn; o.qrz = 2.f * o.qr * o.qz / o.qn;
    o.R[0][0] = 1.f - (o.qyy + o.qzz); o.R[0][1] = o.qxy - o.qrz; o.R[0][2] = o.qry + o.qxz;
    o.R[1][0] = o.qrz + o.qxy; o.R[1][1] = 1.f - (o.qxx + o.qzz); o.R[1][2] = o.qyz - o.qrx;
    o.R[2][0] = o.qxz - o.qry; o.R[2][1] = o.qrx + o.qyz; o.R[2][2] = 1.f - (o.qxx + o.qyy);
#pragma unroll
    for (int u = 0; u < 3; ++u)
#pragma unroll
        for (int v = 0; v < 3; ++v) o.RS[u][v] = o.R[u][v] * o.var[v];
#pragma unroll
    for (int u = 0; u < 3; ++u)
#pragma unroll
        for (int v = 0; v < 3; ++v) o.cov[u][v] = o.RS[u][0] * o.R[v][0] + o.RS[u][1] * o.R[v][1] + o.RS[u][2] * o.R[v][2];
    const float w = float(f.width), h = float(f.height);
    o.tx = fminf(fmaxf(o.x, (-0.15f * w - f.cx) / f.fx), (1.15f * w - f.cx) / f.fx);
    o.ty = fminf(fmaxf(o.y, (-0.15f * h - f.cy) / f.fy), (1.15f * h - f.cy) / f.fy);
    o.j11 = f.fx / o.depth; o.j13 = -o.j11 * o.tx; o.j22 = f.fy / o.depth; o.j23 = -o.j22 * o.ty;
#pragma unroll
    for (int v = 0; v < 3; ++v) { o.jw1[v] = o.j11 * r1[v] + o.j13 * r3[v]; o.jw2[v] = o.j22 * r2[v] + o.j23 * r3[v]; }
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        o.jc1[v] = o.jw1[0] * o.cov[0][v] + o.jw1[1] * o.cov[1][v] + o.jw1[2] * o.cov[2][v];
        o.jc2[v] = o.jw2[0] * o.cov[0][v] + o.jw2[1] * o.cov[1][v] + o.jw2[2] * o.cov[2][v];
    }
    o.a0 = o.jc1[0] * o.jw1[0] + o.jc1[1] * o.jw1[1] + o.jc1[2] * o.jw1[2];
    o.a = o.a0 + DILATION;
    o.b = o.jc1[0] * o.jw2[0] + o.jc1[1] * o.jw2[1] + o.jc1[2] * o.jw2[2];
    o.c0 = o.jc2[0] * o.jw2[0] + o.jc2[1] * o.jw2[1] + o.jc2[2] * o.jw2[2];
    o.c = o.c0 + DILATION;
}

// ---------------------------------------------------------------------------
// forward preprocess: one thread per primitive. Per-tile counts go through an LDS histogram (one coalesced global atomic
// per touched (workgroup, tile), see intersect.hip) when the tile grid fits.
// AA (LFS_FASTGS_ANTIALIASED): the opacity is multiplied by rho = sqrt(max(0, det(Sigma2d) / det(Sigma2d + DILATION I))) (add_blur, gsplat/Utils.cuh:171-179) before
// anything looks at it - the 1/255 cut, the power threshold, the extents, the tile tests and the records all see o_eff = sigmoid(raw) * rho. sigmoid(raw) is kept in
// the record's free r1.w for the backward. Thread 0 writes the mode word of the workspace: the backward reads it there.
// DEPTH (1: LFS_FASTGS_DEPTH, 2: LFS_FASTGS_INVDEPTH): d = z or 1 / z of the camera-space z the cuts and the sort key already use goes into the record's free r2.w
// (one dword store; the SH kernel that fills r2.xyz afterwards writes three dwords and leaves it alone). Nothing else changes: the default forms store nothing there.
// ---------------------------------------------------------------------------
// FILTER3D (lfs_fastgs_view_ext::filter3d_var, the 3D smoothing filter of Mip-Splatting): v = filter_var[i] is loaded after the depth cut; with s2_k = exp(2 raw_scale_k),
// u_k = v / (s2_k + v) (0 for v = 0) the variances are s2_k + v and the opacity is sigmoid(raw) * kappa, kappa = sqrt(prod (1 - u_k)) = prod s_k / s'_k, before the 1/255
// cut and everything after it (rho of the AA form is that of the filtered covariance). sigmoid(raw) goes to r1.w as in the AA form. The body is shared; the kernels
// below it are its FILTER3D = false / true wrappers under separate names, so the default forms keep theirs. (Both shared bodies take the Frame by value and their
// pointers __restrict__, exactly as the kernels do: with either changed, the default forms no longer compile to the registers they had as kernels of their own.)
template <bool LDS_HIST, bool AA, int DEPTH, bool FILTER3D>
LFS_DI void preprocess_body(
    const uint32_t N, const uint32_t per_block, const float* __restrict__ means, const float* __restrict__ scales_raw, const float* __restrict__ rot_raw,
    const float* __restrict__ opac_raw, const Frame f,
    GaussRec* __restrict__ rec, float2* __restrict__ mean2d_o, float4* __restrict__ conic_opacity_o, ushort4* __restrict__ bounds_o,
    uint32_t* __restrict__ n_touched_o, uint32_t* __restrict__ depth_bits_o, uint32_t* __restrict__ totals, uint32_t* __restrict__ mode_o,
    const float* __restrict__ filter_var) {
    extern __shared__ __attribute__((aligned(16))) uint32_t hist[];
    if (blockIdx.x == 0 && threadIdx.x == 0) *mode_o = (AA ? MODE_ANTIALIASED : 0u) | depth_mode_bits(DEPTH) | (FILTER3D ? MODE_FILTER3D : 0u);
    const uint32_t T = f.gw * f.gh;
    if (LDS_HIST) {
        for (uint32_t t = threadIdx.x; t < T; t += blockDim.x) hist[t] = 0u;
        __syncthreads();
    }
    const uint32_t begin = blockIdx.x * per_block, end = min(begin + per_block, N);
    for (uint32_t i = begin + threadIdx.x; i < end; i += blockDim.x) {
        uint32_t n_touched = 0;
        do {
            const float* m = means + 3 * size_t(i);
            const float* r3 = f.w2c + 8;
            const float depth = r3[0] * m[0] + r3[1] * m[1] + r3[2] * m[2] + r3[3];
            if (depth < f.near_ || depth > f.far_) break;
            const float sig = 1.0f / (1.0f + expf(-opac_raw[i]));
            float base = sig;   // the opacity before rho: sigmoid(raw), or sigmoid(raw) * kappa
            float var3[3];
            if constexpr (FILTER3D) {
                const float v = filter_var[i];
                float keep = 1.f;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float s2 = expf(2.f * scales_raw[3 * size_t(i) + k]);
                    var3[k] = s2 + v;
                    keep *= 1.f - (v > 0.f ? v / var3[k] : 0.f);
                }
                base = sig * sqrtf(keep);
            }
            if (base < MIN_ALPHA) break;
            const float4 q = reinterpret_cast<const float4*>(rot_raw)[i];
            if (q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w < 1e-8f) break;
            Cov cv;
            ewa<FILTER3D>(f, m, scales_raw + 3 * size_t(i), q, cv, var3);
            const float det = cv.a * cv.c - cv.b * cv.b;
            if (det < 1e-8f) break;
            float opacity = base;
            if constexpr (AA) {
                opacity = base * sqrtf(fmaxf(0.f, (cv.a0 * cv.c0 - cv.b * cv.b) / det));
                if (opacity < MIN_ALPHA) break;
            }
            const float ca = cv.c / det, cb = -cv.b / det, cc = cv.a / det;
            const float mx = cv.x * f.fx + f.cx, my = cv.y * f.fy + f.cy;
            const float power_threshold = logf(opacity * MIN_ALPHA_RCP);
            const float fac = sqrtf(2.0f * power_threshold);
            const float ex = fmaxf(fac * sqrtf(cv.a) - 0.5f, 0.f), ey = fmaxf(fac * sqrtf(cv.c) - 0.5f, 0.f);
            const uint32_t x0 = min(f.gw, uint32_t(max(0, __float2int_rd((mx - ex) / float(TILE)))));
            const uint32_t x1 = min(f.gw, uint32_t(max(0, __float2int_ru((mx + ex) / float(TILE)))));
            const uint32_t y0 = min(f.gh, uint32_t(max(0, __float2int_rd((my - ey) / float(TILE)))));
            const uint32_t y1 = min(f.gh, uint32_t(max(0, __float2int_ru((my + ey) / float(TILE)))));
            if ((x1 - x0) * (y1 - y0) == 0) break;
            for (uint32_t ty = y0; ty < y1; ++ty)
                for (uint32_t tx = x0; tx < x1; ++tx)
                    if (will_contribute(mx - 0.5f, my - 0.5f, ca, cb, cc, float(tx * TILE), float(ty * TILE), float(TILE), float(TILE), power_threshold)) {
                        ++n_touched;
                        if (LDS_HIST) atomicAdd(&hist[ty * f.gw + tx], 1u); else atomicAdd(&totals[ty * f.gw + tx], 1u);
                    }
            if (n_touched == 0) break;
            // (r2 = max(SH colour + 0.5, 0) is filled in by the SH kernel of sh.hip right after this one)
            float4* r = reinterpret_cast<float4*>(rec + i);
            r[0] = make_float4(mx, my, 0.5f * LOG2E * ca, LOG2E * cb);
            r[1] = make_float4(0.5f * LOG2E * cc, LOG2E * power_threshold, opacity, (AA || FILTER3D) ? sig : 0.f);
            if constexpr (DEPTH != 0) reinterpret_cast<float*>(rec + i)[11] = DEPTH == 1 ? depth : 1.0f / depth;   // r2.w (depth >= near_plane > 0 here)
            mean2d_o[i] = make_float2(mx, my);
            conic_opacity_o[i] = make_float4(ca, cb, cc, opacity);
            bounds_o[i] = make_ushort4(uint16_t(x0), uint16_t(x1), uint16_t(y0), uint16_t(y1));
            depth_bits_o[i] = __float_as_uint(depth);
        } while (false);
        n_touched_o[i] = n_touched;
    }
    if (LDS_HIST) {
        __syncthreads();
        for (uint32_t t = threadIdx.x; t < T; t += blockDim.x) {
            const uint32_t c = hist[t];
            if (c) atomicAdd(&totals[t], c);
        }
    }
}

#define LFS_FG_PREP_PARAMS \
    const uint32_t N, const uint32_t per_block, const float* __restrict__ means, const float* __restrict__ scales_raw, const float* __restrict__ rot_raw, \
    const float* __restrict__ opac_raw, const Frame f, \
    GaussRec* __restrict__ rec, float2* __restrict__ mean2d_o, float4* __restrict__ conic_opacity_o, ushort4* __restrict__ bounds_o, \
    uint32_t* __restrict__ n_touched_o, uint32_t* __restrict__ depth_bits_o, uint32_t* __restrict__ totals, uint32_t* __restrict__ mode_o
#define LFS_FG_PREP_ARGS N, per_block, means, scales_raw, rot_raw, opac_raw, f, rec, mean2d_o, conic_opacity_o, bounds_o, n_touched_o, depth_bits_o, totals, mode_o
template <bool LDS_HIST, bool AA, int DEPTH>
__global__ void __launch_bounds__(1024) fg_preprocess_kernel(LFS_FG_PREP_PARAMS) {
    preprocess_body<LDS_HIST, AA, DEPTH, false>(LFS_FG_PREP_ARGS, nullptr);
}
// (96 SGPRs: the filter operand's pointer would otherwise take the forms without the LDS histogram two registers past the allocation step their default forms stay
// under; the compiler finds them without spilling to memory - tests/test_kernel_resources_fastgs_filter3d.py)
#ifdef LFS_EMULATE
#define LFS_FG_F3D_SGPRS
#else
#define LFS_FG_F3D_SGPRS __attribute__((amdgpu_num_sgpr(96)))
#endif
template <bool LDS_HIST, bool AA, int DEPTH>
__global__ void __launch_bounds__(1024) LFS_FG_F3D_SGPRS fg_preprocess_f3d_kernel(LFS_FG_PREP_PARAMS, const float* __restrict__ filter_var) {
    preprocess_body<LDS_HIST, AA, DEPTH, true>(LFS_FG_PREP_ARGS, filter_var);
}
#undef LFS_FG_PREP_PARAMS
#undef LFS_FG_PREP_ARGS

// ---------------------------------------------------------------------------
// scatter: (depth bits << 32 | primitive) of every instance into its tile bucket (unordered inside the bucket; the
// per-tile sort orders by (depth, primitive))
// ---------------------------------------------------------------------------
template <bool LDS_HIST>
__global__ void __launch_bounds__(1024) fg_scatter_kernel(
    const uint32_t N, const uint32_t per_block, const Frame f, const float2* __restrict__ mean2d, const float4* __restrict__ conic_opacity,
    const ushort4* __restrict__ bounds, const uint32_t* __restrict__ n_touched, const uint32_t* __restrict__ depth_bits,
    const int32_t* __restrict__ offsets, uint32_t* __restrict__ cursor, int64_t* __restrict__ keys) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t T = f.gw * f.gh;
    uint32_t* cnt = lds; uint32_t* base_s = lds + T;
    const uint32_t begin = blockIdx.x * per_block, end = min(begin + per_block, N);
    auto visit = [&](uint32_t i, auto&& fn) {
        if (n_touched[i] == 0) return;
        const float2 m = mean2d[i]; const float4 co = conic_opacity[i]; const ushort4 b = bounds[i];
        const float thr = logf(co.w * MIN_ALPHA_RCP);
        for (uint32_t ty = b.z; ty < b.w; ++ty)
            for (uint32_t tx = b.x; tx < b.y; ++tx)
                if (will_contribute(m.x - 0.5f, m.y - 0.5f, co.x, co.y, co.z, float(tx * TILE), float(ty * TILE), float(TILE), float(TILE), thr)) fn(ty * f.gw + tx);
    };
    if (LDS_HIST) {
        for (uint32_t t = threadIdx.x; t < T; t += blockDim.x) cnt[t] = 0u;
        __syncthreads();
        for (uint32_t i = begin + threadIdx.x; i < end; i += blockDim.x) visit(i, [&](uint32_t t) { atomicAdd(&cnt[t], 1u); });
        __syncthreads();
        for (uint32_t t = threadIdx.x; t < T; t += blockDim.x) {
            const uint32_t c = cnt[t];
            base_s[t] = c ? atomicAdd(&cursor[t], c) : 0u;
            cnt[t] = 0u;
        }
        __syncthreads();
    }
    for (uint32_t i = begin + threadIdx.x; i < end; i += blockDim.x) {
        const uint64_t key = (uint64_t(depth_bits[i]) << 32) | uint64_t(i);
        visit(i, [&](uint32_t t) {
            const uint32_t slot = LDS_HIST ? base_s[t] + atomicAdd(&cnt[t], 1u) : atomicAdd(&cursor[t], 1u);
            keys[size_t(offsets[t]) + slot] = int64_t(key);
        });
    }
}

// ---------------------------------------------------------------------------
// backward preprocess: blend-backward accumulator -> gradients of the raw parameters (+ densification_info)
// ---------------------------------------------------------------------------
// an invisible primitive (n_touched == 0): the reference leaves these rows at the zeros they were allocated with
LFS_DI void preprocess_bwd_zero_rows(const uint32_t i, float* __restrict__ g_means, float* __restrict__ g_scales_raw, float* __restrict__ g_rot_raw,
                                     float* __restrict__ g_opac_raw) {
#pragma unroll
    for (int c = 0; c < 3; ++c) { g_means[3 * size_t(i) + c] = 0.f; g_scales_raw[3 * size_t(i) + c] = 0.f; }
    reinterpret_cast<float4*>(g_rot_raw)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    g_opac_raw[i] = 0.f;
}

// one visible primitive; dcam = dL/d(mean in camera space) (kernels_backward.cuh:165-168), which the camera gradient below is made of
// AA: the record's opacity is o_eff = sigmoid(raw) * rho, so the accumulator's S = sum alpha dL/dalpha is o_eff dL/do_eff: dL/draw = S (1 - sigmoid(raw)) with the
// sigmoid from r1.w, and dL/drho = S / rho reaches the 2-D covariance through rho^2 = det0 / det1: dL/d(a0, b, c0) += S/2 (c0/det0 - c/det1, 2b (1/det1 - 1/det0),
// a0/det0 - a/det1) - no division by rho (a visible primitive has rho >= 1/255, hence det0 > 0). Everything below dcv is the code both modes share.
// DEPTH (1 / 2, a backward with grad_depth): slot 9 of the row is dL/dd, d = z or 1 / z, and z is the third camera-space coordinate: dL/dz = acc[9] (1 | -1 / z^2) is
// added to dcam[2] before grad_means and the camera gradient are made of it. densification_info keeps its definition (dL/dmean2d only).
// FILTER3D: the geometry is that of the filtered variances s2_k + v, so everything below is the gradient at the effective parameters, g'_k w.r.t. log s'_k included;
// d log s'_k / d raw_k = 1 - u_k and d log kappa / d raw_k = u_k, u_k = v / (s2_k + v): grad_scales_raw_k = g'_k (1 - u_k) + S u_k with S = a2.x. u_k is formed from v and
// s2_k + v (0 for v = 0; 0 again for an overflowed s2_k), never as a quotient of two overflowed values. sigmoid(raw) comes from r1.w as in the AA form.
template <bool AA, int DEPTH, bool FILTER3D>
LFS_DI void preprocess_bwd_one(
    const uint32_t i, const uint32_t N, const float* __restrict__ means, const float* __restrict__ scales_raw, const float* __restrict__ rot_raw,
    const Frame& f, const GaussRec* __restrict__ rec, const float4* __restrict__ conic_opacity, const float* __restrict__ acc,
    float* __restrict__ g_means, float* __restrict__ g_scales_raw, float* __restrict__ g_rot_raw, float* __restrict__ g_opac_raw,
    float* __restrict__ densification_info, float (&dcam)[3], const float* __restrict__ filter_var = nullptr) {
    const float4* a4 = reinterpret_cast<const float4*>(acc + size_t(i) * ACC_STRIDE);
    const float4 a0 = a4[0], a1 = a4[1], a2 = a4[2];
    const GaussRec r = rec[i];
    // accumulator row (fastgs_blend.hip): {S1 = sum h dx, S2 = sum h dy, sum h dx dx, sum h dx dy | sum h dy dy, dc.r, dc.g, dc.b | sum alpha dL/dalpha}
    // with h = -alpha dL/dalpha: dL/dmean2d = conic (S1, S2), dL/dconic = 0.5 (sum h dx dx, sum h dx dy, sum h dy dy)
    const float4 co = conic_opacity[i];
    const float dm2[2] = {co.x * a0.x + co.y * a0.y, co.y * a0.x + co.z * a0.y};
    const float dcon[3] = {0.5f * a0.z, 0.5f * a0.w, 0.5f * a1.x};
    const float opacity = (AA || FILTER3D) ? r.r1.w : r.r1.z;   // sigmoid(raw)
    g_opac_raw[i] = a2.x * (1.0f - opacity);
    const float* m = means + 3 * size_t(i);
    const float dpos[3] = {0.f, 0.f, 0.f}; // (the colour -> position term is added by the SH backward kernel of sh.hip, which runs after this one)
    // ---- EWA backward
    const float4 q = reinterpret_cast<const float4*>(rot_raw)[i];
    Cov cv;
    float var3[3], u3[3];
    if constexpr (FILTER3D) {
        const float v = filter_var[i];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            var3[k] = expf(2.f * scales_raw[3 * size_t(i) + k]) + v;
            u3[k] = v > 0.f ? v / var3[k] : 0.f;
        }
    }
    ewa<FILTER3D>(f, m, scales_raw + 3 * size_t(i), q, cv, var3);
    const float* r1 = f.w2c; const float* r2 = f.w2c + 4; const float* r3 = f.w2c + 8;
    const float A = cv.a, B = cv.b, C = cv.c;
    const float det = A * C - B * B, dr = 1.0f / det, dr2 = dr * dr;
    float dcv[3] = {dr2 * (2.0f * B * C * dcon[1] - C * C * dcon[0] - B * B * dcon[2]),
                    dr2 * (B * C * dcon[0] - (A * C + B * B) * dcon[1] + A * B * dcon[2]),
                    dr2 * (2.0f * A * B * dcon[1] - B * B * dcon[0] - A * A * dcon[2])};
    if constexpr (AA) {   // (dcv[1] is half of dL/db: b enters G twice)
        const float hs = 0.5f * a2.x, dr0 = 1.0f / (cv.a0 * cv.c0 - B * B);
        dcv[0] += hs * (cv.c0 * dr0 - C * dr);
        dcv[1] += hs * B * (dr - dr0);
        dcv[2] += hs * (cv.a0 * dr0 - A * dr);
    }
    float G[3][3];
#pragma unroll
    for (int u = 0; u < 3; ++u)
#pragma unroll
        for (int v = 0; v < 3; ++v)
            G[u][v] = (cv.jw1[u] * cv.jw1[v]) * dcv[0] + (cv.jw1[u] * cv.jw2[v] + cv.jw1[v] * cv.jw2[u]) * dcv[1] + (cv.jw2[u] * cv.jw2[v]) * dcv[2];
    float djw1[3], djw2[3];
#pragma unroll
    for (int v = 0; v < 3; ++v) { djw1[v] = 2.0f * (cv.jc1[v] * dcv[0] + cv.jc2[v] * dcv[1]); djw2[v] = 2.0f * (cv.jc1[v] * dcv[1] + cv.jc2[v] * dcv[2]); }
    const float dj11 = r1[0] * djw1[0] + r1[1] * djw1[1] + r1[2] * djw1[2], dj22 = r2[0] * djw2[0] + r2[1] * djw2[1] + r2[2] * djw2[2];
    const float dj13 = r3[0] * djw1[0] + r3[1] * djw1[1] + r3[2] * djw1[2], dj23 = r3[0] * djw2[0] + r3[1] * djw2[1] + r3[2] * djw2[2];
    const float h1 = dj11 - 2.0f * cv.tx * dj13, h2 = dj22 - 2.0f * cv.ty * dj23;
    dcam[0] = cv.j11 * (dm2[0] - dj13 / cv.depth); dcam[1] = cv.j22 * (dm2[1] - dj23 / cv.depth);
    dcam[2] = -cv.j11 * (cv.x * dm2[0] + h1 / cv.depth) - cv.j22 * (cv.y * dm2[1] + h2 / cv.depth);
    if constexpr (DEPTH == 1) dcam[2] += a2.y;
    if constexpr (DEPTH == 2) dcam[2] -= a2.y / (cv.depth * cv.depth);
#pragma unroll
    for (int c = 0; c < 3; ++c) g_means[3 * size_t(i) + c] = r1[c] * dcam[0] + r2[c] * dcam[1] + r3[c] * dcam[2] + dpos[c];
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        const float dvar = cv.R[0][v] * cv.R[0][v] * G[0][0] + cv.R[1][v] * cv.R[1][v] * G[1][1] + cv.R[2][v] * cv.R[2][v] * G[2][2] +
                           2.0f * (cv.R[0][v] * cv.R[1][v] * G[0][1] + cv.R[0][v] * cv.R[2][v] * G[0][2] + cv.R[1][v] * cv.R[2][v] * G[1][2]);
        if constexpr (FILTER3D) g_scales_raw[3 * size_t(i) + v] = (2.0f * cv.var[v] * dvar) * (1.f - u3[v]) + a2.x * u3[v];
        else g_scales_raw[3 * size_t(i) + v] = 2.0f * cv.var[v] * dvar;
    }
    float dR[3][3];
#pragma unroll
    for (int u = 0; u < 3; ++u)
#pragma unroll
        for (int v = 0; v < 3; ++v) dR[u][v] = 2.0f * (cv.RS[0][v] * G[u][0] + cv.RS[1][v] * G[u][1] + cv.RS[2][v] * G[u][2]);
    const float dqxx = -dR[1][1] - dR[2][2], dqyy = -dR[0][0] - dR[2][2], dqzz = -dR[0][0] - dR[1][1];
    const float dqxy = dR[0][1] + dR[1][0], dqxz = dR[0][2] + dR[2][0], dqyz = dR[1][2] + dR[2][1];
    const float dqrx = dR[2][1] - dR[1][2], dqry = dR[0][2] - dR[2][0], dqrz = dR[1][0] - dR[0][1];
    const float hn = cv.qxx * dqxx + cv.qyy * dqyy + cv.qzz * dqzz + cv.qxy * dqxy + cv.qxz * dqxz + cv.qyz * dqyz + cv.qrx * dqrx + cv.qry * dqry + cv.qrz * dqrz;
    reinterpret_cast<float4*>(g_rot_raw)[i] = make_float4(
        2.0f * (cv.qx * dqrx + cv.qy * dqry + cv.qz * dqrz - cv.qr * hn) / cv.qn,
        2.0f * (2.0f * cv.qx * dqxx + cv.qy * dqxy + cv.qz * dqxz + cv.qr * dqrx - cv.qx * hn) / cv.qn,
        2.0f * (2.0f * cv.qy * dqyy + cv.qx * dqxy + cv.qz * dqyz + cv.qr * dqry - cv.qy * hn) / cv.qn,
        2.0f * (2.0f * cv.qz * dqzz + cv.qx * dqxz + cv.qy * dqyz + cv.qr * dqrz - cv.qz * hn) / cv.qn);
    if (densification_info != nullptr) { // kernels_backward.cuh:229-232
        const float gx = dm2[0] * 0.5f * float(f.width), gy = dm2[1] * 0.5f * float(f.height);
        densification_info[i] += 1.0f;
        densification_info[size_t(N) + i] += sqrtf(gx * gx + gy * gy);
    }
}

// Sum of W2C_VALS per-lane values over a 256-thread workgroup in a FIXED order (no float atomics: the result is the same bits on every run): wave64 butterfly,
// lane 0 of each wavefront -> LDS, then thread j < W2C_VALS adds the four wavefronts' values front to back. Every lane of the workgroup must call it.
constexpr uint32_t W2C_VALS = 12; // rows 0-2 of the [4,4] gradient, row-major
LFS_DI float block_sum12(float (&v)[W2C_VALS], float (*s_part)[W2C_VALS]) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
        for (uint32_t j = 0; j < W2C_VALS; ++j) v[j] += __shfl_xor(v[j], m, 64);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (uint32_t j = 0; j < W2C_VALS; ++j) s_part[threadIdx.x >> 6][j] = v[j];
    }
    __syncthreads();
    const uint32_t j = threadIdx.x < W2C_VALS ? threadIdx.x : 0u;
    return ((s_part[0][j] + s_part[1][j]) + s_part[2][j]) + s_part[3][j];
}

// W2C = false: the kernel as it always was (w2c_partials is not read or written). W2C = true (pose optimisation, rasterization_api.cu:133-136 /
// kernels_backward.cuh:165-183) additionally sums, over the primitives with n_touched > 0, grad_w2c[r][c] += dcam[r] * mean[c], grad_w2c[r][3] += dcam[r]:
// no lane leaves before the workgroup sum (rows past N and invisible primitives take part with dcam = 0), and the workgroup's 12 sums go to
// w2c_partials[blockIdx.x * 12 ..] with plain stores; fg_w2c_reduce_kernel adds the rows up.
// AA: the instantiation for the antialiased mode. The launcher queues both; the one that does not match the mode word the forward left in the workspace returns at once.
// DEPTH: 0 = the forms of a backward without a depth gradient, which look at the antialiased bit only (a depth-mode workspace is an ordinary workspace to
// them: slot 9 of the rows is zero and not read); 1 / 2 = the forms of a backward with grad_depth, which also require their depth bit in the mode word.
// FILTER3D: the forms of a backward with lfs_fastgs_view_ext::filter3d_var (chosen on the host, from its memory of the workspace); they require their bit in the mode
// word as the depth forms do. The kernels below the body are its FILTER3D = false / true wrappers under separate names.
template <bool W2C, bool AA, int DEPTH, bool FILTER3D>
LFS_DI void preprocess_bwd_body(
    const uint32_t N, const float* __restrict__ means, const float* __restrict__ scales_raw, const float* __restrict__ rot_raw,
    const Frame f, const GaussRec* __restrict__ rec, const float4* __restrict__ conic_opacity,
    const uint32_t* __restrict__ n_touched, const float* __restrict__ acc, float* __restrict__ g_means, float* __restrict__ g_scales_raw, float* __restrict__ g_rot_raw,
    float* __restrict__ g_opac_raw, float* __restrict__ densification_info, float* __restrict__ w2c_partials, const uint32_t* __restrict__ mode,
    const float* __restrict__ filter_var) {
    if (((*mode & MODE_ANTIALIASED) != 0u) != AA) return;   // (uniform: before any barrier)
    if constexpr (DEPTH != 0) { if ((*mode & depth_mode_bits(DEPTH)) == 0u) return; }
    if constexpr (FILTER3D) { if ((*mode & MODE_FILTER3D) == 0u) return; }
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if constexpr (!W2C) {   // the kernel as it was: the same early returns, no operand of the sum below exists
        if (i >= N) return;
        if (n_touched[i] == 0) { preprocess_bwd_zero_rows(i, g_means, g_scales_raw, g_rot_raw, g_opac_raw); return; }
        float dcam[3];
        preprocess_bwd_one<AA, DEPTH, FILTER3D>(i, N, means, scales_raw, rot_raw, f, rec, conic_opacity, acc, g_means, g_scales_raw, g_rot_raw, g_opac_raw, densification_info, dcam, filter_var);
    } else {
        __shared__ float s_part[4][W2C_VALS];
        float dcam[3] = {0.f, 0.f, 0.f}, m[3] = {0.f, 0.f, 0.f};
        bool visible = i < N;
        if (visible && n_touched[i] == 0) { preprocess_bwd_zero_rows(i, g_means, g_scales_raw, g_rot_raw, g_opac_raw); visible = false; }
        if (visible) {
            preprocess_bwd_one<AA, DEPTH, FILTER3D>(i, N, means, scales_raw, rot_raw, f, rec, conic_opacity, acc, g_means, g_scales_raw, g_rot_raw, g_opac_raw, densification_info, dcam, filter_var);
            m[0] = means[3 * size_t(i)]; m[1] = means[3 * size_t(i) + 1]; m[2] = means[3 * size_t(i) + 2];
        }
        float v[W2C_VALS];
#pragma unroll
        for (int r = 0; r < 3; ++r) { v[4 * r] = dcam[r] * m[0]; v[4 * r + 1] = dcam[r] * m[1]; v[4 * r + 2] = dcam[r] * m[2]; v[4 * r + 3] = dcam[r]; }
        const float sum = block_sum12(v, s_part);   // every lane of the workgroup arrives here
        if (threadIdx.x < W2C_VALS) w2c_partials[size_t(blockIdx.x) * W2C_VALS + threadIdx.x] = sum;
    }
}

#define LFS_FG_PREP_BWD_PARAMS \
    const uint32_t N, const float* __restrict__ means, const float* __restrict__ scales_raw, const float* __restrict__ rot_raw, \
    const Frame f, const GaussRec* __restrict__ rec, const float4* __restrict__ conic_opacity, \
    const uint32_t* __restrict__ n_touched, const float* __restrict__ acc, float* __restrict__ g_means, float* __restrict__ g_scales_raw, float* __restrict__ g_rot_raw, \
    float* __restrict__ g_opac_raw, float* __restrict__ densification_info, float* __restrict__ w2c_partials, const uint32_t* __restrict__ mode
#define LFS_FG_PREP_BWD_ARGS N, means, scales_raw, rot_raw, f, rec, conic_opacity, n_touched, acc, g_means, g_scales_raw, g_rot_raw, g_opac_raw, densification_info, w2c_partials, mode
template <bool W2C, bool AA, int DEPTH>
__global__ void __launch_bounds__(256) fg_preprocess_bwd_kernel(LFS_FG_PREP_BWD_PARAMS) {
    preprocess_bwd_body<W2C, AA, DEPTH, false>(LFS_FG_PREP_BWD_ARGS, nullptr);
}
template <bool W2C, bool AA, int DEPTH>
__global__ void __launch_bounds__(256) fg_preprocess_bwd_f3d_kernel(LFS_FG_PREP_BWD_PARAMS, const float* __restrict__ filter_var) {
    preprocess_bwd_body<W2C, AA, DEPTH, true>(LFS_FG_PREP_BWD_ARGS, filter_var);
}
#undef LFS_FG_PREP_BWD_PARAMS
#undef LFS_FG_PREP_BWD_ARGS

// one workgroup: the n_rows partial rows of fg_preprocess_bwd_kernel<true> -> grad_w2c [4,4], all 16 floats written (row 3 = 0; n_rows == 0 -> all zeros).
// Thread t adds rows t, t + 256, ... in that order, then the same workgroup sum as above.
__global__ void __launch_bounds__(256) fg_w2c_reduce_kernel(const uint32_t n_rows, const float* __restrict__ w2c_partials, float* __restrict__ grad_w2c) {
    __shared__ float s_part[4][W2C_VALS];
    float v[W2C_VALS];
#pragma unroll
    for (uint32_t j = 0; j < W2C_VALS; ++j) v[j] = 0.f;
    for (uint32_t row = threadIdx.x; row < n_rows; row += 256) {
        const float4* p = reinterpret_cast<const float4*>(w2c_partials + size_t(row) * W2C_VALS);
        const float4 a = p[0], b = p[1], c = p[2];
        v[0] += a.x; v[1] += a.y; v[2] += a.z; v[3] += a.w; v[4] += b.x; v[5] += b.y; v[6] += b.z; v[7] += b.w; v[8] += c.x; v[9] += c.y; v[10] += c.z; v[11] += c.w;
    }
    const float sum = block_sum12(v, s_part);
    if (threadIdx.x < 16) grad_w2c[threadIdx.x] = threadIdx.x < W2C_VALS ? sum : 0.f;
}

// densification_info of an absgrad backward (LFS_FASTGS_ABSGRAD): the per-primitive backward above ran with densification_info = nullptr, this kernel makes the two entries from
// slots 10 / 11 of the row (sum |k gx_p|, sum |k gy_p| of fg_blend_bwd_abs_kernel, k = 0.5 log2(e)) - the expression of preprocess_bwd_one with the |.|-sums in place of dm2.
// One thread per Gaussian, whatever the antialiasing / depth / filter mode; the workspace's mode word must carry the bit (as the depth and filter forms check theirs).
__global__ void __launch_bounds__(256) fg_densify_abs_kernel(const uint32_t N, const uint32_t width, const uint32_t height, const uint32_t* __restrict__ n_touched,
                                                             const float* __restrict__ acc, float* __restrict__ densification_info, const uint32_t* __restrict__ mode) {
    if ((*mode & MODE_ABSGRAD) == 0u) return;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N || n_touched[i] == 0) return;
    const float2 G = *reinterpret_cast<const float2*>(acc + size_t(i) * ACC_STRIDE + 10);
    constexpr float K_RCP = 2.0f / LOG2E;
    const float gx = (G.x * K_RCP) * 0.5f * float(width), gy = (G.y * K_RCP) * 0.5f * float(height);
    densification_info[i] += 1.0f;
    densification_info[size_t(N) + i] += sqrtf(gx * gx + gy * gy);
}
// the absgrad bit of the mode word: the preprocess kernels write the word from their template parameters, which know nothing of it (it changes nothing in them)
__global__ void fg_mode_or_kernel(uint32_t* __restrict__ mode, const uint32_t bits) { *mode |= bits; }

static inline uint32_t per_block_for(uint32_t N) {
    size_t pb = (size_t(N) + 511) / 512;
    if (pb < 1024) pb = 1024;
    return uint32_t((pb + 1023) / 1024 * 1024);
}

// host-side launchers used by fastgs_blend.hip as well
size_t w2c_workspace_bytes(uint32_t N) { // one row of 12 floats per workgroup of fg_preprocess_bwd_kernel<true> (never 0: N == 0 still gets a valid pointer)
    const size_t rows = (size_t(N) + 255) / 256;
    return align256(sizeof(float) * W2C_VALS * (rows ? rows : 1));
}
int launch_w2c_reduce(uint32_t N, const float* w2c_partials, float* grad_w2c, hipStream_t s) {   // N == 0: no partial rows, grad_w2c = 0
    lfs::ProfScope prof("fastgs_w2c_reduce", s);
    hipLaunchKernelGGL(fg_w2c_reduce_kernel, dim3(1), dim3(256), 0, s, (N + 255) / 256, w2c_partials, grad_w2c);
    return (int)hipGetLastError();
}
int launch_scatter(uint32_t N, const Frame& f, const PrimWs& w, int64_t* keys, hipStream_t s) {
    const uint32_t T = f.gw * f.gh, pb = per_block_for(N), blocks = (N + pb - 1) / pb;
    lfs::ProfScope prof("fastgs_scatter", s);
    if (size_t(T) * 8 <= 64 * 1024)
        hipLaunchKernelGGL(fg_scatter_kernel<true>, dim3(blocks), dim3(1024), size_t(T) * 8, s, N, pb, f, w.mean2d, w.conic_opacity, w.bounds, w.n_touched, w.depth_bits, w.offsets, w.cursor, keys);
    else
        hipLaunchKernelGGL(fg_scatter_kernel<false>, dim3(blocks), dim3(1024), 0, s, N, pb, f, w.mean2d, w.conic_opacity, w.bounds, w.n_touched, w.depth_bits, w.offsets, w.cursor, keys);
    return (int)hipGetLastError();
}
Frame make_frame(const lfs_fastgs_view& v) {
    return Frame{v.w2c, v.cam_position, v.active_sh_bases, v.total_bases_sh_rest, v.width, v.height, (v.width + TILE - 1) / TILE, (v.height + TILE - 1) / TILE,
                 v.fx, v.fy, v.cx, v.cy, v.near_plane, v.far_plane};
}
int launch_preprocess_bwd(const lfs_fastgs_view& v, const Frame& f, const PrimWs& w, const lfs_fastgs_view_backward_args& a, const float* sh_rest, const ShAdamArgs* adam,
                          const WsMode& mode, const float* filter_var, hipStream_t s) {
    const uint32_t N = v.N;
    float* const w2c_partials = a.grad_w2c ? static_cast<float*>(a.w2c_workspace) : nullptr;
    float* const densification_info = mode.absgrad ? nullptr : a.densification_info;   // absgrad: fg_densify_abs_kernel below writes it
    {
        // the mode of the forward that filled this workspace is a word IN the workspace, which the host does not read: both AA instantiations are queued, one returns
        // at once. (depth, w2c) pick the pair on the host. (The table lists the kernels in the order the code object has always had them: with W2C first.)
        lfs::ProfScope prof("fastgs_preprocess_bwd", s);
#define LFS_FG_PREP_BWD_PAIR(W2C, DEPTH) {&fg_preprocess_bwd_kernel<W2C, false, DEPTH>, &fg_preprocess_bwd_kernel<W2C, true, DEPTH>}
        static constexpr decltype(&fg_preprocess_bwd_kernel<false, false, 0>) kernels[3][2][2] = {   // [depth][without grad_w2c][antialiased]
            {LFS_FG_PREP_BWD_PAIR(true, 0), LFS_FG_PREP_BWD_PAIR(false, 0)}, {LFS_FG_PREP_BWD_PAIR(true, 1), LFS_FG_PREP_BWD_PAIR(false, 1)},
            {LFS_FG_PREP_BWD_PAIR(true, 2), LFS_FG_PREP_BWD_PAIR(false, 2)}};
#undef LFS_FG_PREP_BWD_PAIR
#define LFS_FG_PREP_BWD_F3D_PAIR(W2C, DEPTH) {&fg_preprocess_bwd_f3d_kernel<W2C, false, DEPTH>, &fg_preprocess_bwd_f3d_kernel<W2C, true, DEPTH>}
        static constexpr decltype(&fg_preprocess_bwd_f3d_kernel<false, false, 0>) kernels_f3d[3][2][2] = {   // the filtered forms, in the same order
            {LFS_FG_PREP_BWD_F3D_PAIR(true, 0), LFS_FG_PREP_BWD_F3D_PAIR(false, 0)}, {LFS_FG_PREP_BWD_F3D_PAIR(true, 1), LFS_FG_PREP_BWD_F3D_PAIR(false, 1)},
            {LFS_FG_PREP_BWD_F3D_PAIR(true, 2), LFS_FG_PREP_BWD_F3D_PAIR(false, 2)}};
#undef LFS_FG_PREP_BWD_F3D_PAIR
        if (filter_var != nullptr) {
            for (const auto kernel : kernels_f3d[mode.depth][a.grad_w2c == nullptr])
                hipLaunchKernelGGL(kernel, dim3((N + 255) / 256), dim3(256), 0, s, N, v.means, v.scales_raw, v.rotations_raw, f, w.rec, w.conic_opacity, w.n_touched, w.acc,
                                   a.grad_means, a.grad_scales_raw, a.grad_rotations_raw, a.grad_opacities_raw, densification_info, w2c_partials, w.mode, filter_var);
        } else {
            for (const auto kernel : kernels[mode.depth][a.grad_w2c == nullptr])
                hipLaunchKernelGGL(kernel, dim3((N + 255) / 256), dim3(256), 0, s, N, v.means, v.scales_raw, v.rotations_raw, f, w.rec, w.conic_opacity, w.n_touched, w.acc,
                                   a.grad_means, a.grad_scales_raw, a.grad_rotations_raw, a.grad_opacities_raw, densification_info, w2c_partials, w.mode);
        }
    }
    if (mode.absgrad) {
        lfs::ProfScope prof("fastgs_densify_abs", s);
        hipLaunchKernelGGL(fg_densify_abs_kernel, dim3((N + 255) / 256), dim3(256), 0, s, N, f.width, f.height, w.n_touched, w.acc, a.densification_info, w.mode);
    }
    if (a.grad_w2c != nullptr) {
        const int rc = launch_w2c_reduce(N, w2c_partials, a.grad_w2c, s);
        if (rc) return rc;
    }
    // SH backward (convert_sh_to_color_backward, kernel_utils.cuh:38-106) with the coalesced three-phase kernel of sh.hip: reads dL/d(clamped colour) from the
    // accumulator rows (floats 6..8 of 16), the clamp mask from the record's colour (floats 8..10 of 16), writes g_sh0 / g_sh_rest fully, adds dL/dposition to g_means
    const uint32_t degree = f.active_sh_bases >= 16 ? 3 : f.active_sh_bases >= 9 ? 2 : f.active_sh_bases >= 4 ? 1 : 0;
    return sh_records_bwd(N, 1 + f.total_rest, degree, v.means, f.cam_pos, v.sh_coefficients_0, sh_rest, w.n_touched, reinterpret_cast<const float*>(w.rec) + 8, 16,
                          w.acc + 5, 16, a.grad_sh_coefficients_0, adam ? nullptr : a.grad_sh_coefficients_rest, a.grad_means, s, adam);
}

} // namespace fgs
} // namespace lfs

using namespace lfs;

namespace lfs { namespace fgs {
// one pinned int64 + event per process: the reference's trainer (and this one) has a single rendering thread
struct Readback { int64_t* host = nullptr; hipEvent_t event = nullptr; bool armed = false; };
static Readback& readback() {
    static Readback rb = [] {
        Readback r;
        if (hipHostMalloc((void**)&r.host, sizeof(int64_t), hipHostMallocDefault) != hipSuccess) r.host = nullptr;
        if (hipEventCreateWithFlags(&r.event, hipEventDisableTiming) != hipSuccess) r.event = nullptr;
        return r;
    }();
    return rb;
}

// The flags of the preprocess that last filled a primitive workspace, by the workspace's address: what the host picks and validates by - render's depth plane, the
// backward's grad_depth, its filtered and its abs form - without reading the mode word back (that would be a host sync). Only workspaces filled with a mode the host must
// know - a depth mode, the 3D filter or absgrad - take an entry; a preprocess without one erases the entry of its address (the workspace counts as a default one again)
// and takes none, so ordinary forwards - evaluation renders, other views - never push such a workspace out. MODE_SLOTS such forwards can be outstanding (filled, their
// backward still to come); one more evicts the least recently filled, which then counts as a default workspace: its depth plane, its grad_depth and a backward with the
// filter's variances are refused with LFS_E_INVALID (fastgs.py names that cause in its error), and a backward on it runs the default form in place of the abs form. Device
// addresses are unique across the devices of a process (one unified address space), so the address alone is the key. A mutex guards the table: the entry points may
// be called from several host threads.
constexpr int MODE_SLOTS = 256;
struct ModeSlot { const void* ws = nullptr; uint32_t flags = 0; uint64_t stamp = 0; };
static ModeSlot g_mode_slots[MODE_SLOTS];
static uint64_t g_mode_stamp = 0;
static std::mutex g_mode_mutex;
static void remember_flags(const void* ws, uint32_t flags) {
    const bool takes_entry = (flags & (MODE_DEPTH | MODE_INVDEPTH | MODE_FILTER3D | MODE_ABSGRAD)) != 0;   // a depth mode, the 3D filter or absgrad
    std::lock_guard<std::mutex> lock(g_mode_mutex);
    ModeSlot* pick = &g_mode_slots[0];
    for (ModeSlot& m : g_mode_slots) {
        if (m.ws == ws) { pick = &m; break; }
        if (m.stamp < pick->stamp) pick = &m;
    }
    if (!takes_entry) {
        if (pick->ws == ws) *pick = ModeSlot{};
        return;
    }
    pick->ws = ws; pick->flags = flags; pick->stamp = ++g_mode_stamp;
}
uint32_t remembered_flags(const void* ws) {   // 0: a workspace that was not (or not recently enough) filled by a preprocess with a depth mode, the 3D filter or absgrad
    std::lock_guard<std::mutex> lock(g_mode_mutex);
    for (const ModeSlot& m : g_mode_slots)
        if (m.ws == ws && m.stamp != 0) return m.flags;
    return 0u;
}
} } // namespace lfs::fgs

// n_instances of the last lfs_fastgs_view_preprocess call on this process: waits for the read-back event only (not for the SH kernel queued after it)
extern "C" int lfs_fastgs_wait_n_instances(int64_t* n_instances) {
    if (!n_instances) return LFS_E_INVALID;
    lfs::fgs::Readback& rb = lfs::fgs::readback();
    if (!rb.armed) return LFS_E_INVALID;
    const hipError_t e = hipEventSynchronize(rb.event);
    if (e != hipSuccess) return (int)e;
    *n_instances = *rb.host;
    rb.armed = false;
    return LFS_OK;
}

extern "C" size_t lfs_fastgs_primitive_workspace_bytes(uint32_t N, uint32_t width, uint32_t height) {
    return fgs::prim_ws(nullptr, N, width, height, (lfs_get_debug_flags() & 16u) != 0).bytes;   // (the deterministic backward's int64 rows: lfs_fastgs.cuh)
}
extern "C" size_t lfs_fastgs_instance_workspace_bytes(uint32_t width, uint32_t height, int64_t n_instances) {
    return n_instances < 0 ? 0 : fgs::inst_ws(nullptr, width, height, uint64_t(n_instances)).bytes;
}

// flags bit 0 (LFS_FASTGS_ANTIALIASED): the antialiased mode of fg_preprocess_kernel. The mode is recorded in the primitive workspace (PrimWs::mode), rewritten by
// every call with N > 0; render and the backward need no flag.
// bits 2 / 3 (LFS_FASTGS_DEPTH / LFS_FASTGS_INVDEPTH, exclusive): the depth forms of the kernel; the host remembers the flags by the workspace's address for the
// render's depth plane and the backward's grad_depth (remember_flags).
static_assert(sizeof(lfs_fastgs_view) == 136, "the ctypes mirror (capi.py) is laid out by hand");
// bit 5 (LFS_FASTGS_ABSGRAD): nothing in this stage changes; the bit is OR-ed into the mode word and remembered on the host, where the backward picks its abs form by it.
// filter_var (lfs_fastgs_view_ext::filter3d_var): the filtered forms (fg_preprocess_f3d_kernel); the workspace is remembered with the internal MODE_FILTER3D bit next to
// its public flags.
static int view_preprocess(const lfs_fastgs_view* view, uint32_t flags, const float* filter_var, int64_t* n_instances, lfs_stream_t stream);
extern "C" int lfs_fastgs_view_preprocess(const lfs_fastgs_view* view, uint32_t flags, int64_t* n_instances, lfs_stream_t stream) {
    return view_preprocess(view, flags, nullptr, n_instances, stream);
}
extern "C" int lfs_fastgs_view_preprocess_ex(const lfs_fastgs_view* view, uint32_t flags, const lfs_fastgs_view_ext* ext, int64_t* n_instances, lfs_stream_t stream) {
    return view_preprocess(view, flags, ext ? ext->filter3d_var : nullptr, n_instances, stream);
}
static int view_preprocess(const lfs_fastgs_view* view, uint32_t flags, const float* filter_var, int64_t* n_instances, lfs_stream_t stream) {
    if (!view) return LFS_E_INVALID;
    const lfs_fastgs_view& v = *view;
    if (flags & ~uint32_t(LFS_FASTGS_ANTIALIASED | LFS_FASTGS_DEPTH | LFS_FASTGS_INVDEPTH | LFS_FASTGS_ABSGRAD)) return LFS_E_INVALID;
    if ((flags & LFS_FASTGS_DEPTH) && (flags & LFS_FASTGS_INVDEPTH)) return LFS_E_INVALID;
    static_assert(LFS_FASTGS_ANTIALIASED == fgs::MODE_ANTIALIASED && LFS_FASTGS_DEPTH == fgs::MODE_DEPTH && LFS_FASTGS_INVDEPTH == fgs::MODE_INVDEPTH &&
                  LFS_FASTGS_ABSGRAD == fgs::MODE_ABSGRAD, "the mode word holds the flags");
    const bool aa = (flags & LFS_FASTGS_ANTIALIASED) != 0;
    const int depth = (flags & LFS_FASTGS_DEPTH) ? 1 : (flags & LFS_FASTGS_INVDEPTH) ? 2 : 0;
    const uint32_t N = v.N;
    if (!n_instances || !v.primitive_workspace || !v.w2c || !v.cam_position || v.width == 0 || v.height == 0) return LFS_E_INVALID;
    if (v.active_sh_bases == 0 || v.active_sh_bases > 16 || (v.active_sh_bases > 1 && v.total_bases_sh_rest + 1 < v.active_sh_bases)) return LFS_E_INVALID;
    fgs::PrimWs w = fgs::prim_ws(v.primitive_workspace, N, v.width, v.height);
    if (v.primitive_workspace_bytes < w.bytes) return LFS_E_WORKSPACE;
    if (N > 0 && (!v.means || !v.scales_raw || !v.rotations_raw || !v.opacities_raw || !v.sh_coefficients_0 || (v.total_bases_sh_rest > 0 && !v.sh_coefficients_rest)))
        return LFS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const fgs::Frame f = fgs::make_frame(v);
    const uint32_t T = f.gw * f.gh;
    if (T > 65535u) return LFS_E_UNSUPPORTED; // bounds are ushort4 (as in the reference: ushort tile keys)
    hipError_t e = hipMemsetAsync(w.totals, 0, (char*)w.offsets - (char*)w.totals, s); // totals + cursor
    if (e != hipSuccess) return (int)e;
    {
        lfs::ProfScope prof("fastgs_preprocess", s);
        if (N > 0) {
            const uint32_t pb = fgs::per_block_for(N), blocks = (N + pb - 1) / pb;
            const bool lds = size_t(T) * 8 <= 64 * 1024;
#define LFS_FG_PREP_ROW(LDS, AA) {&fgs::fg_preprocess_kernel<LDS, AA, 0>, &fgs::fg_preprocess_kernel<LDS, AA, 1>, &fgs::fg_preprocess_kernel<LDS, AA, 2>}
            static constexpr decltype(&fgs::fg_preprocess_kernel<false, false, 0>) kernels[2][2][3] = {   // [no LDS][default mode][depth]: the code object's order
                {LFS_FG_PREP_ROW(true, true), LFS_FG_PREP_ROW(true, false)}, {LFS_FG_PREP_ROW(false, true), LFS_FG_PREP_ROW(false, false)}};
#undef LFS_FG_PREP_ROW
#define LFS_FG_PREP_F3D_ROW(LDS, AA) {&fgs::fg_preprocess_f3d_kernel<LDS, AA, 0>, &fgs::fg_preprocess_f3d_kernel<LDS, AA, 1>, &fgs::fg_preprocess_f3d_kernel<LDS, AA, 2>}
            static constexpr decltype(&fgs::fg_preprocess_f3d_kernel<false, false, 0>) kernels_f3d[2][2][3] = {   // the filtered forms, in the same order
                {LFS_FG_PREP_F3D_ROW(true, true), LFS_FG_PREP_F3D_ROW(true, false)}, {LFS_FG_PREP_F3D_ROW(false, true), LFS_FG_PREP_F3D_ROW(false, false)}};
#undef LFS_FG_PREP_F3D_ROW
            if (filter_var != nullptr)
                hipLaunchKernelGGL(kernels_f3d[!lds][!aa][depth], dim3(blocks), dim3(1024), lds ? size_t(T) * 4 : size_t(0), s, N, pb, v.means, v.scales_raw, v.rotations_raw,
                                   v.opacities_raw, f, w.rec, w.mean2d, w.conic_opacity, w.bounds, w.n_touched, w.depth_bits, w.totals, w.mode, filter_var);
            else
                hipLaunchKernelGGL(kernels[!lds][!aa][depth], dim3(blocks), dim3(1024), lds ? size_t(T) * 4 : size_t(0), s, N, pb, v.means, v.scales_raw, v.rotations_raw,
                                   v.opacities_raw, f, w.rec, w.mean2d, w.conic_opacity, w.bounds, w.n_touched, w.depth_bits, w.totals, w.mode);
        }
        if (N > 0 && (flags & LFS_FASTGS_ABSGRAD)) hipLaunchKernelGGL(fgs::fg_mode_or_kernel, dim3(1), dim3(1), 0, s, w.mode, fgs::MODE_ABSGRAD);
        hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(1024), 0, s, T, w.totals, w.offsets, n_instances);
    }
    // The host needs n_instances to size the instance workspace (the reference syncs here, forward.cu:114-117). Queue the read-back BEFORE the SH
    // launch and mark it with an event: lfs_fastgs_wait_n_instances() then returns as soon as the count has landed while the GPU is already
    // evaluating SH colours, instead of idling through the host round trip (~40 us).
    {
        fgs::Readback& rb = fgs::readback();
        if (rb.host && rb.event) {
            if (hipMemcpyAsync(rb.host, n_instances, sizeof(int64_t), hipMemcpyDeviceToHost, s) == hipSuccess) { (void)hipEventRecord(rb.event, s); rb.armed = true; }
        }
    }
    if (N > 0) { // SH colour (convert_sh_to_color, kernel_utils.cuh:15-36) of the visible primitives, written into the records
        const uint32_t degree = v.active_sh_bases >= 16 ? 3 : v.active_sh_bases >= 9 ? 2 : v.active_sh_bases >= 4 ? 1 : 0;
        const int rc = sh_records_fwd(N, 1 + v.total_bases_sh_rest, degree, v.means, v.cam_position, v.sh_coefficients_0, v.sh_coefficients_rest, w.n_touched,
                                      reinterpret_cast<float*>(w.rec) + 8, 16, s);
        if (rc) return rc;
    }
    const int rc = (int)hipGetLastError();
    if (rc == 0) fgs::remember_flags(v.primitive_workspace, flags | (filter_var != nullptr ? fgs::MODE_FILTER3D : 0u));
    return rc;
}
