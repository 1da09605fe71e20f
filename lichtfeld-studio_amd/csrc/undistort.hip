// Undistortion at load: a source image taken through one of COLMAP's lens models is resampled, once per image, to the distortion-free pinhole
// camera the rasterizers render (lichtfeld-studio_amd/undistort.py chooses that camera). One kernel body, templated on what is resampled:
//   * lfs_image_undistort_u8_to_chw_f32 - the training target: one bilinear tap with the arithmetic and the 8-bit re-quantisation of image_to_chw_kernel
//     (dataprep.hip), plus the validity plane;
//   * lfs_mask_undistort_prepare        - mask_prepare_kernel through the same positions (a mask stays registered with its image), blank pixels forced to 0, the
//     two exact integer sums;
//   * lfs_plane_undistort_nearest_f32   - a float plane (depth targets) by nearest neighbour, NaN where there is no source.
// The destination pixel centre is normalised with the destination intrinsics, distorted with the camera model of lfs_camera.cuh (cam_distortion: rational radial,
// tangential, thin-prism; the fisheye polynomial of cam_project) and scaled to a source position. The map is a kernel ARGUMENT (by value): every coefficient is
// wave-uniform and stays in SGPRs. One thread per destination pixel, 64 x 4 pixels per block; no float atomics, no host read, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/lfs_gsplat.h"
#include "lfs_camera.cuh"
#include "lfs_prof.h"

namespace lfs {
namespace ud {

// destination pixel (x, y) -> source position (continuous image coordinates, pixel centres at +0.5); returns the pixel's validity
LFS_DI bool source_position(const lfs_undistort_map& m, int x, int y, float& sx, float& sy) {
    CamDev cam; // only what the model functions below read
    cam.model = m.model;
#pragma unroll
    for (int i = 0; i < 6; ++i) cam.radial[i] = m.radial[i];
    cam.tangential[0] = m.tangential[0], cam.tangential[1] = m.tangential[1];
#pragma unroll
    for (int i = 0; i < 4; ++i) cam.thin[i] = m.thin[i];
    const f2 uv{((float)x + 0.5f - m.dst_cx) / m.dst_fx, ((float)y + 0.5f - m.dst_cy) / m.dst_fy};
    f2 nd;
    bool ok;
    if (m.model == LFS_CAMERA_FISHEYE) {
        cam.fwd_odd[0] = 1.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) cam.fwd_odd[i + 1] = m.radial[i];
        const float r = stable_norm2(uv.x, uv.y);
        const float theta = atanf(r);
        const float s = r > 0.f ? theta * poly5(cam.fwd_odd, theta * theta) / r : 1.f;
        nd = {s * uv.x, s * uv.y};
        ok = theta < m.max_angle;
    } else {
        float icD;
        f2 d;
        cam_distortion(cam, uv, icD, d);
        nd = {icD * uv.x + d.x, icD * uv.y + d.y};
        ok = icD > 0.8f; // the projection's own criterion (cam_project)
    }
    sx = nd.x * m.src_fx + m.src_cx, sy = nd.y * m.src_fy + m.src_cy;
    // all four taps inside the source (a NaN position fails every comparison)
    ok = ok && sx >= 0.5f && sx <= (float)m.src_width - 0.5f && sy >= 0.5f && sy <= (float)m.src_height - 0.5f;
    return ok;
}

// the 2x2 texels and weights of image_to_chw_kernel at a source position
struct Tap {
    int x0, x1, y0, y1;
    float ax, ay;
};
LFS_DI Tap tap_at(const lfs_undistort_map& m, float sx, float sy) {
    const int sw = (int)m.src_width, sh = (int)m.src_height;
    const float fx = sx - 0.5f, fy = sy - 0.5f;
    const float flx = floorf(fx), fly = floorf(fy);
    Tap t;
    t.ax = fx - flx, t.ay = fy - fly;
    t.x0 = min(max((int)flx, 0), sw - 1), t.x1 = min(max((int)flx + 1, 0), sw - 1);
    t.y0 = min(max((int)fly, 0), sh - 1), t.y1 = min(max((int)fly + 1, 0), sh - 1);
    return t;
}
// OIIO's bilerp order and the store as u8 with round-to-nearest, as image_to_chw_kernel
LFS_DI int bilerp_u8(const Tap& t, uint8_t b00, uint8_t b01, uint8_t b10, uint8_t b11) {
    const float v00 = (float)b00 * (1.0f / 255.0f), v01 = (float)b01 * (1.0f / 255.0f);
    const float v10 = (float)b10 * (1.0f / 255.0f), v11 = (float)b11 * (1.0f / 255.0f);
    const float top = (1.0f - t.ax) * v00 + t.ax * v01, bot = (1.0f - t.ax) * v10 + t.ax * v11;
    const float v = (1.0f - t.ay) * top + t.ay * bot;
    return (int)fminf(fmaxf(v * 255.0f + 0.5f, 0.0f), 255.0f);
}

struct ImagePayload { // u8 [sh,sw,3] -> f32 [3,dh,dw] + validity u8 [dh,dw]
    const uint8_t* __restrict__ src;
    float* __restrict__ dst;
    uint8_t* __restrict__ valid;
    struct Acc {};
    LFS_DI void pixel(const lfs_undistort_map& m, int x, int y, bool ok, float sx, float sy, Acc&) const {
        const size_t plane = (size_t)m.dst_width * m.dst_height, o = (size_t)y * m.dst_width + x;
        valid[o] = ok ? 255 : 0;
        if (!ok) {
#pragma unroll
            for (int c = 0; c < 3; ++c) dst[c * plane + o] = 0.f;
            return;
        }
        const Tap t = tap_at(m, sx, sy);
        const size_t sw = m.src_width;
        const uint8_t* p00 = src + ((size_t)t.y0 * sw + t.x0) * 3;
        const uint8_t* p01 = src + ((size_t)t.y0 * sw + t.x1) * 3;
        const uint8_t* p10 = src + ((size_t)t.y1 * sw + t.x0) * 3;
        const uint8_t* p11 = src + ((size_t)t.y1 * sw + t.x1) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) dst[c * plane + o] = (float)bilerp_u8(t, p00[c], p01[c], p10[c], p11[c]) / 255.0f;
    }
    LFS_DI void finish(const Acc&) const {}
};

struct MaskPayload { // u8 [sh,sw] (or no file) -> u8 [dh,dw] + sums[2], as mask_prepare_kernel
    const uint8_t* __restrict__ src;
    uint8_t* __restrict__ dst;
    int invert, threshold;
    unsigned long long* __restrict__ sums;
    struct Acc {
        unsigned int m = 0, m_crop = 0;
    };
    LFS_DI void pixel(const lfs_undistort_map& m, int x, int y, bool ok, float sx, float sy, Acc& acc) const {
        const int dw = (int)m.dst_width, dh = (int)m.dst_height;
        int q = 0;
        if (ok) {
            if (!src) {
                q = 255; // no mask file: the validity plane
            } else {
                const Tap t = tap_at(m, sx, sy);
                const size_t sw = m.src_width;
                q = bilerp_u8(t, src[(size_t)t.y0 * sw + t.x0], src[(size_t)t.y0 * sw + t.x1], src[(size_t)t.y1 * sw + t.x0], src[(size_t)t.y1 * sw + t.x1]);
                if (threshold >= 0) q = q >= threshold ? 255 : 0;
                if (invert) q = 255 - q;
            }
        }
        dst[(size_t)y * dw + x] = (uint8_t)q;
        acc.m = (unsigned int)q;
        const bool crop = dh > 10 && dw > 10;
        acc.m_crop = (!crop || (x >= 5 && x < dw - 5 && y >= 5 && y < dh - 5)) ? acc.m : 0u;
    }
    // integer wave sums, one 64-bit integer atomic per block and sum: exact, the same on every run
    LFS_DI void finish(const Acc& acc) const {
        unsigned int m = acc.m, m_crop = acc.m_crop;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { m += __shfl_xor(m, d, 64); m_crop += __shfl_xor(m_crop, d, 64); }
        __shared__ unsigned int part[2][4];
        if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = m; part[1][threadIdx.x >> 6] = m_crop; }
        __syncthreads();
        if (threadIdx.x < 2) {
            const unsigned int v = part[threadIdx.x][0] + part[threadIdx.x][1] + part[threadIdx.x][2] + part[threadIdx.x][3];
            if (v) atomicAdd(&sums[threadIdx.x], (unsigned long long)v);
        }
    }
};

struct PlanePayload { // f32 [sh,sw] -> f32 [dh,dw]: the texel that contains the position (interpolate(mode = "nearest") picks by position as well)
    const float* __restrict__ src;
    float* __restrict__ dst;
    struct Acc {};
    LFS_DI void pixel(const lfs_undistort_map& m, int x, int y, bool ok, float sx, float sy, Acc&) const {
        float v = __uint_as_float(0x7fc00000u);
        if (ok) {
            const int ix = min(max((int)floorf(sx), 0), (int)m.src_width - 1), iy = min(max((int)floorf(sy), 0), (int)m.src_height - 1);
            v = src[(size_t)iy * m.src_width + ix];
        }
        dst[(size_t)y * m.dst_width + x] = v;
    }
    LFS_DI void finish(const Acc&) const {}
};

template <class Payload>
__global__ void __launch_bounds__(256) undistort_kernel(const lfs_undistort_map m, const Payload p) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    typename Payload::Acc acc;
    if (x < (int)m.dst_width && y < (int)m.dst_height) {
        float sx, sy;
        const bool ok = source_position(m, x, y, sx, sy);
        p.pixel(m, x, y, ok, sx, sy, acc);
    }
    p.finish(acc); // (every thread of the block: the mask's sums cross lanes)
}

bool map_ok(const lfs_undistort_map* m) {
    if (!m) return false;
    if (m->model != LFS_CAMERA_PINHOLE && m->model != LFS_CAMERA_FISHEYE) return false;
    if (!m->src_width || !m->src_height || !m->dst_width || !m->dst_height) return false;
    if (m->src_width >= (1u << 30) || m->src_height >= (1u << 30) || m->dst_width >= (1u << 30) || m->dst_height >= (1u << 30)) return false;
    if (!(m->src_fx > 0.f) || !(m->src_fy > 0.f) || !(m->dst_fx > 0.f) || !(m->dst_fy > 0.f)) return false;
    if (m->model == LFS_CAMERA_FISHEYE && !(m->max_angle > 0.f)) return false;
    return true;
}

dim3 grid_of(const lfs_undistort_map& m) { return dim3((m.dst_width + 63) / 64, (m.dst_height + 3) / 4); }

} // namespace ud
} // namespace lfs

using namespace lfs::ud;

extern "C" int lfs_image_undistort_u8_to_chw_f32(const lfs_undistort_map* map, const uint8_t* src_hwc, float* dst_chw, uint8_t* valid_u8, lfs_stream_t stream) {
    if (!map_ok(map) || !src_hwc || !dst_chw || !valid_u8) return LFS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    lfs::ProfScope prof("image_undistort", s);
    hipLaunchKernelGGL(undistort_kernel<ImagePayload>, grid_of(*map), dim3(256), 0, s, *map, ImagePayload{src_hwc, dst_chw, valid_u8});
    return (int)hipGetLastError();
}

extern "C" int lfs_mask_undistort_prepare(const lfs_undistort_map* map, const uint8_t* src_u8, uint8_t* dst_u8, uint32_t invert, int32_t threshold, int64_t* sums,
                                          lfs_stream_t stream) {
    if (!map_ok(map) || !dst_u8 || !sums) return LFS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    lfs::ProfScope prof("mask_undistort_prepare", s);
    hipError_t e = hipMemsetAsync(sums, 0, 2 * sizeof(int64_t), s); // the sums are written, not accumulated
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(undistort_kernel<MaskPayload>, grid_of(*map), dim3(256), 0, s, *map,
                       MaskPayload{src_u8, dst_u8, invert ? 1 : 0, (int)threshold, (unsigned long long*)sums});
    return (int)hipGetLastError();
}

extern "C" int lfs_plane_undistort_nearest_f32(const lfs_undistort_map* map, const float* src_f32, float* dst_f32, lfs_stream_t stream) {
    if (!map_ok(map) || !src_f32 || !dst_f32) return LFS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    lfs::ProfScope prof("plane_undistort", s);
    hipLaunchKernelGGL(undistort_kernel<PlanePayload>, grid_of(*map), dim3(256), 0, s, *map, PlanePayload{src_f32, dst_f32});
    return (int)hipGetLastError();
}
