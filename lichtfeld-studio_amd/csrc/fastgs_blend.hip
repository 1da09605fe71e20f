// The reference's default training rasterizer ("fastgs", EWA splatting) — per-pixel stages:
// alpha blending forward (replaces blend_cu, fastgs/rasterization/include/kernels_forward.cuh:353-459) and backward
// (blend_backward_cu, kernels_backward.cuh:236-448), with the same CDNA4 structure as raster.hip: per-8x8-cell culling of
// the tile lists (here with the reference's own exact ellipse/rectangle test, kernel_utils.cuh:108-148, at cell
// granularity), one wavefront per cell walking its list with the 64-byte records arriving through the scalar unit, and a
// transposed wave reduction + one 64-byte atomic per (cell, primitive) in the backward. The reference instead keeps
// per-32-primitive (colour, transmittance) checkpoints of every pixel ("buckets", 16 B x 256 pixels per bucket) and runs the
// backward primitive-parallel; the sums are the same, the traversal here is back to front from the final transmittance.
#include "lfs_fastgs.cuh"
#include "lfs_prof.h"
#include "lfs_tilelists.cuh"

namespace lfs {
namespace fgs {

// cell-level version of kernel_utils.cuh:108-148 on the record's conic in bits (A, B, C) = log2(e) (a/2, b, c/2): the ratios that
// locate the maximum are scale free; thr already carries the safety margin
LFS_DI bool cell_reachable(float mx, float my, float A, float B, float C, float rx0, float ry0, float thr) {
    const float rx1 = rx0 + 7.f, ry1 = ry0 + 7.f;
    const float x_min_diff = rx0 - mx, y_min_diff = ry0 - my;
    const float x_left = x_min_diff > 0.f ? 1.f : 0.f, y_above = y_min_diff > 0.f ? 1.f : 0.f;
    const float not_in_x = x_left + (mx > rx1 ? 1.f : 0.f), not_in_y = y_above + (my > ry1 ? 1.f : 0.f);
    if (not_in_x + not_in_y == 0.f) return true;
    const float ccx = x_left > 0.f ? rx0 : rx1, ccy = y_above > 0.f ? ry0 : ry1;
    const float dfx = mx - ccx, dfy = my - ccy;
    const float dx = copysignf(7.f, x_min_diff), dy = copysignf(7.f, y_min_diff);
    const float tx = not_in_y * __saturatef((2.f * A * dfx + B * dfy) / (2.f * A * dx));
    const float ty = not_in_x * __saturatef((B * dfx + 2.f * C * dfy) / (2.f * C * dy));
    const float ddx = mx - (ccx + tx * dx), ddy = my - (ccy + ty * dy);
    return !(A * ddx * ddx + C * ddy * ddy + B * ddx * ddy > thr); // NaN -> keep
}

__global__ void __launch_bounds__(256) fg_cull_kernel(
    const uint32_t gw, const uint32_t gh, const uint32_t width, const uint32_t height, const uint32_t cull_enabled,
    const GaussRec* __restrict__ recs, const int32_t* __restrict__ offsets, const int32_t* __restrict__ ids,
    int32_t* __restrict__ cell_count, int2* __restrict__ cell_list) {
    __shared__ float4 s_a[2][256], s_b[2][256];
    __shared__ int32_t s_g[2][256];
    const uint32_t total_tiles = gw * gh;
    const CellCtx cc = cell_ctx(total_tiles, total_tiles, gw, TILE, 1, 4);
    if (!cc.in_grid) return;
    const uint32_t lane = threadIdx.x & 63;
    const size_t cell = size_t(cc.tile_global) * WPT + cc.wl;
    const int32_t start = offsets[cc.tile_global], end = offsets[cc.tile_global + 1];
    if (end <= start) {
        if (lane == 0) cell_count[cell] = 0;
        return;
    }
    const uint32_t x0 = (cc.tile_global % gw) * TILE + (cc.wl & 1) * 8, y0 = (cc.tile_global / gw) * TILE + (cc.wl >> 1) * 8;
    const bool cell_live = x0 < width && y0 < height;
    const float rx0 = float(x0), ry0 = float(y0);
    int2* __restrict__ out = cell_list + (size_t(WPT) * size_t(start) + size_t(cc.wl) * size_t(end - start));
    int32_t count = 0;
    auto fetch = [&](int32_t base, int32_t& g, float4& a, float4& b) {
        const int32_t i = base + int32_t(threadIdx.x);
        g = i < end ? ids[i] : 0;
        const float4* r = reinterpret_cast<const float4*>(recs + g);
        a = r[0]; b = r[1];
    };
    int32_t g_reg; float4 a_reg, b_reg;
    fetch(start, g_reg, a_reg, b_reg);
    int buf = 0;
    for (int32_t base = start; base < end; base += 256, buf ^= 1) {
        s_g[buf][threadIdx.x] = g_reg; s_a[buf][threadIdx.x] = a_reg; s_b[buf][threadIdx.x] = b_reg;
        __syncthreads();
        if (base + 256 < end) fetch(base + 256, g_reg, a_reg, b_reg);
        if (!cell_live) continue;
        for (int32_t sub = 0; sub < 4; ++sub) {
            if (base + (sub << 6) >= end) break;
            const int32_t slot = (sub << 6) + int32_t(lane), my_idx = base + slot;
            const bool valid = my_idx < end;
            const int32_t my_g = s_g[buf][slot];
            bool hit = valid;
            if (cull_enabled) {
                const float4 a = s_a[buf][slot], b = s_b[buf][slot];
                hit = valid && cell_reachable(a.x - 0.5f, a.y - 0.5f, a.z, a.w, b.x, rx0, ry0, b.y * 1.001f + 1e-3f);
            }
            const uint64_t m = __ballot(hit);
            if (hit) {
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi(uint32_t(m >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m), 0u));
                out[count + int32_t(rank)] = make_int2(my_g, my_idx);
            }
            count += __popcll(m);
        }
    }
    if (lane == 0) cell_count[cell] = count;
}

// (Frag / frag_eval - one primitive against one pixel - and WPT live in lfs_fastgs.cuh: fastgs_contrib.hip evaluates the same alphas)
// fwd / bwd: ONE wavefront per workgroup (the cells of a tile never cooperate here; a finished cell frees its slot at once - as raster.hip's wave_geom)
// DEPTH (lfs_fastgs_view_render with a depth plane): one more accumulator D += r2.w T alpha over exactly the instances the colour takes, stored to depth_map [1,H,W]; r2.w arrives with
// the record. The default form does not read r2.w or depth_map.
template <bool DEPTH>
__global__ void __launch_bounds__(64) fg_blend_fwd_kernel(
    const uint32_t gw, const uint32_t gh, const uint32_t width, const uint32_t height,
    const GaussRec* __restrict__ recs, const int32_t* __restrict__ offsets, const int32_t* __restrict__ cell_count, const int2* __restrict__ cell_list,
    float* __restrict__ image, float* __restrict__ alpha_map, int32_t* __restrict__ n_contrib, float* __restrict__ depth_map) {
    const uint32_t total_tiles = gw * gh;
    const CellCtx cc = cell_ctx(total_tiles, total_tiles, gw, TILE, WPT, 1);
    if (!cc.in_grid) return;
    const bool inside = cc.i < height && cc.j < width;
    const float px = float(cc.j) + 0.5f, py = float(cc.i) + 0.5f;
    const int32_t start = offsets[cc.tile_global], end = offsets[cc.tile_global + 1];
    const int2* __restrict__ cl = cell_list + (size_t(WPT) * size_t(start) + size_t(cc.wl) * size_t(end - start));
    const int32_t cnt = cell_count[size_t(cc.tile_global) * WPT + cc.wl];
    const float INF = __builtin_inff();
    float thr = inside ? MIN_ALPHA : INF; // "done" is carried as the alpha threshold (see raster.hip)
    float T = 1.f, c0 = 0.f, c1 = 0.f, c2 = 0.f, dsum = 0.f;
    int32_t last = 0; // 1 + global list index of the last blended instance (0: none)
    auto eval = [&](const GaussRec& rec, const int2 e) {
        const Frag f = frag_eval(rec, px, py);
        const bool pass = f.ok && !(f.alpha < thr);
        if (__ballot(pass) == 0ull) return;
        const float next_T = T * (1.f - f.alpha);
        const bool fin = pass && next_T < T_THRESHOLD; // kernels_forward.cuh:432-436: terminates without blending
        const bool contrib = pass && !fin;
        const float w = T * f.alpha;
        if (contrib) {
            c0 = __builtin_fmaf(rec.r2.x, w, c0); c1 = __builtin_fmaf(rec.r2.y, w, c1); c2 = __builtin_fmaf(rec.r2.z, w, c2);
            if constexpr (DEPTH) dsum = __builtin_fmaf(rec.r2.w, w, dsum);
            T = next_T; last = e.y + 1;
        }
        thr = fin ? INF : thr;
    };
    walk_cell_list<1>(cl, recs, 0, cnt, eval, [&]() { return __ballot(thr < INF) != 0ull; });
    if (inside) {
        const size_t np = size_t(width) * height, p = size_t(cc.i) * width + cc.j;
        image[p] = c0; image[np + p] = c1; image[2 * np + p] = c2;
        alpha_map[p] = 1.f - T;
        n_contrib[p] = last;
        if constexpr (DEPTH) depth_map[p] = dsum;
    }
}

// ACC 0: the rows are summed with float atomics, whose arrival order - and so the last bits of every gradient - differs from run to run. ACC 1 / 2: the two passes of
// the deterministic mode (lfs_set_debug_flags bit 4, as the 3DGUT backward's: wave_sum16_atomic in lfs_raster_common.cuh), fg_det_resolve_kernel turns the sums back into floats.
// DEPTH (lfs_fastgs_view_backward with grad_depth): depth is a fourth blended channel - cv = c . g_image + r2.w g_depth feeds dL/dalpha and the colour-behind recurrence - and slot 9
// of the row takes sum w g_depth = dL/dd; the reduction carries ten values instead of nine (wave_sum9_atomic_lds<ACC, 10>), through the same block and atomic.
// ABS (a backward with densification_info on a workspace filled with LFS_FASTGS_ABSGRAD; AbsGS, Ye et al. 2024): slots 10 / 11 of the row take sum |k gx_p|, sum |k gy_p| over the
// same instances, (gx_p, gy_p) = conic . (hx, hy) this pixel's share of dL/dmean2d and k = 0.5 log2(e) the scale the record's conic carries (fg_densify_abs_kernel applies 1 / k):
// twelve values through the same block and atomic (wave_sum9_atomic_lds<ACC, 12>); without DEPTH the value for slot 9 is a zero. Slots 0 .. 9 are computed exactly as in the
// default form. The kernels below the body are its ABS = false / true wrappers under separate names: the default forms keep their names and registers.
#define LFS_FG_BLEND_BWD_PARAMS \
    const uint32_t gw, const uint32_t gh, const uint32_t width, const uint32_t height, \
    const GaussRec* __restrict__ recs, const int32_t* __restrict__ offsets, const int32_t* __restrict__ cell_count, const int2* __restrict__ cell_list, \
    const float* __restrict__ alpha_map, const int32_t* __restrict__ n_contrib, const float* __restrict__ g_image, const float* __restrict__ g_alpha, \
    float* __restrict__ acc, unsigned long long* __restrict__ det64, const float* __restrict__ g_depth
#define LFS_FG_BLEND_BWD_ARGS gw, gh, width, height, recs, offsets, cell_count, cell_list, alpha_map, n_contrib, g_image, g_alpha, acc, det64, g_depth
template <int ACC, bool DEPTH, bool ABS>
LFS_DI void blend_bwd_body(LFS_FG_BLEND_BWD_PARAMS) {
    const uint32_t total_tiles = gw * gh;
    constexpr int NV = ABS ? 12 : DEPTH ? 10 : 9;
    __shared__ __attribute__((aligned(16))) float s_red[red_n_scratch_floats(NV)]; // this wavefront's transpose block (wave_sum9_atomic_lds)
    float* const red_scratch = s_red;
    const CellCtx cc = cell_ctx(total_tiles, total_tiles, gw, TILE, WPT, 1);
    if (!cc.in_grid) return;
    const uint32_t lane = threadIdx.x & 63;
    const bool inside = cc.i < height && cc.j < width;
    const float px = float(cc.j) + 0.5f, py = float(cc.i) + 0.5f;
    const int32_t start = offsets[cc.tile_global], end = offsets[cc.tile_global + 1];
    const int2* __restrict__ cl = cell_list + (size_t(WPT) * size_t(start) + size_t(cc.wl) * size_t(end - start));
    const int32_t cnt = cell_count[size_t(cc.tile_global) * WPT + cc.wl];
    float T = 1.f, gc0 = 0.f, gc1 = 0.f, gc2 = 0.f, gd = 0.f, tail = 0.f, Bsum = 0.f;
    int32_t last = -1;
    if (inside) {
        const size_t np = size_t(width) * height, p = size_t(cc.i) * width + cc.j;
        T = 1.f - alpha_map[p];
        last = n_contrib[p] - 1;
        gc0 = g_image[p]; gc1 = g_image[np + p]; gc2 = g_image[2 * np + p];
        if constexpr (DEPTH) gd = g_depth[p];
        tail = g_alpha[p] * T; // grad_alpha * (1 - alpha_pixel), kernels_backward.cuh:352
    }
    int32_t wmax = last;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) wmax = max(wmax, __shfl_xor(wmax, m, 64));
    wmax = __builtin_amdgcn_readfirstlane(wmax);
    int32_t lo = 0, hi = cnt;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (cl[mid].y <= wmax) lo = mid + 1; else hi = mid;
    }
    if (lo <= 0) return;
    auto eval = [&](const GaussRec& rec, const int2 e) {
        const Frag f = frag_eval(rec, px, py);
        const bool valid = e.y <= last && f.ok && !(f.alpha < MIN_ALPHA);
        if (__ballot(valid) == 0ull) return;
        const float ra = fast_rcp(1.f - f.alpha);
        const float Tn = T * ra;                                  // transmittance in front of this instance
        T = valid ? Tn : T;
        const float w = valid ? Tn * f.alpha : 0.f;               // blending weight (0 masks every sum below)
        float cv = __builtin_fmaf(rec.r2.z, gc2, __builtin_fmaf(rec.r2.y, gc1, rec.r2.x * gc0));
        if constexpr (DEPTH) cv = __builtin_fmaf(rec.r2.w, gd, cv);
        // dL/dalpha = (T c - colour_behind / (1 - alpha)) . g + grad_alpha (1 - alpha_pixel) / (1 - alpha)   (kernels_backward.cuh:412-417)
        const float dl_dalpha = __builtin_fmaf(ra, tail - Bsum, Tn * cv);
        Bsum = __builtin_fmaf(w, cv, Bsum);
        const float aD = valid ? f.alpha * dl_dalpha : 0.f;      // (no clamp mask on alpha, as in the reference)
        const float hx = -aD * f.dx, hy = -aD * f.dy;
        // accumulator row: {sum hx, sum hy, sum hx dx, sum hx dy | sum hy dy, dc.r, dc.g, dc.b | sum alpha dL/dalpha}
        //   dL/dmean2d = conic . (sum hx, sum hy), dL/dconic = 0.5 (sum hx dx, sum hx dy, sum hy dy)   (fastgs_prep.hip); depth form: | sum w g_depth}
        float* row = acc + size_t(e.x) * ACC_STRIDE;
        if constexpr (ABS) {
            // |k gx_p| = |aD| |kA dx + kB dy|, |k gy_p| = |aD| |kB dx + kC dy| (kB = r0.w / 2): aD = 0 masks both like every other sum
            const float hb = 0.5f * rec.r0.w;
            const float mx = __builtin_fmaf(rec.r0.z, f.dx, hb * f.dy), my = __builtin_fmaf(rec.r1.x, f.dy, hb * f.dx);
            const float v[12] = {hx, hy, hx * f.dx, hx * f.dy, hy * f.dy, w * gc0, w * gc1, w * gc2, aD, DEPTH ? w * gd : 0.f, fabsf(aD) * fabsf(mx), fabsf(aD) * fabsf(my)};
            wave_sum9_atomic_lds<ACC, 12>(v, row, lane, red_scratch, ACC == 2 ? det64 + size_t(e.x) * ACC_STRIDE : nullptr);
        } else if constexpr (DEPTH) {
            const float v[10] = {hx, hy, hx * f.dx, hx * f.dy, hy * f.dy, w * gc0, w * gc1, w * gc2, aD, w * gd};
            wave_sum9_atomic_lds<ACC, 10>(v, row, lane, red_scratch, ACC == 2 ? det64 + size_t(e.x) * ACC_STRIDE : nullptr);
        } else {
            const float v[9] = {hx, hy, hx * f.dx, hx * f.dy, hy * f.dy, w * gc0, w * gc1, w * gc2, aD};
            wave_sum9_atomic_lds<ACC>(v, row, lane, red_scratch, ACC == 2 ? det64 + size_t(e.x) * ACC_STRIDE : nullptr);
        }
    };
    walk_cell_list<-1>(cl, recs, lo - 1, lo, eval, []() { return true; });
}
template <int ACC, bool DEPTH>
__global__ void __launch_bounds__(64) fg_blend_bwd_kernel(LFS_FG_BLEND_BWD_PARAMS) { blend_bwd_body<ACC, DEPTH, false>(LFS_FG_BLEND_BWD_ARGS); }
template <int ACC, bool DEPTH>
__global__ void __launch_bounds__(64) fg_blend_bwd_abs_kernel(LFS_FG_BLEND_BWD_PARAMS) { blend_bwd_body<ACC, DEPTH, true>(LFS_FG_BLEND_BWD_ARGS); }
#undef LFS_FG_BLEND_BWD_PARAMS
#undef LFS_FG_BLEND_BWD_ARGS

// deterministic mode, after pass 2: acc[i] = fixed-point sum * 2^(e - 40), e from the pass-1 maximum that acc[i] still holds as bits (the slots no form writes hold 0 and stay 0)
__global__ void __launch_bounds__(256) fg_det_resolve_kernel(const size_t n, float* __restrict__ acc, const unsigned long long* __restrict__ det64) {
    const size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t mbits = reinterpret_cast<const uint32_t*>(acc)[i];
    float out = 0.f;
    if (mbits != 0u) {
        const int e = max(int((mbits >> 23) & 0xffu), 1) - 127;
        out = float(ldexp(double((long long)det64[i]), e - 40)); // exact scaling; one rounding to float
    }
    acc[i] = out;
}

static uint32_t g_fastgs_debug = 0;

} // namespace fgs
} // namespace lfs

using namespace lfs;

extern "C" void lfs_fastgs_set_debug_flags(uint32_t flags) { fgs::g_fastgs_debug = flags; }

static_assert(sizeof(lfs_fastgs_sh_rest_adam) == 48 && sizeof(lfs_fastgs_view_backward_args) == 144, "the ctypes mirrors (capi.py) are laid out by hand");

// Whether the workspace carries d in its records is validated on the HOST (the flags the library remembers by the workspace's address: no device read, no launch on
// a refusal); the antialiased bit is picked on the device.
extern "C" int lfs_fastgs_view_render(const lfs_fastgs_view* view, int64_t n_instances, void* instance_workspace, size_t instance_workspace_bytes,
                                      float* image, float* alpha, float* depth, lfs_stream_t stream) {
    if (!view) return LFS_E_INVALID;
    const uint32_t N = view->N, width = view->width, height = view->height;
    void* const primitive_workspace = view->primitive_workspace;
    if (depth && (!primitive_workspace || fgs::ws_mode(fgs::remembered_flags(primitive_workspace)).depth == 0)) return LFS_E_INVALID;
    if (!primitive_workspace || !image || !alpha || width == 0 || height == 0 || n_instances < 0 || n_instances > 0x7FFFFFFFll) return LFS_E_INVALID;
    if (N >= (1u << 26) || uint64_t(n_instances) >= (1ull << 29)) return LFS_E_UNSUPPORTED; // 32-bit byte offsets of the record walker
    fgs::PrimWs w = fgs::prim_ws(primitive_workspace, N, width, height);
    if (view->primitive_workspace_bytes < w.bytes) return LFS_E_WORKSPACE;
    fgs::InstWs iw = fgs::inst_ws(instance_workspace, width, height, uint64_t(n_instances));
    if (!instance_workspace || instance_workspace_bytes < iw.bytes) return LFS_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const fgs::Frame f = fgs::make_frame(*view);   // (the kernels of this stage read the image and grid extents only)
    const uint32_t T = f.gw * f.gh;
    if (n_instances > 0) {
        int rc = fgs::launch_scatter(N, f, w, iw.keys, s);
        if (rc) return rc;
        static bool big_lds_enabled = false;
        if (!big_lds_enabled) {
            hipError_t ae = hipFuncSetAttribute(reinterpret_cast<const void*>(&tile_sort_lds_kernel<1024>), hipFuncAttributeMaxDynamicSharedMemorySize, 16384 * 8);
            if (ae != hipSuccess) return (int)ae;
            ae = hipFuncSetAttribute(reinterpret_cast<const void*>(&tile_sort_bins_kernel<256>), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * 4096 * 8);
            if (ae != hipSuccess) return (int)ae;
            big_lds_enabled = true;
        }
        lfs::ProfScope prof_sort("fastgs_tile_sort", s);
        hipLaunchKernelGGL(tile_sort_bins_kernel<256>, dim3(T), dim3(256), 2 * 1024 * 8, s, 1u, 1024u, T, 0u, w.offsets, iw.keys, iw.ids, iw.keys);
        hipLaunchKernelGGL((tile_sort_bins_kernel<512, 512, false, 32>), dim3(T), dim3(512), 4096 * 8, s, 1025u, 4096u, T, 0u, w.offsets, iw.keys, iw.ids, iw.keys); // (as intersect.hip)
        hipLaunchKernelGGL(tile_sort_lds_kernel<1024>, dim3(T), dim3(1024), 16384 * 8, s, 4097u, 16384u, T, 0u, w.offsets, iw.keys, iw.ids, iw.keys);
        hipLaunchKernelGGL(tile_sort_global_kernel, dim3(T), dim3(1024), 0, s, 16385u, T, 0u, w.offsets, iw.keys, iw.ids);
    }
    const uint32_t grid = cell_grid_blocks(T, 1);
    {
        lfs::ProfScope prof("fastgs_cull", s);
        hipLaunchKernelGGL(fgs::fg_cull_kernel, dim3(grid), dim3(256), 0, s, f.gw, f.gh, width, height, (fgs::g_fastgs_debug & 1u) ? 0u : 1u,
                           w.rec, w.offsets, iw.ids, iw.cell_count, iw.cell_list);
    }
    lfs::ProfScope prof("fastgs_blend_fwd", s);
    const uint32_t wgrid = cell_grid_blocks(uint64_t(T) * fgs::WPT, fgs::WPT);
    if (depth) hipLaunchKernelGGL(fgs::fg_blend_fwd_kernel<true>, dim3(wgrid), dim3(64), 0, s, f.gw, f.gh, width, height, w.rec, w.offsets, iw.cell_count, iw.cell_list,
                                  image, alpha, w.n_contrib, depth);
    else hipLaunchKernelGGL(fgs::fg_blend_fwd_kernel<false>, dim3(wgrid), dim3(64), 0, s, f.gw, f.gh, width, height, w.rec, w.offsets, iw.cell_count, iw.cell_list,
                            image, alpha, w.n_contrib, static_cast<float*>(nullptr));
    return (int)hipGetLastError();
}

extern "C" size_t lfs_fastgs_w2c_workspace_bytes(uint32_t N) { return fgs::w2c_workspace_bytes(N); }

// filter_var (lfs_fastgs_view_ext::filter3d_var) must agree with what the library remembers for the workspace - filled with the 3D filter or not - in both directions:
// LFS_E_INVALID before any launch otherwise (a backward of the wrong form would differentiate a function the forward did not render).
static int view_backward(const lfs_fastgs_view* view, const lfs_fastgs_view_backward_args* args, const float* filter_var, lfs_stream_t stream);
extern "C" int lfs_fastgs_view_backward(const lfs_fastgs_view* view, const lfs_fastgs_view_backward_args* args, lfs_stream_t stream) {
    return view_backward(view, args, nullptr, stream);
}
extern "C" int lfs_fastgs_view_backward_ex(const lfs_fastgs_view* view, const lfs_fastgs_view_backward_args* args, const lfs_fastgs_view_ext* ext, lfs_stream_t stream) {
    return view_backward(view, args, ext ? ext->filter3d_var : nullptr, stream);
}
static int view_backward(const lfs_fastgs_view* view, const lfs_fastgs_view_backward_args* args, const float* filter_var, lfs_stream_t stream) {
    if (!view || !args) return LFS_E_INVALID;
    const lfs_fastgs_view& v = *view;
    const lfs_fastgs_view_backward_args& a = *args;
    const uint32_t N = v.N;
    // what the workspace was filled with, looked up once; below it becomes what this call runs. (No workspace: all zero - such a view is refused further down.)
    fgs::WsMode mode = fgs::ws_mode(v.primitive_workspace ? fgs::remembered_flags(v.primitive_workspace) : 0u);
    if (v.primitive_workspace && mode.filter3d != (filter_var != nullptr)) return LFS_E_INVALID;
    // the optimizer-fused form: the parameter it updates replaces the view's sh_coefficients_rest; it has no camera gradient and no depth gradient
    const float* sh_rest = v.sh_coefficients_rest;
    lfs::ShAdamArgs adam_args{};
    const lfs::ShAdamArgs* adam = nullptr;
    if (a.adam) {
        if (v.total_bases_sh_rest == 0 || !a.adam->exp_avg || !a.adam->exp_avg_sq) return LFS_E_INVALID;
        if (a.grad_w2c || a.grad_depth) return LFS_E_INVALID;
        adam_args = lfs::ShAdamArgs{a.adam->exp_avg, a.adam->exp_avg_sq, a.adam->lr, a.adam->beta1, a.adam->beta2, a.adam->eps, a.adam->bias_correction1_rcp,
                                    a.adam->bias_correction2_sqrt_rcp};
        adam = &adam_args;
        sh_rest = a.adam->sh_coefficients_rest;
    }
    // the abs form (LFS_FASTGS_ABSGRAD): only where its two sums have a reader; without densification_info the call launches what a default workspace's does
    mode.absgrad = mode.absgrad && a.densification_info != nullptr;
    if (!a.grad_depth) mode.depth = 0;   // with grad_depth: the workspace's depth kind, which it must have
    else if (mode.depth == 0) return LFS_E_INVALID;
    if (a.grad_w2c) {
        if (!a.w2c_workspace || a.w2c_workspace_bytes < fgs::w2c_workspace_bytes(N)) return LFS_E_WORKSPACE;
        if (reinterpret_cast<uintptr_t>(a.w2c_workspace) % 16 != 0) return LFS_E_INVALID;   // fg_w2c_reduce_kernel reads the partial rows as float4
    } else if (a.w2c_workspace || a.w2c_workspace_bytes != 0) return LFS_E_INVALID;
    if (!v.primitive_workspace || !v.w2c || !v.cam_position || !a.grad_image || !a.grad_alpha || !a.alpha || v.width == 0 || v.height == 0 || a.n_instances < 0)
        return LFS_E_INVALID;
#ifdef LFS_EMULATE
    const bool det = false;   // (the emulated library has no integer-atomic passes)
#else
    const bool det = (lfs_get_debug_flags() & 16u) != 0;   // the workspace then carries the int64 rows: it was sized with the bit set, or it is refused here
#endif
    fgs::PrimWs w = fgs::prim_ws(v.primitive_workspace, N, v.width, v.height, det);
    if (v.primitive_workspace_bytes < w.bytes) return LFS_E_WORKSPACE;
    fgs::InstWs iw = fgs::inst_ws(a.instance_workspace, v.width, v.height, uint64_t(a.n_instances));
    if (!a.instance_workspace || a.instance_workspace_bytes < iw.bytes) return LFS_E_WORKSPACE;
    if (N == 0) return a.grad_w2c ? fgs::launch_w2c_reduce(0, static_cast<const float*>(a.w2c_workspace), a.grad_w2c, (hipStream_t)stream) : LFS_OK;   // (grad_w2c is fully written: zeros)
    if (!v.means || !v.scales_raw || !v.rotations_raw || !a.grad_means || !a.grad_scales_raw || !a.grad_rotations_raw || !a.grad_opacities_raw || !a.grad_sh_coefficients_0 ||
        (v.total_bases_sh_rest > 0 && (!sh_rest || (!a.grad_sh_coefficients_rest && !adam)))) return LFS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const fgs::Frame f = fgs::make_frame(v);
    // debug bit 1: the accumulator rows of the previous backward on this workspace are kept (no blending backward). Its float atomics arrive in a different order on
    // every run; with the rows held fixed, the per-primitive stage of two calls can be compared bit for bit (tests/test_gpu_fastgs_w2c.py)
    // TEST-ONLY: with the bit left set every gradient is computed from stale rows. The optimizer-fused form (adam != nullptr) ignores it.
    const bool keep_acc = (fgs::g_fastgs_debug & 2u) != 0 && adam == nullptr;
    if (!keep_acc) {
        hipError_t e = hipMemsetAsync(w.acc, 0, sizeof(float) * ACC_STRIDE * size_t(N), s);
        if (e != hipSuccess) return (int)e;
    }
    const uint32_t T = f.gw * f.gh;
    if (a.n_instances > 0 && !keep_acc) {
        lfs::ProfScope prof("fastgs_blend_bwd", s);
        const uint32_t wgrid = cell_grid_blocks(uint64_t(T) * fgs::WPT, fgs::WPT);
#define LFS_FG_BWD_PAIR(ACC, DEPTH) {&fgs::fg_blend_bwd_abs_kernel<ACC, DEPTH>, &fgs::fg_blend_bwd_kernel<ACC, DEPTH>}
        static constexpr decltype(&fgs::fg_blend_bwd_kernel<0, false>) kernels[3][2][2] = {   // [ACC 1, 2, 0][without grad_depth][default form]: the code object's order
            {LFS_FG_BWD_PAIR(1, true), LFS_FG_BWD_PAIR(1, false)}, {LFS_FG_BWD_PAIR(2, true), LFS_FG_BWD_PAIR(2, false)}, {LFS_FG_BWD_PAIR(0, true), LFS_FG_BWD_PAIR(0, false)}};
#undef LFS_FG_BWD_PAIR
        const auto blend_bwd = [&](int acc) {
            hipLaunchKernelGGL(kernels[acc == 0 ? 2 : acc - 1][mode.depth == 0][!mode.absgrad], dim3(wgrid), dim3(64), 0, s, f.gw, f.gh, v.width, v.height, w.rec, w.offsets,
                               iw.cell_count, iw.cell_list, a.alpha, w.n_contrib, a.grad_image, a.grad_alpha, w.acc, w.det64, a.grad_depth);
        };
        if (det) { // pass 1: per-slot maxima of |total| (integer atomicMax), pass 2: 64-bit fixed-point sums, then back to float
            const size_t n_acc = ACC_STRIDE * size_t(N);
            hipError_t e = hipMemsetAsync(w.det64, 0, sizeof(unsigned long long) * n_acc, s);
            if (e != hipSuccess) return (int)e;
            blend_bwd(1); blend_bwd(2);
            hipLaunchKernelGGL(fgs::fg_det_resolve_kernel, dim3(uint32_t((n_acc + 255) / 256)), dim3(256), 0, s, n_acc, w.acc, w.det64);
        } else blend_bwd(0);
    }
    return fgs::launch_preprocess_bwd(v, f, w, a, sh_rest, adam, mode, filter_var, s);
}
