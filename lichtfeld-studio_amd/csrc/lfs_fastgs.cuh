// Workspace layout and constants shared by fastgs_prep.hip and fastgs_blend.hip (the EWA "fastgs" rasterizer,
// SURVEY.md §8f row 1; reference: fastgs/rasterization/*).
#pragma once
#include "lfs_raster_common.cuh"
#include "../../include/lfs_gsplat.h"

namespace lfs {
// sh.hip: the SH kernels with strided colour operands (colours live inside the 64-B blend records / accumulator rows)
int sh_records_fwd(uint32_t n, uint32_t K, uint32_t degree, const float* means, const float* campos, const float* sh0, const float* shN,
                   const uint32_t* mask_u32, float* colors, uint32_t colors_stride, hipStream_t s);
// adam != NULL (single-view steps): v_shN is not written, shN and its moments are updated in place by the same kernel (sh_bwd_kernel<.., ADAM>)
struct ShAdamArgs { float* exp_avg; float* exp_avg_sq; float lr, beta1, beta2, eps, bc1_rcp, bc2_sqrt_rcp; };
int sh_records_bwd(uint32_t n, uint32_t K, uint32_t degree, const float* means, const float* campos, const float* sh0, const float* shN,
                   const uint32_t* mask_u32, const float* colors, uint32_t colors_stride, const float* v_colors, uint32_t v_stride,
                   float* v_sh0, float* v_shN, float* v_means, hipStream_t s, const ShAdamArgs* adam = nullptr);
namespace fgs {

// fastgs/rasterization/include/rasterization_config.h:14-33
constexpr float DILATION = 0.3f;
constexpr float MIN_ALPHA_RCP = 255.0f;
constexpr float MIN_ALPHA = 1.0f / 255.0f;
constexpr float MAX_ALPHA = 0.999f;
constexpr float T_THRESHOLD = 1e-4f;
constexpr uint32_t TILE = 16;
constexpr float LOG2E = 1.4426950408889634f;
constexpr uint32_t MODE_ANTIALIASED = 1u; // PrimWs::mode bit 0 (= LFS_FASTGS_ANTIALIASED of lfs_fastgs_view_preprocess)
constexpr uint32_t MODE_DEPTH = 4u;       // bit 2 (= LFS_FASTGS_DEPTH): r2.w of every visible record = camera-space z
constexpr uint32_t MODE_INVDEPTH = 8u;    // bit 3 (= LFS_FASTGS_INVDEPTH): r2.w = 1 / z
constexpr uint32_t MODE_ABSGRAD = 32u;    // bit 5 (= LFS_FASTGS_ABSGRAD): a backward with densification_info runs the abs form of the blend backward + fg_densify_abs_kernel
constexpr uint32_t MODE_FILTER3D = 1u << 16; // internal (no public flag): filled by a preprocess with the 3D smoothing filter (lfs_fastgs_view_ext::filter3d_var);
                                              // the opacity of the records is sigmoid(raw) * kappa [* rho] and r1.w = sigmoid(raw), as in the antialiased mode
// the DEPTH template parameter of the per-primitive kernels: 0 none, 1 z, 2 1 / z
constexpr uint32_t depth_mode_bits(int depth) { return depth == 1 ? MODE_DEPTH : depth == 2 ? MODE_INVDEPTH : 0u; }

struct Frame { // one camera; w2c / cam_position stay device pointers (torch tensors of the caller)
    const float* w2c; const float* cam_pos;
    uint32_t active_sh_bases, total_rest, width, height, gw, gh;
    float fx, fy, cx, cy, near_, far_;
};

inline size_t align256(size_t v) { return (v + 255) & ~size_t(255); }

// Per-primitive + per-tile + per-pixel state: written by the forward, read by the backward.
//   rec[N]   64-B blend record: r0 = {mean2d.x, mean2d.y, A, B}, r1 = {C, thr', opacity, -}, r2 = {max(colour, 0), -},
//            r3 unused; with (A, B, C) = log2(e) * (conic.x / 2, conic.y, conic.z / 2) and thr' = log2(e) *
//            log(255 * opacity): sigma' = A dx^2 + B dx dy + C dy^2 is the Gaussian exponent in bits (one v_exp_f32).
//            Antialiased mode: opacity = sigmoid(raw) * rho everywhere, and r1.w = sigmoid(raw) for the backward.
//            Depth modes: r2.w = d = z or 1 / z (camera space), blended by the depth forms of the blend kernels like a fourth colour channel.
//   mode     one word of the (otherwise spare) 256-byte n_instances slot: the flags of the preprocess that filled the workspace. The per-primitive backward
//            picks its antialiased or default instantiation by it on the device, so render and backward carry no flag. The depth, 3D filter and absgrad bits are ALSO
//            remembered on the host, by the workspace's address (fastgs_prep.hip: remember_flags; WsMode below): a depth plane or a depth gradient on a workspace
//            without the depth bits is refused before any launch, and the depth, filtered and abs forms of the kernels are chosen on the host from that table; they
//            check their bit in this word again.
struct PrimWs {
    GaussRec* rec; float2* mean2d; float4* conic_opacity; ushort4* bounds; uint32_t* n_touched; uint32_t* depth_bits;
    uint32_t* totals; uint32_t* cursor; int32_t* offsets; int64_t* n_instances; uint32_t* mode; int32_t* n_contrib; float* acc; unsigned long long* det64; size_t bytes;
};
// det (lfs_set_debug_flags bit 4, the deterministic backward): one int64 accumulator row per primitive behind everything else, so the other pointers do not move.
// The size query and the backward ask for it; preprocess and render neither need nor check it.
inline PrimWs prim_ws(void* base, uint32_t N, uint32_t width, uint32_t height, bool det = false) {
    const size_t T = size_t((width + TILE - 1) / TILE) * ((height + TILE - 1) / TILE), P = size_t(width) * height;
    PrimWs w; char* p = (char*)base; size_t o = 0;
    w.rec = (GaussRec*)(p + o); o += align256(sizeof(GaussRec) * N);
    w.mean2d = (float2*)(p + o); o += align256(sizeof(float2) * N);
    w.conic_opacity = (float4*)(p + o); o += align256(sizeof(float4) * N);
    w.bounds = (ushort4*)(p + o); o += align256(sizeof(ushort4) * N);
    w.n_touched = (uint32_t*)(p + o); o += align256(4 * size_t(N));
    w.depth_bits = (uint32_t*)(p + o); o += align256(4 * size_t(N));
    w.totals = (uint32_t*)(p + o); o += align256(4 * T);
    w.cursor = (uint32_t*)(p + o); o += align256(4 * T);
    w.offsets = (int32_t*)(p + o); o += align256(4 * (T + 1));
    w.n_instances = (int64_t*)(p + o); w.mode = (uint32_t*)(p + o) + 2; o += 256;
    w.n_contrib = (int32_t*)(p + o); o += align256(4 * P);
    w.acc = (float*)(p + o); o += align256(sizeof(float) * ACC_STRIDE * N);
    w.det64 = nullptr;
    if (det) { w.det64 = (unsigned long long*)(p + o); o += align256(sizeof(unsigned long long) * ACC_STRIDE * size_t(N)); }
    w.bytes = o;
    return w;
}
// Per-instance state: keys (depth bits << 32 | primitive) -> sorted ids, and the compacted per-8x8-cell lists.
struct InstWs { int64_t* keys; int32_t* ids; int32_t* cell_count; int2* cell_list; size_t bytes; };
inline InstWs inst_ws(void* base, uint32_t width, uint32_t height, uint64_t n_instances) {
    const size_t T = size_t((width + TILE - 1) / TILE) * ((height + TILE - 1) / TILE);
    InstWs w; char* p = (char*)base; size_t o = 0;
    w.keys = (int64_t*)(p + o); o += align256(8 * n_instances);
    w.ids = (int32_t*)(p + o); o += align256(4 * n_instances);
    w.cell_count = (int32_t*)(p + o); o += align256(4 * 4 * T);
    w.cell_list = (int2*)(p + o); o += align256(8 * 4 * n_instances);
    w.bytes = o;
    return w;
}

// accumulator row of the blend backward (16 floats per primitive, one 64-B line):
//   0,1 sum h (dx, dy) | 2,3,4 sum h (dx dx, dx dy, dy dy), h = -alpha dL/dalpha | 5,6,7 dL/d(clamped colour) | 8 sum alpha dL/dalpha |
//   9 dL/dd = sum w g_depth (depth form of the backward only; 0 otherwise) | 10,11 sum |k gx_p|, sum |k gy_p| (abs form only; 0 otherwise) | 12..15 unused

// The per-pixel evaluation shared by the blend kernels (fastgs_blend.hip) and the contribution statistic (fastgs_contrib.hip): one definition, the same alpha bits.
constexpr uint32_t WPT = 4; // 8x8 cells per 16x16 tile
struct Frag { float dx, dy, alpha; bool ok; };
// one primitive against this lane's pixel: sigma' = A dx^2 + B dx dy + C dy^2 (bits), alpha = min(opacity 2^-sigma', 0.999)
LFS_DI Frag frag_eval(const GaussRec& rec, const float px, const float py) {
    Frag f;
    f.dx = rec.r0.x - px; f.dy = rec.r0.y - py;
    const float u = __builtin_fmaf(rec.r0.w, f.dy, rec.r0.z * f.dx);
    const float s = __builtin_fmaf(rec.r1.x * f.dy, f.dy, f.dx * u);
    f.alpha = fminf(rec.r1.z * __builtin_amdgcn_exp2f(-s), MAX_ALPHA);
    f.ok = !(s < 0.f); // kernels_forward.cuh:425-426
    return f;
}

// What the host remembers of the preprocess that last filled a primitive workspace (fastgs_prep.hip: remember_flags), as render and the backward use it: ONE lookup per
// call, so every form a call picks comes from the same state of the table. All zero: a default (or antialiased-only) workspace, or one the table no longer holds.
uint32_t remembered_flags(const void* primitive_workspace);
struct WsMode { int depth; bool filter3d, absgrad; };   // depth: 0 none, 1 z, 2 1 / z (the DEPTH template parameter of the per-primitive kernels)
inline WsMode ws_mode(uint32_t remembered) {
    return WsMode{(remembered & MODE_DEPTH) ? 1 : (remembered & MODE_INVDEPTH) ? 2 : 0, (remembered & MODE_FILTER3D) != 0u, (remembered & MODE_ABSGRAD) != 0u};
}

// host-side launchers of fastgs_prep.hip that fastgs_blend.hip uses as well
int launch_scatter(uint32_t N, const Frame& f, const PrimWs& w, int64_t* keys, hipStream_t s);
Frame make_frame(const lfs_fastgs_view& v);
// sh_rest / adam: the view's coefficients and no optimizer, or the optimizer-fused form's parameter. mode: the forms this backward runs - depth with grad_depth only,
// absgrad with densification_info only, filter3d with filter_var (the [N] variances) only
int launch_preprocess_bwd(const lfs_fastgs_view& v, const Frame& f, const PrimWs& w, const lfs_fastgs_view_backward_args& a, const float* sh_rest, const ShAdamArgs* adam,
                          const WsMode& mode, const float* filter_var, hipStream_t s);
size_t w2c_workspace_bytes(uint32_t N);
int launch_w2c_reduce(uint32_t N, const float* w2c_partials, float* grad_w2c, hipStream_t s);
} // namespace fgs
} // namespace lfs
