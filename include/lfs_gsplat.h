/* lfs_gsplat.h — C ABI of the MI355X-native (gfx950) 3DGS training rasterizer.
 *
 * Drop-in boundary for the reference's native operator backend
 * (MrNeRF/LichtFeld-Studio): every entry point below replaces one function of
 * /root/reference/gsplat/Ops.h (namespace gsplat::) or of
 * /root/reference/fastgs/optimizer/include/adam.h, with the at::Tensor
 * arguments flattened to raw DEVICE pointers + sizes + a hipStream_t.
 * The libtorch wrappers that restore the exact Ops.h signatures live in
 * include/lfs_gsplat_torch.hpp + lichtfeld-studio_amd/csrc/torch_ops.cpp.
 *
 * Conventions (same as the reference):
 *   - all pointers are device pointers, contiguous, fp32 unless noted;
 *   - quaternions are (w,x,y,z) and need not be normalised;
 *   - viewmats are row-major world->camera [C,4,4]; Ks row-major [C,3,3];
 *   - scales / opacities are the ACTIVATED values (exp / sigmoid applied);
 *   - every function enqueues on `stream` and returns without synchronising;
 *   - return value: 0 on success, a hipError_t (>0) from the runtime, or a
 *     negative LFS_E_* code for argument errors. Nothing is launched on error.
 *   - "workspace" buffers are caller-owned scratch (size from the matching
 *     *_workspace_bytes function, 256-byte aligned); contents are undefined
 *     afterwards unless stated.
 */
#ifndef LFS_GSPLAT_H
#define LFS_GSPLAT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LFS_API __attribute__((visibility("default")))

typedef void* lfs_stream_t; /* hipStream_t */

enum { LFS_OK = 0, LFS_E_INVALID = -1, LFS_E_UNSUPPORTED = -2, LFS_E_WORKSPACE = -3 };

/* gsplat/Common.h:46-50 */
enum { LFS_CAMERA_PINHOLE = 0, LFS_CAMERA_ORTHO = 1, LFS_CAMERA_FISHEYE = 2 };
/* gsplat/Cameras.h:16-22 */
enum {
    LFS_SHUTTER_ROLLING_TOP_TO_BOTTOM = 0,
    LFS_SHUTTER_ROLLING_LEFT_TO_RIGHT = 1,
    LFS_SHUTTER_ROLLING_BOTTOM_TO_TOP = 2,
    LFS_SHUTTER_ROLLING_RIGHT_TO_LEFT = 3,
    LFS_SHUTTER_GLOBAL = 4
};

/* gsplat/Cameras.h:27-61 UnscentedTransformParameters */
typedef struct lfs_ut_params {
    float alpha;                       /* 0.1 */
    float beta;                        /* 2   */
    float kappa;                       /* 0   */
    float in_image_margin_factor;      /* 0.1 */
    int32_t require_all_sigma_points_valid; /* 1 */
} lfs_ut_params;

/* The camera block every projection / rasterization entry point of Ops.h
 * takes (viewmats0, viewmats1, Ks, camera_model, rs_type, radial/tangential/
 * thin-prism coefficients, image size). n_radial / n_thin_prism say how many
 * coefficients per camera the tensors really hold (missing ones are 0; the
 * reference reads 6 / 4 unconditionally). */
typedef struct lfs_cameras {
    uint32_t C;
    uint32_t image_width, image_height;
    int32_t camera_model;              /* LFS_CAMERA_* */
    int32_t rs_type;                   /* LFS_SHUTTER_* */
    const float* viewmats0;            /* [C,4,4] */
    const float* viewmats1;            /* [C,4,4] or NULL */
    const float* Ks;                   /* [C,3,3] */
    const float* radial_coeffs;        /* [C,n_radial] or NULL */
    int32_t n_radial;
    const float* tangential_coeffs;    /* [C,2] or NULL */
    const float* thin_prism_coeffs;    /* [C,n_thin_prism] or NULL */
    int32_t n_thin_prism;
} lfs_cameras;

/* ---- gsplat::projection_ut_3dgs_fused  (gsplat/Ops.h:66-90, Projection.cpp:22-110,
 *      ProjectionUT3DGSFused.cu:17-203). radii int32 [C,N,2]; means2d [C,N,2];
 *      depths [C,N]; conics [C,N,3]; compensations [C,N] or NULL. Entries of culled
 *      Gaussians: radii = 0, the other outputs are written as 0 (the reference leaves
 *      them uninitialised). opacities [N] may be NULL. */
LFS_API int lfs_projection_ut_3dgs_fused(
    uint32_t N, const float* means, const float* quats, const float* scales, const float* opacities,
    const lfs_cameras* cams, float eps2d, float near_plane, float far_plane, float radius_clip,
    const lfs_ut_params* ut_params,
    int32_t* radii, float* means2d, float* depths, float* conics, float* compensations,
    lfs_stream_t stream);

/* ---- gsplat::spherical_harmonics_fwd / _bwd (gsplat/Ops.h:12-25, SphericalHarmonics.cpp:15-76,
 *      SphericalHarmonicsCUDA.cu). n = number of directions, coeffs [n,K,3], masks bool[n] or NULL.
 *      fwd: colors [n,3]; masked-out rows are written as 0.
 *      bwd: v_coeffs [n,K,3] is FULLY written (zeros where masked / unused bases: no pre-zeroing
 *      needed); v_dirs [n,3] or NULL, fully written. */
LFS_API int lfs_spherical_harmonics_fwd(
    uint32_t n, uint32_t K, uint32_t degrees_to_use, const float* dirs, const float* coeffs, const uint8_t* masks,
    float* colors, lfs_stream_t stream);
LFS_API int lfs_spherical_harmonics_bwd(
    uint32_t n, uint32_t K, uint32_t degrees_to_use, const float* dirs, const float* coeffs, const uint8_t* masks,
    const float* v_colors, float* v_coeffs, float* v_dirs, lfs_stream_t stream);

/* ---- gsplat::intersect_tile (gsplat/Ops.h:27-38, Intersect.cpp:15-122, IntersectTile.cu).
 *      Two calls with one host read of *n_isects in between (the reference syncs at the same
 *      place, Intersect.cpp:76). Non-packed layout only: means2d [C,N,2], radii int32 [C,N,2],
 *      depths [C,N].
 *   1) lfs_intersect_tile_count: tiles_per_gauss int32 [C,N]; *n_isects (device int64).
 *   2) lfs_intersect_tile_emit : isect_ids int64 [n_isects], flatten_ids int32 [n_isects];
 *      sort != 0 -> ordered exactly as a stable ascending sort of isect_ids
 *      (key = cam << (32+tile_n_bits) | tile << 32 | depth bits). tile_offsets (optional,
 *      int32 [C*tile_h*tile_w], may be NULL) receives what lfs_intersect_offset would compute,
 *      for free, when sort != 0. The SAME workspace must be passed to both calls. */
LFS_API size_t lfs_intersect_tile_workspace_bytes(uint32_t C, uint32_t N, uint32_t tile_width, uint32_t tile_height);
LFS_API int lfs_intersect_tile_count(
    uint32_t C, uint32_t N, const float* means2d, const int32_t* radii,
    uint32_t tile_size, uint32_t tile_width, uint32_t tile_height,
    int32_t* tiles_per_gauss, int64_t* n_isects, void* workspace, size_t workspace_bytes, lfs_stream_t stream);
LFS_API int lfs_intersect_tile_emit(
    uint32_t C, uint32_t N, const float* means2d, const int32_t* radii, const float* depths,
    uint32_t tile_size, uint32_t tile_width, uint32_t tile_height, int sort, int64_t n_isects,
    const int32_t* tiles_per_gauss, int64_t* isect_ids, int32_t* flatten_ids, int32_t* tile_offsets,
    void* workspace, size_t workspace_bytes, lfs_stream_t stream);

/*      Extended forms (what the fused training step and the libtorch wrapper call; same results):
 *      _count_ex: tile_offsets (nullable, int32 [C*tile_h*tile_w]) is written by the scan kernel instead of a device copy in _emit;
 *                 flags & LFS_ISECT_COUNTERS_ZERO: the workspace is the one of the caller's previous _count_ex call with the same C, N and tile
 *                 grid (the kernels leave its counters zero) - skips the memset. n_isects and max_tile_isects (nullable: the longest tile list) may
 *                 point to pinned host memory (written by the kernel); stamp_out (nullable) then receives `stamp` LAST, behind a system-scope fence: the
 *                 host waits for the completion event and then for its own stamp before it trusts the counts.
 *      _emit_ex : scratch (nullable, int64 [n_isects]): with it the scatter runs as two binning passes with coalesced stores
 *                 (C*tile_h <= 512 and bits(C*N) + bits(tile_w) <= 32; otherwise, or without it, the one-pass scatter). max_tile_isects: the value
 *                 _count_ex reported (the per-tile sort then launches only the size classes that occur), or -1. */
#define LFS_ISECT_COUNTERS_ZERO 1u
LFS_API int lfs_intersect_tile_count_ex(
    uint32_t C, uint32_t N, const float* means2d, const int32_t* radii,
    uint32_t tile_size, uint32_t tile_width, uint32_t tile_height,
    int32_t* tiles_per_gauss, int64_t* n_isects, int64_t* max_tile_isects, int32_t* tile_offsets, uint32_t flags, int64_t* stamp_out, int64_t stamp,
    void* workspace, size_t workspace_bytes, lfs_stream_t stream);
LFS_API int lfs_intersect_tile_emit_ex(
    uint32_t C, uint32_t N, const float* means2d, const int32_t* radii, const float* depths,
    uint32_t tile_size, uint32_t tile_width, uint32_t tile_height, int sort, int64_t n_isects,
    const int32_t* tiles_per_gauss, int64_t* isect_ids, int32_t* flatten_ids, int32_t* tile_offsets, int64_t* scratch, int64_t max_tile_isects,
    void* workspace, size_t workspace_bytes, lfs_stream_t stream);

/* ---- gsplat::intersect_offset (gsplat/Ops.h:39-43, IntersectTile.cu:206-286).
 *      offsets int32 [C,tile_h,tile_w] from SORTED isect_ids. */
LFS_API int lfs_intersect_offset(
    int64_t n_isects, const int64_t* isect_ids, uint32_t C, uint32_t tile_width, uint32_t tile_height,
    int32_t* offsets, lfs_stream_t stream);

/* ---- gsplat::rasterize_to_pixels_from_world_3dgs_fwd / _bwd (gsplat/Ops.h:92-166,
 *      Rasterization.cpp, RasterizeToPixelsFromWorld3DGS{Fwd,Bwd}.cu). channels in 1..4.
 *      colors [C,N,channels], opacities [C,N], backgrounds [C,channels] or NULL,
 *      masks bool [C,tile_h,tile_w] or NULL, tile_offsets int32 [C,tile_h,tile_w],
 *      flatten_ids int32 [n_isects] (values in [0, C*N)).
 *      fwd: render_colors [C,H,W,channels], render_alphas [C,H,W,1], last_ids int32 [C,H,W].
 *      bwd: v_means [N,3], v_quats [N,4], v_scales [N,3], v_colors [C,N,channels],
 *           v_opacities [C,N] — all FULLY written (no pre-zeroing needed). v_render_alphas may be NULL (= zeros). */
/*      workspace: camera state + one 64-B record, one 64-B gradient accumulator row and one 32-B culling
 *      record per (camera, Gaussian) + the compacted per-8x8-cell lists ((tile_size/8)^2 * n_isects * 8 B,
 *      worst case). Returns 0 for an unsupported tile_size. */
LFS_API size_t lfs_rasterize_workspace_bytes(uint32_t C, uint32_t N, uint32_t channels, uint32_t image_width,
                                             uint32_t image_height, uint32_t tile_size, int64_t n_isects);
/*      developer switch, not part of the reference API: bit 0 = build the per-cell lists without culling (fwd output must be bit-identical either way;
 *      tests/test_gpu_raster.py); bits 1 - 3: unused (the experimental kernels they selected were measured and removed);
 *      bit 4 = deterministic backward accumulation (two passes, 64-bit fixed point: run-to-run bit-identical gradients; lfs_rasterize_workspace_bytes and
 *      lfs_fastgs_primitive_workspace_bytes grow while it is set, and both backwards refuse a workspace sized without it);
 *      bit 5 = the one-pass intersection scatter even when a scratch array is given; bit 6 = the training step packs the rasterizer's records with the separate
 *      raster_pack pass of rounds 1 - 3 instead of inside the projection kernel (A/B, tests/test_emulated_step_pack.py); bit 7: unused (round 6: the projection kernel clearing the
 *      backward's accumulator rows instead of the memset - measured slower, removed). */
LFS_API void lfs_set_debug_flags(uint32_t flags);
LFS_API uint32_t lfs_get_debug_flags(void);
LFS_API int lfs_rasterize_to_pixels_from_world_3dgs_fwd(
    uint32_t N, uint32_t channels, const float* means, const float* quats, const float* scales,
    const float* colors, const float* opacities, const float* backgrounds, const uint8_t* masks,
    const lfs_cameras* cams, uint32_t tile_size, const lfs_ut_params* ut_params,
    const int32_t* tile_offsets, const int32_t* flatten_ids, int64_t n_isects,
    float* render_colors, float* render_alphas, int32_t* last_ids,
    void* workspace, size_t workspace_bytes, lfs_stream_t stream);
LFS_API int lfs_rasterize_to_pixels_from_world_3dgs_bwd(
    uint32_t N, uint32_t channels, const float* means, const float* quats, const float* scales,
    const float* colors, const float* opacities, const float* backgrounds, const uint8_t* masks,
    const lfs_cameras* cams, uint32_t tile_size, const lfs_ut_params* ut_params,
    const int32_t* tile_offsets, const int32_t* flatten_ids, int64_t n_isects,
    const float* render_alphas, const int32_t* last_ids,
    const float* v_render_colors, const float* v_render_alphas,
    float* v_means, float* v_quats, float* v_scales, float* v_colors, float* v_opacities,
    void* workspace, size_t workspace_bytes, lfs_stream_t stream);

/*      extension (not in Ops.h): the same backward, for a caller that still owns the workspace the matching
 *      forward call filled (same inputs, nothing else ran on that workspace in between): skips rebuilding
 *      the records and the per-cell lists. Used by the autograd Function of rasterizer.py. */
LFS_API int lfs_rasterize_to_pixels_from_world_3dgs_bwd_prepared(
    uint32_t N, uint32_t channels, const float* means, const float* quats, const float* scales,
    const float* colors, const float* opacities, const float* backgrounds, const uint8_t* masks,
    const lfs_cameras* cams, uint32_t tile_size, const lfs_ut_params* ut_params,
    const int32_t* tile_offsets, const int32_t* flatten_ids, int64_t n_isects,
    const float* render_alphas, const int32_t* last_ids,
    const float* v_render_colors, const float* v_render_alphas,
    float* v_means, float* v_quats, float* v_scales, float* v_colors, float* v_opacities,
    void* workspace, size_t workspace_bytes, lfs_stream_t stream);
/* ... with the clamped MSE of lfs_mse_loss_fwd_bwd folded into the kernel's prologue (extension: one camera, 3 channels, no masks):
 * dL/d(render) is derived from render_colors [H,W,3] and target_chw [3,H,W] in registers and never stored; *loss += weight * mse. */
LFS_API int lfs_rasterize_to_pixels_from_world_3dgs_bwd_prepared_mse(
    uint32_t N, const float* means, const float* quats, const float* scales, const float* colors, const float* opacities,
    const float* backgrounds, const lfs_cameras* cams, uint32_t tile_size, const int32_t* tile_offsets, const int32_t* flatten_ids,
    int64_t n_isects, const float* render_colors, const float* render_alphas, const int32_t* last_ids, const float* target_chw, float weight,
    float* loss, float* v_means, float* v_quats, float* v_scales, float* v_colors, float* v_opacities, void* workspace, size_t workspace_bytes,
    lfs_stream_t stream);

/* ---- Fused L2 extensions (not in Ops.h; lichtfeld-studio_amd/fused.py, trainer.py): the libtorch element-wise
 *      work rasterizer.cpp:200-263 / splat_data.cpp:267-286 / the trainer's loss wrap around the operators,
 *      as single passes. Same arithmetic as the op-by-op path (tests/test_gpu_fused.py).
 *   lfs_sh_model_fwd : colors [N,3] = clamp_min(SH(normalize(means - campos(viewmat)), cat(sh0, shN)) + 0.5, 0)
 *                      with mask = all(radii > 0); viewmat = ONE rigid row-major [4,4] on the device.
 *   lfs_sh_model_bwd : v_colors = dL/dcolors (the clamp is applied inside from `colors`); v_sh0 [N,1,3], v_shN [N,K-1,3]
 *                      written (accumulate = 0) or added to (accumulate != 0); v_means [N,3] += dL/d(dirs).
 *   lfs_activations_fwd / _bwd : quats = normalize(raw), scales = exp(raw), opacities = sigmoid(raw) and the vjp.
 *   lfs_mse_loss_fwd_bwd : *loss += weight * mean((clamp(render,0,1) - target)^2), v_render = d/d(render);
 *                      render / v_render HWC [H,W,3], target CHW [3,H,W]. */
LFS_API int lfs_sh_model_fwd(
    uint32_t n, uint32_t K, uint32_t degrees_to_use, const float* means, const float* viewmat, const float* sh0, const float* shN,
    const int32_t* radii, float* colors, lfs_stream_t stream);
LFS_API int lfs_sh_model_bwd(
    uint32_t n, uint32_t K, uint32_t degrees_to_use, const float* means, const float* viewmat, const float* sh0, const float* shN,
    const int32_t* radii, const float* colors, const float* v_colors, int accumulate,
    float* v_sh0, float* v_shN, float* v_means, lfs_stream_t stream);
/* lfs_sh_model_bwd for a step with ONE view, fused with the optimizer: the gradient of shN is not stored but consumed by the
 * Adam update (fast_gs::optimizer::adam_step arithmetic, adam_kernels.cuh:13-36) of shN / its moments in place; v_sh0 written,
 * v_means += dL/d(dirs) computed from the pre-update shN. Element-wise identical to lfs_sh_model_bwd + lfs_adam_step on shN. */
LFS_API int lfs_sh_model_bwd_adam(
    uint32_t n, uint32_t K, uint32_t degrees_to_use, const float* means, const float* viewmat, const float* sh0, float* shN,
    const int32_t* radii, const float* colors, const float* v_colors, float* v_sh0, float* v_means,
    float* shN_exp_avg, float* shN_exp_avg_sq, float lr, float beta1, float beta2, float eps, float bias_correction1_rcp,
    float bias_correction2_sqrt_rcp, lfs_stream_t stream);
/* Multi-view forms for SH-sharded data parallelism (the owner of n Gaussians evaluates the views of all ranks in ONE launch; coefficient
 * rows are read once for all views): viewmats [V,4,4]; radii [V,view_stride,2], colors / v_colors [V,view_stride,3] with the first n rows of
 * every view used. Backward: the coefficient gradient is summed over the views, then written / added (accumulate) to v_sh0, v_shN, or -
 * shN_exp_avg != NULL, accumulate == 0 - consumed by shN's Adam update as in lfs_sh_model_bwd_adam; v_means += sum over views of dL/d(dirs). */
LFS_API int lfs_sh_model_fwd_views(
    uint32_t n, uint32_t K, uint32_t degrees_to_use, uint32_t n_views, uint32_t view_stride, const float* means, const float* viewmats,
    const float* sh0, const float* shN, const int32_t* radii, float* colors, lfs_stream_t stream);
LFS_API int lfs_sh_model_bwd_views(
    uint32_t n, uint32_t K, uint32_t degrees_to_use, uint32_t n_views, uint32_t view_stride, const float* means, const float* viewmats,
    const float* sh0, float* shN, const int32_t* radii, const float* colors, const float* v_colors, int accumulate,
    float* v_sh0, float* v_shN, float* v_means, float* shN_exp_avg, float* shN_exp_avg_sq, float lr, float beta1, float beta2, float eps,
    float bias_correction1_rcp, float bias_correction2_sqrt_rcp, lfs_stream_t stream);
LFS_API int lfs_activations_fwd(uint32_t N, const float* raw_quats, const float* raw_scales, const float* raw_opacities,
                                float* quats, float* scales, float* opacities, lfs_stream_t stream);
LFS_API int lfs_activations_bwd(uint32_t N, const float* raw_quats, const float* scales, const float* opacities,
                                const float* v_quats, const float* v_scales, const float* v_opacities,
                                float scale_reg, float opacity_reg, /* + d/d(activated) of scale_reg * mean(scales) + opacity_reg * mean(opacities), trainer.cpp:132-158 */
                                int accumulate,
                                float* g_raw_quats, float* g_raw_scales, float* g_raw_opacities, lfs_stream_t stream);
LFS_API int lfs_mse_loss_fwd_bwd(uint32_t H, uint32_t W, const float* render_hwc, const float* target_chw, float weight,
                                 float* v_render_hwc, float* loss, lfs_stream_t stream);
/*      the same for a CHW render that is NOT clamped (the fastgs path, fast_rasterizer.cpp:62-66) */
LFS_API int lfs_mse_loss_chw_fwd_bwd(uint32_t H, uint32_t W, const float* render_chw, const float* target_chw, float weight,
                                     float* v_render_chw, float* loss, lfs_stream_t stream);

/* ---- "next" row 1 of SURVEY.md §8f: the reference's default training rasterizer (fastgs, EWA splatting).
 *      Replaces fast_gs::rasterization::forward_wrapper / backward_wrapper (fastgs/rasterization/include/rasterization_api.h:27-75,
 *      src/rasterization_api.cu, forward.cu, backward.cu, kernels_{forward,backward}.cuh). Inputs are the RAW parameters
 *      (log-scales, un-normalised quaternions wxyz, opacity logits, sh0 [N,1,3], sh_rest [N,total_bases_sh_rest,3]); w2c is a
 *      row-major [4,4] (rows 0-2 used) and cam_position [3], both on the device. image [3,H,W], alpha [1,H,W] (CHW, no background).
 *      The reference's four opaque buffer tensors become two caller-owned workspaces that must survive until the backward.
 *      One entry point per stage, each on the same lfs_fastgs_view (the scene's raw parameters, one camera, the primitive workspace);
 *      every optional output or operand is a field that may be NULL:
 *        1) lfs_fastgs_view_preprocess : per-primitive stage + per-tile counts; *n_instances (device int64) = list length
 *        2) (host reads n_instances: the reference syncs at the same place, forward.cu:114-117)
 *        3) lfs_fastgs_view_render     : instance lists (scatter + per-tile depth sort), per-cell culling, blending
 *        4) lfs_fastgs_view_backward   : blending backward + per-primitive backward; gradients FULLY written */
LFS_API size_t lfs_fastgs_primitive_workspace_bytes(uint32_t N, uint32_t width, uint32_t height);
LFS_API size_t lfs_fastgs_instance_workspace_bytes(uint32_t width, uint32_t height, int64_t n_instances);
typedef struct lfs_fastgs_view {
    uint32_t N;
    const float *means, *scales_raw, *rotations_raw;
    const float* opacities_raw;             /* read by the preprocess only */
    const float* sh_coefficients_0;         /* the backward takes NULL (the reference's backward does not take it either) */
    const float* sh_coefficients_rest;      /* NULL when total_bases_sh_rest == 0 */
    uint32_t total_bases_sh_rest;
    const float *w2c, *cam_position;
    uint32_t active_sh_bases, width, height;
    float fx, fy, cx, cy, near_plane, far_plane;
    void* primitive_workspace;              /* lfs_fastgs_primitive_workspace_bytes(N, width, height) */
    size_t primitive_workspace_bytes;
} lfs_fastgs_view;
/* flags of lfs_fastgs_view_preprocess. A bit that is not defined here: LFS_E_INVALID before any launch.
 * LFS_FASTGS_ANTIALIASED (the reference's OptimizationParameters::antialiasing, which it connects to nothing): with (a0, b, c0) the projected covariance before the
 * 0.3 px^2 dilation and (a, b, c) after it, rho = sqrt(max(0, (a0 c0 - b^2) / (a c - b^2))) (add_blur, gsplat/Utils.cuh:171-179) and the opacity of the primitive is
 * sigmoid(raw) * rho wherever the default mode uses sigmoid(raw): the 1/255 cut (after the cuts on sigmoid(raw), the quaternion and a c - b^2), the power threshold,
 * the extents, the tile tests, the blend. The mode is recorded in the primitive workspace, rewritten by every preprocess with N > 0: render and backward take the
 * same arguments in both modes, and the backward is the full derivative (through rho into means, scales, rotations and grad_w2c). */
#define LFS_FASTGS_ANTIALIASED 1u
/* Depth modes (the reference's render_mode D / ED / RGB_D / RGB_ED on the EWA path). With z_i the camera-space z of primitive i (>= near_plane when visible):
 * LFS_FASTGS_DEPTH blends d_i = z_i, LFS_FASTGS_INVDEPTH d_i = 1 / z_i. The two exclude each other (both: LFS_E_INVALID), each combines with LFS_FASTGS_ANTIALIASED.
 * The preprocess writes d_i into a free word of the blend record and the flag into the workspace's mode word; the workspace size does not change, and a render
 * without a depth plane and a backward without grad_depth treat such a workspace as an ordinary one. (Bit 1, value 2, stays undefined.)
 * The library remembers, by address and without a device read, the workspaces filled in a depth mode: up to 256 whose backward is still to come (a preprocess
 * without a depth flag takes no entry and only clears its own address); with more outstanding, the least recently filled one is forgotten and from then on
 * counts as a default-mode workspace. */
#define LFS_FASTGS_DEPTH 4u
#define LFS_FASTGS_INVDEPTH 8u
/* Absolute screen-space gradients for densification (AbsGS, Ye et al. 2024; gsplat's absgrad). Combines with every flag above and with the 3D filter operand, and
 * changes nothing in the preprocess, the render, the records, the workspace sizes or any gradient. A backward on a workspace filled with it, with densification_info
 * != NULL, adds for every primitive i with n_touched != 0
 *     densification_info[0][i] += 1,   densification_info[1][i] += sqrt((0.5 W Gx_i)^2 + (0.5 H Gy_i)^2),
 * Gx_i = sum_p |gx_p|, Gy_i = sum_p |gy_p| over the pixels p the backward blends i into, (gx_p, gy_p) = conic_i . (hx, hy) that pixel's share of dL/dmean2d_i -
 * the default mode's expression with the per-pixel absolute values summed instead of the signed ones, which cancel on a large Gaussian over fine texture.
 * With densification_info == NULL the backward launches what it launches on a default workspace. Remembered with the workspace like the depth flags (the same 256
 * entries). (Bit 4, value 16, stays undefined.) */
#define LFS_FASTGS_ABSGRAD 32u
LFS_API int lfs_fastgs_view_preprocess(const lfs_fastgs_view* view, uint32_t flags, int64_t* n_instances /* device */, lfs_stream_t stream);
/* n_instances of this process's last lfs_fastgs_view_preprocess call, read back asynchronously: blocks until the 8-byte copy (queued before the SH kernel)
 * has landed, not until the stream is idle. Alternative to reading the device value with a stream synchronisation. */
LFS_API int lfs_fastgs_wait_n_instances(int64_t* n_instances);
/* Reads N, width, height and the primitive workspace of the view. depth (NULL, or [1,H,W]) = sum_i w_i d_i over exactly the instances that contribute to the
 * colour (w_i = T_i alpha_i): the ACCUMULATED value, the reference's D / RGB_D; the expected value (ED) is depth / alpha, the caller's business. image and alpha
 * are the same bits with and without it. LFS_E_INVALID, nothing launched: depth given on a workspace that was not last filled by a preprocess with a depth flag in
 * this process (the library's memory of them: above). */
LFS_API int lfs_fastgs_view_render(const lfs_fastgs_view* view, int64_t n_instances, void* instance_workspace, size_t instance_workspace_bytes,
                                   float* image, float* alpha, float* depth, lfs_stream_t stream);
/* Extension for a step with ONE view, the backward fused with the optimizer: sh_coefficients_rest (the parameter itself; the view's pointer is not read) and its
 * Adam moments are updated in place by the SH backward (fast_gs::optimizer::adam_step arithmetic); the [N,total_rest,3] gradient is never stored. */
typedef struct lfs_fastgs_sh_rest_adam {
    float *sh_coefficients_rest, *exp_avg, *exp_avg_sq;
    float lr, beta1, beta2, eps, bias_correction1_rcp, bias_correction2_sqrt_rcp;
} lfs_fastgs_sh_rest_adam;
typedef struct lfs_fastgs_view_backward_args {
    int64_t n_instances;
    void* instance_workspace;
    size_t instance_workspace_bytes;
    const float *grad_image, *grad_alpha, *alpha;
    /* NULL, or the gradient [1,H,W] of lfs_fastgs_view_render's depth plane. Depth is a fourth blended channel of the blending backward (dL/dalpha and the
     * colour-behind recurrence see d_i g_depth next to c_i . g_image), dL/dd_i = sum w g_depth is one more slot of the accumulator row, and dL/dz_i = dL/dd_i
     * (1 | -1 / z_i^2) is added to the camera-space mean gradient: it reaches grad_means and row 2 of grad_w2c. LFS_E_INVALID, nothing launched: given on a workspace
     * the library does not know as a depth-mode one (as the render's depth). */
    const float* grad_depth;
    float* densification_info;              /* NULL, or [2,N] accumulated into: (visibility count, screen-space gradient norm) */
    float *grad_means, *grad_scales_raw, *grad_rotations_raw, *grad_opacities_raw, *grad_sh_coefficients_0;
    float* grad_sh_coefficients_rest;       /* not written when adam is given (may be NULL then, and when total_bases_sh_rest == 0) */
    /* NULL, or the camera gradient of the reference's pose optimisation (rasterization_api.cu:133-136: requested when w2c requires grad): [4,4] row-major, FULLY
     * written whatever N and n_instances are: rows 0-2 = sum over the primitives with n_touched > 0 of dL/d(mean in camera space) (x) (mean, 1)
     * (kernels_backward.cuh:165-183: no term through cam_position, none for the direct dependence of the EWA Jacobian on w2c, none from the SH colours), row 3 = 0.
     * Summed without float atomics, in a fixed order: the same bits on every run for the same dL/d(mean in camera space). w2c_workspace (16-byte aligned,
     * lfs_fastgs_w2c_workspace_bytes(N) bytes) holds one row of partial sums per 256 primitives. With grad_w2c: LFS_E_WORKSPACE for a NULL or short workspace,
     * LFS_E_INVALID for one that is not 16-byte aligned. Without: w2c_workspace must be NULL and its size 0 (LFS_E_INVALID). */
    float* grad_w2c;
    void* w2c_workspace;
    size_t w2c_workspace_bytes;
    /* NULL: the gradient tensors above. Given: LFS_E_INVALID when total_bases_sh_rest == 0 or a pointer of it is NULL, and - before any launch - together with
     * grad_w2c or grad_depth (pose optimisation and depth supervision take the separate optimizer). */
    const lfs_fastgs_sh_rest_adam* adam;
} lfs_fastgs_view_backward_args;
LFS_API size_t lfs_fastgs_w2c_workspace_bytes(uint32_t N);
LFS_API int lfs_fastgs_view_backward(const lfs_fastgs_view* view, const lfs_fastgs_view_backward_args* args, lfs_stream_t stream);
/* ---- The 3D smoothing filter of Mip-Splatting (the other half of LFS_FASTGS_ANTIALIASED, which is its 2D Mip filter). Nothing in the reference provides it.
 *      With v_i >= 0 the filter variance of Gaussian i (lfs_filter3d_compute below), R S^2 R^T + v I = R (S^2 + v I) R^T: the filtered modes of the per-primitive
 *      kernels use s'_ik = sqrt(s_ik^2 + v_i) wherever the default mode uses exp(raw_scale), and o'_i = sigmoid(raw_i) * kappa_i, kappa_i = prod_k s_ik / s'_ik,
 *      wherever it uses sigmoid(raw_i): the 1/255 cut, the EWA projection, rho of the antialiased mode (o_eff = o' rho(s')), the power threshold, the extents, the
 *      tile tests, the records. A filtered render of (raw_scales, raw, v) is the default render of (log s', logit(o')).
 *      Backward, with g'_k the gradient w.r.t. log s'_k, S = o_eff dL/do_eff and u_k = v / (s_k^2 + v):
 *        grad_scales_raw_k = g'_k (1 - u_k) + S u_k,  grad_opacities_raw = S (1 - sigmoid(raw));  everything else is the gradient at the effective parameters.
 *      v itself takes no gradient (it is a statistic of the training cameras, recomputed by the trainer).
 *      The operand arrives through an extension struct on two entries; further per-view operands go into this struct. ext == NULL, or ext->filter3d_var == NULL,
 *      IS the entry without _ex. The public flags are those of lfs_fastgs_view_preprocess. The filtered mode is recorded in the workspace's mode word (an internal
 *      bit) and in the library's by-address memory of workspaces (as the depth modes): lfs_fastgs_view_backward_ex returns LFS_E_INVALID before any launch, nothing
 *      written, when its ext disagrees - in either direction - with what is remembered for the workspace. lfs_fastgs_view_render is the same call in every mode.
 *      args->adam works with the filter. The workspace sizes do not change. */
typedef struct lfs_fastgs_view_ext {
    const float* filter3d_var;              /* [N] (device) or NULL */
} lfs_fastgs_view_ext;
LFS_API int lfs_fastgs_view_preprocess_ex(const lfs_fastgs_view* view, uint32_t flags, const lfs_fastgs_view_ext* ext, int64_t* n_instances /* device */,
                                          lfs_stream_t stream);
LFS_API int lfs_fastgs_view_backward_ex(const lfs_fastgs_view* view, const lfs_fastgs_view_backward_args* args, const lfs_fastgs_view_ext* ext, lfs_stream_t stream);
/* The filter variance. One packed camera: rows 0-2 of the row-major world-to-camera matrix, the pinhole intrinsics in pixels, the image size.
 *   camera c SEES Gaussian i  iff  z_ic > 0.2 and -0.15 W_c <= x <= 1.15 W_c and -0.15 H_c <= y <= 1.15 H_c   ((x, y) the pinhole projection in pixels)
 *   nu_i = max over the cameras that see i of max(fx_c, fy_c) / z_ic;  a Gaussian no camera sees takes the smallest nu among the seen ones;
 *   filter_var[i] = variance_scale / nu_i^2 (Mip-Splatting's variance_scale: 0.2);  no Gaussian seen, or C == 0: every filter_var[i] = 0.
 * cameras: device array of C records. workspace: 4-byte aligned, lfs_filter3d_workspace_bytes() bytes. No host read, no allocation, no float atomics: the same
 * bits on every run. N == 0: LFS_OK, nothing launched. LFS_E_INVALID: NULL means / filter_var, NULL cameras with C > 0, a negative or NaN variance_scale. */
typedef struct lfs_filter3d_camera {
    float w2c[12];
    float fx, fy, cx, cy;
    uint32_t width, height;
} lfs_filter3d_camera;
LFS_API size_t lfs_filter3d_workspace_bytes(void);
LFS_API int lfs_filter3d_compute(uint32_t N, const float* means, uint32_t C, const lfs_filter3d_camera* cameras /* device */, float variance_scale,
                                 float* filter_var, void* workspace, size_t workspace_bytes, lfs_stream_t stream);
LFS_API void lfs_fastgs_set_debug_flags(uint32_t flags); /* bit 0: no per-cell culling (bit-identity test); bit 1: the backward skips the blending
                                                           * backward and reuses the accumulator rows the previous backward left in the primitive workspace (its float
                                                           * atomics round differently from run to run: bit-identity tests of the per-primitive stage hold them fixed).
                                                           * Bit 1 is for tests ONLY and must never be set elsewhere: while it is set, every gradient of
                                                           * lfs_fastgs_view_backward comes from stale accumulator rows. With args->adam, which updates parameters in
                                                           * place, the bit is ignored. */

/* ---- "next" row 2 of SURVEY.md §8f: fused SSIM (fusedssim / fusedssim_backward, include/kernels/ssim.cuh:11-30,
 *      src/training/kernels/ssim.cu:64-510) and the trainer's photometric loss (trainer.cpp:122-125).
 *      img1 / img2 / maps [B,CH,H,W]; 11-tap Gaussian window, zero padding. dm_* may all be NULL (train == false).
 *      lfs_photometric_loss_fwd_bwd (extension): *loss += weight * ((1 - lambda) * L1 + lambda * (1 - mean SSIM over the
 *      "valid" crop)) of clamp(render, 0, 1) against target; render / v_render HWC [H,W,3], target CHW [3,H,W]. */
LFS_API int lfs_fused_ssim_fwd(uint32_t B, uint32_t CH, uint32_t H, uint32_t W, float C1, float C2, const float* img1, const float* img2,
                               float* ssim_map, float* dm_dmu1, float* dm_dsigma1_sq, float* dm_dsigma12, lfs_stream_t stream);
LFS_API int lfs_fused_ssim_bwd(uint32_t B, uint32_t CH, uint32_t H, uint32_t W, float C1, float C2, const float* img1, const float* img2,
                               const float* dL_dmap, const float* dm_dmu1, const float* dm_dsigma1_sq, const float* dm_dsigma12,
                               float* dL_dimg1, lfs_stream_t stream);
LFS_API size_t lfs_photometric_loss_workspace_bytes(uint32_t H, uint32_t W);
LFS_API int lfs_photometric_loss_fwd_bwd(uint32_t H, uint32_t W, const float* render_hwc, const float* target_chw, float lambda_dssim,
                                         float weight, float* v_render_hwc, float* loss, void* workspace, size_t workspace_bytes,
                                         lfs_stream_t stream);
/* ... and for a CHW render [3,H,W] (the fastgs rasterizer's image layout), which is NOT clamped (fast_rasterizer.cpp:63 hands
 * the image to the loss as is); v_render_chw [3,H,W] */
LFS_API int lfs_photometric_loss_chw_fwd_bwd(uint32_t H, uint32_t W, const float* render_chw, const float* target_chw, float lambda_dssim,
                                             float weight, float* v_render_chw, float* loss, void* workspace, size_t workspace_bytes,
                                             lfs_stream_t stream);

/* general forms of the two losses: render / v_render in either layout (render_is_chw), clamped on the way in or not (an image that went through the
 * bilateral grid reaches the loss un-clamped, trainer.cpp:662-676) */
LFS_API int lfs_photometric_loss_ex_fwd_bwd(uint32_t H, uint32_t W, const float* render, uint32_t render_is_chw, uint32_t clamp_render, const float* target_chw,
                                            float lambda_dssim, float weight, float* v_render, float* loss, void* workspace, size_t workspace_bytes,
                                            lfs_stream_t stream);
LFS_API int lfs_mse_loss_ex_fwd_bwd(uint32_t H, uint32_t W, const float* render, uint32_t render_is_chw, uint32_t clamp_render, const float* target_chw, float weight,
                                    float* v_render, float* loss, lfs_stream_t stream);

/* masked forms (extension; DESIGN.md §8 "Masked training"). mask_u8 [H,W]: 255 = the pixel counts fully, 0 = ignored; mask_sums int64[2] on the device =
 * {S_img = sum of the mask, S_crop = sum over the SSIM crop (5 pixels per side when H, W > 10, else the image)}, as lfs_mask_prepare writes them. The kernels read
 * the sums on the device (no host read):
 *   L1m   = sum_c sum_p M_p |r - t| / (3 S_img)                     (0 when S_img == 0)
 *   SSIMm = sum_c sum_{p in crop} M_p ssim_{c,p} / (3 S_crop)        (the SSIM map is that of the UNMASKED images)
 *   *loss += weight * ((1 - lambda) L1m + lambda (1 - SSIMm))       (the SSIM term is 0 when S_crop == 0)
 * and, when alpha [H,W] is given (with v_alpha [H,W]; both or neither), the opacity penalty outside the mask:
 *   *loss += weight * alpha_weight * sum_p (255 - M_p) alpha_p / (255 H W),   v_alpha_p = weight * alpha_weight * (255 - M_p) / (255 H W).
 * Workspace: lfs_photometric_loss_workspace_bytes. The MSE form: *loss += weight * sum_c sum_p M_p (r - t)^2 / (3 S_img). */
LFS_API int lfs_photometric_loss_masked_fwd_bwd(uint32_t H, uint32_t W, const float* render, uint32_t render_is_chw, uint32_t clamp_render, const float* target_chw,
                                                const uint8_t* mask_u8, const int64_t* mask_sums, float lambda_dssim, float weight, const float* alpha,
                                                float alpha_weight, float* v_alpha, float* v_render, float* loss, void* workspace, size_t workspace_bytes,
                                                lfs_stream_t stream);
LFS_API int lfs_mse_loss_masked_fwd_bwd(uint32_t H, uint32_t W, const float* render, uint32_t render_is_chw, uint32_t clamp_render, const float* target_chw,
                                        const uint8_t* mask_u8, const int64_t* mask_sums, float weight, float* v_render, float* loss, lfs_stream_t stream);

/* depth supervision (extension). lfs_depth_prepare: target_in [H,W] (any float; valid = finite and > 0) -> target_out [H,W] = the value where valid,
 * NaN where not (target_out may be target_in: the plane is prepared in place), and sums int64[1] on the device = sum_p valid_p M_p with M_p the mask byte (255 without a mask): 255 x the sum of the weights
 * m_p = valid_p M_p / 255, exact. lfs_depth_l1_loss_fwd_bwd on a prepared target (weights_u8 the same mask or NULL):
 *   *loss_acc += weight * sum_p m_p |D_p - t_p| / max(sum m, 1),   grad_depth_p = weight * m_p * sign(D_p - t_p) / max(sum m, 1)   (0 where m_p = 0; sign(0) = 0)
 * with the normaliser read from sums on the device (no host read). */
LFS_API int lfs_depth_prepare(uint32_t H, uint32_t W, const float* target_in, const uint8_t* weights_u8, float* target_out, int64_t* sums, lfs_stream_t stream);
LFS_API int lfs_depth_l1_loss_fwd_bwd(uint32_t H, uint32_t W, const float* depth, const float* target, const uint8_t* weights_u8, const int64_t* sums, float weight,
                                      float* grad_depth, float* loss_acc, lfs_stream_t stream);

/* ---- bilateral-grid appearance model (row 2 of §8f, BASELINE config 5): gs::bilateral_grid::slice_forward_cuda /
 *      slice_backward_cuda / tv_loss_forward_cuda / tv_loss_backward_cuda (include/kernels/bilateral_grid.cuh:12-33,
 *      src/training/kernels/bilateral_grid_{forward,backward,tv}.cu). grid [12,L,H,W]; image h x w (both >= 2), uniform
 *      x/y coordinates, guidance z = luma. Extensions: chw != 0 reads / writes the image planes as [3,h,w] instead of
 *      [h,w,3]; clamp_input != 0 folds BilateralGrid::apply's clamp(rgb, 0, 1) (components/bilateral_grid.cpp:115) into
 *      both passes. grad_grid is ACCUMULATED into (the reference zero-fills, then atomically adds: zero it for the same
 *      result); grad_rgb is fully written. TV: grids [N,12,L,H,W]; *loss += weight * tv; the backward takes dL/dloss as a
 *      host float (the reference reads it with .item(), bilateral_grid_tv.cu:181). */
LFS_API int lfs_bilateral_slice_fwd(uint32_t L, uint32_t H, uint32_t W, uint32_t h, uint32_t w, const float* grid, const float* rgb,
                                    uint32_t chw, uint32_t clamp_input, float* output, lfs_stream_t stream);
LFS_API int lfs_bilateral_slice_bwd(uint32_t L, uint32_t H, uint32_t W, uint32_t h, uint32_t w, const float* grid, const float* rgb,
                                    const float* grad_output, uint32_t chw, uint32_t clamp_input, float* grad_grid, float* grad_rgb,
                                    lfs_stream_t stream);
/* Pure host, no launch: which kernels lfs_bilateral_slice_fwd / _bwd run for this shape (both take their decision from this function).
 *   out[0] forward path: 0 generic (grid read from global memory), 1 LDS value window;   out[1] worst-case forward window, in floats
 *   out[2] backward path: 0 generic (global float atomics per pixel), 1 windowed (MFMA); out[3] dynamic LDS the windowed kernel would need, in bytes
 *   out[4] bound on the windowed backward's 16-column tiles: ceil(x-extent of a 64-pixel strip's window * L / 16)
 * LFS_E_INVALID for exactly the shapes the two launchers refuse. */
LFS_API int lfs_bilateral_slice_plan(uint32_t L, uint32_t H, uint32_t W, uint32_t h, uint32_t w, uint32_t out[5]);
LFS_API int lfs_bilateral_tv_loss_fwd(uint32_t N, uint32_t L, uint32_t H, uint32_t W, const float* grids, float weight, float* loss,
                                      lfs_stream_t stream);
LFS_API int lfs_bilateral_tv_loss_bwd(uint32_t N, uint32_t L, uint32_t H, uint32_t W, const float* grids, float grad_output, uint32_t accumulate,
                                      float* grad_grids, lfs_stream_t stream);

/* ---- data side (row 4 of §8f; the host formats are in lfs_io.h):
 *      lfs_image_u8_to_chw_f32: Camera::load_and_get_image (src/core/camera.cpp:101-140) fused with load_image's downscale
 *      (src/core/image_io.cpp:33-57, OpenImageIO resample(interpolate = true)): src u8 [sh,sw,3] -> dst f32 [3,dh,dw] in [0,1];
 *      when the sizes differ the image is resampled bilinearly and re-quantised to 8 bit first, as the reference's host path does.
 *      lfs_mean_neighbor_distances: compute_mean_neighbor_distances (src/core/splat_data.cpp:64-111), points [N,3] -> out [N], device pointers. The
 *      reference's nanoflann query is (1 + 10)-approximate (SearchParameters(10) sets eps, :97), so its result depends on the kd-tree: the entry copies the
 *      points to the host, builds nanoflann's tree there (single-threaded divideTree, leaf size 10), walks it on the GPU in searchLevel's order and
 *      synchronises the stream before it returns. Bit-identical to the reference's function. LFS_E_UNSUPPORTED if the tree is deeper than 128 levels.
 *      lfs_mean_neighbor_distances_exact (extension): the same quantity from an exact all-pairs search; asynchronous. */
LFS_API int lfs_image_u8_to_chw_f32(const uint8_t* src_hwc, uint32_t src_width, uint32_t src_height, float* dst_chw, uint32_t dst_width,
                                    uint32_t dst_height, lfs_stream_t stream);
/* lfs_mask_prepare (extension): one u8 plane [sh,sw] -> the training-size mask [dh,dw] through the sample positions and the 8-bit re-quantisation of
 * lfs_image_u8_to_chw_f32 (mask and image stay registered), then threshold (threshold >= 0: value >= threshold ? 255 : 0; < 0 keeps soft values), then invert
 * (255 - value). WRITES sums int64[2] = {sum of dst, sum of dst over the loss's crop}: exact integers, identical on every run. Asynchronous. */
LFS_API int lfs_mask_prepare(const uint8_t* src_u8, uint32_t src_width, uint32_t src_height, uint8_t* dst_u8, uint32_t dst_width, uint32_t dst_height,
                             uint32_t invert, int32_t threshold, int64_t* sums, lfs_stream_t stream);
/* ---- undistortion at load (extension). The map of one view: a source image taken through a lens model, and the distortion-free pinhole camera
 *      the training target is resampled to. Pixel centres are at +0.5 on both sides. A destination pixel (x, y) is normalised with the destination intrinsics,
 *      distorted by the model and read from the source at
 *        (sx, sy) = (src_fx * xd + src_cx, src_fy * yd + src_cy).
 *      model LFS_CAMERA_PINHOLE: the OpenCV terms, radial = k1 k2 k3 (numerator) k4 k5 k6 (denominator), tangential p1 p2, thin s1..s4; the model accepts a pixel
 *      when its radial factor is > 0.8. model LFS_CAMERA_FISHEYE: theta = atan(r), r_d = theta (1 + k1 theta^2 + .. + k4 theta^8) with radial[0..3]; the model
 *      accepts a pixel when theta < max_angle (the angle up to which r_d grows; the caller computes it, > 0). A pixel is VALID iff the model accepts it and
 *      0.5 <= sx <= src_width - 0.5 and 0.5 <= sy <= src_height - 0.5: all four bilinear taps are inside the source, nothing is extrapolated. */
typedef struct lfs_undistort_map {
    int32_t model;                       /* LFS_CAMERA_PINHOLE | LFS_CAMERA_FISHEYE */
    uint32_t src_width, src_height;      /* the decoded file */
    uint32_t dst_width, dst_height;      /* the training target */
    float src_fx, src_fy, src_cx, src_cy; /* at the source file's size */
    float radial[6], tangential[2], thin[4];
    float max_angle;                     /* fisheye only */
    float dst_fx, dst_fy, dst_cx, dst_cy;
} lfs_undistort_map;
/* All three: asynchronous, one thread per destination pixel, no host read. LFS_E_INVALID before any launch for a NULL map / source (the mask entry excepted) /
 * destination, a zero size, a size >= 2^30, a model other than the two above, a focal length that is not > 0, a fisheye max_angle that is not > 0.
 *   lfs_image_undistort_u8_to_chw_f32: src u8 [sh,sw,3] -> dst f32 [3,dh,dw] and valid u8 [dh,dw] (255 | 0). One bilinear tap at (sx, sy) with the arithmetic and
 *     the 8-bit re-quantisation of lfs_image_u8_to_chw_f32; an invalid pixel is 0 in all three channels.
 *   lfs_mask_undistort_prepare: lfs_mask_prepare through the same positions: tap, re-quantise, threshold, invert, THEN 0 where the pixel is invalid (an inverted
 *     mask does not count blank pixels). src_u8 NULL = "no mask file": the output is the validity plane itself (255 | 0; threshold and invert do not apply).
 *     WRITES sums int64[2] as lfs_mask_prepare does.
 *   lfs_plane_undistort_nearest_f32: src f32 [sh,sw] -> dst f32 [dh,dw], the texel that contains (sx, sy); NaN where the pixel is invalid. */
LFS_API int lfs_image_undistort_u8_to_chw_f32(const lfs_undistort_map* map, const uint8_t* src_hwc, float* dst_chw, uint8_t* valid_u8, lfs_stream_t stream);
LFS_API int lfs_mask_undistort_prepare(const lfs_undistort_map* map, const uint8_t* src_u8, uint8_t* dst_u8, uint32_t invert, int32_t threshold, int64_t* sums,
                                       lfs_stream_t stream);
LFS_API int lfs_plane_undistort_nearest_f32(const lfs_undistort_map* map, const float* src_f32, float* dst_f32, lfs_stream_t stream);
LFS_API int lfs_mean_neighbor_distances(uint32_t N, const float* points, float* out, lfs_stream_t stream);
LFS_API int lfs_mean_neighbor_distances_exact(uint32_t N, const float* points, float* out, lfs_stream_t stream);

/* ---- gsplat::quats_to_rotmats (gsplat/Ops.h:45-48, QuatToRotmatCUDA.cu:14-39): rotmats [N,3,3] row-major */
LFS_API int lfs_quats_to_rotmats(uint32_t N, const float* quats, float* rotmats, lfs_stream_t stream);

/* ---- gsplat::relocation (gsplat/Ops.h:50-57, RelocationCUDA.cu:12-43): ratios int32 [N], binoms [n_max,n_max] */
LFS_API int lfs_relocation(
    uint32_t N, const float* opacities, const float* scales, const int32_t* ratios, const float* binoms, int32_t n_max,
    float* new_opacities, float* new_scales, lfs_stream_t stream);

/* ---- gsplat::add_noise (gsplat/Ops.h:59-65, RelocationCUDA.cu:88-144): means updated in place */
LFS_API int lfs_add_noise(
    uint32_t N, const float* raw_opacities, const float* raw_scales, const float* raw_quats, const float* noise,
    float* means, float current_lr, lfs_stream_t stream);

/* Extension: the front half of the fused 3DGUT training step (one camera, global shutter, 3 channels).
 *   lfs_activations_project_ut : lfs_activations_fwd + lfs_projection_ut_3dgs_fused in one pass over the raw parameters (normalize / exp / sigmoid, then the
 *       projection on the activated values - the same operations in the same order); quats / scales / opacities receive the activated values. */
LFS_API int lfs_activations_project_ut(
    uint32_t N, const float* means, const float* raw_quats, const float* raw_scales, const float* raw_opacities, const lfs_cameras* cams,
    float eps2d, float near_plane, float far_plane, float radius_clip, const lfs_ut_params* ut_params,
    float* quats, float* scales, float* opacities, int32_t* radii, float* means2d, float* depths, lfs_stream_t stream);

/* ---- The --gut training step as ONE host call (csrc/gut_step.hip; replaces Trainer::train_step -> rasterize() -> the Ops.h sequence of
 *      src/training/trainer.cpp:579-770 / rasterization/rasterizer.cpp:200-344 for one pinhole, global-shutter camera per step, RGB, MSE, fused Adam).
 *      No host read on the critical path: the intersection lists are sized for `capacity` entries and sorted by the size classes that cover
 *      `assumed_longest` entries per tile; the true count stays on the device. When it exceeds either assumption the kernels raise a device flag,
 *      empty all lists and the Adam kernels return without updating anything: the caller learns it from the counts - written to PINNED host memory
 *      host_counts[3] = {n_isects, longest tile list, stamp} early in the step - after it has enqueued everything (lfs_gut_step_wait, lfs_gut_step_fits),
 *      enlarges the workspace and calls again with the same arguments.
 *   lfs_gut_step_args: parameters are updated in place; exp_avg / exp_avg_sq / adam[k] in FusedAdam's group order (fused_adam.cpp:22-95, strategy_utils.cpp:35-40)
 *      means, sh0, shN, raw_scales, raw_quats, raw_opacities; adam[k] = {lr, beta1, beta2, eps, 1/(1-beta1^t), 1/sqrt(1-beta2^t)} (fused_adam.cpp:78-92).
 *      viewmat [4,4], Kmat [3,3], background [3] (nullable), target_chw [3,H,W] on the device; *loss = loss_weight * mse(clamp(render,0,1), target) (stored).
 *   workspace: lfs_gut_step_layout_for(...).bytes; the layout names the byte offsets of what a caller may want to look at afterwards (the render
 *      [H,W,3], alpha [H,W], radii int32 [N,2], ...). tile_offsets has T + 1 entries (the last one is n_isects). After a fused-tail one-call
 *      step (lfs_gut_train_step_ex / _opt) the key form of isect_ids and - K <= 16 - the quats / scales / opacities blocks are not written: the step reads neither.
 *      The split form (lfs_gut_view_forward) and the three-pass lfs_gut_train_step still write them.
 *   lfs_gut_view_forward / lfs_gut_view_backward: the same step split for callers that need GRADIENT TENSORS (data-parallel ranks, several views per step,
 *      losses other than MSE): forward into the workspace, then backward into grads[6] (group order; written or, accumulate != 0, added to). */
typedef struct lfs_gut_step_args {
    uint32_t N, K, sh_degree, image_width, image_height, tile_size;
    float *means, *sh0, *shN, *raw_scales, *raw_quats, *raw_opacities;
    float* exp_avg[6]; float* exp_avg_sq[6];
    float adam[6][6];
    const float* viewmat; const float* Kmat; const float* background; const float* target_chw;
    float loss_weight, scale_reg, opacity_reg;
    float* loss;
} lfs_gut_step_args;
typedef struct lfs_gut_step_layout {
    size_t bytes, render, alpha, last_ids, radii, means2d, depths, colors, quats, scales, opacities, tile_offsets, flatten_ids, isect_ids, counts, abort_flag;
} lfs_gut_step_layout;
LFS_API int lfs_gut_step_layout_for(uint32_t N, uint32_t image_width, uint32_t image_height, uint32_t tile_size, int64_t capacity, lfs_gut_step_layout* out);
LFS_API int lfs_gut_step_fits(int64_t n_isects, int64_t longest, int64_t capacity, int64_t assumed_longest); /* 1: the attempt with these assumptions was valid */
LFS_API int lfs_gut_step_supported(uint32_t N, uint32_t image_width, uint32_t image_height, uint32_t tile_size); /* 0: this shape is outside the speculative step (more than
    512 tile rows, index-bit limit, debug bit 5): lfs_gut_* return LFS_E_UNSUPPORTED - enqueue the operators one by one instead (trainer.py does) */
LFS_API int lfs_gut_train_step(const lfs_gut_step_args* args, int64_t capacity, int64_t assumed_longest, void* workspace, size_t workspace_bytes,
                               int64_t* host_counts /* pinned [3], or NULL: counts stay in the workspace */, int64_t stamp, lfs_stream_t stream);
LFS_API int lfs_gut_view_forward(const lfs_gut_step_args* args, int64_t capacity, int64_t assumed_longest, void* workspace, size_t workspace_bytes,
                                 int64_t* host_counts, int64_t stamp, lfs_stream_t stream);
LFS_API int lfs_gut_view_backward(const lfs_gut_step_args* args, int64_t capacity, const float* v_render /* [H,W,3], used when args->target_chw == NULL */,
                                  float* const* grads /* [6] host */, int accumulate, void* workspace, size_t workspace_bytes, lfs_stream_t stream);
/*   = lfs_gut_view_backward_sh (rasterizer backward + SH backward: grads[1], grads[2] final) then lfs_gut_view_backward_finish (grads[0], grads[3..5]); a
 *   data-parallel caller starts the all-reduce of the SH gradients between the two (dist.GradBucket.all_reduce_early). With args->exp_avg[2] /
 *   exp_avg_sq[2] / adam[2] set (one view per step, accumulate == 0) lfs_gut_view_backward_sh applies shN's Adam update itself, as lfs_sh_model_bwd_adam
 *   does, and grads[2] is neither read nor written: the steps whose loss is not the folded MSE (L1 + D-SSIM, bilateral grid, MCMC) keep the 45-of-59-float
 *   tensor out of the optimizer launch that way. */
LFS_API int lfs_gut_view_backward_sh(const lfs_gut_step_args* args, int64_t capacity, const float* v_render, float* const* grads, int accumulate,
                                     void* workspace, size_t workspace_bytes, lfs_stream_t stream);
LFS_API int lfs_gut_view_backward_finish(const lfs_gut_step_args* args, int64_t capacity, float* const* grads, int accumulate,
                                         void* workspace, size_t workspace_bytes, lfs_stream_t stream);
/*   lfs_gut_view_backward_rows: the view's backward WITHOUT the SH backward - grads[0] (means, no SH direction term), grads[3..5] and dL/dcolour rows [N,3] ->
 *   v_colors_out: the factored gradient exchange of the replicated data-parallel layout (dist.ColorGradExchange) gathers the rows of all ranks and runs
 *   lfs_sh_model_bwd_views over all views on every rank (radii = colors = NULL there: rows pre-masked with colour > 0 by the rank that rendered the view). */
LFS_API int lfs_gut_view_backward_rows(const lfs_gut_step_args* args, int64_t capacity, const float* v_render, float* const* grads /* [6] host */, int accumulate,
                                       float* v_colors_out, void* workspace, size_t workspace_bytes, lfs_stream_t stream);
/*   The _ex forms of the gradient-tensor backwards: riders of the view's finish pass. densification_info [2,N] (device; ADC's statistic, default_strategy.cpp): for every
 *   Gaussian visible in THIS view (both radii > 0) row 0 += 1 and row 1 += s, the screen-equivalent norm of the view's own rasterizer part of dL/dmean,
 *      g_c = Rinv^T v, z = (Rinv^T (mean - origin)).z, s = sqrt((g_c.x z W / (2 fx))^2 + (g_c.y z H / (2 fy))^2)
 *   (what dL/dmean2d * 0.5 * (W, H) is on the EWA route: grad_threshold keeps its meaning; the SH direction term of dL/dmean is not in it). The radii are the
 *   ones lfs_gut_view_forward left in the workspace. ext == NULL or densification_info == NULL: the entry without _ex - the same launches, the same bits (the
 *   old entries are argument adapters of these). lfs_gut_view_backward_sh has no finish pass and no _ex form. */
typedef struct lfs_gut_view_ext {
    float* densification_info;   /* [2,N] device or NULL */
} lfs_gut_view_ext;
LFS_API int lfs_gut_view_backward_ex(const lfs_gut_step_args* args, int64_t capacity, const float* v_render, float* const* grads, int accumulate,
                                     const lfs_gut_view_ext* ext, void* workspace, size_t workspace_bytes, lfs_stream_t stream);
LFS_API int lfs_gut_view_backward_finish_ex(const lfs_gut_step_args* args, int64_t capacity, float* const* grads, int accumulate,
                                            const lfs_gut_view_ext* ext, void* workspace, size_t workspace_bytes, lfs_stream_t stream);
LFS_API int lfs_gut_view_backward_rows_ex(const lfs_gut_step_args* args, int64_t capacity, const float* v_render, float* const* grads /* [6] host */, int accumulate,
                                          float* v_colors_out, const lfs_gut_view_ext* ext, void* workspace, size_t workspace_bytes, lfs_stream_t stream);
LFS_API int lfs_gut_step_wait(const int64_t* host_counts, int64_t stamp, double timeout_s, int64_t* n_isects, int64_t* longest);
/*   lfs_gut_train_step_ex (round 6): lfs_gut_train_step with its three per-Gaussian tail passes (SH backward + Adam on sh0 / shN, finish + Adam on the other four tensors,
 *      and the NEXT step's SH colours) as ONE launch. next_viewmat (device [4,4], nullable): the view the next step will render - its SH colours are then written to the
 *      workspace's colours for every Gaussian, from the coefficient rows as they leave their Adam update. colors_ready != 0: the caller's statement that the previous call on
 *      this workspace was this entry point with next_viewmat naming the matrix args->viewmat holds now, same N / K / sh_degree, that it fitted its buffers, and that nothing
 *      has written means / sh0 / shN since - the SH colour kernel is then not launched. Same results as lfs_gut_train_step. (= lfs_gut_train_step_opt with opts == NULL:
 *      the three lfs_gut_train_step* entry points are argument adapters of one enqueue sequence in csrc/gut_step.hip.) */
LFS_API int lfs_gut_train_step_ex(const lfs_gut_step_args* args, const float* next_viewmat, int colors_ready, int64_t capacity, int64_t assumed_longest, void* workspace,
                                  size_t workspace_bytes, int64_t* host_counts, int64_t stamp, lfs_stream_t stream);
/*   lfs_gut_train_step_opt: lfs_gut_train_step_ex for the configuration the reference trains - the photometric loss, the MCMC strategy's noise, shN frozen for the first
 *      1000 iterations - as one enqueue without a host read or a gradient tensor. opts == NULL or an all-zero struct: lfs_gut_train_step_ex itself, bit for bit.
 *      loss_kind 1 enqueues: the forward | memset(*loss) | the two photometric kernels on the workspace's render into loss_workspace (lfs_gut_step_loss_workspace_bytes;
 *      no allocation) | the accumulator-rows backward with that dL/d(render) | the tail. *loss is stored, as in the MSE form (no regulariser term in it).
 *      noise (device [N,3], standard normal) / noise_lr: what lfs_add_noise(raw_opacities, raw_scales, raw_quats, noise, means, noise_lr) would add is added to each mean
 *      in front of its Adam update, computed from the raw values before THEIR updates; the gradients are those of the un-noised mean the forward rendered (the order of
 *      mcmc.cpp:362-393: post_backward, then the optimizer step). The next view's colours (next_viewmat) are evaluated from the noised, updated mean.
 *      freeze_shN: FusedAdam group 2 is skipped (fused_adam.cpp:68-70): shN and its moments keep their bytes; exp_avg[2] / exp_avg_sq[2] may be NULL. (The step
 *      COUNT of that group is the caller's: FusedAdam::step increments it before it skips the group, :66, and a caller that wants the reference's trajectory does too.)
 *      AN ATTEMPT THAT DID NOT FIT (lfs_gut_step_fits == 0) updated no parameter and no moment and did NOT apply the noise; *loss then holds the loss of an empty render
 *      and is to be ignored. The caller enlarges the workspace and calls again with the SAME noise tensor.
 *      K > 16 (SH degree 4) with freeze_shN or noise: LFS_E_UNSUPPORTED before anything is enqueued (the three-pass tail has neither); with loss_kind 1 alone the
 *      three passes run, as in lfs_gut_train_step_ex. colors_ready: the contract of lfs_gut_train_step_ex. */
typedef struct lfs_gut_step_options {
    uint32_t loss_kind;      /* 0: folded clamped MSE (= lfs_gut_train_step_ex); 1: (1-lambda) L1 + lambda (1 - SSIM) of clamp(render,0,1), trainer.cpp:122-125 */
    float    lambda_dssim;
    uint32_t freeze_shN;     /* group 2 not updated this step (iteration <= 1000) */
    const float* noise;      /* device [N,3] or NULL: gsplat::add_noise folded in front of the means' Adam update */
    float    noise_lr;       /* its current_lr */
    void*    loss_workspace; size_t loss_workspace_bytes;   /* loss_kind 1: SSIM derivative maps + v_render */
} lfs_gut_step_options;
LFS_API size_t lfs_gut_step_loss_workspace_bytes(uint32_t image_width, uint32_t image_height);
LFS_API int lfs_gut_train_step_opt(const lfs_gut_step_args* args, const lfs_gut_step_options* opts /* NULL = all zero */, const float* next_viewmat, int colors_ready,
                                   int64_t capacity, int64_t assumed_longest, void* workspace, size_t workspace_bytes, int64_t* host_counts, int64_t stamp,
                                   lfs_stream_t stream);

/* Extension: the all-inline training step of the fused 3DGUT path (one camera, global shutter, 3 channels, ONE view per step on one rank - the
 * reference's training configuration). No parameter gradient is materialised:
 *   lfs_rasterize_to_pixels_from_world_3dgs_bwd_prepared_mse_acc : ..._bwd_prepared_mse without its last kernel - the per-Gaussian sums (rows of 16
 *       floats: dL/dA 9 | -dL/dg 3 | dL/dopacity | dL/dcolour 3) stay in the workspace at lfs_rasterize_workspace_acc_offset(C, N);
 *   lfs_sh_model_bwd_adam_all : SH backward reading dL/dcolour from those rows, Adam on sh0 AND shN in place, dL/d(dirs) written to v_dirs [N,3];
 *   lfs_gut_finish_adam       : rows -> dL/d(means, quats, scales, opacity) (raster_finish) -> raw-parameter gradients (normalize / exp / sigmoid vjp +
 *       the regularisers) -> Adam on means, raw_scales, raw_quats, raw_opacities, in one pass; *loss = the fused MSE (stored, not added).
 * Element for element the operations of the separate kernels (lfs_..._bwd_prepared_mse, lfs_sh_model_bwd_adam, lfs_activations_bwd, lfs_adam_step_multi). */
LFS_API size_t lfs_rasterize_workspace_acc_offset(uint32_t C, uint32_t N);
LFS_API int lfs_rasterize_to_pixels_from_world_3dgs_bwd_prepared_mse_acc(
    uint32_t N, const float* means, const float* quats, const float* scales, const float* colors, const float* opacities,
    const float* backgrounds, const lfs_cameras* cams, uint32_t tile_size, const int32_t* tile_offsets, const int32_t* flatten_ids,
    int64_t n_isects, const float* render_colors, const float* render_alphas, const int32_t* last_ids, const float* target_chw, float weight,
    void* workspace, size_t workspace_bytes, lfs_stream_t stream);
LFS_API int lfs_sh_model_bwd_adam_all(
    uint32_t n, uint32_t K, uint32_t degrees_to_use, const float* means, const float* viewmat, float* sh0, float* shN,
    const int32_t* radii, const float* colors, const float* acc_rows, float* v_dirs /* [n,3], written */,
    float* sh0_exp_avg, float* sh0_exp_avg_sq, const float* sh0_scalars /* host: lr, beta1, beta2, eps, bc1_rcp, bc2_sqrt_rcp */,
    float* shN_exp_avg, float* shN_exp_avg_sq, const float* shN_scalars, lfs_stream_t stream);
/* For steps that need the gradient tensors (multi-GPU all-reduce, several views per step, any loss): lfs_..._bwd_prepared_acc = lfs_..._bwd_prepared without
 * its last kernel (3 channels, one camera, no masks), then lfs_gut_finish_grads turns the accumulator rows into dL/d(means [rasterizer part], raw_scales,
 * raw_quats, raw_opacities) - written, or added to when accumulate != 0 - and dL/dcolour [N,3] in ONE pass (raster_finish + lfs_activations_bwd + the copy of
 * dL/dmeans; the regularisers as in lfs_activations_bwd); loss (nullable): += the fused MSE of lfs_..._bwd_prepared_mse_acc. */
LFS_API int lfs_rasterize_to_pixels_from_world_3dgs_bwd_prepared_acc(
    uint32_t N, const float* means, const float* quats, const float* scales, const float* colors, const float* opacities,
    const float* backgrounds, const lfs_cameras* cams, uint32_t tile_size, const int32_t* tile_offsets, const int32_t* flatten_ids,
    int64_t n_isects, const float* render_alphas, const int32_t* last_ids, const float* v_render_colors, const float* v_render_alphas,
    void* workspace, size_t workspace_bytes, lfs_stream_t stream);
LFS_API int lfs_gut_finish_grads(
    uint32_t N, const float* means, const float* raw_quats, const float* quats, const float* scales, const float* opacities, float scale_reg, float opacity_reg,
    int accumulate, float* g_means, float* g_raw_scales, float* g_raw_quats, float* g_raw_opacities, float* v_colors, float* loss,
    void* workspace, size_t workspace_bytes, lfs_stream_t stream);
/* lfs_gut_finish_grads with the riders of lfs_gut_view_ext (above): radii [N,2] of the view (nullable without a statistic); densification_info without radii is
 * LFS_E_INVALID before any launch. ext NULL or its pointer NULL: lfs_gut_finish_grads - the same launch, the same bits. */
LFS_API int lfs_gut_finish_grads_ex(
    uint32_t N, const float* means, const float* raw_quats, const float* quats, const float* scales, const float* opacities, float scale_reg, float opacity_reg,
    int accumulate, float* g_means, float* g_raw_scales, float* g_raw_quats, float* g_raw_opacities, float* v_colors, float* loss,
    const int32_t* radii, const lfs_gut_view_ext* ext, void* workspace, size_t workspace_bytes, lfs_stream_t stream);
LFS_API int lfs_gut_finish_adam(
    uint32_t N, float* means, float* raw_scales, float* raw_quats, float* raw_opacities, const float* quats, const float* scales, const float* opacities,
    const float* v_dirs /* [N,3] from lfs_sh_model_bwd_adam_all */, float* const* exp_avg /* [4] host: means, raw_scales, raw_quats, raw_opacities */,
    float* const* exp_avg_sq, const float* scalars /* [4][6] host */, float scale_reg, float opacity_reg, float* loss, void* workspace, size_t workspace_bytes,
    lfs_stream_t stream);

/* Extension ("device-side index ops with no host syncs"): MCMC::relocate_gs of the reference
 * (src/training/strategies/mcmc.cpp:113-194) as ONE enqueue without a host round trip. The reference finds the dead Gaussians with nonzero()
 * (a device->host sync for the count), draws as many sources from the alive ones with torch::multinomial(opacity), calls gsplat::relocation on
 * them, copies every parameter row source -> dead and zeroes the sources' Adam moments. Here, all on `stream`:
 *   dead_i   = sigmoid(raw_opacities_i) <= min_opacity  ||  |raw_quats_i|^2 < 1e-8
 *   source_i = inverse-CDF sample over the alive opacities with the caller's uniform number uniforms[i] in [0,1) (dead i only; fp64 prefix sums in a
 *              fixed order: the same uniforms give the same sources on every rank), count_j = how often j was drawn. source_i = the first j with
 *              cdf_j > uniforms[i] * total; a source is never a dead row, for any uniforms[i] in [0, 1] (whether the row found is alive is read from its
 *              weight: a dead one - a target at the total, an ulp step of the rounded sums - gives way to the last alive row before it)
 *   for every drawn j: (opacity, scale)_j <- relocation(opacity_j, scale_j, min(count_j + 1, n_max)), opacity clamped to [min_opacity, 1 - 1e-7]
 *                      (mcmc.cpp:149-164), raw values written back; Adam moments of ALL rows[] of j zeroed (mcmc.cpp:87-111)
 *   for every dead i : every parameter row of rows[] <- the (updated) row of source_i
 * rows[k] = {param, exp_avg, exp_avg_sq, width} for the six parameter tensors in the order means, sh0, shN, raw_scales, raw_quats, raw_opacities
 * (exp_avg / exp_avg_sq may be NULL). *n_dead (device, optional) receives the number of dead Gaussians. Nothing happens when no Gaussian is alive. */
typedef struct lfs_param_rows { float* param; float* exp_avg; float* exp_avg_sq; uint32_t width; } lfs_param_rows;
LFS_API size_t lfs_mcmc_relocate_workspace_bytes(uint32_t N);
LFS_API int lfs_mcmc_relocate(
    uint32_t N, const lfs_param_rows* rows /* [6], host */, const double* uniforms /* [N] device */, const float* binoms, int32_t n_max,
    float min_opacity, int32_t* n_dead, void* workspace, size_t workspace_bytes, lfs_stream_t stream);

/* ---- fast_gs::optimizer::adam_step (fastgs/optimizer/include/adam.h:9-20, adam_kernels.cuh:13-36).
 *      bias_correction1_rcp = 1/(1-beta1^t), bias_correction2_sqrt_rcp = 1/sqrt(1-beta2^t)
 *      (fused_adam.cpp:78-79). In place on param / exp_avg / exp_avg_sq. Unlike the reference
 *      (legacy default stream, adam.cu:22) the launch goes to `stream`. */
LFS_API int lfs_adam_step(
    float* param, float* exp_avg, float* exp_avg_sq, const float* param_grad, int64_t n_elements,
    float lr, float beta1, float beta2, float eps, float bias_correction1_rcp, float bias_correction2_sqrt_rcp,
    lfs_stream_t stream);

/* One launch for several parameter tensors (the 6 Gaussian parameter groups of
 * FusedAdam::step, fused_adam.cpp:22-95): same arithmetic as lfs_adam_step per tensor. */
typedef struct lfs_adam_tensor {
    float* param; float* exp_avg; float* exp_avg_sq; const float* grad;
    int64_t n_elements;
    float lr, beta1, beta2, eps, bias_correction1_rcp, bias_correction2_sqrt_rcp;
} lfs_adam_tensor;
#define LFS_ADAM_MAX_TENSORS 8
LFS_API int lfs_adam_step_multi(const lfs_adam_tensor* tensors /* host array */, int32_t n_tensors, lfs_stream_t stream);

/* ---- Visible-only Adam (extension; csrc/adam_visible.hip): gsplat's SelectiveAdam / the official 3DGS code's sparse_adam. A step has a
 *      visibility set V of Gaussians, given as bits: bit i of a uint32 array of lfs_visibility_words(N) = ceil(N / 32) words, bits >= N zero.
 *        i in V:     the rows of i get exactly lfs_adam_step's update - the same bits, with the scalars of the tensor's entry (the caller computes the bias
 *                    corrections from its global step count, as for lfs_adam_step_multi).
 *        i not in V: param, exp_avg and exp_avg_sq of its rows are neither read nor written and grad is not read - a NaN in such a gradient row has no effect -
 *                    except where a 16-byte access of a narrow row straddles into a visible neighbour's row (those elements are stored back as loaded).
 *      Consequence: a gradient term that reaches every Gaussian (a regulariser) does not move the Gaussians outside V.
 *   lfs_fastgs_view_visibility: bit i = (n_touched[i] != 0) of the view's primitive workspace as lfs_fastgs_view_preprocess left it - the predicate under which
 *      lfs_fastgs_view_backward adds 1 to densification_info[0][i]. Reads N, width, height and the workspace of the view. accumulate != 0: ORed into bits (the
 *      union over a step's views); 0: bits is overwritten, bits >= N of the last word with 0. One lane per Gaussian, one ballot per wave, each wave stores its own
 *      two words: no atomics, no host read. N == 0: LFS_OK, nothing launched. LFS_E_INVALID before any launch: NULL view / primitive workspace / bits, a zero image
 *      size; LFS_E_WORKSPACE: a workspace shorter than lfs_fastgs_primitive_workspace_bytes.
 *   lfs_adam_step_multi_visible: lfs_adam_step_multi over the rows of V, ONE launch. Every tensor is [N, width] with width = n_elements / N; tensors with 0
 *      elements are skipped. LFS_E_INVALID before any launch: n_elements % N != 0 (N == 0 with a non-empty tensor included), NULL visible_bits with N > 0, a NULL
 *      tensor pointer, more than LFS_ADAM_MAX_TENSORS tensors. Bits at or past N are ignored. */
LFS_API uint32_t lfs_visibility_words(uint32_t N);
LFS_API int lfs_fastgs_view_visibility(const lfs_fastgs_view* view, uint32_t* bits, int accumulate, lfs_stream_t stream);
LFS_API int lfs_adam_step_multi_visible(const lfs_adam_tensor* tensors /* host array */, int32_t n_tensors, const uint32_t* visible_bits, uint32_t N,
                                        lfs_stream_t stream);

/* ---- Contribution statistic of the EWA rasterizer (extension; csrc/fastgs_contrib.hip): what a Gaussian contributes to a view's image.
 *      For Gaussian i, over exactly the pixels p into which lfs_fastgs_view_render blends i (the alpha test passed and the pixel did not terminate AT i: an instance
 *      that terminates a pixel is not in the image and not in the statistic), with w = T alpha, T the transmittance in front of the instance, the 16-byte row
 *      stats[i] is UPDATED (never cleared: the caller zero-fills a buffer once and accumulates views into it):
 *        dword 0    bit pattern of max w       unsigned integer maximum (non-negative floats order like their bits)
 *        dword 1    number of pixels blended   uint32 add - wraps after 2^32 (pixel, view) pairs: keep W * H * views < 2^32 per buffer (contribution.py folds into
 *                                              64-bit tensors before that)
 *        dword 2-3  sum w, unsigned 64-bit fixed point with 24 fraction bits (little endian): every wavefront sums the weights of its 8x8 cell in float in a fixed
 *                   order, rounds sum * 2^24 to nearest once and adds the integer
 *      There are no float atomics: the rows are bit-reproducible from run to run and do not depend on the order in which views are accumulated.
 *      Call it after lfs_fastgs_view_preprocess[_ex] AND lfs_fastgs_view_render on the same two workspaces with the same n_instances (the render builds the instance
 *      and cell lists); the mode of the preprocess - antialiased, 3D filter, depth - is in the records, so there is no flag. Reads N, width, height, the intrinsics and
 *      the primitive workspace of the view; writes nothing but stats (device, [N,4] uint32, 8-byte aligned).
 *      Before any launch: LFS_E_INVALID for a NULL view / primitive workspace / stats, a zero image size, a negative n_instances, a misaligned stats; LFS_E_WORKSPACE
 *      for a primitive workspace shorter than lfs_fastgs_primitive_workspace_bytes or an instance workspace that is NULL or shorter than
 *      lfs_fastgs_instance_workspace_bytes; LFS_E_UNSUPPORTED beyond the record walker's limits (as lfs_fastgs_view_render). n_instances == 0 or N == 0: LFS_OK,
 *      nothing launched, stats untouched. */
LFS_API int lfs_fastgs_view_contribution(const lfs_fastgs_view* view, int64_t n_instances, void* instance_workspace, size_t instance_workspace_bytes,
                                         uint32_t* stats /* device [N,4], ADDED TO */, lfs_stream_t stream);

/* ---- Scene transform (extension; csrc/splat_transform.hip): move a splat by a similarity x' = s R x + t, the view-dependent colour included.
 *      The reference's SplatData::transform (src/core/splat_data.cpp:288) leaves shN untouched and averages a non-uniform scale; neither is reproduced.
 *   lfs_sh_rotation_matrices (pure host function): R row-major proper rotation, degree <= 4; out receives M_1 .. M_degree, row-major, packed back to back (9, 25, 49,
 *      81 doubles). a'_l = M_l a_l for band l of one colour channel in the coefficient order and signs of the SH kernels: for every unit d,
 *      sum_k a'_k Y_k(d) = sum_k a_k Y_k(R^T d). An exactly-identity R gives exactly-identity matrices. LFS_E_INVALID: NULL, degree > 4, non-finite entries.
 *   lfs_splat_transform_from_matrix (pure host function): decomposes a row-major 4x4 and fills the float32 record the kernels take - sR, t, the unit quaternion of R
 *      (wxyz, w >= 0), log s rounded once, and ALL four band matrices rounded from float64 (sh_degree only says how many of them lfs_splat_transform_apply uses). R is
 *      re-orthonormalised in float64 first. LFS_E_INVALID: NULL, non-finite entries, a last row other than (0,0,0,1), det <= 0 (s <= 0, reflections), a linear part A
 *      that is not a similarity (max |A^T A / s^2 - I| > 1e-5 with s = cbrt(det A): non-uniform scale and shear are refused, not averaged), sh_degree > 4.
 *   lfs_splat_transform_apply: xf is a HOST pointer (passed to the kernels by value). Each of the four in / out pairs may be NULL together (skipped); an output may be
 *      the same pointer as its input (in place), any other overlap is the caller's error. shN is [N, shN_rows, 3], shN_rows >= (sh_degree + 1)^2 - 1; rows beyond the
 *      rotated bands are copied through. Single-precision operations in exactly this order (no fused multiply-adds):
 *        means       ((sR[i][0] x + sR[i][1] y) + sR[i][2] z) + t[i]
 *        quats       q_R (x) q on the raw quaternion, no normalisation: w = ((w1 w2 - x1 x2) - y1 y2) - z1 z2, x = ((w1 x2 + x1 w2) + y1 z2) - z1 y2,
 *                    y = ((w1 y2 - x1 z2) + y1 w2) + z1 x2, z = ((w1 z2 + x1 y2) - y1 x2) + z1 w2 (1 = q_R, 2 = the Gaussian's)
 *        raw_scales  raw + log_s
 *        shN         per channel and band: a'_i = sum_k M[i][k] a_k, ascending k, left to right
 *      sh0 and the opacities are invariant. N == 0: LFS_OK. LFS_E_INVALID before any launch: NULL xf, sh_degree > 4, a half-NULL pair, shN_rows too small;
 *      LFS_E_UNSUPPORTED: shN_rows > 511. No workspace, no host read, no atomics. */
typedef struct lfs_splat_transform {
    float sR[9];          /* s R, row-major */
    float t[3];
    float q[4];           /* unit quaternion of R, wxyz, w >= 0 */
    float log_s;
    uint32_t sh_degree;   /* bands 1 .. sh_degree of shN are rotated */
    float m1[9], m2[25], m3[49], m4[81];   /* the band matrices, row-major */
} lfs_splat_transform;    /* 728 bytes */
LFS_API int lfs_sh_rotation_matrices(const double* R /* [9] */, uint32_t degree, double* out);
LFS_API int lfs_splat_transform_from_matrix(const double* m /* [16] */, uint32_t sh_degree, lfs_splat_transform* out);
LFS_API int lfs_splat_transform_apply(uint32_t N, const lfs_splat_transform* xf /* host */, const float* means /* [N,3] */, const float* quats /* [N,4] */,
                                      const float* raw_scales /* [N,3] */, const float* shN /* [N,shN_rows,3] */, uint32_t shN_rows, float* means_o, float* quats_o,
                                      float* raw_scales_o, float* shN_o, lfs_stream_t stream);

/* ---- Background colour on the EWA route (extension; csrc/background.hip): the compose stage between lfs_fastgs_view_render and the loss, its
 *      backward, and the RGBA target. The reference blends the background in torch outside its rasterizer (fast_rasterizer.cpp:60-66). Planes are contiguous
 *      [.,H,W] float32 device tensors; bg is passed BY VALUE (kernel arguments: no device tensor, no host read). Single-precision operations in exactly this order,
 *      no fused multiply-adds.
 *   lfs_background_compose: one launch, up to two jobs; either group's three pointers may be NULL together.
 *      render group   shown_c = image_c + (1.0f - alpha) * bg_c              image [3,H,W], alpha [1,H,W] -> shown [3,H,W]; shown == image (in place) is allowed
 *      target group   a = (float)u8 / 255.0f; out_c = a * t_c + (1.0f - a) * bg_c     target_rgb [3,H,W], target_alpha [H,W] uint8 -> target_out [3,H,W]
 *                     (a == 0: out == bg bit for bit; a == 255: out == t). target_out must not be target_rgb: LFS_E_INVALID.
 *   lfs_background_compose_bwd: d = (v_0 bg_0 + v_1 bg_1) + v_2 bg_2; v_alpha = v_alpha_in ? v_alpha_in - d : -d. v_shown [3,H,W], v_alpha_in NULL or [H,W],
 *      v_alpha [H,W] (may be v_alpha_in). dL/d(image) is v_shown itself: the caller hands the same tensor on.
 *   Any other overlap of the operands is the caller's error. LFS_E_INVALID before any launch: a NULL struct, both groups NULL, half a group, a NULL v_shown / v_alpha,
 *   a zero extent, H * W >= 2^31, a non-finite bg. 16-byte accesses are used when H * W % 4 == 0 and every float pointer involved is 16-byte aligned (the uint8 plane:
 *   4-byte); any 4-byte-aligned float tensors are accepted otherwise. No workspace, no atomics. */
typedef struct lfs_background_compose_args {
    uint32_t height, width;
    float bg[3];
    const float *image, *alpha;
    float* shown;
    const float* target_rgb;
    const uint8_t* target_alpha;
    float* target_out;
} lfs_background_compose_args;       /* 72 bytes */
typedef struct lfs_background_compose_bwd_args {
    uint32_t height, width;
    float bg[3];
    const float *v_shown, *v_alpha_in;
    float* v_alpha;
} lfs_background_compose_bwd_args;   /* 48 bytes */
LFS_API int lfs_background_compose(const lfs_background_compose_args* args, lfs_stream_t stream);
LFS_API int lfs_background_compose_bwd(const lfs_background_compose_bwd_args* args, lfs_stream_t stream);

/* ---- SOG export (csrc/sog.hip): Morton codes (kernels/morton_encoding.cu:21-97) and the three kernels of Lloyd's iteration (kernels/kmeans.cu:18-122).
 *      All entry points are asynchronous on `stream`, validate on the host before any launch (LFS_E_INVALID: NULL pointer, negative count, k or D of 0, a
 *      workspace that is not 16-byte aligned; LFS_E_UNSUPPORTED: k > 65536 or D > 64; LFS_E_WORKSPACE: workspace short), use no float atomics (same bits on every
 *      run) and return LFS_OK without a launch for N == 0.
 *      lfs_morton_encode: codes[i] = interleave21(x, y, z) + INT64_MIN with q = uint32((double)(p - min) / (double)cube * 2097151.0), the subtraction in f32,
 *        cube = max(max_axis(max - min), 1e-7f); min / max are part of the call (per-block partials, one folding block, no host read).
 *      lfs_kmeans_assign: labels[i] = argmax_c (x_i . c - |c|^2 / 2), lowest index among exactly equal scores; each score is an ascending-d f32 fmaf chain on
 *        -|c|^2 / 2 (v_mfma_f32_16x16x4_f32). 1 <= k <= 65536, 1 <= D <= 64.
 *      lfs_kmeans_assign_1d: centroids ascending; labels[i] = the first index that minimises fabsf(p - c) under a strict < (kmeans.cu:58-83), duplicates included.
 *      lfs_kmeans_update: centroids[c] = mean of data[order[seg_start[c] .. seg_start[c+1])] (f64 sums in a fixed order); order = point indices sorted by label,
 *        seg_start[k + 1] = the segment bounds. An empty segment leaves its centroid untouched (kmeans.cu:119-121). Indices outside [0, N) are skipped. */
LFS_API size_t lfs_morton_workspace_bytes(int64_t N);
LFS_API int lfs_morton_encode(int64_t N, const float* means /* [N,3] */, int64_t* codes /* [N] */, void* workspace, size_t workspace_bytes, lfs_stream_t stream);
LFS_API size_t lfs_kmeans_assign_workspace_bytes(uint32_t k, uint32_t D); /* 0: k / D out of range */
LFS_API int lfs_kmeans_assign(int64_t N, uint32_t k, uint32_t D, const float* data /* [N,D] */, const float* centroids /* [k,D] */, int32_t* labels /* [N] */,
                              void* workspace, size_t workspace_bytes, lfs_stream_t stream);
LFS_API int lfs_kmeans_assign_1d(int64_t n, uint32_t k, const float* data /* [n] */, const float* sorted_centroids /* [k] */, int32_t* labels /* [n] */,
                                 lfs_stream_t stream);
LFS_API int lfs_kmeans_update(int64_t N, uint32_t k, uint32_t D, const float* data /* [N,D] */, const int32_t* order /* [N] */, const int32_t* seg_start /* [k+1] */,
                              float* centroids /* [k,D], in place */, lfs_stream_t stream);

/* ---- ADMM sparsity optimisation (csrc/sparsity.hip; the reference's training/components/sparsity_optimizer.cpp as device passes without a sort or a host read).
 *      All entry points are asynchronous on `stream`, validate on the host before any launch (LFS_E_INVALID: NULL pointer, a count outside 0 .. 2^31 - 1, a rank
 *      outside its range, a workspace that is not 16-byte aligned; LFS_E_WORKSPACE: workspace short), use no float atomics (same bits on every run) and return
 *      LFS_OK without a launch for N == 0. The workspace is scratch: nothing in it has to survive between calls.
 *      lfs_select_kth_f32: out_value[0] = sort(x)[k - 1] (1 <= k <= N) in torch.sort's order: -0 == +0 (a zero result is +0), any NaN above +inf. A 4-pass radix
 *        select over an order-preserving key: per-workgroup LDS histograms flushed with integer atomics, a one-wave kernel between the passes.
 *      lfs_admm_update: opa = sigmoid(raw); v = opa + u; thr = the k-th smallest v; z = v > thr ? v : 0; u = u + (opa - z) - single-precision operations in this
 *        order; sigmoid is 1 / (1 + expf(-x)), the expression of lfs_activations_fwd. 0 <= k <= N; k == 0: z = 0. `initialize` is this call on a zero-filled u.
 *      lfs_admm_loss_grad: d = (opa - z) + u; g_raw_opacities (+)= scale rho d opa (1 - opa); loss[0] += scale rho / 2 sum d^2 (fixed-order two-stage tree; loss may
 *        be NULL, the workspace is then not used).
 *      lfs_admm_prune_mask: mask_u8[i] = 1 for exactly n_prune (0 .. N) elements, every one of them <= every other raw opacity; among the values equal to the
 *        boundary value the lowest indices are taken. */
LFS_API size_t lfs_select_kth_workspace_bytes(int64_t N);
LFS_API int lfs_select_kth_f32(const float* x /* [N] */, int64_t N, int64_t k, float* out_value /* [1], device */, void* workspace, size_t workspace_bytes,
                               lfs_stream_t stream);
LFS_API size_t lfs_admm_update_workspace_bytes(int64_t N);
LFS_API int lfs_admm_update(const float* raw_opacities /* [N] */, float* u /* [N], in place */, float* z /* [N], out */, int64_t N, int64_t k, void* workspace,
                            size_t workspace_bytes, lfs_stream_t stream);
LFS_API size_t lfs_admm_loss_grad_workspace_bytes(int64_t N);
LFS_API int lfs_admm_loss_grad(const float* raw_opacities /* [N] */, const float* z /* [N] */, const float* u /* [N] */, int64_t N, float rho, float scale,
                               float* g_raw_opacities /* [N] */, int accumulate, float* loss /* [1] or NULL */, void* workspace, size_t workspace_bytes,
                               lfs_stream_t stream);
LFS_API size_t lfs_admm_prune_mask_workspace_bytes(int64_t N);
LFS_API int lfs_admm_prune_mask(const float* raw_opacities /* [N] */, int64_t N, int64_t n_prune, uint8_t* mask_u8 /* [N] */, void* workspace, size_t workspace_bytes,
                                lfs_stream_t stream);

/* ---- instrumentation (not in the reference): per-kernel HIP-event timing on the launch stream.
 *      lfs_profile_enable(1) makes every entry point bracket its principal kernel(s) with events;
 *      lfs_profile_collect waits for them, sums by kernel name (names: max_entries x 64 chars)
 *      and clears the log. Returns the number of distinct names written. */
LFS_API int lfs_profile_enable(int on);
LFS_API int lfs_profile_filter(const char* name); /* only time the scopes called `name` (NULL / "" = all) */
LFS_API int lfs_profile_collect(int max_entries, char* names, float* total_ms, int* counts);

/* Library identification: returns "lfs_gsplat gfx950 <abi-version>" */
LFS_API const char* lfs_version(void);

#ifdef __cplusplus
}
#endif
#endif /* LFS_GSPLAT_H */
