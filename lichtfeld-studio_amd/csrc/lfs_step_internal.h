// Internal (not exported) entry points shared between the operator translation units and the C++ training-step driver (gut_step.hip).
// The "guarded" forms run BEFORE the host knows the intersection count: buffers are sized for `capacity` intersections, the per-tile sort
// classes are launched for lists of up to `assumed_longest` entries, the count stays on the device (RasterLists::n_isects = -1 below), and
// tile_scan_kernel raises *abort_flag - and empties every list - when either assumption fails (lfs_tilelists.cuh).
#pragma once
#include "../../include/lfs_gsplat.h"
#include <hip/hip_runtime.h>

namespace lfs {

struct IsectGuard { int64_t capacity; int64_t assumed_longest; int32_t* abort_flag; };

// the longest tile list the sort classes launched for `assumed_longest` can order (intersect.hip: <= 1024, <= 4096, <= 16384, global)
inline uint32_t sort_class_limit(int64_t assumed_longest) {
    if (assumed_longest <= 1024) return 1024u;
    if (assumed_longest <= 4096) return 4096u;
    if (assumed_longest <= 16384) return 16384u;
    return 0xFFFFFFFFu;
}

int isect_count_impl(uint32_t C, uint32_t N, const float* means2d, const int32_t* radii, uint32_t tile_size, uint32_t tile_width, uint32_t tile_height,
                     int32_t* tiles_per_gauss, int64_t* n_isects, int64_t* max_tile_isects, int32_t* tile_offsets, uint32_t flags, int64_t* stamp_out, int64_t stamp,
                     void* workspace, size_t workspace_bytes, hipStream_t s, const IsectGuard* guard);
// guard != nullptr: n_isects is ignored (read from the workspace offsets on the device), scratch is required
int isect_emit_impl(uint32_t C, uint32_t N, const float* means2d, const int32_t* radii, const float* depths, uint32_t tile_size, uint32_t tile_width,
                    uint32_t tile_height, int sort, int64_t n_isects, const int32_t* tiles_per_gauss, int64_t* isect_ids, int32_t* flatten_ids,
                    int32_t* tile_offsets, int64_t* scratch, int64_t max_tile_isects, void* workspace, size_t workspace_bytes, hipStream_t s, const IsectGuard* guard);
bool isect_two_pass_supported(uint32_t C, uint32_t N, uint32_t tile_width, uint32_t tile_height);
// the [T + 1] offsets inside an intersection workspace (offsets[T] = n_isects): what the guarded rasterizer calls take as tile_offsets
const int32_t* isect_workspace_offsets(void* workspace, uint32_t C, uint32_t N, uint32_t tile_width, uint32_t tile_height);

// ---- one rasterizer call: what is rendered, the tile lists, the workspace, and what the direction reads / writes (raster.hip) ----
struct RasterScene {
    uint32_t N, channels; const float *means, *quats, *scales, *colors, *opacities, *backgrounds; const uint8_t* masks; const lfs_cameras* cams; uint32_t tile_size;
};
// n_isects >= 0: the host knows the count (operator calls); the workspace holds lists for exactly that many intersections. n_isects < 0 (guarded training step): the
// count is on the device - tile_offsets is the [T + 1] array of isect_workspace_offsets, the kernels read its last entry - and the lists are sized for `capacity`.
struct RasterLists {
    const int32_t *tile_offsets, *flatten_ids; int64_t n_isects, capacity;
    int32_t arg() const { return n_isects >= 0 ? int32_t(n_isects) : -1; }
    int64_t sized() const { return n_isects >= 0 ? n_isects : capacity; }
};
struct RasterWorkspace { void* base; size_t bytes; };
// cams_ready / records_ready: the projection kernel wrote the device-side camera state / the records + culling records already (no cam_prep / raster_pack launch)
struct RasterFwdOut { float *render_colors, *render_alphas; int32_t* last_ids; bool cams_ready, records_ready; };
// the clamped MSE of lfs_mse_loss_fwd_bwd folded into the backward (one camera, RGB, no masks): render [H,W,3] = the forward output, target_chw [3,H,W];
// *loss += weight * mean((clamp(render, 0, 1) - target)^2), written by the finish pass - a rows-only call leaves the partial sums in the workspace and takes no loss
struct RasterMse { const float *render, *target_chw; float weight; float* loss; };
struct RasterBwd {
    const float* render_alphas; const int32_t* last_ids;
    const float *v_render_colors, *v_render_alphas;   // dL/d(render); v_render_alphas NULL: zeros
    const RasterMse* mse;                             // given: the fused MSE takes the place of v_render_*
    float *v_means, *v_quats, *v_scales, *v_colors, *v_opacities;   // unused by a rows-only call
    bool prepared;    // the workspace still holds what the forward call with the same inputs left there (camera state, records, cell lists)
    bool rows_only;   // no finish pass: the per-Gaussian accumulator rows stay in the workspace for gut_finish_* / gut_tail (one camera, RGB)
};
int raster_forward(const RasterScene& sc, const RasterLists& l, const RasterWorkspace& ws, const RasterFwdOut& out, hipStream_t s);
int raster_backward(const RasterScene& sc, const RasterLists& l, const RasterWorkspace& ws, const RasterBwd& b, hipStream_t s);
void raster_workspace_parts(void* workspace, uint32_t N, void** recs, void** cull);   // (the camera state is the workspace's first block)
int sh_model_fwd_impl(uint32_t n, uint32_t K, uint32_t degrees_to_use, const float* means, const float* viewmat, const float* sh0, const float* shN,
                      const int32_t* radii /* NULL: every Gaussian */, float* colors, hipStream_t s);
size_t raster_workspace_bytes_for(uint32_t N, uint32_t image_width, uint32_t image_height, uint32_t tile_size, int64_t capacity);
// ---- the finish and tail passes over the accumulator rows of a rows-only backward (raster.hip) ----
struct GutParams { uint32_t N, K, sh_degree; float *means, *sh0, *shN, *raw_scales, *raw_quats, *raw_opacities; };   // (the finish passes use neither K, sh_degree, sh0 nor shN)
struct GutActivated { const float *quats, *scales, *opacities; };   // what the projection kernel left in the step workspace
// FusedAdam's group order, as lfs_gut_step_args holds it: means, sh0, shN, raw_scales, raw_quats, raw_opacities; scalars[k] = {lr, beta1, beta2, eps, bc1_rcp, bc2_sqrt_rcp}
struct GutAdam { float* const* exp_avg; float* const* exp_avg_sq; const float (*scalars)[6]; const int32_t* abort_flag; };   // abort_flag (nullable): set = no update
struct GutRegs { float scale_reg, opacity_reg; };
struct GutGrads { float *means, *raw_scales, *raw_quats, *raw_opacities, *v_colors; int accumulate; };
// next_viewmat (nullable): also the NEXT view's SH colours -> colors [N,3], every Gaussian. freeze_shN: FusedAdam group 2 is not updated (iteration <= 1000), exp_avg[2] /
// exp_avg_sq[2] may be NULL. noise (nullable): lfs_add_noise(noise [N,3], noise_lr) folded in front of the means' Adam update
struct GutTailView { const float *viewmat, *next_viewmat; const int32_t* radii; float* colors; bool freeze_shN; const float* noise; float noise_lr; };
// finish + activation backward + Adam on FusedAdam groups 0, 3, 4, 5; *loss (nullable) = the fused MSE of the backward (stored, not added)
int gut_finish_adam_impl(const GutParams& p, const GutActivated& act, const GutAdam& adam, const GutRegs& regs, const float* v_dirs, float* loss,
                         const RasterWorkspace& ws, hipStream_t s);
int sh_model_bwd_adam_all_impl(uint32_t n, uint32_t K, uint32_t degrees_to_use, const float* means, const float* viewmat, float* sh0, float* shN,
                               const int32_t* radii, const float* colors, const float* acc_rows, float* v_dirs, float* sh0_exp_avg, float* sh0_exp_avg_sq,
                               const float* sh0_scalars, float* shN_exp_avg, float* shN_exp_avg_sq, const float* shN_scalars, hipStream_t s,
                               const int32_t* abort_flag);

// lfs_activations_project_ut with two riders for the training step (both save a launch of a few microseconds each): `zero_words` [zero_n] is cleared (the
// intersection stage's per-tile totals - the count kernel then runs with LFS_ISECT_COUNTERS_ZERO, no memset), and the device-side camera state the rasterizer
// kernels read is written to `cams_out` (what cam_prep_kernel computes; raster_forward with RasterFwdOut::cams_ready then skips that kernel)
int activations_project_ut_impl(uint32_t N, const float* means, const float* raw_quats, const float* raw_scales, const float* raw_opacities, const lfs_cameras* cams,
                                float eps2d, float near_plane, float far_plane, float radius_clip, const lfs_ut_params* ut_params, float* quats, float* scales,
                                float* opacities, int32_t* radii, float* means2d, float* depths, uint32_t* zero_words, uint32_t zero_n, void* cams_out, hipStream_t s,
                                void* recs_out = nullptr, void* cull_out = nullptr, const float* pack_colors = nullptr); // (given: the rasterizer's records - with these colours [N,3] - and culling records from the same pass, lfs_raster_pack.cuh)
uint32_t* isect_workspace_totals(void* workspace, uint32_t C, uint32_t N, uint32_t tile_width, uint32_t tile_height);
int sh_model_bwd_rows_impl(uint32_t n, uint32_t K, uint32_t degrees_to_use, const float* means, const float* viewmat, const float* sh0, const float* shN,
                           const int32_t* radii, const float* colors, const float* acc_rows, int accumulate, float* v_sh0, float* v_shN, float* v_dirs, hipStream_t s,
                           float* shN_exp_avg = nullptr, float* shN_exp_avg_sq = nullptr, const float* shN_scalars = nullptr); // given: shN's Adam step inline, v_shN unused
// lfs_gut_finish_grads with dL/d(dirs) [N,3] (nullable) added to the means gradient; g.v_colors may be NULL then (the SH backward has run already)
int gut_finish_grads_impl(const GutParams& p, const GutActivated& act, const GutRegs& regs, const GutGrads& g, const float* v_dirs, float* loss,
                          const RasterWorkspace& ws, hipStream_t s);

// the fused tail of the all-inline step (raster.hip: gut_tail_kernel): SH backward + the six Adam updates in one pass. LFS_E_UNSUPPORTED for K > 16.
int gut_tail_impl(const GutParams& p, const GutActivated& act, const GutAdam& adam, const GutRegs& regs, const GutTailView& view, float* loss,
                  const RasterWorkspace& ws, hipStream_t s);

} // namespace lfs
