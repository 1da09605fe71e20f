// Internal (not exported) entry points shared between the operator translation units and the C++ training-step driver (gut_step.hip).
// The "guarded" forms run BEFORE the host knows the intersection count: buffers are sized for `capacity` intersections, the per-tile sort
// classes are launched for lists of up to `assumed_longest` entries, the count stays on the device (RasterLists::n_isects = -1 below), and
// tile_scan_kernel raises *abort_flag - and empties every list - when either assumption fails (lfs_tilelists.cuh).
#pragma once
#include "../../include/lfs_gsplat.h"
#include <hip/hip_runtime.h>

namespace lfs {

struct Workspace { void* base; size_t bytes; };   // one stage's workspace (the intersection stage and the rasterizer each have their own)
struct IsectGuard { int64_t capacity; int64_t assumed_longest; int32_t* abort_flag; };
// the longest tile list the sort classes launched for `assumed_longest` can order (intersect.hip: SORT_CLASSES; 0xFFFFFFFF past the last class)
uint32_t sort_class_limit(int64_t assumed_longest);

// ---- one intersection call (intersect.hip): the grid, the inputs, what the direction writes, the workspace, and - the training step only - the guard ----
struct IsectGrid {
    uint32_t C, N, tile_size, tile_width, tile_height;
    uint32_t tiles() const { return C * tile_width * tile_height; }
    uint32_t rows() const { return C * tile_height; }
};
inline IsectGrid isect_grid_of_image(uint32_t N, uint32_t W, uint32_t H, uint32_t tile) { return IsectGrid{1, N, tile, (W + tile - 1) / tile, (H + tile - 1) / tile}; }   // one camera; tile > 0
struct IsectInputs { const float* means2d; const int32_t* radii; const float* depths; };   // (the count reads no depths)
// tiles_per_gauss: nullable in a guarded call (only the unsorted emit reads it, and a guarded emit always sorts)
struct IsectCounts { int32_t* tiles_per_gauss; int64_t *n_isects, *max_tile_isects; int32_t* tile_offsets; uint32_t flags; int64_t* stamp_out; int64_t stamp; };   // (as lfs_intersect_tile_count_ex)
// guarded: n_isects and max_tile_isects are ignored (the count is read from the workspace offsets on the device, the sort classes are the guard's), scratch is required
// keep_keys (default true): the per-tile sort also writes the reference's (camera | tile | depth) keys back into isect_ids. false (the training step, whose rasterizer reads
// flatten_ids and the offsets only): isect_ids keeps the parked (depth bits << 32 | flatten id) entries in bucket order - 8 B per intersection less to store. (Lists
// longer than the last LDS class are ordered in place by tile_sort_global_kernel, which rewrites isect_ids either way.)
struct IsectLists { int sort; int64_t n_isects; const int32_t* tiles_per_gauss; int64_t* isect_ids; int32_t* flatten_ids; int32_t* tile_offsets; int64_t* scratch; int64_t max_tile_isects;
                    bool keep_keys = true; };
// The workspace as byte offsets from its base: totals [T], cursor [T], row_cursor [C * tile_height] (two-pass scatter), offsets [T + 1] (offsets[T] = n_isects:
// what the guarded rasterizer calls take as tile_offsets), block_sums [ceil(C N / 2048) + 1] (the unsorted emit's scan)
struct IsectLayout { size_t totals, cursor, row_cursor, offsets, block_sums, bytes; };
constexpr size_t ISECT_SCAN_ITEMS = 2048;   // Gaussians per workgroup of the unsorted emit's scan
inline IsectLayout isect_layout(const IsectGrid& g) {
    const size_t T = size_t(g.C) * g.tile_width * g.tile_height, nb = (size_t(g.C) * g.N + ISECT_SCAN_ITEMS - 1) / ISECT_SCAN_ITEMS + 1;
    IsectLayout l{}; size_t o = 0;
    auto take = [&o](size_t nbytes) { const size_t at = o; o += (nbytes + 255) & ~size_t(255); return at; };
    l.totals = take(T * 4); l.cursor = take(T * 4); l.row_cursor = take(size_t(g.C) * g.tile_height * 4); l.offsets = take((T + 1) * 4); l.block_sums = take(nb * 8);
    l.bytes = o; return l;
}
template <class T> inline T* at_offset(void* base, size_t offset) { return reinterpret_cast<T*>(static_cast<char*>(base) + offset); }
// Both refuse - and have written, cleared and launched nothing - unless every check has passed.
int isect_count(const IsectGrid& g, const IsectInputs& in, const IsectCounts& c, const Workspace& ws, hipStream_t s, const IsectGuard* guard);
int isect_emit(const IsectGrid& g, const IsectInputs& in, const IsectLists& l, const Workspace& ws, hipStream_t s, const IsectGuard* guard);
bool isect_two_pass_supported(const IsectGrid& g);

// ---- one rasterizer call: what is rendered, the tile lists, the workspace, and what the direction reads / writes (raster.hip) ----
struct RasterScene {
    uint32_t N, channels; const float *means, *quats, *scales, *colors, *opacities, *backgrounds; const uint8_t* masks; const lfs_cameras* cams; uint32_t tile_size;
};
// n_isects >= 0: the host knows the count (operator calls); the workspace holds lists for exactly that many intersections. n_isects < 0 (guarded training step): the
// count is on the device - tile_offsets is the [T + 1] offsets of the intersection workspace (IsectLayout::offsets), the kernels read its last entry - and the lists are sized for `capacity`.
struct RasterLists {
    const int32_t *tile_offsets, *flatten_ids; int64_t n_isects, capacity;
    int32_t arg() const { return n_isects >= 0 ? int32_t(n_isects) : -1; }
    int64_t sized() const { return n_isects >= 0 ? n_isects : capacity; }
};
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
int raster_forward(const RasterScene& sc, const RasterLists& l, const Workspace& ws, const RasterFwdOut& out, hipStream_t s);
int raster_backward(const RasterScene& sc, const RasterLists& l, const Workspace& ws, const RasterBwd& b, hipStream_t s);
void raster_workspace_parts(void* workspace, uint32_t N, void** recs, void** cull);   // (the camera state is the workspace's first block)
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
                         const Workspace& ws, hipStream_t s);

// ---- the SH model entries of the step (sh.hip): the model, one view, and - the Adam forms - FusedAdam's groups 1 (sh0) and 2 (shN) of `adam` ----
// radii NULL (forward only: the step evaluates the colours BEFORE the projection): every Gaussian. colors [N,3]: written by the forward, the clamped forward output for a backward
struct ShView { const float* viewmat; const int32_t* radii; float* colors; };
struct ShGrads { float *v_sh0, *v_shN, *v_dirs; int accumulate; };
int sh_model_fwd_impl(const GutParams& p, const ShView& v, hipStream_t s);
// dL/dcolour from the rasterizer's accumulator rows, dL/d(dirs) WRITTEN to v_dirs [N,3], sh0 and shN updated in place: no SH gradient tensor exists
int sh_model_bwd_adam_all_impl(const GutParams& p, const ShView& v, const GutAdam& adam, const float* acc_rows, float* v_dirs, hipStream_t s);
// the same into gradient tensors; adam (nullable) given: shN's Adam step inline (g.v_shN unused, no accumulation, its abort flag is not looked at)
int sh_model_bwd_rows_impl(const GutParams& p, const ShView& v, const float* acc_rows, const ShGrads& g, const GutAdam* adam, hipStream_t s);

// ---- lfs_activations_project_ut with the training step's riders (projection_ut.hip) ----
struct ProjModel { uint32_t N; const float *means, *raw_quats, *raw_scales, *raw_opacities; };
struct ProjCamera { const lfs_cameras* cams; float eps2d, near_plane, far_plane, radius_clip; const lfs_ut_params* ut; };   // ut NULL: the reference's defaults
struct ProjOut { float *quats, *scales, *opacities; int32_t* radii; float *means2d, *depths; };
// Each rider saves a launch of a few microseconds: zero_words [zero_n] is cleared (the intersection stage's per-tile totals - the count then runs with
// LFS_ISECT_COUNTERS_ZERO, no memset); cams_out receives the device-side camera state (what cam_prep_kernel computes: RasterFwdOut::cams_ready); recs_out given: the
// rasterizer's records - with the colours pack_colors [N,3] - and culling records from the same pass (lfs_raster_pack.cuh: RasterFwdOut::records_ready)
struct ProjRiders { uint32_t* zero_words; uint32_t zero_n; void *cams_out, *recs_out, *cull_out; const float* pack_colors; };
int activations_project_ut_impl(const ProjModel& m, const ProjCamera& c, const ProjOut& out, const ProjRiders* riders /* nullable */, hipStream_t s);
// lfs_gut_finish_grads with dL/d(dirs) [N,3] (nullable) added to the means gradient; g.v_colors may be NULL then (the SH backward has run already)
// dens (nullable; lfs_gut_view_ext): ADC's statistic of this view - info [2,N] (visibility count | screen-equivalent gradient norm) is added to by the densifying form of
// the pass (raster_finish_densify_kernel), which reads the view's radii [N,2]. NULL or info NULL: the pass as it is without it, the same launch and the same bits.
struct GutDensify { const int32_t* radii; float* info; };
int gut_finish_grads_impl(const GutParams& p, const GutActivated& act, const GutRegs& regs, const GutGrads& g, const float* v_dirs, float* loss,
                          const Workspace& ws, hipStream_t s, const GutDensify* dens = nullptr);

// the fused tail of the all-inline step (raster.hip: gut_tail_kernel): SH backward + the six Adam updates in one pass. LFS_E_UNSUPPORTED for K > 16.
// (no GutActivated: the kernel recomputes the activated values from the raw ones it holds - lfs_activations.cuh)
int gut_tail_impl(const GutParams& p, const GutAdam& adam, const GutRegs& regs, const GutTailView& view, float* loss, const Workspace& ws, hipStream_t s);

} // namespace lfs
