// The --gut training step as ONE host call (C++; replaces the reference's Trainer::train_step -> rasterize() -> Ops.h sequence of
// src/training/trainer.cpp:579-770 and rasterization/rasterizer.cpp:200-344 for the path BASELINE.json's metric is quoted on: one camera per step,
// pinhole, global shutter, RGB, MSE, fused Adam).
//
// What was Python + ctypes in rounds 1-2 (fused.py: ~16 launches, each behind an interpreter round trip, and one BLOCKING host read of the
// intersection count in the middle of the step: 0.41 ms of the driver's 2.05 ms per step was not GPU time) is a straight-line enqueue here:
//
//   activations + 3DGUT projection -> tile count + scan -> SH colours -> row / tile binning -> per-tile sort -> pack -> cull -> forward ->
//   backward (MSE folded in) -> SH backward + Adam(sh0, shN) -> finish + activation backward + Adam(means, scales, quats, opacities)
//
// with NO host read on the critical path. The reference synchronises for n_isects (gsplat/Intersect.cpp:75-76) because it allocates its key / value
// arrays to that size. Here the arrays are sized for a CAPACITY the caller picked (last step's count plus a margin), the count stays on the
// device (offsets[T]; every kernel that needs it reads it there), and tile_scan_kernel guards the assumption: a count above the capacity - or a tile
// list longer than the sort classes that were launched - raises a device flag, empties all lists, and makes the two Adam kernels return without
// touching a parameter. The host looks at the (pinned) counts only AFTER it has enqueued the whole step, when they have long been written; in the rare
// overflow case it enlarges the workspace and runs the same step again - nothing was updated by the failed attempt. The GPU queue never drains.
#include "lfs_step_internal.h"
#include "lfs_prof.h"
#include <chrono>
#include <thread>

// The photometric-loss kernels (loss kind 1) live in ssim.hip. This file is also linked WITHOUT it (tests/test_emulated_step_pack.py builds the step driver from a fixed
// list of sources), so the two entry points are weak references here: absent -> loss_kind 1 is LFS_E_UNSUPPORTED, everything else works. In liblfs_gsplat.so they are
// always present.
extern "C" __attribute__((weak)) size_t lfs_photometric_loss_workspace_bytes(uint32_t H, uint32_t W);
extern "C" __attribute__((weak)) int lfs_photometric_loss_fwd_bwd(uint32_t H, uint32_t W, const float* render_hwc, const float* target_chw, float lambda_dssim, float weight,
                                                                  float* v_render_hwc, float* loss, void* workspace, size_t workspace_bytes, lfs_stream_t stream);
static bool have_loss_kernels() { return &lfs_photometric_loss_workspace_bytes != nullptr && &lfs_photometric_loss_fwd_bwd != nullptr; }

namespace lfs {
namespace {

inline size_t a256(size_t v) { return (v + 255) & ~size_t(255); }

struct StepWs {
    float *quats, *scales, *opacities, *means2d, *depths, *colors, *v_dirs, *render, *alpha;
    int32_t *radii, *tiles_per_gauss, *flatten_ids, *last_ids, *abort_flag;
    int64_t *isect_ids, *binned, *dev_counts;
    uint32_t* isect_totals; const int32_t* isect_offsets;   // inside the intersection workspace: the per-tile totals [T], the offsets [T + 1]
    IsectGrid grid;                                          // one camera; computed once (step_layout)
    Workspace isect, raster;
    size_t bytes;
};
// the step workspace as byte offsets: what a caller may look at (lfs_gut_step_layout) and the driver's own blocks
struct StepLayout { lfs_gut_step_layout pub; size_t tiles_per_gauss, v_dirs, isect, binned, raster, raster_bytes; IsectGrid grid; IsectLayout il; };

bool step_layout(uint32_t N, uint32_t W, uint32_t H, uint32_t tile, int64_t capacity, StepLayout& l) {
    if (tile == 0 || W == 0 || H == 0 || capacity <= 0) return false;
    l.grid = isect_grid_of_image(N, W, H, tile);
    l.il = isect_layout(l.grid);
    l.raster_bytes = raster_workspace_bytes_for(N, W, H, tile, capacity);
    if (l.raster_bytes == 0) return false;
    size_t o = 0;
    auto take = [&](size_t nbytes) { const size_t at = o; o += a256(nbytes); return at; };
    const size_t n = N, P = size_t(W) * H, cap = size_t(capacity);
    lfs_gut_step_layout& p = l.pub;
    p.quats = take(16 * n); p.scales = take(12 * n); p.opacities = take(4 * n); p.radii = take(8 * n); p.means2d = take(8 * n); p.depths = take(4 * n);
    l.tiles_per_gauss = take(4 * n); p.colors = take(12 * n); l.v_dirs = take(12 * n);
    l.isect = take(l.il.bytes); p.tile_offsets = l.isect + l.il.offsets;
    p.isect_ids = take(8 * cap); p.flatten_ids = take(4 * cap); l.binned = take(8 * cap);
    l.raster = take(l.raster_bytes);
    p.render = take(12 * P); p.alpha = take(4 * P); p.last_ids = take(4 * P); p.abort_flag = take(4); p.counts = take(32);
    p.bytes = o;
    return true;
}

void step_ws(void* base, const StepLayout& l, StepWs& w) {
    const lfs_gut_step_layout& p = l.pub;
    w.bytes = p.bytes; w.grid = l.grid;
    w.quats = at_offset<float>(base, p.quats); w.scales = at_offset<float>(base, p.scales); w.opacities = at_offset<float>(base, p.opacities);
    w.radii = at_offset<int32_t>(base, p.radii); w.means2d = at_offset<float>(base, p.means2d); w.depths = at_offset<float>(base, p.depths);
    w.tiles_per_gauss = at_offset<int32_t>(base, l.tiles_per_gauss); w.colors = at_offset<float>(base, p.colors); w.v_dirs = at_offset<float>(base, l.v_dirs);
    w.isect = Workspace{at_offset<char>(base, l.isect), l.il.bytes}; w.raster = Workspace{at_offset<char>(base, l.raster), l.raster_bytes};
    w.isect_totals = at_offset<uint32_t>(w.isect.base, l.il.totals); w.isect_offsets = at_offset<const int32_t>(w.isect.base, l.il.offsets);
    w.isect_ids = at_offset<int64_t>(base, p.isect_ids); w.flatten_ids = at_offset<int32_t>(base, p.flatten_ids); w.binned = at_offset<int64_t>(base, l.binned);
    w.render = at_offset<float>(base, p.render); w.alpha = at_offset<float>(base, p.alpha); w.last_ids = at_offset<int32_t>(base, p.last_ids);
    w.abort_flag = at_offset<int32_t>(base, p.abort_flag); w.dev_counts = at_offset<int64_t>(base, p.counts);
}

struct Front { lfs_cameras cams; RasterScene scene; RasterLists lists; Workspace ws; };   // (scene.cams points at cams: filled in place, not copied)

// what every guarded rasterizer call of a view takes: the camera block, the scene, the lists (count on the device, sized for `capacity`) and the workspace
void front_of(const lfs_gut_step_args* a, const StepWs& w, int64_t capacity, Front& f) {
    f.cams = lfs_cameras{};
    f.cams.C = 1; f.cams.image_width = a->image_width; f.cams.image_height = a->image_height; f.cams.camera_model = LFS_CAMERA_PINHOLE; f.cams.rs_type = LFS_SHUTTER_GLOBAL;
    f.cams.viewmats0 = a->viewmat; f.cams.Ks = a->Kmat;
    f.scene = RasterScene{};
    f.scene.N = a->N; f.scene.channels = 3; f.scene.means = a->means; f.scene.quats = w.quats; f.scene.scales = w.scales; f.scene.colors = w.colors;
    f.scene.opacities = w.opacities; f.scene.backgrounds = a->background; f.scene.cams = &f.cams; f.scene.tile_size = w.grid.tile_size;
    f.lists = RasterLists{w.isect_offsets, w.flatten_ids, -1, capacity};
    f.ws = w.raster;
}
// the groups of the finish and tail launchers, out of the argument block and the workspace
GutParams params_of(const lfs_gut_step_args* a) { return GutParams{a->N, a->K, a->sh_degree, a->means, a->sh0, a->shN, a->raw_scales, a->raw_quats, a->raw_opacities}; }
GutActivated activated_of(const StepWs& w) { return GutActivated{w.quats, w.scales, w.opacities}; }
GutAdam adam_of(const lfs_gut_step_args* a, const StepWs& w) { return GutAdam{a->exp_avg, a->exp_avg_sq, a->adam, w.abort_flag}; }

// what a call needs of its argument block: the forward's tensors only; all six Adam states; or all six with shN's optional (FusedAdam skips the frozen group)
enum class Need { Forward, Adam, AdamFrozenShN };

int check_args(const lfs_gut_step_args* a, Need need) {
    if (!a || !a->means || !a->sh0 || !a->raw_scales || !a->raw_quats || !a->raw_opacities || !a->viewmat || !a->Kmat) return LFS_E_INVALID;
    if (a->N == 0 || a->K == 0 || a->K > 32 || (a->K > 1 && !a->shN)) return LFS_E_INVALID;
    if ((a->sh_degree + 1) * (a->sh_degree + 1) > a->K || a->sh_degree > 4) return LFS_E_INVALID;
    if (need != Need::Forward) {
        if (a->K < 2 || !a->target_chw || !a->loss) return LFS_E_INVALID;   // (degree-0-only models take the gradient-tensor step: there is no shN to update)
        for (int k = 0; k < 6; ++k) if ((!a->exp_avg[k] || !a->exp_avg_sq[k]) && !(need == Need::AdamFrozenShN && k == 2)) return LFS_E_INVALID;
    }
    return LFS_OK;
}

// What every entry point does before it enqueues anything: check the arguments (and, for the training step, its options `o`), lay the workspace out and check its size.
int open_step(const lfs_gut_step_args* a, Need need, const lfs_gut_step_options* o, int64_t capacity, void* workspace, size_t workspace_bytes, StepWs& w) {
    const int rc = check_args(a, need);
    if (rc) return rc;
    if (o && a->K > 16 && (o->freeze_shN || o->noise)) return LFS_E_UNSUPPORTED;   // the three-pass tail of degree 4 has neither (enqueue_tail)
    StepLayout l;
    if (!workspace || !step_layout(a->N, a->image_width, a->image_height, a->tile_size, capacity, l)) return LFS_E_INVALID;
    if (workspace_bytes < l.pub.bytes) return LFS_E_WORKSPACE;
    step_ws(workspace, l, w);
    if (o && o->loss_kind == 1) {
        if (!have_loss_kernels()) return LFS_E_UNSUPPORTED;
        if (!o->loss_workspace) return LFS_E_INVALID;
        if (o->loss_workspace_bytes < lfs_gut_step_loss_workspace_bytes(a->image_width, a->image_height)) return LFS_E_WORKSPACE;
    }
    return LFS_OK;
}

// everything up to and including the rasterizer forward; shared by the Adam-inline step and the gradient-tensor step
// What a one-call training step leaves out of its forward (FwdLean; the split forward lfs_gut_view_forward passes none of it): work whose result the step never reads.
//   no_activations : the projection kernel does not store the activated quaternions / scales / opacities - the fused tail recomputes them from the raw values
//                    (lfs_activations.cuh). Only with the records packed by the projection kernel: raster_pack_kernel (debug bit 6) reads them.
//   no_keys        : the per-tile sort does not write the reference's keys back into isect_ids (the rasterizer reads flatten_ids and the offsets), and the count does
//                    not write tiles_per_gauss (only the unsorted emit reads it)
// (Measured and left out, profiles/r20/lean_step: the backward's accumulator memset as a rider of the scan launch - the 64 MB of zero lines then drain under the
// cull and the forward, which lose more than the memset launch costs.)
struct FwdLean { bool no_activations, no_keys; };

int enqueue_forward(const lfs_gut_step_args* a, const StepWs& w, int64_t capacity, int64_t assumed_longest, int64_t* host_counts, int64_t stamp, hipStream_t s, Front& f,
                    bool colors_ready = false, const FwdLean& lean = FwdLean{}) {   // colors_ready: w.colors holds this view's SH colours already (the previous step's fused tail wrote them)
    front_of(a, w, capacity, f);
    const lfs_ut_params ut{0.1f, 2.f, 0.f, 0.1f, 1};   // Cameras.h:27-61 defaults, as the trainer passes them (rasterizer_autograd.cpp:223-234)
    // trainer constants of rasterizer.cpp:176-181: eps2d 0.3, near 0.01, far 1e4, radius_clip 0
    // the projection kernel also clears the intersection stage's per-tile totals and writes the rasterizer's camera state (first block of the raster workspace):
    // two launches of a few microseconds each that a step does not need (the 32 KB memset and cam_prep_kernel)
    // Round 4: the SH colours are evaluated FIRST (for every Gaussian - visibility is not known yet, 6 % more coefficient rows on SYN-B) so that the projection
    // kernel, which has the activated quaternion / scale / opacity in registers, can write the rasterizer's 64-byte record and the 32-byte culling record of every
    // visible Gaussian itself: raster_pack_kernel's second pass over the Gaussians (0.040 ms, 152 MB re-read) is gone. Debug bit 6: the round-3 order (A/B, tests).
    const bool pack_here = !(lfs_get_debug_flags() & 64u);
    void *recs = nullptr, *cull = nullptr;
    raster_workspace_parts(w.raster.base, a->N, &recs, &cull);
    int rc = LFS_OK;
    if (pack_here && !colors_ready) {
        rc = sh_model_fwd_impl(params_of(a), ShView{a->viewmat, /*radii=*/nullptr, w.colors}, s);
        if (rc) return rc;
    }
    const ProjCamera cam{&f.cams, /*eps2d=*/0.3f, /*near_plane=*/0.01f, /*far_plane=*/10000.f, /*radius_clip=*/0.f, &ut};
    const ProjRiders riders{w.isect_totals, w.grid.tiles(), /*cams_out=*/w.raster.base, pack_here ? recs : nullptr, pack_here ? cull : nullptr, pack_here ? w.colors : nullptr};
    const bool store_act = !(lean.no_activations && pack_here);
    rc = activations_project_ut_impl(ProjModel{a->N, a->means, a->raw_quats, a->raw_scales, a->raw_opacities}, cam,
                                     ProjOut{store_act ? w.quats : nullptr, store_act ? w.scales : nullptr, store_act ? w.opacities : nullptr, w.radii, w.means2d, w.depths}, &riders, s);
    if (rc) return rc;
    const IsectGuard guard{capacity, assumed_longest, w.abort_flag};
    const IsectInputs in{w.means2d, w.radii, w.depths};
    int64_t* counts = host_counts ? host_counts : w.dev_counts;   // [n_isects, longest tile list, stamp]
    IsectCounts cnt{};   // (no tile_offsets copy: the rasterizer reads the workspace's own; the projection kernel has cleared the totals)
    cnt.tiles_per_gauss = lean.no_keys ? nullptr : w.tiles_per_gauss; cnt.n_isects = counts; cnt.max_tile_isects = counts + 1; cnt.stamp_out = counts + 2; cnt.stamp = stamp; cnt.flags = LFS_ISECT_COUNTERS_ZERO;
    rc = isect_count(w.grid, in, cnt, w.isect, s, &guard);
    if (rc) return rc;
    if (!pack_here && !colors_ready) { // the SH colours need the projection's radii only: enqueued between the count and the binning passes, as the Python step did with its `overlap` hook
        rc = lfs_sh_model_fwd(a->N, a->K, a->sh_degree, a->means, a->viewmat, a->sh0, a->shN, w.radii, w.colors, s);
        if (rc) return rc;
    }
    IsectLists lists{};   // (guarded: the count and the longest list are the guard's)
    lists.sort = 1; lists.n_isects = -1; lists.max_tile_isects = -1; lists.tiles_per_gauss = lean.no_keys ? nullptr : w.tiles_per_gauss; lists.isect_ids = w.isect_ids; lists.flatten_ids = w.flatten_ids; lists.scratch = w.binned;
    lists.keep_keys = !lean.no_keys;
    rc = isect_emit(w.grid, in, lists, w.isect, s, &guard);
    if (rc) return rc;
    return raster_forward(f.scene, f.lists, f.ws, RasterFwdOut{w.render, w.alpha, w.last_ids, /*cams_ready=*/true, /*records_ready=*/pack_here}, s);
}

// accumulator-rows rasterizer backward of the view in the workspace. v_render NULL: args->target_chw is the loss target, the clamped MSE is folded in; otherwise
// v_render [H,W,3] is dL/d(render)
int enqueue_backward(const lfs_gut_step_args* a, const StepWs& w, const Front& f, const float* v_render, hipStream_t s) {
    const RasterMse mse{w.render, a->target_chw, a->loss_weight, nullptr};
    RasterBwd b{};
    b.render_alphas = w.alpha; b.last_ids = w.last_ids; b.v_render_colors = v_render; b.mse = v_render ? nullptr : &mse; b.prepared = true; b.rows_only = true;
    return raster_backward(f.scene, f.lists, f.ws, b, s);
}

const float* acc_rows_of(const lfs_gut_step_args* a, const StepWs& w) {
    return reinterpret_cast<const float*>(static_cast<const char*>(w.raster.base) + lfs_rasterize_workspace_acc_offset(1, a->N));
}

// The tail as three per-Gaussian passes (SH backward + Adam on sh0 / shN, then finish + activation backward + Adam on means, raw_scales, raw_quats, raw_opacities): the
// three-pass form, and what the fused-tail form runs for K > 16 (no colours for the next step). loss (nullable): receives the fused MSE of the backward.
int three_pass_tail(const lfs_gut_step_args* a, const StepWs& w, float* loss, hipStream_t s) {
    const int rc = sh_model_bwd_adam_all_impl(params_of(a), ShView{a->viewmat, w.radii, w.colors}, adam_of(a, w), acc_rows_of(a, w), w.v_dirs, s);
    if (rc) return rc;
    return gut_finish_adam_impl(params_of(a), activated_of(w), adam_of(a, w), GutRegs{a->scale_reg, a->opacity_reg}, w.v_dirs, loss, w.raster, s);
}

// The fused-tail form's tail: the three passes as ONE launch (raster.hip: gut_tail_kernel), with shN frozen and the MCMC noise on request. K > 16 (SH degree 4) has no
// such kernel: the three passes run (the caller's next call must pass colors_ready = 0 - GutStep checks K); freeze and noise were refused by open_step.
int enqueue_tail(const lfs_gut_step_args* a, const StepWs& w, const lfs_gut_step_options& o, const float* next_viewmat, float* loss, hipStream_t s) {
    if (a->K > 16) return three_pass_tail(a, w, loss, s);
    const GutTailView view{a->viewmat, next_viewmat, w.radii, w.colors, o.freeze_shN != 0, o.noise, o.noise_lr};
    return gut_tail_impl(params_of(a), adam_of(a, w), GutRegs{a->scale_reg, a->opacity_reg}, view, loss, w.raster, s);
}

// ---- the training step: ONE sequence (open -> forward -> [loss kernels] -> backward -> tail) in two forms ----------------------------------------------------
//
// ThreePass (lfs_gut_train_step): the tail is SH backward + Adam(sh0, shN) | finish + Adam(means, scales, quaternions, opacities).
//
// FusedTail (lfs_gut_train_step_ex / _opt): those passes as ONE launch, dL/d(dirs) handed over in registers - and, when the caller names the NEXT step's view
// (next_viewmat, device [4,4]), that view's SH colours for every Gaussian from the coefficient rows as they leave their Adam update: the next call then passes
// colors_ready = 1 and its SH colour kernel is not launched.
//   three-pass :  ... backward | SH backward + Adam (0.26 ms) | finish + Adam (0.10) | [next step] SH colours (0.07) | projection ...
//   fused tail :  ... backward | tail (SH backward + six Adam updates + next colours) | [next step] projection ...
// colors_ready = 1 is the caller's statement that (a) the previous call on this workspace was this form with next_viewmat pointing at the matrix args->viewmat holds
// now, (b) with the same N, K and sh_degree, (c) it fitted its buffers (lfs_gut_step_fits), and (d) nothing has written means / sh0 / shN since. gut_step.GutStep keeps that
// book. Same results as the three-pass form, bit for bit in the deterministic accumulation mode.
// With options - what the reference actually trains (trainer.cpp:122-126, mcmc.cpp:349-386, fused_adam.cpp:68-70): the photometric loss L1 + D-SSIM instead of the folded
// MSE, the MCMC strategy's noise in front of the means' Adam update, and shN frozen while iteration <= 1000 - still one enqueue, no host read, no gradient tensor.
// loss_kind 1:
//   forward | memset(*loss) | ssim_fwd + ssim_bwd on the workspace's render -> loss_workspace (derivative maps, then v_render [H,W,3]) | accumulator-rows backward with that
//   v_render | tail (loss == NULL: *loss was written by the loss kernels)
// An attempt that did not fit rendered empty lists: its loss kernels see the background, its backward accumulates nothing, its tail returns at the abort flag - no parameter,
// no moment and no noise is applied, and *loss holds the loss of the empty render. NULL or all-zero options: the step without options, bit for bit.
enum class Form { ThreePass, FusedTail };

int train_step_impl(Form form, const lfs_gut_step_args* a, const lfs_gut_step_options* opts, const float* next_viewmat, int colors_ready, int64_t capacity,
                    int64_t assumed_longest, void* workspace, size_t workspace_bytes, int64_t* host_counts, int64_t stamp, lfs_stream_t stream) {
    const lfs_gut_step_options none{};
    const lfs_gut_step_options& o = opts ? *opts : none;
    if (o.loss_kind > 1) return LFS_E_INVALID;
    const bool ssim = o.loss_kind == 1;
    hipStream_t s = (hipStream_t)stream;
    StepWs w;
    int rc = open_step(a, o.freeze_shN ? Need::AdamFrozenShN : Need::Adam, &o, capacity, workspace, workspace_bytes, w);
    if (rc) return rc;
    FwdLean lean{};
    lean.no_keys = form == Form::FusedTail;   // (the three-pass form keeps writing what it wrote)
    lean.no_activations = form == Form::FusedTail && a->K <= 16;   // (K > 16: the fused-tail form runs the three passes, which read the stored values)
    Front f;
    rc = enqueue_forward(a, w, capacity, assumed_longest, host_counts, stamp, s, f, colors_ready != 0, lean);
    if (rc) return rc;
    float* v_render = nullptr;
    if (ssim) {
        const size_t maps_bytes = lfs_photometric_loss_workspace_bytes(a->image_height, a->image_width);
        v_render = reinterpret_cast<float*>(static_cast<char*>(o.loss_workspace) + a256(maps_bytes));
        const hipError_t e = hipMemsetAsync(a->loss, 0, sizeof(float), s);
        if (e != hipSuccess) return (int)e;
        rc = lfs_photometric_loss_fwd_bwd(a->image_height, a->image_width, w.render, a->target_chw, o.lambda_dssim, a->loss_weight, v_render, a->loss, o.loss_workspace,
                                          maps_bytes, stream);
        if (rc) return rc;
    }
    rc = enqueue_backward(a, w, f, v_render, s);
    if (rc) return rc;
    float* const tail_loss = ssim ? nullptr : a->loss;
    if (form == Form::FusedTail) return enqueue_tail(a, w, o, next_viewmat, tail_loss, s);
    return three_pass_tail(a, w, tail_loss, s);
}

} // namespace
} // namespace lfs

using namespace lfs;

extern "C" int lfs_gut_step_layout_for(uint32_t N, uint32_t image_width, uint32_t image_height, uint32_t tile_size, int64_t capacity, lfs_gut_step_layout* out) {
    StepLayout l{};
    if (!out || !step_layout(N, image_width, image_height, tile_size, capacity, l)) return LFS_E_INVALID;
    *out = l.pub;
    return LFS_OK;
}

// 1: the speculative step takes this problem shape (its binning needs the two-pass scatter: at most 512 tile rows, Gaussian index + tile column in 32 bits, debug
// bit 5 off; tile sizes the rasterizer has cell kernels for). 0: lfs_gut_* would return LFS_E_UNSUPPORTED - the caller enqueues the operators one by one instead.
extern "C" int lfs_gut_step_supported(uint32_t N, uint32_t image_width, uint32_t image_height, uint32_t tile_size) {
    if (N == 0 || tile_size < 8 || tile_size > 64 || (tile_size & 7) || image_width == 0 || image_height == 0) return 0;
    return isect_two_pass_supported(isect_grid_of_image(N, image_width, image_height, tile_size)) ? 1 : 0;
}

extern "C" int lfs_gut_step_fits(int64_t n_isects, int64_t longest, int64_t capacity, int64_t assumed_longest) {
    return (n_isects <= capacity && uint64_t(longest) <= uint64_t(sort_class_limit(assumed_longest))) ? 1 : 0;
}

extern "C" size_t lfs_gut_step_loss_workspace_bytes(uint32_t image_width, uint32_t image_height) {
    if (!have_loss_kernels()) return 0;
    return a256(lfs_photometric_loss_workspace_bytes(image_height, image_width)) + a256(size_t(12) * image_width * image_height);
}

// the three entry points of the training step: argument adapters of train_step_impl
extern "C" int lfs_gut_train_step(const lfs_gut_step_args* a, int64_t capacity, int64_t assumed_longest, void* workspace, size_t workspace_bytes,
                                  int64_t* host_counts, int64_t stamp, lfs_stream_t stream) {
    return train_step_impl(Form::ThreePass, a, nullptr, nullptr, 0, capacity, assumed_longest, workspace, workspace_bytes, host_counts, stamp, stream);
}

extern "C" int lfs_gut_train_step_ex(const lfs_gut_step_args* a, const float* next_viewmat, int colors_ready, int64_t capacity, int64_t assumed_longest, void* workspace,
                                     size_t workspace_bytes, int64_t* host_counts, int64_t stamp, lfs_stream_t stream) {
    return train_step_impl(Form::FusedTail, a, nullptr, next_viewmat, colors_ready, capacity, assumed_longest, workspace, workspace_bytes, host_counts, stamp, stream);
}

extern "C" int lfs_gut_train_step_opt(const lfs_gut_step_args* a, const lfs_gut_step_options* opts, const float* next_viewmat, int colors_ready, int64_t capacity,
                                      int64_t assumed_longest, void* workspace, size_t workspace_bytes, int64_t* host_counts, int64_t stamp, lfs_stream_t stream) {
    return train_step_impl(Form::FusedTail, a, opts, next_viewmat, colors_ready, capacity, assumed_longest, workspace, workspace_bytes, host_counts, stamp, stream);
}

// Backward of the view lfs_gut_view_forward left in the workspace, into GRADIENT TENSORS (data-parallel ranks, several views per step, iterations <= 1000):
// grads = means, sh0, shN, raw_scales, raw_quats, raw_opacities - written (accumulate == 0) or added to. Two halves, so that a data-parallel caller can put
// the all-reduce of the SH gradients (45 of 59 floats per Gaussian at degree 3) on the wire between them:
//   lfs_gut_view_backward_sh     : accumulator-only rasterizer backward (with target_chw the clamped MSE is folded in, otherwise v_render [H,W,3] is the
//                                  caller's dL/d(render)), then the SH backward straight from the accumulator rows -> grads[1], grads[2] final for this view
//   lfs_gut_view_backward_finish : rows + dL/d(dirs) -> grads[0], grads[3..5] (raster_finish + activation backward + regularisers); *loss += the fused MSE
// An attempt that did not fit its buffers (lfs_gut_step_fits) rendered EMPTY lists: the caller checks the counts of the forward before it calls these.
extern "C" int lfs_gut_view_backward_sh(const lfs_gut_step_args* a, int64_t capacity, const float* v_render, float* const* grads /* [6] host */, int accumulate,
                                        void* workspace, size_t workspace_bytes, lfs_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    StepWs w;
    int rc = open_step(a, Need::Forward, nullptr, capacity, workspace, workspace_bytes, w);
    if (rc) return rc;
    // args->exp_avg[2] given: shN's Adam step runs inside the SH backward (one view per step, one rank - the reference's MCMC / L1+D-SSIM / bilateral-grid
    // steps, whose other five tensors go through gradient tensors and FusedAdam); grads[2] is then neither read nor written
    const bool inline_shN = a->K > 1 && a->exp_avg[2] != nullptr;
    if (inline_shN && (accumulate || !a->exp_avg_sq[2])) return LFS_E_INVALID;
    if (!grads || !grads[1] || (a->K > 1 && !grads[2] && !inline_shN) || (!a->target_chw && !v_render)) return LFS_E_INVALID;
    Front f;
    front_of(a, w, capacity, f);
    rc = enqueue_backward(a, w, f, a->target_chw ? nullptr : v_render, s);
    if (rc) return rc;
    const GutAdam adam = adam_of(a, w);
    return sh_model_bwd_rows_impl(params_of(a), ShView{a->viewmat, w.radii, w.colors}, acc_rows_of(a, w), ShGrads{grads[1], grads[2], w.v_dirs, accumulate},
                                  inline_shN ? &adam : nullptr, s);
}

// The _ex forms carry the riders of the finish pass (lfs_gut_view_ext: ADC's densification statistic of the view, from the radii the forward left in the workspace);
// the entries without _ex are their argument adapters (ext = NULL: the same launches, the same bits).
static GutDensify densify_of(const lfs_gut_view_ext* ext, const StepWs& w) { return GutDensify{w.radii, ext ? ext->densification_info : nullptr}; }

extern "C" int lfs_gut_view_backward_finish_ex(const lfs_gut_step_args* a, int64_t capacity, float* const* grads /* [6] host */, int accumulate,
                                               const lfs_gut_view_ext* ext, void* workspace, size_t workspace_bytes, lfs_stream_t stream) {
    StepWs w;
    const int rc = open_step(a, Need::Forward, nullptr, capacity, workspace, workspace_bytes, w);
    if (rc) return rc;
    if (!grads || !grads[0] || !grads[3] || !grads[4] || !grads[5] || (a->target_chw && !a->loss)) return LFS_E_INVALID;
    const GutDensify dens = densify_of(ext, w);
    return gut_finish_grads_impl(params_of(a), activated_of(w), GutRegs{a->scale_reg, a->opacity_reg}, GutGrads{grads[0], grads[3], grads[4], grads[5], nullptr, accumulate},
                                 w.v_dirs, a->target_chw ? a->loss : nullptr, w.raster, (hipStream_t)stream, &dens);
}

extern "C" int lfs_gut_view_backward_finish(const lfs_gut_step_args* a, int64_t capacity, float* const* grads /* [6] host */, int accumulate,
                                            void* workspace, size_t workspace_bytes, lfs_stream_t stream) {
    return lfs_gut_view_backward_finish_ex(a, capacity, grads, accumulate, nullptr, workspace, workspace_bytes, stream);
}

// The view's backward for the FACTORED gradient exchange of the replicated data-parallel layout (dist.ColorGradExchange): rasterizer backward, then the finish pass -
// grads[0], grads[3..5] (means WITHOUT the SH direction term, scales, quaternions, opacities), written or added to - and dL/dcolour [N,3] -> v_colors_out. No SH
// backward here: per view the gradient of the SH coefficients is the outer product basis(direction) x dL/dcolour, every rank knows every rank's camera, so the ranks
// exchange the 3-float rows and each evaluates the multi-view SH backward (lfs_sh_model_bwd_views) over ALL views itself.
extern "C" int lfs_gut_view_backward_rows_ex(const lfs_gut_step_args* a, int64_t capacity, const float* v_render, float* const* grads /* [6] host */, int accumulate,
                                             float* v_colors_out, const lfs_gut_view_ext* ext, void* workspace, size_t workspace_bytes, lfs_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    StepWs w;
    int rc = open_step(a, Need::Forward, nullptr, capacity, workspace, workspace_bytes, w);
    if (rc) return rc;
    if (!grads || !grads[0] || !grads[3] || !grads[4] || !grads[5] || !v_colors_out || (!a->target_chw && !v_render) || (a->target_chw && !a->loss)) return LFS_E_INVALID;
    Front f;
    front_of(a, w, capacity, f);
    rc = enqueue_backward(a, w, f, a->target_chw ? nullptr : v_render, s);
    if (rc) return rc;
    const GutDensify dens = densify_of(ext, w);
    return gut_finish_grads_impl(params_of(a), activated_of(w), GutRegs{a->scale_reg, a->opacity_reg}, GutGrads{grads[0], grads[3], grads[4], grads[5], v_colors_out, accumulate},
                                 nullptr, a->target_chw ? a->loss : nullptr, w.raster, s, &dens);
}

extern "C" int lfs_gut_view_backward_rows(const lfs_gut_step_args* a, int64_t capacity, const float* v_render, float* const* grads /* [6] host */, int accumulate,
                                          float* v_colors_out, void* workspace, size_t workspace_bytes, lfs_stream_t stream) {
    return lfs_gut_view_backward_rows_ex(a, capacity, v_render, grads, accumulate, v_colors_out, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int lfs_gut_view_backward_ex(const lfs_gut_step_args* a, int64_t capacity, const float* v_render, float* const* grads /* [6] host */, int accumulate,
                                        const lfs_gut_view_ext* ext, void* workspace, size_t workspace_bytes, lfs_stream_t stream) {
    const int rc = lfs_gut_view_backward_sh(a, capacity, v_render, grads, accumulate, workspace, workspace_bytes, stream);
    return rc ? rc : lfs_gut_view_backward_finish_ex(a, capacity, grads, accumulate, ext, workspace, workspace_bytes, stream);
}

extern "C" int lfs_gut_view_backward(const lfs_gut_step_args* a, int64_t capacity, const float* v_render, float* const* grads /* [6] host */, int accumulate,
                                     void* workspace, size_t workspace_bytes, lfs_stream_t stream) {
    return lfs_gut_view_backward_ex(a, capacity, v_render, grads, accumulate, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int lfs_gut_view_forward(const lfs_gut_step_args* a, int64_t capacity, int64_t assumed_longest, void* workspace, size_t workspace_bytes,
                                    int64_t* host_counts, int64_t stamp, lfs_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    StepWs w;
    const int rc = open_step(a, Need::Forward, nullptr, capacity, workspace, workspace_bytes, w);
    if (rc) return rc;
    Front f;
    return enqueue_forward(a, w, capacity, assumed_longest, host_counts, stamp, s, f);
}

// Wait until the counts of the call stamped `stamp` have arrived in pinned host memory (they were written early in the step; by the time the host has
// enqueued the rest this returns at once). 0 = ok, LFS_E_INVALID on timeout.
extern "C" int lfs_gut_step_wait(const int64_t* host_counts, int64_t stamp, double timeout_s, int64_t* n_isects, int64_t* longest) {
    if (!host_counts) return LFS_E_INVALID;
    const volatile int64_t* c = host_counts;
    const auto t0 = std::chrono::steady_clock::now();
    int spins = 0;
    while (c[2] != stamp) {
        if (++spins > 64) {
            std::this_thread::yield();
            if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s) return LFS_E_INVALID;
        }
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    if (n_isects) *n_isects = c[0];
    if (longest) *longest = c[1];
    return LFS_OK;
}
