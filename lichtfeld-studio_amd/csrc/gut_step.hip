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
    void *isect_ws, *raster_ws;
    size_t isect_ws_bytes, raster_ws_bytes, bytes;
};

bool step_ws(void* base, uint32_t N, uint32_t W, uint32_t H, uint32_t tile, int64_t capacity, StepWs& w, lfs_gut_step_layout* lay) {
    if (tile == 0 || W == 0 || H == 0 || capacity <= 0) return false;
    const uint32_t tw = (W + tile - 1) / tile, th = (H + tile - 1) / tile;
    char* p = static_cast<char*>(base);
    size_t o = 0;
    auto take = [&](size_t nbytes) { const size_t at = o; o += a256(nbytes); return at; };
    const size_t n = N, P = size_t(W) * H, cap = size_t(capacity);
    const size_t o_quats = take(16 * n), o_scales = take(12 * n), o_opac = take(4 * n), o_radii = take(8 * n), o_m2d = take(8 * n), o_depths = take(4 * n);
    const size_t o_tpg = take(4 * n), o_colors = take(12 * n), o_vdirs = take(12 * n);
    w.isect_ws_bytes = lfs_intersect_tile_workspace_bytes(1, N, tw, th);
    const size_t o_iws = take(w.isect_ws_bytes);
    const size_t o_ids = take(8 * cap), o_flat = take(4 * cap), o_binned = take(8 * cap);
    w.raster_ws_bytes = raster_workspace_bytes_for(N, W, H, tile, capacity);
    if (w.raster_ws_bytes == 0) return false;
    const size_t o_rws = take(w.raster_ws_bytes);
    const size_t o_render = take(12 * P), o_alpha = take(4 * P), o_last = take(4 * P), o_flag = take(4), o_counts = take(32);
    w.bytes = o;
    w.quats = (float*)(p + o_quats); w.scales = (float*)(p + o_scales); w.opacities = (float*)(p + o_opac); w.radii = (int32_t*)(p + o_radii);
    w.means2d = (float*)(p + o_m2d); w.depths = (float*)(p + o_depths); w.tiles_per_gauss = (int32_t*)(p + o_tpg); w.colors = (float*)(p + o_colors);
    w.v_dirs = (float*)(p + o_vdirs); w.isect_ws = p + o_iws; w.isect_ids = (int64_t*)(p + o_ids); w.flatten_ids = (int32_t*)(p + o_flat);
    w.binned = (int64_t*)(p + o_binned); w.raster_ws = p + o_rws; w.render = (float*)(p + o_render); w.alpha = (float*)(p + o_alpha);
    w.last_ids = (int32_t*)(p + o_last); w.abort_flag = (int32_t*)(p + o_flag); w.dev_counts = (int64_t*)(p + o_counts);
    if (lay) {
        lay->bytes = o; lay->quats = o_quats; lay->scales = o_scales; lay->opacities = o_opac; lay->radii = o_radii; lay->means2d = o_m2d; lay->depths = o_depths;
        lay->colors = o_colors; lay->isect_ids = o_ids; lay->flatten_ids = o_flat; lay->render = o_render; lay->alpha = o_alpha; lay->last_ids = o_last;
        lay->abort_flag = o_flag; lay->counts = o_counts;
        lay->tile_offsets = o_iws + size_t(reinterpret_cast<const char*>(isect_workspace_offsets(nullptr, 1, N, tw, th)) - static_cast<const char*>(nullptr));
    }
    return true;
}

struct Front { lfs_cameras cams; RasterScene scene; RasterLists lists; RasterWorkspace ws; };   // (scene.cams points at cams: filled in place, not copied)

// what every guarded rasterizer call of a view takes: the camera block, the scene, the lists (count on the device, sized for `capacity`) and the workspace
void front_of(const lfs_gut_step_args* a, const StepWs& w, int64_t capacity, Front& f) {
    const uint32_t tile = a->tile_size, tw = (a->image_width + tile - 1) / tile, th = (a->image_height + tile - 1) / tile;
    f.cams = lfs_cameras{};
    f.cams.C = 1; f.cams.image_width = a->image_width; f.cams.image_height = a->image_height; f.cams.camera_model = LFS_CAMERA_PINHOLE; f.cams.rs_type = LFS_SHUTTER_GLOBAL;
    f.cams.viewmats0 = a->viewmat; f.cams.Ks = a->Kmat;
    f.scene = RasterScene{};
    f.scene.N = a->N; f.scene.channels = 3; f.scene.means = a->means; f.scene.quats = w.quats; f.scene.scales = w.scales; f.scene.colors = w.colors;
    f.scene.opacities = w.opacities; f.scene.backgrounds = a->background; f.scene.cams = &f.cams; f.scene.tile_size = tile;
    f.lists = RasterLists{isect_workspace_offsets(w.isect_ws, 1, a->N, tw, th), w.flatten_ids, -1, capacity};
    f.ws = RasterWorkspace{w.raster_ws, w.raster_ws_bytes};
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
    if (!workspace) return LFS_E_INVALID;
    if (!step_ws(workspace, a->N, a->image_width, a->image_height, a->tile_size, capacity, w, nullptr)) return LFS_E_INVALID;
    if (workspace_bytes < w.bytes) return LFS_E_WORKSPACE;
    if (o && o->loss_kind == 1) {
        if (!have_loss_kernels()) return LFS_E_UNSUPPORTED;
        if (!o->loss_workspace) return LFS_E_INVALID;
        if (o->loss_workspace_bytes < lfs_gut_step_loss_workspace_bytes(a->image_width, a->image_height)) return LFS_E_WORKSPACE;
    }
    return LFS_OK;
}

// everything up to and including the rasterizer forward; shared by the Adam-inline step and the gradient-tensor step
int enqueue_forward(const lfs_gut_step_args* a, const StepWs& w, int64_t capacity, int64_t assumed_longest, int64_t* host_counts, int64_t stamp, hipStream_t s, Front& f,
                    bool colors_ready = false) {   // colors_ready: w.colors holds this view's SH colours already (the previous step's fused tail wrote them)
    const uint32_t N = a->N, W = a->image_width, H = a->image_height, tile = a->tile_size;
    const uint32_t tw = (W + tile - 1) / tile, th = (H + tile - 1) / tile;
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
    raster_workspace_parts(w.raster_ws, N, &recs, &cull);
    int rc = LFS_OK;
    if (pack_here && !colors_ready) {
        rc = sh_model_fwd_impl(N, a->K, a->sh_degree, a->means, a->viewmat, a->sh0, a->shN, nullptr, w.colors, s);
        if (rc) return rc;
    }
    rc = activations_project_ut_impl(N, a->means, a->raw_quats, a->raw_scales, a->raw_opacities, &f.cams, 0.3f, 0.01f, 10000.f, 0.f, &ut, w.quats, w.scales,
                                     w.opacities, w.radii, w.means2d, w.depths, isect_workspace_totals(w.isect_ws, 1, N, tw, th), tw * th, w.raster_ws, s,
                                     pack_here ? recs : nullptr, pack_here ? cull : nullptr, pack_here ? w.colors : nullptr);
    if (rc) return rc;
    const IsectGuard guard{capacity, assumed_longest, w.abort_flag};
    int64_t* counts = host_counts ? host_counts : w.dev_counts;   // [n_isects, longest tile list, stamp]
    rc = isect_count_impl(1, N, w.means2d, w.radii, tile, tw, th, w.tiles_per_gauss, counts, counts + 1, nullptr, LFS_ISECT_COUNTERS_ZERO, counts + 2, stamp, w.isect_ws,
                          w.isect_ws_bytes, s, &guard);
    if (rc) return rc;
    if (!pack_here && !colors_ready) { // the SH colours need the projection's radii only: enqueued between the count and the binning passes, as the Python step did with its `overlap` hook
        rc = lfs_sh_model_fwd(N, a->K, a->sh_degree, a->means, a->viewmat, a->sh0, a->shN, w.radii, w.colors, s);
        if (rc) return rc;
    }
    rc = isect_emit_impl(1, N, w.means2d, w.radii, w.depths, tile, tw, th, 1, -1, w.tiles_per_gauss, w.isect_ids, w.flatten_ids, nullptr, w.binned, -1, w.isect_ws,
                         w.isect_ws_bytes, s, &guard);
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
    return reinterpret_cast<const float*>(static_cast<const char*>(w.raster_ws) + lfs_rasterize_workspace_acc_offset(1, a->N));
}

// The tail as three per-Gaussian passes (SH backward + Adam on sh0 / shN, then finish + activation backward + Adam on means, raw_scales, raw_quats, raw_opacities): the
// three-pass form, and what the fused-tail form runs for K > 16 (no colours for the next step). loss (nullable): receives the fused MSE of the backward.
int three_pass_tail(const lfs_gut_step_args* a, const StepWs& w, float* loss, hipStream_t s) {
    const int rc = sh_model_bwd_adam_all_impl(a->N, a->K, a->sh_degree, a->means, a->viewmat, a->sh0, a->shN, w.radii, w.colors, acc_rows_of(a, w), w.v_dirs, a->exp_avg[1],
                                              a->exp_avg_sq[1], a->adam[1], a->exp_avg[2], a->exp_avg_sq[2], a->adam[2], s, w.abort_flag);
    if (rc) return rc;
    return gut_finish_adam_impl(params_of(a), activated_of(w), adam_of(a, w), GutRegs{a->scale_reg, a->opacity_reg}, w.v_dirs, loss, RasterWorkspace{w.raster_ws, w.raster_ws_bytes}, s);
}

// The fused-tail form's tail: the three passes as ONE launch (raster.hip: gut_tail_kernel), with shN frozen and the MCMC noise on request. K > 16 (SH degree 4) has no
// such kernel: the three passes run (the caller's next call must pass colors_ready = 0 - GutStep checks K); freeze and noise were refused by open_step.
int enqueue_tail(const lfs_gut_step_args* a, const StepWs& w, const lfs_gut_step_options& o, const float* next_viewmat, float* loss, hipStream_t s) {
    if (a->K > 16) return three_pass_tail(a, w, loss, s);
    const GutTailView view{a->viewmat, next_viewmat, w.radii, w.colors, o.freeze_shN != 0, o.noise, o.noise_lr};
    return gut_tail_impl(params_of(a), activated_of(w), adam_of(a, w), GutRegs{a->scale_reg, a->opacity_reg}, view, loss, RasterWorkspace{w.raster_ws, w.raster_ws_bytes}, s);
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
    Front f;
    rc = enqueue_forward(a, w, capacity, assumed_longest, host_counts, stamp, s, f, colors_ready != 0);
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
    if (!out) return LFS_E_INVALID;
    StepWs w;
    if (!step_ws(nullptr, N, image_width, image_height, tile_size, capacity, w, out)) return LFS_E_INVALID;
    return LFS_OK;
}

// 1: the speculative step takes this problem shape (its binning needs the two-pass scatter: at most 512 tile rows, Gaussian index + tile column in 32 bits, debug
// bit 5 off; tile sizes the rasterizer has cell kernels for). 0: lfs_gut_* would return LFS_E_UNSUPPORTED - the caller enqueues the operators one by one instead.
extern "C" int lfs_gut_step_supported(uint32_t N, uint32_t image_width, uint32_t image_height, uint32_t tile_size) {
    if (N == 0 || tile_size < 8 || tile_size > 64 || (tile_size & 7) || image_width == 0 || image_height == 0) return 0;
    const uint32_t tw = (image_width + tile_size - 1) / tile_size, th = (image_height + tile_size - 1) / tile_size;
    return isect_two_pass_supported(1, N, tw, th) ? 1 : 0;
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
    return sh_model_bwd_rows_impl(a->N, a->K, a->sh_degree, a->means, a->viewmat, a->sh0, a->shN, w.radii, w.colors, acc_rows_of(a, w), accumulate, grads[1], grads[2], w.v_dirs,
                                  s, inline_shN ? a->exp_avg[2] : nullptr, inline_shN ? a->exp_avg_sq[2] : nullptr, inline_shN ? a->adam[2] : nullptr);
}

extern "C" int lfs_gut_view_backward_finish(const lfs_gut_step_args* a, int64_t capacity, float* const* grads /* [6] host */, int accumulate,
                                            void* workspace, size_t workspace_bytes, lfs_stream_t stream) {
    StepWs w;
    const int rc = open_step(a, Need::Forward, nullptr, capacity, workspace, workspace_bytes, w);
    if (rc) return rc;
    if (!grads || !grads[0] || !grads[3] || !grads[4] || !grads[5] || (a->target_chw && !a->loss)) return LFS_E_INVALID;
    return gut_finish_grads_impl(params_of(a), activated_of(w), GutRegs{a->scale_reg, a->opacity_reg}, GutGrads{grads[0], grads[3], grads[4], grads[5], nullptr, accumulate},
                                 w.v_dirs, a->target_chw ? a->loss : nullptr, RasterWorkspace{w.raster_ws, w.raster_ws_bytes}, (hipStream_t)stream);
}

// The view's backward for the FACTORED gradient exchange of the replicated data-parallel layout (dist.ColorGradExchange): rasterizer backward, then the finish pass -
// grads[0], grads[3..5] (means WITHOUT the SH direction term, scales, quaternions, opacities), written or added to - and dL/dcolour [N,3] -> v_colors_out. No SH
// backward here: per view the gradient of the SH coefficients is the outer product basis(direction) x dL/dcolour, every rank knows every rank's camera, so the ranks
// exchange the 3-float rows and each evaluates the multi-view SH backward (lfs_sh_model_bwd_views) over ALL views itself.
extern "C" int lfs_gut_view_backward_rows(const lfs_gut_step_args* a, int64_t capacity, const float* v_render, float* const* grads /* [6] host */, int accumulate,
                                          float* v_colors_out, void* workspace, size_t workspace_bytes, lfs_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    StepWs w;
    int rc = open_step(a, Need::Forward, nullptr, capacity, workspace, workspace_bytes, w);
    if (rc) return rc;
    if (!grads || !grads[0] || !grads[3] || !grads[4] || !grads[5] || !v_colors_out || (!a->target_chw && !v_render) || (a->target_chw && !a->loss)) return LFS_E_INVALID;
    Front f;
    front_of(a, w, capacity, f);
    rc = enqueue_backward(a, w, f, a->target_chw ? nullptr : v_render, s);
    if (rc) return rc;
    return gut_finish_grads_impl(params_of(a), activated_of(w), GutRegs{a->scale_reg, a->opacity_reg}, GutGrads{grads[0], grads[3], grads[4], grads[5], v_colors_out, accumulate},
                                 nullptr, a->target_chw ? a->loss : nullptr, RasterWorkspace{w.raster_ws, w.raster_ws_bytes}, s);
}

extern "C" int lfs_gut_view_backward(const lfs_gut_step_args* a, int64_t capacity, const float* v_render, float* const* grads /* [6] host */, int accumulate,
                                     void* workspace, size_t workspace_bytes, lfs_stream_t stream) {
    const int rc = lfs_gut_view_backward_sh(a, capacity, v_render, grads, accumulate, workspace, workspace_bytes, stream);
    return rc ? rc : lfs_gut_view_backward_finish(a, capacity, grads, accumulate, workspace, workspace_bytes, stream);
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
