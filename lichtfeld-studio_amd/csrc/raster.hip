// K7 / K8 — world-space (3DGUT) alpha compositing and its backward (replace
// gsplat::rasterize_to_pixels_from_world_3dgs_fwd / _bwd; reference:
// gsplat/RasterizeToPixelsFromWorld3DGSFwd.cu:19-279, ...Bwd.cu:16-373,
// host gsplat/Rasterization.cpp:20-261, helpers gsplat/Utils.cuh:80-194).
//
// CDNA4 design (not the reference's block-cooperative shared-memory batches):
//  * pack   : one pass turns every Gaussian into a 64-byte record - all the
//             per-Gaussian work the reference redoes per tile batch (rotmat,
//             1/scale, matrix product) happens once per Gaussian, coalesced.
//             Global shutter (round 6, LFS_REC_ROT): { U M (9), G^2, G, log2
//             opacity, rgb } with M = c S^-1 R^T Rinv and U the rotation that
//             puts g = M (o - mu) on the third axis: the distance of a ray to
//             the centre is then |g| sin(angle) = G^2 m / l from the three
//             components of q = U M d alone - no foot vector in the forward,
//             no difference of large numbers anywhere (lfs_raster_common.cuh).
//             Rolling shutters: { M (9), mu (3), ... }, per-pixel origins.
//  * raster : a wavefront owns an 8x8 pixel cell of a tile and walks the tile's
//             depth-sorted list ALONE: the list position is wave-uniform, so the
//             record arrives through the scalar unit (s_load_dwordx16 into
//             SGPRs, served by the scalar cache / L2) and feeds v_fma_f32
//             directly. No LDS staging, no __syncthreads, no 64-lane broadcast
//             reads; early-out, the alpha < 1/255 skip and the backward's
//             "behind the last contributor" skip are per 8x8 cell (ballot),
//             4x finer than the reference's 16x16 block.
//  * bwd    : with a = s w (s = alpha dL/dalpha, w the foot vector) the record's
//             gradient is dL/dM = -B M^-T, B = sum s w w^T, and dL/dg = -sum a
//             (LFS_ACC_SYM): a lane accumulates B (6), a (3), dL/dopacity,
//             dL/drgb = 13 floats; an LDS transpose (ds_write_addtid_b32 rows,
//             ds_read_b128 columns, two quad-permute DPP adds) leaves the wave
//             sums one per quad and ONE global_atomic_add_f32 instruction per
//             (wave, Gaussian) adds them to a [C*N][16] accumulator (the
//             reference: 14 shuffle reductions x 5 steps + 14 scalar atomics per
//             (warp, Gaussian)). Rolling shutters: dL/dM (9) + dL/dg (3).
//  * finish : one pass maps the accumulator through the quaternion / scale /
//             mean vjp (done per (pixel, Gaussian) in the reference);
//             dL/dscale_c = B_cc / s_c has no cancellation left in it.
// Measured and removed in round 5 (commit f684d4b, profiles/r05/lease4/ab_fwdzero_off.txt): the forward kernel clearing the backward's accumulator rows on the side (two or three
// 16-byte stores per lane at kernel start, instead of the 64 MB hipMemsetAsync in front of the backward: 9 - 10 us): raster_fwd 0.234 -> 0.247 ms, step +0.015 - 0.025 ms - stores
// issued by a VALU-bound kernel are not free. Round 6 (profiles/r06/lease15_ab_tail_acc_clear.txt): the same 64 MB cleared by the step's PROJECTION kernel (four 16-byte stores per lane at its
// top): projection 0.064 -> 0.081 ms, step +0.007 ms against the memset's 0.0115 ms + launch gap - that kernel moves 204 MB in 64 us and has no memory slack either: removed.
// Measured and removed in round 3 (kernels in git history up to e34272a, numbers under profiles/): 16x8 "wide" cells with two pixels per lane
// (profiles/r01/raster_wide_cells_ab.json: bwd 0.84 vs 0.69 ms), quadrant-row kernels with DPP-broadcast records (profiles/r02/raster_rows_vs_default_pmc.txt:
// 1.17x the VALU instructions), SH colours + record packing in one kernel (profiles/r02/fuse_front_ab.txt: no gain).
#include "lfs_camera.cuh"
#include "lfs_prof.h"
#ifndef LFS_EMULATE
#include <hip/hip_ext.h>
#endif
#include "lfs_raster_common.cuh"
#include "lfs_cull_conic.cuh"
#include "lfs_raster_pack.cuh"
#include "lfs_adam.cuh"
#include "lfs_raster_finish.cuh"   // finish_geometry, FinishAdam / FinishGrads, LOSS_SLOTS
#include "lfs_sh.cuh"
#include "lfs_mcmc_noise.cuh"
#include "lfs_activations.cuh"
#include "lfs_step_internal.h"
#ifdef LFS_EMULATE   // (the densifying finish pass is a code object of its own on the GPU; a host build of this file carries it)
#define LFS_RASTER_DENSIFY_INLINE
#include "raster_densify.hip"
#endif

// LFS_BWD_REORTH (default 1 since round 5; -DLFS_BWD_REORTH=0 = the rounds 1 - 4 backward, kept for A/B: tools/build_variant.py noreorth raster.hip -DLFS_BWD_REORTH=0): the backward
// re-orthogonalises the foot vector against the ray direction before it is used in a gradient - K8's gradients for FLAT Gaussians (tools/aniso_probe.py).
#ifndef LFS_BWD_REORTH
#define LFS_BWD_REORTH 1
#endif
// Host build on the wavefront emulator (tests/emul) only: wave-evaluation counters [fwd, fwd that composited, bwd, bwd that accumulated]
#ifdef LFS_EMULATE
extern "C" { __attribute__((visibility("default"))) unsigned long long lfs_emul_counters[8] = {0, 0, 0, 0, 0, 0, 0, 0}; }
#define LFS_EMUL_COUNT(i) do { if ((threadIdx.x & 63) == 0) ++lfs_emul_counters[i]; } while (0)
// lane utilisation of an accumulated backward evaluation: [4] += live lanes, [5] += 8x4 half cells (rows 0-3 / 4-7) with a live lane, [6] += 4x4 quarters with one
#define LFS_EMUL_LANES(m) do { const unsigned long long m_ = (m); if ((threadIdx.x & 63) == 0) { lfs_emul_counters[4] += __builtin_popcountll(m_); \
    lfs_emul_counters[5] += ((m_ & 0xffffffffull) != 0) + ((m_ >> 32) != 0); \
    for (int q_ = 0; q_ < 4; ++q_) { const unsigned long long qm_ = (0x0f0f0f0full << ((q_ & 1) * 4)) << ((q_ >> 1) * 32); lfs_emul_counters[6] += (m_ & qm_) != 0; } } } while (0)
#else
#define LFS_EMUL_COUNT(i) do { } while (0)
#define LFS_EMUL_LANES(m) do { } while (0)
#endif

namespace lfs {

static inline size_t align256(size_t v) { return (v + 255) & ~size_t(255); }
struct RasterWs { CamDev* cams; GaussRec* recs; float* acc; CullRec* cull; int32_t* cell_count; int2* cell_list; unsigned long long* det64; size_t bytes; };
// cells = C * tiles * (tile_size/8)^2 ; the compacted per-cell lists hold at most (tile_size/8)^2 * n_isects entries
struct RasterWsOffsets { size_t cams, recs, acc, cull, cell_count, cell_list, det64, bytes; };   // byte offsets of the parts above (det64: only in the deterministic mode)
static RasterWsOffsets raster_ws_offsets(uint32_t C, uint32_t N, uint64_t cells, uint64_t cell_entries, bool det) {
    RasterWsOffsets at; size_t o = 0;
    at.cams = o; o += align256(sizeof(CamDev) * C);
    at.recs = o; o += align256(sizeof(GaussRec) * size_t(C) * N);
    at.acc = o; o += align256(sizeof(float) * (ACC_STRIDE * size_t(C) * N + LOSS_SLOTS)); // + the fused-loss partial sums
    at.cull = o; o += align256(sizeof(CullRec) * size_t(C) * N);
    at.cell_count = o; o += align256(sizeof(int32_t) * cells);
    at.cell_list = o; o += align256(sizeof(int2) * cell_entries);
    at.det64 = o;
    if (det) o += align256(sizeof(unsigned long long) * ACC_STRIDE * size_t(C) * N); // deterministic backward (debug bit 4)
    at.bytes = o;
    return at;
}
static RasterWs raster_ws(void* base, const RasterWsOffsets& at, bool det) {
    char* p = (char*)base;
    return RasterWs{(CamDev*)(p + at.cams), (GaussRec*)(p + at.recs), (float*)(p + at.acc), (CullRec*)(p + at.cull), (int32_t*)(p + at.cell_count), (int2*)(p + at.cell_list),
                    det ? (unsigned long long*)(p + at.det64) : nullptr, at.bytes};
}
// a one-camera workspace up to its culling records (camera state, records, accumulator rows): all the finish and tail passes touch. false: `ws` ends before them
static bool rows_ws(const Workspace& ws, uint32_t N, RasterWs& w) {
    const RasterWsOffsets at = raster_ws_offsets(1, N, 0, 0, false);
    w = raster_ws(ws.base, at, false);
    return ws.bytes >= at.cull;
}

__global__ void cam_prep_kernel(const lfs_cameras cams, CamDev* __restrict__ out) {
    for (uint32_t c = threadIdx.x; c < cams.C; c += blockDim.x) {
        CamDev cd;
        cam_init(cd, cams, c);
        out[c] = cd;
    }
}

// ---------------------------------------------------------------------------
// pack
// ---------------------------------------------------------------------------
template <bool UNIFORM_ORIGIN>
__global__ void __launch_bounds__(256) raster_pack_kernel(
    const uint32_t C, const uint32_t N, const uint32_t channels,
    const float* __restrict__ means, const float* __restrict__ quats, const float* __restrict__ scales,
    const float* __restrict__ colors, const float* __restrict__ opacities,
    const CamDev* __restrict__ cams, GaussRec* __restrict__ recs, CullRec* __restrict__ cull) {
    const size_t idx = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (idx >= size_t(C) * N) return;
    const uint32_t cid = uint32_t(idx / N), gid = uint32_t(idx % N);
    const f3 mu{means[3 * gid], means[3 * gid + 1], means[3 * gid + 2]};
    const float4 q = reinterpret_cast<const float4*>(quats)[gid];
    const float sc[3] = {scales[3 * gid], scales[3 * gid + 1], scales[3 * gid + 2]};
    const float* cp = colors + idx * channels;
    GaussRec rec;
    CullRec cr;
    pack_gaussian<UNIFORM_ORIGIN>(cams[cid], mu, q, sc, opacities[idx], cp[0], channels > 1 ? cp[1] : 0.f, channels > 2 ? cp[2] : 0.f, rec, cr);
    recs[idx] = rec;
    cull[idx] = cr;
}

// ---------------------------------------------------------------------------
// cull: per 8x8 cell, compact the tile's depth-sorted list down to the entries that CAN reach the
// 1/255 alpha threshold on at least one of the cell's rays (conservative: never drops a contributor, so
// fwd/bwd results are exactly those of walking the full tile list). Lane = list entry; the cell's box of rays in normalised
// camera coordinates is wave-uniform and tested against the entry's silhouette conic (lfs_cull_conic.cuh). Output per cell: count + (gaussian, list index)
// pairs in list order, stored in the cell's slice of a [cells_per_tile * n_isects] array.
// ---------------------------------------------------------------------------

template <bool UNIFORM_ORIGIN>
__global__ void __launch_bounds__(256) raster_cull_kernel(
    const uint32_t C, const uint32_t tw, const uint32_t th, const uint32_t W, const uint32_t H,
    const uint32_t tile_size, const uint32_t blocks_per_tile, const uint32_t waves_per_block, const uint32_t cull_enabled,
    const CamDev* __restrict__ cams, const CullRec* __restrict__ cull, const uint8_t* __restrict__ masks,
    const int32_t* __restrict__ offsets, const int32_t* __restrict__ ids, const int32_t n_isects,
    int32_t* __restrict__ cell_count, int2* __restrict__ cell_list) {
    // The (up to 4) cells of a workgroup belong to the same tile and walk the same list: the workgroup gathers each
    // batch of 64 * waves entries ONCE (one entry per thread: id + 32-B culling record, a dependent random gather that
    // would otherwise be repeated by every cell and keep the texture-address unit busy) and hands it over through LDS;
    // every wave then tests the whole batch against its own cell. Double-buffered: one barrier per batch.
    __shared__ float4 s_a[2][256], s_b[2][256];
    __shared__ int32_t s_g[2][256];
    const uint32_t n_tiles = tw * th, total_tiles = C * n_tiles;
    const CellCtx cc = cell_ctx(n_tiles, total_tiles, tw, tile_size, blocks_per_tile, waves_per_block);
    if (!cc.in_grid) return; // (uniform per workgroup)
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wpt = (tile_size >> 3) * (tile_size >> 3);
    const size_t cell = size_t(cc.tile_global) * wpt + cc.wl;
    const int32_t start = offsets[cc.tile_global];
    const int32_t end = (cc.tile_global == total_tiles - 1 && n_isects >= 0) ? n_isects : offsets[cc.tile_global + 1]; // n_isects < 0: offsets has T + 1 entries (guarded step)
    const bool tile_masked = masks != nullptr && !masks[cc.tile_global];
    if (tile_masked || end <= start) { // uniform per workgroup
        if (lane == 0) cell_count[cell] = 0;
        return;
    }

    // cell bounds in normalised camera coordinates (x/z, y/z) over the rays that can composite at all
    const CamDev& cam = cams[cc.cid];
    const float big = 3.0e38f;
    bool active = false, behind = false;
    float tu_min = big, tu_max = -big, tv_min = big, tv_max = -big;
    auto probe = [&](uint32_t j, uint32_t i) {
        f3 ro, rd;
        const bool ok = cam_pixel_ray(cam, f2{float(j) + 0.5f, float(i) + 0.5f}, ro, rd);
        const bool act = i < H && j < W && ok;
        active = active || act;
        if (UNIFORM_ORIGIN) {
            const f3 cd = mul_t(cam.Rinv, rd); // back to camera space
            const bool front = cd.z > 0.f;
            behind = behind || (act && !front);
            const float iz = front ? 1.f / cd.z : 0.f;
            const float tu = cd.x * iz, tv = cd.y * iz;
            tu_min = fminf(tu_min, act ? tu : big); tu_max = fmaxf(tu_max, act ? tu : -big);
            tv_min = fminf(tv_min, act ? tv : big); tv_max = fmaxf(tv_max, act ? tv : -big);
        }
    };
    probe(cc.j, cc.i);
    const bool cell_live = __ballot(active) != 0ull; // a dead cell still helps with the loads and the barriers
    bool can_cull = UNIFORM_ORIGIN && cull_enabled != 0;
    float tu_lo = 0.f, tu_hi = 0.f, tv_lo = 0.f, tv_hi = 0.f;
    if (UNIFORM_ORIGIN) {
        can_cull = can_cull && (__ballot(behind) == 0ull);
        const float mu_ = 0.25f / cam.fx, mv_ = 0.25f / cam.fy; // numerical safety margin: a quarter pixel
        tu_lo = wave_min(tu_min) - mu_;
        tu_hi = wave_max(tu_max) + mu_;
        tv_lo = wave_min(tv_min) - mv_;
        tv_hi = wave_max(tv_max) + mv_;
        can_cull = can_cull && (tu_hi - tu_lo < 1e30f) && (tv_hi - tv_lo < 1e30f);
    }
    tu_lo = uniform_f(tu_lo); tu_hi = uniform_f(tu_hi); tv_lo = uniform_f(tv_lo); tv_hi = uniform_f(tv_hi);
    const bool need_recs = UNIFORM_ORIGIN && cull_enabled != 0; // workgroup-uniform (can_cull is per cell)

    int2* __restrict__ out = cell_list + (size_t(wpt) * size_t(start) + size_t(cc.wl) * size_t(end - start));
    int32_t count = 0;
    const int32_t E = int32_t(blockDim.x);          // entries per batch
    const int32_t nsub = E >> 6;                    // = waves in the workgroup
    auto fetch = [&](int32_t base, int32_t& g, CullRec& cr) {
        const int32_t i = base + int32_t(threadIdx.x);
        g = i < end ? ids[i] : 0;
        if (need_recs) cr = cull[g];
    };
    // DEPTH batches are in flight per thread (id load -> dependent record gather: two memory round trips each). 2 and 4 measured: no gain (0.072 -> 0.073 / 0.078 ms on SYN-B) -
    // the kernel is bound by the gather throughput (L2 / texture-address unit), not by the latency of a workgroup's dependent loads. (The loop keeps its DEPTH form: written
    // for one batch without it, the compiler lays the kernel out differently, and this change leaves the measured code as it is.)
    constexpr int DEPTH = 1;
    int32_t g_reg[DEPTH]; CullRec cr_reg[DEPTH];
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) {
        cr_reg[d].a = make_float4(0.f, 0.f, 0.f, 0.f); cr_reg[d].b = cr_reg[d].a; g_reg[d] = 0;
        if (start + d * E < end) fetch(start + d * E, g_reg[d], cr_reg[d]);
    }
    int buf = 0;
    for (int32_t base0 = start; base0 < end; base0 += DEPTH * E) {
#pragma unroll
        for (int d = 0; d < DEPTH; ++d) {
            const int32_t base = base0 + d * E;
            if (base >= end) break; // uniform
            s_g[buf][threadIdx.x] = g_reg[d];
            if (need_recs) { s_a[buf][threadIdx.x] = cr_reg[d].a; s_b[buf][threadIdx.x] = cr_reg[d].b; }
            __syncthreads();
            if (base + DEPTH * E < end) fetch(base + DEPTH * E, g_reg[d], cr_reg[d]); // in flight during the tests below
            if (cell_live) {
                for (int32_t sub = 0; sub < nsub; ++sub) {
                    const int32_t slot = (sub << 6) + int32_t(lane);
                    const int32_t my_idx = base + slot;
                    if (base + (sub << 6) >= end) break; // uniform
                    const bool valid = my_idx < end;
                    const int32_t my_g = s_g[buf][slot];
                    bool hit = valid;
                    if (can_cull) {
                        const float4 a = s_a[buf][slot], b = s_b[buf][slot];
                        hit = valid && !conic_culled(ConicRec{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}, tu_lo, tu_hi, tv_lo, tv_hi);
                    }
                    const uint64_t m = __ballot(hit);
                    if (hit) {
                        const uint32_t rank = __builtin_amdgcn_mbcnt_hi(uint32_t(m >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m), 0u));
                        out[count + int32_t(rank)] = make_int2(my_g, my_idx);
                    }
                    count += __popcll(m);
                }
            }
            buf ^= 1;
        }
    }
    if (lane == 0) cell_count[cell] = count;
}

// Ray modes (template parameter of fwd / bwd):
//   0 rolling shutter : world-space ray (ro, rd) per pixel, record = {M, mu}
//   1 global shutter  : camera-space direction d (any camera model), record = {M Rinv, M (o - mu)}
// (A third mode with d = (u, v, 1) for pinholes was tried: the three multiplications it saves come back as v_mov,
//  because a VOP3 instruction on gfx9 can read only one SGPR and fma(M01, v, M02) needs two.)
constexpr int RAY_ROLLING = 0, RAY_GLOBAL = 1;

// Distance of the Gaussian centre to the ray line in the Gaussian's normalised frame. With q = M d (un-normalised),
// t = (gro . q) / |q|^2 and the foot vector w = gro - t q:  |w| equals the reference's |normalize(q) x gro|, and the
// backward collapses to dL/dgro = -s w, dL/dq = t s w (s = vis * dL/dvis): no normalisation, no cross products.
struct RayEval { f3 om, w, q; float t, vis, rl; }; // w = c w_true and `vis` is alpha_raw = opac * vis_true (see lfs_raster_common.cuh)
template <int MODE>
LFS_DI void ray_eval(const GaussRec& rec, const f3& ro, const f3& d, RayEval& e) {
    e.om = {0.f, 0.f, 0.f};
#if LFS_REC_ROT
    if (MODE == RAY_GLOBAL) { // the record lives in the frame in which g = (0, 0, G) (lfs_raster_common.cuh, LFS_REC_ROT): |w|^2 = G^2 m / l, no difference of large numbers anywhere
        const f3 q{fma3(rec.r0.x, d.x, rec.r0.y, d.y, rec.r0.z, d.z),
                   fma3(rec.r1.x, d.x, rec.r1.y, d.y, rec.r1.z, d.z),
                   fma3(rec.r2.x, d.x, rec.r2.y, d.y, rec.r2.z, d.z)};
        const float rec_k = rec.r0.w;
        const float m = __builtin_fmaf(q.y, q.y, q.x * q.x);
        const float l = __builtin_fmaf(q.z, q.z, m);
        const float rl = fast_rcp(l);      // l == 0 (inactive lane: d = 0; degenerate record): inf, and m = q.z = 0 - the two products below are v_mul_legacy_f32 (0 * inf = 0): u = 0, t = 0, w = 0
        const float u = mul_zero(m, rl);   // sin^2 of the angle between the ray and the direction to the centre
        e.vis = __builtin_amdgcn_exp2f(__builtin_fmaf(-rec_k, u, rec.r3.x));
        e.t = rec.r2.w * mul_zero(q.z, rl);
#ifndef LFS_EMULATE
        asm volatile("" ::"s"(rec.r1.w), "s"(rec.r2.w)); // (no instruction: the unused fields of the record - r1.w, and G in the forward - stay "used", so the record still arrives as ONE s_load_dwordx16; without it the compiler splits the load into two to four)
#endif
        e.q = q; e.rl = rl;
        e.w = {-e.t * q.x, -e.t * q.y, rec.r2.w * u};
        return;
    }
#endif
    f3 gro;
    if (MODE != RAY_ROLLING) gro = {rec.r0.w, rec.r1.w, rec.r2.w};
    else {
        e.om = {ro.x - rec.r0.w, ro.y - rec.r1.w, ro.z - rec.r2.w};
        gro = {fma3(rec.r0.x, e.om.x, rec.r0.y, e.om.y, rec.r0.z, e.om.z),
               fma3(rec.r1.x, e.om.x, rec.r1.y, e.om.y, rec.r1.z, e.om.z),
               fma3(rec.r2.x, e.om.x, rec.r2.y, e.om.y, rec.r2.z, e.om.z)};
    }
    const f3 q{fma3(rec.r0.x, d.x, rec.r0.y, d.y, rec.r0.z, d.z),
               fma3(rec.r1.x, d.x, rec.r1.y, d.y, rec.r1.z, d.z),
               fma3(rec.r2.x, d.x, rec.r2.y, d.y, rec.r2.z, d.z)};
    const float l = fma3(q.x, q.x, q.y, q.y, q.z, q.z);
    // l == 0 (inactive lane: d = 0; degenerate record: M = 0): q = 0 as well, so t = 0 * FLT_MAX = 0 and w = gro - one v_min instead of compare + select
    const float rl = fminf(fast_rcp(l), 3.402823466e38f);
    e.t = fma3(gro.x, q.x, gro.y, q.y, gro.z, q.z) * rl;
    e.q = q; e.rl = rl;
    e.w = {__builtin_fmaf(-e.t, q.x, gro.x), __builtin_fmaf(-e.t, q.y, gro.y), __builtin_fmaf(-e.t, q.z, gro.z)};
    e.vis = __builtin_amdgcn_exp2f(__builtin_fmaf(-e.w.z, e.w.z, __builtin_fmaf(-e.w.y, e.w.y, __builtin_fmaf(-e.w.x, e.w.x, rec.r3.x))));
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
// this lane's ray in the form the mode wants; false when the pixel has no ray
template <int MODE>
LFS_DI bool lane_ray(const CamDev& cam, const uint32_t j, const uint32_t i, f3& ro, f3& d) {
    const f2 ip{float(j) + 0.5f, float(i) + 0.5f};
    if (MODE == RAY_ROLLING) return cam_pixel_ray(cam, ip, ro, d);
    ro = cam.origin;
    f3 cd;
    const bool ok = cam_unproject(cam, ip, cd);
    d = ok ? cd : f3{0.f, 0.f, 0.f};
    return ok;
}

template <int CDIM, int MODE>
__global__ void __launch_bounds__(256) raster_fwd_kernel(
    const uint32_t C, const uint32_t N, const uint32_t tw, const uint32_t th, const uint32_t W, const uint32_t H,
    const uint32_t tile_size, const uint32_t blocks_per_tile, const uint32_t waves_per_block,
    const CamDev* __restrict__ cams, const GaussRec* __restrict__ recs, const float* __restrict__ colors,
    const float* __restrict__ backgrounds, const uint8_t* __restrict__ masks,
    const int32_t* __restrict__ offsets, const int32_t* __restrict__ cell_count, const int2* __restrict__ cell_list, const int32_t n_isects,
    float* __restrict__ render_colors, float* __restrict__ render_alphas, int32_t* __restrict__ last_ids,
    int32_t* __restrict__ /* unused since the forward's entry marks were removed; dropping it changes the kernel's signature: left for the next change of this kernel */) {
    const uint32_t n_tiles = tw * th, total_tiles = C * n_tiles;
    const CellCtx cc = cell_ctx(n_tiles, total_tiles, tw, tile_size, blocks_per_tile, waves_per_block);
    if (!cc.in_grid) return;
    const uint32_t cid = cc.cid;
    const bool inside = cc.i < H && cc.j < W;
    const size_t pix_id = (size_t(cid) * H + cc.i) * W + cc.j;
    const float* bg = backgrounds ? backgrounds + cid * CDIM : nullptr;

    if (masks != nullptr && !masks[cc.tile_global]) { // Fwd.cu:141-150 (alpha / last id written as 0 instead of left undefined)
        if (inside) {
#pragma unroll
            for (int k = 0; k < CDIM; ++k) render_colors[pix_id * CDIM + k] = bg ? bg[k] : 0.f;
            render_alphas[pix_id] = 0.f;
            last_ids[pix_id] = 0;
        }
        return;
    }

    const CamDev& cam = cams[cid];
    f3 ro, rd;
    const bool ray_ok = lane_ray<MODE>(cam, cc.j, cc.i, ro, rd);
    // "done" is carried as the lane's alpha threshold: 1/255 while the pixel is live, +inf once it has terminated (or never
    // had a ray). One compare then answers both "not done" and "alpha >= 1/255", and the per-lane state stays out of the
    // boolean VGPR juggling the compiler otherwise emits for a loop-carried bool (6 VALU per evaluation, measured in the ISA).
    const float INF = __builtin_inff();
    float thr = (inside && ray_ok) ? (1.f / 255.f) : INF;

    const uint32_t wpt = (tile_size >> 3) * (tile_size >> 3);
    const int32_t start = offsets[cc.tile_global];
    const int32_t end = (cc.tile_global == total_tiles - 1 && n_isects >= 0) ? n_isects : offsets[cc.tile_global + 1]; // n_isects < 0: offsets has T + 1 entries (guarded step)
    const int2* __restrict__ cl = cell_list + (size_t(wpt) * size_t(start) + size_t(cc.wl) * size_t(end - start));
    const int32_t cnt = cell_count[size_t(cc.tile_global) * wpt + cc.wl];
    // (Measured and removed: the forward marking the entries nothing composited, for the backward to skip - raster_fwd 0.233 -> 0.256 ms, raster_bwd 0.4856 -> 0.4845 ms,
    // 734 -> 722 img/s: profiles/r06/lease18_fwd_marks_projfast_ab.txt.)

    float T = 1.f;
    float pix[CDIM];
#pragma unroll
    for (int k = 0; k < CDIM; ++k) pix[k] = 0.f;
    int32_t cur_idx = 0;

    // One evaluation of a record against this lane's ray (wave-uniform record in SGPRs).
    auto eval = [&](const GaussRec& rec, const int2 e) {
        RayEval re;
        ray_eval<MODE>(rec, ro, rd, re);
        const float alpha = fminf(0.999f, re.vis);
        const bool pass = !(alpha < thr); // live pixel and alpha >= 1/255 (a NaN alpha passes, as in the reference's `if (alpha < 1/255) continue`)
        LFS_EMUL_COUNT(0);
        if (__ballot(pass) == 0ull) return;
        LFS_EMUL_COUNT(1);
        const float next_T = T * (1.f - alpha);
        const bool fin = pass && next_T <= 1e-4f; // the terminating Gaussian is not composited
        const bool contrib = pass && !fin;
        const float vis = alpha * T;
        if (contrib) {
            if (CDIM <= 3) {
                pix[0] = __builtin_fmaf(rec.r3.y, vis, pix[0]);
                if (CDIM > 1) pix[1] = __builtin_fmaf(rec.r3.z, vis, pix[1]);
                if (CDIM > 2) pix[2] = __builtin_fmaf(rec.r3.w, vis, pix[2]);
            } else {
                const float* cp = colors + size_t(e.x) * CDIM;
#pragma unroll
                for (int k = 0; k < CDIM; ++k) pix[k] = __builtin_fmaf(cp[k], vis, pix[k]);
            }
            cur_idx = e.y;
            T = next_T;
        }
        thr = fin ? INF : thr;
    };
    walk_cell_list<1>(cl, recs, 0, cnt, eval, [&]() { return __ballot(thr < INF) != 0ull; });

    if (inside) {
        render_alphas[pix_id] = 1.f - T;
#pragma unroll
        for (int k = 0; k < CDIM; ++k) render_colors[pix_id * CDIM + k] = bg ? pix[k] + T * bg[k] : pix[k];
        last_ids[pix_id] = cur_idx;
    }
}

// ---------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------
// Optional fused loss (extension, CDIM = 3, one camera): the kernel derives dL/d(render) = d/d(render) of
// weight * mean((clamp(render, 0, 1) - target)^2) from the forward image and the CHW target itself and adds the loss to *loss -
// the arithmetic of l2_fused.hip's mse_loss_kernel per pixel, so v_render_colors is never materialised and the loss kernel's
// pass over the image disappears.
struct MseFuse { const float* render; const float* target; float scale; float* loss; unsigned long long* det64; };

template <int CDIM, int MODE, bool LOSS = false, int ACC = 0>
__global__ void __launch_bounds__(256) raster_bwd_kernel(
    const uint32_t C, const uint32_t N, const uint32_t tw, const uint32_t th, const uint32_t W, const uint32_t H,
    const uint32_t tile_size, const uint32_t blocks_per_tile, const uint32_t waves_per_block,
    const CamDev* __restrict__ cams, const GaussRec* __restrict__ recs, const float* __restrict__ colors,
    const float* __restrict__ backgrounds, const uint8_t* __restrict__ masks,
    const int32_t* __restrict__ offsets, const int32_t* __restrict__ cell_count, const int2* __restrict__ cell_list, const int32_t n_isects,
    const float* __restrict__ render_alphas, const int32_t* __restrict__ last_ids,
    const float* __restrict__ v_render_colors, const float* __restrict__ v_render_alphas,
    float* __restrict__ acc, float* __restrict__ v_colors_extra, const MseFuse mse = MseFuse{}) {
    const uint32_t n_tiles = tw * th, total_tiles = C * n_tiles;
    constexpr int RED_BLOCK = (LFS_RED_QUAD_ASM && RED_QUAD_SCRATCH_FLOATS > RED_SCRATCH_FLOATS) ? RED_QUAD_SCRATCH_FLOATS : RED_SCRATCH_FLOATS;
    __shared__ __attribute__((aligned(16))) float s_red[RED_BLOCK]; // the wavefront's transpose block (wave_sum16_atomic_lds / _quad; one wavefront per workgroup: wave_geom)
    float* const red_scratch = s_red + (threadIdx.x >> 6) * RED_BLOCK;
#if LFS_RED_QUAD_ASM
    const uint32_t red_base = __builtin_amdgcn_readfirstlane(uint32_t(reinterpret_cast<uintptr_t>(red_scratch)));   // LDS byte address of the block (low half of the flat address)
    asm volatile("s_mov_b32 m0, %0" ::"s"(red_base));   // the one write of M0 in this kernel (lfs_raster_common.cuh, wave_sum16_atomic_quad)
    const float4* const red_rd = reinterpret_cast<const float4*>(red_scratch + ((threadIdx.x & 63u) >> 2) * RED_QROW + 4u * (threadIdx.x & 3u));
    constexpr bool RED_SKIP = LFS_ACC_SYM && MODE == RAY_GLOBAL && CDIM == 3;   // (slots 9 .. 11 of the LFS_ACC_SYM row are empty)
    const bool red_atomic_lane = (threadIdx.x & 3u) == 0u && !(RED_SKIP && ((threadIdx.x & 63u) >> 2) >= 9u && ((threadIdx.x & 63u) >> 2) <= 11u);
    const RedBuf red_buf = red_buf_make(acc, uint64_t(C) * N, threadIdx.x & 63u, red_atomic_lane);   // (ACC == 0: the totals leave through a buffer atomic, lfs_raster_common.cuh)
#endif
    const CellCtx cc = cell_ctx(n_tiles, total_tiles, tw, tile_size, blocks_per_tile, waves_per_block);
    if (!cc.in_grid) return;
    const uint32_t cid = cc.cid;
    if (masks != nullptr && !masks[cc.tile_global]) return; // masked tiles composited nothing
    const uint32_t lane = threadIdx.x & 63;
    const bool inside = cc.i < H && cc.j < W;
    const size_t pix_id = (size_t(cid) * H + cc.i) * W + cc.j;
    const float* bg = backgrounds ? backgrounds + cid * CDIM : nullptr;

    const CamDev& cam = cams[cid];
    f3 ro, rd;
    const bool ray_ok = lane_ray<MODE>(cam, cc.j, cc.i, ro, rd);
    const bool active = inside && ray_ok;

    const uint32_t wpt = (tile_size >> 3) * (tile_size >> 3);
    const int32_t start = offsets[cc.tile_global];
    const int32_t end = (cc.tile_global == total_tiles - 1 && n_isects >= 0) ? n_isects : offsets[cc.tile_global + 1]; // n_isects < 0: offsets has T + 1 entries (guarded step)
    const int2* __restrict__ cl = cell_list + (size_t(wpt) * size_t(start) + size_t(cc.wl) * size_t(end - start));
    const int32_t cnt = cell_count[size_t(cc.tile_global) * wpt + cc.wl];

    float T_final = 1.f, v_ra = 0.f;
    int32_t bin_final = -1; // Bwd.cu:183 uses 0 for inactive pixels; -1 keeps them out of entry 0 as well
    float vc[CDIM];
#pragma unroll
    for (int k = 0; k < CDIM; ++k) vc[k] = 0.f;
    if (active) {
        T_final = 1.f - render_alphas[pix_id];
        bin_final = last_ids[pix_id];
        v_ra = v_render_alphas ? v_render_alphas[pix_id] : 0.f;
        if (!LOSS) {
#pragma unroll
            for (int k = 0; k < CDIM; ++k) vc[k] = v_render_colors[pix_id * CDIM + k];
        }
    }
    if (LOSS) { // every pixel of the image belongs to exactly one lane of one wavefront
        float lsum = 0.f;
        if (inside) {
            const size_t P = size_t(H) * W;
#pragma unroll
            for (int k = 0; k < CDIM; ++k) {
                const float x = mse.render[pix_id * CDIM + k];
                const float d = fminf(fmaxf(x, 0.f), 1.f) - mse.target[size_t(k) * P + pix_id];
                lsum += d * d;
                const float g = (x >= 0.f && x <= 1.f) ? 2.f * d * mse.scale : 0.f;
                if (active) vc[k] = g;
            }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) lsum += __shfl_xor(lsum, m, 64);
        if (ACC != 1 && lane == 0 && lsum != 0.f) unsafeAtomicAdd(mse.loss + ((blockIdx.x * 4u + (threadIdx.x >> 6)) & (LOSS_SLOTS - 1)), lsum * mse.scale);
    }
    float T = T_final;
    // T_final * (v_alpha_out - bg . v_color_out): the transmittance-tail term of d/d(alpha)
    float tail = v_ra;
    if (bg) {
        float bd = 0.f;
#pragma unroll
        for (int k = 0; k < CDIM; ++k) bd += bg[k] * vc[k];
        tail -= bd;
    }
    tail *= T_final;

    // wave max of bin_final (uniform): nothing behind it can matter for this cell
    int32_t wmax = bin_final;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) wmax = max(wmax, __shfl_xor(wmax, m, 64));
    wmax = __builtin_amdgcn_readfirstlane(wmax);
    // number of cell-list entries whose list index is <= wmax (entries are in ascending list order)
    int32_t lo = 0, hi = cnt;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (cl[mid].y <= wmax) lo = mid + 1; else hi = mid;
    }
    const int32_t n_walk = lo;
    if (n_walk <= 0) return;

    auto eval = [&](const GaussRec& rec, const int2 e) {
        RayEval re;
        ray_eval<MODE>(rec, ro, rd, re);
#if LFS_BWD_REORTH
        if (!(LFS_REC_ROT && MODE == RAY_GLOBAL)) // (the rotated records of LFS_REC_ROT form w without a difference: nothing to take out)
        {   // w = gro - t q is the difference of two vectors of length |o - mu| / s_min: for a FLAT Gaussian (one scale 20 - 100 x below the others, 5 units away: 1e4) its
            // component ALONG q carries an absolute rounding error of ulp(1e4) ~ 1e-3 - harmless in |w|^2 (alpha above is computed from the un-corrected w, bit-identical
            // to the forward), but dL/dgro = -s w is multiplied by 1 / s_min again in the finish pass. w is orthogonal to q by construction: one Gram-Schmidt step takes
            // the spurious component out (w . q is a product with the LARGE q, so it is resolved exactly where the error sits). tools/aniso_probe.py.
            const float c = fma3(re.w.x, re.q.x, re.w.y, re.q.y, re.w.z, re.q.z) * re.rl;
            re.w = {__builtin_fmaf(-c, re.q.x, re.w.x), __builtin_fmaf(-c, re.q.y, re.w.y), __builtin_fmaf(-c, re.q.z, re.w.z)};
        }
#endif
        const float araw = re.vis;
        const float alpha = fminf(0.999f, araw);
        LFS_EMUL_COUNT(2);
        const bool valid = e.y <= bin_final && !(alpha < (1.f / 255.f)); // (inactive lanes carry bin_final = -1; vis > 1 cannot happen)
        if (__ballot(valid) == 0ull) return;
        LFS_EMUL_COUNT(3);
        LFS_EMUL_LANES(__ballot(valid));

        // Invalid lanes are masked by zeroing three scalars (fac, v_op, and through it s): every reduced value below is
        // a product with one of them. (All factors are finite for an inactive lane: its direction is 0, so w = gro, t = 0.)
        // (round 6: -2 VALU per evaluation) an invalid lane takes part with alpha = 0: 1 / (1 - 0) = 1 exactly (v_rcp_f32 is exact at 1: tests/test_gpu_raster.py), so its T is multiplied by 1 and its
        // fac is 0 * T - one select instead of the two on T and fac
        const float alpha_v = valid ? alpha : 0.f;
        const float ra = fast_rcp(1.f - alpha_v);
        const float Tn = T * ra;
        T = Tn;
        const float fac = alpha_v * Tn;
        float v[16], v_extra = 0.f, cv;
        if (CDIM <= 3) {
            cv = rec.r3.y * vc[0];
            if (CDIM > 1) cv = __builtin_fmaf(rec.r3.z, vc[1], cv);
            if (CDIM > 2) cv = __builtin_fmaf(rec.r3.w, vc[2], cv);
        } else {
            const float* cp = colors + size_t(e.x) * CDIM;
            cv = cp[0] * vc[0];
#pragma unroll
            for (int k = 1; k < CDIM; ++k) cv = __builtin_fmaf(cp[k], vc[k], cv);
        }
        // dL/dalpha = (tail - B) / (1 - alpha) + T (c . v_c), B = sum over the entries behind of fac_j (c_j . v_c)
        const float v_alpha = __builtin_fmaf(ra, tail, Tn * cv);   // `tail` carries tail - B: one fma per entry instead of a subtraction and an fma
        tail = __builtin_fmaf(-fac, cv, tail);
#pragma unroll
        for (int k = 0; k < CDIM; ++k) {
            const float vrgb = fac * vc[k];
            if (k < 3) v[13 + k] = vrgb; else v_extra = vrgb;
        }
#pragma unroll
        for (int k = CDIM; k < 3; ++k) v[13 + k] = 0.f;
        // through alpha = min(0.999, opac * vis): no gradient on the clamped side
        const float sgeo = (valid && araw <= 0.999f) ? araw * v_alpha : 0.f; // s = alpha_raw * dL/dalpha = opac * dL/dopacity = vis * dL/dvis
        const float v_op = sgeo;                                            // (slot 12 holds opac * dL/dopacity: the finish kernels divide)
        v[12] = v_op;
        if (CDIM == 3 && MODE == RAY_GLOBAL) { // the 18 products on register PAIRS (v_pk_mul_f32): -12 VALU per evaluation, bit-identical sums; 0.621 - 0.631 -> 0.611 - 0.617 ms (same box, 3 pairs)
            v2f V[8];
#if LFS_ACC_SYM
            // B'' = a (x) w (symmetric: six products) and a = s w - lfs_raster_common.cuh, LFS_ACC_SYM. Slots: xx, yy | xz, yz | xy, zz | ax, ay | az
            const v2f wxy = v2f{re.w.x, re.w.y};
            const v2f axy = wxy * sgeo;
            const float az = re.w.z * sgeo;
            V[0] = axy * wxy;
            V[1] = axy * re.w.z;
            V[2] = v2f{axy.x * wxy.y, az * re.w.z};
            V[3] = axy;
            V[4] = v2f{az, 0.f};
            V[5] = v2f{0.f, 0.f};
#elif LFS_REC_ROT
            // w = (-t q.x, -t q.y, G u): a = s w straight from q (one packed product for the two components that are multiples of q)
            // Slots 9 .. 11 of the row hold (a.z, a.x, a.y) in this form - the pair (a.x, a.y) is used as it comes out of the packed product; finish_geometry puts them back.
            const float nst = -(sgeo * re.t);
            const v2f axy = v2f{re.q.x, re.q.y} * nst;
            const float az = re.w.z * sgeo;
            const v2f vgxy = axy * re.t;
            const float vgz = az * re.t;
            V[0] = v2f{rd.x, rd.y} * vgxy.x;
            V[1] = v2f{vgxy.x * rd.z, vgxy.y * rd.x};
            V[2] = v2f{rd.y, rd.z} * vgxy.y;
            V[3] = v2f{rd.x, rd.y} * vgz;
            V[4] = v2f{vgz * rd.z, az};
            V[5] = axy;
#else
            const float ax = re.w.x * sgeo;
            const v2f ayz = v2f{re.w.y, re.w.z} * sgeo;
            const float vgx = ax * re.t;
            const v2f vgyz = ayz * re.t;
            V[0] = v2f{rd.x, rd.y} * vgx;
            V[1] = v2f{vgx * rd.z, vgyz.x * rd.x};
            V[2] = v2f{rd.y, rd.z} * vgyz.x;
            V[3] = v2f{rd.x, rd.y} * vgyz.y;
            V[4] = v2f{vgyz.y * rd.z, ax};
            V[5] = ayz;
#endif
            V[6] = v2f{v_op, fac * vc[0]};
            V[7] = v2f{vc[1], vc[2]} * fac;
#if LFS_RED_QUAD_ASM
            wave_sum16_atomic_quad<ACC, RED_SKIP>(V, acc + size_t(uint32_t(e.x)) * ACC_STRIDE, lane, red_base, red_rd, red_atomic_lane, ACC == 2 ? mse.det64 + size_t(e.x) * ACC_STRIDE : nullptr,
                                                  &red_buf, uint32_t(e.x) << 6);
#else
            wave_sum16_atomic_lds<ACC>(V, acc + size_t(e.x) * ACC_STRIDE, lane, red_scratch, ACC == 2 ? mse.det64 + size_t(e.x) * ACC_STRIDE : nullptr);
#endif
            return;
        }
        const f3 a = re.w * sgeo;                                           // = -dL/dgro (the sign is undone in raster_finish_kernel)
        if (LFS_ACC_SYM && MODE == RAY_GLOBAL) { // the symmetric row (see the packed form above): B'' xx, yy, xz, yz, xy, zz | a | - - -
            v[0] = a.x * re.w.x; v[1] = a.y * re.w.y; v[2] = a.x * re.w.z; v[3] = a.y * re.w.z; v[4] = a.x * re.w.y; v[5] = a.z * re.w.z;
            v[6] = a.x; v[7] = a.y; v[8] = a.z; v[9] = 0.f; v[10] = 0.f; v[11] = 0.f;
            wave_sum16_atomic<ACC>(v, acc + size_t(e.x) * ACC_STRIDE, lane, ACC == 2 ? mse.det64 + size_t(e.x) * ACC_STRIDE : nullptr);
            if (CDIM > 3) {
#pragma unroll
                for (int m = 32; m >= 1; m >>= 1) v_extra += __shfl_xor(v_extra, m, 64);
                if (lane == 0) unsafeAtomicAdd(v_colors_extra + size_t(e.x) * CDIM + 3, v_extra);
            }
            return;
        }
        const f3 vg = a * re.t;                                             // dL/dq, q = (record matrix) d
        // dL/d(record matrix) = vg (x) d  [- a (x) (o - mu) per pixel only when the origin varies]
        v[0] = vg.x * rd.x; v[1] = vg.x * rd.y; v[2] = vg.x * rd.z;
        v[3] = vg.y * rd.x; v[4] = vg.y * rd.y; v[5] = vg.y * rd.z;
        v[6] = vg.z * rd.x; v[7] = vg.z * rd.y; v[8] = vg.z * rd.z;
        if (MODE == RAY_ROLLING) {
            const f3& om = re.om;
            v[0] -= a.x * om.x; v[1] -= a.x * om.y; v[2] -= a.x * om.z;
            v[3] -= a.y * om.x; v[4] -= a.y * om.y; v[5] -= a.y * om.z;
            v[6] -= a.z * om.x; v[7] -= a.z * om.y; v[8] -= a.z * om.z;
        }
        if (LFS_REC_ROT && MODE == RAY_GLOBAL) { v[9] = a.z; v[10] = a.x; v[11] = a.y; } // (the slot order of the rotated records: see the packed form above)
        else { v[9] = a.x; v[10] = a.y; v[11] = a.z; }
        wave_sum16_atomic<ACC>(v, acc + size_t(e.x) * ACC_STRIDE, lane, ACC == 2 ? mse.det64 + size_t(e.x) * ACC_STRIDE : nullptr);
        if (CDIM > 3) {
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) v_extra += __shfl_xor(v_extra, m, 64);
            if (lane == 0) unsafeAtomicAdd(v_colors_extra + size_t(e.x) * CDIM + 3, v_extra);
        }
    };
    walk_cell_list<-1>(cl, recs, n_walk - 1, n_walk, eval, []() { return true; });
}

// ---------------------------------------------------------------------------
// finish: accumulator -> dL/d(means, quats, scales, colors, opacities)
// ---------------------------------------------------------------------------
template <bool UNIFORM_ORIGIN>
__global__ void __launch_bounds__(256) raster_finish_kernel(
    const uint32_t C, const uint32_t N, const uint32_t channels,
    const float* __restrict__ means, const float* __restrict__ quats, const float* __restrict__ scales,
    const CamDev* __restrict__ cams, const float* __restrict__ acc,
    float* __restrict__ v_means, float* __restrict__ v_quats, float* __restrict__ v_scales,
    float* __restrict__ v_colors, float* __restrict__ v_opacities, const float* __restrict__ loss_slots, float* __restrict__ loss,
    const float* __restrict__ opacities) {
    if (loss_slots != nullptr && blockIdx.x == 0) { // fused MSE: fold the backward kernel's partial sums into the caller's accumulator
        float v = threadIdx.x < LOSS_SLOTS ? loss_slots[threadIdx.x] : 0.f;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
        if ((threadIdx.x & 63) == 0 && v != 0.f) unsafeAtomicAdd(loss, v);
    }
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= N) return;
    float vm[3] = {0.f, 0.f, 0.f}, vq[4] = {0.f, 0.f, 0.f, 0.f}, vs[3] = {0.f, 0.f, 0.f};
    bool geom_loaded = false;
    f3 mu{0.f, 0.f, 0.f}; float4 q = make_float4(1.f, 0.f, 0.f, 0.f); float is[3] = {0.f, 0.f, 0.f};
    for (uint32_t cid = 0; cid < C; ++cid) {
        const size_t idx = size_t(cid) * N + gid;
        const float4* a4 = reinterpret_cast<const float4*>(acc + idx * ACC_STRIDE);
        float4 a0 = a4[0], a1 = a4[1], a2 = a4[2], a3 = a4[3];
        { // the row was accumulated against the scaled record (lfs_raster_common.cuh): A' = c A, G' = c G, slot 12 = opac * dL/dopac
            a0.x *= REC_UNSCALE; a0.y *= REC_UNSCALE; a0.z *= REC_UNSCALE; a0.w *= REC_UNSCALE; a1.x *= REC_UNSCALE; a1.y *= REC_UNSCALE; a1.z *= REC_UNSCALE;
            a1.w *= REC_UNSCALE; a2.x *= REC_UNSCALE; a2.y *= REC_UNSCALE; a2.z *= REC_UNSCALE; a2.w *= REC_UNSCALE;
            const float op = opacities[idx];
            a3.x = a3.x != 0.f ? a3.x / op : 0.f;
        }
        v_opacities[idx] = a3.x;
        float* vcol = v_colors + idx * channels;
        vcol[0] = a3.y;
        if (channels > 1) vcol[1] = a3.z;
        if (channels > 2) vcol[2] = a3.w;
        // (channel 3, when present, was accumulated straight into v_colors by the bwd kernel)
        const float A[9] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w, a2.x};
        const f3 G{-a2.y, -a2.z, -a2.w}; // the bwd kernel accumulates -dL/dgro
        bool any = G.x != 0.f || G.y != 0.f || G.z != 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k) any |= A[k] != 0.f;
        if (!any) continue;
        if (!geom_loaded) {
            mu = {means[3 * gid], means[3 * gid + 1], means[3 * gid + 2]};
            q = reinterpret_cast<const float4*>(quats)[gid];
            is[0] = 1.f / scales[3 * gid]; is[1] = 1.f / scales[3 * gid + 1]; is[2] = 1.f / scales[3 * gid + 2];
            geom_loaded = true;
        }
        finish_geometry<UNIFORM_ORIGIN>(q, is, A, G, mu, cams[cid], vm, vq, vs);
    }
    v_means[3 * gid] = vm[0]; v_means[3 * gid + 1] = vm[1]; v_means[3 * gid + 2] = vm[2];
    reinterpret_cast<float4*>(v_quats)[gid] = make_float4(vq[0], vq[1], vq[2], vq[3]);
    v_scales[3 * gid] = vs[0]; v_scales[3 * gid + 1] = vs[1]; v_scales[3 * gid + 2] = vs[2];
}

template <bool ADAM>
__global__ void __launch_bounds__(FINISH_BLOCK) raster_finish_adam_kernel(
    const uint32_t N, float* __restrict__ means, float* __restrict__ raw_scales, float* __restrict__ raw_quats, float* __restrict__ raw_opacities,
    const float* __restrict__ quats, const float* __restrict__ scales, const float* __restrict__ opacities,
    const CamDev* __restrict__ cams, const float* __restrict__ acc, const float* __restrict__ v_dirs, const FinishAdam ad, const FinishGrads gr,
    const float* __restrict__ loss_slots, float* __restrict__ loss, const int32_t* __restrict__ abort_flag = nullptr) {
    constexpr bool DENSIFY = false;   // (the densifying form: raster_densify.hip)
    constexpr const int32_t* radii = nullptr; constexpr float* dens = nullptr;
#include "lfs_raster_finish_body.cuh"
}

// ---------------------------------------------------------------------------
// The TAIL of the all-inline training step in ONE pass over the Gaussians (round 6): SH backward + Adam(sh0, shN) + finish + activation backward +
// Adam(means, scales, quaternions, opacities) + - when the caller names the NEXT view - the SH colours of the next step. Replaces three launches of the one-call step
// (sh_bwd_kernel<.., ADAM>, raster_finish_adam_kernel<true>, next step's sh_fwd_kernel):
//   * dL/d(dirs) goes from the SH backward to the means update in registers (was: 12 B written + read per Gaussian);
//   * the next view's colours are evaluated from the coefficient rows while they sit in registers for their Adam update (was: sh_fwd re-reads 192 B per Gaussian, 65 us);
//   * the pass that follows the 1.1 GB read-modify-write of the SH Adam update no longer exists (finish_adam ran at 3.2 - 3.5 TB/s behind it, 5.9 alone: the dirty lines
//     of the update were still draining - profiles/r06/stream_kernels_alone_1M.json).
// One wavefront per 64 Gaussians, five phases (__syncthreads between them; LDS: basis rows, a second row block, the masked colour gradient):
//   1  lane = Gaussian          : direction of THIS view, visibility, basis -> lds_b; dL/dcolour (accumulator slots 13..15) under the clamp mask -> ldv; the finish pass's
//                                 operands are requested here and land under phase 2
//   2  lane = (Gaussian, basis) : s_k = coefficient row . dL/dcolour -> lds_s (rows of Gaussians without a colour gradient are not fetched)
//   3  lane = Gaussian          : dL/d(dirs) = sum_k s_k grad b_k; then exactly raster_finish_adam_kernel<true>'s arithmetic with it; the updated mean stays in registers
//   4  lane = Gaussian          : direction of the NEXT view from the updated mean, its basis -> lds_s
//   5  lane = (Gaussian, basis) : coefficient row + moments -> Adam -> stored; next colour = sum_k (new basis)_k x (updated row) -> colors (clamped as sh_fwd_kernel)
// The SH arithmetic is pinned contraction-free (lfs_sh.cuh and the blocks below) as in sh.hip; the finish arithmetic is raster_finish_adam_kernel's, statement by statement:
// parameters and moments come out bit-identical to the three kernels (tests/test_gpu_gut_step.py, tests/test_emulated_step_pack.py).
struct GutTail {
    uint32_t N, K; int degree;
    float *means, *sh0, *shN, *raw_scales, *raw_quats, *raw_opacities;
    const float* viewmat; const float* next_viewmat;   // next_viewmat: NULL = no colours for the next step
    const int32_t* radii; float* colors;             // in: this step's colours (clamp mask); out (next_viewmat given): the next step's, for EVERY Gaussian
    const float* acc;
    float *m0, *v0, *mN, *vN; AdamScalars s0, sN;    // sh0 / shN moments
    FinishAdam fin;
    const float* loss_slots; float* loss; const int32_t* abort_flag;
    const float* noise; float noise_lr;               // NOISE: the MCMC strategy's normal deviates [N,3] and its current_lr (lfs_add_noise's operands)
};
// Phase 5 of gut_tail_kernel: the coefficient rows phase 2 fetches stay in registers for it (KEEP: same lane, same rows - 3 x LPG VGPRs, 196 - 224 in all: two wavefronts
// per SIMD, each with 16 rows x 12 B per lane in flight in phase 2), and its first TAIL_DEPTH moment rows (parameter + two moments in flight per lane) are requested in
// front of phase 3 (EARLY). Same-box A/B with the order rotated, 4 rounds of 200 steps, SYN-B (profiles/r06/lease16_count_scan_tail_ab.txt):
//   KEEP EARLY DEPTH   img/s (median)            KEEP EARLY DEPTH   img/s
//    0     0     4      670.3                     1     1     4      687.3   <- this form
//    0     0     8      686.2                     1     1     8      687.9
//    0     1     4      681.7                     1     1     4      686.8   with non-temporal stores of the moments
// FREEZE (iteration <= 1000: FusedAdam skips group 2, fused_adam.cpp:68-70): the lanes k >= 1 fetch their coefficient rows where phase 2 / phase 5 read them, but
// neither load nor store a moment row and store no coefficient row; mN / vN may be NULL. NOISE (the MCMC strategy between refinements, mcmc.cpp:349-386): phase 3 adds
// lfs_add_noise's update (lfs_mcmc_noise.cuh) to the mean in registers in front of its Adam update, from the raw scales / quaternion / opacity as loaded; the SH direction
// and finish_geometry have used the mean as the forward saw it. Its three deviates are requested with the finish operands (3 VGPRs in flight under phase 2).
constexpr int TAIL_DEPTH = 4;
template <int LPG, bool NEXT, bool FREEZE = false, bool NOISE = false>
__global__ void __launch_bounds__(64) gut_tail_kernel(const GutTail t, const CamDev* __restrict__ cams) {
    __shared__ float lds_b[64 * (LPG + 1)];
    __shared__ float lds_s[64 * (LPG + 1)];
    __shared__ float ldv[64 * 3];
    const uint32_t lane = threadIdx.x;
    if (t.abort_flag != nullptr && *t.abort_flag != 0) return; // (uniform) speculative step that did not fit its buffers: no update, no loss - the host runs it again
    if (t.loss_slots != nullptr && blockIdx.x == 0) { // *loss = the fused MSE: raster_finish_adam_kernel's fold (four wavefront sums of 64 slots, then (w0 + w1) + (w2 + w3))
        float w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v = t.loss_slots[64 * j + lane];
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
            w[j] = v;
        }
        if (lane == 0) *t.loss = (w[0] + w[1]) + (w[2] + w[3]);
    }
    const uint32_t N = t.N, K = t.K, KK = K - 1;
    const int degree = t.degree, Kd = (degree + 1) * (degree + 1);
    const uint32_t g0 = blockIdx.x * 64u, gmine = g0 + lane;
    const bool live = gmine < N;
    const uint32_t g = live ? gmine : (N - 1u);   // (tail lanes read the last row: no branch around the loads; they store nothing)
    constexpr int GPI = 64 / LPG;
    const int k = lane % LPG;
    // ---- phase 1 ------------------------------------------------------------------------------------------------------------------------------------------
    bool on = false;
    f3 d{0.f, 0.f, 0.f};
    float inorm = 1.f;
    const float4* a4 = reinterpret_cast<const float4*>(t.acc + size_t(g) * ACC_STRIDE);
    const float4 a3 = a4[3];
    const f3 mu = ld3(t.means, g);
    {
#pragma clang fp contract(off)
        const int2 rr = *reinterpret_cast<const int2*>(t.radii + 2 * size_t(g));
        const f3 kc = ld3(t.colors, g);
        const f3 cp = campos_of(t.viewmat);
        float b[25];
#pragma unroll
        for (int kk = 0; kk < 25; ++kk) b[kk] = 0.f;
        float v0 = 0.f, v1 = 0.f, v2 = 0.f;
        on = live && rr.x > 0 && rr.y > 0;
        if (on) {
            d = {mu.x - cp.x, mu.y - cp.y, mu.z - cp.z};
            if (degree >= 1) { inorm = 1.f / sqrtf(d.x * d.x + d.y * d.y + d.z * d.z); d = {d.x * inorm, d.y * inorm, d.z * inorm}; }
            sh_basis<false, (LPG > 16 ? 4 : 3)>(degree, d.x, d.y, d.z, b, nullptr, nullptr, nullptr);
            v0 = (kc.x > 0.f) ? a3.y : 0.f; v1 = (kc.y > 0.f) ? a3.z : 0.f; v2 = (kc.z > 0.f) ? a3.w : 0.f;
        }
#pragma unroll
        for (int kk = 0; kk < LPG; ++kk) lds_b[lane * (LPG + 1) + kk] = (kk < 25) ? b[kk] : 0.f;
        ldv[lane * 3] = v0; ldv[lane * 3 + 1] = v1; ldv[lane * 3 + 2] = v2;
    }
    // the finish pass's operands (raster_finish_adam_kernel, one round trip): in flight under phase 2
    const uint32_t o4 = g << 2, o12 = g * 12u, o16 = g << 4;
    auto at = [](const void* base, uint32_t byte_off) { return reinterpret_cast<const char*>(base) + byte_off; };
    auto ld3o = [&](const float* base, float (&dst)[3]) { const V3f x = *reinterpret_cast<const V3f*>(at(base, o12)); dst[0] = x.a[0]; dst[1] = x.a[1]; dst[2] = x.a[2]; };
    auto ld4o = [&](const float* base) { return *reinterpret_cast<const float4*>(at(base, o16)); };
    auto ld1o = [&](const float* base) { return *reinterpret_cast<const float*>(at(base, o4)); };
    const float4 a0 = a4[0], a1 = a4[1], a2 = a4[2];
    float m0[3], v0m[3], p1[3], m1[3], v1[3];
    const float4 rq = ld4o(t.raw_quats);
    const FinishAdam& ad = t.fin;
    ld3o(ad.m[0], m0); ld3o(ad.v[0], v0m); ld3o(t.raw_scales, p1); ld3o(ad.m[1], m1); ld3o(ad.v[1], v1);
    float4 mq = ld4o(ad.m[2]), vq4 = ld4o(ad.v[2]);
    float po = ld1o(t.raw_opacities), mo = ld1o(ad.m[3]), vo = ld1o(ad.v[3]);
    float nz[3] = {0.f, 0.f, 0.f};
    if (NOISE) ld3o(t.noise, nz);
    __syncthreads();
    // ---- phase 2: s_k ------------------------------------------------------------------------------------------------------------------------------------
    const uint32_t lane_el = ((lane / LPG) * KK + uint32_t(k - 1)) * 3u;   // (k == 0 lanes never use it)
    // phase 5's row addressing (the same lane meets the same rows in phase 2, whose fetches stay in registers for phase 5: PK)
    const bool row_k = uint32_t(k) < K;
    float* const pbase = (k == 0) ? t.sh0 : t.shN;
    float* const mbase = (k == 0) ? t.m0 : t.mN;
    float* const vbase = (k == 0) ? t.v0 : t.vN;
    auto row_el = [&](const int it) -> size_t {
        const size_t gg = size_t(g0) + uint32_t(it) * GPI + lane / LPG;
        return (k == 0) ? gg * 3 : (gg * KK + uint32_t(k - 1)) * 3;
    };
    auto row_ok = [&](const int it) { return row_k && (g0 + uint32_t(it) * GPI + lane / LPG) < N; };
    V3f PK[LPG];
#pragma unroll
    for (int it = 0; it < LPG; ++it) {
        PK[it].a[0] = PK[it].a[1] = PK[it].a[2] = 0.f;
        if (row_ok(it)) PK[it] = *reinterpret_cast<const V3f*>(pbase + row_el(it));
    }
    {
#pragma clang fp contract(off)
#pragma unroll
        for (int it = 0; it < LPG; ++it) {
            const uint32_t gl = it * GPI + lane / LPG;
            const float w0 = ldv[gl * 3], w1 = ldv[gl * 3 + 1], w2 = ldv[gl * 3 + 2];
            float sk = 0.f;
            // a zero gradient gives 0 x (finite) = 0 whatever the row holds: its 12 bytes are not fetched
            if (g0 + gl < N && k >= 1 && k < Kd && uint32_t(k) < K && (w0 != 0.f || w1 != 0.f || w2 != 0.f)) {
                const V3f p = PK[it];
                sk = p.a[0] * w0 + p.a[1] * w1 + p.a[2] * w2;
            }
            lds_s[gl * (LPG + 1) + k] = sk;
        }
    }
    // phase 5's moment rows: TAIL_DEPTH of them per lane in flight, requested in front of phase 3 (they land under the finish arithmetic)
    constexpr int D = (LPG < TAIL_DEPTH) ? LPG : TAIL_DEPTH;
    V3f M[D], Q[D];
    const bool upd_k = !FREEZE || k == 0;   // FREEZE: only the sh0 lane has an Adam update
    auto load = [&](const int it, const int slot) {
        if (row_ok(it) && upd_k) {
            const size_t e = row_el(it);
            M[slot] = *reinterpret_cast<const V3f*>(mbase + e); Q[slot] = *reinterpret_cast<const V3f*>(vbase + e);
        }
    };
#pragma unroll
    for (int it = 0; it < D; ++it) load(it, it);
    __syncthreads();
    // ---- phase 3: dL/d(dirs), then the finish pass ------------------------------------------------------------------------------------------------------------
    float vd[3] = {0.f, 0.f, 0.f};
    if (on && degree >= 1) {
#pragma clang fp contract(off)
        float b[25], bx[25], by[25], bz[25];
        sh_basis<true, (LPG > 16 ? 4 : 3)>(degree, d.x, d.y, d.z, b, bx, by, bz);
        float gx = 0.f, gy = 0.f, gz = 0.f;
#pragma unroll
        for (int kk = 1; kk < LPG && kk < 25; ++kk) {
            const float sk = lds_s[lane * (LPG + 1) + kk];
            gx += bx[kk] * sk; gy += by[kk] * sk; gz += bz[kk] * sk;
        }
        const float dd = gx * d.x + gy * d.y + gz * d.z;
        vd[0] = (gx - dd * d.x) * inorm; vd[1] = (gy - dd * d.y) * inorm; vd[2] = (gz - dd * d.z) * inorm;
    }
    float pm[3] = {mu.x, mu.y, mu.z};   // the mean: updated below, read again by phase 4
    // the activated quaternion / scales / opacity, from the raw values as loaded: what the projection kernel computed for the forward (lfs_activations.cuh, the same
    // function: the same bits) - the fused-tail step does not store them, and this kernel does not read them back (32 B per Gaussian each way)
    float4 q; float sc[3], o;
    splat_activations(rq, p1, po, q, sc, o);
    {   // raster_finish_adam_kernel<true> from its "everything is in flight" line on, statement by statement
        const float A[9] = {a0.x * REC_UNSCALE, a0.y * REC_UNSCALE, a0.z * REC_UNSCALE, a0.w * REC_UNSCALE, a1.x * REC_UNSCALE, a1.y * REC_UNSCALE, a1.z * REC_UNSCALE,
                            a1.w * REC_UNSCALE, a2.x * REC_UNSCALE};
        const f3 G{-a2.y * REC_UNSCALE, -a2.z * REC_UNSCALE, -a2.w * REC_UNSCALE};
        bool any = G.x != 0.f || G.y != 0.f || G.z != 0.f;
#pragma unroll
        for (int kk = 0; kk < 9; ++kk) any |= A[kk] != 0.f;
        const float v_opac = a3.x != 0.f ? a3.x / o : 0.f;
        float vm[3] = {0.f, 0.f, 0.f}, vq[4] = {0.f, 0.f, 0.f, 0.f}, vs[3] = {0.f, 0.f, 0.f};
        {
            const float is[3] = {1.f / sc[0], 1.f / sc[1], 1.f / sc[2]};
            finish_geometry<true>(q, is, A, G, mu, cams[0], vm, vq, vs);
#pragma unroll
            for (int kk = 0; kk < 3; ++kk) { vm[kk] = any ? vm[kk] : 0.f; vs[kk] = any ? vs[kk] : 0.f; }
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) vq[kk] = any ? vq[kk] : 0.f;
        }
        {
#pragma clang fp contract(off)
            float gm[3] = {vm[0] + vd[0], vm[1] + vd[1], vm[2] + vd[2]};
            const float nrm = sqrtf(rq.x * rq.x + rq.y * rq.y + rq.z * rq.z + rq.w * rq.w);
            float gq[4];
            if (nrm > 1e-12f) {
                const float inv = 1.f / nrm;
                const float y[4] = {rq.x * inv, rq.y * inv, rq.z * inv, rq.w * inv};
                const float dq = vq[0] * y[0] + vq[1] * y[1] + vq[2] * y[2] + vq[3] * y[3];
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) gq[kk] = (vq[kk] - dq * y[kk]) * inv;
            } else {
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) gq[kk] = vq[kk] * 1e12f;
            }
            float gs[3];
#pragma unroll
            for (int kk = 0; kk < 3; ++kk) gs[kk] = (vs[kk] + ad.scale_reg) * sc[kk];
            const float go = (v_opac + ad.opacity_reg) * o * (1.f - o);
            if (NOISE) mcmc_add_noise(pm, p1, rq, po, nz, t.noise_lr);   // lfs_add_noise, from the raw values as loaded (before their own updates below)
#pragma unroll
            for (int kk = 0; kk < 3; ++kk) {
                adam_elem(pm[kk], m0[kk], v0m[kk], gm[kk], ad.s[0]);
                adam_elem(p1[kk], m1[kk], v1[kk], gs[kk], ad.s[1]);
            }
            float pq[4] = {rq.x, rq.y, rq.z, rq.w};
            adam_elem(pq[0], mq.x, vq4.x, gq[0], ad.s[2]); adam_elem(pq[1], mq.y, vq4.y, gq[1], ad.s[2]);
            adam_elem(pq[2], mq.z, vq4.z, gq[2], ad.s[2]); adam_elem(pq[3], mq.w, vq4.w, gq[3], ad.s[2]);
            adam_elem(po, mo, vo, go, ad.s[3]);
            if (live) {
                auto st3a = [&](float* base, const float (&src)[3]) { V3f x; x.a[0] = src[0]; x.a[1] = src[1]; x.a[2] = src[2]; *reinterpret_cast<V3f*>(const_cast<char*>(at(base, o12))) = x; };
                st3a(t.means, pm); st3a(ad.m[0], m0); st3a(ad.v[0], v0m);
                st3a(t.raw_scales, p1); st3a(ad.m[1], m1); st3a(ad.v[1], v1);
                reinterpret_cast<float4*>(t.raw_quats)[gmine] = make_float4(pq[0], pq[1], pq[2], pq[3]);
                reinterpret_cast<float4*>(ad.m[2])[gmine] = mq; reinterpret_cast<float4*>(ad.v[2])[gmine] = vq4;
                t.raw_opacities[gmine] = po; ad.m[3][gmine] = mo; ad.v[3][gmine] = vo;
            }
        }
    }
    // ---- phase 4: the next view's basis (every Gaussian: its visibility there is not known yet) -> lds_s (this lane's own row: phase 3 has consumed it) -----------------
    if (NEXT) {
#pragma clang fp contract(off)
        const f3 cp = campos_of(t.next_viewmat);
        float b[25];
#pragma unroll
        for (int kk = 0; kk < 25; ++kk) b[kk] = 0.f;
        if (live) {   // sh_fwd_kernel<LPG, true> with radii == NULL
            f3 dn{pm[0] - cp.x, pm[1] - cp.y, pm[2] - cp.z};
            if (degree >= 1) { const float inn = 1.f / sqrtf(dn.x * dn.x + dn.y * dn.y + dn.z * dn.z); dn = {dn.x * inn, dn.y * inn, dn.z * inn}; }
            sh_basis<false, (LPG > 16 ? 4 : 3)>(degree, dn.x, dn.y, dn.z, b, nullptr, nullptr, nullptr);
        }
#pragma unroll
        for (int kk = 0; kk < LPG; ++kk) lds_s[lane * (LPG + 1) + kk] = (kk < 25) ? b[kk] : 0.f;
    }
    __syncthreads();
    // ---- phase 5: Adam on the coefficient rows (+ the next colours) ------------------------------------------------------------------------------------------------
    {
#pragma clang fp contract(off)
        const AdamScalars as = (k == 0) ? t.s0 : t.sN;
        auto st_mom = [&](float* q, const V3f& x) {
            *reinterpret_cast<V3f*>(q) = x;
        };
#pragma unroll
        for (int it0 = 0; it0 < LPG; it0 += D) {
#pragma unroll
            for (int u = 0; u < D; ++u) {
                const int it = it0 + u;
                const uint32_t gl = it * GPI + lane / LPG;
                V3f p = PK[it];
                if (row_ok(it) && upd_k) {
                    const float bk = lds_b[gl * (LPG + 1) + k];
                    const float o0 = bk * ldv[gl * 3], o1 = bk * ldv[gl * 3 + 1], o2 = bk * ldv[gl * 3 + 2];
                    V3f m = M[u], qq = Q[u];
                    adam_elem(p.a[0], m.a[0], qq.a[0], o0, as); adam_elem(p.a[1], m.a[1], qq.a[1], o1, as); adam_elem(p.a[2], m.a[2], qq.a[2], o2, as);
                    const size_t e = row_el(it);
                    *reinterpret_cast<V3f*>(pbase + e) = p; st_mom(mbase + e, m); st_mom(vbase + e, qq);
                }
                if (NEXT) {   // sh_fwd_kernel's phase 2 on the updated row (rows k >= Kd meet a zero basis value; lanes without a row contribute c = 0)
                    const float bn = lds_s[gl * (LPG + 1) + k];
                    const bool use = row_ok(it) && k < Kd;
                    float r0 = bn * (use ? p.a[0] : 0.f), r1 = bn * (use ? p.a[1] : 0.f), r2 = bn * (use ? p.a[2] : 0.f);
                    r0 = group_sum<LPG>(r0); r1 = group_sum<LPG>(r1); r2 = group_sum<LPG>(r2);
                    if (k == 0 && g0 + gl < N) {
                        float* co = t.colors + 3 * size_t(g0 + gl);
                        co[0] = fmaxf(r0 + 0.5f, 0.f); co[1] = fmaxf(r1 + 0.5f, 0.f); co[2] = fmaxf(r2 + 0.5f, 0.f);
                    }
                }
                if (it + D < LPG) load(it + D, u);
            }
        }
    }
}

// deterministic mode, after pass 2: acc[i] = fixed-point sum * 2^(e - 40) (e from the pass-1 maximum that acc[i] still holds as bits)
__global__ void __launch_bounds__(256) raster_det_resolve_kernel(const size_t n, float* __restrict__ acc, const unsigned long long* __restrict__ det64) {
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

// Launch geometry of cull / fwd / bwd: one wavefront per 8x8 cell, whole workgroups per tile.
struct RasterGeom { uint32_t tw, th, blocks_per_tile, waves_per_block, threads, grid, wpt; uint64_t cells; };
static uint32_t g_debug_flags = 0; // bit 0: keep every tile-list entry in the cell lists (no culling: the bit-identity tests); bit 4: deterministic backward accumulation
                                   // (two passes, 64-bit fixed point; 3 channels); bit 5: one-pass intersection scatter (intersect.hip). Bits 1-3 were the removed experiments.
static bool raster_geom(const lfs_cameras* cams, uint32_t tile_size, RasterGeom& g) {
    if (tile_size < 8 || tile_size > 64 || (tile_size & 7)) return false;
    g.tw = (cams->image_width + tile_size - 1) / tile_size;
    g.th = (cams->image_height + tile_size - 1) / tile_size;
    g.wpt = (tile_size / 8) * (tile_size / 8);
    g.waves_per_block = (g.wpt % 4 == 0) ? 4 : (g.wpt % 2 == 0) ? 2 : 1; // whole workgroups per tile (9, 25, 49 cells: one wave each)
    g.blocks_per_tile = g.wpt / g.waves_per_block;
    g.threads = g.waves_per_block * 64;
    const uint64_t nb = uint64_t(cams->C) * g.tw * g.th * g.blocks_per_tile;
    g.grid = cell_grid_blocks(nb, g.blocks_per_tile);
    g.cells = uint64_t(cams->C) * g.tw * g.th * g.wpt;
    return true;
}
// fwd / bwd never cooperate across the wavefronts of a workgroup (only the cull kernel shares its gathers through LDS): with one wavefront per workgroup a
// finished cell frees its slot at once instead of waiting for the slowest of its tile's four (profiles/r03/raster_wave_blocks_ab.txt: raster_bwd 0.532 - 0.537 -> 0.514 - 0.526 ms,
// raster_fwd 0.241 - 0.247 -> 0.237 - 0.241 ms)
static RasterGeom wave_geom(const lfs_cameras* cams, const RasterGeom& g) {
    RasterGeom w = g;
    w.waves_per_block = 1; w.blocks_per_tile = g.wpt; w.threads = 64;
    const uint64_t nb = uint64_t(cams->C) * g.tw * g.th * w.blocks_per_tile;
    w.grid = cell_grid_blocks(nb, w.blocks_per_tile);
    return w;
}

} // namespace lfs

using namespace lfs;

extern "C" void lfs_set_debug_flags(uint32_t flags) { g_debug_flags = flags; }
extern "C" uint32_t lfs_get_debug_flags(void) { return g_debug_flags; }

extern "C" size_t lfs_rasterize_workspace_bytes(uint32_t C, uint32_t N, uint32_t channels, uint32_t image_width, uint32_t image_height,
                                                uint32_t tile_size, int64_t n_isects) {
    (void)channels;
    lfs_cameras cams{};
    cams.C = C; cams.image_width = image_width; cams.image_height = image_height;
    RasterGeom g;
    if (!raster_geom(&cams, tile_size, g) || n_isects < 0) return 0;
    return raster_ws_offsets(C, N, g.cells, uint64_t(g.wpt) * uint64_t(n_isects), (g_debug_flags & 16u) != 0).bytes;
}
size_t lfs::raster_workspace_bytes_for(uint32_t N, uint32_t image_width, uint32_t image_height, uint32_t tile_size, int64_t capacity) {
    return lfs_rasterize_workspace_bytes(1, N, 3, image_width, image_height, tile_size, capacity);
}

static int raster_mode(const lfs_cameras* cams) { return cams->rs_type != LFS_SHUTTER_GLOBAL ? lfs::RAY_ROLLING : lfs::RAY_GLOBAL; }

// What both directions check before anything is launched or cleared: the scene's shape, the direction's own operands (`own_ok`, evaluated by the caller), the
// list sizes and the workspace, which is laid out here.
static int raster_check(const RasterScene& sc, const RasterLists& l, const Workspace& ws, bool own_ok, RasterGeom& g, RasterWs& w) {
    const lfs_cameras* cams = sc.cams;
    if (!cams || !cams->viewmats0 || !cams->Ks || cams->C == 0) return LFS_E_INVALID;
    if (cams->camera_model != LFS_CAMERA_PINHOLE && cams->camera_model != LFS_CAMERA_FISHEYE) return LFS_E_UNSUPPORTED;
    if (sc.channels < 1 || sc.channels > 4) return LFS_E_UNSUPPORTED; // Rasterization.cpp:65 asserts 3; depth modes need 1 and 4
    if (!raster_geom(cams, sc.tile_size, g)) return LFS_E_UNSUPPORTED;
    if (uint64_t(cams->C) * sc.N >= (1ull << 26)) return LFS_E_UNSUPPORTED; // 32-bit byte offsets of the record walker (4 GB of 64-B records)
    if (uint64_t(cams->C) * sc.N >= RED_MAX_ROWS) return LFS_E_UNSUPPORTED; // accumulator rows stay below the dead-lane offset of the backward's buffer atomic (lfs_raster_common.cuh)
    if (!own_ok || !l.tile_offsets || !ws.base) return LFS_E_INVALID;
    const int64_t n_sized = l.sized();
    if (n_sized < 0 || n_sized > 0x7FFFFFFFll) return LFS_E_INVALID;
    if (uint64_t(n_sized) >= (1ull << 29)) return LFS_E_UNSUPPORTED; // 32-bit byte offsets inside one cell list
    const bool det = (g_debug_flags & 16u) != 0;
    w = raster_ws(ws.base, raster_ws_offsets(cams->C, sc.N, g.cells, uint64_t(g.wpt) * uint64_t(n_sized), det), det);
    return ws.bytes < w.bytes ? LFS_E_WORKSPACE : LFS_OK;
}

// camera state, 64-byte records + culling records, compacted per-cell lists: everything fwd and bwd walk
static void raster_prepare(const RasterWs& w, const RasterGeom& g, const RasterScene& sc, const RasterLists& l, hipStream_t s, bool cams_ready, bool records_ready) {
    const lfs_cameras* cams = sc.cams;
    const uint32_t C = cams->C;
    const bool uniform = cams->rs_type == LFS_SHUTTER_GLOBAL;
    if (!cams_ready) hipLaunchKernelGGL(cam_prep_kernel, dim3(1), dim3(64), 0, s, *cams, w.cams); // (training step: written by the projection kernel already)
    const size_t CN = size_t(C) * sc.N;
    if (CN > 0 && !records_ready) { // (training step, round 4: records + culling records written by the projection kernel - projection_ut.hip, PACK)
        lfs::ProfScope prof_pack("raster_pack", s);
        const dim3 pg(uint32_t((CN + 255) / 256));
        if (uniform) hipLaunchKernelGGL(raster_pack_kernel<true>, pg, dim3(256), 0, s, C, sc.N, sc.channels, sc.means, sc.quats, sc.scales, sc.colors, sc.opacities, w.cams, w.recs, w.cull);
        else hipLaunchKernelGGL(raster_pack_kernel<false>, pg, dim3(256), 0, s, C, sc.N, sc.channels, sc.means, sc.quats, sc.scales, sc.colors, sc.opacities, w.cams, w.recs, w.cull);
    }
    lfs::ProfScope prof_cull("raster_cull", s);
    const uint32_t cull_on = (g_debug_flags & 1u) ? 0u : 1u;
#define LFS_CULL(U)                                                                                                                     \
    hipLaunchKernelGGL((raster_cull_kernel<U>), dim3(g.grid), dim3(g.threads), 0, s, C, g.tw, g.th, cams->image_width, cams->image_height, \
                       sc.tile_size, g.blocks_per_tile, g.waves_per_block, cull_on, w.cams, w.cull, sc.masks, l.tile_offsets, l.flatten_ids,  \
                       l.arg(), w.cell_count, w.cell_list)
    if (uniform) LFS_CULL(true); else LFS_CULL(false);
#undef LFS_CULL
}

int lfs::raster_forward(const RasterScene& sc, const RasterLists& l, const Workspace& ws, const RasterFwdOut& out, hipStream_t s) {
    RasterGeom g;
    RasterWs w;
    const int rc = raster_check(sc, l, ws, out.render_colors && out.render_alphas && out.last_ids, g, w);
    if (rc) return rc;
    if (sc.N > 0 && (!sc.means || !sc.quats || !sc.scales || !sc.colors || !sc.opacities)) return LFS_E_INVALID;
    if (l.sized() > 0 && !l.flatten_ids) return LFS_E_INVALID;
    const lfs_cameras* cams = sc.cams;
    raster_prepare(w, g, sc, l, s, out.cams_ready, out.records_ready);
    lfs::ProfScope prof("raster_fwd", s);
    const RasterGeom gw = wave_geom(cams, g);
    using FwdKernel = decltype(&raster_fwd_kernel<3, 0>);
    static constexpr FwdKernel table[4][2] = {   // [channels - 1][shutter mode]
        {raster_fwd_kernel<1, 0>, raster_fwd_kernel<1, 1>}, {raster_fwd_kernel<2, 0>, raster_fwd_kernel<2, 1>},
        {raster_fwd_kernel<3, 0>, raster_fwd_kernel<3, 1>}, {raster_fwd_kernel<4, 0>, raster_fwd_kernel<4, 1>}};
    hipLaunchKernelGGL(table[sc.channels - 1][raster_mode(cams)], dim3(gw.grid), dim3(gw.threads), 0, s, cams->C, sc.N, g.tw, g.th,
                       cams->image_width, cams->image_height, sc.tile_size, gw.blocks_per_tile, gw.waves_per_block,
                       w.cams, w.recs, sc.colors, sc.backgrounds, sc.masks, l.tile_offsets, w.cell_count, w.cell_list, l.arg(),
                       out.render_colors, out.render_alphas, out.last_ids, (int32_t*)nullptr);
    return (int)hipGetLastError();
}

extern "C" int lfs_rasterize_to_pixels_from_world_3dgs_fwd(
    uint32_t N, uint32_t channels, const float* means, const float* quats, const float* scales,
    const float* colors, const float* opacities, const float* backgrounds, const uint8_t* masks,
    const lfs_cameras* cams, uint32_t tile_size, const lfs_ut_params* ut_params,
    const int32_t* tile_offsets, const int32_t* flatten_ids, int64_t n_isects,
    float* render_colors, float* render_alphas, int32_t* last_ids,
    void* workspace, size_t workspace_bytes, lfs_stream_t stream) {
    (void)ut_params; // carried by the reference signature, unused by its rasterizer as well
    if (n_isects < 0) return LFS_E_INVALID;
    RasterScene sc{}; RasterFwdOut out{};
    sc.N = N; sc.channels = channels; sc.means = means; sc.quats = quats; sc.scales = scales; sc.colors = colors; sc.opacities = opacities;
    sc.backgrounds = backgrounds; sc.masks = masks; sc.cams = cams; sc.tile_size = tile_size;
    out.render_colors = render_colors; out.render_alphas = render_alphas; out.last_ids = last_ids;
    return raster_forward(sc, RasterLists{tile_offsets, flatten_ids, n_isects, 0}, Workspace{workspace, workspace_bytes}, out, (hipStream_t)stream);
}

// where the records / culling records of a (one-camera) rasterizer workspace live: the training step's projection kernel writes them there (the camera state is its first block)
void lfs::raster_workspace_parts(void* workspace, uint32_t N, void** recs, void** cull) {
    const RasterWsOffsets at = raster_ws_offsets(1, N, 0, 0, false);
    *recs = static_cast<char*>(workspace) + at.recs;
    *cull = static_cast<char*>(workspace) + at.cull;
}

// the fused MSE takes one camera, RGB, no masks and no dL/d(alpha); its loss pointer is needed only where a finish pass writes through it
static bool mse_form_ok(const RasterScene& sc, const RasterBwd& b) {
    const RasterMse* m = b.mse;
    return !m || (sc.channels == 3 && sc.cams && sc.cams->C == 1 && !sc.masks && !b.v_render_alphas && m->render && m->target_chw && (b.rows_only || m->loss));
}

int lfs::raster_backward(const RasterScene& sc, const RasterLists& l, const Workspace& ws, const RasterBwd& b, hipStream_t s) {
    RasterGeom g;
    RasterWs w;
    const int rc = raster_check(sc, l, ws, mse_form_ok(sc, b), g, w);
    if (rc) return rc;
    const lfs_cameras* cams = sc.cams;
    const uint32_t C = cams->C, N = sc.N, channels = sc.channels;
    const int64_t n_sized = l.sized();
    const bool det = (g_debug_flags & 16u) != 0 && channels == 3;
    if (N == 0) return LFS_OK;
    if (!sc.means || !sc.quats || !sc.scales || !sc.colors || !sc.opacities) return LFS_E_INVALID;
    if (!b.rows_only && (!b.v_means || !b.v_quats || !b.v_scales || !b.v_colors || !b.v_opacities)) return LFS_E_INVALID;
    if (b.rows_only && (channels != 3 || C != 1)) return LFS_E_INVALID; // the accumulator-only forms feed lfs_gut_finish_adam / lfs_gut_finish_grads (one camera, RGB)
    if (n_sized > 0 && (!l.flatten_ids || !b.render_alphas || !b.last_ids || (!b.v_render_colors && !b.mse))) return LFS_E_INVALID; // v_render_alphas == NULL: zeros
    const bool uniform = cams->rs_type == LFS_SHUTTER_GLOBAL;
    const size_t CN = size_t(C) * N;
    hipError_t e = hipMemsetAsync(w.acc, 0, sizeof(float) * (ACC_STRIDE * CN + (b.mse ? LOSS_SLOTS : 0)), s);
    MseFuse mse_dev{};   // the kernel adds its partial sums into the slots behind the rows; raster_finish (or the step's finish / tail pass) folds them into *loss
    if (b.mse) mse_dev = MseFuse{b.mse->render, b.mse->target_chw, b.mse->weight / float(3u * cams->image_width * cams->image_height), w.acc + ACC_STRIDE * CN, nullptr};
    if (e != hipSuccess) return (int)e;
    if (det) { e = hipMemsetAsync(w.det64, 0, sizeof(unsigned long long) * ACC_STRIDE * CN, s); if (e != hipSuccess) return (int)e; mse_dev.det64 = w.det64; }
    if (channels > 3) { e = hipMemsetAsync(b.v_colors, 0, sizeof(float) * channels * CN, s); if (e != hipSuccess) return (int)e; }
    if (!b.prepared) raster_prepare(w, g, sc, l, s, false, false);
    if (n_sized > 0) {
        // One launch (every mode but the deterministic one): timed, when asked for, through the dispatch packet's own signal (lfs_prof.h, prof_kernel_events) - no
        // event-record packets around the dominant kernel inside bench.py's timed region (profiles/r06/lease33_ext_launch_timing_ab.txt). The deterministic mode's two passes + resolve keep the event scope.
        hipEvent_t pe0 = nullptr, pe1 = nullptr;
#ifndef LFS_EMULATE
        const bool ext_timed = !det && lfs::prof_kernel_events("raster_bwd", &pe0, &pe1);
#else
        const bool ext_timed = false;
#endif
        lfs::ProfScope prof(ext_timed ? "" : "raster_bwd", s);
        const RasterGeom gw = wave_geom(cams, g);
        using BwdKernel = decltype(&raster_bwd_kernel<3, 0>);
#define LFS_BWD_DET(LOSSV) {{raster_bwd_kernel<3, 0, LOSSV, 1>, raster_bwd_kernel<3, 0, LOSSV, 2>}, {raster_bwd_kernel<3, 1, LOSSV, 1>, raster_bwd_kernel<3, 1, LOSSV, 2>}}
        // the deterministic mode's passes (1: per-slot maxima of |total|, integer atomicMax; 2: 64-bit fixed-point sums, then back to float): [no fused loss][shutter mode][pass - 1]
        // (the tables name the kernels in the order the code object has always defined them: its layout follows the order of first use)
        static constexpr BwdKernel det_passes[2][2][2] = {LFS_BWD_DET(true), LFS_BWD_DET(false)};
#undef LFS_BWD_DET
        static constexpr BwdKernel fused_mse[2] = {raster_bwd_kernel<3, 0, true>, raster_bwd_kernel<3, 1, true>};   // [shutter mode]
        static constexpr BwdKernel plain[4][2] = {   // [channels - 1][shutter mode]
            {raster_bwd_kernel<1, 0>, raster_bwd_kernel<1, 1>}, {raster_bwd_kernel<2, 0>, raster_bwd_kernel<2, 1>},
            {raster_bwd_kernel<3, 0>, raster_bwd_kernel<3, 1>}, {raster_bwd_kernel<4, 0>, raster_bwd_kernel<4, 1>}};
        const int mode = raster_mode(cams);
#define LFS_BWD_ARGS C, N, g.tw, g.th, cams->image_width, cams->image_height, sc.tile_size, gw.blocks_per_tile, gw.waves_per_block, w.cams, w.recs, sc.colors, sc.backgrounds, \
                     sc.masks, l.tile_offsets, w.cell_count, w.cell_list, l.arg(), b.render_alphas, b.last_ids, b.v_render_colors, b.v_render_alphas, w.acc, b.v_colors, mse_dev
        auto launch = [&](BwdKernel k) {
#ifndef LFS_EMULATE
            if (ext_timed) { hipExtLaunchKernelGGL(k, dim3(gw.grid), dim3(gw.threads), 0, s, pe0, pe1, 0, LFS_BWD_ARGS); return; }
#endif
            hipLaunchKernelGGL(k, dim3(gw.grid), dim3(gw.threads), 0, s, LFS_BWD_ARGS);
        };
#undef LFS_BWD_ARGS
        if (det) {
            launch(det_passes[b.mse ? 0 : 1][mode][0]); launch(det_passes[b.mse ? 0 : 1][mode][1]);
            const size_t n_acc = ACC_STRIDE * CN;
            hipLaunchKernelGGL(raster_det_resolve_kernel, dim3(uint32_t((n_acc + 255) / 256)), dim3(256), 0, s, n_acc, w.acc, w.det64);
        } else launch(b.mse ? fused_mse[mode] : plain[channels - 1][mode]);
    }
    if (b.rows_only) return (int)hipGetLastError();
    const dim3 fg((N + 255) / 256);
    lfs::ProfScope prof_fin("raster_finish", s);
    const float* slots = b.mse ? w.acc + ACC_STRIDE * CN : nullptr;
    float* loss_out = b.mse ? b.mse->loss : nullptr;
    if (uniform) hipLaunchKernelGGL(raster_finish_kernel<true>, fg, dim3(256), 0, s, C, N, channels, sc.means, sc.quats, sc.scales, w.cams, w.acc, b.v_means, b.v_quats, b.v_scales, b.v_colors, b.v_opacities, slots, loss_out, sc.opacities);
    else hipLaunchKernelGGL(raster_finish_kernel<false>, fg, dim3(256), 0, s, C, N, channels, sc.means, sc.quats, sc.scales, w.cams, w.acc, b.v_means, b.v_quats, b.v_scales, b.v_colors, b.v_opacities, slots, loss_out, sc.opacities);
    return (int)hipGetLastError();
}

extern "C" int lfs_rasterize_to_pixels_from_world_3dgs_bwd_prepared(
    uint32_t N, uint32_t channels, const float* means, const float* quats, const float* scales,
    const float* colors, const float* opacities, const float* backgrounds, const uint8_t* masks,
    const lfs_cameras* cams, uint32_t tile_size, const lfs_ut_params* ut_params,
    const int32_t* tile_offsets, const int32_t* flatten_ids, int64_t n_isects,
    const float* render_alphas, const int32_t* last_ids,
    const float* v_render_colors, const float* v_render_alphas,
    float* v_means, float* v_quats, float* v_scales, float* v_colors, float* v_opacities,
    void* workspace, size_t workspace_bytes, lfs_stream_t stream) {
    (void)ut_params;
    if (n_isects < 0) return LFS_E_INVALID;
    RasterScene sc{}; RasterBwd b{};
    sc.N = N; sc.channels = channels; sc.means = means; sc.quats = quats; sc.scales = scales; sc.colors = colors; sc.opacities = opacities;
    sc.backgrounds = backgrounds; sc.masks = masks; sc.cams = cams; sc.tile_size = tile_size;
    b.render_alphas = render_alphas; b.last_ids = last_ids; b.v_render_colors = v_render_colors; b.v_render_alphas = v_render_alphas;
    b.v_means = v_means; b.v_quats = v_quats; b.v_scales = v_scales; b.v_colors = v_colors; b.v_opacities = v_opacities; b.prepared = true;
    return raster_backward(sc, RasterLists{tile_offsets, flatten_ids, n_isects, 0}, Workspace{workspace, workspace_bytes}, b, (hipStream_t)stream);
}

// the self-contained form: camera state, records and cell lists are rebuilt in front of the backward
extern "C" int lfs_rasterize_to_pixels_from_world_3dgs_bwd(
    uint32_t N, uint32_t channels, const float* means, const float* quats, const float* scales,
    const float* colors, const float* opacities, const float* backgrounds, const uint8_t* masks,
    const lfs_cameras* cams, uint32_t tile_size, const lfs_ut_params* ut_params,
    const int32_t* tile_offsets, const int32_t* flatten_ids, int64_t n_isects,
    const float* render_alphas, const int32_t* last_ids,
    const float* v_render_colors, const float* v_render_alphas,
    float* v_means, float* v_quats, float* v_scales, float* v_colors, float* v_opacities,
    void* workspace, size_t workspace_bytes, lfs_stream_t stream) {
    (void)ut_params;
    if (n_isects < 0) return LFS_E_INVALID;
    RasterScene sc{}; RasterBwd b{};
    sc.N = N; sc.channels = channels; sc.means = means; sc.quats = quats; sc.scales = scales; sc.colors = colors; sc.opacities = opacities;
    sc.backgrounds = backgrounds; sc.masks = masks; sc.cams = cams; sc.tile_size = tile_size;
    b.render_alphas = render_alphas; b.last_ids = last_ids; b.v_render_colors = v_render_colors; b.v_render_alphas = v_render_alphas;
    b.v_means = v_means; b.v_quats = v_quats; b.v_scales = v_scales; b.v_colors = v_colors; b.v_opacities = v_opacities;
    return raster_backward(sc, RasterLists{tile_offsets, flatten_ids, n_isects, 0}, Workspace{workspace, workspace_bytes}, b, (hipStream_t)stream);
}

// "prepared" backward with the clamped MSE loss of lfs_mse_loss_fwd_bwd folded in (extension): render_colors [H,W,3] = the forward
// output, target_chw [3,H,W]; *loss += weight * mean((clamp(render, 0, 1) - target)^2). One camera, 3 channels, no masks.
extern "C" int lfs_rasterize_to_pixels_from_world_3dgs_bwd_prepared_mse(
    uint32_t N, const float* means, const float* quats, const float* scales, const float* colors, const float* opacities,
    const float* backgrounds, const lfs_cameras* cams, uint32_t tile_size, const int32_t* tile_offsets, const int32_t* flatten_ids,
    int64_t n_isects, const float* render_colors, const float* render_alphas, const int32_t* last_ids, const float* target_chw, float weight,
    float* loss, float* v_means, float* v_quats, float* v_scales, float* v_colors, float* v_opacities, void* workspace, size_t workspace_bytes,
    lfs_stream_t stream) {
    if (!cams || !render_colors || !target_chw || !loss || n_isects < 0) return LFS_E_INVALID;
    if (n_isects == 0) return LFS_E_UNSUPPORTED; // nothing rendered: use lfs_mse_loss_fwd_bwd (the loss of the background image)
    const RasterMse mse{render_colors, target_chw, weight, loss};
    RasterScene sc{}; RasterBwd b{};   // (RGB, no masks)
    b.render_alphas = render_alphas; b.last_ids = last_ids; b.mse = &mse;
    b.v_means = v_means; b.v_quats = v_quats; b.v_scales = v_scales; b.v_colors = v_colors; b.v_opacities = v_opacities; b.prepared = true;
    sc.N = N; sc.channels = 3; sc.means = means; sc.quats = quats; sc.scales = scales; sc.colors = colors; sc.opacities = opacities;
    sc.backgrounds = backgrounds; sc.cams = cams; sc.tile_size = tile_size;
    return raster_backward(sc, RasterLists{tile_offsets, flatten_ids, n_isects, 0}, Workspace{workspace, workspace_bytes}, b, (hipStream_t)stream);
}


// ---- the all-inline training step (extension; one camera, global shutter, 3 channels): accumulator-only backward + fused finish / Adam ----
// lfs_rasterize_..._bwd_prepared_mse without its last kernel: the per-Gaussian sums stay in the workspace (rows of 16 floats at
// lfs_rasterize_workspace_acc_offset) together with the loss partial sums; lfs_sh_model_bwd_adam_all reads dL/dcolour from the rows and writes
// dL/d(dirs) into them, lfs_gut_finish_adam turns them into the parameter updates.
extern "C" size_t lfs_rasterize_workspace_acc_offset(uint32_t C, uint32_t N) { return raster_ws_offsets(C, N, 0, 0, false).acc; }

extern "C" int lfs_rasterize_to_pixels_from_world_3dgs_bwd_prepared_mse_acc(
    uint32_t N, const float* means, const float* quats, const float* scales, const float* colors, const float* opacities,
    const float* backgrounds, const lfs_cameras* cams, uint32_t tile_size, const int32_t* tile_offsets, const int32_t* flatten_ids,
    int64_t n_isects, const float* render_colors, const float* render_alphas, const int32_t* last_ids, const float* target_chw, float weight,
    void* workspace, size_t workspace_bytes, lfs_stream_t stream) {
    if (n_isects < 0) return LFS_E_INVALID;
    if (n_isects == 0) return LFS_E_UNSUPPORTED;
    if (!cams || !render_colors || !target_chw) return LFS_E_INVALID;
    const RasterMse mse{render_colors, target_chw, weight, nullptr};
    RasterScene sc{}; RasterBwd b{};   // (RGB, no masks)
    b.render_alphas = render_alphas; b.last_ids = last_ids; b.mse = &mse; b.prepared = true; b.rows_only = true;
    sc.N = N; sc.channels = 3; sc.means = means; sc.quats = quats; sc.scales = scales; sc.colors = colors; sc.opacities = opacities;
    sc.backgrounds = backgrounds; sc.cams = cams; sc.tile_size = tile_size;
    return raster_backward(sc, RasterLists{tile_offsets, flatten_ids, n_isects, 0}, Workspace{workspace, workspace_bytes}, b, (hipStream_t)stream);
}

// the same for a caller-provided dL/d(render) (any loss): lfs_..._bwd_prepared without its last kernel
extern "C" int lfs_rasterize_to_pixels_from_world_3dgs_bwd_prepared_acc(
    uint32_t N, const float* means, const float* quats, const float* scales, const float* colors, const float* opacities,
    const float* backgrounds, const lfs_cameras* cams, uint32_t tile_size, const int32_t* tile_offsets, const int32_t* flatten_ids,
    int64_t n_isects, const float* render_alphas, const int32_t* last_ids, const float* v_render_colors, const float* v_render_alphas,
    void* workspace, size_t workspace_bytes, lfs_stream_t stream) {
    if (!cams || !v_render_colors || n_isects < 0) return LFS_E_INVALID;
    RasterScene sc{}; RasterBwd b{};   // (RGB, no masks)
    b.render_alphas = render_alphas; b.last_ids = last_ids; b.v_render_colors = v_render_colors; b.v_render_alphas = v_render_alphas; b.prepared = true; b.rows_only = true;
    sc.N = N; sc.channels = 3; sc.means = means; sc.quats = quats; sc.scales = scales; sc.colors = colors; sc.opacities = opacities;
    sc.backgrounds = backgrounds; sc.cams = cams; sc.tile_size = tile_size;
    return raster_backward(sc, RasterLists{tile_offsets, flatten_ids, n_isects, 0}, Workspace{workspace, workspace_bytes}, b, (hipStream_t)stream);
}

// ---- the finish and tail passes over the accumulator rows ----
constexpr int FINISH_GROUP[4] = {0, 3, 4, 5};   // FusedAdam's groups in raster_finish_adam_kernel's order: means, raw_scales, raw_quats, raw_opacities
static AdamScalars adam_scalars(const float (&v)[6]) { return AdamScalars{v[0], v[1], v[2], v[3], v[4], v[5]}; }

// FinishAdam of a pass over N Gaussians: the regularisers of trainer.cpp:132-158 (as lfs_activations_bwd): scale_reg * mean(scales) over 3N values, opacity_reg *
// mean(opacities) - and, with `adam`, the moments and scalars of its four groups (false: one of them is missing)
static bool fill_finish_adam(FinishAdam& ad, uint32_t N, const GutRegs& regs, const GutAdam* adam) {
    ad = FinishAdam{};
    ad.scale_reg = regs.scale_reg / (3.f * float(N)); ad.opacity_reg = regs.opacity_reg / float(N);
    for (int j = 0; adam && j < 4; ++j) {
        const int k = FINISH_GROUP[j];
        if (!adam->exp_avg[k] || !adam->exp_avg_sq[k]) return false;
        ad.m[j] = adam->exp_avg[k]; ad.v[j] = adam->exp_avg_sq[k]; ad.s[j] = adam_scalars(adam->scalars[k]);
    }
    return true;
}
static const float* loss_slots_of(const RasterWs& w, uint32_t N, const float* loss) { return loss ? w.acc + ACC_STRIDE * size_t(N) : nullptr; }

// The accumulator rows -> gradient TENSORS of the raw parameters in one pass (raster_finish + lfs_activations_bwd + the copy of dL/dmeans): for steps
// that need the gradients themselves (multi-GPU all-reduce, several views per step, non-MSE losses). g.* are written or, accumulate != 0, added to;
// v_colors [N,3] is written (the SH backward consumes it and adds dL/d(dirs) onto g.means). loss (nullable): += the fused MSE partial sums.
int lfs::gut_finish_grads_impl(const GutParams& p, const GutActivated& act, const GutRegs& regs, const GutGrads& g, const float* v_dirs, float* loss,
                               const Workspace& ws, hipStream_t s, const GutDensify* dens) {
    const uint32_t N = p.N;
    const bool densify = dens != nullptr && dens->info != nullptr;
    if (densify && !dens->radii) return LFS_E_INVALID;   // (before anything else: the statistic without the view's radii is refused whatever N is)
    if (N == 0) return LFS_OK;
    if (!p.means || !p.raw_quats || !act.quats || !act.scales || !act.opacities || !g.means || !g.raw_scales || !g.raw_quats || !g.raw_opacities || (!g.v_colors && !v_dirs) || !ws.base) return LFS_E_INVALID;
    RasterWs w;
    if (!rows_ws(ws, N, w)) return LFS_E_WORKSPACE;
    FinishAdam ad;
    fill_finish_adam(ad, N, regs, nullptr);
    const FinishGrads gr{g.means, g.raw_scales, g.raw_quats, g.raw_opacities, g.v_colors, g.accumulate};
    if (densify) {
        return finish_densify_launch(N, p.means, p.raw_quats, act.quats, act.scales, act.opacities, w.cams, w.acc, v_dirs, ad, gr, loss_slots_of(w, N, loss), loss, dens->radii,
                                     dens->info, s);
    }
    lfs::ProfScope prof("finish_grads", s);
    hipLaunchKernelGGL(raster_finish_adam_kernel<false>, dim3((N + FINISH_BLOCK - 1) / FINISH_BLOCK), dim3(FINISH_BLOCK), 0, s, N, p.means, (float*)nullptr, p.raw_quats,
                       (float*)nullptr, act.quats, act.scales, act.opacities, w.cams, w.acc, v_dirs, ad, gr, loss_slots_of(w, N, loss), loss, (const int32_t*)nullptr);
    return (int)hipGetLastError();
}

// ext (nullable) with densification_info: the densifying form of the pass, which reads `radii` [N,2] of the view (LFS_E_INVALID without them, before any launch).
// ext NULL or its pointer NULL: lfs_gut_finish_grads - the same launch, the same bits.
extern "C" int lfs_gut_finish_grads_ex(
    uint32_t N, const float* means, const float* raw_quats, const float* quats, const float* scales, const float* opacities, float scale_reg, float opacity_reg,
    int accumulate, float* g_means, float* g_raw_scales, float* g_raw_quats, float* g_raw_opacities, float* v_colors, float* loss,
    const int32_t* radii, const lfs_gut_view_ext* ext, void* workspace, size_t workspace_bytes, lfs_stream_t stream) {
    const GutDensify dens{radii, ext ? ext->densification_info : nullptr};
    if (dens.info && !radii) return LFS_E_INVALID;
    if (N != 0 && !v_colors) return LFS_E_INVALID;
    GutParams p{};   // (read only: the kernel's gradient-tensor forms store no parameter)
    p.N = N; p.means = const_cast<float*>(means); p.raw_quats = const_cast<float*>(raw_quats);
    return lfs::gut_finish_grads_impl(p, GutActivated{quats, scales, opacities}, GutRegs{scale_reg, opacity_reg},
                                      GutGrads{g_means, g_raw_scales, g_raw_quats, g_raw_opacities, v_colors, accumulate}, nullptr, loss,
                                      Workspace{workspace, workspace_bytes}, (hipStream_t)stream, dens.info ? &dens : nullptr);
}

extern "C" int lfs_gut_finish_grads(
    uint32_t N, const float* means, const float* raw_quats, const float* quats, const float* scales, const float* opacities, float scale_reg, float opacity_reg,
    int accumulate, float* g_means, float* g_raw_scales, float* g_raw_quats, float* g_raw_opacities, float* v_colors, float* loss,
    void* workspace, size_t workspace_bytes, lfs_stream_t stream) {
    return lfs_gut_finish_grads_ex(N, means, raw_quats, quats, scales, opacities, scale_reg, opacity_reg, accumulate, g_means, g_raw_scales, g_raw_quats, g_raw_opacities,
                                   v_colors, loss, nullptr, nullptr, workspace, workspace_bytes, stream);
}

int lfs::gut_finish_adam_impl(const GutParams& p, const GutActivated& act, const GutAdam& adam, const GutRegs& regs, const float* v_dirs, float* loss,
                              const Workspace& ws, hipStream_t s) {
    const uint32_t N = p.N;
    if (N == 0) return LFS_OK;
    if (!v_dirs) return LFS_E_INVALID;
    if (!p.means || !p.raw_scales || !p.raw_quats || !p.raw_opacities || !act.quats || !act.scales || !act.opacities || !adam.exp_avg || !adam.exp_avg_sq || !adam.scalars || !ws.base) return LFS_E_INVALID;
    RasterWs w;
    if (!rows_ws(ws, N, w)) return LFS_E_WORKSPACE;
    FinishAdam ad;
    if (!fill_finish_adam(ad, N, regs, &adam)) return LFS_E_INVALID;
    lfs::ProfScope prof("finish_adam", s);
    hipLaunchKernelGGL(raster_finish_adam_kernel<true>, dim3((N + FINISH_BLOCK - 1) / FINISH_BLOCK), dim3(FINISH_BLOCK), 0, s, N, p.means, p.raw_scales, p.raw_quats, p.raw_opacities,
                       act.quats, act.scales, act.opacities, w.cams, w.acc, v_dirs, ad, FinishGrads{}, loss_slots_of(w, N, loss), loss, adam.abort_flag);
    return (int)hipGetLastError();
}

// The fused tail of the all-inline step (gut_tail_kernel): SH backward + all six Adam updates (+ the next view's SH colours -> colors [N,3] when next_viewmat is given).
// LFS_E_UNSUPPORTED for K > 16 (degree 4): the caller enqueues lfs_sh_model_bwd_adam_all + lfs_gut_finish_adam instead.
// The activated quaternions / scales / opacities are not an input: the kernel recomputes them from the raw values (lfs_activations.cuh).
int lfs::gut_tail_impl(const GutParams& p, const GutAdam& adam, const GutRegs& regs, const GutTailView& view, float* loss, const Workspace& ws, hipStream_t s) {
    const uint32_t N = p.N, K = p.K;
    if (N == 0) return LFS_OK;
    const uint32_t Kd = (p.sh_degree + 1) * (p.sh_degree + 1);
    if (p.sh_degree > 3 || Kd > K || K < 2) return LFS_E_INVALID;
    if (K > 16) return LFS_E_UNSUPPORTED;
    if (!p.means || !p.sh0 || !p.shN || !p.raw_scales || !p.raw_quats || !p.raw_opacities || !view.viewmat || !view.radii ||
        !view.colors || !adam.exp_avg || !adam.exp_avg_sq || !adam.scalars || !ws.base) return LFS_E_INVALID;
    for (int k = 0; k < 6; ++k) if ((!adam.exp_avg[k] || !adam.exp_avg_sq[k]) && !(view.freeze_shN && k == 2)) return LFS_E_INVALID;
    RasterWs w;
    if (!rows_ws(ws, N, w)) return LFS_E_WORKSPACE;
    GutTail t{};
    t.N = N; t.K = K; t.degree = int(p.sh_degree);
    t.means = p.means; t.sh0 = p.sh0; t.shN = p.shN; t.raw_scales = p.raw_scales; t.raw_quats = p.raw_quats; t.raw_opacities = p.raw_opacities;
    t.viewmat = view.viewmat; t.next_viewmat = view.next_viewmat; t.radii = view.radii; t.colors = view.colors; t.acc = w.acc;
    t.m0 = adam.exp_avg[1]; t.v0 = adam.exp_avg_sq[1]; t.s0 = adam_scalars(adam.scalars[1]);
    t.mN = adam.exp_avg[2]; t.vN = adam.exp_avg_sq[2]; t.sN = adam_scalars(adam.scalars[2]);
    fill_finish_adam(t.fin, N, regs, &adam);
    t.loss_slots = loss_slots_of(w, N, loss); t.loss = loss; t.abort_flag = adam.abort_flag;
    t.noise = view.noise; t.noise_lr = view.noise_lr;
    const dim3 grid((N + 63) / 64), block(64);
    lfs::ProfScope prof("tail_sh_finish_adam", s);
    using TailKernel = void (*)(const GutTail, const CamDev*);
#define LFS_TAIL_ROW(LPG, NEXT) {gut_tail_kernel<LPG, NEXT, false, false>, gut_tail_kernel<LPG, NEXT, false, true>, gut_tail_kernel<LPG, NEXT, true, false>, gut_tail_kernel<LPG, NEXT, true, true>}
    static const TailKernel table[2][2][4] = {{LFS_TAIL_ROW(4, false), LFS_TAIL_ROW(4, true)}, {LFS_TAIL_ROW(16, false), LFS_TAIL_ROW(16, true)}};   // [LPG][NEXT][2 FREEZE + NOISE]
#undef LFS_TAIL_ROW
    hipLaunchKernelGGL(table[K <= 4 ? 0 : 1][view.next_viewmat ? 1 : 0][(view.freeze_shN ? 2 : 0) + (view.noise ? 1 : 0)], grid, block, 0, s, t, w.cams);
    return (int)hipGetLastError();
}

// the public form takes its four groups in the kernel's order: scalars[k] = {lr, beta1, beta2, eps, bc1_rcp, bc2_sqrt_rcp} for k = means, raw_scales, raw_quats,
// raw_opacities; *loss = the fused MSE of the backward (stored, not added)
extern "C" int lfs_gut_finish_adam(
    uint32_t N, float* means, float* raw_scales, float* raw_quats, float* raw_opacities, const float* quats, const float* scales, const float* opacities,
    const float* v_dirs, float* const* exp_avg /* [4] host */, float* const* exp_avg_sq /* [4] host */, const float* scalars /* [4][6] host */, float scale_reg,
    float opacity_reg, float* loss, void* workspace, size_t workspace_bytes, lfs_stream_t stream) {
    if (N == 0) return LFS_OK;
    if (!exp_avg || !exp_avg_sq || !scalars) return LFS_E_INVALID;
    float *m[6] = {}, *v[6] = {}, sc[6][6] = {};
    for (int j = 0; j < 4; ++j) { const int k = FINISH_GROUP[j]; m[k] = exp_avg[j]; v[k] = exp_avg_sq[j]; for (int i = 0; i < 6; ++i) sc[k][i] = scalars[6 * j + i]; }
    GutParams p{};
    p.N = N; p.means = means; p.raw_scales = raw_scales; p.raw_quats = raw_quats; p.raw_opacities = raw_opacities;
    return lfs::gut_finish_adam_impl(p, GutActivated{quats, scales, opacities}, GutAdam{m, v, sc, nullptr}, GutRegs{scale_reg, opacity_reg}, v_dirs, loss,
                                     Workspace{workspace, workspace_bytes}, (hipStream_t)stream);
}
