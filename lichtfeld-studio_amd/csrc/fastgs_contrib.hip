// Contribution statistic of the EWA ("fastgs") rasterizer (extension): per Gaussian, over the pixels of one view into which the forward blends it,
// the maximum, the number and the sum of its blending weights w = T alpha - what RadSplat (max w), LightGaussian / Mini-Splatting (sum w) and the other
// contribution-based pruning rules reduce over the training rays. A translation unit of its own: fastgs_blend.hip's code object keeps every byte.
//
// The walk is fg_blend_fwd_kernel's: one wavefront per 8x8 cell over the cell's list, the records through the scalar unit, the same frag_eval, the same transmittance
// recurrence, so `contrib` below is bit for bit the forward's predicate (and the blend backward's `valid`). Nothing of the image is accumulated; per (wavefront,
// instance) with a non-empty ballot: one wave reduction each for the sum and the maximum (DPP inside the rows of 16 lanes, v_readlane across them: a fixed order), the count from the ballot, and
// lane 0 issues three integer atomics into the Gaussian's 16-byte row {max w as bits | pairs | sum w in 40.24 fixed point (two dwords)}. Non-negative floats order
// like their bit patterns, integer adds commute: the row does not depend on the order in which wavefronts, calls or views arrive. No float atomics, no LDS, no scratch.
#include "lfs_fastgs.cuh"
#include "lfs_prof.h"

namespace lfs {
namespace fgs {

constexpr float CONTRIB_FIX = 16777216.f;   // 2^24: the fraction bits of the sum word

LFS_DI float row_value(float v, int lane) { return __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(v), lane)); }

__global__ void __launch_bounds__(64) fg_contrib_kernel(
    const uint32_t gw, const uint32_t gh, const uint32_t width, const uint32_t height,
    const GaussRec* __restrict__ recs, const int32_t* __restrict__ offsets, const int32_t* __restrict__ cell_count, const int2* __restrict__ cell_list,
    uint32_t* __restrict__ stats) {
    const uint32_t total_tiles = gw * gh;
    const CellCtx cc = cell_ctx(total_tiles, total_tiles, gw, TILE, WPT, 1);
    if (!cc.in_grid) return;
    const uint32_t lane = threadIdx.x & 63;
    const bool inside = cc.i < height && cc.j < width;
    const float px = float(cc.j) + 0.5f, py = float(cc.i) + 0.5f;
    const int32_t start = offsets[cc.tile_global], end = offsets[cc.tile_global + 1];
    const int2* __restrict__ cl = cell_list + (size_t(WPT) * size_t(start) + size_t(cc.wl) * size_t(end - start));
    const int32_t cnt = cell_count[size_t(cc.tile_global) * WPT + cc.wl];
    const float INF = __builtin_inff();
    float thr = inside ? MIN_ALPHA : INF; // "done" (and a lane outside the image) is carried as the alpha threshold, as in fg_blend_fwd_kernel
    float T = 1.f;
    auto eval = [&](const GaussRec& rec, const int2 e) {
        const Frag f = frag_eval(rec, px, py);
        const bool pass = f.ok && !(f.alpha < thr);
        if (__ballot(pass) == 0ull) return;
        const float next_T = T * (1.f - f.alpha);
        const bool fin = pass && next_T < T_THRESHOLD; // terminates without blending: not in the image, not in the statistic
        const bool contrib = pass && !fin;
        const float w = contrib ? T * f.alpha : 0.f;   // (the forward's product, bit for bit; 0 is the neutral element of both reductions)
        T = contrib ? next_T : T;
        thr = fin ? INF : thr;
        const uint64_t m = __ballot(contrib);
        if (m == 0ull) return;
        // rows of 16 lanes by DPP (lane^1, lane^2, rotate by 4, by 8), the four row results through v_readlane: a fixed order, and nothing that waits on lgkmcnt -
        // a ds_bpermute butterfly would make every reduction wait for the record loads the walker keeps in flight
        float sum = w, mx = w;
        sum += dpp_mov<0xB1>(sum); mx = fmaxf(mx, dpp_mov<0xB1>(mx));
        sum += dpp_mov<0x4E>(sum); mx = fmaxf(mx, dpp_mov<0x4E>(mx));
        sum += dpp_mov<0x124>(sum); mx = fmaxf(mx, dpp_mov<0x124>(mx));
        sum += dpp_mov<0x128>(sum); mx = fmaxf(mx, dpp_mov<0x128>(mx));
        sum = ((row_value(sum, 0) + row_value(sum, 16)) + row_value(sum, 32)) + row_value(sum, 48);
        mx = fmaxf(fmaxf(row_value(mx, 0), row_value(mx, 16)), fmaxf(row_value(mx, 32), row_value(mx, 48)));
        if (lane == 0) {
            uint32_t* const row = stats + (size_t(uint32_t(e.x)) << 2);
            atomicMax(row, __float_as_uint(mx));
            atomicAdd(row + 1, uint32_t(__popcll(m)));
            atomicAdd(reinterpret_cast<unsigned long long*>(row + 2), (unsigned long long)llrintf(sum * CONTRIB_FIX));   // sum <= 64 x 0.999: exact scaling, one rounding
        }
    };
    walk_cell_list<1>(cl, recs, 0, cnt, eval, [&]() { return __ballot(thr < INF) != 0ull; });
}

} // namespace fgs
} // namespace lfs

using namespace lfs;

// The instance and cell lists are the ones lfs_fastgs_view_render left in the instance workspace; the records, the tile offsets and the mode (antialiased, 3D filter,
// depth: all of it is in the records) the ones of the preprocess. Nothing but `stats` is written.
extern "C" int lfs_fastgs_view_contribution(const lfs_fastgs_view* view, int64_t n_instances, void* instance_workspace, size_t instance_workspace_bytes,
                                            uint32_t* stats, lfs_stream_t stream) {
    if (!view || !stats || !view->primitive_workspace) return LFS_E_INVALID;
    const uint32_t N = view->N, width = view->width, height = view->height;
    if (width == 0 || height == 0 || n_instances < 0 || n_instances > 0x7FFFFFFFll) return LFS_E_INVALID;
    if (reinterpret_cast<uintptr_t>(stats) % 8 != 0) return LFS_E_INVALID;   // the sum word takes a 64-bit atomic
    if (N >= (1u << 26) || uint64_t(n_instances) >= (1ull << 29)) return LFS_E_UNSUPPORTED; // 32-bit byte offsets of the record walker
    const fgs::PrimWs w = fgs::prim_ws(view->primitive_workspace, N, width, height);
    if (view->primitive_workspace_bytes < w.bytes) return LFS_E_WORKSPACE;
    const fgs::InstWs iw = fgs::inst_ws(instance_workspace, width, height, uint64_t(n_instances));
    if (!instance_workspace || instance_workspace_bytes < iw.bytes) return LFS_E_WORKSPACE;
    if (n_instances == 0 || N == 0) return LFS_OK;
    hipStream_t s = (hipStream_t)stream;
    const fgs::Frame f = fgs::make_frame(*view);
    const uint32_t T = f.gw * f.gh;
    lfs::ProfScope prof("fastgs_contribution", s);
    const uint32_t wgrid = cell_grid_blocks(uint64_t(T) * fgs::WPT, fgs::WPT);
    hipLaunchKernelGGL(fgs::fg_contrib_kernel, dim3(wgrid), dim3(64), 0, s, f.gw, f.gh, width, height, w.rec, w.offsets, iw.cell_count, iw.cell_list, stats);
    return (int)hipGetLastError();
}
