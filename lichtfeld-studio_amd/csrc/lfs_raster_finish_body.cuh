// The body of the one-round-trip finish pass, included as TEXT into its kernels - raster_finish_adam_kernel<ADAM> (raster.hip: DENSIFY = false, radii = dens = nullptr) and
// raster_finish_densify_kernel (raster_densify.hip: ADAM = false, DENSIFY = true). Text, not a __device__ function template: as a function inlined into the two default
// kernels the same statements came out with commuted s_or operands and two swapped instructions - the same registers and sizes, not the same bytes - and
// tools/code_object_identity.py against the build before is how an edit here shows that the default forms did not change.
// Names the including kernel provides: ADAM, DENSIFY (constant expressions), N, means, raw_scales, raw_quats, raw_opacities, quats, scales, opacities, cams, acc, v_dirs, ad,
// gr, loss_slots, loss, abort_flag, radii, dens.
    static_assert(!(ADAM && DENSIFY), "the densifying form is a gradient-tensor form");
    int32_t rad[2] = {0, 0};
    float dn[2] = {0.f, 0.f};
#ifndef LFS_EMULATE
    // ONE memory round trip per wavefront (round 6). The form before had four in series - abort-flag pointer -> flag -> the accumulator rows (their LDS hand-over
    // sits behind a scheduling barrier no load may cross) -> the other 21 loads (two of them issued late, behind the first arithmetic) - in a kernel whose 29 streams
    // reach 5.1 TB/s in a trivial pass (tools/hbm_stream.hip: multi_rmw_32_streams) and that ran at 3.1 - 3.7. Here every load of the pass is issued before the first
    // wait, through (SGPR base, 32-bit byte offset) addresses - three offset registers instead of a 64-bit address pair per stream - and the abort flag is looked at
    // where it matters: in front of the stores.
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = gid < N;
    const uint32_t g = live ? gid : (N - 1u);              // (tail lanes read the last row: no branch around the loads)
    const uint32_t o4 = g << 2, o12 = g * 12u, o16 = g << 4;
    auto at = [](const void* base, uint32_t byte_off) { return reinterpret_cast<const char*>(base) + byte_off; };
    auto ld3o = [&](const float* base, float (&dst)[3]) { const V3f t = *reinterpret_cast<const V3f*>(at(base, o12)); dst[0] = t.a[0]; dst[1] = t.a[1]; dst[2] = t.a[2]; };
    auto ld4o = [&](const float* base) { return *reinterpret_cast<const float4*>(at(base, o16)); };
    auto ld1o = [&](const float* base) { return *reinterpret_cast<const float*>(at(base, o4)); };
    int32_t aborted = 0;
    if (ADAM && abort_flag != nullptr) aborted = *abort_flag; // (scalar load: in flight with everything else)
    // the 64 accumulator rows of a wavefront (4 KB contiguous) as four fully coalesced 1-KB loads, handed to their lanes through a wave-private LDS block below
    // (row stride 20 floats: 16-byte aligned, conflict-free on the read side) instead of four 16-byte loads per lane at a 64-byte stride: finish_adam 0.106 / 0.102 -> 0.102 / 0.097 ms
    // (round 3, profiles/r03/finish_lds_rows_ab.txt)
    __shared__ float4 s_rows[FINISH_BLOCK / 64][64 * 5];
    float4* const rows = s_rows[threadIdx.x >> 6];
    const uint32_t lane = threadIdx.x & 63, g0 = (blockIdx.x * blockDim.x + threadIdx.x) - lane;
    float4 t_rows[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { // (rows past the end: the last row again - an address clamp instead of a branch around the load)
        const uint32_t idx = i * 64 + lane, row = min(g0 + (idx >> 2), N - 1u);
        t_rows[i] = *reinterpret_cast<const float4*>(at(acc, (row << 6) + ((idx & 3u) << 4)));
    }
    float mu_a[3], sc[3], vd[3] = {0.f, 0.f, 0.f};
    ld3o(means, mu_a); ld3o(scales, sc);
    if (ADAM || v_dirs != nullptr) ld3o(v_dirs, vd);   // (gradient-tensor form: nullable - the SH backward then adds dL/d(dirs) onto g_means afterwards)
    const float4 q = ld4o(quats), rq = ld4o(raw_quats);
    const float o = ld1o(opacities);
    float m0[3] = {0.f, 0.f, 0.f}, v0[3] = {0.f, 0.f, 0.f}, p1[3] = {0.f, 0.f, 0.f}, m1[3] = {0.f, 0.f, 0.f}, v1[3] = {0.f, 0.f, 0.f};
    float4 mq = make_float4(0.f, 0.f, 0.f, 0.f), vq4 = mq;
    float po = 0.f, mo = 0.f, vo = 0.f;
    if (ADAM) {
        ld3o(ad.m[0], m0); ld3o(ad.v[0], v0); ld3o(raw_scales, p1); ld3o(ad.m[1], m1); ld3o(ad.v[1], v1);
        mq = ld4o(ad.m[2]); vq4 = ld4o(ad.v[2]);
        po = ld1o(raw_opacities); mo = ld1o(ad.m[3]); vo = ld1o(ad.v[3]);
    }
    if (DENSIFY) {   // the radii pair and the two current rows of the statistic
        const int2 r2 = *reinterpret_cast<const int2*>(at(radii, g << 3));
        rad[0] = r2.x; rad[1] = r2.y;
        dn[0] = ld1o(dens); dn[1] = ld1o(dens + N);
    }
    float loss_v = 0.f;
    if (loss_slots != nullptr && blockIdx.x == 0) loss_v = threadIdx.x < LOSS_SLOTS ? loss_slots[threadIdx.x] : 0.f;   // (LOSS_SLOTS = 256: the first four wavefronts carry the slots)
    // ---- everything is in flight; from here on the pass only consumes (the accumulator rows were requested first and are the first to be waited for) ----
#pragma unroll
    for (int i = 0; i < 4; ++i) { const uint32_t idx = i * 64 + lane; rows[(idx >> 2) * 5 + (idx & 3)] = t_rows[i]; }
    __builtin_amdgcn_wave_barrier();
    if (loss_slots != nullptr && blockIdx.x == 0) { // *loss = the fused MSE (a store in a fixed order: the step needs no zeroed accumulator)
        __shared__ float wave_sum[FINISH_BLOCK / 64];
        float v = loss_v;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
        if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = v;
        __syncthreads();
        if (threadIdx.x == 0 && aborted == 0) {
            const float total = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
            if (ADAM) *loss = total; else if (total != 0.f) unsafeAtomicAdd(loss, total);
        }
    }
    if (!live || aborted != 0) return; // (aborted: uniform) speculative step that did not fit its buffers: no update, the host runs it again
    float vm[3] = {0.f, 0.f, 0.f}, vq[4] = {0.f, 0.f, 0.f, 0.f}, vs[3] = {0.f, 0.f, 0.f};
    const float4* a4 = rows + lane * 5;
    const float4 a0 = a4[0], a1 = a4[1], a2 = a4[2], a3 = a4[3];
    const float A[9] = {a0.x * REC_UNSCALE, a0.y * REC_UNSCALE, a0.z * REC_UNSCALE, a0.w * REC_UNSCALE, a1.x * REC_UNSCALE, a1.y * REC_UNSCALE, a1.z * REC_UNSCALE,
                        a1.w * REC_UNSCALE, a2.x * REC_UNSCALE};
    const f3 G{-a2.y * REC_UNSCALE, -a2.z * REC_UNSCALE, -a2.w * REC_UNSCALE};
    bool any = G.x != 0.f || G.y != 0.f || G.z != 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) any |= A[k] != 0.f;
    const f3 mu{mu_a[0], mu_a[1], mu_a[2]};
    auto st3a = [&](float* base, const float (&src)[3]) { V3f t; t.a[0] = src[0]; t.a[1] = src[1]; t.a[2] = src[2]; *reinterpret_cast<V3f*>(const_cast<char*>(at(base, o12))) = t; };
    auto ld3a = [&](const float* base, float (&dst)[3]) { ld3o(base, dst); };
    const float v_opac = a3.x != 0.f ? a3.x / o : 0.f;
#else   // LFS_EMULATE: the emulator switches lanes only at cross-lane operations, so it has no wave-private LDS hand-over - the same pass with plain per-lane loads
    if (ADAM && abort_flag != nullptr && *abort_flag != 0) return; // (uniform) speculative step that did not fit its buffers: no update, the host runs it again
    if (loss_slots != nullptr && blockIdx.x == 0) { // *loss = the fused MSE (a store in a fixed order: the step needs no zeroed accumulator)
        __shared__ float wave_sum[FINISH_BLOCK / 64];
        float v = threadIdx.x < LOSS_SLOTS ? loss_slots[threadIdx.x] : 0.f;   // (LOSS_SLOTS = 256: the first four wavefronts carry the slots whatever the block size)
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
        if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = v;
        __syncthreads();
        if (threadIdx.x == 0) {
            const float total = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
            if (ADAM) *loss = total; else if (total != 0.f) unsafeAtomicAdd(loss, total);
        }
    }
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= N) return;
    float vm[3] = {0.f, 0.f, 0.f}, vq[4] = {0.f, 0.f, 0.f, 0.f}, vs[3] = {0.f, 0.f, 0.f};
    const float4* a4 = reinterpret_cast<const float4*>(acc + size_t(gid) * ACC_STRIDE);
    const float4 a0 = a4[0], a1 = a4[1], a2 = a4[2], a3 = a4[3];
    // the row was accumulated against the scaled record (lfs_raster_common.cuh): A' = c A, G' = c G, slot 12 = opac * dL/dopac (divided where `o` is loaded)
    const float A[9] = {a0.x * REC_UNSCALE, a0.y * REC_UNSCALE, a0.z * REC_UNSCALE, a0.w * REC_UNSCALE, a1.x * REC_UNSCALE, a1.y * REC_UNSCALE, a1.z * REC_UNSCALE,
                        a1.w * REC_UNSCALE, a2.x * REC_UNSCALE};
    const f3 G{-a2.y * REC_UNSCALE, -a2.z * REC_UNSCALE, -a2.w * REC_UNSCALE};
    bool any = G.x != 0.f || G.y != 0.f || G.z != 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) any |= A[k] != 0.f;
    // (lfs_math.cuh ld3 / st3: three floats as one 12-byte access)
    auto ld3a = [&](const float* base, float (&dst)[3]) { const f3 t = ld3(base, gid); dst[0] = t.x; dst[1] = t.y; dst[2] = t.z; };
    auto st3a = [&](float* base, const float (&src)[3]) { st3(base, gid, f3{src[0], src[1], src[2]}); };
    float sc[3], vd[3] = {0.f, 0.f, 0.f};
    const f3 mu = ld3(means, gid);
    ld3a(scales, sc);
    if (ADAM || v_dirs != nullptr) ld3a(v_dirs, vd);   // (gradient-tensor form: nullable - the SH backward then adds dL/d(dirs) onto g_means afterwards)
    // Every operand of the pass is requested HERE, before any arithmetic (round 3): the kernel used to fetch in three dependent phases (rows -> quaternion
    // inside `if (any)` -> moments), which left each wavefront with 3 - 7 loads in flight and the kernel at 3.5 TB/s. The geometry vjp below now runs for
    // every Gaussian and is SELECTED by `any` (un-touched Gaussians keep exact zeros; their 1/scale may be inf), so no load hides behind a branch.
    const float4 q = reinterpret_cast<const float4*>(quats)[gid];
    const float4 rq = reinterpret_cast<const float4*>(raw_quats)[gid];
    const float o = opacities[gid];
    const float v_opac = a3.x != 0.f ? a3.x / o : 0.f;
    float m0[3] = {0.f, 0.f, 0.f}, v0[3] = {0.f, 0.f, 0.f}, p1[3] = {0.f, 0.f, 0.f}, m1[3] = {0.f, 0.f, 0.f}, v1[3] = {0.f, 0.f, 0.f};
    float4 mq = make_float4(0.f, 0.f, 0.f, 0.f), vq4 = mq;
    float po = 0.f, mo = 0.f, vo = 0.f;
    if (ADAM) {
        ld3a(ad.m[0], m0); ld3a(ad.v[0], v0); ld3a(raw_scales, p1); ld3a(ad.m[1], m1); ld3a(ad.v[1], v1);
        mq = reinterpret_cast<const float4*>(ad.m[2])[gid]; vq4 = reinterpret_cast<const float4*>(ad.v[2])[gid];
        po = raw_opacities[gid]; mo = ad.m[3][gid]; vo = ad.v[3][gid];
    }
    if (DENSIFY) { rad[0] = radii[2 * gid]; rad[1] = radii[2 * gid + 1]; dn[0] = dens[gid]; dn[1] = dens[size_t(N) + gid]; }
#endif // LFS_EMULATE
    { // exactly raster_finish_kernel<true> for C == 1 (selected by `any` at the end)
        const float is[3] = {1.f / sc[0], 1.f / sc[1], 1.f / sc[2]};
        finish_geometry<true>(q, is, A, G, mu, cams[0], vm, vq, vs);
#pragma unroll
        for (int k = 0; k < 3; ++k) { vm[k] = any ? vm[k] : 0.f; vs[k] = any ? vs[k] : 0.f; }
#pragma unroll
        for (int k = 0; k < 4; ++k) vq[k] = any ? vq[k] : 0.f;
    }
    {
#pragma clang fp contract(off)
        // + dL/d(dirs) of the SH backward (sh.hip adds it onto the rasterizer's dL/dmeans in the separate path)
        float gm[3] = {vm[0] + vd[0], vm[1] + vd[1], vm[2] + vd[2]};
        // activations_bwd_kernel<false> (l2_fused.hip)
        const float nrm = sqrtf(rq.x * rq.x + rq.y * rq.y + rq.z * rq.z + rq.w * rq.w);
        float gq[4];
        if (nrm > 1e-12f) {
            const float inv = 1.f / nrm;
            const float y[4] = {rq.x * inv, rq.y * inv, rq.z * inv, rq.w * inv};
            const float d = vq[0] * y[0] + vq[1] * y[1] + vq[2] * y[2] + vq[3] * y[3];
#pragma unroll
            for (int k = 0; k < 4; ++k) gq[k] = (vq[k] - d * y[k]) * inv;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) gq[k] = vq[k] * 1e12f;
        }
        float gs[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) gs[k] = (vs[k] + ad.scale_reg) * sc[k];
        const float go = (v_opac + ad.opacity_reg) * o * (1.f - o);
        if (!ADAM) { // gradient tensors out (activations_bwd_kernel's stores; dL/dmeans = the rasterizer's part, the SH backward adds the rest)
            const float v_col[3] = {a3.y, a3.z, a3.w};
            if (gr.v_colors != nullptr) st3a(gr.v_colors, v_col);
            float4* gqo = reinterpret_cast<float4*>(gr.g_quats) + gid;
            if (gr.accumulate) {
                float om[3], os[3];
                ld3a(gr.g_means, om); ld3a(gr.g_scales, os);
                const float4 oq = *gqo;
#pragma unroll
                for (int k2 = 0; k2 < 3; ++k2) { gm[k2] = om[k2] + gm[k2]; gs[k2] = os[k2] + gs[k2]; }
                gq[0] = oq.x + gq[0]; gq[1] = oq.y + gq[1]; gq[2] = oq.z + gq[2]; gq[3] = oq.w + gq[3];
                st3a(gr.g_means, gm); st3a(gr.g_scales, gs);
                *gqo = make_float4(gq[0], gq[1], gq[2], gq[3]);
                gr.g_opac[gid] += go;
            } else {
                st3a(gr.g_means, gm); st3a(gr.g_scales, gs);
                *gqo = make_float4(gq[0], gq[1], gq[2], gq[3]);
                gr.g_opac[gid] = go;
            }
            if (DENSIFY) {   // (this lane is live: tail lanes, which hold the last row's operands, returned above and do not add twice)
                const CamDev& cam = cams[0];
                const m3& Ri = cam.Rinv;
                const float gcx = Ri.m[0][0] * vm[0] + Ri.m[1][0] * vm[1] + Ri.m[2][0] * vm[2];
                const float gcy = Ri.m[0][1] * vm[0] + Ri.m[1][1] * vm[1] + Ri.m[2][1] * vm[2];
                const float dx = mu.x - cam.origin.x, dy = mu.y - cam.origin.y, dz = mu.z - cam.origin.z;
                const float z = Ri.m[0][2] * dx + Ri.m[1][2] * dy + Ri.m[2][2] * dz;
                const float sx = (gcx * z) * (float(cam.width) / (2.f * cam.fx)), sy = (gcy * z) * (float(cam.height) / (2.f * cam.fy));
                const float s = sqrtf(sx * sx + sy * sy);
                const bool visible = rad[0] > 0 && rad[1] > 0;
                dens[gid] = dn[0] + (visible ? 1.f : 0.f);
                dens[size_t(N) + gid] = dn[1] + (visible ? s : 0.f);
            }
            return;
        }
        // Adam (adam_multi_kernel's per-element update). Every moment is loaded before the first store (the moment arrays hang off a struct: no
        // __restrict__, a load could not move above an earlier store) and three-float rows move as 12-byte accesses (lfs_math.cuh). Measured on
        // one box against the element-by-element version: no difference (0.094 - 0.104 ms either way; the kernel walks 29 streams)
        float p[3] = {mu.x, mu.y, mu.z};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            adam_elem(p[k], m0[k], v0[k], gm[k], ad.s[0]);
            adam_elem(p1[k], m1[k], v1[k], gs[k], ad.s[1]);
        }
        float pq[4] = {rq.x, rq.y, rq.z, rq.w};
        adam_elem(pq[0], mq.x, vq4.x, gq[0], ad.s[2]); adam_elem(pq[1], mq.y, vq4.y, gq[1], ad.s[2]);
        adam_elem(pq[2], mq.z, vq4.z, gq[2], ad.s[2]); adam_elem(pq[3], mq.w, vq4.w, gq[3], ad.s[2]);
        adam_elem(po, mo, vo, go, ad.s[3]);
        st3a(means, p); st3a(ad.m[0], m0); st3a(ad.v[0], v0);
        st3a(raw_scales, p1); st3a(ad.m[1], m1); st3a(ad.v[1], v1);
        reinterpret_cast<float4*>(raw_quats)[gid] = make_float4(pq[0], pq[1], pq[2], pq[3]);
        reinterpret_cast<float4*>(ad.m[2])[gid] = mq; reinterpret_cast<float4*>(ad.v[2])[gid] = vq4;
        raw_opacities[gid] = po; ad.m[3][gid] = mo; ad.v[3][gid] = vo;
    }
