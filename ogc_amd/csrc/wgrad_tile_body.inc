// wgrad_tile_body.inc — the body of conv1x1_wgrad_kernel and conv1x1_wgrad16_kernel (conv1x1_wgrad.hip): the wave's share of
// the steps, the clamped row tables, the loads that travel with the step, the ping-pong driver and the four-wave reduction.
// Included INTO each kernel, after `typedef ... STEP;` (WgradStep16<BF> / WgradStep32: what differs), and reads the kernel's
// template parameters COB, CIB, PRO, POOLED, XT, YT and its arguments by name.  Text and not a device function: called as one
// (even with every line unchanged inside) the compiler allocated other registers for 47 of the 77 instantiations of the first
// kernel, several with one wavefront per SIMD less.
    typedef typename STEP::Raw Raw;
    // the four waves' partial tiles, one slab each (plain stores: ds_add_f32 sustains well under one lane per cycle), summed
    // by the threads that send them on
    __shared__ float red[WG_WAVES][COB * CIB * 256];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = lane & 15, k = lane >> 4;
    const int co0 = blockIdx.y * (16 * COB), ci0 = blockIdx.z * (16 * CIB);
    const int steps_per_img = hw >> STEP::SHIFT;
    const long long nsteps = (long long)batch * steps_per_img;
    const long long first = ((long long)blockIdx.x * WG_WAVES + wave) * steps_per_wave;
    // this wavefront's steps: [first, first + mine) — everything about the walk is wave-uniform (SALU, scalar branches)
    const int mine = (int)max(0LL, min((long long)steps_per_wave, nsteps - first));

    v4f acc[COB][CIB];
#pragma unroll
    for (int a = 0; a < COB; ++a)
#pragma unroll
        for (int c = 0; c < CIB; ++c) acc[a][c] = (v4f){0.f, 0.f, 0.f, 0.f};

    // The wave walks consecutive steps, so (image, position) advance incrementally: one division per wave instead of a
    // 64-bit division per step (which cost more issue slots than the step's 64 MFMAs).
    const long long start = min(first, nsteps - 1);
    int cur_b = (int)(start / steps_per_img);
    int cur_off = (int)(start - (long long)cur_b * steps_per_img);
    int left = mine - 1; // steps after the current one; the walk stays on the last step once they are used up
    int yrow[COB], xrow[CIB], coef[CIB]; // one sample's activation fits 32-bit offsets (checked by the entry point)
    constexpr int NP = POOLED ? COB : 1;
    int orow[NP];
    const int centres = hw >> s_shift, smask = (1 << s_shift) - 1;
#pragma unroll
    for (int a = 0; a < COB; ++a) {
        yrow[a] = min(co0 + a * 16 + i, cout - 1) * hw;
        if (POOLED) orow[a] = min(co0 + a * 16 + i, cout - 1);
    }
#pragma unroll
    for (int c = 0; c < CIB; ++c) {
        coef[c] = min(ci0 + c * 16 + i, cin - 1);
        xrow[c] = coef[c] * hw;
    }
    // EVERY load of a step is unconditional and of the same shape: rows beyond the tensors are clamped onto the last row
    // (they only feed rows / columns of the tile that are never stored), steps beyond the wave's share re-read its last
    // step and are not computed with.  A load under a per-lane condition (`row < cout ? *p : 0`) becomes its own
    // exec-masked block and the compiler then waits for ALL outstanding loads wherever it needs one — which serialised
    // the ping-pong below: the next step's loads were waited for before the current step's MFMAs (50 % of the time of
    // this kernel at one wavefront per SIMD).  PRO: the affine map of this lane's input channels travels WITH the step
    // (eight cached dword loads more) for the same reason: loaded only at image changes, its wait was a vmcnt(0).
    auto load = [&](Raw(&yv)[COB], Raw(&xv)[CIB], float(&fa)[CIB], float(&fb)[CIB], float2(&cc)[NP], float2(&jv)[NP],
                    int &jpos) { // current step, then advance
        const int pb = cur_off * (1 << STEP::SHIFT) + STEP::PER * k;
        const YT *yb_ = dy + (size_t)cur_b * cout * hw + pb;
        const XT *xb_ = x + (size_t)cur_b * cin * hw + pb;
#pragma unroll
        for (int a = 0; a < COB; ++a) STEP::ld(yb_ + yrow[a], yv[a]);
        if constexpr (POOLED) { // (travels with the step like the affine map below: the sample may change from step to step)
#pragma unroll
            for (int a = 0; a < COB; ++a) {
                const size_t r = (size_t)cur_b * cout + orow[a];
                cc[a] = coef2[r];
                jv[a] = inj[r * centres + (pb >> s_shift)];
            }
            jpos = pb & smask; // this lane's first position inside the neighbourhood (its PER positions lie inside one: S >= 16)
        }
#pragma unroll
        for (int c = 0; c < CIB; ++c) {
            STEP::ld(xb_ + xrow[c], xv[c]);
            if (PRO) {
                fa[c] = aff_a[(size_t)cur_b * cin + coef[c]];
                fb[c] = aff_b[(size_t)cur_b * cin + coef[c]];
            }
        }
        if (left > 0) {
            --left;
            if (++cur_off == steps_per_img) { cur_off = 0; ++cur_b; }
        }
    };
    auto fma = [&](const Raw(&yraw)[COB], const Raw(&xraw)[CIB], const float(&fa)[CIB], const float(&fb)[CIB],
                   const float2(&cc)[NP], const float2(&jv)[NP], int jpos) {
        STEP::template mfma<PRO, POOLED, XT>(acc, yraw, xraw, fa, fb, cc, jv, jpos, pro_relu);
    };

    Raw ya[COB], xa[CIB], yb[COB], xb[CIB];
    float faa[CIB], fba[CIB], fab[CIB], fbb[CIB];
    float2 cca[NP], ccb[NP], jva[NP], jvb[NP];
    int jpa = 0, jpb = 0;
    load(ya, xa, faa, fba, cca, jva, jpa);
    int s = 0;
    for (; s + 1 < mine; s += 2) {               // ping-pong registers: next step's loads fly during the MFMAs.  No branch inside
        load(yb, xb, fab, fbb, ccb, jvb, jpb);   // the loop body: with one, the accumulators travelled AGPR -> VGPR -> AGPR every round
        fma(ya, xa, faa, fba, cca, jva, jpa);
        load(ya, xa, faa, fba, cca, jva, jpa);
        fma(yb, xb, fab, fbb, ccb, jvb, jpb);
    }
    if (s < mine) fma(ya, xa, faa, fba, cca, jva, jpa);

    // C/D layout of 16x16x4: lane l holds rows (l >> 4) * 4 + r (r = 0..3) of column l & 15
#pragma unroll
    for (int a = 0; a < COB; ++a)
#pragma unroll
        for (int c = 0; c < CIB; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[wave][(a * CIB + c) * 256 + (k * 4 + r) * 16 + i] = acc[a][c][r];
    __syncthreads();
    for (int t = threadIdx.x; t < COB * CIB * 256; t += WG_WAVES * OGC_WAVE) {
        const int blk = t >> 8, a = blk / CIB, c = blk % CIB;
        const int row = co0 + a * 16 + ((t & 255) >> 4), col = ci0 + c * 16 + (t & 15);
        const float v = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
        wgrad_emit(dw, slab, row, col, cout, cin, v);
    }
