// moments_body.inc — the first part of the body of wgrad_moments_kernel and wgrad_moments16_kernel (gn_fused_bwd.hip): the wave's
// share of the steps of ONE sample, the accumulator pair, the clamped row tables, the pooled coefficients, and `load`, which
// fetches step `cur` and walks on towards `stop`.  The second part is moments_walk.inc: the ping-pong driver and the four-wave
// reduction of both matrices.  Between the two a kernel defines `fma`, the transform from what `load` fetched to MFMA operands
// with the products into acc1 (H) and acc2 (H2): the transform and the STEP (MomentStep16 / MomentStep32: the shape of a step)
// are what the two kernels differ in.
// Included INTO each kernel, after `typedef ... STEP;`, and reads the kernel's COB, CIB, POOLED, AT, FIRST, LIST, its arguments
// and `first`, `ls` by name.  Text and not a device function, as wgrad_tile_body.inc (see there for what a function cost), and
// apart from that file: its walk crosses samples and carries one accumulator set, and one file for both would branch on its
// caller.  The transform is text in its kernel for the same reason: as a function of the STEP (tried as a static member, called
// from a lambda or directly, and as a closure the STEP returns) the one of the 16-bit kernel changed the registers of 5 of its 16
// instantiations, three of them to another occupancy.
    typedef typename STEP::Raw Raw;
    constexpr int XN = FIRST ? FIRST : CIB; // loads of a lane per step in x's place
    __shared__ float red[WG_WAVES][COB * CIB * 256]; // one slab per wave (see conv1x1_wgrad_kernel), H then H2
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = lane & 15, k = lane >> 4;
    const int img = blockIdx.x / chunks, chunk = blockIdx.x - img * chunks;
    const int co0 = blockIdx.y * (16 * COB), ci0 = blockIdx.z * (16 * CIB);
    int steps_per_img = hw >> STEP::SHIFT;
    const int *lv_ = nullptr;
    if constexpr (LIST) {
        steps_per_img = min(ls.n[img], ls.cap); // entries of the list (>= 1: every centre keeps its first step)
        lv_ = ls.steps + (size_t)img * ls.cap;
        const int waves = chunks * WG_WAVES;
        steps_per_wave = ((steps_per_img + waves - 1) / waves + 1) & ~1;
        if (chunk * WG_WAVES * steps_per_wave >= steps_per_img) return; // (the whole workgroup, ahead of every barrier)
    }
    const int first_step = (chunk * WG_WAVES + wave) * steps_per_wave;
    const int mine = max(0, min(steps_per_wave, steps_per_img - first_step)); // this wavefront's steps: [first_step, first_step + mine)

    v4f acc1[COB][CIB], acc2[COB][CIB];
#pragma unroll
    for (int a = 0; a < COB; ++a)
#pragma unroll
        for (int c = 0; c < CIB; ++c) {
            acc1[a][c] = (v4f){0.f, 0.f, 0.f, 0.f};
            acc2[a][c] = (v4f){0.f, 0.f, 0.f, 0.f};
        }
    int yrow[COB], xrow[XN], jrow[COB];
    float ca[CIB], cb[CIB], pc2[COB], pc3[COB];
    float w1r[FIRST ? CIB : 1][FIRST ? FIRST : 1]; // FIRST: the rows of W1 of this lane's CIB channels (zeros beyond c0)
    const int centres = hw >> s_shift, smask = (1 << s_shift) - 1;
#pragma unroll
    for (int a = 0; a < COB; ++a) {
        const int row = min(co0 + a * 16 + i, cout - 1);
        yrow[a] = row * hw;
        if (POOLED) {
            const float2 cc = coef2[(size_t)img * cout + row];
            pc2[a] = cc.x;
            pc3[a] = cc.y;
            jrow[a] = row * centres;
        }
    }
    const float2 *jb_ = POOLED ? inj + (size_t)img * cout * centres : nullptr;
#pragma unroll
    for (int c = 0; c < CIB; ++c) {
        const int ch = min(ci0 + c * 16 + i, cin - 1);
        if constexpr (FIRST == 0) xrow[c] = ch * hw;
        ca[c] = aff_a[(size_t)img * cin + ch];
        cb[c] = aff_b[(size_t)img * cin + ch];
        if constexpr (FIRST > 0) {
#pragma unroll
            for (int e = 0; e < FIRST; ++e) w1r[c][e] = e < first.c0 ? first.w1[ch * first.c0 + min(e, first.c0 - 1)] : 0.f;
        }
    }
    if constexpr (FIRST > 0) { // one load shape per channel of x0; channels beyond c0 re-read the last one and are zeroed in the transform
#pragma unroll
        for (int e = 0; e < FIRST; ++e) xrow[e] = min(e, first.c0 - 1) * hw;
    }
    const AT *yb_ = dy + (size_t)img * cout * hw + STEP::PER * k;
    const AT *xb_ = FIRST ? reinterpret_cast<const AT *>(first.x0) + (size_t)img * first.c0 * hw + STEP::PER * k
                          : x + (size_t)img * cin * hw + STEP::PER * k;
    int cur = min(first_step, steps_per_img - 1);
    const int stop = min(first_step + mine, steps_per_img) - 1; // the walk stays on the wave's last step once it is reached
    // Unconditional loads of one shape (see conv1x1_wgrad_kernel: a load under a per-lane condition makes the compiler wait
    // for ALL outstanding loads wherever it needs one, which serialises the ping-pong): rows beyond the tensors are clamped
    // onto the last row — they only reach rows / columns of H, H2 that are never stored — and steps beyond the wave's
    // share re-read its last step and are not computed with.
    int ent = LIST ? lv_[cur] : 0; // LIST: the entry of step `cur` (wave-uniform), fetched one step ahead of its loads
    auto load = [&](Raw(&yv)[COB], Raw(&xv)[XN], float2(&jv)[COB], int &jpos, int &went) { // step `cur`, then advance
        const int pb = (LIST ? min(ent & LIVE_MASK, (hw >> STEP::SHIFT) - 1) : cur) * (1 << STEP::SHIFT);
        if constexpr (LIST) went = ent; // (wave-uniform: the weight is formed where it is used)
#pragma unroll
        for (int a = 0; a < COB; ++a) STEP::ld(yb_ + yrow[a] + pb, yv[a]);
#pragma unroll
        for (int c = 0; c < XN; ++c) STEP::ld(xb_ + xrow[c] + pb, xv[c]);
        if (POOLED) { // a lane's positions lie inside one neighbourhood (S >= 16)
#pragma unroll
            for (int a = 0; a < COB; ++a) jv[a] = jb_[jrow[a] + STEP::centre(pb, k, s_shift)];
            jpos = STEP::inside(pb, k, smask); // this lane's first position inside the neighbourhood
        }
        cur = min(cur + 1, max(stop, 0));
        if constexpr (LIST) ent = lv_[cur];
    };
