// wgrad_shared_body.inc — the body of conv1x1_wgrad_shared_kernel and conv1x1_wgrad_shared16_kernel (conv1x1_wgrad.hip): the
// piece tables, the fetch walk with its coefficient loads, the double-buffered stage loop and the register-tile epilogue.
// Included INTO each kernel, after `typedef ... STAGE;` (WgradStage32<BF> / WgradStage64: what differs) and
// `STAGE::Elem *const lds` = the kernel's dynamic LDS, [2][256][STAGE::LD]; reads PRO, POOLED, XT, YT and the kernel's arguments
// by name.  (Text and not a device function: see wgrad_tile_body.inc.)
    typedef typename STAGE::Elem Elem;
    typedef typename STAGE::Piece Piece;
    constexpr int YROWS = 128, ROWS = YROWS + 128, YJ = 4, XJ = 4, NJ = YJ + XJ; // pieces per thread: dy, x
    constexpr int RSTEP = 32;                                        // rows between a thread's pieces
    constexpr int POS = STAGE::POS, LD = STAGE::LD, PER = STAGE::PER;
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int i = lane & 15, k = lane >> 4;
    const int co0 = blockIdx.y * YROWS, ci0 = blockIdx.z * 128;
    const int half_r = wave >> 1, half_c = wave & 1;                 // this wavefront's 64 x 64 part of the tile
    const int stages_per_img = hw / POS;
    const long long nstages = (long long)batch * stages_per_img;
    const long long first = (long long)blockIdx.x * stages_per_wg;
    const int mine = (int)max(0LL, min((long long)stages_per_wg, nstages - first));
    if (mine == 0) return;                                           // (workgroup-uniform)

    // my pieces of a stage: piece q (PER positions) of rows rr + RSTEP j (j < YJ: dy rows, then XJ x rows), clamped onto the tensors
    const int q = t & 7, rr = t >> 3;
    int grow[NJ], lrow[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int r = rr + RSTEP * (j < YJ ? j : j - YJ);
        grow[j] = j < YJ ? min(co0 + r, cout - 1) : min(ci0 + r, cin - 1);
        lrow[j] = (j < YJ ? r : YROWS + r) * LD + PER * q;
    }
    const int centres = POOLED ? hw >> s_shift : 0;
    int cur_b = (int)(first / stages_per_img);
    int cur_off = (int)(first - (long long)cur_b * stages_per_img);

    Piece raw[NJ];
    float fa[XJ], fb[XJ];
    float2 cc[YJ], jv[YJ];
    int jpos = 0;
    auto fetch = [&]() { // the current stage into registers, then advance
        const int pos = cur_off * POS + PER * q;
        const YT *yb_ = dy + (size_t)cur_b * cout * hw + pos;
        const XT *xb_ = x + (size_t)cur_b * cin * hw + pos;
#pragma unroll
        for (int j = 0; j < YJ; ++j) raw[j] = STAGE::ld(yb_ + (size_t)grow[j] * hw);
#pragma unroll
        for (int j = YJ; j < NJ; ++j) raw[j] = STAGE::ld(xb_ + (size_t)grow[j] * hw);
        if constexpr (POOLED) { // a piece's positions lie inside one neighbourhood (S >= 16)
#pragma unroll
            for (int j = 0; j < YJ; ++j) {
                const size_t r = (size_t)cur_b * cout + grow[j];
                cc[j] = coef2[r];
                jv[j] = inj[r * centres + (pos >> s_shift)];
            }
            jpos = pos & ((1 << s_shift) - 1);
        }
        if constexpr (PRO) {
#pragma unroll
            for (int j = 0; j < XJ; ++j) {
                fa[j] = aff_a[(size_t)cur_b * cin + grow[YJ + j]];
                fb[j] = aff_b[(size_t)cur_b * cin + grow[YJ + j]];
            }
        }
        if (++cur_off == stages_per_img) { cur_off = 0; ++cur_b; }
    };
    auto park = [&](Elem *buf) { // transform (the expressions of conv1x1_wgrad_kernel) and store to LDS
#pragma unroll
        for (int j = 0; j < YJ; ++j) {
            Piece v = raw[j];
            STAGE::template park_y<POOLED>(v, cc[j], jv[j], jpos);
            *reinterpret_cast<Piece *>(buf + lrow[j]) = v;
        }
#pragma unroll
        for (int j = 0; j < XJ; ++j) {
            Piece v = raw[YJ + j];
            STAGE::template park_x<PRO>(v, fa[j], fb[j], pro_relu);
            *reinterpret_cast<Piece *>(buf + lrow[YJ + j]) = v;
        }
    };

    v4f acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][c] = (v4f){0.f, 0.f, 0.f, 0.f};
    const int yoff = (half_r * 64 + i) * LD + PER * k, xoff = (YROWS + half_c * 64 + i) * LD + PER * k;
    auto half_stage = [&](const Elem *buf, int h) { STAGE::half_stage(acc, buf, yoff, xoff, h); };

    Elem *buf0 = lds, *buf1 = lds + ROWS * LD;
    fetch();
    park(buf0);
    __syncthreads();
    for (int st = 0; st < mine; ++st) {
        const bool more = st + 1 < mine; // (workgroup-uniform)
        if (more) fetch();
        half_stage(buf0, 0);
        if (more) park(buf1);            // (buf1 was last read before the barrier that ended the previous stage)
        half_stage(buf0, 1);
        __syncthreads();
        Elem *tmp = buf0; buf0 = buf1; buf1 = tmp;
    }
    // C/D layout of 16x16x4: lane l holds rows (l >> 4) * 4 + r (r = 0..3) of column l & 15; workgroups add with fp32 atomics
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = co0 + half_r * 64 + a * 16 + k * 4 + r, col = ci0 + half_c * 64 + c * 16 + i;
                const float v = acc[a][c][r];
                wgrad_emit(dw, slab, row, col, cout, cin, v);
            }
