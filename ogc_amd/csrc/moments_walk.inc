// moments_walk.inc — the second part of the body of the two moment kernels (see moments_body.inc): the ping-pong driver over the
// wave's steps with the kernel's `fma`, then both matrices through the four waves' slabs to the atomics.
    Raw ya[COB], xa[XN], yb[COB], xb[XN];
    float2 ja[COB], jb[COB];
    int pa_ = 0, pb_ = 0;
    int wa_ = 0, wb_ = 0;
    load(ya, xa, ja, pa_, wa_);
    int s = 0;
    for (; s + 1 < mine; s += 2) { // ping-pong registers: next step's loads fly during the MFMAs (no branch in the body)
        load(yb, xb, jb, pb_, wb_);
        fma(ya, xa, ja, pa_, wa_);
        load(ya, xa, ja, pa_, wa_);
        fma(yb, xb, jb, pb_, wb_);
    }
    if (s < mine) fma(ya, xa, ja, pa_, wa_);

    float *dst = hm + (size_t)img * 2 * cout * cin;
#pragma unroll
    for (int which = 0; which < 2; ++which) {
        if (which) __syncthreads();
#pragma unroll
        for (int a = 0; a < COB; ++a)
#pragma unroll
            for (int c = 0; c < CIB; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r) // C/D layout: lane l holds rows (l >> 4) * 4 + r of column l & 15
                    red[wave][(a * CIB + c) * 256 + (k * 4 + r) * 16 + i] = which ? acc2[a][c][r] : acc1[a][c][r];
        __syncthreads();
        for (int t = threadIdx.x; t < COB * CIB * 256; t += WG_WAVES * OGC_WAVE) {
            const int blk = t >> 8, a = blk / CIB, c = blk % CIB;
            const int row = co0 + a * 16 + ((t & 255) >> 4), col = ci0 + c * 16 + (t & 15);
            const float v = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
            if (row < cout && col < cin && v != 0.0f) unsafeAtomicAdd(dst + ((size_t)which * cout + row) * cin + col, v);
        }
    }
