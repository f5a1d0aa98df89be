// kabsch.hip — batched 3x3 "Kabsch rotation": R = V diag(1, 1, det(V U^T)) U^T for S = U diag(s) V^T.
//
// Replaces the torch.svd call on (B*K, 3, 3) cross-covariances in the reference's weighted-Kabsch fit
// (losses/seg_loss_unsup.py:44-53).  rocSOLVER's batched SVD costs ~40 launches per call for 40 matrices; here one
// thread handles one matrix with a cyclic Jacobi eigen-solve of S^T S in fp64 (three sweeps reach machine
// precision for 3x3), recovers U column by column (with Gram-Schmidt completion for vanishing singular values) and
// forms R (ogc_kabsch3 in svd3.h, shared with rigid_icp.hip).  The rotation is unique whenever S has rank >= 2 and
// sigma_2 > sigma_3 is not needed for uniqueness of
// the product V diag(..) U^T; any correct SVD gives the same R up to rounding, so results agree with the reference
// to fp32 accuracy.  A matrix containing NaN/inf yields the identity (the reference's `valid_batches` rule, :38-42).
#include "ogc_common.h"
#include "svd3.h"

namespace {

__global__ void kabsch_rotation_kernel(int nb, const float *__restrict__ S_in, float *__restrict__ R_out,
                                       int *__restrict__ valid_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb) return;
    double S[3][3];
    bool finite = true;
    double scale = 0.0;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            const float v = S_in[i * 9 + r * 3 + c];
            finite = finite && isfinite(v);
            S[r][c] = v;
            scale = fmax(scale, fabs((double)v));
        }
    float *Ro = R_out + i * 9;
    if (valid_out) valid_out[i] = finite ? 1 : 0;
    if (!finite || scale == 0.0) { // ill-posed (NaN) -> identity; all-zero S: any rotation is optimal, torch gives I
        for (int k = 0; k < 9; ++k) Ro[k] = (k % 4 == 0) ? 1.0f : 0.0f;
        return;
    }
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) S[r][c] /= scale;
    double Rd[3][3];
    if (!ogc_kabsch3(S, Rd)) { // cannot happen for scale > 0, kept for safety
        for (int k = 0; k < 9; ++k) Ro[k] = (k % 4 == 0) ? 1.0f : 0.0f;
        return;
    }
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) Ro[r * 3 + c] = (float)Rd[r][c];
}

} // namespace

extern "C" int ogc_kabsch_rotation(int nb, const float *S, float *R, int *valid, ogc_stream_t stream) {
    OGC_REQUIRE(nb >= 0, "ogc_kabsch_rotation: negative batch");
    if (nb == 0) return OGC_OK;
    OGC_REQUIRE(S && R, "ogc_kabsch_rotation: null pointer");
    hipLaunchKernelGGL(kabsch_rotation_kernel, dim3(ogc_divup(nb, 64)), dim3(64), 0, (hipStream_t)stream, nb, S, R,
                       valid);
    OGC_CHECK_LAUNCH("ogc_kabsch_rotation");
    return OGC_OK;
}
