/*
 * ogc_ops.h — C ABI of libogc_ops.so, the MI355X (gfx950) implementation of OGC's
 * point-cloud operator stack.
 *
 * This is the drop-in boundary for the reference's native extension `pointnet2_cuda`
 * (PYBIND11_MODULE in pointnet2/src/pointnet2_api.cpp:10-25).  Every entry point below
 * replaces exactly one of the ten pybind functions registered there; the argument order
 * and meaning are the reference's, with `at::Tensor` replaced by raw device pointers and
 * the implicit "current CUDA stream" replaced by an explicit hipStream_t (passed as
 * void* so that this header has no HIP dependency).
 *
 * Contract shared by all entry points (reference: SURVEY.md §8b):
 *   - all tensors are dense, row-major, contiguous device memory; floats are fp32,
 *     indices are int32; dims are passed as int (flat offsets must fit in 32 bits);
 *   - the CALLER allocates every output and scratch buffer and keeps ownership;
 *   - launches are asynchronous on `stream`; no global state; re-entrant;
 *   - return value: OGC_OK (0) or a negative OGC_ERR_* code.  Unlike the reference
 *     (which prints and calls exit(-1), e.g. ball_query_gpu.cu:62-66) nothing here ever
 *     terminates the process; ogc_last_error() gives a thread-local message.
 *
 * Distance arithmetic everywhere is the reference's source expression evaluated in fp32,
 * left to right, WITHOUT fused multiply-add:
 *     d = (ux-x)*(ux-x) + (uy-y)*(uy-y) + (uz-z)*(uz-z)
 * (interpolate_gpu.cu:40, ball_query_gpu.cu:33, sampling_gpu.cu:133).
 */
#ifndef OGC_OPS_H
#define OGC_OPS_H

#ifdef __cplusplus
extern "C" {
#endif

typedef void *ogc_stream_t; /* hipStream_t */
typedef unsigned short ogc_bf16_t; /* one bfloat16 (the upper half of an fp32), storage only: the `_h` entry points */

enum {
    OGC_OK = 0,
    OGC_ERR_INVALID_ARG = -1, /* null pointer, negative dim, k out of range ... */
    OGC_ERR_LAUNCH = -2,      /* hipGetLastError() != hipSuccess after the launch */
    OGC_ERR_UNSUPPORTED = -3  /* shape outside what the kernels handle */
};

/* Library version (major*10000 + minor*100 + patch) and last error text (thread-local).  OGC_VERSION is the version of THIS
 * header; a caller checks ogc_version() == OGC_VERSION before anything else (ogc_amd/_lib.py does): the minor number moves with
 * every change of an existing prototype.  0.2.0: ogc_adam_step takes its five hyper-parameters as double (float before), new
 * entry points ogc_zero_arena_begin / _end, ogc_conv1x1_gemm_any, ogc_conv1x1_wgrad_affine_pooled, ogc_conv1x1_dgrad_pooled.  0.2.1 (the patch number moves with new entry
 * points): ogc_gather_xyz_pair, ogc_flow_advance, ogc_linear_cn, ogc_gru_reset, ogc_gru_blend,
 * ogc_soft_corr_flow, ogc_three_nn_weights; ogc_furthest_point_sampling_chain accepts temp == NULL.  0.2.2: the `_h` entry points
 * (activations of the shared MLPs stored as bf16; see "16-bit activations" at the end of this header).  0.2.4: ogc_set_deterministic /
 * ogc_get_deterministic.  0.2.5: ogc_group_linear_fwd_direct.  0.2.6: ogc_rigid_icp.
 * 0.2.7: ogc_ground_plane_fit.
 * 0.2.8: ogc_seg_eval.  ogc_flow_eval added under 0.2.8: no prototype changed, and the number is pinned by a test of that release.
 * The supervised mask loss (ogc_sup_loss_ws_doubles, ogc_sup_match_cost, ogc_sup_mask_loss_fwd / _bwd) likewise: new entry points
 * only, and two tests of 0.2.8 pin the number.  ogc_seg_eval_ignore likewise: a new entry point, ogc_seg_eval unchanged.
 * ogc_soft_carry likewise: a new entry point, no prototype changed.  ogc_scan_crop_camera / _front / _tile and ogc_box_segm /
 * _chunk likewise.  ogc_kittisf_unproject and ogc_png_unfilter likewise.  ogc_live_steps_fwd, ogc_conv1x1_gemm_affine_first_live
 * and ogc_conv1x1_gemm_affine_pool_live likewise.  ogc_moving_stats / _label_cap likewise.  ogc_surface_candidates, ogc_surface_thin /
 * _ws_bytes and ogc_nearest_label likewise.  ogc_depth_render / _ws_bytes / _timed and ogc_depth_points likewise.
 * ogc_slot_confidence likewise.  ogc_room_compose and ogc_mesh_apply_poses likewise. */
#define OGC_VERSION 208
int ogc_version(void);
/* 0: the squared distance of every search is the reference's SOURCE expression, ((dx*dx) + (dy*dy)) + (dz*dz), one rounding per
 * operation (what all parity tests pin).  1: this is libogc_ops_fmad.so, the same library with the search kernels (FPS, kNN,
 * three-NN, ball query) compiled to evaluate fma(dz, dz, fma(dy, dy, dx*dx)) — what `nvcc --fmad=true`, the reference's build,
 * makes of that expression (pointnet2/setup.py has no -fmad=false); for comparisons against index tensors produced by the real
 * CUDA binary on tie-heavy data.  Opt-in: OGC_FMAD=1 in the environment of ogc_amd. */
int ogc_distance_contracted(void);
/* The deterministic-gradient mode (csrc/det.hip; OGC_DETERMINISTIC=1 in the environment of ogc_amd sets it at load time).  The
 * reference accumulates gradients with float atomics (pointnet2/src/group_points_gpu.cu:24, interpolate_gpu.cu:211-213,
 * sampling_gpu.cu:62): their order, and so the last bits of every sum, change from launch to launch — as do this library's fast
 * kernels.  With the mode on, the entry points below form every sum in a FIXED order (bit-identical results from run to run and
 * from process to process on one device and build), slower, same contracts otherwise:
 *   scatter-adds as gathers over ascending position lists — ogc_group_points_grad, ogc_gather_points_grad, ogc_group_concat_grad,
 *     ogc_group_linear_bwd, ogc_three_interpolate_grad, ogc_chamfer_terms_grad; the transposed lists of ogc_group_reverse and
 *     ogc_reverse_neighbours come out sorted, which fixes the order inside ogc_group_points_grad_rev*, ogc_three_interpolate_grad_rev*
 *     and ogc_neighbour_consistency_bwd;
 *   per-workgroup partials + one ordered pass — the weight gradients ogc_conv1x1_wgrad* (all forms), the BatchNorm statistics and
 *     gradient sums of ogc_batch_norm_fwd / _bwd / _maxpool_fwd / _maxpool_bwd.
 * Not converted (the GroupNorm statistics taken in convolution epilogues, the moment matrices of ogc_conv1x1_wgrad_moments*): the
 * host layers route around them while the mode is on (ogc_amd/fused.py, DETERMINISTIC).  Forward results do not depend on the mode
 * except through BatchNorm's batch statistics (fp64 sums, now in slab order). */
int ogc_set_deterministic(int on);
int ogc_get_deterministic(void);
const char *ogc_last_error(void);

/* ---- furthest point sampling -------------------------------------------------------
 * replaces furthest_point_sampling_wrapper(b, n, m, points, temp, idx)
 *   pointnet2/src/sampling.cpp:38-49 -> sampling_gpu.cu:93-253
 * xyz (b,n,3) f32; temp (b,n) f32 scratch, must arrive filled with 1e10 (pointnet2.py:33),
 * left holding the final min-distances; idx (b,m) i32, idx[:,0] = 0.
 * Tie order among equal maxima reproduces the reference's block reduction for
 * block_size = min(1024, 2^floor(log2 n)) (cuda_utils.h:10-14). */
int ogc_furthest_point_sampling(int b, int n, int m, const float *xyz, float *temp,
                                int *idx, ogc_stream_t stream);

/* Furthest point sampling along a CHAIN of levels (utils/pointnet2_util.py:22-27 and utils/flowstep3d_util.py:112-118
 * sample level l+1 from the centres of level l, which are stored in sampling order).
 * ties_out (b) i32, optional: the first round of this run in which more than one point attained the maximum (exact
 * fp32 ties: duplicated points, lattices, and — late in a run that keeps a large share of the cloud — chance
 * coincidences), INT_MAX if there was none.
 * ties_in (b) i32, optional: ties_out of the run that PRODUCED this cloud (xyz = its first n samples, in sampling
 * order).  Where ties_in[i] >= m the result is known without sampling: every one of the parent's first m rounds picked
 * the unique farthest point from its earlier samples in the whole cloud, so inside the subset sample r is still the
 * unique farthest point from samples 0..r-1 — the answer is 0, 1, ..., m-1 (written directly; temp is left untouched
 * and ties_out[i] = ties_in[i], so the chain can go on).  Otherwise the rounds are run as usual, so the result is in
 * every case the one ogc_furthest_point_sampling returns.  Clouds of more than 16384 points are always sampled and
 * report ties_out = 0 (nothing known).
 * temp may be NULL for clouds of up to 16384 points (0.2.1): the running minima start at 1e10, stay in registers and are not
 * handed back — what every caller of the reference does with them (pointnet2.py:33-35 allocates, fills and drops temp), without the
 * fill launch and the (b, n) buffer. */
int ogc_furthest_point_sampling_chain(int b, int n, int m, const float *xyz, float *temp, int *idx,
                                      const int *ties_in, int *ties_out, ogc_stream_t stream);

/* ---- gather -------------------------------------------------------------------------
 * replaces gather_points_wrapper(b, c, n, npoints, points, idx, out)
 *   sampling.cpp:11-21 -> sampling_gpu.cu:8-43
 * out[b,c,j] = points[b,c,idx[b,j]];  points (b,c,n), idx (b,npoints), out (b,c,npoints) */
int ogc_gather_points(int b, int c, int n, int npoints, const float *points, const int *idx,
                      float *out, ogc_stream_t stream);

/* replaces gather_points_grad_wrapper(b, c, n, npoints, grad_out, idx, grad_points)
 *   sampling.cpp:24-35 -> sampling_gpu.cu:46-90
 * grad_points[b,c,idx[b,j]] += grad_out[b,c,j]; caller zero-fills grad_points (pointnet2.py:73) */
int ogc_gather_points_grad(int b, int c, int n, int npoints, const float *grad_out,
                           const int *idx, float *grad_points, ogc_stream_t stream);

/* ---- k nearest neighbours ----------------------------------------------------------
 * replaces knn_wrapper(b, n, m, k, unknown, known, dist2, idx)
 *   interpolate.cpp:26-36 -> interpolate_gpu.cu:9-79
 * unknown (b,n,3), known (b,m,3); dist2 (b,n,k) SQUARED distances ascending, idx (b,n,k).
 * Ties keep the lower index first; if m < k the tail is idx=0, dist2=+inf; non-finite
 * distances are never selected.  1 <= k <= 200 (the reference's scratch-array bound,
 * interpolate_gpu.cu:30-31); larger k returns OGC_ERR_INVALID_ARG instead of overrunning. */
int ogc_knn(int b, int n, int m, int k, const float *unknown, const float *known,
            float *dist2, int *idx, ogc_stream_t stream);

/* replaces three_nn_wrapper(b, n, m, unknown, known, dist2, idx)
 *   interpolate.cpp:14-23 -> interpolate_gpu.cu:81-146 ; k = 3 special case of ogc_knn */
int ogc_three_nn(int b, int n, int m, const float *unknown, const float *known, float *dist2,
                 int *idx, ogc_stream_t stream);

/* ---- three-point interpolation -----------------------------------------------------
 * replaces three_interpolate_wrapper(b, c, m, n, points, idx, weight, out)
 *   interpolate.cpp:39-52 -> interpolate_gpu.cu:149-189
 * out[b,c,i] = w[b,i,0]*p[b,c,idx[b,i,0]] + w[b,i,1]*p[..1] + w[b,i,2]*p[..2], left to right
 * points (b,c,m), idx/weight (b,n,3), out (b,c,n) */
int ogc_three_interpolate(int b, int c, int m, int n, const float *points, const int *idx,
                          const float *weight, float *out, ogc_stream_t stream);

/* replaces three_interpolate_grad_wrapper(b, c, n, m, grad_out, idx, weight, grad_points)
 *   interpolate.cpp:55-68 -> interpolate_gpu.cu:192-232
 * grad_points[b,c,idx[b,i,j]] += grad_out[b,c,i]*w[b,i,j]; caller zero-fills (pointnet2.py:181) */
int ogc_three_interpolate_grad(int b, int c, int n, int m, const float *grad_out,
                               const int *idx, const float *weight, float *grad_points,
                               ogc_stream_t stream);

/* ---- grouping ------------------------------------------------------------------------
 * replaces group_points_wrapper(b, c, n, npoints, nsample, points, idx, out)
 *   group_points.cpp:26-36 -> group_points_gpu.cu:47-86
 * out[b,c,p,s] = points[b,c,idx[b,p,s]]; points (b,c,n), idx (b,npoints,nsample) */
int ogc_group_points(int b, int c, int n, int npoints, int nsample, const float *points,
                     const int *idx, float *out, ogc_stream_t stream);

/* replaces group_points_grad_wrapper(b, c, n, npoints, nsample, grad_out, idx, grad_points)
 *   group_points.cpp:11-23 -> group_points_gpu.cu:8-44
 * grad_points[b,c,idx[b,p,s]] += grad_out[b,c,p,s]; caller zero-fills (pointnet2.py:224) */
int ogc_group_points_grad(int b, int c, int n, int npoints, int nsample, const float *grad_out,
                          const int *idx, float *grad_points, ogc_stream_t stream);

/* ---- ball query ------------------------------------------------------------------------
 * replaces ball_query_wrapper(b, n, m, radius, nsample, new_xyz, xyz, idx)
 *   ball_query.cpp:16-27 -> ball_query_gpu.cu:9-66
 * xyz (b,n,3) candidates, new_xyz (b,m,3) centres, idx (b,m,nsample).  Row = first nsample
 * indices k (ascending) with d2(k) < radius*radius, padded with the first hit; a centre with
 * no hit gets an all-zero row.  The reference's kernel leaves such rows untouched and relies
 * on the caller's pre-zeroed buffer (pointnet2.py:251); this one WRITES EVERY ROW, so idx may
 * be uninitialised memory (a pre-zeroed buffer works unchanged). */
int ogc_ball_query(int b, int n, int m, float radius, int nsample, const float *new_xyz,
                   const float *xyz, int *idx, ogc_stream_t stream);

/* ==== fused extensions (no counterpart in the reference's native module; they replace
 * Python-level op sequences of the reference, cited per function) ======================= */

/* kNN followed by the radius clamp every reference caller applies in Python
 *   pointnet2/pointnet2.py:283-286, utils/flowstep3d_util.py:42-44,
 *   losses/seg_loss_unsup.py:120-122, losses/flow_loss_unsup.py:57-59:
 *     dist = sqrt(dist2); idx[dist > radius] = idx[..., 0]
 * One launch, no host synchronisation (the reference's boolean-mask assignment syncs).
 * dist (b,n,k) receives sqrt(dist2) (what KNN.forward returns, pointnet2.py:103), idx the
 * clamped indices.  radius < 0 means "no clamp" (QueryAndGroup radius=None).
 * Entries whose index was clamped carry dist = +inf (every reference caller discards the
 * distances after the clamp): with radius >= 0 the search is RADIUS-LIMITED — it stops as
 * soon as the scanned cells cover the radius and the nearest neighbour is known, instead of
 * collecting all k neighbours first (C4's smoothness term: k = 32, r = 1 m holds ~2 points). */
int ogc_knn_clamped(int b, int n, int m, int k, float radius, const float *unknown,
                    const float *known, float *dist, int *idx, ogc_stream_t stream);

/* One cell grid for several radius searches of the same clouds in themselves.  The smoothness term of the OGC loss searches every
 * cloud twice — k nearest within r_knn, then the first nsample within r_ball
 *   losses/seg_loss_unsup.py:120-123 (KnnLoss), :151-152 (BallQLoss), both on (pc, pc)
 * — and ogc_knn_clamped / ogc_ball_query each sort the cloud into cells first (a third to a half of either call).  Here the
 * caller builds the grid ONCE, for the largest radius it will ask for, into memory it owns, and runs the searches on it:
 *   ogc_cell_grid_bytes(b, n)            size of the grid buffer (bytes; 256-byte aligned device memory)
 *   ogc_cell_grid_build(b, n, r, xyz, grid)        cells of edge 1.01 r over each cloud's bounding box; xyz (b,n,3), n >= 1024
 *   ogc_ball_query_cells(b, n, radius, nsample, xyz, grid, grid_radius, idx)       == ogc_ball_query(b, n, n, radius, nsample, xyz, xyz, idx)
 *   ogc_knn_clamped_cells(b, n, k, radius, xyz, grid, grid_radius, dist, idx)      == ogc_knn_clamped(b, n, n, k, radius, xyz, xyz, dist, idx)
 * for any radius <= grid_radius (the radius the grid was built with; larger ones are refused: OGC_ERR_UNSUPPORTED), bit for bit —
 * cells longer than a query needs only add candidates.  The grid stays valid until the caller frees or overwrites it; the k-NN
 * search writes a per-cloud flag into it (rows it left to its second kernel), nothing else does. */
long long ogc_cell_grid_bytes(int b, int n);
int ogc_cell_grid_build(int b, int n, float radius, const float *xyz, void *grid, ogc_stream_t stream);
int ogc_ball_query_cells(int b, int n, float radius, int nsample, const float *xyz, const void *grid, float grid_radius, int *idx,
                         ogc_stream_t stream);
int ogc_knn_clamped_cells(int b, int n, int k, float radius, const float *xyz, void *grid, float grid_radius, float *dist, int *idx,
                          ogc_stream_t stream);

/* The NaN rule and the Adam update of a training step (train_seg.py:81-83 + torch.optim.Adam.step(), train_seg.py:320) as two
 * launches over a chunk table, on torch's own state tensors (ogc_amd/csrc/adam.hip; fp32 parameters).
 *   table  (device, int64, 5 x n_tensors): pointers of the parameters, exp_avg, exp_avg_sq, step counts (0-dim fp32 tensors),
 *          then the element counts;  chunks (device, int32, n_chunks x 2): (tensor, first element) of every
 *          ogc_adam_chunk()-element piece;  grad_ptrs: HOST array of the n_tensors gradient pointers (<= ogc_adam_max_tensors());
 *   flag   (device, int32, zero on entry): 1 afterwards when a gradient held a NaN — the update and the step counts are then
 *          skipped on the device;  step_snapshot: n_tensors floats of scratch.  Hyper-parameters are doubles as in ATen's
 *          fused kernel (they meet the fp32 state in double expressions rounded once). */
int ogc_adam_max_tensors(void);
int ogc_adam_chunk(void);
int ogc_adam_step(int n_tensors, int n_chunks, const long long *table, const int *chunks, const void *const *grad_ptrs,
                  float *step_snapshot, int *flag, double lr, double beta1, double beta2, double eps, double weight_decay,
                  ogc_stream_t stream);

/* Batched 3x3 Kabsch rotation.  Replaces torch.svd + the reflection fix of the weighted-Kabsch fit
 *   losses/seg_loss_unsup.py:44-53:  u,s,v = svd(S); R = v diag(1,1,det(v u^T)) u^T.
 * S (nb,3,3) f32 cross-covariances (P_c^T diag(w) Q_c), R (nb,3,3) f32 out; valid (nb) i32 out or NULL:
 * 0 where S contains NaN/inf (then R = I — the reference's `valid_batches` rule, :38-42), else 1.
 * One thread per matrix, Jacobi eigen-solve of S^T S in fp64. */
int ogc_kabsch_rotation(int nb, const float *S, float *R, int *valid, ogc_stream_t stream);

/* Batched classical point-to-point ICP, every iteration inside one launch.  Replaces utils/icp_util.py:73-124 `icp` (sklearn's
 * nearest-neighbour search + numpy's SVD on the CPU, once per iteration), the ego-motion fit of test_flow_kittisf.py:103.
 * src, dst (B,n,3) f32 — one n for both, as the reference asserts; init_pose (B,4,4) f64 row-major or NULL; T (B,4,4) f64
 * row-major out; distances (B,n) f64 out: nearest-neighbour distances of the last search; iters (B) i32 out: the reference's
 * returned `i` (the loop index at the break, or max_iterations - 1).
 *   src <- init_pose src;  per iteration: nearest dst point of every src point (lower index on exact ties), best-fit rigid step
 *   between the two centred sets (SVD of the 3x3 cross-covariance, last row of V^T negated when det R < 0), src <- step src, stop
 *   when |prev_error - mean(distances of this search)| < tolerance;  T = best fit from the ORIGINAL src to the moved src.
 * Arithmetic in fp64 on the widened fp32 inputs, as numpy does for the reference; sums in a fixed order (bit-identical from run to
 * run).  One workgroup per pair, dst in LDS: n <= OGC_ICP_MAX_POINTS (OGC_ERR_INVALID_ARG beyond, and for n < 3 or
 * max_iterations < 1).  B == 0 is a no-op. */
#define OGC_ICP_MAX_POINTS 4096
int ogc_rigid_icp(int B, int n, const float *src, const float *dst, const double *init_pose, int max_iterations, double tolerance,
                  double *T, double *distances, int *iters, ogc_stream_t stream);

/* Batched ground-plane fitting, seed, every fit and every retry inside one launch.  Replaces utils/gpf_util.py:45-66, the loop of
 * `ground_plane_fitting` (numpy + scikit-spatial's Plane.best_fit on the CPU), the ground removal of test_flow_waymo.py:157-174.
 * pc (B,n,3) f32; plane (B,6) f64 out: centre, unit normal with a vertical_axis component >= 0; is_ground (B,n) i32 out, 0/1;
 * attempts (B) i32 out: the fits started (1 when the first succeeds).
 *   lpr = mean of the n_lpr smallest heights (coordinate vertical_axis);  selection = height < lpr + thresh_seed;  n_iter times:
 *   centre = mean of the selection, normal = eigenvector of the smallest eigenvalue of its 3x3 scatter,
 *   selection = |(p - centre) . normal| < thresh_dist.  A fit fails on fewer than 3 selected points, on a scatter that is not
 *   finite, or on a selection of rank below 2: l2 <= l1 * count * DBL_EPSILON for the scatter's eigenvalues l1 >= l2 >= l3
 *   (numpy.linalg.matrix_rank's rule applied at the resolution a scatter matrix has).  Then thresh_seed += 0.05 (repeated addition
 *   in double) and the cloud starts again from the seed; once the sum exceeds 0.8 it gives up: is_ground and plane all zero.
 * Arithmetic in fp64 on the widened fp32 inputs; sums in a fixed order (bit-identical from run to run).  One workgroup per
 * cloud, a thread's points in registers: 3 <= n <= OGC_GPF_MAX_POINTS, 1 <= n_lpr < n, n_iter >= 1, vertical_axis in 0..2
 * (OGC_ERR_INVALID_ARG otherwise, nothing launched).  B == 0 is a no-op. */
#define OGC_GPF_MAX_POINTS 8192
int ogc_ground_plane_fit(int B, int n, const float *pc, int n_iter, int n_lpr, double thresh_seed, double thresh_dist,
                         int vertical_axis, double *plane, int *is_ground, int *attempts, ogc_stream_t stream);

/* Segmentation evaluation of a batch in one launch: everything metrics/seg_metric.py computes per sample (eval_segm :38-93,
 * ClusteringMetrics :181-243) except the assignment, which ogc_lsap_maximize(B, 64, score) does next.  No host round trip.
 * segm (B,n) i32 GT labels in [0, OGC_SEG_EVAL_MAX_LABELS); mask (B,n,k) f32 point-major; ignore_npoint_thresh >= 0.  Outputs:
 *   hard (B,n) i32        arg-max over the k slots: the first maximum; a NaN counts as the maximum and the first NaN wins.
 *   counts (B,64,k) i32   points with label g and arg-max slot p.  Rows are RAW labels; an absent label is an empty row.
 *   pred_iou, confidence (B,k) f64, valid (B,k) i32, n_gt (B) i32   the AP table.  A GT object is ignored when 0 < size < thresh;
 *       a prediction is invalid when strictly more than half of its points lie in ignored objects or nothing is left of it;
 *       IoU = inter / (gt size + kept prediction size - inter) in fp64 on exact integers, maximum over the kept objects (0 when
 *       none is kept); n_gt = kept objects.  confidence keeps the reference's quirk: the column of the j-th VALID slot is
 *       summed over the points of the j-th PRESENT slot and divided by that slot's full size (an invalid slot takes the source
 *       of the last valid one before it, or the first present slot).
 *   score (B,64,64) f32   [g,p] = m / ((a_g + b_p - m) + 1e-8f) in float32, one rounding per operation, on the table whose rows
 *       with size < thresh are zeroed when thresh > 0 (a_g, b_p: its row and column sums); zero in those rows, in rows past the
 *       largest label and in columns >= k.
 *   rows (B) i32          rows g <= largest label that are not zeroed: the divisor of the mean IoU.
 *   ri (B) f64            (n_v^2 - sum a_g^2 - sum b_p^2 + 2 sum m^2) / n_v^2, the sums in 64-bit integers, then one fp64 division
 *       of the two converted integers; NaN when n_v (the points left in the table) is 0.
 *   status (B) i32        0 ok; bit 0: a label >= OGC_SEG_EVAL_MAX_LABELS was seen; bit 1: a negative label was seen.  Such a
 *       sample has all its other outputs zeroed and does not touch its neighbours; nothing is indexed with such a label.
 * Integer sums by LDS atomics, fp64 sums in a fixed order, no floating-point atomics: two calls give identical bits.
 * 1 <= k <= 64, n >= 1, thresh >= 0, no null pointer (OGC_ERR_INVALID_ARG otherwise, nothing launched).  B == 0 is a no-op. */
#define OGC_SEG_EVAL_MAX_LABELS 64
int ogc_seg_eval(int B, int n, int k, const int *segm, const float *mask, int ignore_npoint_thresh, int *hard, int *counts,
                 double *pred_iou, double *confidence, int *valid, int *n_gt, float *score, int *rows, double *ri, int *status,
                 ogc_stream_t stream);

/* ogc_seg_eval with a per-point ignore mask: ignore (B,n) i32, non-zero = the point is ignored.  The reference ships no such
 * metric (its test_seg_waymo.py imports a module that is not in its tree); THIS PACKAGE DEFINES IT from the code the reference
 * does have: an ignored point is a point of a GT object below ignore_npoint_thresh.  The results are what the reference's
 * eval_segm / ClusteringMetrics give with threshold max(thresh, 2) on the sample in which every ignored point carries a fresh
 * label of its own (an object of one point); see DESIGN.md 4h for the conditions under which thresh = 0 is covered and the
 * CPU check of the definition.  Differences from ogc_seg_eval, everything else being computed from these as there:
 *   - the label of an ignored point is never read (it may be anything; only non-ignored points can set a status bit);
 *   - hard is written for every point; counts (B,64,k) holds the non-ignored points only; ignored (B,k) i32 is the number of
 *     ignored points of every slot;
 *   - the size of a GT object, also for the comparison with thresh, is its number of non-ignored points; n_gt, rows and the
 *     largest label come from the non-ignored points;
 *   - the size of a slot is sum_g counts + ignored, its ignored area ignored + the points of dropped objects;
 *   - the Rand index runs over non-ignored points of objects that are not dropped;
 *   - confidence is unchanged: the sum runs over every point of the source slot, ignored ones included, over its full size.
 * A sample whose points are all ignored has n_gt = rows = 0, every valid 0 and ri NaN.  With an all-zero ignore every output
 * has the bits of ogc_seg_eval's.  Same launch shape, argument checks (ignore and ignored must not be null either) and
 * run-to-run bit equality. */
int ogc_seg_eval_ignore(int B, int n, int k, const int *segm, const float *mask, const int *ignore, int ignore_npoint_thresh,
                        int *hard, int *counts, int *ignored, double *pred_iou, double *confidence, int *valid, int *n_gt,
                        float *score, int *rows, double *ri, int *status, ogc_stream_t stream);

/* Scene-flow metrics of a batch in one launch (metrics/flow_metric.py:16-24).  gt_flow, flow_pred (B,N,3) f32, contiguous.
 * Per point, in fp32 with one rounding per operation: d = pred - gt, e = sqrtf((dx*dx + dy*dy) + dz*dz), s the same on gt,
 * r = e / (s + (float)eps); strict: e < (float)t || r < 0.05f; relaxed: e < (float)(2t) || r < 0.1f; outlier: e > (float)(6t) ||
 * r > 0.1f, t = epe_norm_thresh.  Outputs, which do not depend on their previous contents:
 *   epe_sum (B) f64     the sum of e over the sample's points, formed in a fixed order (per-workgroup partials, one ordered
 *                       finish; no floating-point atomics): identical bits from call to call and from process to process.
 *   counts (B,3) i32    the sample's strict-accurate, relaxed-accurate and outlier points.
 * A NaN satisfies no comparison and makes its own sample's epe_sum NaN; other samples are untouched.  One kernel launch, no
 * allocation, no fill, no synchronisation: capturable.  Several workgroups per sample exchange their partials through a static
 * table of the library: calls on DIFFERENT streams of one device must not overlap in time.
 * B < 0, N < 1, epe_norm_thresh not finite or <= 0, eps not finite or < 0, a null pointer: OGC_ERR_INVALID_ARG, nothing
 * launched.  B == 0 is a no-op whatever else is passed. */
int ogc_flow_eval(int B, int N, const float *gt_flow, const float *flow_pred, double epe_norm_thresh, double eps,
                  double *epe_sum, int *counts, ogc_stream_t stream);

/* The confidences of predicted segmentations, for training on them (datasets.py load_prediction / load_confidence), in one
 * launch and without ground truth.  mask (B,n,k) f32 point-major.  Per sample, the PRESENT slots are those that own at least one
 * point, in ascending slot index, numbered j = 0 .. n_object-1: the order in which compress_label_id numbers the saved arg-max
 * labels when a reader loads them.  Outputs, which do not depend on their previous contents:
 *   hard (B,n) i32      arg-max over the k slots by the rule of ogc_seg_eval: the first maximum; a NaN counts as the maximum and
 *                       the first NaN wins.  May be NULL: then it is not written, and nothing else changes.
 *   slots (B,k) i32     the slot index of the j-th present slot; -1 for j >= n_object.
 *   sizes (B,k) i32     its number of points; 0 for j >= n_object.
 *   conf (B,k) f32      (float)(S / sizes), rounded once, S the fp64 sum of the widened mask[b,p,slot] over the slot's own points
 *                       (metrics/seg_metric.py:81-85 for a prediction, without the validity filter of eval_segm and without the
 *                       column quirk that ogc_seg_eval keeps); 0 for j >= n_object.
 *   n_object (B) i32    the number of present slots, >= 1.
 * A NaN makes the confidence of the slot that owns its point NaN; every other slot and every other sample is untouched.
 * The sums are formed in a fixed order (per-workgroup partials, one ordered finish; no floating-point atomics): identical bits
 * from call to call and from process to process.  A workgroup takes OGC_SLOT_CONF_TILE points of one sample, so a sample spans
 * ceil(n / OGC_SLOT_CONF_TILE) workgroups and its bits depend on n alone — unless n > OGC_SLOT_CONF_TILE and B times that number
 * exceeds OGC_SLOT_CONF_MAX_PARTIALS: then a workgroup takes several consecutive tiles and the order, still fixed, is a
 * function of (B, n).  One kernel launch, no allocation, no fill, no synchronisation: capturable.  Several workgroups per sample
 * exchange their partials through a static table of the library, as ogc_flow_eval's do: calls on DIFFERENT streams of one device
 * must not overlap in time (stream order is all that is needed between calls).
 * 1 <= k <= OGC_SLOT_CONF_MAX_K, n >= 1, no null pointer other than hard: OGC_ERR_INVALID_ARG otherwise, nothing launched.
 * B == 0 is a no-op whatever else is passed. */
#define OGC_SLOT_CONF_MAX_K 64
#define OGC_SLOT_CONF_TILE 1024
#define OGC_SLOT_CONF_MAX_PARTIALS 2048
int ogc_slot_confidence(int B, int n, int k, const float *mask, int *hard, int *slots, int *sizes, float *conf, int *n_object,
                        ogc_stream_t stream);

/* The supervised mask loss (losses/seg_loss_sup.py) without its (B, N, K, K) tensors.  Throughout: mask (B,n,k) f32 point-major,
 * the model's soft masks; gt_mask (B,n,k) f32 with entries in [0, 1], not necessarily 0/1 (batch_segm_to_mask_withconf scales
 * columns by a confidence); valid (B,n) f32, or NULL for all ones.  The element function e(p, t) is what
 * F.binary_cross_entropy(p, t, reduction='none') computes in float32, (t - 1) * max(log1p(-p), -100) - t * max(log(p), -100), so
 * p == 0 with t == 1 gives exactly 100; with use_focal it is multiplied by (1 - p_t)^gamma, p_t = t p + (1 - t)(1 - p), then by
 * alpha_t = alpha t + (1 - alpha)(1 - t) when alpha >= 0, in the order of FocalLoss.forward.  gamma == 2 is a plain square, any
 * other gamma powf.  One rounding per operation.  A p that is NaN or outside [0, 1] makes every sum it enters NaN; it never traps.
 * Sums over points are fp64 in a fixed order (per-workgroup partials of OGC_SUP_LOSS_TILE points each, then one ordered finish),
 * no floating-point atomics: two calls give identical bits.  The partials pass through ws, a caller-owned buffer of at least
 * ogc_sup_loss_ws_doubles(B, n, k) doubles (0 for arguments outside the limits) whose previous contents do not matter; the
 * library holds no static table, so calls on different streams are independent.  No allocation, no fill, no synchronisation:
 * capturable (two launches per forward entry point, one for the backward).
 * Limits of all three: 1 <= k <= OGC_SUP_LOSS_MAX_K, n >= 1, gamma finite and >= 1, alpha not NaN (gamma and alpha are checked
 * whatever use_focal says), no null pointer other than valid: OGC_ERR_INVALID_ARG otherwise, nothing launched.  B == 0 is a no-op.
 *
 * ogc_sup_match_cost: the two tables CrossEntropyLoss / FocalLoss.match_cost and DiceLoss.match_cost are built from, both
 *   (B,k,k) f32, rows = predicted slot i, columns = GT slot j:
 *     cost_ce[b,i,j]   = (1/n) sum_n valid * e(mask[b,n,i], gt_mask[b,n,j])
 *     cost_dice[b,i,j] = 1 - (2 sum_n p t v + 1) / (sum_n p v + sum_n t v + 1)
 *   per-point terms in float32 ((p * t) * v, p * v, t * v), the sums and the final expressions in fp64, rounded once.  (The
 *   reference's DiceLoss.match_cost then takes the mean of the WHOLE (B,k,k) table; that is left to the caller.)
 * ogc_sup_mask_loss_fwd: col4row (B,k) i32, predicted slot i is matched to GT column col4row[b,i] (perm = eye[col_ind] and
 *   einsum('bij,bnj->bni') of the reference; the permuted labels are never written).
 *     sums (B,k,4) f64 = {sum v * e(p_i, t_col), sum p t v, sum p v, sum t v}
 *     terms (2) f32    = {l_ce: sum of sums[..., 0] / (B n k); l_dice: mean over (B,k) of 1 - (2 inter + 1) / (a + b + 1)}, in fp64
 *                        from sums, rounded once.
 *   An entry of col4row outside [0, k) (ogc_lsap_maximize writes -1 for a cost holding a NaN) makes that slot's sums and both
 *   terms NaN; nothing is indexed with it.
 * ogc_sup_mask_loss_bwd: grad_mask (B,n,k) f32 = grad_out[0] * d(w_ce * l_ce + w_dice * l_dice) / d mask, grad_out one f32 in
 *   device memory.  BCE as torch's backward, (p - t) / max((1 - p) p, 1e-12) * v / (B n k), exactly 0 where p == t in {0, 1};
 *   the focal factor's derivative goes through p_t; the Dice part is formed from the saved sums.  fp64 arithmetic on the
 *   widened inputs, rounded once; one element-wise kernel.  Labels are detached: no gradient for gt_mask.  A slot whose
 *   col4row entry is outside [0, k) gets NaN. */
#define OGC_SUP_LOSS_MAX_K 32
#define OGC_SUP_LOSS_TILE 64
long long ogc_sup_loss_ws_doubles(int B, int n, int k);
int ogc_sup_match_cost(int B, int n, int k, const float *mask, const float *gt_mask, const float *valid, int use_focal,
                       double alpha, double gamma, double *ws, float *cost_ce, float *cost_dice, ogc_stream_t stream);
int ogc_sup_mask_loss_fwd(int B, int n, int k, const float *mask, const float *gt_mask, const float *valid, const int *col4row,
                          int use_focal, double alpha, double gamma, double *ws, double *sums, float *terms,
                          ogc_stream_t stream);
int ogc_sup_mask_loss_bwd(int B, int n, int k, const float *mask, const float *gt_mask, const float *valid, const int *col4row,
                          int use_focal, double alpha, double gamma, const double *sums, double w_ce, double w_dice,
                          const float *grad_out, float *grad_mask, ogc_stream_t stream);

/* Grouping with relative coordinates in front, in one output tensor.  Replaces, in QueryAndGroup.forward
 *   pointnet2/pointnet2.py:284-296:  grouped_xyz = group(xyz^T, idx) - new_xyz^T[..., None];
 *                                    new_features = cat([grouped_xyz, group(features, idx)], dim=1)
 * (two gathers, a broadcast subtraction and a concatenation copy of the largest activation of the level).
 * xyz (b,n,3), new_xyz (b,npoints,3), points (b,c,n) (NULL iff c == 0), idx (b,npoints,nsample) i32,
 * out (b,3+c,npoints,nsample): channels 0..2 = xyz[idx] - new_xyz, channels 3.. = points[idx]. */
int ogc_group_concat(int b, int c, int n, int npoints, int nsample, const float *xyz, const float *new_xyz,
                     const float *points, const int *idx, float *out, ogc_stream_t stream);

/* Gradient of ogc_group_concat w.r.t. points: scatter-add of channels 3.. of grad_out (b,3+c,npoints,nsample) into
 * grad_points (b,c,n), which the caller zero-fills (as for ogc_group_points_grad). */
int ogc_group_concat_grad(int b, int c, int n, int npoints, int nsample, const float *grad_out, const int *idx,
                          float *grad_points, ogc_stream_t stream);

/* First layer of a set-abstraction MLP without the grouped tensor (utils/pointnet2_util.py:33-40: QueryAndGroup, then the
 * first Conv2d of the SharedMLP).  That layer is linear in [x_j - c_i ; f_j], so its feature part commutes with the
 * gather:  y[b, m, i, j] = P[b, m, idx[b, i, j]] + sum_k wx[m, k] * rel[b, k, i, j],  P = W_f . f per point (b, m, n),
 * rel (b, 3, npoints, nsample) the relative coordinates (ogc_group_concat with c = 0), wx (m, 3) the xyz columns of the
 * weight.  The (b, 3 + c, npoints, nsample) grouped tensor, its read by the convolution and the scatter of its gradient
 * never happen.  groups > 0: also the statistics of y for the GroupNorm that follows, in the layout of
 * ogc_conv1x1_gemm_gnstats (ogc_conv1x1_gn_slots() copies of (b, groups, 2) f64, overwritten).
 * Needs npoints * nsample % 4 == 0 and 16-byte aligned tensors (OGC_ERR_UNSUPPORTED otherwise).
 * ogc_group_linear_bwd reads the gradient tensor ONCE for both results that need it:  grad_p[b, m, idx] += grad_y (the
 * scatter-add of ogc_group_points_grad: grad_p (b, m, n) must be zeroed by the caller) and dwx[m, k] += sum grad_y * rel
 * (dwx (m, 3), zeroed by the caller).  Needs n <= 16384, npoints * nsample >= 4096 and a multiple of 16
 * (OGC_ERR_UNSUPPORTED otherwise: use ogc_group_points_grad and ogc_conv1x1_wgrad on (rel, grad_y)).  The remaining
 * gradients are small per-point GEMMs: d features = W_f^T grad_p, d W_f = sum_b grad_p f^T. */
int ogc_group_linear_fwd(int b, int m, int n, int npoints, int nsample, int groups, const float *P, const int *idx,
                         const float *rel, const float *wx, float *y, double *stats, ogc_stream_t stream);
/* ogc_group_linear_fwd for 1 .. 4 feature channels (an encoder's first level: the features are the coordinates) without the
 * point-wise product P: feats (b, cf, n), w (m, 3 + cf) the layer's weight rows; every output is ONE fused-multiply-add chain over
 * the input channels [rel x, y, z, f_0 ..] ascending — the order of the reference's convolution over cat([grouped_xyz,
 * grouped_features]) (pointnet2/pointnet2.py:286-297, utils/nn_util.py:45-85) and of this library's matrix kernels.  Other
 * arguments, statistics layout and preconditions as ogc_group_linear_fwd. */
int ogc_group_linear_fwd_direct(int b, int m, int cf, int n, int npoints, int nsample, int groups, const float *feats,
                                const int *idx, const float *rel, const float *w, float *y, double *stats, ogc_stream_t stream);
int ogc_group_linear_fwd_direct_h(int b, int m, int cf, int n, int npoints, int nsample, int groups, const float *feats,
                                  const int *idx, const float *rel, const float *w, ogc_bf16_t *y, double *stats, ogc_stream_t stream);
int ogc_group_linear_bwd(int b, int m, int n, int npoints, int nsample, const float *grad_y, const int *idx,
                         const float *rel, float *grad_p, float *dwx, ogc_stream_t stream);

/* The grouping gradient as a gather (round 2): grad_points[b,c,j] = sum of grad_out[b,c,t] over the positions t = p * nsample + s
 * with idx[b,p,s] == j — group_points_gpu.cu:8-25 / ogc_group_points_grad without atomics, every output written once (the
 * caller need not zero grad_points).  The transposed lists depend on idx only: ogc_group_reverse builds them once per
 * neighbour tensor (all channels, every step that reuses the tensor): the positions are cut into chunks of
 * tc = ogc_group_reverse_chunk(n, npoints, nsample); rev_start (b, chunks, n + 1) i32 delimits, per chunk and point, the
 * entries in rev_pos (b, npoints * nsample) u16 (positions relative to their chunk; the lists of chunk ch start at ch * tc;
 * order inside a list unspecified).  Inside every aligned group of 16 positions a run of equal indices (clamped / padded rows) is
 * listed once, by its first position; heads (b, npoints * nsample / 16) u16 has one bit per position, set for run heads — the
 * gradient kernel folds a run into its head while it stages the values.  Indices outside [0, n) are ignored.  n <= 16384,
 * npoints * nsample a multiple of 16. */
int ogc_group_reverse_chunk(int n, int npoints, int nsample);
int ogc_group_reverse(int b, int n, int npoints, int nsample, const int *idx, int *rev_start, unsigned short *rev_pos,
                      unsigned short *heads, ogc_stream_t stream);
int ogc_group_points_grad_rev(int b, int c, int n, int npoints, int nsample, const float *grad_out, const int *rev_start,
                              const unsigned short *rev_pos, const unsigned short *heads, float *grad_points,
                              ogc_stream_t stream);

/* The gradient of three_interpolate as the same gather: rev_* = ogc_group_reverse(b, m, n, 3, idx (b,n,3), ...) — position
 * t = 3 i + k stands for grad_out[b,c,i] * weight[b,i,k].  grad_points (b,c,m) is overwritten.  3 n a multiple of 16. */
/* ogc_group_points_grad_rev that also returns, from the same pass over grad_out, the three coordinate columns of a grouped first
 * layer's weight gradient (ogc_group_linear_fwd): dwx (c, 3) = sum_{b, pos} grad_out[b, ch, pos] * rel[b, k, pos] — the result of
 * ogc_conv1x1_wgrad(rel, grad_out) without its second read of grad_out.  dwx is zeroed by the call.  (_h: grad_out in bf16.) */
int ogc_group_points_grad_rev_dwx(int b, int c, int n, int npoints, int nsample, const float *grad_out, const int *rev_start,
                                  const unsigned short *rev_pos, const unsigned short *heads, const float *rel,
                                  float *grad_points, float *dwx, ogc_stream_t stream);
int ogc_three_interpolate_grad_rev(int b, int c, int n, int m, const float *grad_out, const float *weight,
                                   const int *rev_start, const unsigned short *rev_pos, const unsigned short *heads,
                                   float *grad_points, ogc_stream_t stream);
/* ... with grad_out a channel slice of a wider gradient (what autograd hands the interpolation underneath the concatenation of
 * PointnetFPModule.forward, utils/pointnet2_util.py:115-117): grad_out_bstride floats between consecutive samples' (c, n) planes,
 * >= c n; rows stay n contiguous floats.  Saves the copy `.contiguous()` would make. */
int ogc_three_interpolate_grad_rev_bs(int b, int c, int n, int m, const float *grad_out, long long grad_out_bstride,
                                      const float *weight, const int *rev_start, const unsigned short *rev_pos,
                                      const unsigned short *heads, float *grad_points, ogc_stream_t stream);

/* The scalar algebra either side of the fused loss terms (losses/seg_loss_unsup.py:353-392: a mean per term and view, summed
 * and weighted; the masks' gradient as the sum of its five consumers'), one launch per direction.  Pointer / size ARRAYS are host
 * memory, read during the call; at most 8 tensors.
 * ogc_view_means:      out[k] = mean of row k, rows of tensor 0 first: tensor i is dense fp32, viewed as (rows[i], len[i]).
 * ogc_view_means_grad: grad[i][r, :] = (weight[k(i, r)] * g_loss[0]) * (1 / len[i]) — the adjoint of the means under
 *                      loss = <weight, out>; weight (sum rows) and g_loss (1) are device memory.
 * ogc_sum_ranges:      out[e] = sum over the parts i with first[i] <= e < first[i] + count[i] of src[i][e - first[i]], in part
 *                      order; 0 where no part covers e.  total = elements of out. */
int ogc_view_means(int parts, const float *const *src, const int *rows, const long long *len, float *out, ogc_stream_t stream);
int ogc_view_means_grad(int parts, float *const *grad, const int *rows, const long long *len, const float *weight,
                        const float *g_loss, ogc_stream_t stream);
int ogc_sum_ranges(int parts, const float *const *src, const long long *first, const long long *count, long long total,
                   float *out, ogc_stream_t stream);

/* Dynamic (rigid-motion) term of the OGC loss, fused.  Replaces DynamicLoss.forward + fit_motion_svd_batch
 *   losses/seg_loss_unsup.py:64-98, :10-61 (K-fold expanded clouds, einsums, ~65 launches per step).
 * ogc_rigid_moments: per (cloud, slot) the weighted moments of p = pc and q = pc2 with weights mask[:, slot], accumulated
 *   in fp64 in ONE pass: mom (vb,k,16) f64 scratch {W, sum w p, sum w q, sum w p q^T}; outputs S (vb*k,3,3) f32 =
 *   sum w (p - pbar)(q - qbar)^T (the input of ogc_kabsch_rotation) and means (vb*k,6) f32 = (pbar, qbar).  A slot with
 *   zero weight gives NaN (as the reference's division does), which ogc_kabsch_rotation flags invalid.
 * ogc_rigid_translation: t = qbar - R pbar; fits flagged invalid get R = I, t = 0 (:40-42, :58-59).  R is updated in place.
 * ogc_rigid_blend: backward == 0: out (vb,n) = || sum_k mask[n,k] (R_k p_n + t_k) - q_n ||_p;  backward != 0:
 *   out (vb,n,k) = d/d mask of that, times grad_out (vb,n) (the fit itself is detached, :91).  p = 1 or 2; k <= 32.
 *   p == 0 (forward only): out (vb,n,3) = sum_k mask[n,k] (R_k p_n + t_k) - q_n, the vector itself — with pc2 = pc the
 *   mask-blended rigid flow of object-aware ICP (oa_icp.py:31-38, :75-83).
 * pc, pc2 (vb,n,3), mask (vb,n,k) point-major, R (vb*k,3,3), t (vb*k,3). */
int ogc_rigid_moments(int vb, int n, int k, const float *pc, const float *pc2, const float *mask, double *mom, float *S,
                      float *means, ogc_stream_t stream);
int ogc_rigid_translation(int total, const float *means, const int *valid, float *R, float *t, ogc_stream_t stream);
int ogc_rigid_blend(int vb, int n, int k, int p, int backward, const float *pc, const float *pc2, const float *mask,
                    const float *R, const float *t, const float *grad_out, float *out, ogc_stream_t stream);

/* Invariance term of the OGC loss, fused.  Replaces match_mask_by_iou's IoU matrix and InvarianceLoss.distance
 *   losses/seg_loss_unsup.py:212-233, :252-262 (arg-max, one-hot tensors, einsums, permutation products).
 * ogc_mask_iou: iou (pb,k,k) f32 of the hard (arg-max, first maximum) segmentations of mask1 / mask2 (pb,n,k):
 *   intersection / clamp(|g in 1| + |p in 2| - intersection, 1e-10); counts (pb,k,k) i32 scratch.
 * ogc_matched_distance: backward == 0: out1 (pb,n) = ||mask1[n] - mask2[n, col12]||_p, out2 (pb,n) =
 *   ||mask2[n] - mask1[n, col21]||_p with col12 / col21 (pb,k) i32 the assignments of ogc_lsap_maximize for iou and
 *   iou^T; backward != 0: out1 / out2 (pb,n,k) = gradients w.r.t. mask1 / mask2 through the FIRST operand of each
 *   distance only (the permuted targets are detached, :259-260), times grad12 / grad21 (pb,n).  p = 1 or 2; k <= 32. */
int ogc_mask_iou(int pb, int n, int k, const float *mask1, const float *mask2, int *counts, float *iou,
                 ogc_stream_t stream);
int ogc_matched_distance(int pb, int n, int k, int p, int backward, const float *mask1, const float *mask2,
                         const int *col12, const int *col21, const float *grad12, const float *grad21, float *out1,
                         float *out2, ogc_stream_t stream);

/* Linear sum assignment (maximise), batched, on the device.  Replaces the host round trip of the invariance loss
 *   losses/seg_loss_unsup.py:234-239:  scipy.optimize.linear_sum_assignment(iou[b], maximize=True)[1] per sample.
 * score (np,k,k) f32 row-major (rows = slots of mask1), col4row (np,k) i32 out: column assigned to each row.
 * Restates scipy's rectangular_lsap procedure (shortest augmenting paths, its column visiting order and its
 * tie-break) in fp64, so tied IoUs (empty slots) resolve exactly as on the host.  A problem containing NaN or
 * +inf scores yields -1 in every entry (scipy raises ValueError).  k <= 64. */
int ogc_lsap_maximize(int np, int k, const float *score, int *col4row, ogc_stream_t stream);

/* Eigenvalues (ascending) of small symmetric fp64 matrices, lower triangle referenced.  Replaces the singular
 * values of the nuclear-norm monitor  losses/seg_loss_unsup.py:300-314  (sum sqrt(eig(M^T M)) == sum svd(M)).
 * A (nb,k,k) f64, w (nb,k) f64 out; cyclic Jacobi, one wavefront per matrix; NaN/inf input -> NaN.  k <= 64. */
int ogc_sym_eigvals(int nb, int k, const double *A, double *w, ogc_stream_t stream);

/* Mask smoothness over neighbour lists, fused.  Replaces, in KnnLoss / BallQLoss
 *   losses/seg_loss_unsup.py:123-129, :152-158:
 *     nn_mask = grouping_operation(mask, idx); loss = (mask.unsqueeze(3) - nn_mask).norm(p, dim=1).mean(dim=-1)
 * mask (b,n,c) f32 POINT-major (the layout the network emits), idx (b,n,k) i32 into the same cloud,
 * out (b,n) f32: out[i] = (1/k) sum_j ||mask[i] - mask[idx[i,j]]||_p, p = 1 or 2. */
int ogc_neighbour_consistency_fwd(int b, int n, int c, int k, int p, const float *mask, const int *idx, float *out,
                                  ogc_stream_t stream);

/* Transposed neighbour lists (coordinates only; lets the gradient above be a gather instead of a scatter-add).
 * idx (b,n,k) i32 -> rev_start (b,n+1) i32: CSR offsets of the edges ARRIVING at each point; rev_src (b,n*k) i32:
 * their source points (order inside a list unspecified; only rev_start[b][n] entries are used).  Edges that cannot
 * contribute are left out and repeated ones merged: a self edge (idx[i][j] == i) has zero gradient; the copies of a
 * row's first entry (ball-query padding, radius-clamped kNN) become ONE edge, marked by bit 31 of its rev_src entry,
 * whose weight is rev_mult[b][i] (b,n) i32 = number of entries of row i equal to idx[i][0].  ws: (b,n) i32 scratch. */
int ogc_reverse_neighbours(int b, int n, int k, const int *idx, int *rev_start, int *rev_src, int *rev_mult, int *ws,
                           ogc_stream_t stream);

/* Gradient of ogc_neighbour_consistency_fwd w.r.t. mask, through both the centre and the neighbour operand
 * (torch's subgradients: sign(0) = 0 for p = 1, 0 where the norm vanishes for p = 2).
 * rev_start / rev_src / rev_mult from ogc_reverse_neighbours(idx); grad_out (b,n) f32, grad_mask (b,n,c) f32 out
 * (overwritten).  c <= 40. */
int ogc_neighbour_consistency_bwd(int b, int n, int c, int k, int p, const float *mask, const int *idx,
                                  const int *rev_start, const int *rev_src, const int *rev_mult, const float *grad_out,
                                  float *grad_mask, ogc_stream_t stream);

/* Soft nearest-neighbour targets of object-aware ICP, fused.  Replaces, per refinement iteration of
 *   oa_icp.py:62-72:  corr = softmax(-cdist(p1, p2) / temperature); corr *= mask1 @ mask2^T;
 *                     corr /= corr.sum(-1).clamp(1e-10); target = corr @ p2
 * (two (b, n1, n2) tensors — 1 GB each at b = 4, n = 8192 — written and re-read several times) by one pass with
 * running-maximum rescaling.  p1 (b,n1,3) warped source points, p2 (b,n2,3), mask1 (b,n1,k), mask2 (b,n2,k) with the
 * slots of mask2 already permuted to mask1's order; target (b,n1,3) out.  Distances use torch.cdist's large-matrix
 * formula (|a|^2 + |b|^2 - 2 a.b, clamped, sqrt).  k <= 32. */
int ogc_soft_nn_target(int b, int n1, int n2, int k, float temperature, const float *p1, const float *p2,
                       const float *mask1, const float *mask2, float *target, ogc_stream_t stream);

/* Values carried over a soft correspondence, fused (multi-frame voting).  Replaces
 *   vote.py:17-28, :52-58:  corr = softmax(-cdist(p1, p2) / temperature);  out = corr @ x
 * (an (n1, n2) matrix per adjacent frame pair — 268 MB at 8192 points — multiplied into thin matrices) by two passes over the
 * candidates on the matrix cores: the nearest distance of every query, then the weights against that fixed maximum fed straight
 * into the second product.  Nothing of size n1 x n2 is stored.
 *   out[b, m, :] = sum_n softmax_n(-|p1[b,m] - p2[b,n]| / temperature) * x[b, n, :]
 * p1 (b,n1,3) query points, already warped (pc + flow); p2 (b,n2,3) candidates; x (b,n2,c) values living on the candidates;
 * out (b,n1,c).  Distances use torch.cdist's large-matrix formula (|a|^2 + |b|^2 - 2 a.b, clamped, sqrt).  1 <= c <= 64
 * (OGC_ERR_UNSUPPORTED beyond: split x by columns), n2 >= 1, temperature > 0; b == 0 or n1 == 0 is a no-op.  A sample's result
 * does not depend on the other samples of the call (sums in a fixed order). */
int ogc_soft_carry(int b, int n1, int n2, int c, float temperature, const float *p1, const float *p2, const float *x,
                   float *out, ogc_stream_t stream);

/* Data preparation, stage 1: the crop of a raw scan to the front-view cloud, as a STABLE stream compaction.  Replaces
 *   data_prepare/kittidet/process_kittidet.py:99-114, data_prepare/semantickitti/process_semantickitti.py:61-78   (camera)
 *   data_prepare/waymo/process_waymo.py:132-141                                                                    (front)
 * scan (n, stride) f32 with xyz in columns 0..2; out_pc (n, 3) f32, keep_idx (n,) i32, count (1,) i32, all device memory.
 * Rows 0 .. count-1 of out_pc / keep_idx hold the kept points and their scan rows IN SCAN ORDER (the reference indexes with the
 * boolean mask, and FPS starts at row 0 and breaks ties by index); rows >= count are not written.  n == 0: OGC_OK, count = 0,
 * no kernel.  Two launches on `stream` and OGC_SCAN_CROP_TILE points per workgroup; no workgroup waits for another.
 *
 * camera: `cam` points to OGC_SCAN_CROP_CAMERA_DOUBLES doubles on the device:
 *   [0, 12)  V2C, 3 x 4 row-major (Tr_velo_to_cam / Tr)        [12, 21)  R0, 3 x 3 row-major (R0_rect)
 *   [21, 33) P, 3 x 4 row-major (P2)                           [33] image width   [34] image height
 *   [35]     0: R0 is skipped (SemanticKITTI has none), otherwise it is applied
 * Per point p, in fp64, sums left to right, never contracted: ref = V2C [p, 1]; rect = R0 ref (or ref); img = P [rect, 1];
 * u = img0 / img2, v = img1 / img2; out = fp32(rect * (-1, -1, 1)).  Kept iff u < W && u >= 0 && v < H && v >= 0 &&
 * p.x > clip_distance (fp32) && out.z < depth_thresh (fp32).  inf / NaN from img2 == 0 fail the comparisons.  stride >= 3.
 * front: kept iff scan[:, 5] == -1 && x > |y| && (x*x + y*y) + z*z < 3600 && |y| < 50 && x < 35, all fp32 with one rounding per
 * operation; out is the input xyz.  stride >= 6. */
#define OGC_SCAN_CROP_TILE 1024
#define OGC_SCAN_CROP_CAMERA_DOUBLES 36
int ogc_scan_crop_camera(int n, int stride, const float *scan, const double *cam, float clip_distance, float depth_thresh,
                         float *out_pc, int *keep_idx, int *count, ogc_stream_t stream);
int ogc_scan_crop_front(int n, int stride, const float *scan, float *out_pc, int *keep_idx, int *count, ogc_stream_t stream);
int ogc_scan_crop_tile(void); /* OGC_SCAN_CROP_TILE of the library */

/* Data preparation, stage 2: labels of points from oriented boxes, the LAST box that holds a point wins.  Replaces the box loops
 *   data_prepare/waymo/process_waymo.py:48-84, data_prepare/kittidet/process_kittidet.py:33-65
 * pc (n, 3) f32; sign_x / _y / _z in {1, -1}, applied to the point first; boxes (k, OGC_BOX_SEGM_BOX_DOUBLES) f64:
 *   [0, 9) rot, 3 x 3 row-major    [9, 12) centre c    [12, 15) lo    [15, 18) hi
 * ids (k, 2) i32: object id, class id.  segm, semantic_segm (n,) i32 out.  Per point and box in fp64, never contracted:
 *   d = sign * p - c;  q_i = (rot_i0 d_0 + rot_i1 d_1) + rot_i2 d_2;  inside iff lo_i < q_i && q_i < hi_i for i = 0, 1, 2
 * and the point gets the ids of the highest k whose box holds it, 0 / 0 when none does (k == 0: all zeros).  One thread per
 * point, the boxes staged in LDS OGC_BOX_SEGM_CHUNK at a time from the last to the first. */
#define OGC_BOX_SEGM_CHUNK 128
#define OGC_BOX_SEGM_BOX_DOUBLES 18
int ogc_box_segm(int n, int k, const float *pc, int sign_x, int sign_y, int sign_z, const double *boxes, const int *ids,
                 int *segm, int *semantic_segm, ogc_stream_t stream);
int ogc_box_segm_chunk(void); /* OGC_BOX_SEGM_CHUNK of the library */

/* Data preparation, KITTI Scene Flow: disparity and optical-flow maps unprojected to two clouds in correspondence, far and
 * invalid pixels dropped by a STABLE compaction, instance ids relabelled.  Replaces
 *   data_prepare/kittisf/process_kittisf.py:43-87, kittisf_util.py:6-27 (pixel2xyz), :59-63 (disp_2_depth), :72-81 (filter_segm)
 * disp1, disp2, inst (height, width) and flow (height, width, 3) are the 16-bit samples of the four PNGs; fb = focal length *
 * 0.54 as the caller rounds it to fp32, f = P[0][0], p02 .. p23 the entries of P_rect_02.  Per pixel (row i, column j), fp32,
 * one rounding per operation, never contracted:
 *   valid  = d1 > 0 && d2 > 0 && flow[2] == 1
 *   depthk = fb / (float(dk) / 256 + 1e-5f)                                                          k = 1, 2
 *   x1 = -((float(j) * (depth1 + p23) - (p02 * depth1 + p03)) / f),  y1 likewise with float(i), p12, p13;  z1 = depth1
 *   px2 = float(j) + (float(flow[0]) - 32768) / 64,  py2 = float(i) + (float(flow[1]) - 32768) / 64
 *   x2, y2 as x1, y1 with px2, py2, depth2;  z2 = depth2
 *   keep = valid && z1 < depth_thresh && z2 < depth_thresh
 * pc1, pc2 (height * width, 3) f32, segm, keep_idx (height * width,) i32, count (1,) i32, all device memory.  Rows 0 .. count-1
 * hold the kept pixels IN PIXEL ORDER, keep_idx = i * width + j; rows >= count are not written.  segm: the raw ids (inst) present
 * AMONG THE KEPT PIXELS whose semantic, id >> 8, is one of the n_select values of select_semantics (device, i32; values outside
 * 0..255 match nothing) are numbered 1, 2, ... in ascending id order; every other kept pixel gets 0.
 * Three launches on `stream` (the clearing of a 65 536-bit presence table in the stream's workspace, count, scatter),
 * OGC_SCAN_CROP_TILE pixels per workgroup, no workgroup waits for another.  height == 0 or width == 0: OGC_OK, count = 0, no
 * kernel.  height * width beyond 32-bit indexing, n_select outside 0..256, a null pointer (select_semantics may be null when
 * n_select == 0): OGC_ERR_INVALID_ARG, nothing launched. */
int ogc_kittisf_unproject(int height, int width, const unsigned short *disp1, const unsigned short *disp2,
                          const unsigned short *flow, const unsigned short *inst, float fb, float f, float p02, float p03,
                          float p12, float p13, float p23, float depth_thresh, const int *select_semantics, int n_select,
                          float *pc1, float *pc2, int *segm, int *keep_idx, int *count, ogc_stream_t stream);

/* The row filters of a PNG undone on the HOST (csrc/png_unfilter.h; no stream, nothing is launched — hence the integers last).
 * in: the inflated IDAT stream, height rows of (1 filter byte + row_bytes bytes); out: height * row_bytes bytes; bpp the bytes
 * per complete pixel.  A null pointer, a negative size, bpp not in {1, 2, 3, 6}, row_bytes % bpp != 0, a filter byte above 4:
 * OGC_ERR_INVALID_ARG with a message. */
int ogc_png_unfilter(const unsigned char *in, unsigned char *out, int height, int row_bytes, int bpp);

/* Data preparation, Waymo: the three integers per frame pair that the selection of moving samples takes, for a ragged batch of B
 * samples in ONE launch.  Replaces, per pair, data_prepare/waymo/select_mov.py:74-96 and the reader's filter_segm
 * (datasets/dataset_waymo.py:110-128) on the pair's first frame.
 * The raw arrays of the first frames, concatenated along points: pc, flow (total, 3) f32; segm, semantic_segm (total,) i32; offsets
 * (B + 1,) i32, sample b owns the points offsets[b] .. offsets[b + 1] - 1; motion (B, 12) f64, the row-major 3 x 3 rotation r, then
 * the translation t; ignore_class_ids (n_ignore,) i32.  All device memory.  stats (B, 4) i32 out = {n_distinct, n_fg, n_mov, status}:
 *   n_distinct  the number of distinct values of the FILTERED labels: a point's label becomes 0 when its semantic class is one of
 *               ignore_class_ids or when its object has fewer than ignore_npoint_thresh points in this sample.
 *   n_fg        the points with y >= (float)ground_y, compared in fp32.
 *   n_mov       those of them with, in fp64 from the fp32 inputs, one rounding per operation, never contracted,
 *                 d_i = ((((r_i0 x + r_i1 y) + r_i2 z) + t_i) - p_i) - flow_i,   sqrt((d_0^2 + d_1^2) + d_2^2) > moving_thresh
 *               (strict; the square root correctly rounded; a NaN is not moving).
 *   status      0, or 1: a label outside [0, OGC_MOVING_STATS_LABEL_CAP), or 2: offsets[b] < 0, offsets[b + 1] < offsets[b] or
 *               offsets[b + 1] > total.  With a status the other three fields are 0, nothing outside the arrays is read, and the
 *               other samples are unaffected.  The host only holds the pointer to offsets, so this is where they are checked.
 * One workgroup per sample, integer LDS atomics and integer reductions only: the result does not depend on the order of the
 * points or on the launch geometry.  An empty sample gives {0, 0, 0, 0}.  B == 0: OGC_OK, no launch.  A negative B, total,
 * n_ignore or ignore_npoint_thresh, a ground_y that is not finite, a moving_thresh that is not finite or negative, a null pointer
 * (the four point arrays may be null when total == 0, ignore_class_ids when n_ignore == 0): OGC_ERR_INVALID_ARG, nothing
 * launched. */
#define OGC_MOVING_STATS_LABEL_CAP 4096
int ogc_moving_stats(int B, int total, const int *offsets, const float *pc, const float *flow, const int *segm,
                     const int *semantic_segm, const double *motion, const int *ignore_class_ids, int n_ignore,
                     int ignore_npoint_thresh, double ground_y, double moving_thresh, int *stats, ogc_stream_t stream);
int ogc_moving_stats_label_cap(void); /* OGC_MOVING_STATS_LABEL_CAP of the library */

/* Data preparation, OGC-DR: an even sampling of mesh surfaces and the label transfer of the single-view set, what
 * data_prepare/ogcdr/sample_pointcloud.py does with trimesh.sample.sample_surface_even and data_prepare/ogcdrsv/collect_segm.py with
 * scipy's cdist.  All buffers device memory; every check that needs their contents is made on the device and reported in a status
 * buffer the caller reads when it reads the result.  C == 0 (B == 0): OGC_OK, nothing launched.
 *
 * ogc_surface_candidates: C area-weighted random points on the triangles of M meshes, fp64.  vertices (V, 3) f64 and faces (F, 3) i32
 * are the meshes concatenated, the faces indexing the concatenated vertices; cum_area (F) f64 is, per mesh, the running sum of its
 * face areas 0.5 * |cross|, restarting at each mesh; face_offsets, cand_offsets (M + 1) i32 delimit faces and candidates per mesh.
 * Candidate j of mesh m draws u0, u1, u2 in [0, 1) from Philox4x32-10 with key (seed & 0xffffffff, seed >> 32): counter (j, m, 0, 0)
 * gives u0 from words 0, 1 and u1 from words 2, 3, counter (j, m, 1, 0) gives u2 from words 0, 1; u = ((hi >> 5) * 2^26 + (lo >> 6)) *
 * 2^-53 with hi the first word.  So a candidate depends on (seed, m, j) and its mesh alone.  pick = u0 * total area; the face is the
 * first whose running sum exceeds pick (searchsorted, side "right"), clamped to the first face whose running sum reaches the total:
 * a face that adds no area is never chosen (trimesh's side "left" can choose a leading degenerate face at pick == 0).  If u1 + u2 > 1,
 * (u1, u2) = (1 - u1, 1 - u2); p = (o + u1 * e1) + u2 * e2 per coordinate with o = v[f0], e1 = v[f1] - o, e2 = v[f2] - o, one rounding
 * per operation.  points (C, 3) f64, face_idx (C) i32 (a row of faces) out.  status (1) i32 out: 0, or 1 a face index outside [0, V),
 * 2 offsets that do not start at 0, descend or do not end at F / C, 3 a mesh with candidates whose total area is not a positive
 * finite number; with a status set points and face_idx are not written.  Negative sizes, 3 F beyond 32 bits, C > 0 without a mesh, a
 * null pointer: OGC_ERR_INVALID_ARG, nothing launched. */
int ogc_surface_candidates(int C, int M, int V, int F, const double *vertices, const int *faces, const double *cum_area,
                           const int *face_offsets, const int *cand_offsets, long long seed, double *points, int *face_idx, int *status,
                           ogc_stream_t stream);
/* ogc_surface_thin: first-come greedy thinning, exact.  points (C, 3) f64, cand_offsets (M + 1) i32, radius (M) f64; keep (C) i32 out.
 * The definition is sequential: walking a mesh's candidates in index order, candidate i is kept (1) iff no kept candidate j < i of the
 * same mesh has ((dx*dx) + (dy*dy)) + (dz*dz) <= r_m * r_m in fp64, one rounding per operation, the bound inclusive; otherwise it is
 * removed (0).  Candidates of different meshes never interact.  This is the rule trimesh.sample.sample_surface_even documents as
 * rejection sampling; this definition, not trimesh's code, is the contract.
 * It is computed in rounds, one launch each (csrc/surface_thin.hip), over a uniform grid built inside the call.  A call with
 * rounds_done == 0 builds the grid in ws and queues `rounds` rounds; status (3) i32 then holds {code, candidates still undecided,
 * rounds that decided something}.  While status[1] != 0 the caller calls again with the same buffers and rounds_done = the rounds
 * queued so far, which queues `rounds` more; keep is final once status[1] == 0.  A round with nothing left to decide returns at once.
 * code: 0, or 1 a coordinate that is not finite, 2 a radius that is negative or not finite, 3 cand_offsets that do not start at 0,
 * descend or do not end at C; with a code set keep is not written and status[1] is 0.
 * ws: ws_bytes >= ogc_surface_thin_ws_bytes(C, M) bytes, 256-byte aligned.  C > 2^26: OGC_ERR_UNSUPPORTED.  Negative sizes, rounds
 * outside [0, 65536], C > 0 with M == 0, a null pointer, a small or misaligned workspace: OGC_ERR_INVALID_ARG.  Nothing launched. */
long long ogc_surface_thin_ws_bytes(int C, int M); /* -1 for a C outside [0, 2^26] */
int ogc_surface_thin(int C, int M, const double *points, const int *cand_offsets, const double *radius, int rounds, int rounds_done,
                     int *keep, int *status, void *ws, long long ws_bytes, ogc_stream_t stream);
/* ogc_nearest_label: per query the nearest source point of its sample and that point's label, `labels[cdist(query, source).argmin(1)]`.
 * query (B, Nq, 3), source (B, Ns, 3) f32, labels (B, Ns) i32; out_label, out_idx (B, Nq) i32.  The distance is
 * sqrt(((dx*dx) + (dy*dy)) + (dz*dz)) in fp64 from the fp32 inputs, one rounding per operation, the root correctly rounded, and the
 * ROOT is compared: two squares can round to one root, and the lowest source index among the minima wins, as in numpy's argmin.  A
 * NaN distance never wins.  B == 0 or Nq == 0: OGC_OK, nothing launched.  Ns < 1 otherwise, B > 65535, B * Nq or B * Ns beyond
 * 32-bit indexing of the coordinates, a null pointer: OGC_ERR_INVALID_ARG, nothing launched. */
int ogc_nearest_label(int B, int Nq, int Ns, const float *query, const float *source, const int *labels, int *out_label, int *out_idx,
                      ogc_stream_t stream);

/* Depth render of triangle meshes and the cloud of its hit points (csrc/depth_render.hip): the device stage of the
 * OGC-DRSV preparation, what data_prepare/ogcdrsv/build_ogcdrsv.py obtains from open3d's visualiser.  The definition below is THIS
 * package's contract; open3d's rasteriser is not what the result is pinned to.  All arithmetic is fp64, one rounding per operation,
 * nothing contracted, sums left to right; tests/depth_render_cases.py repeats the sequence in numpy.
 *
 * view: OGC_DEPTH_VIEW_DOUBLES doubles in HOST memory, read before the call returns: eye e (3), right (3), up (3), back (3) — an
 * orthonormal frame the caller vouches for, the camera looks along -back —, focal length f in pixels, principal point cx, cy, near,
 * far.  All finite, f > 0, 0 < near <= far, otherwise OGC_ERR_INVALID_ARG.  The image is width x height, row 0 the top row; pixel (x, y)
 * has its centre q = (x + 0.5, y + 0.5) and the row-major number y * width + x.
 *   camera     d = p - e;  xc = (right0*d0 + right1*d1) + right2*d2,  yc likewise with up,  zc = -((back0*d0 + back1*d1) + back2*d2)
 *   screen     sx = cx + f * (xc / zc),  sy = cy - f * (yc / zc)
 *   near       a face with a vertex at zc < near is dropped whole and counted in status[2]; nothing is clipped
 *   empty      a face with a non-finite camera or screen coordinate, or whose screen area
 *              (s1x - s0x) * (s2y - s0y) - (s1y - s0y) * (s2x - s0x) is exactly 0, covers nothing
 *   coverage   the three edge functions (bx - ax) * (qy - ay) - (by - ay) * (qx - ax) over (a, b) = (s0, s1), (s1, s2), (s2, s0):
 *              q is covered iff all three are >= 0 or all three are <= 0 — inclusive and two-sided, nothing is culled — and q lies in
 *              the closed bounding interval of the three screen vertices in x and in y.  A centre on an edge two faces share belongs
 *              to both; the depth test settles it.
 *   depth      n = cross(c1 - c0, c2 - c0) of the camera coordinates c = (xc, yc, zc), each component a * b - c * d;
 *              nc0 = (nx*c0x + ny*c0y) + nz*c0z;  the ray g = ((qx - cx) / f, -((qy - cy) / f), 1);  ng = (nx*gx + ny*gy) + nz;
 *              no hit when ng == 0;  t = nc0 / ng, no hit when t is not finite;  t is clamped into [min zc, max zc] of the face's
 *              three vertices;  the hit is kept iff near <= t <= far
 *   winner     the smallest t wins the pixel; among faces with that t, the lowest face index
 *   point      per coordinate k:  e_k + t * ((gx * right_k + gy * up_k) - back_k), rounded to fp32 last
 * ogc_depth_render: vertices (V, 3) f64, faces (F, 3) i32 -> depth (height, width) f64, +inf where no face is hit, and
 * face (height, width) i32, -1 there.  status (3) i32 out: {code, (P, written by ogc_depth_points), faces dropped by the near rule}.
 * code: 0, or 1 a face index outside [0, V), 2 a face with a vertex coordinate that is not finite (the larger code if both occur);
 * with a code set depth and face are not written.  F == 0 gives the empty image.  The image is the same in every run: both stages
 * take minima with integer atomics (csrc/depth_render.hip).  ws: ws_bytes >= ogc_depth_render_ws_bytes(F) bytes, 256-byte aligned
 * (not needed when F == 0).  F > 2^24: OGC_ERR_UNSUPPORTED.  Negative sizes, a side of the image outside [1, 16384], a view as above,
 * a null pointer, a small or misaligned workspace: OGC_ERR_INVALID_ARG.  Nothing launched.
 * ogc_depth_points: the covered pixels of depth and face (same view, same status buffer, after ogc_depth_render on the same stream)
 * as a stable compaction in row-major pixel order: points (P, 3) f32, pixel (P) i32 the pixel's number, face_out (P) i32; the three
 * buffers have room for width * height rows.  status[1] = P.  With status[0] != 0 nothing is written. */
#define OGC_DEPTH_VIEW_DOUBLES 17
long long ogc_depth_render_ws_bytes(int F); /* -1 for an F outside [0, 2^24] */
int ogc_depth_render(int V, int F, const double *vertices, const int *faces, const double *view, int width, int height, double *depth,
                     int *face, int *status, void *ws, long long ws_bytes, ogc_stream_t stream);
int ogc_depth_points(int width, int height, const double *view, const double *depth, const int *face, float *points, int *pixel,
                     int *face_out, int *status, ogc_stream_t stream);
/* ogc_depth_render_timed: ogc_depth_render with HIP events around its three stages, for tools/ogcdrsv_render_time.py.  Unlike every
 * other launching entry point it WAITS, for its last event: stage_ms (3 floats, HOST memory) = milliseconds of {setup: status, face
 * records, item offsets, the empty image; the depth pass; the face pass}.  Same results, same refusals. */
int ogc_depth_render_timed(int V, int F, const double *vertices, const int *faces, const double *view, int width, int height,
                           double *depth, int *face, int *status, void *ws, long long ws_bytes, float *stage_ms, ogc_stream_t stream);

/* Scene composition of the OGC-DR preparation (csrc/room_compose.hip): where the objects of a room stand in every frame,
 * what data_prepare/ogcdr/build_ogcdr.py:130-320 and :438-470 draw from np.random.  The definition below is THIS package's contract;
 * the reference's random stream cannot be reproduced.  All arithmetic is fp64, one rounding per operation, nothing contracted;
 * tests/ogcdr_compose_cases.py repeats it in numpy with sequential attempt loops.
 *
 * ogc_room_compose composes T trial scenes, one workgroup each.  Device memory: vertices (V, 3) f64, the canonical meshes of all
 * objects of all trials concatenated; vert_offsets (O + 1) i32; obj_offsets (T + 1) i32, the objects of trial t; room (T, 2) f64, the
 * xz range; seeds (T) i64.  HOST memory, read before the call returns: constants, OGC_ROOM_DOUBLES doubles = {ground_level,
 * wall_thickness, y angle range lo, hi, motion angle range about y lo, hi, about x or z lo, hi, prob_rotation_y, shift range lo, hi},
 * all finite (the reference: -0.49, 0.01, 0, 360, -10, 10, -10, 10, 0.6, 0.02, 0.04; its prob_rotation is 1 and no parameter), and
 * limits, OGC_ROOM_INTS ints = {n_frame in [1, 8], max_iter in [1, 65536], max_retry in [0, 255]}.
 *   random     Philox4x32-10 as in ogc_surface_candidates, key = (seed & 0xffffffff, seed >> 32) of the trial's seed, counter =
 *              (attempt, object, frame * 256 + fails, stream); object is the index inside the trial, fails the trial's running count of
 *              failed frame tries when the frame is tried (0 for frame 0).  Words (0, 1) and words (2, 3) give one uniform each.
 *              stream 0: attempt 0 gives u_a, u_b, attempt 1 gives u_c (first uniform).  stream 1: the two placement uniforms of
 *              attempt i (x, then z).  stream 2: the two sign uniforms of attempt i.  A range [lo, hi] is drawn as lo + u * (hi - lo).
 *   sin, cos   of an angle a in degrees, by this sequence, so that no libm decides a bit: q = rint(a / 90); r = a - 90 * q;
 *              t = r * K, K = 0x1.1df46a2529d39p-6, the double nearest pi / 180; s = t * t; ps and pc the Horner evaluations, innermost
 *              first, of the coefficients (-1)^k / (2k + 1)! and (-1)^k / (2k)!, k = 1 .. 8, each rounded to double (ps = c1 + s * (c2 +
 *              s * (... + s * c8))); sin_t = t + t * (s * ps); cos_t = 1 + s * pc; q mod 4 = 0, 1, 2, 3 picks (sin, cos) = (sin_t, cos_t),
 *              (cos_t, -sin_t), (-sin_t, -cos_t), (-cos_t, sin_t).  Within 2^-52 of the true values (tests/test_ogcdr_compose_cpu.py).
 *   rotation   frame 0: about y by the y angle range at u_a.  Frame f >= 1: if u_a < prob_rotation_y about y by the first motion range
 *              at u_b, otherwise by the second motion range at u_b about x if u_c < 0.5, about z otherwise.  The matrices are scipy's
 *              Rotation.from_euler on one lower-case axis: x [1 0 0; 0 c -s; 0 s c], y [c 0 s; 0 1 0; -s 0 c], z [c -s 0; s c 0; 0 0 1].
 *              R_f = r R_(f-1), every entry ((r_i0 * R_0j + r_i1 * R_1j) + r_i2 * R_2j).
 *   box        of an object under R: per axis i the minimum and maximum over its vertices of ((R_i0 * x + R_i1 * y) + R_i2 * z), then
 *              + 0.0, so that a zero extreme is +0 whichever vertex gave it.  t_y = ground_level - min_y.
 *   meet       two xz boxes [lo, hi] meet iff in both axes |c1 - c2| < (w1 + w2) / 2, c = (lo + hi) / 2, w = hi - lo of the stored
 *              corners (check_intersection_interval).
 *   frame 0    objects in index order.  b = max - min in x and z; attempt i: loc0 = (-room / 2 + wall) + u * ((room - b) - 2 * wall) per
 *              axis, the box [loc0, loc0 + b]; the lowest attempt below max_iter whose box meets no earlier object's box of this frame
 *              is accepted: t_xz = loc0 - min_xz.  An object without one: code 1.
 *   frame f    lo = min_xz + t_xz of the last frame, hi = max_xz + that, b = hi - lo; attempt i: d = +-(shift lo + u * (hi - lo)) per
 *              axis, + iff the sign uniform < 0.5; loc0 = lo + d; rejected if in either axis loc0 < -room / 2 + wall or
 *              loc0 > (room / 2 - wall) - b, otherwise tested as in frame 0 with the box [loc0, loc0 + b]; t_xz = t_xz of the last
 *              frame + d.  An object without an accepted attempt fails the try: fails + 1 > max_retry gives code 2, otherwise
 *              fails += 1 and the frame is drawn again from its rotations.
 * Out: poses (O, n_frame, 4, 4) f64, [R t; 0 0 0 1], the map from the canonical mesh to the frame's mesh; attempt (O, n_frame) i32, the
 * accepted attempt; fails (T, n_frame) i32, the failure count at which each frame was accepted; status (T, 2) i32 = {code, frame}:
 * 0 composed; 1 frame 0 found no place for an object; 2 the dynamics used up its retries at `frame`; 3 a vertex or room value of the
 * trial that is not finite; 4, in every trial, offsets that do not start at 0, descend, do not end at V / O, delimit an object without
 * vertices or give a trial more than OGC_ROOM_MAX_OBJECTS objects (the offsets are device memory: this limit is found there).  With a
 * non-zero code the trial's other outputs are unspecified.  T == 0: OGC_OK.  Negative sizes, 3 V or 2 T beyond 32 bits, a constant
 * that is not finite, a limit outside its range, a null pointer: OGC_ERR_INVALID_ARG, nothing launched.
 * ogc_mesh_apply_poses: vertices (V, 3) f64, vert_offsets (O + 1) i32 (ascending from 0 to V: not checked, a vertex takes the pose of
 * the last object whose offset does not exceed it), poses (O, n_frame, 4, 4) f64 -> out (n_frame, V, 3) f64,
 * out_i = ((R_i0 * x + R_i1 * y) + R_i2 * z) + t_i, one thread per vertex and frame.  V == 0 or n_frame == 0: OGC_OK.  Negative sizes,
 * 3 V n_frame beyond 32 bits, vertices without an object, a null pointer: OGC_ERR_INVALID_ARG. */
#define OGC_ROOM_DOUBLES 11
#define OGC_ROOM_INTS 3
#define OGC_ROOM_MAX_OBJECTS 32
#define OGC_ROOM_MAX_FRAMES 8
#define OGC_ROOM_MAX_ITER 65536
#define OGC_ROOM_MAX_RETRY 255
int ogc_room_compose(int T, int O, int V, const double *vertices, const int *vert_offsets, const int *obj_offsets, const double *room,
                     const long long *seeds, const double *constants, const int *limits, double *poses, int *attempt, int *fails,
                     int *status, ogc_stream_t stream);
int ogc_mesh_apply_poses(int V, int O, int n_frame, const double *vertices, const int *vert_offsets, const double *poses, double *out,
                         ogc_stream_t stream);

/* Attention core of the MaskFormer head's nn.MultiheadAttention layers
 *   utils/transformer_util.py:5-62 (cross-attention slots <- points, self-attention among the slots; 8 heads,
 *   models/segnet_kitti.py:49-51):   out = softmax(scale * Q K^T) V   per (sample, head), fp32.
 * q (b, lq, .), k, v (b, lk, .) are read in place from the projection outputs: row strides ldq / ldk / ldv floats, the
 * pointer is the first column of the operand inside its packed buffer, head i is the column block [i*d, (i+1)*d).
 * out (b, lq, h*d) contiguous, heads merged (what the output projection takes); prob (b, h, lq, lk) the attention
 * probabilities, kept for the backward pass.  d in {16, 32} (OGC_ERR_UNSUPPORTED otherwise); pointers 16-byte aligned,
 * strides multiples of 4.
 * bwd: dout (b, lq, h*d) -> dq / dk / dv written with row strides lddq / lddk / lddv (e.g. the column blocks of one
 * packed (b, l, 3*h*d) gradient); needs lq * lk floats of LDS per workgroup (OGC_ERR_UNSUPPORTED beyond 64 KiB). */
int ogc_attention_fwd(int b, int lq, int lk, int h, int d, float scale, const float *q, int ldq, const float *k,
                      int ldk, const float *v, int ldv, float *out, float *prob, ogc_stream_t stream);
int ogc_attention_bwd(int b, int lq, int lk, int h, int d, float scale, const float *q, int ldq, const float *k,
                      int ldk, const float *v, int ldv, const float *out, const float *prob, const float *dout,
                      float *dq, int lddq, float *dk, int lddk, float *dv, int lddv, ogc_stream_t stream);

/* nn.Linear on a few hundred rows (the decoder layers' projections and feed-forward network act on K slot embeddings
 * per sample, utils/transformer_util.py:5-62; 160 rows x 128 features at C4), one launch per direction, fp32 FMAs:
 *   fwd: y (rows, n_out) = x (rows, n_in) weight^T + bias        weight (n_out, n_in) as nn.Linear stores it; bias or NULL
 *   bwd: grad_x = grad_y weight,  grad_weight = grad_y^T x,  grad_bias = sum over the rows of grad_y
 *        — any of the three outputs may be NULL (not all); all are overwritten.
 * Any sizes are accepted; the kernels are laid out for rows <= ~1000 (32 x 32 output tiles, no split over the rows). */
int ogc_small_linear_fwd(int rows, int n_in, int n_out, const float *x, const float *weight, const float *bias,
                         float *y, ogc_stream_t stream);
int ogc_small_linear_bwd(int rows, int n_in, int n_out, const float *x, const float *weight, const float *grad_y,
                         float *grad_x, float *grad_weight, float *grad_bias, ogc_stream_t stream);

/* Backward of  y = conv(relu(GroupNorm(y_prev)))  inside a SharedMLP (utils/nn_util.py:45-85) WITHOUT the GroupNorm
 * backward passes (ogc_amd/csrc/gn_fused_bwd.hip).  pa, pb (b, cin): the GroupNorm of y_prev as an affine map per sample and
 * channel (ogc_group_norm_coeffs); mask = [pa y_prev + pb > 0] (relu != 0) or 1.
 *   ogc_conv1x1_wgrad_moments: moments (b, 2, cout, cin): H = g_y mask^T and H2 = g_y (mask . y_prev)^T per sample
 *       (overwritten).  hw % 16 == 0.
 *   ogc_gn_moments_combine: grad_w (cout, cin) = sum_b H2 diag(pa_b) + H diag(pb_b); grad_gamma, grad_beta (cin) of the
 *       GroupNorm — ONE buffer of 2 cin floats, grad_beta == grad_gamma + cin; coef (b, cin, 3) = (alpha, c2, c3) of its adjoint
 *       g_prev = alpha mask g_z + c2 y_prev + c3.  mean, rstd (b, groups), gamma (cin), w (cout, cin); cin <= 512.
 *   ogc_conv1x1_dgrad_adjoint: grad_prev (b, cin, hw) = alpha mask (w^T grad_y) + c2 y_prev + c3 — the input gradient of the
 *       convolution carried through ReLU and GroupNorm in the GEMM's epilogue.  hw % 64 == 0, cout <= 160. */
int ogc_conv1x1_wgrad_moments(int b, int cin, int cout, int hw, int relu, const float *y_prev, const float *pa,
                              const float *pb, const float *grad_y, float *moments, ogc_stream_t stream);
int ogc_gn_moments_combine(int b, int cin, int cout, int hw, int groups, const float *moments, const float *w,
                           const float *pa, const float *pb, const float *mean, const float *rstd, const float *gamma,
                           float *grad_w, float *coef, float *grad_gamma, float *grad_beta, ogc_stream_t stream);
int ogc_conv1x1_dgrad_adjoint(int b, int cin, int cout, int hw, int relu, const float *w, const float *grad_y,
                              const float *y_prev, const float *pa, const float *pb, const float *coef, float *grad_prev,
                              ogc_stream_t stream);

/* The first two layers of a set-abstraction MLP,  y2 = conv(relu(GroupNorm(y1)), w),  y1 = conv(x0, w1),  without y1 or its
 * gradient in memory (ogc_amd/csrc/first_conv.h).  x0 (b, c0, hw) is the grouped input, c0 <= 8; w1 (c1, c0).  Every kernel
 * rebuilds the values of y1 it would have loaded: w1[r][0] * x0[0], then fused multiply-adds over the channels ascending — what
 * ogc_conv1x1_gemm_gnstats stores, bit for bit.  All four: c1 <= 64, hw % 64 == 0, x0 16-byte aligned, c1 * hw < 2^31.
 *   ogc_first_conv_stats: the statistics of y1 for its GroupNorm, in ogc_conv1x1_gemm_gnstats's layout (overwritten);
 *       (c1 / groups) % 4 == 0, groups <= 32.
 *   ogc_conv1x1_gemm_affine_first: ogc_conv1x1_gemm_affine with in = y1 (M output channels, K = c1, groups >= 1: the
 *       statistics of the output as there).  Given the same pa, pb the output equals ogc_conv1x1_gemm_affine's on a stored y1.
 *   ogc_conv1x1_wgrad_moments_first: ogc_conv1x1_wgrad_moments with y_prev = y1 (cin = c1).
 *   ogc_conv1x1_dgrad_adjoint_first: ogc_conv1x1_dgrad_adjoint with y_prev = y1 (cin = c1, cout <= 64) whose result
 *       g1 = alpha mask (w^T grad_y) + c2 y1 + c3 is not stored: grad_w1 (c1, c0) = sum over samples and positions of g1 x0^T,
 *       the weight gradient of the first convolution (overwritten; fp32 atomic sums). */
int ogc_first_conv_stats(int b, int c1, int c0, int hw, int groups, const float *x0, const float *w1, double *stats,
                         ogc_stream_t stream);
int ogc_conv1x1_gemm_affine_first(int b, int M, int K, int hw, int relu, int groups, int c0, const float *w, const float *x0,
                                  const float *w1, const float *pa, const float *pb, float *out, double *stats,
                                  ogc_stream_t stream);
int ogc_conv1x1_wgrad_moments_first(int b, int cin, int cout, int hw, int relu, int c0, const float *x0, const float *w1,
                                    const float *pa, const float *pb, const float *grad_y, float *moments,
                                    ogc_stream_t stream);
int ogc_conv1x1_dgrad_adjoint_first(int b, int cin, int cout, int hw, int relu, int c0, const float *w, const float *grad_y,
                                    const float *x0, const float *w1, const float *pa, const float *pb, const float *coef,
                                    float *grad_w1, ogc_stream_t stream);

/* The tail of a set-abstraction MLP backwards, without the dense gradient in between:  last layer
 *   y = conv(relu(GroupNorm(y_prev)))  followed by  out = max over the neighbourhood of relu(GroupNorm'(y))
 * (utils/pointnet2_util.py:38-42).  The gradient of that pooled GroupNorm w.r.t. y is affine in y except at the arg-max
 * position of every neighbourhood:   g_y[b, ch, pr, j] = fmaf(c2, y, c3) + (j == argmax[b, ch, pr] ? ag : 0).
 *   ogc_group_norm_maxpool_bwd_sparse: ogc_group_norm_maxpool_bwd with  coef2 (b, c, 2) = (c2, c3)  and
 *       inj (b, c, p, 2) = (ag, argmax as its bit pattern)  in place of grad_x (b, c, p, s); grad_gamma / grad_beta as there.
 *       x_at_argmax (b, c, p) or NULL: x[b, c, pr, argmax] where the forward pass kept it (yext of
 *       ogc_conv1x1_gemm_affine_pool) — the sums pass then gathers from x only for channels whose scale rstd * gamma
 *       is zero (x itself is always required).
 *   ogc_conv1x1_wgrad_moments_pooled / ogc_conv1x1_dgrad_adjoint_pooled: ogc_conv1x1_wgrad_moments / _dgrad_adjoint of the
 *       convolution that wrote y, taking (y, coef2, inj) for grad_y and rebuilding it with the expression above while they
 *       load y — results identical, bit for bit, to the dense sequence; the pass that reads y and writes grad_y (the size of
 *       the layer's activation each way) is gone.  hw = centres * nsample, nsample in {16, 32, 64}. */
int ogc_group_norm_maxpool_bwd_sparse(int b, int c, int p, int s, int groups, int relu, const float *x,
                                      const float *x_at_argmax, const float *gamma, const float *mean, const float *rstd, const float *out, const int *argmax,
                                      const float *grad_out, float *coef2, float *inj, float *grad_gamma,
                                      float *grad_beta, double *ws, ogc_stream_t stream);
int ogc_conv1x1_wgrad_moments_pooled(int b, int cin, int cout, int hw, int relu, int nsample, const float *y_prev,
                                     const float *pa, const float *pb, const float *y, const float *coef2,
                                     const float *inj, float *moments, ogc_stream_t stream);
int ogc_conv1x1_dgrad_adjoint_pooled(int b, int cin, int cout, int hw, int relu, int nsample, const float *w, const float *y,
                                     const float *coef2, const float *inj, const float *y_prev, const float *pa,
                                     const float *pb, const float *coef, float *grad_prev, ogc_stream_t stream);

/* The same four kernels of a first level's chain (first pair + pooled tail, fp32) over the LIVE steps of its neighbour lists only.
 * A list idx (b, p, nsample) ends in repeats of its first entry where the search found fewer than nsample points inside the
 * radius (utils/pointnet2_util.py:59-79); those columns carry bit-equal values and gradients through the column-wise chain, and
 * in a sum over positions a weight stands for them.  Per centre, with steps of 16 columns and T = nsample / 16:
 *     fill = 1 + max{ j : idx[j] != idx[0] } (1: none),   s* = min(fill / 16, T - 1):   steps 0 .. s* are live, the rest skipped;
 *     when s* < T - 1 the last column of step s* is a repeat and gets the weight 1 + 16 (T - 1 - s*).
 *   ogc_live_steps: live (b, p * T): per sample the live steps ascending, entry = position / 16, with T - 1 - s* in bits 28 up on
 *       the entry of step s* (zero on a centre's earlier steps); n_live (b): entries in use.  nsample in {16, 32, 64},
 *       p <= 32768.  No atomics: the same list in deterministic mode.
 *   *_live: the entry point without the suffix, summing over the listed steps with those weights: moments, grad_w1 agree with
 *       the dense form up to fp32 summation order.  ogc_conv1x1_dgrad_adjoint_pooled_live writes grad_prev at the positions of
 *       live steps ONLY; ogc_conv1x1_wgrad_moments_first_live / _dgrad_adjoint_first_live read grad_y there only.
 *       nsample in {32, 64}; live_cap (entries per sample of `live`) >= hw / 16, the worst case — n_live stays on the device,
 *       the grids are sized for that case, and workgroups beyond the list leave at once.
 *   A level whose first layer is not a first pair (a grouped first layer, then ONE middle layer, then the pooled tail: the second
 *       level of the segmentation nets) takes the list from the tail down to the middle layer.  The pooled list forms serve its tail
 *       as they are (cin <= 64, cout <= 128: the adjoint's LDS is the weight tile plus, per wave, (ag, arg) for four entries and
 *       (c2, c3) once per row — 55.5 KB at cout = 128).  The middle layer has the PLAIN list forms:
 *       ogc_conv1x1_wgrad_moments_live: ogc_conv1x1_wgrad_moments reading y_prev and grad_y at the positions of live steps only,
 *       the term of an entry's last position weighted as above.
 *       ogc_conv1x1_dgrad_adjoint_live_fill: ogc_conv1x1_dgrad_adjoint reading grad_y and y_prev at live positions only and writing
 *       grad_prev DENSELY — a live position gets the dense form's expression, and the 16 k positions of the k steps an entry skips
 *       get the value of the entry's last position, which they repeat bit for bit: grad_prev equals the dense form's everywhere, and
 *       whatever reads it (the grouped first layer's backward) needs no list.  k is clamped to the steps left in the centre: a
 *       malformed list writes nothing outside the sample. */
int ogc_live_steps(int b, int p, int nsample, const int *idx, int *live, int *n_live, ogc_stream_t stream);
int ogc_conv1x1_wgrad_moments_pooled_live(int b, int cin, int cout, int hw, int relu, int nsample, const float *y_prev,
                                          const float *pa, const float *pb, const float *y, const float *coef2,
                                          const float *inj, const int *live, const int *n_live, int live_cap, float *moments,
                                          ogc_stream_t stream);
int ogc_conv1x1_dgrad_adjoint_pooled_live(int b, int cin, int cout, int hw, int relu, int nsample, const float *w, const float *y,
                                          const float *coef2, const float *inj, const float *y_prev, const float *pa,
                                          const float *pb, const float *coef, const int *live, const int *n_live, int live_cap,
                                          float *grad_prev, ogc_stream_t stream);
int ogc_conv1x1_wgrad_moments_live(int b, int cin, int cout, int hw, int relu, int nsample, const float *y_prev, const float *pa,
                                   const float *pb, const float *grad_y, const int *live, const int *n_live, int live_cap,
                                   float *moments, ogc_stream_t stream);
int ogc_conv1x1_dgrad_adjoint_live_fill(int b, int cin, int cout, int hw, int relu, int nsample, const float *w,
                                        const float *grad_y, const float *y_prev, const float *pa, const float *pb,
                                        const float *coef, const int *live, const int *n_live, int live_cap, float *grad_prev,
                                        ogc_stream_t stream);
int ogc_conv1x1_wgrad_moments_first_live(int b, int cin, int cout, int hw, int relu, int c0, int nsample, const float *x0,
                                         const float *w1, const float *pa, const float *pb, const float *grad_y,
                                         const int *live, const int *n_live, int live_cap, float *moments, ogc_stream_t stream);
int ogc_conv1x1_dgrad_adjoint_first_live(int b, int cin, int cout, int hw, int relu, int c0, int nsample, const float *w,
                                         const float *grad_y, const float *x0, const float *w1, const float *pa, const float *pb,
                                         const float *coef, const int *live, const int *n_live, int live_cap, float *grad_w1,
                                         ogc_stream_t stream);

/* The two FORWARD kernels of the same chain over the live steps only (fp32): ogc_conv1x1_gemm_affine_first and
 * ogc_conv1x1_gemm_affine_pool read their input and write `out` at the positions of live steps ONLY — a skipped position of `out`
 * keeps whatever it held, and nothing of the chain's backward list forms reads it.
 *   The forward list.  A wave of these kernels owns a TILE of four list entries and must hold every live entry of each 64-position
 *       tile of the dense kernels it touches (a GROUP: the entries with the same entry >> 2 — one centre at nsample 64, a pair of
 *       centres at 32).  ogc_live_steps_fwd writes `live` / `n_live` exactly as ogc_live_steps does and, in the same launch, fwd
 *       (b, p * T), n_fwd (b): the same entries in the same order, packed greedily so that no group crosses a tile boundary — a
 *       group that does not fit the slots left in the current tile starts the next one, and the slots it leaves hold the PAD marker
 *       -1 (every real entry is >= 0).  n_fwd counts entries and the pads in front of the last one; slots behind entry n_fwd - 1 are
 *       read as pads.  Every tile holds at least one whole group, so p * T entries cover the worst case.  nsample in {32, 64},
 *       p * nsample a multiple of 64, p <= 32768.
 *   The statistics are the dense form's: per dense tile and 16-row block the dense kernel adds ONE fp32 partial sum of 256 values,
 *       (Q0 + Q1) + (Q2 + Q3) with Qs the sum over step s (four lanes of 4 rows x 4 positions each, rows outer, then two exchange
 *       stages inside the quad of lanes); the list form takes Qs of a live step from the quad that holds it and Qs of a skipped step
 *       as (d + d) + (d + d), d being what each lane of that step would have summed: the four rows of the last column of the centre's
 *       last live step, four times each.  The partial sums are therefore bit-equal, and `stats` differs from the dense form's only in
 *       the order of its fp64 additions, as two runs of the dense form do.  yext / aext (b, M, centres) are the dense form's: maxima
 *       are exact in any order, and with the smallest index winning a tie every arg-max lies in a live step.
 *   live, n_live, live_cap of the two *_live entry points: the FORWARD list; otherwise the arguments and preconditions of the entry
 *       points without the suffix and of the list forms above (K <= 64 for the pooled one). */
int ogc_live_steps_fwd(int b, int p, int nsample, const int *idx, int *live, int *n_live, int *fwd, int *n_fwd, ogc_stream_t stream);
int ogc_conv1x1_gemm_affine_first_live(int b, int M, int K, int hw, int relu, int groups, int c0, int nsample, const float *w,
                                       const float *x0, const float *w1, const float *pa, const float *pb, const int *live,
                                       const int *n_live, int live_cap, float *out, double *stats, ogc_stream_t stream);
int ogc_conv1x1_gemm_affine_pool_live(int b, int M, int K, int hw, int relu, int groups, int nsample, const float *w,
                                      const float *in, const float *pa, const float *pb, const float *next_gamma, const int *live,
                                      const int *n_live, int live_cap, float *out, double *stats, float *yext, int *aext,
                                      ogc_stream_t stream);

/* A whole per-neighbourhood MLP and its max-pool in one launch, for INFERENCE
 *   utils/flowstep3d_util.py:57-66 (FlowEmbedding, the correlation layer) and :126-138 (set abstraction):
 *     for conv, bn in zip(mlp_convs, mlp_bns): x = relu(bn(conv(x)));   x = max(x, -1)
 * with BatchNorm in evaluation mode, i.e. an affine map per output channel that the caller folds into the weights:
 *   wt_l (c_{l-1} rounded up to 4, c_l) = TRANSPOSED folded weights (rows beyond c_{l-1} zero), b_l (c_l) folded biases,
 *   x (b, c0, p, nsample) -> out (b, c_last, p) = max over nsample of relu(W3' relu(W2' relu(W1' x + b1) + b2) + b3);
 *   c3 == 0: two layers.  fp32 on v_mfma_f32_16x16x4_f32; the activations between the layers never leave the register
 *   file.  ogc_mlp_chain_pool_supported() says whether a kernel exists for a shape (1) or the caller runs its layers
 *   one by one (0). */
int ogc_mlp_chain_pool_supported(int c0, int c1, int c2, int c3, int nsample);
int ogc_mlp_chain_pool(int b, int c0, int c1, int c2, int c3, int p, int nsample, const float *x, const float *wt1,
                       const float *b1, const float *wt2, const float *b2, const float *wt3, const float *b3, float *out,
                       ogc_stream_t stream);

/* The FlowStep3D correlation layer after its neighbour search, in one launch, for INFERENCE
 *   utils/flowstep3d_util.py:53-66 (FlowEmbedding.forward): group pos2 and feat2 by idx, subtract pos1, concatenate
 *   [pos2[idx] - pos1 (3), feat2[idx] (cf), feat1 repeated (cf)] -> 3 x (conv, BatchNorm(eval), ReLU) -> max over nsample.
 * pos1 (b,3,n1), pos2 (b,3,n2), feat1 (b,cf,n1), feat2 (b,cf,n2), idx (b,n1,nsample) = the clamped neighbour indices
 * (ogc_knn_clamped); weights as for ogc_mlp_chain_pool (wt1 has 3 + 2 cf rows, padded to a multiple of 4); out (b,c3,n1).
 * The (b, 3 + 2 cf, n1, nsample) tensor is never formed: its rows are gathered while the first layer's operands load. */
int ogc_corr_layer_pool_supported(int cf, int c1, int c2, int c3, int nsample);
int ogc_corr_layer_pool(int b, int cf, int c1, int c2, int c3, int n1, int n2, int nsample, const float *pos1,
                        const float *pos2, const float *feat1, const float *feat2, const int *idx, const float *wt1,
                        const float *b1, const float *wt2, const float *b2, const float *wt3, const float *b3, float *out,
                        ogc_stream_t stream);

/* Mask read-out of the segmentation nets
 *   models/segnet_kitti.py:85-88 (segnet_sapien.py / segnet_ogcdr.py :77-80):
 *   mask = softmax_k( F.normalize(feats, dim=1)^T F.normalize(slots, dim=1) / temperature ),  temperature = 0.05.
 * feats (b, d, n) per-point features, slots (b, d, k) object embeddings, mask (b, n, k); fp32, contiguous.  The norms
 * are clamped at 1e-12 as F.normalize does.  k <= 32, d <= 256 (OGC_ERR_UNSUPPORTED otherwise).
 * bwd: grad_mask (b, n, k) -> grad_feats (b, d, n) and grad_slots (b, d, k), both overwritten; mask is the forward
 * output.  ws: scratch of ogc_slot_masks_ws_floats(b, d, n, k) floats (per-workgroup partial sums of the slot
 * gradient, added in a fixed order: the result repeats bit for bit). */
long long ogc_slot_masks_ws_floats(int b, int d, int n, int k);
int ogc_slot_masks_fwd(int b, int d, int n, int k, float temperature, const float *feats, const float *slots,
                       float *mask, ogc_stream_t stream);
int ogc_slot_masks_bwd(int b, int d, int n, int k, float temperature, const float *feats, const float *slots,
                       const float *mask, const float *grad_mask, float *grad_feats, float *grad_slots, float *ws,
                       ogc_stream_t stream);

/* Fused GroupNorm (+ ReLU) forward / backward.  Replaces the nn.GroupNorm -> ReLU(inplace) tail of every
 * Conv2d block of the segmentation nets' SharedMLPs
 *   utils/nn_util.py:6-11 (GroupNorm), :45-85 (_ConvBase ordering), models/segnet_kitti.py:8 (BN_CONFIG).
 * x, y, grad_y, grad_x (b, c, hw) f32 contiguous; gamma, beta, grad_gamma, grad_beta (c); mean, rstd (b*groups)
 * (written by fwd, read by bwd); biased variance, rstd = 1/sqrt(var + eps); relu != 0 applies max(.,0) in fwd
 * and masks grad_y where the output was <= 0 in bwd.
 * ws: caller-allocated scratch holding per-slice partial sums (every entry used is written before it is read: no
 * clearing, no atomics).  fwd: 2*b*groups*ogc_group_norm_stats_slots() doubles; bwd: 2*b*c*ogc_group_norm_bwd_slots()
 * doubles. */
int ogc_group_norm_stats_slots(void);
int ogc_group_norm_bwd_slots(void);
int ogc_group_norm_fwd(int b, int c, int hw, int groups, float eps, int relu, const float *x,
                       const float *gamma, const float *beta, float *y, float *mean, float *rstd,
                       double *ws, ogc_stream_t stream);
int ogc_group_norm_bwd(int b, int c, int hw, int groups, int relu, const float *x, const float *gamma,
                       const float *beta, const float *mean, const float *rstd, const float *grad_y,
                       float *grad_x, float *grad_gamma, float *grad_beta, double *ws, ogc_stream_t stream);

/* GroupNorm (+ ReLU) fused with the max over the neighbourhood — the tail of a set-abstraction MLP
 *   utils/pointnet2_util.py:38-42 (SharedMLP then F.max_pool2d over nsample).
 * x (b, c, p, s) -> out (b, c, p), argmax (b, c, p) i32 (index in [0, s) of the winning neighbour; first index on
 * ties).  s must be a power of two in [4, 256] and x 16-byte aligned (OGC_ERR_UNSUPPORTED otherwise).
 * bwd: grad_out (b, c, p) -> grad_x (b, c, p, s), grad_gamma, grad_beta; scratch sizes as for ogc_group_norm_*. */
int ogc_group_norm_maxpool_fwd(int b, int c, int p, int s, int groups, float eps, int relu, const float *x,
                               const float *gamma, const float *beta, float *out, int *argmax, float *mean,
                               float *rstd, double *ws, ogc_stream_t stream);
int ogc_group_norm_maxpool_bwd(int b, int c, int p, int s, int groups, int relu, const float *x,
                               const float *gamma, const float *mean, const float *rstd, const float *out,
                               const int *argmax, const float *grad_out, float *grad_x, float *grad_gamma,
                               float *grad_beta, double *ws, ogc_stream_t stream);
/* ogc_group_norm_maxpool_bwd with x_at_argmax (b, c, p) = x[b, c, pr, argmax[b, c, pr]] handed in (same source as above). */
int ogc_group_norm_maxpool_bwd_ext(int b, int c, int p, int s, int groups, int relu, const float *x,
                                   const float *x_at_argmax, const float *gamma, const float *mean, const float *rstd,
                                   const float *out, const int *argmax, const float *grad_out, float *grad_x,
                                   float *grad_gamma, float *grad_beta, double *ws, ogc_stream_t stream);

/* Fused BatchNorm2d (+ ReLU) (+ max over the neighbourhood), forward / backward — the F.relu(bn(conv(.))) chains and
 * the trailing .max(dim=-1) of the FlowStep3D blocks
 *   utils/flowstep3d_util.py:57-66 (FlowEmbedding), :126-138 (PointNetSetAbstraction), :181-183 (feature propagation).
 * nn.BatchNorm2d semantics.  training != 0: batch statistics per channel over (b, hw), biased variance,
 * rstd = 1/sqrt(var + eps); running_mean / running_var (c), when non-NULL, are updated in place with `momentum` and the
 * unbiased variance.  training == 0: running statistics (required) are used, and the backward is the affine map's.
 * x, y, grad_y, grad_x (b, c, hw) [maxpool: x (b, c, p, s) -> out, argmax (b, c, p); s a power of two in [4, 256]];
 * gamma, beta, grad_gamma, grad_beta, mean, rstd (c) (mean / rstd written by fwd, read by bwd).
 * stats / slots: optional statistics supplied by the producing kernel (`slots` copies of a (c, 2) f64 accumulator), else
 * NULL / 0 and ws (2c f64) is used.  bwd ws: 3c f64.
 * All four: b <= 65535 and c * hw (c * p * s) < 2^31, OGC_ERR_INVALID_ARG otherwise, nothing launched.
 * training == 0 with mean == rstd == NULL (inference, nothing kept for a backward pass): the affine map is formed from the
 * running statistics inside the apply kernel itself — one launch. */
int ogc_batch_norm_fwd(int b, int c, int hw, float eps, int relu, int training, float momentum, const float *x,
                       const float *gamma, const float *beta, float *running_mean, float *running_var, float *y,
                       float *mean, float *rstd, double *ws, const double *stats, int slots, ogc_stream_t stream);
int ogc_batch_norm_bwd(int b, int c, int hw, int relu, int training, const float *x, const float *gamma,
                       const float *beta, const float *mean, const float *rstd, const float *grad_y, float *grad_x,
                       float *grad_gamma, float *grad_beta, double *ws, ogc_stream_t stream);
int ogc_batch_norm_maxpool_fwd(int b, int c, int p, int s, float eps, int relu, int training, float momentum,
                               const float *x, const float *gamma, const float *beta, float *running_mean,
                               float *running_var, float *out, int *argmax, float *mean, float *rstd, double *ws,
                               const double *stats, int slots, ogc_stream_t stream);
int ogc_batch_norm_maxpool_bwd(int b, int c, int p, int s, int relu, int training, const float *x, const float *gamma,
                               const float *mean, const float *rstd, const float *out, const int *argmax,
                               const float *grad_out, float *grad_x, float *grad_gamma, float *grad_beta, double *ws,
                               ogc_stream_t stream);

/* Weight gradient of a 1x1 convolution (bias-free), NCHW, fp32, on the fp32 MFMA pipe:
 *   dw[co, ci] = sum_b sum_p dy[b, co, p] * x[b, ci, p]
 * Replaces the weight-gradient half of the Conv2d(1x1) layers of SharedMLP (utils/nn_util.py:45-85, :155-172), which
 * MIOpen computes through two full NCHW->NHWC transposes.  x (b, cin, hw), dy (b, cout, hw), dw (cout, cin) — dw is
 * overwritten.  hw must be a multiple of 16 and x, dy 16-byte aligned (OGC_ERR_UNSUPPORTED otherwise). */
int ogc_conv1x1_wgrad(int b, int cin, int cout, int hw, const float *x, const float *dy, float *dw,
                      ogc_stream_t stream);

/* Forward / input gradient of the same 1x1 convolution as one fp32-MFMA GEMM over NCHW tensors:
 *   out[b, m, p] = sum_k A[m, k] * in[b, k, p]
 * forward:        transpose_a = 0, A = w (M = Cout, K = Cin),  in = x,  out = y
 * input gradient: transpose_a = 1, A = w^T (M = Cin, K = Cout), in = dy, out = dx      (w is always (Cout, Cin))
 * Requires hw % 64 == 0, K <= 160 and 16-byte aligned tensors (OGC_ERR_UNSUPPORTED otherwise -> vendor conv). */
int ogc_conv1x1_gemm(int b, int M, int K, int hw, int transpose_a, const float *w, const float *in,
                     float *out, ogc_stream_t stream);

/* The forward convolution above, also producing the first pass of the GroupNorm that follows every Conv2d of a
 * SharedMLP (utils/nn_util.py:45-85): per (batch, group) the sum and the sum of squares of the outputs, fp64.
 * stats: ogc_conv1x1_gn_slots() copies of a (b, groups, 2) f64 accumulator, slot-major (the copies spread the atomics
 * over cache lines; their sum is the statistic) — overwritten.  Pass it to ogc_group_norm_fwd_stats /
 * ogc_group_norm_maxpool_fwd_stats, which then skip their own statistics pass over the tensor.
 * Requires, beyond ogc_conv1x1_gemm: groups <= 32, (M / groups) % 4 == 0 and K <= 100 (OGC_ERR_UNSUPPORTED otherwise:
 * wider layers run the plain GEMM and the GroupNorm entry points compute their own statistics). */
int ogc_conv1x1_gn_slots(void);
/* 1 if the forward convolution can produce the next GroupNorm's statistics on the way for this shape (ogc_conv1x1_gemm_gnstats,
 * affine = 0; ogc_conv1x1_gemm_affine with groups > 0, affine = 1): K <= 100, or a shape of the streaming kernel (fp32
 * operands, 100 < K <= 160, hw a multiple of 64, b * hw / 64 >= 2048). */
int ogc_conv1x1_gemm_stats_supported(int b, int M, int K, int hw, int affine);
/* 1 when ogc_conv1x1_gemm takes this shape on its streaming kernel (K in 101 .. 160, >= 2048 position tiles, fp32 operands):
 * the shapes for which the host layers prefer it to a vendor GEMM for a plain product */
int ogc_conv1x1_gemm_stream_supported(int b, int M, int K, int hw);
/* The same product for ANY reduction length and row count (ogc_amd/csrc/gemm_chunk.hip: K walked in chunks, the weights'
 * chunk in LDS, the input chunk in registers; few positions: the wavefronts of a workgroup split the rows): the Conv1d of
 * the feature-propagation modules (utils/pointnet2_util.py:96-120 — 384 -> 128 on 1024 points ...) and the input gradient
 * of layers wider than 160 channels, which went to the vendor library before.  hw % 64 == 0; operands as
 * ogc_set_matmul_precision says (fp32 operands whatever the switch until 0.2.2). */
int ogc_conv1x1_gemm_any(int b, int M, int K, int hw, int transpose_a, const float *w, const float *in, float *out,
                         ogc_stream_t stream);

/* Operand precision of ogc_conv1x1_gemm* / ogc_conv1x1_wgrad* (process-wide; returns the previous setting).
 * 0 (default): fp32 operands on v_mfma_f32_16x16x4_f32 — exact fp32 FMA chains, the parity mode.
 * 1: operands rounded to bf16 (nearest even) on v_mfma_f32_16x16x16_bf16, fp32 accumulation, tensors in memory stay
 *    fp32 — the arithmetic torch.autocast(bfloat16) gives the reference's Conv2d layers (BASELINE config "OGC-DR ...,
 *    bf16"); GroupNorm statistics, losses and everything else stay fp32. */
int ogc_set_matmul_precision(int bf16);
int ogc_conv1x1_gemm_gnstats(int b, int M, int K, int hw, int groups, const float *w, const float *in, float *out,
                             double *stats, ogc_stream_t stream);

/* Deferred normalisation: inside a SharedMLP the GroupNorm (+ ReLU) output of one layer is only ever read by the next
 * layer's convolution, so it need not be written.  ogc_group_norm_coeffs turns the statistics of layer l (supplied by
 * the producing convolution, or computed here from x when stats == NULL; ws: 2*b*groups*ogc_group_norm_stats_slots() f64 then) into mean / rstd
 * (b*groups) for the backward pass and the per-(b, channel) affine map a, bb (b*c):  GroupNorm(x)[b, ch] = a*x + bb.
 * ogc_conv1x1_gemm_affine is the forward convolution of layer l+1 on act(a*in + bb) applied while loading (relu != 0:
 * act = ReLU; groups > 0: also the statistics of ITS output, as ogc_conv1x1_gemm_gnstats, same restrictions);
 * ogc_conv1x1_wgrad_affine is that layer's weight gradient with the same recomputed operand.  The input gradient is
 * ogc_conv1x1_gemm(transpose_a = 1) followed by ogc_group_norm_bwd on (in, mean, rstd), unchanged. */
int ogc_group_norm_coeffs(int b, int c, int hw, int groups, float eps, const float *x, const float *gamma,
                          const float *beta, const double *stats, int slots, double *ws, float *mean, float *rstd,
                          float *a, float *bb, ogc_stream_t stream);
int ogc_conv1x1_gemm_affine(int b, int M, int K, int hw, int relu, int groups, const float *w, const float *in,
                            const float *pa, const float *pb, float *out, double *stats, ogc_stream_t stream);
int ogc_conv1x1_wgrad_affine(int b, int cin, int cout, int hw, int relu, const float *x, const float *pa,
                             const float *pb, const float *dy, float *dw, ogc_stream_t stream);
/* The LAST layer of a set-abstraction MLP backwards for layers wider than the fused GroupNorm path takes (64 channels), with the
 * gradient of its pooled GroupNorm in the sparse form of ogc_group_norm_maxpool_bwd_sparse below: g_y (the size of the layer's
 * activation) is rebuilt from (y, coef2, inj) while y is loaded instead of being written by one kernel and read by two.
 *   ogc_conv1x1_wgrad_affine_pooled: ogc_conv1x1_wgrad_affine with (y, coef2, inj) for dy;
 *   ogc_conv1x1_dgrad_pooled:        grad_z[b] = w^T . g_y[b]  (ogc_amd/csrc/gemm_chunk.hip), w (cout, cin); needs >= 1024 tiles of
 *                                    64 positions (OGC_ERR_UNSUPPORTED otherwise), hw % 64 == 0.
 * nsample in {16, 32, 64} dividing hw; fp32 operands.  Reference: utils/pointnet2_util.py:38-42, utils/nn_util.py:45-85. */
int ogc_conv1x1_wgrad_affine_pooled(int b, int cin, int cout, int hw, int relu, int nsample, const float *x, const float *pa,
                                    const float *pb, const float *y, const float *coef2, const float *inj, float *dw,
                                    ogc_stream_t stream);
int ogc_conv1x1_dgrad_pooled(int b, int cin, int cout, int hw, int nsample, const float *w, const float *y, const float *coef2,
                             const float *inj, float *grad_z, ogc_stream_t stream);

/* ogc_group_norm_fwd / ogc_group_norm_maxpool_fwd with the statistics supplied (`slots` copies, see above). */
int ogc_group_norm_fwd_stats(int b, int c, int hw, int groups, float eps, int relu, const float *x,
                             const float *gamma, const float *beta, float *y, float *mean, float *rstd,
                             const double *stats, int slots, ogc_stream_t stream);
int ogc_group_norm_maxpool_fwd_stats(int b, int c, int p, int s, int groups, float eps, int relu, const float *x,
                                     const float *gamma, const float *beta, float *out, int *argmax, float *mean,
                                     float *rstd, const double *stats, int slots, ogc_stream_t stream);

/* Max-pool of a set-abstraction MLP without re-reading its last layer's output
 *   utils/pointnet2_util.py:38-42: new_features = mlp(grouped); F.max_pool2d(new_features, [1, nsample]).
 * The last layer is conv -> GroupNorm -> ReLU, and y -> act(a*y + bb) is monotone per (batch, channel): the pooled
 * value is the activation of the LARGEST raw output of the neighbourhood when a >= 0 and of the SMALLEST when a < 0,
 * and sign(a) = sign(gamma) is known before the convolution runs.
 * ogc_conv1x1_gemm_affine_pool is ogc_conv1x1_gemm_affine (groups >= 1: statistics are always produced) whose
 * positions are (centre, neighbour) pairs, hw = centres * nsample with nsample in {16, 32, 64}; next_gamma (M) is the
 * scale of the GroupNorm that follows.  Next to out and stats it writes yext (b, M, centres) — per row the largest
 * output of each neighbourhood where next_gamma >= 0, the smallest where it is negative — and aext, the index in
 * [0, nsample) of the first neighbour attaining it.  ogc_group_norm_pool_extremes turns those and the statistics into
 * exactly what ogc_group_norm_maxpool_fwd_stats computes from the full tensor — out (b, c, p), argmax, mean, rstd —
 * so the backward pass (ogc_group_norm_maxpool_bwd) is unchanged.  (Two DIFFERENT raw values that round to the same
 * activation are told apart here and not there; with gamma == 0, and where the ReLU gates the whole neighbourhood, both
 * report neighbour 0.) */
int ogc_conv1x1_gemm_affine_pool(int b, int M, int K, int hw, int relu, int groups, int nsample, const float *w,
                                 const float *in, const float *pa, const float *pb, const float *next_gamma,
                                 float *out, double *stats, float *yext, int *aext, ogc_stream_t stream);
int ogc_group_norm_pool_extremes(int b, int c, int p, int s, int groups, float eps, int relu, const float *yext,
                                 const int *aext, const float *gamma, const float *beta, float *out, int *argmax,
                                 float *mean, float *rstd, const double *stats, int slots, ogc_stream_t stream);

/* The two nearest-neighbour distance terms of the Chamfer loss and their gradient (fused extension; replaces the gather /
 * difference / norm sequence of losses/flow_loss_unsup.py:24-35 around the two knn(1, ., .) searches, which stay ogc_knn calls).
 * p1 (b, n1, 3) = pc1 + flow, pc2 (b, n2, 3), idx12 (b, n1) = nearest point of pc2 for every point of p1, idx21 (b, n2) the other
 * way round; p = 1 or 2 (the reference's loss_norm).  dist1 (b, n1), dist2 (b, n2) as the reference's dist1 / dist2.
 * _grad: grad_p1 (b, n1, 3) = gradient of sum(g1 * dist1) + sum(g2 * dist2) w.r.t. p1 with the indices held constant
 * (`idx.detach()` in the reference); zeroed by the entry point, accumulated with fp32 atomics. */
int ogc_chamfer_terms(int b, int n1, int n2, int p, const float *p1, const float *pc2, const int *idx12, const int *idx21,
                      float *dist1, float *dist2, ogc_stream_t stream);
int ogc_chamfer_terms_grad(int b, int n1, int n2, int p, const float *p1, const float *pc2, const int *idx12, const int *idx21,
                           const float *g1, const float *g2, float *grad_p1, ogc_stream_t stream);

/* The element-wise glue of FlowStep3D's refinement loop in inference (fused extensions; csrc/flow_step.hip).  Each replaces a
 * run of framework operators of models/flownet_kitti.py on tensors of a few thousand elements, with the same fp32 operations in
 * the same order (one rounding each, nothing contracted) — except ogc_linear_cn and ogc_soft_corr_flow, whose dot products are
 * FMA chains in an order of their own (the reference calls addmm / normalises and calls bmm): those two agree with the reference
 * within tolerance, not to the bit:
 *   ogc_gather_xyz_pair  out (b, 3, m) = xyz (b, 3, n)[:, :, idx (b, m)] and out_t (b, m, 3) = its transpose
 *                        (gather_operation + transpose(1, 2).contiguous(), utils/flowstep3d_util.py:110-118);
 *   ogc_flow_advance     d = delta * scale (no multiplication when scale == 1), new = cur + d, flow = new - ref, all (b, 3, n);
 *                        out_delta, out_new_t (b, n, 3) and out_flow may be null (flownet_kitti.py:229-231, :245-250: scale is
 *                        the fp32 rounding of 1 / (k_decay_fact * it + 1), as torch divides by a Python scalar);
 *   ogc_linear_cn        y (b, cout, n) = weight (cout, cin) x (b, cin, n) + bias, cout <= 4 — nn.Linear between two
 *                        transposes (flownet_kitti.py:19, :38), fp32 FMA chains over the four quarters of cin, added in order; bias may be null;
 *   ogc_gru_reset        hx (b, c + cx, n) = cat([h, x]); rc (b, c, n, s) the reset gate's un-pooled convolution output, batch
 *                        stride rc_batch_stride floats: out (b, c + cx, n) = cat([sigmoid(max_s rc) * h, x]) (:147-149);
 *   ogc_gru_blend        z = sigmoid(max_s zc), q = tanh(max_s qc), out (b, c, n) = (1 - z) * h + z * q (:147, :149-150); zc, qc
 *                        (b, c, n, s) and h (b, c, n) with their batch strides in floats.
 *   ogc_soft_corr_flow   GlobalCorrLayer's dense soft correspondence and coarse flow (:53-70): w_ij = exp(-(1 - cos(f1_i, f2_j)) /
 *                        (exp(*epsilon) + 0.03)) where (|p_i|^2 + |q_j|^2) - 2 p_i.q_j < support, else 0; flow (b, 3, n1) =
 *                        sum_j w_ij q_j / (sum_j w_ij + 1e-8) - p_i.  pc1 (b, 3, n1), pc2 (b, 3, n2), f1 (b, c, n1), f2 (b, c, n2),
 *                        c a multiple of 4 up to 256; epsilon: the layer's parameter on the device (no host read).
 *   ogc_three_nn_weights weight (b, n, 3) from ogc_three_nn's squared distances dist2 (b, n, 3): r_k = 1 / max(sqrt(d2_k), 1e-10)
 *                        (mode 0, utils/flowstep3d_util.py:169-170) or 1 / (sqrt(d2_k) + 1e-8) (mode 1, utils/pointnet2_util.py:99-101),
 *                        weight_k = r_k / ((r_0 + r_1) + r_2).
 * When s is a multiple of 4: gate pointers 16-byte aligned and gate batch strides multiples of 4 floats (other s: no requirement). */
int ogc_gather_xyz_pair(int b, int n, int m, const float *xyz, const int *idx, float *out, float *out_t, ogc_stream_t stream);
int ogc_flow_advance(int b, int n, float scale, const float *cur, const float *delta, const float *ref, float *out_delta,
                     float *out_new, float *out_new_t, float *out_flow, ogc_stream_t stream);
int ogc_linear_cn(int b, int cin, int cout, int n, const float *x, const float *weight, const float *bias, float *y,
                  ogc_stream_t stream);
int ogc_three_nn_weights(int b, int n, int mode, const float *dist2, float *weight, ogc_stream_t stream);
int ogc_soft_corr_flow(int b, int n1, int n2, int c, float support, const float *epsilon, const float *pc1, const float *pc2,
                       const float *f1, const float *f2, float *flow, ogc_stream_t stream);
int ogc_gru_reset(int b, int c, int cx, int n, int s, const float *rc, long long rc_batch_stride, const float *hx, float *out,
                  ogc_stream_t stream);
int ogc_gru_blend(int b, int c, int n, int s, const float *zc, long long zc_batch_stride, const float *qc,
                  long long qc_batch_stride, const float *h, long long h_batch_stride, float *out, ogc_stream_t stream);

/* One zero fill per training step (fused extension; nothing in the reference to replace: its Python zero-fills every gradient
 * buffer it hands to the native module, pointnet2/pointnet2.py:73,181,224).  ogc_zero_arena_begin fills [base, base + bytes)
 * with zeros by ONE launch on `stream`; until ogc_zero_arena_end every operator of this library that would zero an
 * accumulator lying inside that region, on that stream, skips its own fill.  The caller hands every byte of the region to at
 * most one operator between the two calls.  bytes and base multiples of 4. */
int ogc_zero_arena_begin(void *base, int bytes, ogc_stream_t stream);
int ogc_zero_arena_end(void);

/* ---- 16-bit activations (`matmul_precision: bf16` of BASELINE config 2, verdict row g2) ------------------------------------------
 * Inside a set-abstraction MLP (reference: utils/nn_util.py:45-85 on models/segnet_ogcdr.py:26-41) the only tensors of the size
 * of an activation are the convolutions' raw outputs y and the gradients with respect to them; under bf16 operands every kernel
 * that streams one is bound by its bytes.  The `_h` entry points below are the entry points of the same name with those tensors
 * (and only those) stored as bf16 — ogc_bf16_t, round to nearest even on the way out; every argument is otherwise unchanged, and
 * so is the arithmetic: fp32 accumulation, fp64 statistics, fp32 coefficients, fp32 pooled outputs.  Statistics and
 * neighbourhood extremes a kernel produces next to a 16-bit output are those of the ROUNDED values, so that the norm that
 * follows describes exactly the tensor it reads.  They need ogc_set_matmul_precision(1) (operands are bf16 as well —
 * including the pooled forms, which keep fp32 operands for fp32 tensors) and 8-byte aligned tensors; OGC_ERR_UNSUPPORTED
 * otherwise.  ogc_conv1x1_wgrad_xf_h: x fp32 (the relative coordinates of a grouped first layer), dy bf16. */
int ogc_group_linear_fwd_h(int b, int m, int n, int npoints, int nsample, int groups, const float *P, const int *idx,
                           const float *rel, const float *wx, ogc_bf16_t *y, double *stats, ogc_stream_t stream);
/* ... with P stored point-major, Pt (b, n, m): a position's channels are contiguous and one lane fetches them with 16-byte loads
 * (a quarter of the cache-line lookups of the channel-major gather, which bound the 16-bit form).  m % 64 == 0, m / groups in
 * {16, 32, 64} (or groups == 0), an even position count; y bit-identical to ogc_group_linear_fwd_h on the transposed P. */
int ogc_group_linear_fwd_pt_h(int b, int m, int n, int npoints, int nsample, int groups, const float *Pt, const int *idx,
                              const float *rel, const float *wx, ogc_bf16_t *y, double *stats, ogc_stream_t stream);
int ogc_group_points_grad_rev_h(int b, int c, int n, int npoints, int nsample, const ogc_bf16_t *grad_out, const int *rev_start,
                                const unsigned short *rev_pos, const unsigned short *heads, float *grad_points,
                                ogc_stream_t stream);
int ogc_group_points_grad_rev_dwx_h(int b, int c, int n, int npoints, int nsample, const ogc_bf16_t *grad_out, const int *rev_start,
                                    const unsigned short *rev_pos, const unsigned short *heads, const float *rel,
                                    float *grad_points, float *dwx, ogc_stream_t stream);
int ogc_conv1x1_gemm_h(int b, int M, int K, int hw, int transpose_a, const float *w, const ogc_bf16_t *in, ogc_bf16_t *out,
                       ogc_stream_t stream);
int ogc_conv1x1_gemm_affine_h(int b, int M, int K, int hw, int relu, int groups, const float *w, const ogc_bf16_t *in,
                              const float *pa, const float *pb, ogc_bf16_t *out, double *stats, ogc_stream_t stream);
int ogc_conv1x1_gemm_affine_pool_h(int b, int M, int K, int hw, int relu, int groups, int nsample, const float *w,
                                   const ogc_bf16_t *in, const float *pa, const float *pb, const float *next_gamma,
                                   ogc_bf16_t *out, double *stats, float *yext, int *aext, ogc_stream_t stream);
int ogc_conv1x1_wgrad_xf_h(int b, int cin, int cout, int hw, const float *x, const ogc_bf16_t *dy, float *dw,
                           ogc_stream_t stream);
int ogc_conv1x1_wgrad_affine_h(int b, int cin, int cout, int hw, int relu, const ogc_bf16_t *x, const float *pa,
                               const float *pb, const ogc_bf16_t *dy, float *dw, ogc_stream_t stream);
int ogc_conv1x1_wgrad_affine_pooled_h(int b, int cin, int cout, int hw, int relu, int nsample, const ogc_bf16_t *x,
                                      const float *pa, const float *pb, const ogc_bf16_t *y, const float *coef2,
                                      const float *inj, float *dw, ogc_stream_t stream);
int ogc_conv1x1_dgrad_pooled_h(int b, int cin, int cout, int hw, int nsample, const float *w, const ogc_bf16_t *y,
                               const float *coef2, const float *inj, ogc_bf16_t *grad_z, ogc_stream_t stream);
int ogc_conv1x1_wgrad_moments_h(int b, int cin, int cout, int hw, int relu, const ogc_bf16_t *y_prev, const float *pa,
                                const float *pb, const ogc_bf16_t *grad_y, float *moments, ogc_stream_t stream);
int ogc_conv1x1_wgrad_moments_pooled_h(int b, int cin, int cout, int hw, int relu, int nsample, const ogc_bf16_t *y_prev,
                                       const float *pa, const float *pb, const ogc_bf16_t *y, const float *coef2,
                                       const float *inj, float *moments, ogc_stream_t stream);
int ogc_conv1x1_dgrad_adjoint_h(int b, int cin, int cout, int hw, int relu, const float *w, const ogc_bf16_t *grad_y,
                                const ogc_bf16_t *y_prev, const float *pa, const float *pb, const float *coef,
                                ogc_bf16_t *grad_prev, ogc_stream_t stream);
int ogc_conv1x1_dgrad_adjoint_pooled_h(int b, int cin, int cout, int hw, int relu, int nsample, const float *w,
                                       const ogc_bf16_t *y, const float *coef2, const float *inj, const ogc_bf16_t *y_prev,
                                       const float *pa, const float *pb, const float *coef, ogc_bf16_t *grad_prev,
                                       ogc_stream_t stream);
int ogc_group_norm_bwd_h(int b, int c, int hw, int groups, int relu, const ogc_bf16_t *x, const float *gamma,
                         const float *beta, const float *mean, const float *rstd, const ogc_bf16_t *grad_y,
                         ogc_bf16_t *grad_x, float *grad_gamma, float *grad_beta, double *ws, ogc_stream_t stream);
int ogc_group_norm_maxpool_bwd_sparse_h(int b, int c, int p, int s, int groups, int relu, const ogc_bf16_t *x,
                                        const float *x_at_argmax, const float *gamma, const float *mean, const float *rstd,
                                        const float *out, const int *argmax, const float *grad_out, float *coef2, float *inj,
                                        float *grad_gamma, float *grad_beta, double *ws, ogc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* OGC_OPS_H */
