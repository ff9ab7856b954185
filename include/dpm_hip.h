/* dpm_hip.h -- C ABI of libdpm_hip.so: the MI355X (gfx950) kernels behind DeepPointMap's
 * encode -> match -> register hot path.
 *
 * The reference has no FFI layer of its own: its lower boundary is the string-keyed operator
 * tables `Sampler(method)` / `Querier(method)` (network/encoder/utils.py:21-28,129-133), the
 * third-party pytorch3d ops they dispatch to (utils.py:12,94,102,115,278-283;
 * system/modules/utils.py:10,80) and plain torch modules.  Each entry point below names the
 * reference interface it replaces.  INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller, the
 *    library never allocates, frees or retains it; scratch is passed in as `workspace`
 *    (sized by the entry point's dpm_*_workspace_bytes; DESIGN.md section 3 has the layout rules).
 *  - all tensors are fp32, dense, "point-major": xyz (B,N,3), features (B,N,C); index
 *    tensors are int32; `lengths[b]` = number of valid (leading) points of frame b.
 *  - every call is asynchronous on `stream` (a hipStream_t passed as void*), re-entrant and
 *    free of global mutable state, so one Decoder may be driven from several host threads
 *    (reference system/core.py:54-57,93-103).
 *  - return value: 0 = ok, <0 = invalid argument / unsupported shape, >0 = hipError_t.
 */
#ifndef DPM_HIP_H
#define DPM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *dpm_stream_t;

#define DPM_OK 0
#define DPM_EINVAL (-1)
#define DPM_EUNSUPPORTED (-2)

#define DPM_ACT_NONE 0
#define DPM_ACT_RELU 1
#define DPM_ACT_SIGMOID 2

/* library / ABI version (major*1000+minor) and a printable name for a status code.  The shipped library reads no
 * environment variable in any entry point.  A build with -DDPM_EXPERIMENT (measurement switches that skip work or swap
 * kernel layouts, read with getenv; scripts/ only) ORs DPM_VERSION_EXPERIMENT into the version so that callers can
 * refuse it: bench.py does. */
#define DPM_VERSION_EXPERIMENT 0x40000000
int dpm_version(void);
const char *dpm_error_string(int status);

/* Encoder.forward input staging (network/encoder/encoder.py:52): channel-first (B,C,N) points +
 * bool padding (B,N; nonzero = padded) -> xyz (B,N,3), lengths (B,) = count of valid points.
 * Valid points must be the leading ones, as the reference's FPS assumes (utils.py:255). */
int dpm_prepare_points(const float *points_cf, const uint8_t *padding, int B, int C, int N,
                       float *xyz, int32_t *lengths, dpm_stream_t stream);

/* (B,R,C) point-major -> (B,C,R) channel-first (the layout Encoder.forward returns). */
int dpm_to_channel_first(const float *x, int B, int R, int C, float *out, dpm_stream_t stream);
/* The same with the output rows ldo >= R floats apart (batch elements C * ldo apart).  The decoder stages the reference's
 * channel-first descriptors (B,131,M) (odometry.py:47-49) as token rows of 132 floats, so that the 128 feature columns of
 * a row start 16-byte aligned for the projection GEMM (descriptor_attention.py:24-30). */
int dpm_to_channel_first_ld(const float *x, int B, int R, int C, float *out, int ldo, dpm_stream_t stream);

/* The encoder's return triple [coor (B,3,S), feat (B,C,S), padding (B,S; 1 = padded)] (network/encoder/encoder.py:51-69)
 * from the point-major level (xyz (B,S,3), fea (B,S,C), lengths), and -- desc != NULL -- the unified descriptor
 * (B,C+3,S) = [feat ; coor * coor_scale] of ExtractionThread.process (system/modules/odometry.py:47-49), in one pass. */
int dpm_emit_descriptors(const float *xyz, const float *fea, const int32_t *lengths, int B, int S, int C,
                         double coor_scale, float *coor, float *feat, uint8_t *padding, float *desc, dpm_stream_t stream);

/* Lower sampling levels as prefixes of the first level's picks (the four lower Sampler.fps calls of
 * network/encoder/pointnext.py:38-47 when npoint is descending): for level i with K = npoint[i] (host array),
 * xyz_out / idx_out hold the levels back to back ((B,K,3) / (B,K) each), len_out is (n_levels,B). */
int dpm_nested_levels(const float *xyz0, const int32_t *len0, int B, int K0, int n_levels, const int32_t *npoint,
                      float *xyz_out, int32_t *idx_out, int32_t *len_out, dpm_stream_t stream);

/* out[p, m, c] = src[index[p] * frame_stride + m * ld + c], p < n, m < rows, c < cols: per-pair copies of per-frame
 * rows (what torch.index_select did for the pair lists of odometry.py:103-127). */
int dpm_gather_frames(const float *src, long long frame_stride, int rows, int ld, int cols, const int32_t *index, int n,
                      float *out, dpm_stream_t stream);

/* Sampler.fps / Sampler.fps_t3d == pytorch3d.ops.sample_farthest_points
 * (network/encoder/utils.py:210-285): start index 0, dist = (dx*dx+dy*dy)+dz*dz evaluated in
 * fp32 without contraction, next pick = first argmax.  idx (B,K) is -1 where lengths[b] < K;
 * new_xyz (B,K,3) is zero there (masked_gather, utils.py:298-343); new_lengths[b] = number of
 * idx >= 0.  workspace: dpm_fps_workspace_bytes(B,N,K) bytes. */
size_t dpm_fps_workspace_bytes(int B, int N, int K);
int dpm_fps(const float *xyz, const int32_t *lengths, int B, int N, int K, int32_t *idx,
            float *new_xyz, int32_t *new_lengths, void *workspace, dpm_stream_t stream);
/* same, with the algorithm forced: 0 = auto (1 up to 16 384 points, 5 up to 65 536, 1 again beyond), 1 = register / brute force,
 * 2 = bucket-pruned over Z-ordered grid cells (N <= 65 536), 5 = the bucket kernel over a Sort-Tile-Recursive packing
 * (16 384 < N <= 65 536).  All give identical bits; the tests run all of them.  3, 4, 6, 7 (speculative multi-pick rounds,
 * one-wave tree: exact but slower, removed in round 3) return DPM_EUNSUPPORTED. */
int dpm_fps_ex(const float *xyz, const int32_t *lengths, int B, int N, int K, int32_t *idx,
               float *new_xyz, int32_t *new_lengths, void *workspace, int algo, dpm_stream_t stream);
/* `random_start_point=True` (utils.py:248): frame b starts from point start[b] (clamped to its valid points) instead of
 * point 0; the caller draws the indices (the reference: random.randint(0, lengths[n] - 1), one draw per frame in batch
 * order).  Default algorithm choice (1 / 5 / 2 by N). */
int dpm_fps_start(const float *xyz, const int32_t *lengths, const int32_t *start, int B, int N, int K, int32_t *idx,
                  float *new_xyz, int32_t *new_lengths, void *workspace, dpm_stream_t stream);

/* Querier.hybrid_query / hybrid_query_t3d == pytorch3d.ops.knn_points + radius mask
 * (network/encoder/utils.py:76-89,113-123): for each centre the K nearest valid points, slots
 * whose squared distance exceeds radius^2 replaced by the nearest index.  Slot 0 is the nearest
 * point.  idx (B,S,K).  Distances and tie handling reproduce the reference's CPU path exactly
 * (see csrc/knn.hip).  workspace: dpm_knn_workspace_bytes(B,N) bytes (0 for small N; NULL selects
 * the brute-force path). */
size_t dpm_knn_workspace_bytes(int B, int N);
int dpm_knn_hybrid(const float *points, const int32_t *lengths, const float *centers, int B, int N,
                   int S, int K, double radius, int32_t *idx, void *workspace, dpm_stream_t stream);

/* Same query when the centres are a SUBSET of the points (SetAbstraction centres are FPS picks of `points`) and the
 * self-query of ALL points with the same radius and K has already been answered (the preceding LocalAggregation):
 * center_src (B,S) = index of centre s in `points` (the FPS index, -1 for padded centres), reuse_idx (B,N,K) = that
 * earlier answer.  Rows with center_src >= 0 are copied (they are the identical computation), padded ones computed. */
int dpm_knn_hybrid_reuse(const float *points, const int32_t *lengths, const float *centers, int B, int N,
                         int S, int K, double radius, int32_t *idx, void *workspace, const int32_t *reuse_idx,
                         const int32_t *center_src, dpm_stream_t stream);

/* dpm_knn_hybrid in two calls sharing one workspace (N >= 1024, the grid path): the grid depends on the points and
 * the radius only, so a caller that pipelines frames builds it while the frames are still being sampled and runs the
 * search when the centres exist.  One search per build (the build resets the tie queue the search fills). */
int dpm_knn_build_grid(const float *points, const int32_t *lengths, int B, int N, double radius, void *workspace,
                       dpm_stream_t stream);
int dpm_knn_hybrid_prebuilt(const float *points, const int32_t *lengths, const float *centers, int B, int N,
                            int S, int K, double radius, int32_t *idx, void *workspace, dpm_stream_t stream);
/* Read-only census of what the last build and search on `workspace` (B frames of N >= 1024 points) did, for tests and
 * debugging: out (device, 8 B + 2 32-bit words) receives per frame the grid header -- lox, loy, 1 / cell edge (floats),
 * cells per axis, the margin err2 of the expanded-form distance (float), the half-widths H of the covering and h of the
 * inner block, 0 -- then the number of tied rows offered to the tie queue (a row offered while the queue is full is offered
 * once more by the full search) and the number of rows the fast search left to the full search.  Two copies in stream
 * order; no kernel counts anything for it. */
int dpm_knn_debug_census(const void *workspace, int B, int N, int32_t *out, dpm_stream_t stream);

/* Querier.ball_query / ball_query_t3d == pytorch3d.ops.ball_query (utils.py:57-73,99-110): the K
 * smallest indices among the valid points within `radius` (expanded-form distance, like the
 * reference), ascending, padded with the first of them.  idx (B,S,K). */
int dpm_ball_query(const float *points, const int32_t *lengths, const float *centers, int B, int N, int S,
                   int K, double radius, int32_t *idx, dpm_stream_t stream);

/* Sampler.voxel (network/encoder/utils.py:150-207): per frame, the point nearest the centre of every occupied voxel
 * (smallest index among equals) among the points within `sample_range` of the origin, in ascending voxel-id order; if
 * more than K voxels are occupied, the K most populated ones in the order torch.topk(counts, K) returns them (its CPU
 * kernel's choice and order among equal counts, replayed).  points (B,N,D) with D >= 3 (xyz first), padding (B,N)
 * uint8 (1 = padded: moved to 2*sample_range before the bounding box is taken, as the reference does).
 * Two calls, because the grid size is data dependent:
 *   dpm_voxel_sampler_bounds  -> hdr (B,8) floats: xyz_min[3], X, Y, Z (integer-valued, utils.py:159-161), 0, 0;
 *                                the caller reads X*Y*Z back and sizes the workspace for max_cells >= max_b X*Y*Z;
 *   dpm_voxel_sampler_select  -> sel (B,cap) original point indices in output order, -1 = padding rows
 *                                (utils.py:192-198), and n_unique (B) = occupied voxels.  K >= 1: cap == K;
 *                                K < 0 (the reference's K=None, B == 1 there): cap == N, all voxels.
 *                                A frame whose grid exceeds max_cells (or is not finite) gets hdr[6] = 1 and no points.
 *                                hdr[7] = 1 marks a frame where two points of a voxel were exactly equally near its
 *                                centre: the reference's pick then follows its unstable torch.sort, which one thread
 *                                replays over the frame's N distances (exact, slow: lattices / duplicated points only).
 * N <= 2^24.  workspace: dpm_voxel_sampler_workspace_bytes(B, N, max_cells). */
int dpm_voxel_sampler_bounds(const float *points, const uint8_t *padding, int B, int N, int D, double voxel_size,
                             double sample_range, float *hdr, dpm_stream_t stream);
size_t dpm_voxel_sampler_workspace_bytes(int B, int N, long long max_cells);
int dpm_voxel_sampler_select(const float *points, const uint8_t *padding, int B, int N, int D, double voxel_size,
                             double sample_range, float *hdr, long long max_cells, int K, int32_t *sel, int cap,
                             int32_t *n_unique, void *workspace, dpm_stream_t stream);

/* ---------------------------------------------------------------- pose graph (host) ---- */

/* HOST function (no GPU involved).  PoseGraph.__optim_open3d (system/modules/pose_graph.py:565-613):
 * open3d.pipelines.registration.global_optimization(graph, GlobalOptimizationLevenbergMarquardt(),
 * GlobalOptimizationConvergenceCriteria(), GlobalOptimizationOption(edge_prune_threshold=0, preference_loop_closure=2,
 * reference_node)) on a graph whose edges are all certain (pose_graph.py:597) -- a restatement of open3d 0.16's published
 * algorithm (parity unpinned: open3d is absent; see deeppointmap_amd/posegraph_optim.py).
 * poses (n,4,4) row-major doubles (scan -> world); edge k: src[k] -> dst[k], X (E,4,4) = the o3d PoseGraphEdge
 * transformation (source-scan coordinates into the target scan's frame), info (E,6,6) rotation block first.
 * criteria: NULL = open3d's defaults, else 8 doubles {max_iteration, min_relative_increment,
 * min_relative_residual_increment, min_right_term, min_residual, max_iteration_lm, upper_scale_factor,
 * lower_scale_factor}.  out_poses (n,4,4): refined poses, node `reference_node` unchanged.  stats (6): iterations,
 * residual at the start, residual at the end -- of the first and of the second Levenberg-Marquardt pass. */
int dpm_posegraph_optimize(const double *poses, int n, const int32_t *src, const int32_t *dst, const double *X,
                           const double *info, int E, int reference_node, const double *criteria, double *out_poses,
                           double *stats);

/* HOST function (no GPU involved): torch.topk(values, k, largest, sorted=True) on one row of n floats without NaNs, by
 * the step-by-step replay of its CPU kernel that the device code uses (csrc/topk_emulate.h, same source compiled for
 * the host) -- which elements survive and in which order among equal values.  out_idx (k).  Exists so that the replay
 * can be held to torch.topk by tests that run without a GPU. */
int dpm_host_topk_replay(const float *values, int n, int k, int largest, int32_t *out_idx);
/* Same for torch.sort(values, descending, stable=False) -> out_idx (n): std::sort over (value, index) pairs. */
int dpm_host_sort_replay(const float *values, int n, int descending, int32_t *out_idx);

/* SetAbstraction / LocalAggregation body (network/encoder/pointnext.py:52-61,97-107):
 * out[b,s,:] = max_k relu(LN(W [fea[idx[b,s,k]], (xyz[idx]-center)/radius] + bias)).
 * W (Cout, Cin+3) row-major exactly as the Conv2d weight (Cout,Cin+3,1,1): first Cin columns
 * features, last 3 relative xyz.  LN: eps 1e-5, biased variance, affine (gamma, beta).
 * fp32 MFMA for Cout in {32,64,128,256,512} and K in {16,32} (every shipped layer); the _generic
 * entry is the plain-VALU kernel for any other shape (same contract). */
int dpm_group_mlp_max_generic(const float *xyz, const float *fea, const float *centers,
                              const int32_t *idx, const float *W, const float *bias, const float *gamma,
                              const float *beta, int B, int N, int S, int K, int Cin, int Cout, double radius,
                              float *out, dpm_stream_t stream);
int dpm_group_mlp_max(const float *xyz, const float *fea, const float *centers, const int32_t *idx,
                      const float *W, const float *bias, const float *gamma, const float *beta,
                      int B, int N, int S, int K, int Cin, int Cout, double radius, float *out,
                      dpm_stream_t stream);

/* First-stage SetAbstraction with Encoder.point_mlp0 (encoder.py:25,53) folded in: the input
 * features are W0 xyz + b0 (W0 (Cin,3) = the Conv1d weight, b0 (Cin)), evaluated inside the
 * gather, so the (B,N,Cin) level-0 feature tensor is never written or read.  Cout in {32,64,128},
 * K in {16,32}; otherwise DPM_EUNSUPPORTED (callers then materialise the features with dpm_linear). */
int dpm_group_mlp_max_from_xyz(const float *xyz, const float *W0, const float *b0, const float *centers,
                               const int32_t *idx, const float *W, const float *bias, const float *gamma,
                               const float *beta, int B, int N, int S, int K, int Cin, int Cout,
                               double radius, float *out, dpm_stream_t stream);

/* The same layer with the projection hoisted out of the gather ("project before gather", the encoder's default):
 * W [fea_n ; rel] + b = (W_f fea_n + b) + W_r rel, so P = fea W_f^T + b (B,N,Cout) is computed once per POINT with
 * dpm_linear (x = fea, W = the first Cin columns, ldw = Cin+3) and this kernel does the per-(centre, neighbour) rest:
 * out[b,s,:] = max_k relu(LN(P[idx[b,s,k]] + W_rel (xyz[idx]-center)/radius)).  W_rel points at column Cin of the
 * Conv2d weight, ldw_rel = Cin+3.  Cout in {32,64,128,256,512}; P and out 16-byte aligned.
 * dpm_group_affine_ln_max: first-stage variant, P is affine in the point itself (P = A xyz + c with A (Cout,3) =
 * W_f W0 and c (Cout) = W_f b0 + b, both produced with dpm_linear) and is evaluated on the fly; Cout in {32,64,128}. */
int dpm_group_gather_ln_max(const float *P, const float *xyz, const float *centers, const int32_t *idx,
                            const float *W_rel, int ldw_rel, const float *gamma, const float *beta, int B, int N,
                            int S, int K, int Cout, double radius, float *out, dpm_stream_t stream);
int dpm_group_affine_ln_max(const float *A, const float *cvec, const float *xyz, const float *centers,
                            const int32_t *idx, const float *W_rel, int ldw_rel, const float *gamma,
                            const float *beta, int B, int N, int S, int K, int Cout, double radius, float *out,
                            dpm_stream_t stream);
/* The folded form of dpm_group_gather_ln_max (round 5): the relative-coordinate term W_rel (p - c) / radius is linear in the point
 * and in the centre separately, so P' = P + xyz (W_rel / radius)^T is made once per point by the projection's epilogue
 * (dpm_linear_bf16x3_rank3) and this kernel computes out[b,s,:] = max_k relu(LN(P'[idx[b,s,k]] - (W_rel / radius) center)):
 * four subtractions instead of fifteen operations per gathered row and lane, no coordinates gathered.  Same shapes and alignment
 * as dpm_group_gather_ln_max.  |W_rel p / radius| exceeds the term it replaces by up to |p| / radius, so the pre-LayerNorm values
 * carry ~1e-6 relative rounding error instead of ~1e-7 (DESIGN.md section 4 has the measured effect on descriptors and poses).
 * dpm_group_affine_ln_max folds the same way internally (A + W_rel / radius). */
int dpm_group_gather_ln_max_folded(const float *P, const float *centers, const int32_t *idx, const float *W_rel, int ldw_rel,
                                   const float *gamma, const float *beta, int B, int N, int S, int K, int Cout, double radius,
                                   float *out, dpm_stream_t stream);
/* The folded forms for a layer whose LayerNorm mean removal has been moved into its weights (round 5): the caller passes
 * W' = (I - 11^T / Cout) W -- every column of [W_f | W_rel], the bias, and for the affine form the columns of A and the vector
 * cvec, have zero mean over the Cout output channels -- so that every pre-LayerNorm row (network/encoder/pointnext.py:52-61: the
 * grouped features after the 1x1 Conv2d) has zero mean by construction and the kernels compute the variance from the rows as they
 * are (no row sum, no subtraction: about a third of the per-row instructions).  The caller THEN multiplies channel c of the layer
 * (its row of [W_f | W_rel], bias_c; A, cvec) by sign(gamma_c) (+1 for 0): gamma y + beta = |gamma| (sign(gamma) y) + beta is then
 * non-decreasing in the gathered value and commutes with the maximum over the neighbours bit for bit, so |gamma|, beta and the ReLU
 * are applied once per centre (gamma is passed as stored; the kernels take its magnitude; the signs leave the sum of squares, all the
 * variance needs, as it was).  tests/test_centred_algebra.py states the identities in fp64.  PRECONDITIONS, not checked: with other
 * weights the result is a LayerNorm without its mean removal / with |gamma| for gamma.  Otherwise as dpm_group_gather_ln_max_folded / dpm_group_affine_ln_max. */
int dpm_group_gather_ln_max_centred(const float *P, const float *centers, const int32_t *idx, const float *W_rel, int ldw_rel,
                                    const float *gamma, const float *beta, int B, int N, int S, int K, int Cout, double radius,
                                    float *out, dpm_stream_t stream);
int dpm_group_affine_ln_max_centred(const float *A, const float *cvec, const float *xyz, const float *centers,
                                    const int32_t *idx, const float *W_rel, int ldw_rel, const float *gamma,
                                    const float *beta, int B, int N, int S, int K, int Cout, double radius, float *out,
                                    dpm_stream_t stream);

/* 1x1 Conv1d / nn.Linear (build_mlp, network/encoder/utils.py:358-389; decoder heads):
 * out[r, :Cout] = act(x[r,:Cin] W^T + bias + residual[r]); W (Cout,Cin) row-major with leading
 * dimension ldw; x/out/residual have leading dimensions ldx/ldo/ldr (rows R). bias, residual
 * may be NULL. */
int dpm_linear(const float *x, int ldx, const float *W, int ldw, const float *bias,
               const float *residual, int ldr, float *out, int ldo, int R, int Cin, int Cout, int act,
               dpm_stream_t stream);
/* same for `batch` independent problems: operand b lives at ptr + b*stride (strides in floats; a
 * stride of 0 shares the operand).  With W = the second descriptor set this is the M x N similarity
 * contraction of Decoder._descriptor_pairing (decoder.py:185).  fp32 MFMA (exact fp32). */
int dpm_linear_batched(const float *x, int ldx, long long sx, const float *W, int ldw, long long sw,
                       const float *bias, const float *residual, int ldr, long long sr, float *out,
                       int ldo, long long so, int batch, int R, int Cin, int Cout, int act,
                       dpm_stream_t stream);

/* LayerNorm1d / nn.LayerNorm over the channel axis (network/encoder/utils.py:392-402,
 * descriptor_attention.py:20-22): out = act(LN(x + pre)*gamma + beta + post); pre/post NULL-able,
 * all (R,C) with leading dimension = C except x (ldx) and out (ldo). */
int dpm_layernorm(const float *x, int ldx, const float *pre, const float *gamma, const float *beta,
                  const float *post, float *out, int ldo, int R, int C, int act, dpm_stream_t stream);

/* Conv1d(k=1)/nn.Linear followed by LayerNorm1d (network/encoder/utils.py:358-413 build_mlp; the post-norm blocks of
 * network/decoder/descriptor_attention.py:31-48) as ONE kernel: out = act(LN(x W^T + bias + pre) * gamma + beta + post),
 * eps 1e-5, biased variance.  Cout in {32,64,128,256}; pre / post packed (R,Cout) or NULL.  Returns DPM_EUNSUPPORTED
 * for other widths / unaligned operands (run dpm_linear + dpm_layernorm then). */
int dpm_linear_layernorm(const float *x, int ldx, const float *W, int ldw, const float *bias, const float *pre,
                         const float *gamma, const float *beta, const float *post, float *out, int ldo, int R, int Cin,
                         int Cout, int act, dpm_stream_t stream);

/* FeaturePropagation interpolation (network/encoder/pointnext.py:199-216): for each fine point
 * the 3 nearest valid coarse points (expanded-form distance), w_j = (1/max(d_j,1e-8))/sum;
 * out[b,n,:] = cat[fea1[b,n,:D1], sum_j w_j fea2[b,idx_j,:D2]].  S==1 broadcasts fea2. */
int dpm_three_interp_cat(const float *xyz1, const float *xyz2, const int32_t *lengths2,
                         const float *fea1, const float *fea2, int B, int N, int S, int D1, int D2,
                         float *out, dpm_stream_t stream);

/* ---------------------------------------------------------------- decoder -------------- */

/* PositionEmbeddingCoordsSine.forward (network/decoder/descriptor_attention.py:66-83):
 * xyz rows (R, leading dim ld, metres) -> out (R,E); dim_t (F) is the reference's table
 * temperature**(2*(i//2)/F); channels >= 3F are zero. */
int dpm_posemb(const float *xyz, int ld, const float *dim_t, int F, int E, int R, float *out,
               dpm_stream_t stream);

/* Scaled-dot-product core of nn.MultiheadAttention (descriptor_attention.py:14-15,35-45):
 * out[b,m,h*d:(h+1)*d] = softmax(Q_h K_h^T / sqrt(d)) V_h; no masks, dropout 0.  head_dim 32 (every shipped config:
 * model_channel 256, 8 heads) runs on the matrix cores; 8, 16, 64 and 128 (other Decoder(args)) through a generic kernel;
 * other widths return DPM_EUNSUPPORTED.  At head_dim 32 the score product Q K^T is computed on the bf16 matrix pipe from exact
 * three-way bf16 splits of both operands (six term products, fp32 accumulate: fp32-accumulation accuracy; dpm_linear_bf16x3
 * below has the arithmetic), the product with V in exact fp32 -- in every dpm_attention* entry point alike.
 * Q/K/V/out: row leading dims ld*, batch strides s* (in floats). */
int dpm_attention(const float *Q, int ldq, long long sq, const float *K, int ldk, long long sk,
                  const float *V, int ldv, long long sv, float *out, int ldo, long long so, int B, int M,
                  int N, int heads, int head_dim, dpm_stream_t stream);
/* The same with batch element b reading the keys / values of element (b + kv_shift) mod B: the source and target
 * tokens of P pairs stacked as B = 2P sequences with kv_shift = P make both directions of DescriptorAttentionLayer's
 * cross attention (descriptor_attention.py:41-44) one launch. */
int dpm_attention_shifted(const float *Q, int ldq, long long sq, const float *K, int ldk, long long sk,
                          const float *V, int ldv, long long sv, float *out, int ldo, long long so, int B, int M,
                          int N, int heads, int head_dim, int kv_shift, dpm_stream_t stream);

/* ... and with nn.MultiheadAttention's key_padding_mask (descriptor_attention.py:33-42): key_mask (B,N) bytes, non-zero
 * = key n of sequence b is padding and takes no part in the softmax (sequence b reads row (b + kv_shift) mod B of the
 * mask, like its keys); NULL = no mask. */
int dpm_attention_masked(const float *Q, int ldq, long long sq, const float *K, int ldk, long long sk,
                         const float *V, int ldv, long long sv, float *out, int ldo, long long so, int B, int M,
                         int N, int heads, int head_dim, int kv_shift, const uint8_t *key_mask, dpm_stream_t stream);

/* dpm_attention_shifted over batch elements DRAWN from a smaller set of stored sequences: element b's queries are stored
 * sequence seq_index[b] (Q + seq_index[b] * sq), its keys / values stored sequence seq_index[(b + kv_shift) mod B]
 * (K / V + ... * sk / sv); out is per batch element.  The consecutive-frame registrations of a batch (odometry.py:103-127)
 * use every frame as a source and as a target, and the q | k | v projection of the first cross-attention block
 * (descriptor_attention.py:41-44) depends on the frame alone: it is computed once per frame and attended through this
 * entry point -- row-wise kernels give the same rows whatever the row count, so the result equals the per-pair form bit
 * for bit.  head_dim 32 only; seq_index (B) int32 on the device. */
int dpm_attention_indexed(const float *Q, int ldq, long long sq, const float *K, int ldk, long long sk,
                          const float *V, int ldv, long long sv, float *out, int ldo, long long so, int B, int M,
                          int N, int heads, int head_dim, int kv_shift, const int32_t *seq_index, dpm_stream_t stream);

/* Key-split form of dpm_attention_shifted for FEW queries against MANY keys (scan-to-map registration: 256 scan tokens
 * attending a 4096-token map tile, mapping.py:153-155 -> descriptor_attention.py:41-44): the keys are cut into `nsplit`
 * ranges of whole 64-key tiles that run as separate workgroups, and a second kernel joins the ranges (rescaled to the
 * common maximum, fixed order).  Same result up to the rounding of that join.  2 <= nsplit <= 64, every range non-empty;
 * head_dim 32 only; workspace: dpm_attention_split_workspace_bytes(B, M, heads, head_dim, nsplit). */
size_t dpm_attention_split_workspace_bytes(int B, int M, int heads, int head_dim, int nsplit);
int dpm_attention_split(const float *Q, int ldq, long long sq, const float *K, int ldk, long long sk, const float *V,
                        int ldv, long long sv, float *out, int ldo, long long so, int B, int M, int N, int heads,
                        int head_dim, int kv_shift, int nsplit, void *workspace, dpm_stream_t stream);

/* nn.MultiheadAttention's in_proj followed by its attention (descriptor_attention.py:33-44) with K and V handed over as the
 * attention kernel's operand planes instead of fp32 rows (round 5).  dpm_linear_bf16x3_kvplanes is dpm_linear_bf16x3 for a
 * q | k | v projection over sequences of `tokens` rows: columns [0, kv_col0) go to `out` as fp32 rows (Q), columns [kv_col0, Cout) =
 * K (heads x 32) then V (heads x 32) go to kv_planes as one 24 576-byte image per (sequence = row / tokens, head, 64-key tile):
 * the three bf16 planes of the K tile in the swizzled rows the score product reads, then the three planes of the V tile
 * transposed in the order the P V product reads -- exactly what the attention kernel's own staging makes of the fp32 rows, so
 * dpm_attention_planes returns dpm_attention_shifted / _indexed's result bit for bit while each K / V element is split once
 * instead of once per 64-query block that reads it.  kv_planes: dpm_attention_planes_bytes(sequences, tokens, heads) bytes,
 * 16-byte aligned.  Needs tokens % 64 == 0, R % tokens == 0, kv_col0 % 64 == 0, Cout - kv_col0 == 64 * heads, 16-byte aligned
 * x / bias / out with ldx % 4 == 0; DPM_EUNSUPPORTED otherwise (callers then run dpm_linear_bf16x3 + dpm_attention_*).
 * dpm_attention_planes: head_dim 32, N % 64 == 0, no key mask; seq_index as in dpm_attention_indexed or NULL. */
size_t dpm_attention_planes_bytes(int n_sequences, int N, int heads);
int dpm_linear_bf16x3_kvplanes(const float *x, int ldx, const void *w_planes, int ldw, long long plane_stride,
                               const float *bias, float *out, int ldo, int R, int Cin, int Cout, int kv_col0, int tokens,
                               int heads, void *kv_planes, dpm_stream_t stream);
int dpm_attention_planes(const float *Q, int ldq, long long sq, const void *kv_planes, float *out, int ldo, long long so,
                         int B, int M, int N, int heads, int kv_shift, const int32_t *seq_index, dpm_stream_t stream);

/* The same contraction as dpm_linear (Conv1d(k=1) / nn.Linear: network/encoder/utils.py:358-389, the decoder's projections
 * and heads) on the bf16 matrix pipe with every fp32 operand split exactly into three bf16 terms and six of the nine term
 * products accumulated in fp32 (the three dropped ones are below 2^-23 of the product): fp32-accumulation accuracy at 3/8 of
 * the matrix-pipe time of the exact-fp32 instruction (csrc/gemm_b3.hip).  dpm_split_bf16x3 makes the weight planes once per
 * weight version: planes = 3 x n bf16 (hi | mid | lo), plane p of element i at planes[p * n + i].  dpm_linear_bf16x3 takes a row
 * block of such planes: w_planes -> plane 0 of the first weight row, rows ldw elements apart, planes plane_stride elements
 * apart.  DPM_EUNSUPPORTED for Cin % 32 != 0, Cout % 4 != 0 or unaligned bias / residual / output (x may have any row stride);
 * a caller that falls back to dpm_linear then must do so for EVERY call of that layer (the two kernels differ in the last bits). */
int dpm_split_bf16x3(const float *W, long long n, void *planes, dpm_stream_t stream);
int dpm_linear_bf16x3(const float *x, int ldx, const void *w_planes, int ldw, long long plane_stride, const float *bias,
                      const float *residual, int ldr, float *out, int ldo, int R, int Cin, int Cout, int act,
                      dpm_stream_t stream);
/* dpm_linear_bf16x3 plus a rank-3 term added in fp32 in the epilogue, before residual and activation:
 * out[r, c] += scale * (x3[r, 0:3] . w3[c, 0:3]), x3 (R,3) packed, w3 rows ldw3 floats apart.  It is the POINT half of a grouping
 * layer's relative-coordinate columns (network/encoder/pointnext.py:52-56: W [fea ; (p - c) / r] = W_f fea + W_r p / r - W_r c / r),
 * with x3 = the points' coordinates, w3 = W_r, scale = 1 / r; dpm_group_gather_ln_max_folded subtracts the centre half. */
int dpm_linear_bf16x3_rank3(const float *x, int ldx, const void *w_planes, int ldw, long long plane_stride, const float *bias,
                            const float *residual, int ldr, float *out, int ldo, int R, int Cin, int Cout, int act,
                            const float *x3, const float *w3, int ldw3, double scale, dpm_stream_t stream);
/* dpm_linear_layernorm (Conv1d(k=1) / Linear + LayerNorm1d, network/encoder/utils.py:358-413, descriptor_attention.py:36-48)
 * on the bf16x3 product, weights as planes of dpm_split_bf16x3; rows identical to dpm_linear_bf16x3 followed by dpm_layernorm.
 * DPM_EUNSUPPORTED for Cout outside {32, 64, 128, 256}, Cin % 32 != 0 or unaligned operands. */
int dpm_linear_layernorm_bf16x3(const float *x, int ldx, const void *w_planes, int ldw, long long plane_stride,
                                const float *bias, const float *pre, const float *gamma, const float *beta, const float *post,
                                float *out, int ldo, int R, int Cin, int Cout, int act, dpm_stream_t stream);

/* The tail of a decoder block (descriptor_attention.py:41-48: cross attention's out-projection + residual + norm2, then the MLP +
 * residual + norm3) as ONE kernel for C = 256: out = LN3(relu(z2 W0^T + b0) W2^T + b2 + z2) [+ post] with
 * z2 = LN2(a Wo^T + bo + pre).  a, pre, post (may be NULL), out packed (R, C) fp32; out must not be a (it may be pre's storage);
 * the weights (C, C) packed as bf16x3 planes of dpm_split_bf16x3 (plane p of element i at planes[p * plane_stride + i]); the
 * biases may be NULL.  Rows identical, bit for bit, to dpm_linear_layernorm_bf16x3 (pre), dpm_linear_bf16x3 (ReLU),
 * dpm_linear_layernorm_bf16x3 (pre = z2, post).  DPM_EUNSUPPORTED for C != 256 or operands that are not 16-byte aligned. */
int dpm_decoder_tail_bf16x3(const float *a, const float *pre, const float *post, float *out, int R, int C, const void *wo_planes,
                            long long plane_stride_o, const float *bo, const float *gamma2, const float *beta2,
                            const void *w0_planes, long long plane_stride_0, const float *b0, const void *w2_planes,
                            long long plane_stride_2, const float *b2, const float *gamma3, const float *beta3,
                            dpm_stream_t stream);

/* InvResMLP's point-wise pair (network/encoder/pointnext.py:118-138: pw_conv = Conv1d(C, 4C, 1) -> LayerNorm1d -> ReLU ->
 * Conv1d(4C, C, 1) -> LayerNorm1d, then the residual and ReLU) as ONE kernel for C = 32, H = 4C = 128 (the first level, whose
 * 4C-wide intermediate is otherwise written to and read back from HBM): out = relu(LN2(relu(LN1(x W1^T + b1)) W2^T + b2) + post).
 * x (R,32) rows ldx floats apart; post / out packed (R,32); W1 (128,32) and W2 (32,128) as bf16x3 planes of dpm_split_bf16x3
 * (plane p of element i at planes[p * plane_stride + i]), W2's COLUMNS permuted before the split: stored column 32 s + 8 g + e
 * holds original column 16 (2 s + (e >> 2)) + 4 g + (e & 3), s < 4, g < 4, e < 8 (the order in which the kernel's accumulator
 * registers hold the intermediate).  Same bf16x3 arithmetic as dpm_linear_layernorm_bf16x3 twice; the row statistics are summed
 * in another association (results agree to rounding).  DPM_EUNSUPPORTED for other widths or unaligned operands. */
int dpm_pwconv_pair_bf16x3(const float *x, int ldx, const void *w1_planes, long long plane_stride1, const float *b1,
                           const float *gamma1, const float *beta1, const void *w2_planes_kperm, long long plane_stride2,
                           const float *b2, const float *gamma2, const float *beta2, const float *post, float *out, int R,
                           int C, int H, dpm_stream_t stream);

/* F.normalize(x, p=2, dim=-1) (decoder.py:185): x / max(||x||, 1e-12), rows (R,C). */
int dpm_l2_normalize(const float *x, int R, int C, float *out, dpm_stream_t stream);

/* Decoder._descriptor_pairing from the L2-normalised head outputs on (decoder.py:185-191) as ONE operator: a (batch,M,C),
 * b (batch,N,C) row-major -> S = a b^T (fp32 MFMA), P = softmax_row(S/tau) * softmax_col(S/tau), the k largest entries of
 * the flattened P sorted descending (ties: smaller flat index first): out_val (batch,k), out_idx (batch,k) with
 * row = idx / N, col = idx % N.  The M x N matrix never exists in memory: two launches over row strips of 64, the strip
 * recomputed in the second (csrc/match.hip).  DPM_EUNSUPPORTED for N > 256, k > 2048, C % 32 != 0 or unaligned operands:
 * the caller then runs dpm_linear_batched + dpm_dual_softmax_topk (same values up to the last bit of the column sums). */
size_t dpm_match_workspace_bytes(int batch, int M, int N, int k);
int dpm_match_topk(const float *a, const float *b, int batch, int M, int N, int C, double tau, int k, float *out_val,
                   int32_t *out_idx, void *workspace, dpm_stream_t stream);

/* Decoder._descriptor_pairing tail (decoder.py:186-191): S (M,N) similarity, overwritten with
 * P = softmax_row(S/tau) * softmax_col(S/tau); then the k largest entries of the flattened P,
 * sorted descending: out_val (k), out_idx (k) flat indices (row = idx / N, col = idx % N).
 * `batch` independent (M,N) problems are laid out back to back (S (batch,M,N), outputs (batch,k)). */
size_t dpm_pairing_workspace_bytes(int batch, int M, int N);
int dpm_dual_softmax_topk(float *S, int batch, int M, int N, double tau, int k, float *out_val,
                          int32_t *out_idx, void *workspace, dpm_stream_t stream);

/* Decoder._get_corres_sets input assembly (decoder.py:204-205): for the k flat indices,
 * X[0:k] = [x[src] | y[dst]], X[k:2k] = [y[dst] | x[src]] (rows of 2E), and the decoded
 * src_idx/dst_idx (k). x (batch,M,E), y (batch,N,E), X (batch,2k,2E). */
int dpm_gather_pairs(const float *x, const float *y, const int32_t *flat_idx, int batch, int k, int M,
                     int N, int E, float *X, int32_t *src_idx, int32_t *dst_idx, dpm_stream_t stream);

/* torch.mean over the points of each batch element (OverlapHead, heads.py:64-65):
 * x (B,R,C) -> out[b, 0:C] with row stride ldo. */
int dpm_mean_rows(const float *x, int B, int R, int C, float *out, int ldo, dpm_stream_t stream);

/* Decoder._get_corres_sets + _solve_transformation_SVD (decoder.py:208-265): offsets (2k,3)
 * [first k: src->dst, next k: dst->src], keypoint coordinates, pair indices and confidences ->
 * result[0:9] R row-major, [9:12] T, [12] rmse, [13] #correspondences, [14] #inliers,
 * [15] iterations, [16] mean of the first 30 inlier confidences (simvec_to_num,
 * system/modules/utils.py:18), [17:20] reserved, [20:20+#inliers] inlier confidences in
 * correspondence order.  result holds 20 + 2k floats; `header` (NULL-able) receives a copy of
 * result[0:20].  R = V U^T of the fp64 SVD, no reflection fix.
 * offsets == NULL: src_xyz/dst_xyz/conf are taken as k ready-made correspondences (rows) and
 * only _solve_transformation_SVD runs.  `batch` independent pairs: offsets (batch,2k,3), indices
 * and conf (batch,k), coordinates at src_xyz + b*stride_src, result (batch, 20+2k), header rows
 * header_stride floats apart.  Limit: the 2k weights and the torch.topk replay scratch live in LDS (24 B per pair next to
 * the kernel's static arrays, together at most the CU's 160 KB: k up to about 6000 on gfx950); beyond that
 * DPM_EUNSUPPORTED. */
size_t dpm_kabsch_workspace_bytes(int batch, int k);
int dpm_corr_kabsch(const float *offsets, const float *src_xyz, int ld_src, long long stride_src,
                    const float *dst_xyz, int ld_dst, long long stride_dst, const int32_t *src_idx,
                    const int32_t *dst_idx, const float *conf, int batch, int k, double eps_offset,
                    int num_iter, double std_ratio, void *workspace, float *result, float *header,
                    int header_stride, dpm_stream_t stream);

/* ---------------------------------------------------------------- scan pre-processing ---- */

/* VoxelSample(voxel_size, 'first') -> DistanceSample(min_dis, max_dis) -> CoordinatesNormalization(ratio)
 * (dataloader/transforms.py:322-356,387-397,400-407): xyz = N raw points, `stride` floats apart (3 for packed
 * xyz, 4 for KITTI .bin records).  Output: the kept points in ascending voxel-id order, divided by ratio
 * (out_xyz (out_capacity,3)), their original indices (out_idx, NULL-able), status[0] = number kept,
 * status[1] = 1 if the voxel grid (X*Y*Z cells) exceeded max_cells (nothing is written then).
 * workspace: dpm_preprocess_workspace_bytes(max_cells). */
size_t dpm_preprocess_workspace_bytes(long long max_cells);
int dpm_preprocess_scan(const float *xyz, int N, int stride, double voxel_size, double min_dis, double max_dis,
                        double ratio, long long max_cells, float *out_xyz, int32_t *out_idx, int out_capacity,
                        int32_t *status, void *workspace, dpm_stream_t stream);

/* Building blocks of OutlierFilter / LowPassFilter (dataloader/transforms.py:230-289), which the reference runs
 * through pytorch3d.knn_points and open3d.estimate_normals between DistanceSample and CoordinatesNormalization:
 *
 * dpm_knn_self: exact K nearest OTHER points of every point of one cloud xyz (N,3) (== knn_points(p, p, K+1)
 *   with column 0 dropped; rows ordered by (distance, index); direct-form squared distances).  Any of idx (N,K),
 *   dist2 (N,K), mean_dist (N) [mean over the K columns of sqrt(dist2), transforms.py:240-241] may be NULL.
 *   `cell` = edge of the search grid in the units of xyz (a few times the typical neighbour spacing).
 * dpm_point_normals: unit normal of every point = eigenvector of the smallest eigenvalue of the covariance of
 *   the points within `radius` (itself included), (0,0,1) when fewer than 3 are in range (transforms.py:268-271).
 * dpm_lowpass_similarity: sim[i] = sum of the `flux` largest |n_i . n_j| over the K neighbours idx[i,:]
 *   (transforms.py:279-281).
 * dpm_stat_filter: mean / unbiased std of stat (N); mode 0 keeps stat <= mean + k_std*std (OutlierFilter,
 *   transforms.py:242-246), mode 1 keeps stat > mean - k_std*std (LowPassFilter, transforms.py:282); survivors
 *   are compacted in order into xyz_out (coordinates divided by `ratio`: CoordinatesNormalization folded into the
 *   last filter, 1.0 = untouched) / idx_out (idx_in NULL: positions), their number into n_out[0].
 * workspace for the first two: dpm_knn_self_workspace_bytes(N). */
size_t dpm_knn_self_workspace_bytes(int N);
int dpm_knn_self(const float *xyz, int N, int K, double cell, int32_t *idx, float *dist2, float *mean_dist,
                 void *workspace, dpm_stream_t stream);
int dpm_point_normals(const float *xyz, int N, double radius, float *normals, void *workspace, dpm_stream_t stream);
int dpm_lowpass_similarity(const float *normals, const int32_t *idx, int N, int K, int flux, float *sim,
                           dpm_stream_t stream);
int dpm_stat_filter(const float *stat, int N, double k_std, int mode, double ratio, const float *xyz_in,
                    const int32_t *idx_in, float *xyz_out, int32_t *idx_out, int32_t *n_out, dpm_stream_t stream);

/* The two filters whole, with the frame's length in DEVICE memory (the rule of the training transforms below): xyz
 * (capacity,3) fp32, idx (capacity,) int32 [original indices, NULL-able: positions], count (1,) int32.  The length is
 * count[0] clamped to [0, capacity]; every launch is sized by the capacity, rows at and past the count are never read, and
 * the host never waits.  Survivors land in input order below count_out[0] in xyz_out (capacity,3) [divided by `ratio`, a
 * true division: CoordinatesNormalization folded in, 1.0 = untouched] and idx_out (capacity,) [NULL-able].  Outputs must not
 * alias inputs.  Same kernels, same arithmetic and, on xyz[:count], the same bytes as the building blocks above; two runs
 * give identical bytes.  A frame of at most K points (K = nb_neighbors / normals_num; 0 and 1 included) passes through:
 * its live rows in order, count_out = count.  `cell` = edge of the neighbour-search grid, as in dpm_knn_self.
 *
 * dpm_outlier_filter_dc: OutlierFilter (transforms.py:230-246, pytorch3d branch): mean distance to the nb_neighbors
 *   nearest other points, keep stat <= mean + std_ratio * std.
 * dpm_lowpass_filter_dc: LowPassFilter (transforms.py:256-289, max_remain off): normals within normals_radius, the
 *   normals_num nearest other points, the sum of the `flux` largest |n_i . n_j|, keep stat > mean - filter_std * std.
 * Checked before anything is queued: DPM_EINVAL for capacity < 0, K < 1, flux < 1 or flux > K; DPM_EUNSUPPORTED for
 * K + 1 > 64 or flux > 8; capacity 0 returns DPM_OK at once.  workspace: dpm_filter_dc_workspace_bytes(capacity, K)
 * (the search grid, the sorted points, the statistic, the normals and the neighbour indices of one frame). */
size_t dpm_filter_dc_workspace_bytes(int capacity, int K);
int dpm_outlier_filter_dc(const float *xyz, const int32_t *idx_in, const int32_t *count, int capacity, int nb_neighbors,
                          double std_ratio, double cell, double ratio, float *xyz_out, int32_t *idx_out,
                          int32_t *count_out, void *workspace, dpm_stream_t stream);
int dpm_lowpass_filter_dc(const float *xyz, const int32_t *idx_in, const int32_t *count, int capacity,
                          double normals_radius, int normals_num, double filter_std, int flux, double cell, double ratio,
                          float *xyz_out, int32_t *idx_out, int32_t *count_out, void *workspace, dpm_stream_t stream);

/* ---------------------------------------------------------------- training transforms --- */

/* The transforms only training configs use (dataloader/transforms.py).  ONE RULE: a frame is a fixed-capacity buffer
 * plus a count in DEVICE memory -- xyz (capacity,3) fp32, idx (capacity,) int32 [original indices, NULL-able: positions],
 * count (1,) int32.  Every entry reads the count through its pointer, sizes its grid by the capacity and writes the new
 * count to device memory; rows at and past the count are never read.  Selections are stable, ordered compactions; outputs
 * must not alias inputs.  Two runs give identical bytes.  workspace: dpm_augment_workspace_bytes(capacity, cells) with
 * cells = img_len*img_width (ground filter), max_cells (voxel select) or 0 (mask select).
 *
 * dpm_ground_filter: GroundFilter (transforms.py:174-227).  Cell = int32(x / grid_width + img_len / 2) in float32,
 *   truncated towards zero (so (-1, 0) lands in row 0 and is kept; columns alike); points outside the image and cells
 *   with fewer than 3 points are dropped; a cell with zmax - zmin > ground_height (float32) keeps all its points,
 *   any other cell keeps one representative when preserve_sparse_ground.  ground_height <= 0 is the identity.
 *   ORDER AND REPRESENTATIVE ARE DEFINED HERE, not by the reference, whose unstable np.argsort over cell ids leaves the
 *   in-cell order -- and with it the representative -- to the numpy build: kept points come in ascending input position,
 *   and a sparse cell's representative is its point with the lowest input position.  The SETS (non-ground points, sparse
 *   cells) equal the reference's.
 * dpm_voxel_select: VoxelSample (transforms.py:322-356), retention 0 = 'first' (the bytes of dpm_preprocess_scan with
 *   the crop and the normalisation off), 1 = 'center' (per voxel the point nearest the voxel centre, distance in fp64
 *   as the reference's int32 * python float promotes, equal distances to the lower position).  Output in ascending
 *   voxel id.  status[0] = number kept (usable as the new count), status[1] = 1 when the grid exceeded max_cells
 *   (nothing kept then).  An empty frame stays empty.
 * dpm_mask_select: keep = distance crop (DistanceSample, transforms.py:387-397; use_distance) AND u[i] >= drop_ratio in
 *   float32 (RandomDrop, transforms.py:429-434; u NULL = off, u has `capacity` entries) AND outside every occlusion wedge
 *   (RandomShield, transforms.py:447-474): wedges = n_wedges x (start, end, wraps, dis_threshold) floats in HOST memory,
 *   at most 16; azimuth = atan2(y, x) * 180 / pi and distance = |xyz| in float32; a point goes when start <= azimuth <= end
 *   (wraps: azimuth >= start OR azimuth <= end, end already reduced by 360) AND distance >= dis_threshold.
 * dpm_points_affine: in place on the first count rows.  mode 0: R x + T, params = R row-major (9) then T (3)
 *   (RandomRT, transforms.py:529); mode 1: x += jitter (capacity,3) (RandomPosJitter, transforms.py:561-563); mode 2:
 *   x / params[0], a true division (CoordinatesNormalization, transforms.py:406); mode 3: VerticalCorrect
 *   (transforms.py:300-319), params = (sin, cos) of the angle: per point the rotation about normalize(x cross z) built in
 *   fp64 and rounded to float32 before it multiplies the point.  A point on the z axis becomes NaN, as in the reference.
 * dpm_gather_points: out[j] = in[sel[j]] (RandomShuffle, RandomSample, FarthestPointSample: transforms.py:359-384,
 *   410-420).  limit < 0: all min(count, n_sel) rows; limit >= 0: a frame of at most `limit` points is copied unchanged,
 *   a longer one keeps min(limit, n_sel) rows.  A selector outside [0, count) gives a zero row with index -1.
 * dpm_pack_frames: ToTensor(padding_to) + map_collate_fn (transforms.py:69-98, body.py:155-161) for S frames given as
 *   HOST arrays of device pointers: points (S,3,padding_to) channel-first with zero fill, padding (S,padding_to) bytes
 *   (1 past a frame's count), status (S,2) = (count, 1 when count > padding_to; that frame's rows are zero). */
size_t dpm_augment_workspace_bytes(int capacity, long long cells);
int dpm_ground_filter(const float *xyz, const int32_t *idx_in, const int32_t *count, int capacity, int img_len,
                      int img_width, double grid_width, double ground_height, int preserve_sparse_ground, float *out_xyz,
                      int32_t *out_idx, int32_t *out_count, void *workspace, dpm_stream_t stream);
int dpm_voxel_select(const float *xyz, const int32_t *idx_in, const int32_t *count, int capacity, double voxel_size,
                     int retention, long long max_cells, float *out_xyz, int32_t *out_idx, int32_t *status,
                     void *workspace, dpm_stream_t stream);
int dpm_mask_select(const float *xyz, const int32_t *idx_in, const int32_t *count, int capacity, int use_distance,
                    double min_dis, double max_dis, const float *u, double drop_ratio, const float *wedges, int n_wedges,
                    float *out_xyz, int32_t *out_idx, int32_t *out_count, void *workspace, dpm_stream_t stream);
int dpm_points_affine(float *xyz, const int32_t *count, int capacity, int mode, const double *params,
                      const float *jitter, dpm_stream_t stream);
int dpm_gather_points(const float *xyz, const int32_t *idx_in, const int32_t *count, int capacity, const int32_t *sel,
                      int n_sel, int limit, float *out_xyz, int32_t *out_idx, int32_t *out_count, dpm_stream_t stream);
/* Deskew (csrc/deskew.hip; no counterpart in the reference, which assumes compensated scans): in place on the first count
 * rows, one launch, no host synchronisation.  motion: 16 doubles in HOST memory, D = P0^-1 P1 row-major, the sensor's pose
 * at the end of the sweep in its frame at the start; the sensor is at D(s) = (Exp(s Log R_D), s t_D) at sweep fraction s.
 * A row measured at fraction s becomes D(s_ref)^-1 D(s) p, 0 <= s_ref <= 1.  Where s comes from, time_mode:
 *   0  the column of the row's ray: s = (idx[i] mod azimuth_steps) / azimuth_steps, azimuth_steps >= 1;
 *   1  the row's own azimuth: s = frac(atan2f(y, x) / 2 pi); with azimuth_steps > 0 rounded to the nearest column
 *      (column azimuth_steps is column 0), with 0 continuous.  Raw frames only: any transform that turns the points first
 *      makes it meaningless; idx may be NULL;
 *   2  times[idx[i]], n_times fp32 fractions by ORIGINAL row; a row whose index lies outside [0, n_times) stays as it is.
 * The axis, the angle, t_D and D(s_ref)^-1 are derived in float64 on the host; the kernel works in float32.  An identity
 * motion (bit-equal to the identity matrix) launches nothing: the rows keep their bytes. */
int dpm_points_deskew(float *xyz, const int32_t *idx, const int32_t *count, int capacity, int time_mode, const float *times,
                      int n_times, int azimuth_steps, const double *motion, double s_ref, dpm_stream_t stream);
int dpm_pack_frames(const float *const *xyz, const int32_t *const *counts, const int32_t *capacities, int S,
                    int padding_to, float *points, unsigned char *padding, int32_t *status, dpm_stream_t stream);

/* ---------------------------------------------------------------- frame ingest ---------- */

/* The device side of "F scan files arrive": what dataloader/heads/bin.py:16-17 (drop a record when one of its first
 * three floats is NaN) and dataloader/transforms.py's PointCloud.__init__ (the frame's buffers) do per frame, for a whole
 * batch in ONE asynchronous copy and THREE launches whatever F is, without a host synchronisation.
 * staging_host: a (pinned) block of staging_bytes bytes, as 32-bit words: a header of F x 4 int64 = (offset of the
 * frame's first record in words from the start of the block, rows, stride in floats >= 3, drop_nan 0 / 1), then the
 * records.  staging_dev: device memory of the same size, the target of the copy; the caller keeps both untouched until
 * the stream has passed this call.  Outputs, frames of the layout of the training transforms: xyz (F,capacity,3) = the
 * kept records' first three floats in input order, moved AS BITS (NaN payloads, -0.0, denormals survive), rows at and
 * past the count zero; idx (F,capacity) = 0..capacity-1; count (F,) = kept records.  Each frame equals
 * PointCloud(filtered array, capacity) byte for byte; no atomics, two runs give identical bytes.
 * Every header field is checked on the host before anything is queued: rows > capacity, a stride below 3, records
 * outside the block are DPM_EINVAL.  chunk must be the kernels' compaction chunk (4096): the caller sizes
 * workspace = F * ceil(capacity / chunk) int32 with it. */
int dpm_ingest_frames(const void *staging_host, void *staging_dev, long long staging_bytes, int F, int capacity,
                      int chunk, float *xyz, int32_t *idx, int32_t *count, void *workspace, dpm_stream_t stream);

/* ---------------------------------------------------------------- map tiles ------------- */

/* PoseGraph.__global_mapping + centring of global_map_query_graph (system/modules/pose_graph.py:373-409,
 * 504-510): key_points (n_scans,C,S) device-resident unified descriptors (last three rows xyz in metres),
 * select (K) scan indices in tile order (NULL: 0..K-1), poses (n_scans,12) [R row-major, T] = SE3_pred,
 * centering (12) -> out (C, K*S): features copied, xyz -> R_c^T ((R_k x + t_k) - t_c). */
int dpm_map_tile(const float *key_points, const int32_t *select, const float *poses, const float *centering,
                 int C, int S, int K, float *out, dpm_stream_t stream);

/* ---------------------------------------------------------------- registration edge ---- */

/* calculate_information_matrix_from_pcd (system/modules/utils.py:60-113), pytorch3d branch:
 * pcd1 (3,N1), pcd2 (3,N2) channel-first metres; Rt = 12 floats (R row-major, then T);
 * out6x6 = sum over source points whose transformed nearest target lies within `radius` of the
 * G^T G of that target point.  Exact nearest neighbours via a uniform grid. */
size_t dpm_infomat_workspace_bytes(int n_pairs, int N1, int N2);
/* Rt may point into a dpm_corr_kabsch result (its first 12 floats are R row-major, T). */
int dpm_information_matrix(const float *pcd1, int N1, const float *pcd2, int N2, const float *Rt,
                           double radius, float *out6x6, void *workspace, dpm_stream_t stream);
/* n_pairs edges in one pass: pcd (F,3,N) scans in metres, pair p = (src_frame[p], dst_frame[p]);
 * pose p at Rt + p*rt_stride (12 floats), output p at out + p*out_stride (36 floats). */
int dpm_information_matrix_batched(const float *pcd, int N, const int32_t *src_frame,
                                   const int32_t *dst_frame, int n_pairs, const float *Rt, int rt_stride,
                                   double radius, float *out, int out_stride, void *workspace,
                                   dpm_stream_t stream);
/* The same computation in two calls sharing one workspace (dpm_infomat_workspace_bytes(n_pairs, N, N)):
 * the target grids depend only on the scans, so a caller that pipelines frames builds them before the
 * poses exist (next to the encoder) and runs only the search after the registration
 * (system/modules/odometry.py:116-118 calls the function right after registration_forward). */
int dpm_infomat_build_grids(const float *pcd, int N, const int32_t *dst_frame, int n_pairs, double radius,
                            void *workspace, dpm_stream_t stream);
int dpm_infomat_search_grids(const float *pcd, int N, const int32_t *src_frame, const int32_t *dst_frame,
                             int n_pairs, const float *Rt, int rt_stride, double radius, float *out,
                             int out_stride, void *workspace, dpm_stream_t stream);

/* ---------------------------------------------------------------- refined poses --------- */

/* Batched ICP.  Stands in for the offline third-party ICP that produced the per-scene refined_SE3.pkl the reference's
 * training step reads (pipeline/modules/model_pipeline.py:199-282, dataloader/body.py:142-146); nothing in the reference
 * writes that file.  pcd (F,3,N) fp32 channel-first scans in metres, lengths (F) valid leading points per frame; pair p
 * registers frame src_frame[p] onto frame dst_frame[p] starting from init_pose + 16*p (4x4 row-major fp64, the pose of
 * the source in the target).  metric DPM_ICP_POINT: residual R p + t - q; DPM_ICP_PLANE: n . (R p + t - q) with the
 * target normals `normals` (F,N,3) fp32 (dpm_point_normals of each target frame; NULL for the point metric).  q is the
 * exact nearest target point within the stage's max_dist (ties to the smaller index).  The schedule -- stage_max_dist /
 * stage_max_iter, n_stages <= 16 entries in HOST memory -- runs back to back on grids built once; every stage restarts
 * all pairs from where they stand.  A pair stops when its rotation step < tol_rot (rad) and its translation step <
 * tol_trans (m).  Outputs per pair: pose (16 fp64; must not alias init_pose), fitness = matches / source points and rmse
 * of the matches at the last evaluated pose, iterations (steps taken, summed over the stages), status of the last stage.
 * A system that cannot be solved (no match; fewer than six matches, a Cholesky pivot below 1e-9 of its block's largest
 * diagonal entry, a non-finite sum) leaves the pose at its last good value: no NaN or Inf is ever written to it.
 * debug_match (P,N) int32 / debug_system (P,29) fp64, both NULL-able: the matched original target index of every source
 * point (-1: none) and the summed system [H upper triangle row-major (21), g (6), matches, squared residuals] of the last
 * search that ran.  Two launches per iteration, no host synchronisation, capturable in a HIP graph; the same call twice
 * gives identical bytes, and a pair's bytes do not depend on the other pairs of the call.
 * workspace: dpm_icp_workspace_bytes(n_pairs, N). */
#define DPM_ICP_POINT 0
#define DPM_ICP_PLANE 1
#define DPM_ICP_CONVERGED 0
#define DPM_ICP_MAX_ITER 1
#define DPM_ICP_NO_MATCH 2
#define DPM_ICP_SINGULAR 3
size_t dpm_icp_workspace_bytes(int n_pairs, int N);
int dpm_icp_refine_batched(const float *pcd, int F, int N, const int32_t *lengths, const float *normals,
                           const int32_t *src_frame, const int32_t *dst_frame, int n_pairs, const double *init_pose,
                           int metric, const double *stage_max_dist, const int32_t *stage_max_iter, int n_stages,
                           double tol_rot, double tol_trans, double *pose, float *fitness, float *rmse,
                           int32_t *iterations, int32_t *status, int32_t *debug_match, double *debug_system,
                           void *workspace, dpm_stream_t stream);

/* ---------------------------------------------------------------- global map ------------ */

/* ResultLogger.draw_trajectory's point-cloud map (system/modules/recoder.py:167-190): every scan's cloud moved by its
 * SE3_pred, concatenated, open3d voxel_down_sample(vs).  Here: the voxel-centroid map of the union, computed in HBM
 * with integer atomics (bit-reproducible, independent of arrival order), output in order of first appearance.
 * A batch of scans: clouds (n_scans) device pointers to (3,N_i) fp32 channel-first clouds, offsets (n_scans+1) int64
 * prefix sums of N_i (offsets[0] = 0, n_batch = offsets[n_scans]), poses (n_scans,12) [R row-major, T] fp32; the
 * three arrays are device memory.  Batches may be fed one after another (base = global index of the batch's first
 * point), so host-resident clouds can be streamed through a bounded staging buffer.  Sequence, per map of n_points:
 *   init -> bounds (every batch) -> [caller reads the 256-byte workspace header: unsigned min[3], max[3]
 *   (order-preserving images of fp32), non-finite coordinate count; computes min_b = min - vs/2 in fp64 and checks
 *   that the extent fits 3 x 21 bits] -> insert (every batch, same order) -> finish -> [header word 8 = M voxels,
 *   word 7 = keys out of range (must be 0), 64-bit words at byte 64/72 = runs flushed / CAS attempts] -> emit:
 *   centroids (3,M) fp32, counts (M) int32.
 * Limits: n_points < 2^31 and n_points * (vs * 2^32 + 2) < 2^62 (the 64-bit fixed-point sums cannot wrap).
 * workspace: dpm_voxel_map_workspace_bytes(n_points) <= 51 bytes per point + 8 KB. */
size_t dpm_voxel_map_workspace_bytes(long long n_points);
int dpm_voxel_map_init(long long n_points, void *workspace, dpm_stream_t stream);
int dpm_voxel_map_bounds(const float *const *clouds, const long long *offsets, const float *poses, int n_scans,
                         long long n_batch, void *workspace, dpm_stream_t stream);
int dpm_voxel_map_insert(const float *const *clouds, const long long *offsets, const float *poses, int n_scans,
                         long long n_batch, long long base, long long n_points, double min_x, double min_y,
                         double min_z, double voxel_size, void *workspace, dpm_stream_t stream);
int dpm_voxel_map_finish(long long n_points, void *workspace, dpm_stream_t stream);
int dpm_voxel_map_emit(const void *workspace, long long n_points, double min_x, double min_y, double min_z,
                       double voxel_size, float *centroids, int32_t *counts, int M, dpm_stream_t stream);

/* RegistrationLoss of the reference (network/loss.py) for training, without any (B,M,N) tensor (csrc/reg_loss.hip).
 * Side a = src (M points), side b = dst (N points); coordinates (B,3,M) / (B,3,N), features (B,C,M) / (B,C,N) fp32
 * contiguous, padding (B,M) / (B,N) bytes, nonzero on padding.
 * pairs (make_pairs): nn_a[b,i] = first j minimising dist2 = (dx dx + dy dy) + dz dz (fp32, that order, no contraction) when
 *   that minimum is <= (float)(eps * eps), else -1; nn_b the same from the b side.  neutral_a / neutral_b (may be NULL): per row
 *   the number of entries with dist2 <= eps^2 other than the neighbour (the row sum of the reference's neutral mask).
 * forward (pairing_loss of both directions, one feature pair): z = a^ b^T / tau with x^ = x / max(||x||, 1e-12); a row
 *   counts when it is not padding and nn >= 0; its term is logsumexp_j z_ij - z_i,nn(i), the softmax over every column
 *   (padding included) except, when `neutral` is set, the entries with dist2 <= eps^2 other than nn(i).  *loss = (mean_a +
 *   mean_b) / 2, a direction without counted rows contributing 0; stats (8 floats): [loss, mean_a, mean_b, n_a, n_b, hits_a,
 *   hits_b, 0], hits = counted rows whose argmax_j of the raw similarity (first on ties) is nn (neutral == 0 only).
 *   argmax_a / argmax_b (B,M) / (B,N) (may be NULL; neutral == 0 only) receive those argmaxes.  workspace:
 *   dpm_reg_loss_workspace_bytes(B,M,N,C); it holds what the backward reads and must stay intact until then.
 * backward: grad_a (B,C,M), grad_b (B,C,N) of *grad_loss (device scalar) x loss, from the forward's workspace and stats.
 * C in {64, 128, 192, 256}, else DPM_EUNSUPPORTED.  Deterministic (no float atomics). */
int dpm_reg_loss_pairs(const float *xyz_a, const float *xyz_b, int B, int M, int N, double eps, int32_t *nn_a, int32_t *nn_b,
                       int32_t *neutral_a, int32_t *neutral_b, dpm_stream_t stream);
size_t dpm_reg_loss_workspace_bytes(int B, int M, int N, int C);
int dpm_reg_loss_forward(const float *fea_a, const float *fea_b, const float *xyz_a, const float *xyz_b, const uint8_t *pad_a,
                         const uint8_t *pad_b, const int32_t *nn_a, const int32_t *nn_b, int B, int M, int N, int C, double tau,
                         double eps, int neutral, int32_t *argmax_a, int32_t *argmax_b, float *loss, float *stats,
                         void *workspace, dpm_stream_t stream);
int dpm_reg_loss_backward(const float *xyz_a, const float *xyz_b, const int32_t *nn_a, const int32_t *nn_b, int B, int M, int N,
                          int C, double tau, double eps, int neutral, const float *grad_loss, const float *stats,
                          const void *workspace, float *grad_a, float *grad_b, dpm_stream_t stream);

/* Attention for training (csrc/attention_train.hip): the scaled-dot-product core of nn.MultiheadAttention
 * (descriptor_attention.py:14-15, 33-44: softmax(Q_h K_h^T / sqrt(d)) V_h per head, dropout 0, key_padding_mask) with a
 * backward, replacing autograd over the (B, heads, M, N) probability tensor.  Operands as in dpm_attention_masked: Q (B*M, E),
 * K / V (B*N, E) row views with leading dims ld* and batch strides s* (floats; pointers 16-byte aligned, ld* and s* multiples
 * of 4), key_mask (B,N) bytes, non-zero = padding key, NULL = none.  head_dim 32 only (else DPM_EUNSUPPORTED).
 * forward: out (row view like Q) and lse (B, heads, M): log sum_n exp(score[m, n]) over the unmasked keys of each score row.
 * backward: from Q, K, V, out, lse and dout (row view) -> dQ (B*M, E), dK, dV (B*N, E) contiguous; strips of the score matrix
 *   are recomputed (P = exp(S - lse), dV = P^T dOut, dP = dOut V^T, dS = P (dP - rowsum(dOut out)) / sqrt(d), dQ = dS K,
 *   dK = dS^T Q); masked keys get dK = dV = 0 exactly.  workspace: dpm_attention_train_workspace_bytes(B, M, N, heads).
 * All products in fp32 on the matrix cores; no floating-point atomics: two runs give identical bytes.  A sequence whose keys
 * are all padding yields NaN (as the reference). */
size_t dpm_attention_train_workspace_bytes(int B, int M, int N, int heads);
int dpm_attention_train_forward(const float *Q, int ldq, long long sq, const float *K, int ldk, long long sk, const float *V,
                                int ldv, long long sv, float *out, int ldo, long long so, float *lse, int B, int M, int N,
                                int heads, int head_dim, const uint8_t *key_mask, dpm_stream_t stream);
int dpm_attention_train_backward(const float *Q, int ldq, long long sq, const float *K, int ldk, long long sk, const float *V,
                                 int ldv, long long sv, const float *out, int ldo, long long so, const float *lse,
                                 const float *dout, int ldd, long long sd, const uint8_t *key_mask, float *dQ, float *dK,
                                 float *dV, int B, int M, int N, int heads, int head_dim, void *workspace, dpm_stream_t stream);

/* Offset pairs of the decoder's training forward (decoder.py:62-83: the (B,M,N) distance matrix, its threshold mask and
 * torch.nonzero) without that matrix (csrc/offset_pairs.hip).  xyz_a (B,3,M), xyz_b (B,3,N) fp32 contiguous, pad_* (B,M) / (B,N)
 * bytes, non-zero = padding.  A pair (b, i, j) exists when neither token is padding and dist2 = (dx dx + dy dy) + dz dz (fp32,
 * that order, no contraction) <= (float)(eps * eps).
 * count: counts (B*M) pairs per a row and offsets (B*M + 1), their exclusive scan with the total K last (-1: beyond int32).
 * fill: triples (K,3) int32 (b, i, j) in lexicographic order (torch.nonzero's), from the offsets of count.
 * gather: out (K,E) = x[(b_k * rows + i_k or j_k)] (side 0: the a index, 1: the b index); x (B*rows, E) rows ldx apart.
 * segment_sum: out (R,E) = per row r the sum of g[perm[k]] (perm NULL: g[k]) over k in [offsets[r], offsets[r+1]) in that
 *   order (g rows ldg apart): the backward of gather, many pairs per token, in a fixed order without atomics. */
int dpm_offset_pairs_count(const float *xyz_a, const float *xyz_b, const uint8_t *pad_a, const uint8_t *pad_b, int B, int M, int N,
                           double eps, int32_t *counts, int32_t *offsets, dpm_stream_t stream);
int dpm_offset_pairs_fill(const float *xyz_a, const float *xyz_b, const uint8_t *pad_a, const uint8_t *pad_b, int B, int M, int N,
                          double eps, const int32_t *offsets, int32_t *triples, dpm_stream_t stream);
int dpm_offset_pairs_gather(const float *x, int ldx, const int32_t *triples, int side, int rows, long long K, int E, float *out,
                            dpm_stream_t stream);
int dpm_offset_pairs_segment_sum(const float *g, int ldg, const int32_t *offsets, const int32_t *perm, long long R, int E,
                                 float *out, dpm_stream_t stream);

/* The grouping layer for training (csrc/group_train.hip): SetAbstraction / LocalAggregation's
 * gather -> [fea ; rel] -> Conv2d -> LayerNorm -> ReLU -> max over the K neighbours (pointnext.py:52-61, 97-107) with a
 * backward, replacing autograd over the (B, Cout, K, S) activations of build_mlp.  Same contract as dpm_group_gather_ln_max:
 * P (B,N,Cout) = fea W_f^T + b made by the caller, W_rel (Cout rows, ldw_rel apart, 3 used), idx clamped to [0, N).
 * forward: out (B,S,Cout) and slots (B,S,Cout) bytes: the k whose row gave the maximum (the smallest on ties), 255 where no
 *   row exceeds the ReLU floor (out = 0, no gradient).
 * backward: from dout (B,S,Cout) and the forward's slots -> dP (B,N,Cout) (rows nobody gathered are exact zeros), dW_rel
 *   (Cout,3) contiguous, dgamma, dbeta (Cout).  The pre-norm rows and their statistics are recomputed; the rows are regrouped
 *   by gathered point (a counting sort of idx, integer atomics only) and every dP row has one writer that adds in (s, k)
 *   order; the weight gradients are per-wave partials added in wave order: two runs give identical bytes.
 *   workspace: dpm_group_train_workspace_bytes(B,N,S,K,Cout), 16-byte aligned.
 * Cout in {32,64,128,256,512} and K in {16,32}, else DPM_EUNSUPPORTED (workspace_bytes: 0). */
int dpm_group_train_forward(const float *P, const float *xyz, const float *centers, const int32_t *idx, const float *W_rel,
                            int ldw_rel, const float *gamma, const float *beta, int B, int N, int S, int K, int Cout,
                            double radius, float *out, uint8_t *slots, dpm_stream_t stream);
size_t dpm_group_train_workspace_bytes(int B, int N, int S, int K, int Cout);
int dpm_group_train_backward(const float *P, const float *xyz, const float *centers, const int32_t *idx, const float *W_rel,
                             int ldw_rel, const float *gamma, int B, int N, int S, int K, int Cout, double radius,
                             const float *dout, const uint8_t *slots, float *dP, float *dW_rel, float *dgamma, float *dbeta,
                             void *workspace, dpm_stream_t stream);

/* The loop head for training (csrc/loop_head_train.hip; network/decoder/heads.py:45-69 OverlapHead under
 * pipeline/modules/model_pipeline.py:156-181, the reference's loop-detection stage: everything but the head is frozen).
 * loop_pool: x (B*L, E) token rows, ldx floats apart (16-byte aligned, ldx a multiple of 4), W1 (E,E) row-major, b1 (E) ->
 *   m (B,E), m[b,c] = (1/L) sum_l relu(x[b,l,:] . W1[c,:] + b1[c]): OverlapHead.mlp's first convolution, its ReLU and the mean
 *   over ALL L tokens (padding included, as torch.mean(dim=-1) there); the second convolution is affine and commutes with the
 *   mean, so it acts on m.  backward: from g = dL/dm (B,E) -> dW1 (E,E), db1 (E); the ReLU mask is recomputed with the
 *   forward's instruction sequence (same bits), x gets no gradient.  Neither direction writes a (B*L, E) tensor.
 *   workspace: dpm_loop_pool_workspace_bytes(B, L, E) for either call (per-tile column sums forward, a fixed number of
 *   partial dW1 backward); E = 256 only, else DPM_EUNSUPPORTED (workspace_bytes: 0).
 * loop_bce: pred, target (B,) -> *loss = mean(-(t max(log p, -100) + (1 - t) max(log(1 - p), -100))) (F.binary_cross_entropy,
 *   model_pipeline.py:158), stats (8) = [loss, n_pos, n_neg, n_equal, true_pos, false_pos, 0, 0] with the prediction p > 0.5
 *   (model_pipeline.py:160-173) and dpred_unit (B,) = (p - t) / max(p (1 - p), 1e-12) / B, the gradient of the loss: the
 *   backward is a product with it, there is no dpm_loop_bce_backward.
 * All products in fp32 on the matrix cores, no floating-point atomics: two runs give identical bytes. */
size_t dpm_loop_pool_workspace_bytes(int B, int L, int E);
int dpm_loop_pool_forward(const float *x, int ldx, const float *W1, const float *b1, int B, int L, int E, float *m,
                          void *workspace, dpm_stream_t stream);
int dpm_loop_pool_backward(const float *x, int ldx, const float *W1, const float *b1, const float *g, int B, int L, int E,
                           float *dW1, float *db1, void *workspace, dpm_stream_t stream);
int dpm_loop_bce_forward(const float *pred, const float *target, int B, float *loss, float *stats, float *dpred_unit,
                         dpm_stream_t stream);

/* The dense layers for training (csrc/dense_train.hip): build_mlp's Conv -> LayerNorm -> ReLU (network/encoder/utils.py:358-413),
 * the projections, LayerNorms and MLP of DescriptorAttentionLayer (network/decoder/descriptor_attention.py:16-48) and the heads
 * (network/decoder/heads.py), replacing F.linear / F.layer_norm / F.relu under autograd.  One primitive in two forms:
 *   plain  (gamma NULL):  out = act(x W^T + bias + residual)
 *   normed (gamma given): h = x W^T + bias + residual;  out = act(LN(h) * gamma + beta + post)   (eps 1e-5, biased variance)
 * x (R, Cin) rows ldx >= Cin floats apart, W (Cout, Cin) rows ldw >= Cin apart (any alignment: rows that are not 16-byte aligned
 * are read with scalar loads), bias (Cout) or NULL, residual / post (R, Cout) contiguous or NULL, act DPM_ACT_NONE or
 * DPM_ACT_RELU; out, h (R, Cout) and stats (R, 2) = (mean, rstd) per row are contiguous.  Any R >= 0, Cin, Cout >= 1.
 * forward: writes out and, normed, h and stats -- all the backward needs besides x, W and gamma (the ReLU mask is out > 0).
 *   Every h element is one k-ascending fp32 accumulator chain from zero, + bias, + residual: the same bits in both forms.
 * backward_rows: from dy (R, Cout) -> g = dy . [out > 0] (d post; for the plain form also d residual and the dh of the GEMMs; g
 *   may be NULL in the normed form), and normed: dh = rstd (dn - mean(dn) - xhat mean(dn xhat)) with dn = gamma g, xhat =
 *   (h - mean) rstd (d residual), dgamma = sum_rows g xhat, dbeta = sum_rows g (both or neither; they need workspace).
 *   out may be NULL for DPM_ACT_NONE.
 * backward_gemm: from dh -> dx (R, Cin) = dh W, dW (Cout, Cin) = dh^T x, dbias (Cout) = column sums of dh, all contiguous;
 *   each may be NULL and is skipped then (dbias needs dW).  The rows are cut into at most 32 slices of 64-row tiles whose
 *   partial dW are added in slice order.
 * R = 0 launches no kernel and zeroes dW, dbias, dgamma, dbeta.  workspace: dpm_dense_train_workspace_bytes(R, Cin, Cout) for
 * either backward call (host function: at most 32 (Cout Cin + Cout) + 256 x 2 Cout floats, constant in R beyond 32 tiles of 64 rows;
 * 0 for an invalid shape).
 * All products in fp32 on the matrix cores, no floating-point atomics, every sum in one order: two runs give identical bytes. */
size_t dpm_dense_train_workspace_bytes(long long R, int Cin, int Cout);
int dpm_dense_train_forward(const float *x, int ldx, const float *W, int ldw, const float *bias, const float *residual,
                            const float *gamma, const float *beta, const float *post, long long R, int Cin, int Cout, int act,
                            float *out, float *h, float *stats, dpm_stream_t stream);
int dpm_dense_train_backward_rows(const float *dy, const float *out, const float *h, const float *stats, const float *gamma,
                                  long long R, int Cout, int act, float *g, float *dh, float *dgamma, float *dbeta,
                                  void *workspace, dpm_stream_t stream);
int dpm_dense_train_backward_gemm(const float *dh, const float *x, int ldx, const float *W, int ldw, long long R, int Cin,
                                  int Cout, float *dx, float *dW, float *dbias, void *workspace, dpm_stream_t stream);

/* The map assembly of the registration training step (csrc/map_assemble.hip; pipeline/modules/model_pipeline.py:62-104 and
 * _get_accurate_RT, :199-272).  F = B * S encoded frames, map b = frames [b S, (b+1) S): its first S1 frames are the source map,
 * the other S2 = S - S1 the target map.  1 <= S1 < S, B * S <= 65535, any N, C >= 1.  A pose is 12 floats [R | T], 3x4 row-major.
 * map_poses (model_pipeline.py:70-94, 234-266; utils/pose.py:6-10): R (F,3,3), T (F,3,1), calib (F,4,4) the batch's global
 *   poses and calibrations; icp (F+B,16), has_icp (F+B,) bytes: the refined pose of an entry where the host found one
 *   (get_SE3_from_dict, model_pipeline.py:285-298, already `.float()`).  Entry f < F is frame f into the first frame of its map
 *   (frame 0 for s < S1, frame S1 otherwise), entry F + b is map b's source-first into its target-first.  -> rel (F,12), gt
 *   (B,12): with has_icp rows [:3] of d_calib @ icp @ inverse(s_calib) (fp32; the 4x4 inverse is a Gauss-Jordan elimination with
 *   partial pivoting), otherwise Rc^T Ro | Rc^T (To - Tc).  The two first frames of a map get the exact identity.  A singular
 *   calib is NOT supported: it gives Inf / NaN where the reference's `except` would take the global poses.
 * map_assemble_fwd (model_pipeline.py:40, 84, 95-104, 110-111): coor (F,3,N) unscaled, fea (F,C,N), mask (F,N) bytes ->
 *   src_desc (B, C+3, S1 N), dst_desc (B, C+3, S2 N): C feature rows, then xyz (torch.cat([fea, coor], 1)); src_mask (B, S1 N),
 *   dst_mask (B, S2 N); src_global (B,3,S1 N) = gt_R src_xyz + gt_T; dst_global (B,3,S2 N) = dst_xyz.  Token s' N + n of map b
 *   is point n of the map's frame s' (transpose(1,2).reshape).  Feature rows and masks are copies; xyz of a map's first frame is
 *   coor * (float)coor_scale and nothing else, of the others fma(r2, z, fma(r1, y, r0 * x)) + t per row of rel.
 * map_assemble_bwd: dfea (F,C,N) gathered from the two descriptor gradients (either may be NULL: zeros); the xyz rows and
 *   coor get no gradient.  A gather: exact, identical bytes on every run.
 * Rows are moved as float4 when N % 4 == 0 and the bases are 16-byte aligned, else by scalar accesses (decided per launch). */
int dpm_map_poses(const float *R, const float *T, const float *calib, const float *icp, const uint8_t *has_icp, int B, int S,
                  int S1, float *rel, float *gt, dpm_stream_t stream);
int dpm_map_assemble_fwd(const float *coor, const float *fea, const uint8_t *mask, const float *rel, const float *gt, int B, int S,
                         int S1, int N, int C, double coor_scale, float *src_desc, float *dst_desc, uint8_t *src_mask,
                         uint8_t *dst_mask, float *src_global, float *dst_global, dpm_stream_t stream);
int dpm_map_assemble_bwd(const float *d_src_desc, const float *d_dst_desc, int B, int S, int S1, int N, int C, float *dfea,
                         dpm_stream_t stream);

/* The optimiser step of a parameter group in one launch (csrc/optim.hip; the reference builds torch.optim.AdamW / Adam / SGD in
 * pipeline/modules/utils.py:86-100 and steps them in pipeline/modules/trainer.py:176-178).  tensors (T,5) int64 device table
 * [param, grad, state0, state1, numel] of fp32 arrays (state0 = exp_avg or momentum_buffer, state1 = exp_avg_sq; unused ones 0),
 * chunks (n_chunks,2) int32 device table [tensor, chunk]: one block per row updates elements [chunk * dpm_optim_chunk(),
 * min(numel, (chunk + 1) * dpm_optim_chunk())) of that tensor, so every element of the group must be covered by exactly one row.
 * torch's single-tensor rule in fp32: AdamW p *= 1 - lr wd; Adam and SGD g += wd p; m, v moving averages; p -= lr / (1 - beta1^step)
 * m / (sqrt(v) / sqrt(1 - beta2^step) + eps); SGD with momentum, dampening, nesterov; `first` (SGD): the momentum buffers are
 * being created (buf = g).  `step` (Adam, AdamW) is the step count AFTER this update, >= 1, the same for every tensor of the
 * call.  A tensor whose addresses are all 16-byte aligned moves as float4, any other by scalar accesses; the result does not
 * depend on the chunking.  n_chunks = 0 launches nothing. */
#define DPM_OPTIM_ADAMW 0
#define DPM_OPTIM_ADAM 1
#define DPM_OPTIM_SGD 2
int dpm_optim_chunk(void);
int dpm_optim_step(int algo, const long long *tensors, const int32_t *chunks, int n_chunks, double lr, double beta1, double beta2,
                   double eps, double weight_decay, double step, double momentum, double dampening, int nesterov, int first,
                   dpm_stream_t stream);

/* Data-parallel training: the gradients of a stage in ONE flat fp32 buffer (csrc/optim.hip; replaces the per-tensor bucket copies
 * of torch's DistributedDataParallel, which the reference wraps its model in at pipeline/modules/trainer.py:239-243).  table (T,3)
 * int64 device table [address, offset, numel]: an fp32 tensor of numel elements and its element offset into flat (a multiple of 4
 * by convention; any offset works, unaligned ones by scalar accesses); chunks as for dpm_optim_step.  flat[offset + i] =
 * tensor[i]; address 0 (a gradient that is None on this rank) writes zeros.  Elements of flat outside every row -- the padding --
 * are not touched.  flat_len: elements of flat, a multiple of 4; a row with offset + numel > flat_len moves nothing. */
int dpm_flat_pack(const long long *table, const int32_t *chunks, int n_chunks, float *flat, long long flat_len,
                  dpm_stream_t stream);
/* The inverse, for the initial broadcast of rank 0's parameters (what DistributedDataParallel's constructor does,
 * pipeline/modules/trainer.py:239-243): tensor[i] = flat[offset + i]; rows with address 0 are skipped. */
int dpm_flat_unpack(const long long *table, const int32_t *chunks, int n_chunks, const float *flat, long long flat_len,
                    dpm_stream_t stream);
/* dpm_optim_step with the gradient taken from the exchanged flat buffers instead of a tensor (replaces DistributedDataParallel's
 * all-reduce + unbucketing + the separate optimiser pass, pipeline/modules/trainer.py:239-243 and 176-178).  Column 1 of
 * `tensors` is the tensor's element offset into a slice, not an address.  slices: n_slices >= 1 buffers of fp32, slice r at
 * slices + r * slice_stride (slice_stride % 4 == 0, and offset + numel <= slice_stride for every row: others update nothing).
 * Per element g = slice_0[i]; g = g + slice_r[i] for r = 1 .. n_slices - 1, in this order; g = g / (float)divisor (a true IEEE
 * division, divisor >= 1); then the element rule of dpm_optim_step, the same code.  An all-gathered buffer passes n_slices = W,
 * divisor = W; an all-reduced one n_slices = 1, divisor = W.  n_slices = 1, divisor = 1 is dpm_optim_step on that buffer. */
int dpm_optim_step_synced(int algo, const long long *tensors, const int32_t *chunks, int n_chunks, double lr, double beta1,
                          double beta2, double eps, double weight_decay, double step, double momentum, double dampening,
                          int nesterov, int first, const float *slices, int n_slices, long long slice_stride, double divisor,
                          dpm_stream_t stream);

/* ---------------------------------------------------------------- LiDAR simulator -------- */

/* A spinning-LiDAR model ray-cast through a procedural scene (csrc/lidar_sim.hip; deeppointmap_amd/lidar_sim.py builds the
 * scenes).  It has no counterpart in the reference.  A batch of F frames takes these three calls = three launches,
 * whatever F is, without a host synchronisation; the sequence can be captured in a graph.
 * Scene: prims (P,10) float64 = centre x y z (a cylinder: the centre of its base), three extents (a box: half extents
 * along its own axes; a cylinder: radius, height, 0), cos and sin of the yaw about world z (a cylinder: 1, 0), the z offset
 * of the bounding sphere's centre from the centre and its radius; kind (P,) 0 = box, 1 = capped vertical cylinder;
 * ground (2,) float64 = (z0, 1.0 when the plane z = z0 exists else 0.0).  poses (F,4,4) float64 row-major sensor-to-world.
 * dpm_lidar_cull moves every primitive into frame f's sensor frame in float64, rounds to float32 and keeps, in ascending
 * primitive index, those whose bounding sphere reaches the ball of max_range: kept (F,max_kept,16) fp32 records = the
 * sensor's origin in the primitive's coordinates (3), the three rows that take a sensor-frame direction to those
 * coordinates (9), the extents (3), and primitive index | kind << 30 as bits; plane (F,4) = the ground's unit normal and
 * offset in the sensor frame (zeros without ground); status (F,2) = (kept primitives, 1 when that exceeds max_kept: the
 * surplus is dropped and the caller raises at its next read-back). */
int dpm_lidar_cull(const double *prims, const int32_t *kind, int P, const double *ground, const double *poses, int F,
                   double max_range, int max_kept, float *kept, float *plane, int32_t *status, dpm_stream_t stream);
/* One lane per ray: dirs (rays,3) fp32 unit directions in the sensor frame.  Per ray of every frame the smallest t > 0
 * over all kept surfaces and the ground; equal t goes to the lowest primitive index, the ground last; an origin inside a
 * primitive sees its exit face.  Outputs (F,rays): range fp32, prim int32 (primitive index, P for the ground, -1 for no
 * return), cos_inc = |normal . direction|.  A nearest hit below min_range or beyond max_range is no return (range 0,
 * prim -1, cos_inc 0).  Arithmetic is + - * / sqrt, each rounded once. */
int dpm_lidar_cast(const float *kept, const float *plane, const int32_t *status, int max_kept, int P, const float *dirs,
                   int rays, int F, double min_range, double max_range, float *range, int32_t *prim, float *cos_inc,
                   dpm_stream_t stream);
/* Sweep motion: the sensor moves from poses0[f] to poses1[f] (both (F,4,4) float64 sensor-to-world) while it fires its
 * azimuth_steps columns, column c at sweep fraction s_c = c / azimuth_steps from the pose P0 D(s_c), D = P0^-1 P1, D(s) =
 * (Exp(s Log R_D), s t_D), rotation angle below pi.  dpm_lidar_cull_sweep is dpm_lidar_cull about poses0 with the
 * max_range ball enlarged by |t_D|, and also writes table (F,azimuth_steps,12) fp32 = Exp(s_c Log R_D) row-major (9) and
 * s_c t_D (3), computed in float64 and rounded once.  dpm_lidar_cast_sweep is dpm_lidar_cast with ray r (of column
 * r mod azimuth_steps; rays a multiple of azimuth_steps) turned by its column's rotation and cast from its column's
 * origin; range is measured from that origin, so dpm_lidar_emit's t * dir is the point in the sensor's frame at the
 * ray's own time.  With poses1 == poses0 the table is exactly identity and zero and the outputs equal the static calls'. */
int dpm_lidar_cull_sweep(const double *prims, const int32_t *kind, int P, const double *ground, const double *poses0,
                         const double *poses1, int F, int azimuth_steps, double max_range, int max_kept, float *kept,
                         float *plane, int32_t *status, float *table, dpm_stream_t stream);
int dpm_lidar_cast_sweep(const float *kept, const float *plane, const int32_t *status, int max_kept, int P, const float *dirs,
                         int rays, int F, const float *table, int azimuth_steps, double min_range, double max_range,
                         float *range, int32_t *prim, float *cos_inc, dpm_stream_t stream);
/* Returns -> frames in the layout of the training transforms.  A ray returns when prim >= 0 and (u == NULL or
 * u >= (float)drop_prob); its point is (range + noise) * dir (noise (F,rays) metres or NULL).  xyz (F,rays,3), idx (F,rays)
 * = the ray index of every row, count (F,): the returns in ray order, rows at and past the count zero.  intensity (F,rays)
 * = albedo[prim] * cos_inc and label (F,rays) = class_id[prim] per RAY (0 / -1 without a hit); albedo, class_id (P+1,)
 * with the ground at P.  No atomics: two runs give identical bytes. */
int dpm_lidar_emit(const float *range, const int32_t *prim, const float *cos_inc, const float *dirs, int rays, int F,
                   const float *noise, const float *u, double drop_prob, const float *albedo, const int32_t *class_id, int P,
                   float *xyz, int32_t *idx, int32_t *count, float *intensity, int32_t *label, dpm_stream_t stream);

/* ---------------------------------------------------------------- map evaluation -------- */

/* How far a point-cloud map lies from the surfaces it should lie on (csrc/map_eval.hip; deeppointmap_amd/evaluate.py is the
 * caller).  No counterpart in the reference.  Clouds are (3,M) fp32 channel-first on the device (what globalmap.voxel_map
 * returns).  Every entry point takes an origin of three doubles by value and shifts every point ONCE, q = (float)((double)p -
 * origin); everything after that is fp32 in + - * / sqrt, each rounded once, on numbers no larger than the map's extent.  No
 * floating-point atomics: two runs give identical bytes.  Every call runs on `stream` without a host synchronisation.
 *
 * dpm_scene_distance: per point the unsigned distance to the nearest surface of a simulator scene and that surface's id.
 * records (P,12) fp32, prepared in float64 and rounded once: centre - origin (3), cos and sin of the yaw (a cylinder: 1, 0),
 * the extents (a box: its half extents; a cylinder: radius, HALF height, 0, the centre being the middle of its axis), the kind
 * (0 = box, 1 = cylinder) as BITS, three floats of padding.  ground = z0 - origin_z (rounded to fp32 here), has_ground != 0
 * when the plane exists.  With d = q - centre, in this order of operations:
 *   box       lx = cos*dx + sin*dy, ly = cos*dy - sin*dx, lz = dz; a_k = |l_k| - h_k, o_k = max(a_k, 0);
 *             dist = |sqrt((ox*ox + oy*oy) + oz*oz) + min(max(ax, max(ay, az)), 0)|
 *   cylinder  a0 = sqrt(dx*dx + dy*dy) - r, a1 = |dz| - hh, o_k = max(a_k, 0);
 *             dist = |sqrt(o0*o0 + o1*o1) + min(max(a0, a1), 0)|
 *   ground    |qz - ground|
 * The records are walked in ascending index and a strictly smaller distance wins, the ground last: equal distances keep the
 * lower index and the ground loses ties.  dist (M,) fp32, surf (M,) int32 = 0..P-1, P for the ground.  A point whose shifted
 * coordinates are not all finite, or an empty scene (P = 0 and no ground), gives +inf and -1.  P x M evaluations: no culling. */
int dpm_scene_distance(const float *points, int M, const float *records, int P, double ground, int has_ground, double origin_x,
                       double origin_y, double origin_z, float *dist, int32_t *surf, dpm_stream_t stream);
/* Exact truncated nearest neighbour from query (3,Nq) to target (3,Nt): the winner is the target with the smallest
 * d2 = (dx*dx + dy*dy) + dz*dz on the shifted coordinates among those with d2 <= (float)(max_dist * max_dist); equal d2 goes to
 * the smaller target index (the (distance bits, index) key of csrc/icp.hip).  dist (Nq,) = sqrt(d2) or +inf without one,
 * idx (Nq,) int32 or -1.  Targets with a non-finite coordinate are nobody's neighbour, queries with one have none.  The target
 * side is counting-sorted once per call into a uniform grid with a cell edge of max(1.001 max_dist, extent / 127) -- at most
 * 128 cells per axis; beyond that the edge grows, the result stays exact and only the candidate count grows -- and every
 * query looks into 3 x 3 x 3 cells.  Nt = 0 is allowed (every query: +inf, -1).  workspace: dpm_cloud_nn_workspace_bytes. */
size_t dpm_cloud_nn_workspace_bytes(int Nq, int Nt);
int dpm_cloud_nn(const float *query, int Nq, const float *target, int Nt, double max_dist, double origin_x, double origin_y,
                 double origin_z, float *dist, int32_t *idx, void *workspace, dpm_stream_t stream);
/* A distance array -> out (C+1, 5+T) float64 in two launches: rows = class 0..C-1, then the total over EVERY point; columns =
 * matched count, unmatched count, sum of d, sum of d*d, max d, count with d <= thresholds[t].  A point is matched when its
 * distance is finite and <= (float)max_dist; the sums, the maximum and the threshold counts are taken over matched points (0
 * without any).  A point's class is class_id[surf[i]] (surf (M,) int32 into class_id (n_surf,) int32; a surf outside
 * [0, n_surf) or a class outside [0, C) counts in the total only); C = 0 takes no surf and gives the total row alone.
 * thresholds: T <= DPM_STATS_MAX_THRESHOLDS floats ON THE HOST, read before the launch.  Orders: every block takes a contiguous
 * chunk of the points, lane t of 256 walks first + t, first + t + 256, ... adding (double)d and (double)d * (double)d; the 64
 * lanes of a wave are added by the xor butterfly 32, 16, .. 1, the four waves as (w0 + w1) + (w2 + w3); one final block adds the
 * blocks' partials in block order.  workspace: dpm_distance_stats_workspace_bytes. */
#define DPM_STATS_MAX_THRESHOLDS 8
#define DPM_STATS_MAX_CLASSES 256
size_t dpm_distance_stats_workspace_bytes(int M, int C, int T);
int dpm_distance_stats(const float *dist, int M, const int32_t *surf, const int32_t *class_id, int n_surf, int C,
                       const float *thresholds, int T, double max_dist, double *out, void *workspace, dpm_stream_t stream);

/* ---------------------------------------------------------------- geometric odometry -------- */

/* A rolling hashed voxel map and the registration of a scan against it (csrc/local_map.hip; deeppointmap_amd/odometry.py is
 * the caller).  No counterpart in the reference, which estimates poses with its learned pipeline only.
 *
 * The map is one device buffer of dpm_local_map_bytes(cap_vox, subdiv) bytes, 16-byte aligned: a 256-byte header (word 0:
 * points that found no free slot, word 1: points outside the key range) and two halves, each an open-addressing table of
 * cap_vox slots (a power of two in [2, 2^24], linear probing from splitmix64(key) & (cap_vox - 1), empty key ~0) with
 * S = subdiv^3 sub-cells a slot, subdiv in {1, 2, 3}.  `half` (0 or 1) names the half a call works on; the caller flips it
 * after every prune.  `voxel` (metres) and `origin` (three doubles ON THE HOST, read before the launch) must be the same in
 * every call on one map.  Poses are 16 doubles (4x4 row-major, sensor -> world) IN DEVICE MEMORY: a call queues behind the
 * kernel that wrote them without a host read.  In the map frame a pose is R -> (float)R, t -> (float)(t - origin), a point
 * is q = fma(R2, z, fma(R1, y, R0 * x)) + t per axis, and per axis f = q / voxel (fp32, correctly rounded), the voxel is
 * floor(f) (kept when in [-2^20, 2^20); the key packs the three, biased by 2^20, 21 bits each, x lowest) and the sub-cell
 * coordinate min((int)((f - floor f) * subdiv), subdiv - 1); sub-cell number (c * subdiv + b) * subdiv + a for (x, y, z) =
 * (a, b, c).  A sub-cell holds one point: an owner word (stamp << 32) | row and its fp32 map-frame coordinates.
 * RULE: a sub-cell belongs to the smallest owner word ever offered to it -- an older frame (smaller stamp) is never
 * displaced, within a frame the smaller row wins.  Integer atomics only: what a key leads to is a function of the inserted
 * points alone (slot positions are not); two runs export identical bytes once sorted.  The map is defined only while header
 * word 0 is zero.  Every call runs on `stream` without a host synchronisation. */
size_t dpm_local_map_bytes(int cap_vox, int subdiv);
/* header zeroed, both halves empty */
int dpm_local_map_init(void *map, int cap_vox, int subdiv, dpm_stream_t stream);
/* One frame in two launches (claim, commit).  xyz (cap,3) fp32 row-major, idx (cap,) int32 = the row number the rule sees
 * (a frame's original rows, carried through sampling), count (1,) int32 on the device: rows at and past it are neither read
 * nor written.  A row is offered when (float)(min_range^2) <= (x*x + y*y) + z*z <= (float)(max_range^2) on the SENSOR-frame
 * point (a NaN fails).  stamp < 2^32 - 1 must grow from frame to frame. */
int dpm_local_map_insert(void *map, int cap_vox, int subdiv, int half, double voxel, const double *origin, const float *xyz,
                         const int32_t *idx, const int32_t *count, int cap, const double *pose, unsigned stamp,
                         double min_range, double max_range, dpm_stream_t stream);
/* Half `half` -> the other half (cleared first): a voxel survives when its centre c = ((float)voxel_index + 0.5f) * voxel per
 * axis has (dx*dx + dy*dy) + dz*dz <= (float)(radius^2) from the pose's map-frame translation; its sub-cells are copied. */
int dpm_local_map_prune(void *map, int cap_vox, int subdiv, int half, double voxel, const double *origin, const double *pose,
                        double radius, dpm_stream_t stream);
/* A list of stored frames in two launches for any F (claim, commit; grid y = list entry), no workspace, capturable: what it
 * takes to rebuild a map from keyframes.  store (capacity,3,P) fp32 CHANNEL-major and lengths (capacity,) int32 on the device
 * (a length is clamped to [0, P], as dpm_local_map_insert clamps count); frames (F,) int32 rows of the store (a row outside
 * [0, capacity) offers nothing), poses (F,16) fp64 sensor -> world, stamps (F,) uint32 pairwise distinct and < 2^32 - 1, all on
 * the device; F in [0, 65535], F = 0 is a no-op.  Column i of entry f is offered under exactly dpm_local_map_insert's rule
 * (range gate on the sensor-frame point, the transform, voxel, key and sub-cell) with the owner word (stamps[f] << 32) | i.
 * centre: 16 doubles on the device (a pose; its translation is used) or NULL.  With a centre, a row is offered only when
 * its voxel passes dpm_local_map_prune's test around it -- the same fp32 expression on the voxel's centre,
 * (float)(centre_t - origin) and (float)(radius^2).  Header word 1 counts as dpm_local_map_insert counts it, before the
 * filter; header word 0 counts rows that pass the filter and find no slot.  On a map that does not overflow, the sorted export
 * equals that after dpm_local_map_insert of each entry with its stamp, in any order, followed by dpm_local_map_prune(centre,
 * radius), byte for byte; voxels the prune would drop never take a slot. */
int dpm_local_map_insert_frames(void *map, int cap_vox, int subdiv, int half, double voxel, const double *origin,
                                const float *store, const int32_t *lengths, int capacity, int P, const int32_t *frames,
                                const double *poses, const uint32_t *stamps, int F, const double *centre, double radius,
                                double min_range, double max_range, dpm_stream_t stream);
/* Robust point-to-point ICP of the frame's first count rows against the map, from init_pose (device), over the schedule
 * (stage_max_dist, stage_max_iter: n_stages <= 16 values ON THE HOST): two launches per iteration, capturable.  Every
 * stage_max_dist must be <= voxel: a query looks into the 3 x 3 x 3 voxels around its own.  The match is the occupied
 * sub-cell with the smallest key (bits of d2 = (dx*dx + dy*dy) + dz*dz, n * 32 + sub-cell), n = ((dz+1) * 3 + (dy+1)) * 3 +
 * (dx+1) the neighbour's number, accepted when d2 <= (float)(max_dist^2).  Rows: point-to-point, weighted
 * w = (k / (k + e.e))^2 with k = kernel_scale^2 (metres; 0: w = 1), summed in fp64 in a fixed order into the 29 values of
 * dpm_icp_refine_batched (H and g weighted; match count and squared residuals not); solve, update, stop rule and the
 * DPM_ICP_* statuses as there.  NO_MATCH (also: empty map, count 0) and SINGULAR leave the pose where it was; no NaN or Inf
 * is written.  pose (16), fitness, rmse, iterations, status: one value each, on the device.  Optional: debug_key / debug_sub
 * (cap,) the matched voxel key and sub-cell of every row at the last evaluated pose (-1: none), debug_system (29).
 * workspace: 512 + 256 * ceil(cap / 256) bytes. */
int dpm_local_map_register(const void *map, int cap_vox, int subdiv, int half, double voxel, const double *origin,
                           const float *xyz, const int32_t *count, int cap, const double *init_pose,
                           const double *stage_max_dist, const int32_t *stage_max_iter, int n_stages, double kernel_scale,
                           double tol_rot, double tol_trans, double *pose, float *fitness, float *rmse, int32_t *iterations,
                           int32_t *status, long long *debug_key, int32_t *debug_sub, double *debug_system, void *workspace,
                           dpm_stream_t stream);
/* Every occupied sub-cell of half `half`, in no defined order: keys / owner (max_out,) uint64, sub (max_out,) int32,
 * xyz (max_out,3) fp32 map-frame.  count (1,) int32, ZEROED BY THE CALLER, receives their number, which may exceed max_out
 * (the rest is not written; max_out = 0 only counts). */
int dpm_local_map_export(const void *map, int cap_vox, int subdiv, int half, unsigned long long *keys, int32_t *sub,
                         unsigned long long *owner, float *xyz, int32_t *count, int max_out, dpm_stream_t stream);
/* One plane per held voxel of half `half`, a cache derived from the map in caller-owned buffers indexed by SLOT: planes
 * (cap_vox,4) fp32 (nx, ny, nz, w), 16-byte aligned, and counts (cap_vox,) int32.  One launch, capturable.  The voxel's centre
 * is c = ((float)voxel_index + 0.5f) * voxel per axis; its members are the occupied sub-cell points p of the 27 voxels around
 * it with d = p - c (fp32) and (dx*dx + dy*dy) + dz*dz <= (float)(plane_radius^2); 0 < plane_radius <= 1.5 voxel, so the ball
 * lies inside those voxels (a point exactly 1.5 voxel from c along +x, +y or +z lies on the far face of a neighbour and so
 * in the voxel after it: not a member).  counts = the number of members.  The ten cumulants of d are summed in fp64 in an order fixed by
 * the geometry (neighbour number as in dpm_local_map_register, then sub-cell), the scatter matrix n S_ab - S_a S_b (the
 * covariance times n^2) is diagonalised by cyclic Jacobi in fp64, the eigenvalues l0 <= l1 <= l2 ordered with the smaller
 * axis first among equals.  The normal is the unit eigenvector of l0 rounded to fp32, signed so that its component of
 * largest magnitude (the first axis among equal fp32 magnitudes) is positive; w = (float)(max(l0, 0) / l1), the flatness.
 * counts < 3, or l1 <= 1e-8 l2 -- a line to the precision fp32 coordinates have, which includes l1 <= 0; its "normal" would
 * be rounding noise --: (0, 0, 0, -1).  A slot without a voxel: (0, 0, 0, -1) and count 0.  A voxel's plane is a function of
 * the map's content alone, not of slot positions or arrival order.  The buffers are stale after any insert or prune. */
int dpm_local_map_planes(const void *map, int cap_vox, int subdiv, int half, double voxel, const double *origin,
                         double plane_radius, float *planes, int32_t *counts, dpm_stream_t stream);
/* dpm_local_map_register with point-to-plane rows: the same search, tie-break, schedule, solve, statuses and workspace.
 * planes / counts: what dpm_local_map_planes wrote for this map and half.  The matched point's voxel gives a row only when
 * counts >= min_points and 0 <= w <= (float)max_ratio: e = (nx*ex + ny*ey) + nz*ez with (ex, ey, ez) = query - match,
 * J = (p x n, n) as DPM_ICP_PLANE, weighted (k / (k + e*e))^2 with k = kernel_scale^2.  A match whose voxel has no such plane
 * contributes nothing: the match count (fitness, rmse, NO_MATCH) counts rows, and debug_key / debug_sub are -1 for it. */
int dpm_local_map_register_planes(const void *map, int cap_vox, int subdiv, int half, double voxel, const double *origin,
                                  const float *planes, const int32_t *counts, int min_points, double max_ratio,
                                  const float *xyz, const int32_t *count, int cap, const double *init_pose,
                                  const double *stage_max_dist, const int32_t *stage_max_iter, int n_stages,
                                  double kernel_scale, double tol_rot, double tol_trans, double *pose, float *fitness,
                                  float *rmse, int32_t *iterations, int32_t *status, long long *debug_key, int32_t *debug_sub,
                                  double *debug_system, void *workspace, dpm_stream_t stream);

/* ---------------------------------------------------------------- TSDF surface map ---------- */

/* A truncated signed distance field over hashed voxels and a surface from it (csrc/tsdf_map.hip; deeppointmap_amd/tsdf.py is
 * the caller).  No counterpart in the reference, whose map is a cloud of points.  DESIGN §7l is the definition.
 *
 * The map is one device buffer of dpm_tsdf_bytes(cap_vox) = 256 + 20 cap_vox bytes, 16-byte aligned: a 256-byte header (word
 * 0: samples that found no free slot, word 1: samples outside the key range, word 2: rows without a usable normal -- the
 * plane-distance form below) and one open-addressing table of cap_vox slots
 * (a power of two in [2, 2^24], linear probing from splitmix64(key) & (cap_vox - 1), empty key ~0) as three arrays: key
 * uint64, sum int64, count uint32.  Keys, the map frame and the pose handling are dpm_local_map_insert's: `voxel` and `origin`
 * (three doubles ON THE HOST) the same in every call on one map, a pose 16 doubles IN DEVICE MEMORY entering as (float)R and
 * (float)(t - origin), a point q = fma(R2, z, fma(R1, y, R0 * x)) + t, per axis the voxel floor(q / voxel) from the correctly
 * rounded fp32 quotient, kept in [-2^20, 2^20), the 3 x 21-bit key, the centre c = ((float)voxel_index + 0.5f) * voxel.
 *
 * FUSION.  A row (x, y, z) of a frame is a return seen from the pose's translation.  It is taken when (float)(min_range^2) <=
 * r2 <= (float)(max_range^2) with r2 = (x*x + y*y) + z*z (a NaN fails).  In fp32, every operation rounded once, no fused
 * multiply-add outside q's chain, division and square root correctly rounded:
 *     r = sqrt(r2),  o = (float)(t - origin),  u = (q - o) / r per axis;
 *     n = ceil(truncation / step) on the host in double (at most 4096), tau = (float)truncation, h = (float)step;
 *     for k = -n .. n ascending:  t = r + (float)k * h;  skipped unless t > 0;  p = o + u * t per axis;  the voxel of p (a
 *     sample outside the 21 bits adds one to header word 1 and is skipped);  skipped when its key equals the key of this
 *     ray's previous keyed sample;  e = q - c;  s = (ux*ex + uy*ey) + uz*ez clamped to [-tau, tau], positive on the sensor's
 *     side of the return;  fixed = (long long)rintf(s * 16777216.f), round half to even;  the slot found or claimed, then
 *     sum += fixed and count += 1 (integer atomics).  No free slot: header word 0 counts the sample.
 * 0 < truncation <= 64 (metres): tau 2^24 2^32 < 2^63, so 2^32 samples cannot overflow a sum.  Integer addition commutes: what
 * a key leads to is the same whatever the order of rows, frames or launches (slot positions are not); two runs export
 * identical bytes once sorted.  The map is defined only while header word 0 is zero.  A return at range 0 has no direction:
 * u is NaN and its samples with t > 0 count in header word 1.  Every call runs on `stream` without a host synchronisation.
 *
 * FIELD.  D = (float)((double)sum / ((double)count * 16777216.0)) of a slot.  A voxel is QUALIFIED when count >= min_count
 * (min_count >= 1); a voxel without a slot, or outside the 21 bits, is not. */
size_t dpm_tsdf_bytes(int cap_vox);
/* header zeroed, table empty */
int dpm_tsdf_init(void *map, int cap_vox, dpm_stream_t stream);
/* One frame in one launch, one lane per row, capturable.  xyz (cap,3) fp32 row-major, count (1,) int32 on the device: rows at
 * and past it are never read.  DPM_EINVAL: truncation outside (0, 64], step <= 0, ceil(truncation / step) > 4096. */
int dpm_tsdf_integrate(void *map, int cap_vox, double voxel, const double *origin, const float *xyz, const int32_t *count,
                       int cap, const double *pose, double min_range, double max_range, double truncation, double step,
                       dpm_stream_t stream);
/* The same rule over a list of stored frames in one launch for any F (grid y = list entry), capturable.  store (capacity,3,P)
 * fp32 CHANNEL-major and lengths (capacity,) int32 (a length is clamped to [0, P]), frames (F,) int32 rows of the store (a
 * row outside [0, capacity) offers nothing), poses (F,16) fp64, all on the device; F in [0, 65535], F = 0 is a no-op.  The
 * sorted export equals that after dpm_tsdf_integrate of each entry, byte for byte. */
int dpm_tsdf_integrate_frames(void *map, int cap_vox, double voxel, const double *origin, const float *store,
                              const int32_t *lengths, int capacity, int P, const int32_t *frames, const double *poses, int F,
                              double min_range, double max_range, double truncation, double step, dpm_stream_t stream);
/* PLANE-DISTANCE FUSION.  dpm_tsdf_integrate / _frames with one change: the distance of the voxel's centre to the TANGENT PLANE
 * at the return replaces its distance along the ray (which is wrong by about d tan(incidence) for a centre d beside the ray),
 * and a sample is weighted by the cosine of the incidence.  normals: fp32 IN THE SENSOR FRAME, one per row, unit length
 * expected and not renormalised (either sign); (cap,3) row-major beside xyz, or for the list form a store (capacity,P,3) beside
 * `store` (what ops.icp_target_normals writes).  0 <= cos_min <= 1.  The range gate, r, q, o, u, n, the samples t = r + (float)k
 * * h, the t > 0 test, the voxel of o + u * t, header word 1 and the skip of a repeated key are the rule above, untouched.  Per
 * row, once, in fp32 (R the (float) rotation of the pose, as q's chain uses it):
 *     n_m[a] = fma(R[a][2], nz, fma(R[a][1], ny, R[a][0] * nx));   a0 = (n_m.x*u.x + n_m.y*u.y) + n_m.z*u.z;
 *     m = a0 >= 0 ? n_m : -n_m (away from the sensor, as u);   a = |a0|;   wq = (int)rintf(a * 256.f), round half to even.
 * The row is USABLE when wq >= 1 and a >= (float)cos_min; a zero or NaN normal (or a return at range 0) fails by comparison.  A
 * row that passed the range gate and is not usable adds one to header word 2 -- one per row -- and offers no sample (nor
 * anything to header word 1).  Per kept sample of a usable row, with e = q - c:
 *     s = (m.x*ex + m.y*ey) + m.z*ez clamped to [-tau, tau], positive on the sensor's side;  fixed = (long long)rintf(s *
 *     16777216.f);  sum += wq * fixed and count += wq (integer atomics).  No free slot: header word 0 grows by wq.
 * D = sum / (count * 2^24) is then the weighted mean and the extractions below read it unchanged; a full-weight sample counts
 * 256, and min_count is in those units.  Headroom (|n| <= 1): wq <= 256 and |fixed| <= 2^30, so wq * |fixed| <= 2^38 and a sum
 * holds 2^24 such samples; a count (uint32) wraps after 2^24 full-weight samples of one voxel.  A map is fused in ONE of the two
 * forms: their counts have different units.  Order independence and the equality of the list form with the per-frame calls hold
 * as above. */
int dpm_tsdf_integrate_planes(void *map, int cap_vox, double voxel, const double *origin, const float *xyz, const float *normals,
                              const int32_t *count, int cap, const double *pose, double min_range, double max_range,
                              double truncation, double step, double cos_min, dpm_stream_t stream);
int dpm_tsdf_integrate_planes_frames(void *map, int cap_vox, double voxel, const double *origin, const float *store,
                                     const float *normals, const int32_t *lengths, int capacity, int P, const int32_t *frames,
                                     const double *poses, int F, double min_range, double max_range, double truncation,
                                     double step, double cos_min, dpm_stream_t stream);
/* FREE-SPACE CARVING, lookups only: no slot is claimed, the key set stays as it is.  The frame and list arguments of
 * dpm_tsdf_integrate / _frames; weight in [1, 65535] in the map's count units (1 a sample of a ray-distance map, 256 of a
 * plane-distance map); margin >= 0 metres.  DPM_EINVAL also when max_range / step > 65536.  Per row that passes the range gate,
 * with r, q, o, u as above, for k = 1, 2, ... while t = (float)k * h < r - (float)margin:  the voxel of o + u * t (outside the
 * 21 bits: skipped silently);  skipped when its key equals the key of this ray's previous keyed sample;  if the table holds the
 * key:  sum += weight * tau_fixed with tau_fixed = (long long)rintf(tau * 16777216.f), and count += weight -- the observation
 * "free, at the truncation distance".  The result is a function of (the map before the call, the set of frames), not of their
 * order.  Carving is meant to run AFTER the integrations (it reaches only voxels that exist); a later integrate adds to what
 * is there. */
int dpm_tsdf_carve(void *map, int cap_vox, double voxel, const double *origin, const float *xyz, const int32_t *count, int cap,
                   const double *pose, double min_range, double max_range, double truncation, double step, int weight,
                   double margin, dpm_stream_t stream);
int dpm_tsdf_carve_frames(void *map, int cap_vox, double voxel, const double *origin, const float *store, const int32_t *lengths,
                          int capacity, int P, const int32_t *frames, const double *poses, int F, double min_range,
                          double max_range, double truncation, double step, int weight, double margin, dpm_stream_t stream);
/* Every occupied slot in no defined order: keys (max_out,) uint64, sums (max_out,) int64, counts (max_out,) uint32.  count
 * (1,) int32, ZEROED BY THE CALLER, receives their number, which may exceed max_out (the rest is not written; max_out = 0
 * only counts). */
int dpm_tsdf_export(const void *map, int cap_vox, unsigned long long *keys, long long *sums, uint32_t *counts, int32_t *count,
                    int max_out, dpm_stream_t stream);
/* ROLLING THE MAP.  A TILE is the cube of 2^b voxels per axis (b = tile_bits in [3, 10]) that share key_axis >> b, the BIASED
 * index; its centre per axis, in fp32 with every operation rounded once, is
 *     c = ((float)(((index >> b) << b) - 1048576) + 0.5f * (float)(1 << b)) * (float)voxel,
 * and it is NEAR a pose when, with d = c - (float)(pose[3 | 7 | 11] - origin) per axis,
 *     (dx*dx + dy*dy) + dz*dz <= (float)(radius * radius):
 * dpm_local_map_prune's test on the tile's centre.  A NaN fails: every tile is then far.
 *
 * dpm_tsdf_evict rebuilds the table `src` into `dst`, a second buffer of dpm_tsdf_bytes(cap_vox) bytes that is not src: dst is
 * cleared, src's header words 0 to 2 are copied into it and count_out[0] is set to 0 (first launch); then, one lane per slot of
 * src (second launch), a voxel of a NEAR tile is claimed in dst and its sum and count stored; a voxel of any other tile takes a
 * position in the list -- keys_out (max_out,) uint64, sums_out (max_out,) int64, counts_out (max_out,) uint32, in no defined
 * order -- and is written there when its position is below max_out; OTHERWISE IT STAYS, claimed in dst like a near voxel.
 * count_out (1,) int32 ends as the number of voxels that wanted out, which may exceed max_out; which of them found room is
 * not defined.  In every case the multiset (key, sum, count) of dst and the first min(count_out, max_out) records together is
 * that of src: nothing is dropped, nothing is changed.  src keeps its bytes; the caller swaps the buffers.  max_out = 0 with
 * null lists is legal (a plain rebuild).  pose: 16 doubles on the device.  No host synchronisation, capturable.
 * DPM_EINVAL: src == dst, tile_bits outside [3, 10], radius < 0, and what dpm_tsdf_integrate refuses of map, voxel and origin.
 *
 * dpm_tsdf_absorb adds n records (keys (n,) uint64, sums (n,) int64, counts (n,) uint32 on the device) to the table, one lane
 * per record in one launch: a record whose key has bit 63 set (no voxel's key has; the empty key does) adds one to header word
 * 1 and is skipped; a record with count == 0 is skipped; otherwise the slot is found or claimed and sum += s, count += c by
 * dpm_tsdf_integrate's integer atomics.  No free slot: header word 0 counts the record.  Equal keys inside the list and keys the
 * table holds add, and the result is the same bytes for any order of records.  n = 0 is a no-op (null lists are legal).  After
 * an evict, absorbing its list into dst gives the sorted export of src, byte for byte. */
int dpm_tsdf_evict(const void *src, void *dst, int cap_vox, double voxel, const double *origin, const double *pose,
                   double radius, int tile_bits, unsigned long long *keys_out, long long *sums_out, uint32_t *counts_out,
                   int32_t *count_out, int max_out, dpm_stream_t stream);
int dpm_tsdf_absorb(void *map, int cap_vox, const unsigned long long *keys, const long long *sums, const uint32_t *counts, int n,
                    dpm_stream_t stream);
/* Zero crossings along the axes, one lane per slot, in no defined order, count / max_out as above.  A record is written for
 * a qualified voxel k0 and an axis a when k1 = k0 + e_a is qualified and (D0 < 0) != (D1 < 0): keys = k0, axes = a, xyz
 * (max_out,3) = k0's centre with f * voxel added on axis a, f = D0 / (D0 - D1) (fp32, correctly rounded; map frame).
 * grad(k)_b from the qualified neighbours of k on axis b: both: D(k + e_b) - D(k - e_b); only k + e_b: 2 (D(k + e_b) - D(k));
 * only k - e_b: 2 (D(k) - D(k - e_b)); neither: 0.  normals (max_out,3) = g / sqrt((gx*gx + gy*gy) + gz*gz) per axis with
 * g = grad(k0) + grad(k1), (0, 0, 0) when the root is 0; it points to free space. */
int dpm_tsdf_surface(const void *map, int cap_vox, double voxel, int min_count, unsigned long long *keys, int32_t *axes,
                     float *xyz, float *normals, int32_t *count, int max_out, dpm_stream_t stream);
/* Marching tetrahedra, one lane per slot: triangles in no defined order, count / max_out as above.  The cell anchored at a
 * voxel's centre is meshed only when its 8 corner voxels (corner m = dx | dy << 1 | dz << 2) are qualified.  Its six
 * tetrahedra are the Kuhn decomposition round the diagonal 0 - 7, one per permutation (a, b, c) of the axes: corners 0,
 * 1 << a, 1 << a | 1 << b, 7; neighbouring cells then agree on every face diagonal.  An edge runs from a corner p to a corner q
 * containing p's bits; it carries a vertex when (Dp < 0) != (Dq < 0), named by vertex_keys = the key of p and vertex_dirs =
 * 0, 1, 2 for q ^ p = 1, 2, 4 (axes), 3, 4, 5 for 3, 5, 6 (face diagonals), 6 for 7 (the body diagonal), at p's centre with
 * f * voxel added on every axis of q ^ p, f = Dp / (Dp - Dq).  vertex_keys / vertex_dirs (max_out,3), xyz (max_out,3,3): a
 * triangle's three vertices, wound so that (b - a) x (c - a) points to the positive side (free space).  A corner with D == 0
 * counts as positive; the triangles of zero area it makes are kept. */
int dpm_tsdf_mesh(const void *map, int cap_vox, double voxel, int min_count, unsigned long long *vertex_keys,
                  int32_t *vertex_dirs, float *xyz, int32_t *count, int max_out, dpm_stream_t stream);
/* TILE-OWNED EXTRACTION.  tiles: n_tiles keys of tiles (ROLLING THE MAP above: pack_key(x >> b, y >> b, z >> b) of the biased
 * indices, b = tile_bits in [3, 10]) on the device, SORTED ascending and unique.  A record of dpm_tsdf_surface, or a cell of
 * dpm_tsdf_mesh, is OWNED when the tile of its voxel k0 (the crossing's lower voxel, the cell's corner 0) is in the list, found
 * by binary search; n_tiles = 0 (tiles may then be NULL, tile_bits is not looked at) owns everything.  What an owned record or
 * cell READS is not cut: the 8 corners and, for the normals, the neighbours at +-1 of both ends of an edge, which lie in
 * k0 + {-1, 0, 1, 2}^3, whatever tile holds them.
 *
 * dpm_tsdf_surface_tiles: dpm_tsdf_surface's records, bytes and count / max_out rule, of the owned k0 only.
 *
 * dpm_tsdf_mesh_indexed: the owned cells of dpm_tsdf_mesh -- the same cells, triangles, positions and winding -- as an INDEXED
 * mesh.  A vertex (key of p, direction) exists once: vertex_keys (max_v,) uint64, vertex_dirs (max_v,) int32, xyz (max_v,3) =
 * dpm_tsdf_mesh's position of that name, normals (max_v,3) = for the edge between voxels p and q the rule of dpm_tsdf_surface
 * with k0 = p, k1 = q: g = grad(p) + grad(q), divided per axis by sqrt((gx*gx + gy*gy) + gz*gz), (0, 0, 0) when the root is 0;
 * on the axis edges (direction 0, 1, 2) these are dpm_tsdf_surface's bytes for (key, axis).  faces (max_f,3) int32: a triangle's
 * three vertex indices in dpm_tsdf_mesh's winding.  counts (2,) int32 = V, F, ZEROED BY THE CALL; either may exceed its maximum:
 * then vertices at and past max_v and faces at and past max_f are not written (a written face may name an index >= max_v);
 * max_v = max_f = 0 only counts.  The vertices of a slot of the table are consecutive, directions ascending, and slots follow
 * each other in table order, so the order of vertices and faces depends on the order the voxels arrived in: sort by name for a
 * canonical form.  Six launches (clear; cells: ids (slot << 3 | direction) and a 7-bit mask per slot by 32-bit atomicOr; block
 * sums; their scan; vertices; remap), integer atomics only, no host synchronisation, capturable.
 * workspace: dpm_tsdf_mesh_indexed_bytes(cap_vox) bytes (0 for a cap_vox no table can have), any alignment. */
int dpm_tsdf_surface_tiles(const void *map, int cap_vox, double voxel, int min_count, int tile_bits,
                           const unsigned long long *tiles, int n_tiles, unsigned long long *keys, int32_t *axes, float *xyz,
                           float *normals, int32_t *count, int max_out, dpm_stream_t stream);
size_t dpm_tsdf_mesh_indexed_bytes(int cap_vox);
int dpm_tsdf_mesh_indexed(const void *map, int cap_vox, double voxel, int min_count, int tile_bits,
                          const unsigned long long *tiles, int n_tiles, unsigned long long *vertex_keys, int32_t *vertex_dirs,
                          float *xyz, float *normals, int32_t *faces, int32_t *counts, int max_v, int max_f, void *workspace,
                          dpm_stream_t stream);
/* THE FIELD AT A POINT, and registration against it.  Lookups only: the table is never written.  A row (x, y, z) of a frame
 * under `pose` is q = fma(R2, z, fma(R1, y, R0 * x)) + t in the map frame, as above.  In fp32, every operation rounded once, no
 * fused multiply-add, divisions correctly rounded, with v = (float)voxel; per axis a:
 *     g = q[a] / v - 0.5f,  fl = floorf(g);  the cell is VALID iff fl >= -1048576.f && fl < 1048575.f on every axis (fl and
 *     fl + 1 then fit the 21 bits; a NaN fails);  i0 = (int)fl + 1048576;  f = g - fl, in [0, 1] (1 only through the rounding
 *     of a tiny negative g, which is still valid).
 * D[dx][dy][dz] is the field of the voxel (i0x + dx, i0y + dy, i0z + dz).  The point HAS A VALUE iff the cell is valid and all 8
 * corner voxels are qualified (count >= min_count): a missing corner is never read as 0.  Then
 *     e[dy][dz] = D[1][dy][dz] - D[0][dy][dz];   c[dy][dz] = D[0][dy][dz] + fx * e[dy][dz];
 *     m[dz] = c[1][dz] - c[0][dz];               b[dz] = c[0][dz] + fy * m[dz];
 *     hz = b[1] - b[0];                          d = b[0] + fz * hz;
 *     hy = m[0] + fz * (m[1] - m[0]);
 *     t[dz] = e[0][dz] + fy * (e[1][dz] - e[0][dz]);   hx = t[0] + fz * (t[1] - t[0]);
 *     grad[a] = h[a] / v;                        n2 = (gx*gx + gy*gy) + gz*gz.
 * d is the trilinear interpolant of D between the 8 voxel centres and grad its exact gradient inside the cell, in the map
 * frame's axes.
 *
 * dpm_tsdf_sample: one lane per row, one launch, capturable.  xyz (cap,3) fp32, count (1,) int32 and pose (16 doubles) on the
 * device; n = count clamped to [0, cap].  Rows below n: flag 1 with d and grad (cap,3), or flag 0 and zeros where the point has
 * no value; rows in [n, cap): flag -1 and zeros (their xyz is not read).  cap = 0 is a no-op. */
int dpm_tsdf_sample(const void *map, int cap_vox, double voxel, const double *origin, const float *xyz, const int32_t *count,
                    int cap, const double *pose, int min_count, float *d, float *grad, int32_t *flag, dpm_stream_t stream);
/* dpm_tsdf_register: Gauss-Newton on the sum of D(T p)^2 over the frame's first count rows, from init_pose (device), with the
 * schedule, the robust weight, the 29 fp64 sums, the solve, the stop rule, the DPM_ICP_* statuses and the launch shape of
 * dpm_local_map_register: an init launch, a launch per later stage, and per iteration one accumulate launch (one lane per row)
 * and one one-wave solve launch; no host synchronisation, capturable.  Every stage_max_dist must lie in (0, truncation], the
 * map's truncation (beyond the clamp the field is flat); grad_min >= 0.  A row is given when the point has a value and
 *     fabsf(d) <= (float)max_dist,   n2 >= (float)(grad_min * grad_min),   n2 finite        (a NaN fails by comparison).
 * It enters in fp64: p = (double)q, g = (double)grad, e = (double)d, J = (p x g, g) in DPM_ICP_PLANE's component order, weighted
 * w = (k / (k + e*e))^2 with k = kernel_scale^2 (0: w = 1); the count and the squared residuals are not weighted.  The gradient
 * is not normalised: grad_min keeps the flat, clamped parts of the field out.  The sums are fp64 partials added in a fixed
 * order (lanes, waves, blocks): no floating-point atomics, identical bytes on every run.  The step acts on the map-frame pose;
 * NO_MATCH (also: empty map, count 0) and SINGULAR leave the pose's bytes where they were; fitness = rows / n.  pose (16),
 * fitness, rmse, iterations, status: one value each, on the device.  Optional: debug_flag (cap,) int32 at the last evaluated
 * pose -- 1 the row was given, 0 it was not, -1 past the count -- and debug_system (29).
 * workspace: dpm_tsdf_register_scratch_bytes(cap) bytes (0 for cap < 1), any alignment. */
size_t dpm_tsdf_register_scratch_bytes(int cap);
int dpm_tsdf_register(const void *map, int cap_vox, double voxel, const double *origin, double truncation, int min_count,
                      double grad_min, const float *xyz, const int32_t *count, int cap, const double *init_pose,
                      const double *stage_max_dist, const int32_t *stage_max_iter, int n_stages, double kernel_scale,
                      double tol_rot, double tol_trans, double *pose, float *fitness, float *rmse, int32_t *iterations,
                      int32_t *status, int32_t *debug_flag, double *debug_system, void *workspace, dpm_stream_t stream);
/* RAY-CASTING THE FIELD: what a sensor at a pose would see in the map.  Lookups only; one launch for any F (grid y = pose), no
 * host synchronisation, capturable.  poses (F,16) fp64 and dirs (R,3) fp32 on the device; dirs are in the SENSOR frame, unit
 * length expected and not renormalised.  range (F,R) fp32, normals (F,R,3) fp32, flag (F,R) int32.  F in [0, 65535]; F = 0 or
 * R = 0 is a no-op.  In fp32, every operation rounded once, no fused multiply-add outside u's chain, divisions and square roots
 * correctly rounded, with P the pose as above ((float)R and o = (float)(t - origin)):
 *     u[a] = fma(R[a][2], dz, fma(R[a][1], dy, R[a][0] * dx))        (the point's chain without the translation);
 *     h = (float)step,  t0 = (float)min_range,  K = floor((max_range - min_range) / step) + 1 on the host in double;
 *     sample k = 0 .. K-1:  t_k = t0 + (float)k * h,  p_k[a] = o[a] + u[a] * t_k;  its value d_k and gradient g_k are those of
 *     THE FIELD AT A POINT above at p_k: a sample HAS A VALUE only when its cell is valid and all 8 corners are qualified.
 * With s(d) = d > 0 the ray ENDS at the smallest k >= 1 for which samples k-1 and k both have a value and s(d_{k-1}) != s(d_k); a
 * sample without a value between two signs is no crossing.  flag = 1 (HIT) when s(d_{k-1}): from free space into the surface;
 * flag = 2 (BACK) otherwise: out of the back of a surface.  In both cases
 *     f = d_{k-1} / (d_{k-1} - d_k),   range = t_{k-1} + f * h,   g[a] = g_{k-1}[a] + f * (g_k[a] - g_{k-1}[a]),
 *     len = sqrt((gx*gx + gy*gy) + gz*gz),   m[a] = g[a] / len   (zeros unless len > 0 and finite),
 *     normal[j] = (R[0][j] * m[0] + R[1][j] * m[1]) + R[2][j] * m[2]:
 * the unit gradient turned back into the SENSOR frame (the frame dpm_tsdf_integrate_planes takes normals in), pointing to the
 * field's positive side.  No crossing within the K samples: flag = 0 (MISS), range and normal zeros.  A NaN or zero direction,
 * and a ray that leaves the 21 bits, never get a value: MISS.  An empty table gives MISS everywhere.
 * DPM_EINVAL: step <= 0, min_range < 0, max_range < min_range, K > 65536, min_count < 1.
 *
 * blocks: NULL (the plain form: the 8 lookups of every sample), or an occupied-block set built by dpm_tsdf_blocks FROM THIS
 * TABLE AS IT IS NOW AND WITH THIS min_count.  The set holds the keys (x >> 3, y >> 3, z >> 3) (3 x 18 bits, packed as a voxel
 * key) of the 8 x 8 x 8 blocks that hold a qualified voxel: dpm_tsdf_blocks_bytes(cap_blocks) = 256 + 8 cap_blocks bytes, 16-byte
 * aligned, cap_blocks a power of two in [2, 2^24]: a 256-byte header (word 0: claims that found no room; the set is defined
 * only while it is zero) and an open-addressing set with the table's hash and probing.  dpm_tsdf_blocks clears it and claims,
 * one lane per slot of the table (two launches, capturable, integer compare-and-swap only): membership is a function of the
 * table's content and min_count alone.  A sample whose base voxel i0 lies in a block the set does not hold cannot have a value
 * (its corner (0,0,0) is not qualified), so the marcher skips its 8 lookups; every sample is still formed, none is stepped
 * over, and the outputs equal those of the plain form byte for byte. */
size_t dpm_tsdf_blocks_bytes(int cap_blocks);
int dpm_tsdf_blocks(const void *map, int cap_vox, int min_count, void *blocks, int cap_blocks, dpm_stream_t stream);
int dpm_tsdf_raycast(const void *map, int cap_vox, double voxel, const double *origin, const void *blocks, int cap_blocks,
                     const double *poses, int F, const float *dirs, int R, double min_range, double max_range, double step,
                     int min_count, float *range, float *normals, int32_t *flag, dpm_stream_t stream);

/* ---------------------------------------------------------------- geometric loop closure ---- */

/* Scan Context place descriptors (Kim & Kim, IROS 2018) and the exhaustive search over a database of them
 * (csrc/scan_context.hip; deeppointmap_amd/loop_closure.py is the caller).  No counterpart in the reference, which
 * recognises places with its learned loop head only.  DESIGN §7k is the definition; in short:
 *
 * A descriptor is a polar grid of rings (1..32) x sectors (even, 4..64) cells; three outputs per frame: raw heights
 * (rings, sectors) fp32, column-normalised heights (rings, sectors) fp32 and a 64-bit column occupancy mask.  Tables ON THE
 * HOST, read before the launch: ring_e2 (rings,) fp32 = e_1 .. e_rings, the squared ring edges (float)((m max_range /
 * rings)^2); sector_cs (sectors/2 - 1, 2) fp32 = (cos, sin) of 2 pi m / sectors, m = 1 .. sectors/2 - 1.  A row of xyz with
 * a non-finite coordinate or r2 = x*x + y*y == 0 is skipped; it counts iff (float)(min_range^2) <= r2 < e_rings; its ring is
 * the number of m in 1..rings-1 with r2 >= e_m; half = 0 if y > 0 || (y == 0 && x > 0), else 1 and (x, y) is negated; its
 * sector is half * sectors/2 + the number of m with cos_m * y - sin_m * x >= 0.  h = z + (float)z_offset counts when > 0 and
 * the cell keeps the greatest h (integer atomicMax on its bits); an empty cell is 0.  Per column j: n2 = sum_r h*h (r
 * ascending, sequential fp32), norm = sqrtf(n2), normalised = h / norm where norm > 0 else 0, mask bit j = norm > 0.
 * Three launches (clear, bin, finish), no host synchronisation, capturable; the same bytes whatever the order of the rows.
 * DPM_EINVAL: rings / sectors outside their limits, min_range > max_range. */
/* one frame: xyz (cap,3) fp32 row-major, count (1,) int32 on the device (rows at and past it are never read); raw / norm /
 * mask point at the frame's row of the database tensors */
int dpm_scan_context_build(const float *xyz, const int32_t *count, int cap, int rings, int sectors, double max_range,
                           double min_range, double z_offset, const float *ring_e2, const float *sector_cs, float *raw,
                           float *norm, unsigned long long *mask, dpm_stream_t stream);
/* F <= 65535 frames: pcd (F,3,N) fp32 channel-first, lengths (F,) int32 valid leading points; raw / norm (F,rings,sectors),
 * mask (F,) */
int dpm_scan_context_build_batched(const float *pcd, const int32_t *lengths, int F, int N, int rings, int sectors,
                                   double max_range, double min_range, double z_offset, const float *ring_e2,
                                   const float *sector_cs, float *raw, float *norm, unsigned long long *mask,
                                   dpm_stream_t stream);
/* Query q (Q <= 65535; normalised descriptors q_norm (Q,rings,sectors) and masks q_mask (Q,)) against rows
 * 0 .. limit[q]-1 of the database (db_norm (D,rings,sectors), db_mask (D,); limit (Q,) int32 on the device, clamped to
 * [0, D]).  For a pair and a shift s in 0..sectors-1: used(s) = popcount_j(mq[j] & mc[(j+s) % sectors]), S(s) = sum_j
 * <Aq[:,j], Ac[:,(j+s) % sectors]> (the dot product a ring-ascending fp32 fma chain, the sum j ascending), d(s) = used ?
 * max(1 - S / used, 0) : 1.  The pair's result is its smallest key (bits of d, s); the query's result the K (1..8) smallest
 * keys (bits of d, row), ascending: dist (Q,K) fp32, row (Q,K) int32, shift (Q,K) int32, padded with (inf, -1, -1).  Query
 * column j matches candidate column j + s: the query frame's yaw in the candidate's frame is s * 2 pi / sectors.  Exact
 * selection, fixed summation orders, no atomics: the same bytes on every run.  Two launches, no host synchronisation;
 * nothing of size (Q, D) is stored: workspace holds one K-list per block of database rows. */
size_t dpm_scan_context_search_workspace_bytes(int Q, int D, int K);
int dpm_scan_context_search(const float *q_norm, const unsigned long long *q_mask, int Q, const float *db_norm,
                            const unsigned long long *db_mask, int D, const int32_t *limit, int rings, int sectors, int K,
                            float *dist, int32_t *row, int32_t *shift, void *workspace, dpm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DPM_HIP_H */
