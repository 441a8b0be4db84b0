/* librapflow -- C ABI of the MI355X-native rectified-flow registration sampler.
 *
 * Drop-in boundary for ONE hot path of PRBonn/RAP: rectified_point_flow/{sampler.py, flow_model/,
 * procrustes.py} behind RectifiedPointFlow.sample_rectified_flow (reference modeling.py:632-741).
 * The reference has no native code; its "FFI" for this path is the set of Python call sites listed
 * next to each entry point below.  INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * Conventions (all entry points):
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer (HIP, gfx950) unless named h_*;
 *   - fp32 tensors are dense row-major; packed varlen layout (TP,C) with segment tables, exactly the
 *     reference's collate schema (data/datamodule.py:169-198);
 *   - `stream` is a hipStream_t passed as void*; work is enqueued, the call never synchronises and never
 *     allocates (except rap_model_create / rap_model_destroy);
 *   - returns 0 (RAP_OK) or a negative code: -1 invalid argument, -2 workspace too small,
 *     -3 HIP runtime error (see rap_last_hip_error), -4 allocation failure;
 *   - the caller owns every buffer, including the workspace (size from rap_workspace_bytes).
 */
#ifndef RAPFLOW_H
#define RAPFLOW_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version of this header.  rap_version() returns the value the LIBRARY was built with; a caller compiled against another
 * value must not use the library (round 4, version 4: rap_spinnet_describe gained `flags` and three entry points were removed in
 * round 3 without a bump; the fp16-residual epilogue of rap_gemm_h16 moved from 6 to 7 and 6 is refused; rap_poison_on_flag is new;
 * round 5, version 5: compute dtype 3 (split precision) and the rap_x2_* entry points are new, nothing was removed or re-numbered;
 * round 6, version 6: additive -- the *_latent entry points (in_dim > 0), rap_transform_errors, tuning keys 18 / 19 / 20; the scratch of the
 * kernel-level attention entry points grew by a sanitised copy of cu_seqlens (rap_attention_workspace_bytes reports it)).  Still version
 * 6, additive: rap_pair_metrics_workspace_bytes, rap_pair_metrics and rap_transform_errors_direct (the evaluator's metrics table);
 * rap_icp_workspace_bytes and rap_icp (batched ICP); rap_icp_grid_workspace_bytes, rap_icp_grid, rap_nn_grid_workspace_bytes and
 * rap_nearest_neighbors (the same search over a uniform-grid index); rap_attention_split_workspace_bytes, rap_attention_f32_split and
 * rap_x2_attention_split (kernel-level access to the split-KV attention of few-token calls); rap_gemm_f32_form and rap_gemm_h16_form (the
 * GEMM dispatch decision as host arithmetic), rap_call_plan (every shape-dependent decision of a model call, likewise), rap_gemm_f32_splitk_workspace_bytes and rap_gemm_f32_splitk (kernel-level access to the
 * split-K form of the fp32 residual and SiLU GEMMs of few-token calls); rap_normals_workspace_bytes, rap_estimate_normals,
 * rap_icp_plane_workspace_bytes, rap_icp_plane, rap_icp_plane_grid_workspace_bytes and rap_icp_plane_grid (point-to-plane ICP and the
 * normals it needs); rap_deskew, rap_fuse_frames, rap_submap_overlap with their *_workspace_bytes queries and
 * rap_submap_groups_connected (sweeps and poses -> submaps, their overlap matrix and the connectivity of candidate groups);
 * rap_part_acc_workspace_bytes and rap_part_acc (part accuracy and the part matching that matched_part_ids arguments take);
 * rap_knn_workspace_bytes, rap_k_nearest_neighbors, rap_normals_grid_workspace_bytes, rap_estimate_normals_grid,
 * rap_outlier_grid_workspace_bytes and rap_statistical_outliers_grid (the k nearest rows over the uniform-grid index, and the normal
 * estimation and the outlier removal on it); rap_fps_grid_workspace_bytes, rap_farthest_point_sampling_grid and rap_fps_grid_params
 * (farthest point sampling over a bucket index: the index lists of rap_farthest_point_sampling, less work per pick);
 * rap_orient_normals_workspace_bytes and rap_orient_normals (a consistent orientation of existing normals over the minimum spanning
 * forest of the k-NN graph); rap_scene_refine_workspace_bytes and rap_scene_refine (joint multi-view point-to-plane refinement of the
 * poses of a registered scene); rap_icp_plane_robust, rap_icp_plane_grid_robust and rap_scene_refine_robust with their
 * *_workspace_bytes queries, and the RAP_LOSS_* codes (the point-to-plane estimators under a robust loss). */
#define RAPFLOW_ABI_VERSION 6

/* return codes of every int-returning entry point */
#define RAP_OK 0
#define RAP_ERR_INVALID (-1)
#define RAP_ERR_WORKSPACE (-2)
#define RAP_ERR_HIP (-3)
#define RAP_ERR_ALLOC (-4)

typedef struct rap_model rap_model;

/* PointCloudDiT hyper-parameters (reference config/model/flow_model/point_cloud_dit_12.yaml,
 * flow_model/point_cloud_dit.py:20-36).  head_dim is fixed at 64 (embed_dim == 64 * num_heads),
 * embed_dim a multiple of 256, local_feat_dim a multiple of 4 and <= 40, in_dim == 0.  The native embedding layout is the one of
 * scale_emb_on == local_feat_concat_on == true (config/RAP_inference.yaml:65); a model built with either switch off maps onto it with
 * zero weight columns / unit gains (rap_amd/flow_model.py _native_tensors), qk_norm == false through rap_model_set_qk_norm. */
typedef struct rap_model_desc {
  int32_t embed_dim;      /* 512 */
  int32_t num_layers;     /* 10 / 12 / 16 */
  int32_t num_heads;      /* 8 */
  int32_t local_feat_dim; /* 32 */
} rap_model_desc;

int rap_version(void);
int rap_last_hip_error(void);

/* Number of fp32 values in the raw weight blob: the tensors of PointCloudDiT.state_dict() concatenated
 * in the reference's registration order (flow_model/point_cloud_dit.py:83-117, layer.py:71-89,
 * norm.py:47-58; table in DESIGN.md "Weight contract").  Returns < 0 for an unsupported desc. */
int64_t rap_weight_count(const rap_model_desc* desc);

/* Replaces  PointCloudDiT(...).load_state_dict(ckpt)  (reference sample.py:58, utils/checkpoint.py:13-61).
 * Copies the blob into model-owned device memory and builds the kernel-side packings (split embedding
 * projection, stacked adaLN weights, value/gate-interleaved GEGLU projection).  Allocates. */
int rap_model_create(const rap_model_desc* desc, const float* d_weights, int64_t n_floats, void* stream,
                     rap_model** out);
/* in_dim > 0 (round 6; reference flow_model/embedding.py:107-118,163-166, point_cloud_dit.py:56,86): the model concatenates `in_dim`
 * LATENT point features (the PTv3 encoder output of encoder_on = true; modeling.py:788 builds one with in_dim = 64) into the embedding
 * input.  They are step-invariant like the condition cloud, so they become in_dim more columns of the hoisted embedding GEMM.  The blob's
 * emb_proj.weight is (embed_dim, 147 + local_feat_dim + in_dim) with the latent columns LAST ([cond 63 | x_t 63 | scale 21 | feat F |
 * latent in_dim]; rap_amd/flow_model.py re-orders the reference's [cond | x_t | latent | scale | feat]).  in_dim a multiple of 4, <= 512.
 * in_dim = 0 is rap_weight_count / rap_model_create.  A model with in_dim > 0 must be driven through the *_latent entry points below. */
int64_t rap_weight_count_latent(const rap_model_desc* desc, int32_t in_dim);
int rap_model_create_latent(const rap_model_desc* desc, int32_t in_dim, const float* d_weights, int64_t n_floats, void* stream,
                            rap_model** out);
void rap_model_destroy(rap_model* m);

/* Arithmetic type of the transformer blocks (qkv / out / feed-forward GEMMs and attention) for subsequent calls on `m`:
 * 0 = fp32 (default; exact-fp32 MFMA, the parity configuration of BASELINE configs[1]),
 * 1 = bf16 MFMA (BASELINE configs[2], [4]), 2 = fp16 MFMA,
 * 3 = SPLIT PRECISION ("float32x2", round 5): fp32-ACCURATE results from the fp16 matrix pipe.  Every operand of the block GEMMs and of
 *     both attention products is carried as an fp16 head + an fp16 tail (x = hi + lo, 22 significand bits; weights additionally scaled by
 *     a per-tensor power of two so that their tails are normal numbers) and each contraction keeps hi*hi + hi*lo + lo*hi in the MFMA's
 *     fp32 accumulators -- 3 x 32 matrix-pipe cycles per 16 contraction steps instead of 8 x 64 for the fp32-input MFMA.  Residual stream,
 *     LayerNorm, qk-norm, softmax state, GEGLU, embedding, head, Euler and Procrustes are fp32 exactly as in mode 0; results sit at
 *     mode 0's distance from an fp64 evaluation.  Operands are clipped to the fp16 range (|x| <= 65504), the range
 *     of the reference's own shipped fp16 inference.  The residual-dtype switch below is ignored in this mode.
 * Modes 1 / 2 replace the autocast context the reference runs its
 * GPU inference under (Lightning precision "16-mixed", config/trainer/infer.yaml:6; attn_dtype, layer.py:106-128).
 * Residual stream, LayerNorm, softmax, accumulation, embedding, final_mlp, Euler and Procrustes stay fp32
 * (final_mlp is fp32 in the reference too, point_cloud_dit.py:183-184).  The first call per dtype allocates and
 * fills the 16-bit weight copies.  rap_workspace_bytes depends on the current dtype. */
int rap_model_set_compute_dtype(rap_model* m, int32_t dtype, void* stream);
int rap_model_compute_dtype(const rap_model* m);
/* How many of the model's 2 * num_layers attention launches (layer x {per part, per sample}) take the bounded, offset-free softmax
 * kernel: a launch does when every head of THAT attention has 8 max|gamma_q| max|gamma_k| <= 40 (MultiHeadRMSNorm gains,
 * flow_model/norm.py:15-33); the others take the online-softmax kernel.  Decided per launch, so one hot head of a trained checkpoint
 * costs one (layer, branch) the faster kernel, not the model.  Returns < 0 for a NULL model. */
int rap_model_bounded_attention_launches(const rap_model* m);
/* qk_norm of the reference's constructor (flow_model/point_cloud_dit.py:28; layer.py:75-83,103-104): 1 (default, every shipped configuration) =
 * MultiHeadRMSNorm on q and k; 0 = q and k go to the attention as projected -- no bound on the logits exists then, every attention launch
 * takes the online-softmax kernel, and the gamma entries of the weight blob are ignored.  (The reference's other two constructor switches,
 * scale_emb_on / local_feat_concat_on, only narrow the embedding projection's input: a caller widens emb_proj.weight with zero columns for
 * the absent inputs -- rap_amd.PointCloudDiT does -- which is exact.) */
int rap_model_set_qk_norm(rap_model* m, int32_t on);
int rap_model_qk_norm(const rap_model* m);
/* softcap of the reference's constructor (flow_model/point_cloud_dit.py:27; layer.py:33,64,106-128 hand it to flash-attn): with
 * c > 0 every attention logit s = q.k / sqrt(64) becomes c * tanh(s / c) before the softmax; 0 (default) = off.  A finite c > 0 is accepted,
 * anything else is RAP_ERR_INVALID.  A capped model runs ONE attention plan whatever the call's size: the soft-capped online-softmax kernels,
 * unsplit, on 256-row work items (no bounded softmax: rap_model_bounded_attention_launches is 0 while a cap is set; no key ranges, no key
 * groups).  Not a per-call switch: set it before the first call, like qk_norm.  rap_model_softcap returns the cap (< 0 for a NULL model). */
int rap_model_set_softcap(rap_model* m, float c);
float rap_model_softcap(const rap_model* m);
/* final_mlp_act of the reference's constructor (point_cloud_dit.py:30,111-117): the activation behind the two hidden layers of the head
 * (fp32 in every compute mode).  0 = SiLU (default), 1 = GELU (erf, nn.GELU()'s default), 2 = ReLU; anything else is RAP_ERR_INVALID.  The
 * non-SiLU heads never split K (the split-K form of few-token calls is SiLU's). */
int rap_model_set_final_act(rap_model* m, int32_t act);
int rap_model_final_act(const rap_model* m);
/* Storage type of the residual stream in the 16-bit compute modes: 0 = fp32 (default), 2 = fp16.  With fp16 the stream between the
 * layer kernels is held the way the reference's own "16-mixed" inference holds it (nn.Linear outputs are 16-bit under autocast and
 * flow_model/layer.py:155-164 adds them): every residual sum is formed in fp32 from the GEMM's fp32 accumulators and rounded once,
 * LayerNorm statistics stay fp32, the head (fp32 in the reference too, point_cloud_dit.py:183-184) reads an fp32 image of it.
 * Halves the HBM bytes of the two N = 512 GEMMs and the three LayerNorms of a layer.  Ignored while the compute dtype is fp32.
 * rap_workspace_bytes depends on it.  Not a per-call switch: set it before the first call like the compute dtype. */
int rap_model_set_residual_dtype(rap_model* m, int32_t dtype);
int rap_model_residual_dtype(const rap_model* m);

/* Bytes of caller-provided workspace for one call on a batch of TP points, B samples, `nseg_part`
 * part segments (B*P for rap_sample, VP for rap_dit_forward) and `rows` adaLN rows
 * (num_steps for rap_sample, B for rap_dit_forward).  Depends on the model's compute / residual dtype (query it in the state the call
 * will run in; the setters and the enqueueing entry points serialise on a per-model mutex) and on nothing else: token-row buffers are
 * carved at align_up(TP, 256) rows (the layer kernels run over the padded rows, so any TP takes the persistent 256-row-tile GEMMs),
 * and the split-K planes of few-token 16-bit calls are reserved by shape, whatever tuning key 6 says.  A call whose workspace is too
 * small returns -2, it never overruns. */
size_t rap_workspace_bytes(const rap_model* m, int64_t TP, int32_t B, int32_t nseg_part, int32_t rows);

/* Replaces PointCloudDiT.forward (reference flow_model/point_cloud_dit.py:141-191), called from
 * modeling.py:684-706.  x_t (TP,3), timesteps (B,) raw t in (0,1], cond (TP,3), feat (TP,F), scales (B,),
 * anchor (TP,) uint8/bool, cu_batch (B+1,) int32, cu_part (VP+1,) int32 (zero-length segments allowed).
 * v_out (TP,3); feats_out (TP,embed_dim) or NULL ('transformer_features', :186-190). */
int rap_dit_forward(const rap_model* m, const float* x_t, const float* timesteps, const float* cond, const float* feat,
                    const float* scales, const uint8_t* anchor, const int32_t* cu_batch, const int32_t* cu_part,
                    int32_t B, int32_t VP, int64_t TP, float* v_out, float* feats_out, void* ws, size_t ws_bytes,
                    void* stream);
/* ... with latent (TP, in_dim) fp32 for a model created with in_dim > 0 (`latent_features` of point_cloud_dit.py:146, embedding.py:163-166);
 * latent must be NULL exactly when the model's in_dim is 0. */
int rap_dit_forward_latent(const rap_model* m, const float* x_t, const float* timesteps, const float* cond, const float* feat,
                           const float* latent, const float* scales, const uint8_t* anchor, const int32_t* cu_batch, const int32_t* cu_part,
                           int32_t B, int32_t VP, int64_t TP, float* v_out, float* feats_out, void* ws, size_t ws_bytes,
                           void* stream);

/* Replaces euler_step's tensor update (reference sampler.py:88-90): x0_hat = x_t - v*t ; x_next = x_t - dt*v.
 * n = number of floats (3*TP).  x_next may alias x_t.  traj_xt_slot may be NULL. */
int rap_euler_step(const float* x_t, const float* v, float t, float dt, float* x0_hat, float* x_next,
                   float* traj_xt_slot, int64_t n, void* stream);

/* Replaces fit_transformations (reference procrustes.py:40-84).  points_per_part (B,P) int64 as in the
 * reference; src/tgt (TP,3) packed in (b,p) order.  R_out (B,P,3,3), t_out (B,P,3); empty parts -> zero rows.
 * Convention: tgt ~= src @ R^T + t.  ws >= rap_procrustes_workspace_bytes(B*P). */
size_t rap_procrustes_workspace_bytes(int32_t nparts);
int rap_fit_transformations(const float* src, const float* tgt, const int64_t* points_per_part, int32_t B, int32_t P,
                            float* R_out, float* t_out, void* ws, size_t ws_bytes, void* stream);

/* Replaces rigidify_prediction_with_procrustes (reference procrustes.py:86-118): out = cond_p R_p^T + t_p. */
int rap_rigidify(const float* prediction, const float* condition, const int64_t* points_per_part, int32_t B, int32_t P,
                 float* out, void* ws, size_t ws_bytes, void* stream);

/* The sampler's rigidity-forcing update (reference sampler.py:59-60):
 *   x_t = rigidify(x0_hat, cond) * w0 + x_1 * w1   with w0 = 1 - t + dt, w1 = t - dt (computed in double by the caller). */
int rap_rigidify_blend(const float* x0_hat, const float* condition, const int64_t* points_per_part, int32_t B, int32_t P,
                       const float* x_1, float w0, float w1, float* x_t_out, void* ws, size_t ws_bytes, void* stream);

/* Replaces the whole of sample_rectified_flow + the final fit_transformations
 * (reference modeling.py:632-741 -> sampler.py:11-74 [euler] -> modeling.py:389-391):
 *   dt = 1/num_steps; x_t = x_1; for s: t = 1 - s*dt; v = DiT(x_t, t); x0 = x_t - v t; x_t -= dt v;
 *   if rigidity: x_t = rigid(x0, cond) (1-t+dt) + x_1 (t-dt);  traj_x0[s] = x0 (raw);  traj_xt[s] = x_t;
 *   R,t = fit_transformations(cond, traj_x0[S-1]).
 * traj_x0, traj_xt (num_steps,TP,3); R_out (B,P,3,3); t_out (B,P,3); feats_out (TP,embed_dim) or NULL
 * (transformer features of the last step, modeling.py:678-695). */
int rap_sample(const rap_model* m, const float* cond, const float* feat, const float* scales, const uint8_t* anchor,
               const int64_t* points_per_part, const int32_t* cu_batch, const float* x_1, int32_t B, int32_t P,
               int64_t TP, int32_t num_steps, int32_t rigidity_forcing, float* traj_x0, float* traj_xt, float* R_out,
               float* t_out, float* feats_out, void* ws, size_t ws_bytes, void* stream);
/* ... with the `latent_features` argument of sample_rectified_flow (modeling.py:636): (TP, in_dim) fp32, NULL exactly when in_dim is 0 */
int rap_sample_latent(const rap_model* m, const float* cond, const float* feat, const float* latent, const float* scales,
                      const uint8_t* anchor, const int64_t* points_per_part, const int32_t* cu_batch, const float* x_1, int32_t B,
                      int32_t P, int64_t TP, int32_t num_steps, int32_t rigidity_forcing, float* traj_x0, float* traj_xt, float* R_out,
                      float* t_out, float* feats_out, void* ws, size_t ws_bytes, void* stream);

/* ---- generation selection by rigidity (the caller side of the path) ----
 * Replaces compute_rigidity_rmse (reference eval/metrics.py:511-622): per sample, the RMS of |cond_p R_p^T + t_p - pred_p|
 * over the points of all non-empty parts (average_per_part: mean over parts of the per-part RMS), inf for a sample
 * without points, times scales[b] if scales != NULL.  out (B,).  ws >= rap_rigidity_workspace_bytes(B*P, steps, B). */
size_t rap_rigidity_workspace_bytes(int32_t nparts, int32_t steps, int32_t B);
int rap_rigidity_rmse(const float* cond, const float* pred, const float* R, const float* t, const int64_t* points_per_part,
                      int32_t B, int32_t P, const float* scales, int32_t average_per_part, float* out, void* ws,
                      size_t ws_bytes, void* stream);
/* Replaces the use_average_rigidity_rmse loop of test_step (reference modeling.py:466-500): for every step of the
 * end-point trajectory traj (steps,TP,3): R,t = fit_transformations(cond, traj[s]); rmse[s] = rigidity RMSE; mean_out (B,) =
 * mean over steps.  per_step_out (steps,B) or NULL. */
int rap_trajectory_rigidity_rmse(const float* cond, const float* traj, const int64_t* points_per_part, int32_t B, int32_t P,
                                 int64_t TP, int32_t steps, const float* scales, float* mean_out, float* per_step_out, void* ws,
                                 size_t ws_bytes, void* stream);
/* Replaces the rigidity-selected generation pick (reference modeling.py:518, 560-592): best_out[b] = argmin_g rmse[g][b]
 * (first minimum), or with pick_largest != 0 the overlap-ratio pick argmax_g (modeling.py:601); if clouds != NULL also gathers cloud_out (TP,3), R_out (B,P,3,3), t_out (B,P,3) of the picked generation
 * per sample from clouds (G,TP,3), R (G,B,P,3,3), t (G,B,P,3); cu_batch (B+1,) int32. */
int rap_select_generation(const float* rmse, int32_t G, int32_t B, int32_t P, int64_t TP, const int32_t* cu_batch,
                          const float* clouds, const float* R, const float* t, int32_t pick_largest, int32_t* best_out,
                          float* cloud_out, float* R_out, float* t_out, void* stream);
/* ---- registration errors (the RRE / RTE that BASELINE.json's "SE(3) err" is defined by) ----
 * Replaces compute_transform_errors(..., use_icp=False) (reference eval/metrics.py:165-303): per sample, every non-anchor, non-empty part's
 * ground-truth and predicted pose relative to the (first) anchor part's, delta_R = R_gt_rel^T R_pred_rel, delta_t = (t_pred_rel -
 * t_gt_rel) * scale[b];  rot_err = deg(acos(clamp((tr delta_R - 1) / 2, -1, 1))), trans_err = |delta_t|.  R_* (B,P,3,3), t_* (B,P,3),
 * points_per_part (B,P) int64, anchor_part (B,P) uint8, matched_part_ids (B,P) int64 or NULL (re-orders the PREDICTED poses, :223-227),
 * scale (B,) or NULL (= 1).  Outputs: per-part errors (B,P) (0 for anchor / empty parts) and their means over the valid parts (B,)
 * (NaN for a sample without one, as the reference's 0 / 0).  No workspace, no synchronisation. */
int rap_transform_errors(const float* R_gt, const float* t_gt, const float* R_pred, const float* t_pred, const int64_t* points_per_part,
                         const uint8_t* anchor_part, const int64_t* matched_part_ids, const float* scale, int32_t B, int32_t P,
                         float* rot_err_per_part, float* trans_err_per_part, float* rot_err_mean, float* trans_err_mean, void* stream);

/* Replaces compute_overlap_ratio (reference eval/metrics.py:625-691): per sample the fraction of points that have a point of
 * a DIFFERENT part of the same sample within distance tau, for n_taus (<= 8) thresholds given as a HOST array.
 * ratios_out (n_taus, B) device; min_dist_out (TP,) device or NULL (distance to the nearest other-part point, inf if none).
 * 0 for samples with <= 1 point or fewer than two non-empty parts.  ws >= rap_overlap_workspace_bytes(TP, B, P). */
size_t rap_overlap_workspace_bytes(int64_t TP, int32_t B, int32_t P);
int rap_overlap_ratio(const float* pointclouds_pred, const int64_t* points_per_part, const int32_t* cu_batch, int32_t B, int32_t P,
                      int64_t TP, const float* h_taus, int32_t n_taus, float* ratios_out, float* min_dist_out, void* ws,
                      size_t ws_bytes, void* stream);

/* ---- output transforms (the data format after the path) ----
 * Replaces the 4x4 computation of Evaluator._save_transformation_files (reference eval/evaluator.py:383-490): per (sample,
 * part) the predicted pose relative to the ground-truth pose in metres, R_rel = R_pred R_gt^T, t_rel = s t_pred -
 * (s t_gt) R_rel^T, times inv([R_global | t_global]) when the per-sample global frame (B,3,3)/(B,3) is given.
 * out (B,P,4,4) row-major fp32; all-zero blocks for parts without points. */
int rap_relative_transforms(const float* R_pred, const float* t_pred, const float* R_gt, const float* t_gt, const float* scales,
                            const int64_t* points_per_part, int32_t B, int32_t P, const float* global_rotation,
                            const float* global_translation, float* out, void* stream);

/* Nearest-neighbour metrics of the same evaluator.  ws >= rap_nn_metrics_workspace_bytes(points, B).
 * rap_chamfer_rmse replaces compute_cd (reference eval/metrics.py:14-48): per object sqrt(0.5 (mean_i min_j |gt_i - pred_j|^2 +
 * mean_j min_i |pred_j - gt_i|^2)); gt, pred (TP,3) packed by cu_batch (B+1,) int32; out (B,).
 * rap_correspondence_rmse replaces compute_correspondence_rmse (:386-469) for ONE scan pair: nearest target_gt point of every
 * source_gt point; pairs within distance_threshold are correspondences; out3 = {RMS of |source_pred_i - target_pred_nn(i)| over
 * them (inf if none), their number, number / n_source} (device, 3 floats). */
size_t rap_nn_metrics_workspace_bytes(int64_t n_points, int32_t B);
int rap_chamfer_rmse(const float* pointclouds_gt, const float* pointclouds_pred, const int32_t* cu_batch, int32_t B, int64_t TP,
                     float* out, void* ws, size_t ws_bytes, void* stream);
int rap_correspondence_rmse(const float* source_gt, const float* target_gt, const float* source_pred, const float* target_pred,
                            int32_t n_source, int32_t n_target, float distance_threshold, float* out3, void* ws, size_t ws_bytes,
                            void* stream);

/* Replaces compute_part_acc (reference eval/metrics.py:92-163) for a whole packed batch, without a host round trip.
 * gt, pred (TP,3) packed by cu_batch (B+1,) int32 and points_per_part (B,P) int64 -- rap_overlap_ratio's layout; P <= 256.
 *   cd[b,i,j] = mean_{x in gt_i} min_{y in pred_j} |x-y|^2 + mean_{y in pred_j} min_{x in gt_i} |x-y|^2   (no root, no 1/2)
 * cd_out (B,P,P) fp32 or NULL, indexed by part SLOT, NaN where either part is empty.
 * cost = (cd >= threshold) over the non-empty parts of a sample (n of them) is assigned as scipy.optimize.linear_sum_assignment
 * assigns it -- the same permutation, not only the same value.  part_acc_out (B,) = matched pairs with cd < threshold / n.
 * matched_out (B,P) int64 in the reference's indexing: row i and value j count the NON-EMPTY parts in order, entries from n on are 0
 * (equal to slot indices only when no empty part precedes a used one).  A sample without a non-empty part: NaN and zeros.
 * Deterministic bit for bit.  ws >= rap_part_acc_workspace_bytes(TP, B, P) = two planes of TP * P floats, the work list and
 * O(B * P) words (0 for P > 256).  B = 0: RAP_OK, nothing launched. */
size_t rap_part_acc_workspace_bytes(int64_t TP, int32_t B, int32_t P);
int rap_part_acc(const float* pointclouds_gt, const float* pointclouds_pred, const int64_t* points_per_part, const int32_t* cu_batch,
                 int32_t B, int32_t P, int64_t TP, float threshold, float* part_acc_out, int64_t* matched_out, float* cd_out,
                 void* ws, size_t ws_bytes, void* stream);

/* Scan-pair metrics of a whole packed batch with P = 2, as Evaluator._compute_metrics forms them per pair in a Python loop (reference
 * eval/evaluator.py:124-248 with compute_correspondence_rmse, eval/metrics.py:386-469, and compute_approximate_transform_error, :487-508,
 * under the identity covariance).  Per sample b: source = part 0, target = part 1, every cloud multiplied by scales[b] (metres); a
 * correspondence is a source_gt point whose nearest target_gt point (first arg-min) lies within distance_threshold (the evaluator passes
 * 0.05).  R_pred / t_pred given ("transformed"): `cloud` = the input clouds, the compared clouds are (cloud s) R_pred^T + t_pred s per part;
 * both NULL ("direct"): `cloud` = the predicted clouds, compared as they are.  out4 (B,4) = {RMS of |src_i - tgt_nn(i)| over the
 * correspondences (inf if none), their number / n_source, transform error, their number}; transform error = sqrt(|dt|^2 + |q_xyz(dR)|^2)
 * with R_rel = R_tgt R_src^T, t_rel = s t_tgt - R_rel (s t_src), dR = R_rel_gt^T R_rel_pred, dt = t_rel_pred - t_rel_gt (inf in direct
 * mode).  A sample with an empty part gives {inf, 0, inf, 0}.  pointclouds_gt, cloud (TP,3); points_per_part (B,2) int64; cu_batch (B+1,)
 * int32; scales (B,); R_* (B,2,3,3), t_* (B,2,3).  Deterministic (no floating-point atomics); three launches, no host read.
 * ws >= rap_pair_metrics_workspace_bytes(TP, B). */
size_t rap_pair_metrics_workspace_bytes(int64_t n_points, int32_t B);
int rap_pair_metrics(const float* pointclouds_gt, const float* cloud, const int64_t* points_per_part, const int32_t* cu_batch,
                     const float* scales, const float* R_gt, const float* t_gt, const float* R_pred, const float* t_pred, int32_t B,
                     int64_t TP, float distance_threshold, float* out4, void* ws, size_t ws_bytes, void* stream);
/* Replaces compute_transform_errors_direct (reference eval/metrics.py:305-383): rap_transform_errors without the anchor frame -- every
 * non-empty part counts, delta_R = R_gt^T R_pred, delta_t = (t_pred - t_gt) * scale[b]; same shapes, outputs and NULL rules as
 * rap_transform_errors (per-part errors are 0 for empty parts; the means are over the non-empty parts, NaN for a sample without one). */
int rap_transform_errors_direct(const float* R_gt, const float* t_gt, const float* R_pred, const float* t_pred,
                                const int64_t* points_per_part, const int64_t* matched_part_ids, const float* scale, int32_t B, int32_t P,
                                float* rot_err_per_part, float* trans_err_per_part, float* rot_err_mean, float* trans_err_mean, void* stream);

/* Batched point-to-point ICP: K independent problems in one call, with the semantics of pytorch3d's iterative_closest_point (which the
 * reference calls one problem at a time: eval/metrics.py:79 in align_anchor, :261 in compute_transform_errors).  Problem k aligns
 * X[xs : xs + xn] to Y[ys : ys + yn] with (xs, xn) = x_seg[k], (ys, yn) = y_seg[k]; the tables are (K,2) int32, rows need not be contiguous
 * or ordered, lengths <= 0 are empty, and every row is clamped to its array on the device.  The x segments of one call must not overlap
 * (the work list holds n_x_points / 256 + K + 1 items; a problem that no longer fits is treated as an empty one).  Row-vector convention
 * Xt = X R + T, det R = +1.  Per problem, from R, T = init_R[k], init_T[k] (identity / zero where the pointer is NULL):
 *   for it in 0 .. max_iterations-1:
 *     nn(i) = first arg-min_j |Xt_i - Y_j|^2 (fp32 direct differences);  S = all i, or the i with sqrtf(d2_i) <= max_correspondence_distance;
 *     R, T = Kabsch fit of the ORIGINAL X[S] onto Y[nn(S)];  Xt = X R + T;  rmse = sqrt(mean_S |Xt_i - Y_nn(i)|^2);
 *     rel = 1 in the first iteration, else (prev - rmse) / prev;  iterations = it + 1;  rel <= relative_rmse_thr: converged = 1, stop.
 * Every problem stops on its own.  prev == 0 counts as converged.  An empty S stops the problem with the R, T and the iteration count it
 * had, rmse = inf and converged = 0.  xn == 0 or yn == 0: R, T = init or identity, rmse = NaN, iterations = 0, converged = 0.  Fewer than
 * three points give a finite proper rotation (the fit is not unique).  max_correspondence_distance <= 0: no gate; relative_rmse_thr =
 * -inf: no early stop.  Outputs: R (K,3,3), T (K,3), rmse (K,) fp32, iterations (K,) int32, converged (K,) uint8, and Xt (n_x_points,3) or
 * NULL: the points of every problem's x segment moved by its result (rows outside every segment are not written).
 * 1 + 2 * max_iterations (+ 1) launches enqueued up front; the convergence test never leaves the device, so there is no host read, no
 * allocation, and the call can be captured into a graph.  Deterministic (no floating-point atomics); a problem's bits do not depend on the
 * rest of the batch.  ws >= rap_icp_workspace_bytes(n_x_points, K) (0 for non-positive arguments). */
size_t rap_icp_workspace_bytes(int64_t n_x_points, int32_t K);
int rap_icp(const float* X, const int32_t* x_seg, const float* Y, const int32_t* y_seg, int32_t K, int64_t n_x_points, int64_t n_y_points,
            const float* init_R, const float* init_T, int32_t max_iterations, float relative_rmse_thr, float max_correspondence_distance,
            float* R, float* T, float* rmse, int32_t* iterations, uint8_t* converged, float* Xt, void* ws, size_t ws_bytes, void* stream);

/* rap_icp on a uniform-grid neighbour index: the argument list, the semantics and the RESULTS of rap_icp, bit for bit -- the grid is an
 * accelerator, not an approximation (same fp32 distance, same "first arg-min" winner, same sums in the same order).  The index over
 * the y segments of all K problems is built once per call, on the device (nine launches after the set-up), and queried in every
 * iteration: a query looks at the few dozen rows in the cells around it instead of at every row of its y segment.  Problems whose y
 * segments are the same rows share one grid.  y segments that overlap without being equal can ask for more than n_y_points indexed
 * rows; a problem that no longer fits is searched row by row (exact, and as slow as that sounds).  Rows of Y with a non-finite coordinate
 * can never be a neighbour, here as in rap_icp.  K <= 65535.  No host read, no allocation, no floating-point atomics (integer atomics
 * build the index; no result depends on their order); can be captured into a graph.
 * ws >= rap_icp_grid_workspace_bytes(n_x_points, n_y_points, K): host arithmetic, 0 for non-positive arguments, never less than
 * rap_icp_workspace_bytes(n_x_points, K); about 28 bytes per row of Y on top of it. */
size_t rap_icp_grid_workspace_bytes(int64_t n_x_points, int64_t n_y_points, int32_t K);
int rap_icp_grid(const float* X, const int32_t* x_seg, const float* Y, const int32_t* y_seg, int32_t K, int64_t n_x_points,
                 int64_t n_y_points, const float* init_R, const float* init_T, int32_t max_iterations, float relative_rmse_thr,
                 float max_correspondence_distance, float* R, float* T, float* rmse, int32_t* iterations, uint8_t* converged, float* Xt,
                 void* ws, size_t ws_bytes, void* stream);
/* The index on its own: exact nearest neighbours of K problems.  For every row i of problem k's x segment, idx_out[i] = the row of Y
 * (an index into Y, not into the segment) within k's y segment that is nearest to x_i R[k] + T[k] (x_i itself where R and T are NULL;
 * both or neither; R (K,3,3), T (K,3), row vectors), the first such row among equals, and d2_out[i] = that squared distance (fp32,
 * direct differences).  idx_out[i] = -1 and d2_out[i] = inf where no row lies within max_distance (sqrtf(d2) <= max_distance;
 * max_distance <= 0: no limit), where the y segment is empty, and where x_i has a non-finite coordinate.  idx_out, d2_out are
 * (n_x_points,); rows of X outside every segment are not written.  Segment tables, their clamping, the x segments that must not
 * overlap, K <= 65535 and the execution properties: as rap_icp_grid.  ws >= rap_nn_grid_workspace_bytes(n_x_points, n_y_points, K)
 * (host arithmetic; 0 for non-positive arguments). */
size_t rap_nn_grid_workspace_bytes(int64_t n_x_points, int64_t n_y_points, int32_t K);
int rap_nearest_neighbors(const float* X, const int32_t* x_seg, const float* Y, const int32_t* y_seg, int32_t K, int64_t n_x_points,
                          int64_t n_y_points, const float* R, const float* T, float max_distance, int32_t* idx_out, float* d2_out, void* ws,
                          size_t ws_bytes, void* stream);
/* The k nearest rows over the same index, exact.  For every row i of problem k's x segment: the count_out[i] <= k admissible rows of
 * Y within k's y segment with the smallest (d2, row), in ascending order of (d2, row) -- idx_out[i * k + s] = the row of Y (an index
 * into Y, not into the segment), d2_out[i * k + s] = its squared distance (fp32, direct differences: the distance of
 * rap_nearest_neighbors), s < count_out[i]; the unused slots hold -1 and inf.  A row of Y is admissible when d2 is finite and
 * sqrtf(d2) <= max_distance (max_distance <= 0: no limit); rows of Y with a non-finite coordinate never are, and an x_i with a
 * non-finite coordinate admits none (count 0).  k in 1 .. 32.  idx_out, d2_out are (n_x_points, k), count_out (n_x_points,); rows of X
 * outside every segment are not written.  With k = 1, idx_out and d2_out are what rap_nearest_neighbors returns with R = T = NULL, bit
 * for bit.  The list is put into its order before it is written, so the result is the same from call to call whatever order the index
 * was built in.  Segment tables, their clamping, the x segments that must not overlap, shared and overlapping y segments, K <= 65535 and
 * the execution properties: as rap_nearest_neighbors.  ws >= rap_knn_workspace_bytes(n_x_points, n_y_points, K) (host arithmetic, 0 for
 * non-positive arguments: the terms of rap_nn_grid_workspace_bytes). */
size_t rap_knn_workspace_bytes(int64_t n_x_points, int64_t n_y_points, int32_t K);
int rap_k_nearest_neighbors(const float* X, const int32_t* x_seg, const float* Y, const int32_t* y_seg, int32_t K, int64_t n_x_points,
                            int64_t n_y_points, int32_t k, float max_distance, int32_t* idx_out, float* d2_out, int32_t* count_out,
                            void* ws, size_t ws_bytes, void* stream);

/* Surface normals of packed clouds: the plane fit of every point's neighbourhood, Open3D's estimate_normals with a hybrid search as the
 * reference calls it (dataset_process/utils/dataset_utils.py:325-358: radius 0.5, max_nn 20).  P (n_points,3) fp32; seg (K,2) int32
 * (start, len) rows, clamped to the array on the device, which must not overlap (the work list holds n_points / 256 + K + 1 items; a
 * segment that no longer fits is left out); a segment that repeats an earlier one exactly is worked once, with the earlier one's
 * viewpoint.  For row i of segment k the neighbourhood is the rows j of the SAME segment with
 * sqrtf(d2(p_i, p_j)) <= radius (fp32 direct differences, the distance of rap_icp; radius <= 0: no limit, pure k-NN), of those the
 * max_nn (3 .. 32) with the smallest (d2, j), the row itself included; rows with a non-finite coordinate are never neighbours.  Mean
 * and centred covariance (divided by the count) in fp64 from the fp32 coordinates; the normal is the unit eigenvector of the smallest
 * eigenvalue (fp64 Jacobi), rounded to fp32.  Orientation: with viewpoint (K,3), n . (viewpoint[k] - p_i) >= 0; with NULL, the
 * component of largest magnitude is positive (the lowest index among equals).  Fewer than three neighbours, or a non-finite p_i:
 * normal (0,0,0) and eigenvalues 0 -- a stated departure from Open3D's (0,0,1): rap_icp_plane skips a zero normal, it cannot skip a
 * made-up one.  normals (n_points,3); eigenvalues (n_points,3) ascending, or NULL; rows outside every segment are not written.
 * Brute-force search, O(len^2) per segment: for voxel-downsampled clouds; rap_estimate_normals_grid below is the same estimate from
 * the grid index, for clouds at full resolution.  Two launches, no host read, no atomics,
 * deterministic, a row's bits depend on its own segment only; can be captured into a graph.
 * ws >= rap_normals_workspace_bytes(n_points, K) (host arithmetic; 0 for non-positive arguments). */
size_t rap_normals_workspace_bytes(int64_t n_points, int32_t K);
int rap_estimate_normals(const float* P, const int32_t* seg, int32_t K, int64_t n_points, int32_t max_nn, float radius,
                         const float* viewpoint, float* normals, float* eigenvalues, void* ws, size_t ws_bytes, void* stream);
/* rap_estimate_normals on the uniform-grid index: its argument list and its semantics word for word -- the neighbourhood rule, the fp64
 * mean and covariance, the eigenvector, both orientation rules, the zero normal below three neighbours, repeated segments worked once,
 * rows outside every segment not written.  The neighbour SETS are those of rap_estimate_normals (the k-best walk of
 * rap_k_nearest_neighbors over each segment's own rows is exact).  Mean and covariance are summed over the neighbours in ascending
 * (d2, j); rap_estimate_normals sums in the order its list filled, so the two may differ in the last bits of the fp64 sums, and
 * both are within 2e-6 of an fp64 plane fit; bit equality between them is not promised.  O(len) work per segment in place of O(len^2).
 * Segments that overlap without being equal stay the caller's responsibility.  K <= 65535.  The index is built once per call on the
 * device; no host read, no allocation, no floating-point atomics, deterministic (the same bits from call to call, and for a segment
 * whatever else is in the batch); can be captured into a graph.
 * ws >= rap_normals_grid_workspace_bytes(n_points, K) (host arithmetic, 0 for non-positive arguments: rap_normals_workspace_bytes plus
 * about 28 bytes per point for the index). */
size_t rap_normals_grid_workspace_bytes(int64_t n_points, int32_t K);
int rap_estimate_normals_grid(const float* P, const int32_t* seg, int32_t K, int64_t n_points, int32_t max_nn, float radius,
                              const float* viewpoint, float* normals, float* eigenvalues, void* ws, size_t ws_bytes, void* stream);
/* A consistent orientation for normals that exist already: the step the reference ends its normal estimation with (Open3D's
 * orient_normals_consistent_tangent_plane(k), dataset_process/utils/dataset_utils.py:325-358), restated as a pure function of integers
 * and signs.  P (n_points,3) and normals (n_points,3) fp32, normals in and out; seg (K,2) as rap_estimate_normals_grid takes it: (start,
 * len) rows clamped on the device, which must not overlap, a segment that repeats an earlier one exactly worked once (with the earlier
 * one's viewpoint), K <= 65535.  Rows outside every segment are not written, in normals and in component_out, and a segment's result
 * depends on that segment only.
 *   Vertices.  Row i of a segment is a vertex when its coordinates are finite and its normal is finite and not the zero vector.  Every
 * other row of a segment keeps its normal bits and gets component_out = -1.
 *   Graph.  There is an undirected edge {i, j} when both are vertices, i != j, and j is among the k nearest rows of i or i among those
 * of j.  "The k nearest rows" is the list rap_k_nearest_neighbors returns for a self-search of the segment (x_seg = y_seg = the
 * segment, max_distance 0): the smallest (d2, row), no distance limit, the row itself counted, as Open3D counts it; rows with a
 * non-finite coordinate are in no list.  A list slot whose row is not a vertex gives no edge.  k in 2 .. 32.
 *   Weight.  d = n_i . n_j in fp32 from the normals as passed in, in ONE expression, fma(z_i, z_j, fma(y_i, y_j, x_i * x_j)): the x
 * product rounded, y and z fused onto it; products commute, so both ends compute the same bits.  w = 1 - |d| (fp32).  Edges are ordered
 * as real numbers by (w, lo, hi), lo < hi the two row indices: a total order, so the minimum spanning forest is unique.  (A d that is
 * not finite -- normals beyond 1e19 -- orders by the bits of w like any other value; the result is still a function of the input.)
 *   Propagation.  Along a tree edge the child is flipped when d < 0 against its parent's current direction: sign(v) = sign(seed) times
 * the product over the tree path of (d < 0 ? -1 : +1), d from the input normals; d == 0 does not flip.
 *   Seed, one per connected component: the vertex with the largest z, the lowest row among equals (-0 == 0).  It is flipped when
 * n_z < 0; with viewpoint (K,3), when n . (viewpoint[k] - p) < 0, summed in double from the fp32 values as rap_estimate_normals
 * tests it.
 *   Outputs.  normals[i] is the input normal or its exact negation: only the three sign bits change.  component_out (n_points) int32 or
 * NULL: the row of P (an index into P, not into the segment) of the seed of i's component.
 *   Departure from Open3D, unpinned (Open3D is not part of the reference tree): Open3D adds the edges of a Euclidean minimum spanning
 * tree over a Delaunay tetrahedralisation, so its graph is connected, and starts from one seed.  Here each connected component of the
 * k-NN graph is oriented on its own from its own seed, and component_out says which rows belong together.
 *   k outside 2 .. 32, a NULL P, seg or normals, K or n_points out of range: RAP_ERR_INVALID; a NULL or short workspace:
 * RAP_ERR_WORKSPACE; both before any launch, nothing written.  The lists come from the k-best walk of rap_k_nearest_neighbors;
 * the forest from Boruvka rounds with integer 64-bit minima (no floating-point atomics), one launch per step: 16 launches plus, for t <
 * floor(log2 n_points), 3 + max(1, ceil(log2(n_points >> t))) per round t -- a function of n_points alone, so the call can be captured
 * into a graph; rounds after the last merge leave at their first instruction.  No host read, no allocation, the same bits from call to
 * call and for a segment whatever else is in the batch.
 * ws >= rap_orient_normals_workspace_bytes(n_points, K) (host arithmetic, 0 for non-positive arguments: the terms of
 * rap_normals_grid_workspace_bytes plus about 290 bytes per point, the lists at k = 32 and the forest). */
size_t rap_orient_normals_workspace_bytes(int64_t n_points, int32_t K);
int rap_orient_normals(const float* P, const int32_t* seg, int32_t K, int64_t n_points, int32_t k, const float* viewpoint, float* normals,
                       int32_t* component_out, void* ws, size_t ws_bytes, void* stream);

/* Submaps (submaps.hip): the stage of the reference's data preparation before the "views" exist
 * (dataset_process/utils/processing_utils.py:1927-2090).  Common to the four calls below:
 *   - F frames (sweeps) are ONE packed (n_points,3) fp32 array and cu_frames (F+1) int32 on the device, frame f = rows
 *     [cu_frames[f], cu_frames[f+1]); it must start at 0, not decrease and end at n_points.  S submaps are contiguous runs of frames:
 *     submap_frames (S+1) int32, submap s = frames [submap_frames[s], submap_frames[s+1]), entries in [0, F], not decreasing.  Every
 *     table is replaced by the running maximum of its clamped entries before it indexes anything; empty frames and submaps are valid.
 *   - poses are (F,4,4) float64, row-major, column vectors (x' = R x + t), as the reference's numpy arrays.
 *   - the DEFERRED error: a malformed input is not known to the host when the call returns.  The call then writes NaN (n_voxels: -1,
 *     connected: 0) to every output and ORs a bit into *status (device int32, or NULL; never cleared by a call): 1 a table had to be
 *     changed, 2 the voxel grid of rap_submap_overlap spans 2^21 voxels or more on an axis, 4 a group of
 *     rap_submap_groups_connected has a length outside [1, n_max] or a member outside [0, S).
 *   - limits: n_points < 2^31, F <= 2^24, S <= 4096.  n_points == 0 is valid (the point arrays may then be NULL); F == 0 is valid
 *     with n_points == 0 for rap_deskew and rap_fuse_frames and does nothing.
 *   - the caller's stream, no host read or wait, no floating-point atomics (integer atomics only: results are bit-identical from call
 *     to call), can be captured into a graph; ws >= the *_workspace_bytes query (host arithmetic, 0 for arguments the call refuses),
 *     and nothing outside it or the outputs is written.
 *
 * rap_deskew: per-point motion compensation (deskewing, dataset_utils.py:682-747).  ts (n_points,) fp32 time stamps; rel_pose[f] =
 * inv(pose[f-1]) pose[f], R a rotation by theta in [0, pi) (at theta = pi the axis is not defined: NaN).  Per frame, in fp32:
 * tmin, tmax over the frame (NaN stamps aside); s_i = (ts_i - tmin) / (tmax - tmin) - ts_mid, and s_i = 0.5 - ts_mid where
 * tmax - tmin <= 1e-8.  out_i = R(s_i) p_i + s_i T with R(s) = exp(s log R), the rotation about R's axis by s theta for ANY real s
 * (what roma.rotmat_slerp(I, R, s) evaluates): axis and angle once per frame in double, Rodrigues' formula per point in fp32 with a
 * series below 1e-3 rad.  Bit-for-bit the input where s_i == 0 and where rel_pose[f] is exactly the identity (how a caller says
 * "frame 0 is not deskewed"; such a frame is copied whatever its stamps are, NaN included); elsewhere NaN where ts_i is NaN.
 * Three launches. */
size_t rap_deskew_workspace_bytes(int64_t n_points, int32_t F);
int rap_deskew(const float* points, const float* ts, const int32_t* cu_frames, int32_t F, int64_t n_points, const double* rel_pose,
               float ts_mid, float* out, int32_t* status, void* ws, size_t ws_bytes, void* stream);

/* rap_fuse_frames: frames -> world (create_submap_from_frames, submap_utils.py:26-50, for every submap at once: rows keep their order,
 * so submap s is world[cu_frames[submap_frames[s]] .. cu_frames[submap_frames[s+1]])).  world_i = fp32(R p_i + t - origin) with the
 * arithmetic in double and ONE rounding (origin (3,) float64 or NULL = 0: a 10 km offset does not cost fp32 digits);
 * world_normals_i = fp32(R n_i / |R n_i|), divided by 1 where the norm is below 1e-8 (dataset_utils.py:402-405): a zero normal stays
 * zero.  normals and world_normals: both or neither.  Two launches. */
size_t rap_fuse_frames_workspace_bytes(int64_t n_points, int32_t F);
int rap_fuse_frames(const float* points, const float* normals, const int32_t* cu_frames, int32_t F, int64_t n_points, const double* pose,
                    const double* origin, float* world, float* world_normals, int32_t* status, void* ws, size_t ws_bytes, void* stream);

/* rap_submap_overlap: the S x S matrix of calculate_point_cloud_overlap_ratio_fast (dataset_utils.py:603-650, without its random
 * subsampling).  V_s = the set of voxels floor((R p + t) / voxel_size) (double; pose NULL: floor(p / voxel_size), points already in a
 * common frame) of the rows of submap s, rows with a non-finite coordinate (of R p + t; of p without poses) dropped; a finite coordinate whose
 * quotient reaches +-2^62 is not dropped: it fails the extent limit below (status bit 2).  ratio (S,S) float64, ratio[i][j] =
 * |V_i n V_j| / |V_i u V_j| (integers divided in double: exact wherever the voxel of every point is), 0.0 where V_i or V_j is empty
 * (i == j included), symmetric; n_voxels (S,) int64 = |V_s|.  F >= 1, 1 <= S <= 4096, voxel_size > 0 and finite.  The grid of the
 * whole call may span at most 2^21 - 1 voxel steps per axis (status bit 2 otherwise).  Voxel keys are sorted per submap with two
 * rocPRIM radix sorts; the intersections are binary searches of the smaller set's keys in the larger set.  The workspace query
 * reserves rocPRIM's scratch by a rule (8 bytes per row + 64 KiB) that holds for rocPRIM with caller-owned double buffers as shipped
 * with ROCm 7; the call asks rocPRIM for its actual need, and should a later rocPRIM want more than was reserved, the call returns
 * RAP_ERR_WORKSPACE although ws_bytes equals the query -- then AFTER its first launches, with ratio and n_voxels not written. */
size_t rap_submap_overlap_workspace_bytes(int64_t n_points, int32_t F, int32_t S);
int rap_submap_overlap(const float* points, const int32_t* cu_frames, int32_t F, int64_t n_points, const double* pose,
                       const int32_t* submap_frames, int32_t S, double voxel_size, double* ratio, int64_t* n_voxels, int32_t* status,
                       void* ws, size_t ws_bytes, void* stream);

/* rap_submap_groups_connected: the union-find of check_submap_validity (submap_utils.py:102-164) for G candidate groups at once.
 * ratio (S,S) float64 as above; groups (G,n_max) int32, group g = its first group_len[g] entries (submap numbers), 1 <= n_max <= 64.
 * Members a (earlier in the group) and b are joined where lo <= ratio[a][b] <= hi, both ends inclusive, NaN never; connected[g] = 1
 * where every member is reachable from the first (a group of one: 1).  connected (G,) uint8.  G == 0 does nothing.  One launch, one
 * wave per group, no workspace. */
int rap_submap_groups_connected(const double* ratio, int32_t S, const int32_t* groups, const int32_t* group_len, int32_t G, int32_t n_max,
                                double lo, double hi, uint8_t* connected, int32_t* status, void* stream);

/* Batched point-to-plane ICP: rap_icp's argument list plus Y_normals (n_y_points,3) fp32, and rap_icp's rules for segments, the gate,
 * empty problems (xn == 0 or yn == 0), Xt and the execution properties.  Per problem, from R, T = init or identity:
 *   for it in 0 .. max_iterations-1:
 *     p_i = x_i R + T (fp32);  nn(i) = first arg-min as in rap_icp;  S = the gated i whose normal n = Y_normals[nn(i)] is finite and not 0;
 *     in double: r_i = (p_i - y_nn(i)) . n,  J_i = [p_i x n, n],  A = sum_S J J^T,  b = sum_S J r,  e = sum_S r^2;
 *     S empty: rmse = inf, converged = 0, stop with the R, T it had;
 *     rmse = sqrt(e / |S|): the residual of the transform that ENTERED this iteration;
 *     (omega, tau) = -A^+ b, A^+ without the eigenvalues <= 1e-12 lambda_max (the minimum-norm step: no motion along what a planar
 *     target does not observe);  dR = exp([omega]x);  R <- R dR^T,  T <- T dR^T + tau  (kept in fp64 between iterations; the outputs are
 *     its fp32 rounding);  iterations = it + 1;  rel = 1 in the first iteration, else (prev - rmse) / prev;
 *     prev == 0 or rel <= relative_rmse_thr: converged = 1, stop.
 * The update of the last iteration is applied before the stop, so the reported rmse is one update BEHIND the returned R, T.
 * rap_icp_plane_grid: the same on the uniform-grid index of rap_icp_grid, bit for bit (K <= 65535).
 * ws >= rap_icp_plane_workspace_bytes(n_x_points, K) / rap_icp_plane_grid_workspace_bytes(n_x_points, n_y_points, K). */
size_t rap_icp_plane_workspace_bytes(int64_t n_x_points, int32_t K);
int rap_icp_plane(const float* X, const int32_t* x_seg, const float* Y, const int32_t* y_seg, const float* Y_normals, int32_t K,
                  int64_t n_x_points, int64_t n_y_points, const float* init_R, const float* init_T, int32_t max_iterations,
                  float relative_rmse_thr, float max_correspondence_distance, float* R, float* T, float* rmse, int32_t* iterations,
                  uint8_t* converged, float* Xt, void* ws, size_t ws_bytes, void* stream);
size_t rap_icp_plane_grid_workspace_bytes(int64_t n_x_points, int64_t n_y_points, int32_t K);
int rap_icp_plane_grid(const float* X, const int32_t* x_seg, const float* Y, const int32_t* y_seg, const float* Y_normals, int32_t K,
                       int64_t n_x_points, int64_t n_y_points, const float* init_R, const float* init_T, int32_t max_iterations,
                       float relative_rmse_thr, float max_correspondence_distance, float* R, float* T, float* rmse, int32_t* iterations,
                       uint8_t* converged, float* Xt, void* ws, size_t ws_bytes, void* stream);

/* Joint multi-view refinement of registered scenes: ONE point-to-plane Gauss-Newton problem per scene over the poses of all its views,
 * every directed edge (source view a, target view b) contributing as a rap_icp_plane step would.  Unpinned: the reference has no
 * counterpart (it runs pytorch3d's pairwise ICP only); the yardstick is the fp64 restatement of this comment in
 * tests/scene_refine_oracle.py.
 * Inputs.  P (n_points,3) and normals (n_points,3) fp32, every view in its OWN frame.  view_seg (V,2) int32: (start, len) rows of every
 * view, clamped to the array on the device as rap_icp's segments are (len <= 0: an empty view); views must not overlap.  scene_seg (S,2)
 * int32: (first view, number of views), clamped to the view table likewise; every scene owns a contiguous run of the view table and
 * scenes must not overlap.  edges (E,2) int32: (a, b), directed; an edge is IGNORED (edge_count = 0, edge_rmse = NaN, no contribution)
 * when a or b is out of range, a == b, the two views belong to different scenes or to no scene or to a scene that is left out (below),
 * either view is empty, or the row budget (below) is spent.  A duplicate edge counts twice.  fixed (V,) uint8 marks the views whose pose
 * is not a variable; NULL: the first view of every scene.  A scene without a fixed view is legal (the minimum-norm step below resolves
 * the gauge).  init_R (V,3,3), init_T (V,3), or both NULL for the identity: the row-vector convention of rap_icp, world = x R_v + T_v.
 * Per scene, from the fp64 state R_v, T_v = the fp32 init, for it in 0 .. max_iterations-1:
 *   1. for every live edge e = (a, b), in double: R_e = R_a R_b^T, T_e = (T_a - T_b) R_b^T, both rounded to fp32 (a's rows in b's frame);
 *      q_i = x_i R_e + T_e in fp32 for every row x_i of view a;  nn(i) = first arg-min over view b's rows of the fp32 direct-difference
 *      distance, as in rap_icp;  the pairs that count are those with sqrtf(d2_i) <= max_correspondence_distance (<= 0: no gate) whose
 *      normal n = normals[nn(i)] is finite and not 0;  over them, in double, with y = b's row nn(i):  r = (q - y) . n,  J = [q x n, n],
 *      A_e = sum J J^T,  b_e = sum J r,  e_e = sum r^2,  n_e = the number of pairs (rap_icp_plane's sums, in b's frame);
 *   2. n = sum_e n_e;  n == 0: rmse = inf, converged = 0, stop with the poses (and the iteration count) the scene had;
 *      rmse = sqrt(sum_e e_e / n): the residual of the poses that ENTERED this iteration, one update behind the returned poses;
 *   3. the system of the scene over world-frame twists xi_v = (omega_v, tau_v), which act on world points as p <- p dR^T + tau:
 *      with M_b = [[R_b, 0], [-R_b [T_b]x, R_b]] (column form, xi_local = M_b xi_world):  A_w = M_b^T A_e M_b,  g_w = M_b^T b_e;
 *      in ascending edge order A_w is added to the blocks (a,a) and (b,b) of H and subtracted from (a,b) and (b,a), g_w is added to
 *      g[a] and subtracted from g[b] (the residual depends on the relative pose only: J_b = -J_a).  Equivalently the sums over
 *      J_w = [p_w x n_w, n_w] with p_w = q R_b + T_b, n_w = n R_b.  The rows and columns of fixed views are struck;
 *   4. xi = -H^+ g, H^+ without the eigenvalues <= 1e-12 lambda_max (fp64 cyclic Jacobi): the minimum-norm step.  A view without a live
 *      edge does not move, a planar scene does not slide in its plane, a scene without a fixed view does not drift;
 *   5. every free view: dR = exp([omega_v]x),  R_v <- R_v dR^T,  T_v <- T_v dR^T + tau_v, kept in fp64 between iterations; the outputs
 *      R, T are always the fp32 rounding of the state.  A view whose step is exactly zero, a fixed view, and a view outside every
 *      (admitted) scene keep the fp32 init bit for bit;
 *   6. iterations = it + 1;  rel = 1 in the first iteration, else (prev - rmse) / prev;  prev == 0 or rel <= relative_rmse_thr:
 *      converged = 1, stop.  Every scene stops on its own.
 * Outputs: R (V,3,3), T (V,3) fp32; rmse (S,) fp32, iterations (S,) int32, converged (S,) uint8; edge_rmse (E,) fp32 and edge_count (E,)
 * int32, or NULL: sqrt(e_e / n_e) (NaN where n_e == 0) and n_e of the LAST iteration the edge's scene ran.
 * Limits.  max_views in 2 .. 16: it sizes the solve (96 unknowns; H and its eigenvectors, two 96 x 96 fp64 matrices, live in the 160 KB
 * LDS of a compute unit).  A scene with more views than max_views is LEFT OUT: rmse = NaN, iterations = 0, converged = 0, poses = init.
 * row_budget: the caller's upper bound on the rows of the source views summed over the live edges; the work list holds
 * row_budget / 256 + E + 1 items; edges are admitted in ascending order while sum len(a) <= row_budget, all of an edge or none, and an
 * edge that does not fit is ignored (later, shorter ones are still tried).  V, E <= 65535; n_points <= (2^31 - 1) / 8 as in every call on
 * the grid index.  RAP_ERR_INVALID: NULL P, normals, view_seg, scene_seg, edges, R, T, rmse, iterations or converged; sizes that are not
 * positive or out of range; NaN thresholds; max_iterations <= 0.  RAP_ERR_WORKSPACE: ws NULL or ws_bytes below
 * rap_scene_refine_workspace_bytes(...) (host arithmetic; 0 for arguments the call would refuse).  Both before any launch, with nothing
 * written.
 * Execution: 10 + 4 * max_iterations launches enqueued up front (set-up, the grid index of rap_icp_grid with one grid per view, then per
 * iteration edge poses, the query, the per-edge sums and one block per scene); no host read, no allocation, no floating-point
 * atomics; the same bits from call to call whatever the workspace held; a scene's bits do not depend on the rest of the batch (the
 * order of a scene's edges among themselves does: it is the order of the sums of step 3); the call can be captured into a graph. */
size_t rap_scene_refine_workspace_bytes(int64_t n_points, int32_t V, int32_t S, int32_t E, int64_t row_budget, int32_t max_views);
int rap_scene_refine(const float* P, const float* normals, const int32_t* view_seg, int32_t V, int64_t n_points, const int32_t* scene_seg,
                     int32_t S, const int32_t* edges, int32_t E, int64_t row_budget, int32_t max_views, const uint8_t* fixed,
                     const float* init_R, const float* init_T, int32_t max_iterations, float relative_rmse_thr,
                     float max_correspondence_distance, float* R, float* T, float* rmse, int32_t* iterations, uint8_t* converged,
                     float* edge_rmse, int32_t* edge_count, void* ws, size_t ws_bytes, void* stream);

/* Robust losses for the three point-to-plane calls above.  loss: one of the codes below; loss_scale: its scale k > 0, in the units of the
 * clouds.  Which pairs count is UNCHANGED: the neighbour, the gate and the usable-normal rule are the sibling's.  For every counted pair,
 * in double, from the residual r the sibling forms:
 *   RAP_LOSS_NONE    w = 1                                    rho = r^2 / 2
 *   RAP_LOSS_HUBER   w = 1 if |r| <= k, else k / |r|          rho = r^2 / 2 if |r| <= k, else k (|r| - k / 2)
 *   RAP_LOSS_CAUCHY  w = 1 / (1 + (r/k)^2)                    rho = (k^2 / 2) log1p((r/k)^2)
 *   RAP_LOSS_TUKEY   w = (1 - (r/k)^2)^2 if |r| <= k, else 0  rho = (k^2 / 6) (1 - (1 - (r/k)^2)^3) if |r| <= k, else k^2 / 6
 * and the sums of the sibling become (iteratively reweighted Gauss-Newton)
 *   A = sum w J J^T,  b = sum w J r,  e = sum 2 rho,  W = sum w,  n = the number of counted pairs (zero-weight pairs included).
 * rmse = sqrt(e / n) (the plain rmse for RAP_LOSS_NONE); rap_scene_refine_robust's edge_rmse = sqrt(e_e / n_e) likewise, edge_count
 * stays n_e, and step 1's A_e, b_e, e_e are the weighted sums.  The stopping rule acts on this rmse.  W == 0 (every weight zero) is
 * treated as n == 0: rmse = inf, converged = 0, stop with the pose(s) and the iteration count the problem or scene had.  Everything else
 * is the sibling's algorithm word for word.  With RAP_LOSS_NONE loss_scale is ignored and the call returns the bits of its sibling.
 * weights (n_x_points,) fp32 or NULL (the two pairwise calls): the weight every source row had in the LAST iteration its problem ran, the
 * one of the pose that entered that iteration; 0 for a row that was gated out or matched a row without a usable normal, and for the
 * rows of a problem that ran no iteration; rows outside every segment are not written.
 * RAP_ERR_INVALID, before any launch and with nothing written: a loss code outside 0 .. 3; loss != RAP_LOSS_NONE with a loss_scale that
 * is not finite and positive; whatever the sibling refuses.  ws >= the call's own *_workspace_bytes (the sibling's arguments; host
 * arithmetic, 0 for arguments the call would refuse; the partial sums also carry W, so it is larger than the sibling's).  The execution
 * properties are the siblings': the caller's stream, no host read, no allocation, no floating-point atomics, the same bits from call
 * to call whatever the workspace held, a problem's or scene's bits independent of the rest of the batch, capturable into a graph
 * (one launch more than the sibling where weights is given). */
#define RAP_LOSS_NONE 0
#define RAP_LOSS_HUBER 1
#define RAP_LOSS_CAUCHY 2
#define RAP_LOSS_TUKEY 3
size_t rap_icp_plane_robust_workspace_bytes(int64_t n_x_points, int32_t K);
int rap_icp_plane_robust(const float* X, const int32_t* x_seg, const float* Y, const int32_t* y_seg, const float* Y_normals, int32_t K,
                         int64_t n_x_points, int64_t n_y_points, const float* init_R, const float* init_T, int32_t max_iterations,
                         float relative_rmse_thr, float max_correspondence_distance, float* R, float* T, float* rmse, int32_t* iterations,
                         uint8_t* converged, float* Xt, int32_t loss, float loss_scale, float* weights, void* ws, size_t ws_bytes,
                         void* stream);
size_t rap_icp_plane_grid_robust_workspace_bytes(int64_t n_x_points, int64_t n_y_points, int32_t K);
int rap_icp_plane_grid_robust(const float* X, const int32_t* x_seg, const float* Y, const int32_t* y_seg, const float* Y_normals, int32_t K,
                              int64_t n_x_points, int64_t n_y_points, const float* init_R, const float* init_T, int32_t max_iterations,
                              float relative_rmse_thr, float max_correspondence_distance, float* R, float* T, float* rmse,
                              int32_t* iterations, uint8_t* converged, float* Xt, int32_t loss, float loss_scale, float* weights, void* ws,
                              size_t ws_bytes, void* stream);
size_t rap_scene_refine_robust_workspace_bytes(int64_t n_points, int32_t V, int32_t S, int32_t E, int64_t row_budget, int32_t max_views);
int rap_scene_refine_robust(const float* P, const float* normals, const int32_t* view_seg, int32_t V, int64_t n_points,
                            const int32_t* scene_seg, int32_t S, const int32_t* edges, int32_t E, int64_t row_budget, int32_t max_views,
                            const uint8_t* fixed, const float* init_R, const float* init_T, int32_t max_iterations, float relative_rmse_thr,
                            float max_correspondence_distance, float* R, float* T, float* rmse, int32_t* iterations, uint8_t* converged,
                            float* edge_rmse, int32_t* edge_count, int32_t loss, float loss_scale, void* ws, size_t ws_bytes, void* stream);

/* ---- MiniSpinNet local feature extractor (the step before the path) ----
 * Replaces MiniSpinNet.forward (reference dataset_process/utils/spinnet/patch_embedder.py:49-183 with patchnet.py:16-84 and
 * utils/common.py) as extract_sample_features.py:151-220 / demo.py:959-988 call it: global-z alignment, 512 points per patch,
 * 3 x 7 x 20 voxels x 10 samples, delta 0.8 -- the only configuration the reference ships.  Weight blob = the float tensors
 * of MiniSpinNet.state_dict() in registration order (pnt_layer, pool_layer, conv_net; num_batches_tracked skipped), eval mode.
 * rap_spinnet_describe: pts (N,3) raw cloud, perm (N,) int32 or NULL = the shuffle select_patches applies before the ball
 * query (patch_embedder.py:99-100; the ball query keeps the first 512 in-radius points IN THAT ORDER), kpts (K,3), des_r;
 * desc_out (K,32) unit-norm descriptors = the `features` of the sampling path.  Keypoints are processed in chunks of
 * keypoints_per_chunk; ws >= rap_spinnet_workspace_bytes(keypoints_per_chunk) (about 0.8 MB per keypoint). */
typedef struct rap_spinnet rap_spinnet;
int64_t rap_spinnet_weight_count(void);
int rap_spinnet_create(const float* d_weights, int64_t n_floats, void* stream, rap_spinnet** out);
void rap_spinnet_destroy(rap_spinnet* m);
size_t rap_spinnet_workspace_bytes(int32_t keypoints_per_chunk);
/* flags of rap_spinnet_describe (per call: the handle is immutable after rap_spinnet_create, two callers may share it):
 *   RAP_SPINNET_PATCH_LRF   patch alignment of MiniSpinNet.forward (patch_embedder.py:141-166): unset (default) = is_aligned_to_global_z,
 *                           the shipped demo setting (R = I); set = every patch is rotated so that its own normal -- the singular vector of
 *                           the smallest singular value of the patch covariance, oriented towards the origin (cal_Z_axis,
 *                           utils/common.py:539-557) -- becomes +z (RodsRotatFormula, :472-496);
 *   RAP_SPINNET_IM2COL_PATH A/B: unset (default) = the seven 3x3 cylindrical convolutions as implicit GEMMs (spin_conv3x3_kernel: the
 *                           im2col gather happens in the LDS-DMA source addresses); set = the round-1 path (materialised im2col + the
 *                           fp32 GEMM at 128 padded columns). */
#define RAP_SPINNET_PATCH_LRF 1
#define RAP_SPINNET_IM2COL_PATH 2
int rap_spinnet_describe(const rap_spinnet* m, const float* pts, const int32_t* perm, int64_t N, const float* kpts, int32_t K,
                         float des_r, int32_t flags, float* desc_out, int32_t keypoints_per_chunk, void* ws, size_t ws_bytes, void* stream);

/* Farthest point sampling, the keypoint selection in front of MiniSpinNet (reference dataset_process/utils/
 * point_sampling_utils.py:263-305 -> pytorch3d.ops.sample_farthest_points with lengths, per-cloud K and a random start):
 * points (T,3) holds the clouds: cloud c = rows [cloud_start[c], cloud_start[c] + cloud_len[c]) (packed or zero-padded batches
 * alike); k_per_cloud / start_idx (n_clouds,) int32 (the caller draws the start indices, as pytorch3d does with torch.randint);
 * indices_out (n_clouds, k_max) int32, cloud-local, -1 padded past min(K, length); dist_ws: T floats of scratch.  Ties go to the
 * lowest index (torch.argmax). */
int rap_farthest_point_sampling(const float* points, const int32_t* cloud_start, const int32_t* cloud_len, const int32_t* k_per_cloud,
                                const int32_t* start_idx, int32_t n_clouds, int32_t k_max, int32_t* indices_out, float* dist_ws,
                                void* stream);
/* rap_farthest_point_sampling over a bucket index: the same tables and, for every input, bit for bit the same indices_out (clamped
 * starts, K > length, -1 padding, zero-length clouds, duplicate points and non-finite rows included).  One block per cloud sorts the
 * cloud's rows into the cells of a uniform grid (about points_per_bucket rows per cell, at most max_buckets cells) and keeps per cell
 * the tight box of its rows, the largest running distance in it and the lowest index that attains it; a pick then updates only the
 * cells whose box lies closer to it than their largest distance, and the next pick is the best cell's.  A cloud with a non-finite
 * coordinate is walked by the plain loop inside the same kernel.  The result depends neither on the order the sort leaves inside a
 * cell nor on the other clouds of the call; no host synchronisation.
 * total_points: the rows of `points` (the cloud tables are clamped to it, and it sizes the workspace: 20 bytes per point, the sorted
 * rows and their running distances); workspace >= rap_fps_grid_workspace_bytes(total_points, n_clouds) (host arithmetic; 0 without a
 * point).  Null pointers and bad counts: RAP_ERR_INVALID; a missing or short workspace: RAP_ERR_WORKSPACE before anything is written.
 * rap_fps_grid_params returns the two build constants in effect (rap_set_tuning key 22 sets points_per_bucket to one of 1, 8, 16, 32,
 * 48, 64, 128 and key 23 the block size to 256, 512 or 1024; every setting gives the same indices). */
size_t rap_fps_grid_workspace_bytes(int64_t total_points, int32_t n_clouds);
int rap_farthest_point_sampling_grid(const float* points, int64_t total_points, const int32_t* cloud_start, const int32_t* cloud_len,
                                     const int32_t* k_per_cloud, const int32_t* start_idx, int32_t n_clouds, int32_t k_max,
                                     int32_t* indices_out, void* workspace, size_t workspace_bytes, void* stream);
void rap_fps_grid_params(int32_t* points_per_bucket, int32_t* max_buckets);

/* Voxel down-sampling, the first preprocessing step of the same script (reference dataset_process/utils/dataset_utils.py:279-322,
 * voxel_down_sample_torch): per occupied voxel the point closest to the voxel centre (distance quantised to 1000 levels, ties to the
 * lowest index), indices returned in ascending voxel-key order.  Two steps because the dense key table is sized from the data:
 *   rap_voxel_bounds    -> bounds6_out (device, 6 int64: per-axis min then max of floor(p / voxel_size)), dist_max_out (device float);
 *   the caller copies both to the host (the reference synchronises at the same point), then
 *   rap_voxel_downsample(points, N, voxel_size, h_bounds6 (HOST), dist_max, indices_out (device, >= min(N, slots) int64),
 *                        count_out (device int32: number of kept points), ws >= rap_voxel_workspace_bytes(h_bounds6)).
 * rap_voxel_table_slots returns the table size (8 bytes per slot), or -1 when the grid needs more than 2^33 slots. */
int rap_voxel_bounds(const float* points, int64_t N, float voxel_size, int64_t* bounds6_out, float* dist_max_out, void* stream);
int64_t rap_voxel_table_slots(const int64_t* h_bounds6);
size_t rap_voxel_workspace_bytes(const int64_t* h_bounds6);
/* Exact number of occupied voxels = distinct rows of floor(points / voxel_size) (calculate_voxel_coverage,
 * dataset_process/utils/point_sampling_utils.py:11-31; the down-sampling table above keeps the reference's colliding key and cannot
 * count).  h_bounds6 from rap_voxel_bounds (HOST); count_out: device int64; ws >= rap_voxel_coverage_workspace_bytes(h_bounds6). */
size_t rap_voxel_coverage_workspace_bytes(const int64_t* h_bounds6);
int rap_voxel_coverage(const float* points, int64_t N, float voxel_size, const int64_t* h_bounds6, int64_t* count_out, void* ws,
                       size_t ws_bytes, void* stream);
int rap_voxel_downsample(const float* points, int64_t N, float voxel_size, const int64_t* h_bounds6, float dist_max,
                         int64_t* indices_out, int32_t* count_out, void* ws, size_t ws_bytes, void* stream);
/* The same two results with O(N) memory (a radix sort of one 64-bit key per point instead of a table over the grid volume): for grids
 * whose dense table would be large against N or exceed its slot limit.  Identical outputs (kept indices in ascending voxel-key order;
 * the exact occupied-voxel count).  Limits: N < 2^32; down-sampling needs the largest grid extent v < 2^18 cells.
 * ws >= rap_voxel_sorted_workspace_bytes(N) for both.  Reference: dataset_utils.py:279-322, point_sampling_utils.py:11-31. */
size_t rap_voxel_sorted_workspace_bytes(int64_t N);
int rap_voxel_downsample_sorted(const float* points, int64_t N, float voxel_size, const int64_t* h_bounds6, float dist_max,
                                int64_t* indices_out, int32_t* count_out, void* ws, size_t ws_bytes, void* stream);
int rap_voxel_coverage_sorted(const float* points, int64_t N, float voxel_size, const int64_t* h_bounds6, int64_t* count_out, void* ws,
                              size_t ws_bytes, void* stream);

/* ---- kernel-level entry points (used by the parity tests; same kernels the calls above launch) ---- */
/* C(M,N) = A(M,K) W(N,K)^T (+bias) (+resid) ; epilogue: 0 bias, 1 bias+resid, 2 bias+SiLU,
 * 3 GEGLU (W/bias must be value/gate interleaved by rap_geglu_interleave; C is (M,N/2)),
 * 4 head-major qkv scatter ([3][H][M][64]), 5 bias + anchor embedding select, 6 bias+ReLU, 8 bias+GELU (erf, nn.GELU()'s default;
 * 7 is internal and refused). */
int rap_gemm_f32(int32_t epilogue, const float* A, int32_t lda, const float* W, int32_t ldw, float* C, int32_t ldc,
                 int32_t M, int32_t N, int32_t K, const float* bias, const float* resid, int32_t ldr,
                 const uint8_t* anchor, const float* anchor_emb, int32_t heads, void* stream);
int rap_geglu_interleave(const float* W, const float* b, float* Wp, float* bp, int32_t inner, int32_t K, void* stream);
/* Which kernel a GEMM call takes, as pure host arithmetic (no device is touched; the launchers switch on the same function).  The FORM code is
 *   100 * kernel + 10 * stages + splits
 *   kernel: 1 = 128 x 128 tiles; 2 = 256 x 256, one tile per block (any M: rows are clamped, stores predicated); 3 = 256 x 256 persistent
 *           (one block per CU walks its share of the tiles; M % 256 == 0)
 *   stages: LDS stages of the 128 x 128 kernel: 2, or 4 for the four-stage ring of the 16-bit kernels (launches of at most tuning key 18
 *           blocks); 0 for the 256 x 256 kernels
 *   splits: blocks per tile that K is divided over: 1 (no split), 2 or 4 -- on the 128 x 128 kernel only
 * so e.g. 121, 141, 144, 201, 301.  0: nothing is launched (M <= 0).  Negative (RAP_ERR_INVALID): the shape is refused.  The current
 * tuning keys are honoured (6 split K, 11 / 12 persistent, 18 ring), as by the calls themselves.
 * rap_gemm_f32_form: the call rap_gemm_f32 / rap_gemm_f32_splitk makes with these arguments; has_ws != 0: a split-K workspace is handed in
 *   (planes: the planes it holds for epilogue 2 -- 2 or 4; ignored otherwise).
 * rap_gemm_h16_form: dtype 1 / 2: rap_gemm_h16 (epilogue 5: rap_gemm_h16_qkvnorm), has_ws != 0: rap_gemm_h16_splitk with its workspace;
 *   dtype 3: rap_x2_gemm (K, lda, ldw in physical fp16 columns). */
int rap_gemm_f32_form(int32_t epilogue, int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldw, int32_t ldc, int32_t ldr,
                      int32_t has_ws, int32_t planes);
int rap_gemm_h16_form(int32_t dtype, int32_t epilogue, int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldw, int32_t has_ws);
/* What a model call of a given shape does, as pure host arithmetic: no model handle, no device.  The launch path itself runs by the function
 * this reports (api.hip: plan_call), so the answer cannot drift from the call.  The current tuning keys are honoured (5, 6, 7, 11, 12, 17 - 20).
 *   compute_dtype / resid_dtype: as rap_model_set_compute_dtype / rap_model_set_residual_dtype; d, heads, num_layers, in_dim: the model
 *   (qk-norm on, softcap = 0, SiLU head: a capped model runs every attention launch unsplit on 256-row items, a GELU / ReLU head never
 *   splits K -- rap_model_set_softcap, rap_model_set_final_act); TP tokens, B samples, nseg_part part segments (empty ones counted: B x P of rap_sample, VP of rap_dit_forward);
 *   rows: rows of the adaLN table (flow steps of rap_sample, B of rap_dit_forward: the workspace size depends on it, nothing else does);
 *   bounded != 0: the attention launches take the bounded softmax (rap_model_bounded_attention_launches counts them).
 * out[0 .. RAP_CALL_PLAN_FIELDS - 1] (n_out >= RAP_CALL_PLAN_FIELDS):
 *    0 arithmetic of the call (a split-precision model below tuning key 17: 0)   1 TQ = align_up(TP, 256)
 *    2 query rows per attention work item   3 key groups per block of the 16-bit attention
 *    4 / 5 work-list sizes of the per-part / per-sample branch   6 / 7 their key ranges (fp32 and split precision; 1 = unsplit)
 *    8 / 9 fp32: that branch's split launch keeps every CU to one block   10 combine + LayerNorm fusion on   11 split-K planes reserved
 *   12 .. 19 form codes (rap_gemm_f32_form / rap_gemm_h16_form) of the static-embedding, x_t-embedding, QKV, out-projection, ff1, ff2 and
 *      the two head GEMMs (head: M = TQ; a rap_dit_forward call of the fp16 stream with a feature output runs them at M = TP)
 *   20 workspace bytes (rap_workspace_bytes of such a model: the larger of the two layouts for a split-precision one)
 * Bad arguments (a NULL or short out, an unknown dtype, a width rap_model_create refuses, TP / B / rows <= 0): RAP_ERR_INVALID, out untouched. */
#define RAP_CALL_PLAN_FIELDS 21
int rap_call_plan(int32_t compute_dtype, int32_t resid_dtype, int32_t d, int32_t heads, int32_t num_layers, int32_t in_dim, int64_t TP,
                  int32_t B, int32_t nseg_part, int32_t rows, int32_t bounded, int64_t* out, int32_t n_out);
/* Epilogues 1 (bias + residual) and 2 (bias + SiLU) of rap_gemm_f32 with the split-K form rap_sample uses on few-token calls (tuning key
 * 6).  Counting tiles of 128 x 128 and k-tiles of 32 columns:
 *   epilogue 1: K >= 1024 and at most 128 tiles, or K >= 512 and at most 64 tiles: K over 4 blocks per tile (block y takes k-tiles
 *     [nk y / 4, nk (y + 1) / 4): the shares need not be equal), workspace 4 M N floats;
 *   epilogue 2: planes (2 or 4; anything else: RAP_ERR_INVALID) blocks per tile when K >= 512, K / 32 is a multiple of planes and there are at
 *     most 64 tiles, workspace planes M N floats.
 * The blocks write fp32 partial tiles to ws and a combine pass forms resid + bias + partials (or SiLU of bias + partials) in a fixed order
 * (deterministic; equals the unsplit result up to the fp32 association of the k-sum).  ldc % 4 == 0 and ldr % 4 == 0 (rows move as 16-byte
 * pieces), otherwise the call runs unsplit.  resid (epilogue 1: required, may alias C) has row stride ldr.
 * rap_gemm_f32_splitk_workspace_bytes: 0 when the rule does not split -- a function of the shape alone (key 6 gates the launch, not the
 * reservation).  With a workspace size of 0 the call is rap_gemm_f32.  NULL operands, other epilogues (RAP_ERR_INVALID) and a workspace
 * below the query's value (RAP_ERR_WORKSPACE) are refused before anything touches the device. */
size_t rap_gemm_f32_splitk_workspace_bytes(int32_t epilogue, int32_t M, int32_t N, int32_t K, int32_t planes);
int rap_gemm_f32_splitk(int32_t epilogue, const float* A, int32_t lda, const float* W, int32_t ldw, float* C, int32_t ldc, int32_t M,
                        int32_t N, int32_t K, const float* bias, const float* resid, int32_t ldr, int32_t planes, void* ws,
                        size_t ws_bytes, void* stream);
/* The work list of one attention launch, as rap_sample / rap_dit_forward build it (once per call, on the device): one item
 * {seg_start, seg_len, q0, 0} (4 x int32) per `block_queries` (256) query rows of every segment of cu_seqlens (nseg + 1 entries),
 * LONGEST SEGMENT FIRST when sort_ws (nseg ints of scratch) is given -- a block streams all keys of its segment, blocks are
 * dispatched in order, so the long blocks of a ragged batch (reference: 200 ... 40 000 points per part) must not start last --
 * segment order when sort_ws is NULL; items beyond the last one are zero (seg_len 0 = no work).  items_out: max_items x 4 int32. */
int rap_build_attention_worklist(const int32_t* cu_seqlens, int32_t nseg, int32_t block_queries, int32_t* items_out,
                                 int32_t max_items, int32_t* sort_ws, void* stream);
/* flash_attn_varlen_qkvpacked_func equivalent (reference layer.py:106-111,123-128) on head-major qkv
 * [3][H][TP][64]; out (TP, H*64).  ws >= rap_attention_workspace_bytes(TP, nseg). */
size_t rap_attention_workspace_bytes(int64_t TP, int32_t nseg);
int rap_attention_f32(const float* qkv_headmajor, const int32_t* cu_seqlens, int32_t nseg, float* out, int64_t TP,
                      int32_t heads, const float* logit_bound /* NULL or H device floats, see rap_attention_h16; each must be
                      <= 40 (the fp32 kernel then drops the softmax offset: |score| log2 e <= 58); a head whose bound is larger gets
                      NaN outputs */, void* ws,
                      size_t ws_bytes, void* stream);
/* The SOFT-CAPPED attention kernels a model with rap_model_set_softcap(c > 0) runs, one per arithmetic: every logit s = q.k / sqrt(64)
 * becomes softcap * tanh(s / softcap) before the online softmax (flash-attn's softcap).  Operands, layouts and workspace
 * (rap_attention_workspace_bytes) are those of rap_attention_f32 / rap_attention_h16 (q as projected or normalised, q_mul = 8: not
 * pre-scaled) / rap_x2_attention; there is no logit_bound (the bounded softmax has no capped form).  One launch form each: 256-row work
 * items, unsplit, whatever the tuning keys 5, 16 and 20 say.  softcap <= 0 or not finite: RAP_ERR_INVALID; a workspace below the query's
 * value: RAP_ERR_WORKSPACE; both before anything is written. */
int rap_attention_f32_softcap(const float* qkv_headmajor, const int32_t* cu_seqlens, int32_t nseg, float* out, int64_t TP,
                              int32_t heads, float softcap, void* ws, size_t ws_bytes, void* stream);
int rap_attention_h16_softcap(int32_t dtype, const uint16_t* qk, const uint16_t* vt, int32_t vt_nblk, const int32_t* cu_seqlens,
                              int32_t nseg, uint16_t* out, int64_t TP, int32_t heads, float softcap, void* ws, size_t ws_bytes,
                              void* stream);
int rap_x2_attention_softcap(const uint16_t* qk, const uint16_t* vt, int32_t vt_nblk, const int32_t* cu_seqlens, int32_t nseg,
                             uint16_t* out, int64_t TP, int32_t heads, float softcap, void* ws, size_t ws_bytes, void* stream);
/* Kernel-level access to the SPLIT forms of the fp32 and the split-precision attention that few-token rap_sample / rap_dit_forward calls
 * run (tuning key 5): every work item is cut into `splits` key ranges (1, 2 or 4; anything else: RAP_ERR_INVALID), each range writes its
 * un-normalised partial output and row sums to the workspace, and one combine pass merges them in a fixed order (deterministic).
 * splits = 1 is rap_attention_f32 / rap_x2_attention, bit for bit.  Rows outside [cu_seqlens[0], cu_seqlens[nseg]) come out as ZEROS
 * when splits > 1 (the combine pass covers every row of out).
 * rap_attention_split_workspace_bytes: rap_attention_workspace_bytes(TP, nseg) plus, for splits > 1, splits x TP x heads x 64 floats of
 *   partial outputs and splits x TP x heads x 2 floats of (maximum, row sum) -- the split-precision need; the fp32 form uses half of the
 *   second plane.  0 for heads <= 0, TP < 0, nseg < 0 or a splits value that is none of 1, 2, 4.
 * rap_attention_f32_split: only the bounded softmax can add partial results: splits > 1 without logit_bound is RAP_ERR_INVALID; a head
 *   whose bound is above 40 gets NaN outputs, as in rap_attention_f32.
 * rap_x2_attention_split: n_tokens (0 <= n_tokens <= TP; 0 = TP) is the number of rows the combine pass of splits > 1 writes -- rows
 *   n_tokens .. TP - 1 of out are not touched (the filler rows of rap_sample's padded buffers); cu_seqlens must not reach beyond it.
 * A workspace below the query's value is RAP_ERR_WORKSPACE before anything is written. */
size_t rap_attention_split_workspace_bytes(int64_t TP, int32_t nseg, int32_t heads, int32_t splits);
int rap_attention_f32_split(const float* qkv_headmajor, const int32_t* cu_seqlens, int32_t nseg, float* out, int64_t TP,
                            int32_t heads, const float* logit_bound, int32_t splits, void* ws, size_t ws_bytes, void* stream);
/* The fp32 kernels that run between the GEMMs of a flow step.  Every argument is checked before any launch, whatever the row count:
 * RAP_ERR_INVALID for a NULL required operand, a negative row count or one that does not fit the launchers' int (never truncated), d not
 * one of 256, 512, 768, 1024, heads <= 0, feat_dim outside {0, 4, ..., 40} or feat == NULL with feat_dim > 0, inner <= 0 / inner % 32 != 0 /
 * K <= 0 for rap_geglu_interleave.  Zero rows with valid arguments: RAP_OK, nothing written. */
int rap_layernorm_mod(const float* x, float* out, int64_t TP, int32_t d, const float* mod, int64_t mod_stride,
                      const int32_t* token_row, void* stream);
int rap_layernorm_affine(const float* x, float* out, int64_t TP, int32_t d, const float* gain, const float* shift,
                         void* stream);
int rap_qknorm(float* qkv_headmajor, int64_t TP, int32_t heads, const float* gamma_q, const float* gamma_k, void* stream);
int rap_posenc_x(const float* x, float* ax, int64_t TP, void* stream);
int rap_posenc_static(const float* cond, const float* scales, const int32_t* token_sample, const float* feat,
                      int32_t feat_dim, float* astatic, int64_t TP, void* stream);
int rap_token_sample(const int32_t* cu_batch, int32_t B, int32_t* token_sample, void* stream);
/* The small kernels of rap_sample / rap_model_create that have no other entry point (for the parity tests; same launchers, same checks
 * as above).
 * rap_head_out3: v (TP, 3) = y (TP, K; row stride ldy >= K, ldy % 4 == 0) W (3, K)^T, the last layer of the output head; K one of 128, 256,
 *   384, 512.
 * rap_max_abs: *out = max(*out, max_i |x[i]|) as fp32 bits -- *out must hold +0 before the call; NaN entries are ignored, n = 0 leaves it.
 * rap_qk_logit_bound: out[h] = 8 max|gamma_q[h]| max|gamma_k[h]| * 1.001 for gamma (heads, 64): the logit bound rap_sample hands the
 *   bounded-softmax attention after qk-norm (see rap_attention_h16 for what it guarantees).
 * rap_sanitize_cu: out[i] = max_{j <= i} clamp(cu[j], 0, limit) for i < n: a segment table made safe to index with (a consistent table is
 *   returned unchanged); 0 <= limit <= INT32_MAX. */
int rap_head_out3(const float* y, int32_t ldy, const float* W, float* v, int64_t TP, int32_t K, void* stream);
int rap_max_abs(const float* x, int64_t n, float* out, void* stream);
int rap_qk_logit_bound(const float* gamma_q, const float* gamma_k, int32_t heads, float* out, void* stream);
int rap_sanitize_cu(const int32_t* cu, int32_t n, int64_t limit, int32_t* out, void* stream);
/* adaLN (scale|shift) table for model `m`: t (rows,), out (rows, 2*num_layers, 2*embed_dim);
 * scratch >= rows*(256 + 4*num_layers*embed_dim) floats. */
int rap_adaln_table(const rap_model* m, const float* t, int32_t rows, float* scratch, float* out, void* stream);


/* ---- reduced-precision kernel-level entry points (dtype 1 = bf16, 2 = fp16; 16-bit tensors as uint16_t*) ---- */
/* dst[i] = round-to-nearest-even(src[i]) for i < n.  n % 4 == 0 (values move four at a time; any other n: RAP_ERR_INVALID before any launch). */
int rap_convert_h16(int32_t dtype, const float* src, uint16_t* dst, int64_t n, void* stream);
/* C = A (M,K) W(N,K)^T, fp32 accumulate.  epilogue: 0 C half = acc + bias; 1 C fp32 = (resid +) acc + bias;
 * 7 C fp16 = fp16(resid + acc + bias) with `resid` pointing at an FP16 (M,N) matrix (required; row stride ldr; may alias C): the residual GEMM
 * of the 16-bit residual stream, one rounding of the fp32 sum (saturating at +-65504), fp16 whatever the operand dtype
 * (6 -- this epilogue's number before ABI version 4, and a different epilogue before that -- is refused);
 * 3 GEGLU on value/gate-interleaved W (C half (M,N/2)); 4 qkv split: q,k -> C half [2][H][M][64], v -> vt, the
 * TRANSPOSED image [H][vt_nblk][64 d][64 pos] the attention kernel consumes: token t sits in block t >> 6 at
 * pos = (t & 51) | ((t & 4) << 1) | ((t & 8) >> 1); vt_nblk * 64 >= M rounded up to 256; every row from M up to M rounded up to 256 is
 * written as 0, by whichever kernel the shape selects (blocks beyond that, if vt_nblk is larger, are not touched). */
int rap_gemm_h16(int32_t dtype, int32_t epilogue, const uint16_t* A, int32_t lda, const uint16_t* W, int32_t ldw, void* C,
                 int32_t ldc, int32_t M, int32_t N, int32_t K, const float* bias, const float* resid, int32_t ldr,
                 int32_t heads, uint16_t* vt, int32_t vt_nblk, void* stream);
/* Epilogues 1 and 7 of rap_gemm_h16 with the split-K form rap_sample uses for the K = 4d feed-forward GEMM of few-token calls (tuning
 * key 6): when rap_gemm_h16_splitk_workspace_bytes(M, N, K) > 0 (K >= 1024 and at most 128 tiles of 128 x 128), K is split over 2 or 4
 * blocks per tile that write fp32 partial tiles to ws, and a combine pass forms resid + (bias + sum of partials) in a fixed order
 * (deterministic; equals the unsplit result up to the fp32 association of the k-sum).  resid: fp32 (epilogue 1, may be NULL) or fp16
 * (epilogue 7, required) (M,N) matrix with row stride ldr, may alias C.  With a workspace size of 0 the call is rap_gemm_h16. */
size_t rap_gemm_h16_splitk_workspace_bytes(int32_t M, int32_t N, int32_t K);
int rap_gemm_h16_splitk(int32_t dtype, int32_t epilogue, const uint16_t* A, int32_t lda, const uint16_t* W, int32_t ldw, void* C,
                        int32_t ldc, int32_t M, int32_t N, int32_t K, const float* bias, const void* resid, int32_t ldr, void* ws,
                        size_t ws_bytes, void* stream);
/* flash_attn_varlen_qkvpacked_func equivalent on 16-bit operands (fp32 softmax): qk [2][H][TP][64], vt as above,
 * out half (TP, H*64).  ws >= rap_attention_workspace_bytes(TP, nseg).
 * logit_bound: NULL, or H device floats B[h] with q.k/8 <= B[h] <= 40 for every query/key pair of head h GUARANTEED by
 * the caller (after the reference's qk-norm B = 8 max|gamma_q| max|gamma_k|): selects the bounded-softmax kernel
 * (p = exp(s - B), no running maximum; bf16 only -- other dtypes ignore it).  Same softmax, different evaluation order.
 * What rap_qk_logit_bound's B = 8 max|gamma_q| max|gamma_k| * 1.001 guarantees for the q, k the qk-norm kernels WRITE: q.k/8 <= B when
 * they are fp32 or fp16 (two operand roundings of at most 2^-11 fit the 0.1 % slack); in bf16 the two roundings of up to 2^-8 can carry
 * q.k/8 up to B (1 + 2^-7) -- harmless here (exp(s - B) <= exp(0.31) at B = 40, nowhere near overflow), so the slack is not widened.
 * (Inside rap_sample / rap_dit_forward the bf16 path additionally has qk-norm write q pre-scaled by log2(e)/8 and drops the
 * offset: p = exp2(q'.k); this entry point keeps the un-scaled q convention.) */
/* The QKV projection with the reference's MultiHeadRMSNorm (flow_model/norm.py:28-33) fused into its epilogue -- what rap_sample /
 * rap_dit_forward run in the 16-bit modes (tuning key 7 = 0 restores GEMM + rap_qknorm_h16): q, k rows are normalised from the fp32
 * accumulators, multiplied by gamma and by q_mul (q) or 8 (k), then rounded ONCE to 16 bit into qk_out [2][H][M][64]; v goes to the
 * transposed image vt exactly as epilogue 4 of rap_gemm_h16.  N = 3 * heads * 64, K % 64 == 0, K >= 128. */
int rap_gemm_h16_qkvnorm(int32_t dtype, const uint16_t* A, int32_t lda, const uint16_t* W, int32_t ldw, uint16_t* qk_out, int32_t M,
                         int32_t K, int32_t heads, const float* gamma_q, const float* gamma_k, float q_mul, uint16_t* vt,
                         int32_t vt_nblk, void* stream);
int rap_attention_h16(int32_t dtype, const uint16_t* qk, const uint16_t* vt, int32_t vt_nblk, const int32_t* cu_seqlens,
                      int32_t nseg, uint16_t* out, int64_t TP, int32_t heads, const float* logit_bound, void* ws,
                      size_t ws_bytes, void* stream);
int rap_layernorm_mod_h16(int32_t dtype, const float* x, uint16_t* out, int64_t TP, int32_t d, const float* mod,
                          int64_t mod_stride, const int32_t* token_row, void* stream);
int rap_layernorm_affine_h16(int32_t dtype, const float* x, uint16_t* out, int64_t TP, int32_t d, const float* gain,
                             const float* shift, void* stream);
/* Kernel-level access to the residual-stream side of the 16-bit block, for the parity tests (no kernel of their own).
 * rap_layernorm_mod_h16_stream / rap_layernorm_affine_h16_stream: the two calls above with the residual-stream dtype exposed: x is fp32
 *   (TP, d) when x_f16 = 0 -- then they ARE the calls above, bit for bit -- or fp16 (TP, d) when x_f16 = 1 (dtype 1, 2 only).
 * rap_resid_combine_layernorm_h16: the combine pass of a split-K residual GEMM and the LayerNorm that follows it in one launch, as few-token
 *   model calls run them (tuning key 19).  part: `splits` (1..8) fp32 planes [splits][rows][d]; bias: d floats or NULL; h: the residual
 *   stream (rows, d), fp32 (h_f16 = 0) or fp16 (h_f16 = 1; dtype 1, 2 only), updated IN PLACE:
 *     h = ((0 + part[0] + part[1] + ...) + bias) + h   in fp32, in this order; an fp16 stream takes ONE rounding of that sum, saturating at
 *     +-65504 (+-inf -> +-65504, NaN stays NaN);
 *   out = LayerNorm of the STORED h (eps 1e-5), modulated as rap_layernorm_mod_h16 does when mod != NULL (mod_stride, token_row as there),
 *   else affine with gain and shift (both required then) -- bit-identical to the combine pass followed by the plain LayerNorm.  out is
 *   (rows, d) in the operand type, (rows, 2 d) paired for dtype 3.  Nothing but h[:rows] and out[:rows] is written.
 * rap_convert_f16_sat: dst fp16 [n] = round-to-nearest-even(clamp(src fp32 [n], -65504, 65504)), NaN stays NaN; n % 4 == 0.
 * rap_convert_f16_to_f32: dst fp32 [n] = src fp16 [n], exact (a signalling NaN leaves quiet, payload kept); n % 8 == 0.
 * Refused with RAP_ERR_INVALID before any launch, WHATEVER the row count: a NULL required operand; dtype outside 1..3; dtype 3 with an fp16
 * stream; x_f16 / h_f16 outside {0, 1}; d not one of 256, 512, 768, 1024; splits outside 1..8; neither mod nor both of gain and shift;
 * a negative row count or n; n % 4 != 0 (sat) / n % 8 != 0 (to_f32).  rows = 0 / n = 0 with valid arguments: RAP_OK, nothing written. */
int rap_layernorm_mod_h16_stream(int32_t dtype, const void* x, int32_t x_f16, uint16_t* out, int64_t TP, int32_t d, const float* mod,
                                 int64_t mod_stride, const int32_t* token_row, void* stream);
int rap_layernorm_affine_h16_stream(int32_t dtype, const void* x, int32_t x_f16, uint16_t* out, int64_t TP, int32_t d, const float* gain,
                                    const float* shift, void* stream);
int rap_resid_combine_layernorm_h16(int32_t dtype, const float* part, int32_t splits, const float* bias, void* h, int32_t h_f16,
                                    uint16_t* out, int64_t rows, int32_t d, const float* mod, int64_t mod_stride, const int32_t* token_row,
                                    const float* gain, const float* shift, void* stream);
int rap_convert_f16_sat(const float* src, uint16_t* dst, int64_t n, void* stream);
int rap_convert_f16_to_f32(const uint16_t* src, float* dst, int64_t n, void* stream);
int rap_qknorm_h16(int32_t dtype, uint16_t* qk, int64_t TP, int32_t heads, const float* gamma_q, const float* gamma_k,
                   void* stream);

/* ---- split-precision kernel-level entry points (compute dtype 3, round 5) ----
 * PAIRED layout of a split fp32 matrix (rows, K): (rows, 2K) fp16; logical column k sits at physical column 64 (k >> 5) + (k & 31) as
 * its fp16 head, and 32 columns further as its fp16 tail -- every 32-column chunk is one 128-byte line [32 heads | 32 tails].  K % 32 == 0.
 * rap_x2_pack:   dst = split(src * scale)  (src fp32 (rows, cols), row stride ld_src; scale a power of two for weights, 1 otherwise).
 * rap_x2_unpack: dst fp32 (rows, cols) = (head + tail) * inv_scale.
 * rap_x2_gemm:   C = A (M,K) W(N,K)^T from paired A (M, lda) and W (N, ldw), K_physical = 2 K (>= 128, % 64 == 0), lda, ldw >= K_physical and % 8 == 0,
 *   N % 256 == 0 (anything else: RAP_ERR_INVALID before any launch); the accumulators are
 *   multiplied by acc_scale (the inverse of the weight planes' scale) before the epilogue:
 *     1  C fp32 (M,N) = resid + acc + bias (resid may be NULL / alias C; ldc, ldr >= N and % 4 == 0: rows move as 16-byte pieces);
 *     3  GEGLU on value/gate-interleaved W: C paired (M, ldc >= N, ldc % 8 == 0) holds the N/2 outputs (h + bh) * gelu_erf(g + bg);
 *     5  QKV projection with MultiHeadRMSNorm fused (N = 3 * heads * 64): q, k -> C paired [2][heads][2 chunks][M][64 physical] (chunk c =
 *        head dims 32c .. 32c+31; q multiplied by q_mul, k by 8 as in rap_gemm_h16_qkvnorm; gamma_q = gamma_k = NULL: no norm, q and k
 *        leave as projected -- qk_norm = False), v -> vt paired
 *        [heads][vt_nblk][2 chunks][64 d][64 physical]: token t sits in block t >> 6, chunk (t >> 5) & 1, at in-chunk position
 *        p = (t & 19) | ((t & 4) << 1) | ((t & 8) >> 1) as head (column p) and tail (column 32 + p); vt_nblk * 64 >= M rounded up to 256.
 * rap_x2_attention: flash_attn_varlen_qkvpacked_func on those planes (online softmax in fp32): out paired (TP, 2 * heads * 64).
 *   ws >= rap_attention_workspace_bytes(TP, nseg).
 * LayerNorm with paired output: rap_layernorm_mod_h16 / rap_layernorm_affine_h16 with dtype 3 (out is (TP, 2 d)). */
int rap_x2_pack(const float* src, int64_t ld_src, int64_t rows, int32_t cols, float scale, uint16_t* dst, void* stream);
int rap_x2_unpack(const uint16_t* src, int64_t rows, int32_t cols, float inv_scale, float* dst, void* stream);
int rap_x2_gemm(int32_t epilogue, const uint16_t* A, int32_t lda, const uint16_t* W, int32_t ldw, void* C, int32_t ldc, int32_t M, int32_t N,
                int32_t K_physical, const float* bias, const float* resid, int32_t ldr, float acc_scale, int32_t heads, const float* gamma_q,
                const float* gamma_k, float q_mul, uint16_t* vt, int32_t vt_nblk, void* stream);
int rap_x2_attention(const uint16_t* qk, const uint16_t* vt, int32_t vt_nblk, const int32_t* cu_seqlens, int32_t nseg, uint16_t* out,
                     int64_t TP, int32_t heads, void* ws, size_t ws_bytes, void* stream);
/* rap_x2_attention over `splits` key ranges per work item: see rap_attention_split_workspace_bytes above. */
int rap_x2_attention_split(const uint16_t* qk, const uint16_t* vt, int32_t vt_nblk, const int32_t* cu_seqlens, int32_t nseg,
                           uint16_t* out, int64_t TP, int64_t n_tokens, int32_t heads, int32_t splits, void* ws, size_t ws_bytes,
                           void* stream);

/* ---- input side of the boundary: raw multi-part scans -> the packed batch rap_sample consumes ----
 * Replaces, in their evaluation-split form (no augmentation), PointCloudDataset._transform
 * (rectified_point_flow/data/dataset.py:733-900) and variable_collate_fn (data/datamodule.py:169-198) for a whole batch, on the
 * device: per sample the frame of the largest ("primary" = anchor) part -- centred on its centroid, scaled by 1.5 x its largest
 * |coordinate| -- then global centring; per part the centred cloud (cond), its pose (R = I, t = centroid; anchor: t = -gt_trans),
 * the anchor masks, and the collated cu_seqlens.  fp64 arithmetic like numpy, fp32 results.
 *   points (TP,3) fp32 or fp64 (points_are_f64), parts of a sample contiguous, samples contiguous; points_per_part (B,P) int64 on
 *   the device, 0 = padding (anywhere in the row: zero rotation / translation rows, never the anchor); every sample needs at least
 *   one point to be usable -- one without any gets scale 0, global translation 0, zero rows and no anchor, and does not disturb the others.
 *   order: NULL, or (TP,) int64 -- for every output point its source index INSIDE its part (what np.random.permutation returned
 *   for that part, dataset.py:819); order_flag: NULL or a device int32 the call ORs 1 into when an index is out of range (such an
 *   index is clamped into its part before it is used: the outputs are then not a permutation, but nothing outside the part is read).
 *   outputs: cond, gt (TP,3) f32; feat_out (TP,F) f32 (feat_in gathered the same way; F may be 0); anchor_indices (TP,) u8;
 *   part_indices (TP,) i64; rotations (B,P,3,3), translations (B,P,3), scales (B,), anchor_parts (B,P) u8,
 *   global_translation (B,3) f32 (mean of the raw sample, original units), cu_seqlens (B+1,) i64.
 *   ws >= rap_collate_workspace_bytes(B, P).  Three launches, no host synchronisation. */
size_t rap_collate_workspace_bytes(int32_t B, int32_t P);
int rap_collate_transform(const void* points, int32_t points_are_f64, const int64_t* points_per_part, int32_t B, int32_t P,
                          int64_t TP, const int64_t* order, const float* feat_in, int32_t F, float* cond, float* gt,
                          float* feat_out, uint8_t* anchor_indices, int64_t* part_indices, float* rotations, float* translations,
                          float* scales, uint8_t* anchor_parts, float* global_translation, int64_t* cu_seqlens,
                          int32_t* order_flag, void* ws, size_t ws_bytes, void* stream);

/* Statistical outlier removal in front of FPS / MiniSpinNet: Open3D's PointCloud.remove_statistical_outlier(nb_neighbors, std_ratio)
 * as dataset_process/extract_sample_features.py:378-385 calls it (20, 2.5).  Open3D is not in the reference mount; the kernel follows
 * its published rule (mean distance to the nb_neighbors nearest points INCLUDING the point itself; threshold = mean + std_ratio *
 * Bessel-corrected std over the cloud; inlier = 0 < d < threshold): parity unpinned.  points (N,3) f32; nb_neighbors <= 32;
 * inlier_indices (>= N int64, ascending), count_out (device int32), stats_out NULL or 3 device doubles {mean, std, threshold};
 * ws >= rap_outlier_workspace_bytes(N).  Brute-force k-NN through the LDS (N^2 pair distances), no host synchronisation. */
size_t rap_outlier_workspace_bytes(int64_t N);
int rap_statistical_outliers(const float* points, int64_t N, int32_t nb_neighbors, double std_ratio, int64_t* inlier_indices,
                             int32_t* count_out, double* stats_out, void* ws, size_t ws_bytes, void* stream);
/* rap_statistical_outliers with its neighbour search on the uniform-grid index: the same argument list and the same rule.  Only the
 * first of its five kernels differs: the mean of sqrtf(d2) over the nb_neighbors smallest d2 of every point (itself included; -1
 * where there is none) comes from the k-best walk of rap_k_nearest_neighbors, summed in double in ascending order as the brute-force
 * kernel sums it; statistics, count, scan and emit are the same kernels.  O(N) work in place of N^2 pair distances: for raw scans.
 * The index is built once per call on the device; no host synchronisation, deterministic.
 * ws >= rap_outlier_grid_workspace_bytes(N) (host arithmetic, 0 for N <= 0: rap_outlier_workspace_bytes plus about 28 bytes per point). */
size_t rap_outlier_grid_workspace_bytes(int64_t N);
int rap_statistical_outliers_grid(const float* points, int64_t N, int32_t nb_neighbors, double std_ratio, int64_t* inlier_indices,
                                  int32_t* count_out, double* stats_out, void* ws, size_t ws_bytes, void* stream);

/* Consistency of a packed batch -- what the reference asserts in split_parts (utils/point_clouds.py:33-52).  rap_sample and the
 * Procrustes entry points REQUIRE sum(points_per_part) == TP and, per sample, sum_p points_per_part[b][p] == cu_seqlens[b+1] -
 * cu_seqlens[b]; they do not read anything back to check it (rap_sample clamps the part table to TP, so a malformed batch gives
 * wrong poses, not an out-of-bounds access).  This entry point writes the verdict to a device int32: 0 = consistent; bit 0 sum
 * != TP, bit 1 cu_seqlens ends, bit 2 cu_seqlens decreasing, bit 3 a sample's parts vs its span, bit 4 a negative size. */
int rap_check_batch(const int64_t* points_per_part, const int32_t* cu_batch, int32_t B, int32_t P, int64_t TP, int32_t* flag_out,
                    void* stream);
/* The deferred form of that check (no host read-back on the call path): enqueue rap_check_batch, the sampling call, then
 * rap_poison_on_flag on every result buffer -- if *flag (device int32, as rap_check_batch wrote it) is non-zero, buf[0..n) is
 * overwritten with NaN, so results of an inconsistent batch cannot be mistaken for poses.  rap_amd.RectifiedPointFlow does this by
 * default and raises on the host the first time it can read the flag without stalling the stream. */
int rap_poison_on_flag(const int32_t* flag, float* buf, int64_t n, void* stream);

/* ---- measurement hooks (bench.py roofline leg) ----
 * When enabled, every attention and layer-GEMM launch inside rap_dit_forward / rap_sample is bracketed by two
 * hipEvents recorded on the launch stream.  rap_profile_collect synchronises on them and returns, per class
 * (0 attention per part, 1 attention per sample, 2 layer GEMMs), the summed milliseconds and the launch count
 * into HOST arrays of 3 entries.  rap_profile_collect_ex (round 5) takes n_classes entries and also reports the HBM-bound ring:
 * 3 LayerNorm, 4 posenc(x_t), 5 Euler update, 6 Procrustes moments + solve, 7 rigid apply / blend (8 classes in all).
 * Off by default; the state is process-global behind a mutex (safe to call from several threads, the figures are per process). */
int rap_profile_enable(int on);
int rap_profile_collect_ex(float* h_ms_out, int64_t* h_count_out, int32_t n_classes);
/* Production switches between two SHIPPED code paths that compute the same function (process-global, atomic; not per model):
 *   key 5  split-KV attention for few-token calls        {0 off, 1 on (default)}       fp32 path and split precision
 *   key 6  split-K of the bias + residual GEMM, few rows  {0 off, 1 on (default)}       every precision (16-bit / split precision: K >= 1024, i.e. ff2)
 *   key 7  qk-norm fused into the QKV GEMM epilogue       {1 (default), 0 = own kernel} both precisions
 *   key 9  GEGLU's Phi                                    {1 (default): erfc polynomial, |error| <= 1.5e-7; 0: erff}   fp32 path
 *   key 11 persistent 16-bit GEMM (one block per CU walks {1 (default), 0 = one 256 x 256 tile per block}   16-bit path
 *          its XCD's tiles; full-tile shapes only)
 *   key 12 persistent fp32 GEMM (same, 256 x 256 kernel)  {1 (default), 0 = one tile per block}              fp32 path
 *   key 13 16-bit attention: K / V^T tiles by LDS-DMA      {1 (default), 0 = staged through registers}       16-bit path
 *   key 15 attention work lists of rap_sample / forward    {1 (default): longest segment first, 0: segment order}   both precisions
 *   key 16 split-precision attention: blocks per CU          {2 (default): one 8-wave block, 4: two}                 compute dtype 3
 *   key 17 split precision from this many token rows per call {1024 (default); 0 = always}: SMALLER calls of a model in compute dtype 3
 *          run the exact-fp32 kernels (both are fp32-accurate; below a few thousand tokens the fp32 path's few-token forms are faster).
 *          rap_workspace_bytes of such a model covers both layouts, so the key may change between the size query and the call
 *   key 18 four-stage LDS-DMA ring of the 128 x 128 16-bit / split-precision GEMM (few-token calls) for launches of at most this many
 *          blocks {256 (default); 0 = never: two stages, two blocks per CU}.  Bit-identical results.
 *   key 19 few-token 16-bit / split-precision calls: the combine pass of every residual GEMM folded into the LayerNorm that follows it
 *          {1 (default), 0 = the round-5 launch sequence}.  Bit-identical in the 16-bit modes; in split precision the fused sequence
 *          also splits K of the out-projection (fp32-class agreement)
 *   key 20 16-bit attention of few-token calls (<= 4 096 token rows)
 *          {1 (default): the eight waves of a block are query waves x KEY GROUPS -- work items of 64 rows x 4 key groups up to 2 048 token
 *             rows, 128 rows x 2 key groups up to 4 096; the groups' partial (O, l, m) meet in LDS, nothing extra leaves the CU.  The keys of a
 *             row are summed in another order than by the unsplit kernel: deterministic, same error bound, not bit-identical to it;
 *           2: work items of 128 rows and a four-stage K / V^T ring, no key groups -- bit-identical to 0;
 *           0: 256-row items, two stages (round 5);
 *           64 / 128: that item size + ring, 66 / 130: 64 rows x 4 / 128 rows x 2 key groups -- forced for every call of at most 8 192 token
 *             rows AND for rap_attention_h16 (the A/B values)}.  (rap_workspace_bytes does not depend on it.)
 *   key 22 rap_farthest_point_sampling_grid: points per bucket {32 (default), 1, 8, 16, 48, 64, 128}.  Bit-identical results.
 *   key 23 rap_farthest_point_sampling_grid: threads of the one block per cloud {512 (default), 256, 1024}.  Bit-identical results.
 * Operand range of compute dtype 3 (and of the fp16 residual stream): every paired activation -- LayerNorm output, q / k (also without
 * qk-norm), v, attention output, GEGLU output -- is clipped to +-65 504 before it is split into head and tail (NaN stays NaN), and
 * rap_model_set_compute_dtype(3) refuses weights that are not finite.  scripts/check_checkpoint.py compares the mode with exact fp32 on
 * the weights it is given and exits non-zero on a miss.
 * Any other key returns RAP_ERR_INVALID.  (Keys 0-4 selected among the kernel variants of the round-1/2 experiments; those variants
 * are no longer in the tree, and what is left of the switch exists only in a library built with -DRAP_ABLATION_BUILD.) */
int rap_set_tuning(int32_t key, int32_t value);
int rap_profile_reset(void);
int rap_profile_collect(float* h_ms_out, int64_t* h_count_out);

#ifdef __cplusplus
}
#endif
#endif /* RAPFLOW_H */
