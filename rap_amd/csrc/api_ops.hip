// C ABI of librapflow, second part (see include/rapflow.h): the entry points that are thin bindings over one kernel file each --
// kernel-level GEMM / attention / LayerNorm calls, rigidity, overlap, MiniSpinNet, nn / pair metrics, voxel, collate, outlier.
// Host code only; the model, its workspace and the sampling loop are in api.hip.
#include "../../include/rapflow.h"
#include "half.h"
#include "kernels.h"
#include "fps_grid.h"
#include "softcap.h"

#include <cmath>
#include <new>
#include <vector>

// ---------------------------------------------------------------------------------------------
// kernel-level entry points
// ---------------------------------------------------------------------------------------------
extern "C" int rap_gemm_f32(int32_t epilogue, const float* A, int32_t lda, const float* W, int32_t ldw, float* C, int32_t ldc,
                            int32_t M, int32_t N, int32_t K, const float* bias, const float* resid, int32_t ldr,
                            const uint8_t* anchor, const float* anchor_emb, int32_t heads, void* stream) {
  if (!A || !W || !C) return RAP_ERR_INVALID;
  if (epilogue == EPI_BIAS_RESID && !resid) return RAP_ERR_INVALID;
  if (epilogue == EPI_BIAS_ANCHOR && (!anchor || !anchor_emb)) return RAP_ERR_INVALID;
  GemmParams g{};
  g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K; g.bias = bias;
  g.resid = resid; g.ldr = ldr; g.anchor = anchor; g.anchor_emb = anchor_emb; g.heads = heads;
  return launch_gemm_f32((hipStream_t)stream, epilogue, g);
}

// the dispatch decision of rap_gemm_f32 / the model's fp32 GEMMs as host arithmetic (kernels.h: the form codes)
extern "C" int rap_gemm_f32_form(int32_t epilogue, int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldw, int32_t ldc, int32_t ldr,
                                 int32_t has_ws, int32_t planes) {
  static float ws_given;      // (never dereferenced: the form only asks whether a workspace was handed in)
  GemmParams g{};
  g.lda = lda; g.ldw = ldw; g.ldc = ldc; g.ldr = ldr; g.M = M; g.N = N; g.K = K;
  g.splitk_ws = has_ws ? &ws_given : nullptr; g.splitk_planes = planes;
  return gemm_f32_form(epilogue, g);
}
// the residual (1) and SiLU (2) epilogues with the split-K workspace rap_sample hands them on few-token calls
extern "C" size_t rap_gemm_f32_splitk_workspace_bytes(int32_t epilogue, int32_t M, int32_t N, int32_t K, int32_t planes) {
  const int s = gemm_f32_splits_by_shape(epilogue, M, N, K, planes);
  if (s <= 1) return 0;
  return (size_t)(epilogue == EPI_BIAS_RESID ? 4 : planes) * (size_t)M * (size_t)N * sizeof(float);
}
extern "C" int rap_gemm_f32_splitk(int32_t epilogue, const float* A, int32_t lda, const float* W, int32_t ldw, float* C, int32_t ldc, int32_t M,
                                   int32_t N, int32_t K, const float* bias, const float* resid, int32_t ldr, int32_t planes, void* ws,
                                   size_t ws_bytes, void* stream) {
  if (!A || !W || !C || (epilogue != EPI_BIAS_RESID && epilogue != EPI_BIAS_SILU)) return RAP_ERR_INVALID;
  if (epilogue == EPI_BIAS_RESID && !resid) return RAP_ERR_INVALID;
  if (epilogue == EPI_BIAS_SILU && planes != 2 && planes != 4) return RAP_ERR_INVALID;
  const size_t need = rap_gemm_f32_splitk_workspace_bytes(epilogue, M, N, K, planes);
  if (need && (!ws || ws_bytes < need)) return RAP_ERR_WORKSPACE;
  GemmParams g{};
  g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K; g.bias = bias;
  g.resid = resid; g.ldr = ldr;
  g.splitk_ws = need ? reinterpret_cast<float*>(ws) : nullptr;
  g.splitk_planes = need && epilogue == EPI_BIAS_SILU ? planes : 0;
  return launch_gemm_f32((hipStream_t)stream, epilogue, g);
}

extern "C" int rap_geglu_interleave(const float* W, const float* b, float* Wp, float* bp, int32_t inner, int32_t K,
                                    void* stream) {
  if (!W || !b || !Wp || !bp || inner <= 0 || inner % 32 != 0 || K <= 0) return RAP_ERR_INVALID;
  return launch_geglu_interleave((hipStream_t)stream, W, b, Wp, bp, inner, K);
}

// [work items | sanitised copy of the caller's cu_seqlens]: the kernel-level attention entry points index with the copy only (ADVICE r05:
// an entry above TP in the caller's table made seg_start + q run past the planes; the model path has sanitised its tables since round 5)
// (work items reserved at the smallest granularity, 64 rows: tuning key 20's forced item sizes reach rap_attention_h16 too).
// The split-KV forms (splits > 1) put their partial planes behind the two tables:
// [partial O: splits x TP x heads x 64 floats | (max, row sum): splits x TP x heads x 2 floats] (the fp32 form keeps its row sums in the
// first half of the last plane)
struct AttnWs { AttnWorkItem* items; int max_items; int32_t* cu_s; float *part_o, *part_ml; size_t total; };
static AttnWs carve_attn(int64_t TP, int32_t nseg, int32_t heads, int32_t splits, void* base) {
  AttnWs p{}; Carver c(base);
  p.items = (AttnWorkItem*)c.take(((size_t)(TP / 64) + (size_t)nseg + 1) * sizeof(AttnWorkItem));
  p.cu_s = (int32_t*)c.take(((size_t)nseg + 1) * sizeof(int32_t));
  if (splits > 1) {
    p.part_o = (float*)c.take((size_t)splits * (size_t)TP * (size_t)heads * 64 * sizeof(float));
    p.part_ml = (float*)c.take((size_t)splits * (size_t)TP * (size_t)heads * 2 * sizeof(float));
  }
  p.total = c.total();
  return p;
}
extern "C" size_t rap_attention_workspace_bytes(int64_t TP, int32_t nseg) { return carve_attn(TP, nseg, 0, 1, nullptr).total; }
// What the attention entry points start with, after their own pointer checks: the segment-table and workspace checks (tp_max: the
// entry point's limit on TP), the carved workspace (heads, splits: the split forms' partial planes), the clamped, non-decreasing copy of
// cu_seqlens inside it, and from that the work list with bq query rows per item (0: the fp32 kernel's own granularity; the list then
// holds room for 256-row items) and w->max_items for the launch
static int attn_begin(hipStream_t stream, const int32_t* cu_seqlens, int32_t nseg, int64_t TP, int64_t tp_max, void* ws, size_t ws_bytes,
                      int bq, AttnWs* w, int32_t heads = 0, int32_t splits = 1) {
  if (!cu_seqlens || nseg < 0 || TP < 0 || TP > tp_max) return RAP_ERR_INVALID;
  *w = carve_attn(TP, nseg, heads, splits, ws);
  if (!ws || ws_bytes < w->total) return RAP_ERR_WORKSPACE;
  w->max_items = (int)(TP / (bq ? bq : RAP_ATTN_BQ)) + nseg + 1;
  const int rc = launch_sanitize_cu(stream, cu_seqlens, nseg + 1, (long)TP, w->cu_s);
  return rc ? rc : launch_build_attn_worklist(stream, w->cu_s, nseg, w->items, w->max_items, bq);
}

// the work list of one attention launch as rap_sample / rap_dit_forward build it: one {seg_start, seg_len, q0, 0} item per
// `block_queries` query rows of every segment, longest segment first when sort_ws (nseg ints) is given, zero items after the last
extern "C" int rap_build_attention_worklist(const int32_t* cu_seqlens, int32_t nseg, int32_t block_queries, int32_t* items_out,
                                            int32_t max_items, int32_t* sort_ws, void* stream) {
  if (!cu_seqlens || !items_out || nseg < 0 || max_items < 0 || block_queries <= 0) return RAP_ERR_INVALID;
  return launch_build_attn_worklist((hipStream_t)stream, cu_seqlens, nseg, reinterpret_cast<AttnWorkItem*>(items_out), max_items,
                                    block_queries, sort_ws);
}

extern "C" int rap_attention_f32(const float* qkv_headmajor, const int32_t* cu_seqlens, int32_t nseg, float* out,
                                 int64_t TP, int32_t heads, const float* logit_bound, void* ws, size_t ws_bytes,
                                 void* stream_) {
  if (!qkv_headmajor || !out) return RAP_ERR_INVALID;
  hipStream_t stream = (hipStream_t)stream_;
  AttnWs w;
  if (int rc = attn_begin(stream, cu_seqlens, nseg, TP, 0x7fffffffLL / 8, ws, ws_bytes, 0, &w)) return rc;
  return launch_attention_f32(stream, qkv_headmajor, out, (int)TP, heads, w.items, w.max_items, logit_bound, nullptr, nullptr, 1);
}

// the soft-capped kernels of a model with rap_model_set_softcap (one launch form each: 256-row items, unsplit; softcap_ok: softcap.h)
extern "C" int rap_attention_f32_softcap(const float* qkv_headmajor, const int32_t* cu_seqlens, int32_t nseg, float* out, int64_t TP,
                                         int32_t heads, float softcap, void* ws, size_t ws_bytes, void* stream_) {
  if (!qkv_headmajor || !out || heads <= 0 || !softcap_ok(softcap)) return RAP_ERR_INVALID;
  hipStream_t stream = (hipStream_t)stream_;
  AttnWs w;
  if (int rc = attn_begin(stream, cu_seqlens, nseg, TP, 0x7fffffffLL / 8, ws, ws_bytes, 0, &w)) return rc;
  return launch_attention_f32_softcap(stream, qkv_headmajor, out, (int)TP, heads, w.items, w.max_items, softcap);
}

// The split-KV forms few-token model calls run (attention_f32_splits / attention_x2_splits pick them there), for the parity tests
// (workspace: carve_attn)
static bool attn_splits_ok(int32_t splits) { return splits == 1 || splits == 2 || splits == 4; }
extern "C" size_t rap_attention_split_workspace_bytes(int64_t TP, int32_t nseg, int32_t heads, int32_t splits) {
  if (TP < 0 || nseg < 0 || heads <= 0 || !attn_splits_ok(splits)) return 0;
  return carve_attn(TP, nseg, heads, splits, nullptr).total;
}
extern "C" int rap_attention_f32_split(const float* qkv_headmajor, const int32_t* cu_seqlens, int32_t nseg, float* out, int64_t TP,
                                       int32_t heads, const float* logit_bound, int32_t splits, void* ws, size_t ws_bytes, void* stream_) {
  if (!qkv_headmajor || !out || heads <= 0 || !attn_splits_ok(splits) || (splits > 1 && !logit_bound)) return RAP_ERR_INVALID;
  hipStream_t stream = (hipStream_t)stream_;
  AttnWs w;
  if (int rc = attn_begin(stream, cu_seqlens, nseg, TP, 0x7fffffffLL / 8, ws, ws_bytes, 0, &w, heads, splits)) return rc;
  if (splits == 1)
    return launch_attention_f32(stream, qkv_headmajor, out, (int)TP, heads, w.items, w.max_items, logit_bound, nullptr, nullptr, 1);
  return launch_attention_f32(stream, qkv_headmajor, out, (int)TP, heads, w.items, w.max_items, logit_bound, w.part_o, w.part_ml, splits,
                              w.cu_s, nseg);
}

// The launchers below take the row count as an int and answer RAP_OK to an empty call before they look at anything else: the entry
// points check every argument first, whatever the row count, and refuse a count the int would truncate (2^32 + 4 rows are not 4 rows).
static bool rows_fit_int(int64_t rows, int64_t round_up_to = 1) { return rows >= 0 && rows <= 0x7fffffffLL - (round_up_to - 1); }
static bool model_width_ok(int32_t d) { return d == 256 || d == 512 || d == 768 || d == 1024; }
extern "C" int rap_layernorm_mod(const float* x, float* out, int64_t TP, int32_t d, const float* mod, int64_t mod_stride,
                                 const int32_t* token_row, void* stream) {
  if (!x || !out || !mod || !model_width_ok(d) || !rows_fit_int(TP, 4)) return RAP_ERR_INVALID;
  return launch_layernorm_mod((hipStream_t)stream, x, out, (int)TP, d, mod, (long)mod_stride, token_row);
}
extern "C" int rap_layernorm_affine(const float* x, float* out, int64_t TP, int32_t d, const float* gain, const float* shift,
                                    void* stream) {
  if (!x || !out || !gain || !shift || !model_width_ok(d) || !rows_fit_int(TP, 4)) return RAP_ERR_INVALID;
  return launch_layernorm_affine((hipStream_t)stream, x, out, (int)TP, d, gain, shift);
}
// heads x TP rows per plane, `rows_per_block` of them to a block: the row count fits an int and the grid fits the launch limit
static bool qknorm_shape_ok(int64_t TP, int32_t heads, int rows_per_block) {
  return heads > 0 && rows_fit_int(TP) && 2 * (int64_t)heads * TP / rows_per_block < 0x7fffffffLL;
}
extern "C" int rap_qknorm(float* qkv_headmajor, int64_t TP, int32_t heads, const float* gamma_q, const float* gamma_k,
                          void* stream) {
  if (!qkv_headmajor || !gamma_q || !gamma_k || !qknorm_shape_ok(TP, heads, 16)) return RAP_ERR_INVALID;
  return launch_qknorm((hipStream_t)stream, qkv_headmajor, (int)TP, heads, gamma_q, gamma_k);
}
extern "C" int rap_posenc_x(const float* x, float* ax, int64_t TP, void* stream) {
  if (!x || !ax || !rows_fit_int(TP)) return RAP_ERR_INVALID;
  return launch_posenc_x((hipStream_t)stream, x, ax, (int)TP);
}
extern "C" int rap_posenc_static(const float* cond, const float* scales, const int32_t* token_sample, const float* feat,
                                 int32_t feat_dim, float* astatic, int64_t TP, void* stream) {
  if (!cond || !scales || !token_sample || !astatic || !rows_fit_int(TP)) return RAP_ERR_INVALID;
  if (feat_dim < 0 || feat_dim > 40 || feat_dim % 4 != 0 || (feat_dim > 0 && !feat)) return RAP_ERR_INVALID;
  return launch_posenc_static((hipStream_t)stream, cond, scales, token_sample, feat, feat_dim, astatic, (int)TP);
}
// The small kernels between the GEMMs that had no entry point of their own (the head tail, the weight-scale maximum, the logit bound
// of the bounded softmax, the segment-table sanitiser), for the parity tests: the launchers rap_sample / rap_model_create call.
extern "C" int rap_head_out3(const float* y, int32_t ldy, const float* W, float* v, int64_t TP, int32_t K, void* stream) {
  if (!y || !W || !v || !rows_fit_int(TP, 4)) return RAP_ERR_INVALID;
  if ((K != 128 && K != 256 && K != 384 && K != 512) || ldy < K || ldy % 4 != 0) return RAP_ERR_INVALID;
  return launch_head_out3((hipStream_t)stream, y, ldy, W, v, (int)TP, K);
}
extern "C" int rap_max_abs(const float* x, int64_t n, float* out, void* stream) {
  if (!x || !out || n < 0) return RAP_ERR_INVALID;
  return launch_max_abs((hipStream_t)stream, x, (size_t)n, out);
}
extern "C" int rap_qk_logit_bound(const float* gamma_q, const float* gamma_k, int32_t heads, float* out, void* stream) {
  if (!gamma_q || !gamma_k || !out || heads <= 0) return RAP_ERR_INVALID;
  return launch_qk_logit_bound((hipStream_t)stream, gamma_q, gamma_k, heads, out);
}
extern "C" int rap_sanitize_cu(const int32_t* cu, int32_t n, int64_t limit, int32_t* out, void* stream) {
  if (!cu || !out || n < 0 || limit < 0 || limit > 0x7fffffffLL) return RAP_ERR_INVALID;
  return launch_sanitize_cu((hipStream_t)stream, cu, n, (long)limit, out);
}
extern "C" int rap_token_sample(const int32_t* cu_batch, int32_t B, int32_t* token_sample, void* stream) {
  if (!cu_batch || !token_sample) return RAP_ERR_INVALID;
  return launch_token_sample((hipStream_t)stream, cu_batch, B, token_sample);
}

// ---- reduced-precision kernel-level entry points (dtype: 1 = bf16, 2 = fp16; 16-bit tensors as uint16_t*) ----
extern "C" int rap_convert_h16(int32_t dtype, const float* src, uint16_t* dst, int64_t n, void* stream) {
  if (!src || !dst || n < 0 || n % 4 != 0 || (dtype != RAP_DT_BF16 && dtype != RAP_DT_F16)) return RAP_ERR_INVALID;
  return launch_convert_h16((hipStream_t)stream, dtype, src, dst, (size_t)n);
}
// the operand / output / shape fields every 16-bit GEMM entry point below fills the same way (the rest keeps GemmParamsH's defaults)
static GemmParamsH gemm_h16_params(const uint16_t* A, int lda, const uint16_t* W, int ldw, void* C, int ldc, int M, int N, int K,
                                   const float* bias, int ldr) {
  GemmParamsH g{};
  g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K; g.bias = bias; g.ldr = ldr;
  return g;
}
extern "C" int rap_gemm_h16(int32_t dtype, int32_t epilogue, const uint16_t* A, int32_t lda, const uint16_t* W, int32_t ldw,
                            void* C, int32_t ldc, int32_t M, int32_t N, int32_t K, const float* bias, const float* resid,
                            int32_t ldr, int32_t heads, uint16_t* vt, int32_t vt_nblk, void* stream) {
  if (!A || !W || !C) return RAP_ERR_INVALID;
  GemmParamsH g = gemm_h16_params(A, lda, W, ldw, C, ldc, M, N, K, bias, ldr);
  g.resid = resid; g.heads = heads; g.vt = vt; g.vt_nblk = vt_nblk;
  if (epilogue == EPI_H_BIAS_RESID_H16) { g.resid_h = reinterpret_cast<const uint16_t*>(resid); g.resid = nullptr; }   // fp16 residual
  return launch_gemm_h16((hipStream_t)stream, dtype, epilogue, g);
}
// the residual epilogues (1, 6) with an optional split-K workspace (what rap_sample hands ff2 on few-token calls)
extern "C" size_t rap_gemm_h16_splitk_workspace_bytes(int32_t M, int32_t N, int32_t K) {
  const int s = gemm_h16_splits_by_shape(M, N, K);
  return s > 1 ? (size_t)s * (size_t)M * (size_t)N * sizeof(float) : 0;
}
extern "C" int rap_gemm_h16_splitk(int32_t dtype, int32_t epilogue, const uint16_t* A, int32_t lda, const uint16_t* W, int32_t ldw, void* C,
                                   int32_t ldc, int32_t M, int32_t N, int32_t K, const float* bias, const void* resid, int32_t ldr,
                                   void* ws, size_t ws_bytes, void* stream) {
  if (!A || !W || !C || (epilogue != EPI_H_BIAS_RESID_F32 && epilogue != EPI_H_BIAS_RESID_H16)) return RAP_ERR_INVALID;
  const size_t need = rap_gemm_h16_splitk_workspace_bytes(M, N, K);
  if (need && (!ws || ws_bytes < need)) return RAP_ERR_WORKSPACE;
  GemmParamsH g = gemm_h16_params(A, lda, W, ldw, C, ldc, M, N, K, bias, ldr);
  if (epilogue == EPI_H_BIAS_RESID_H16) g.resid_h = reinterpret_cast<const uint16_t*>(resid); else g.resid = reinterpret_cast<const float*>(resid);
  g.splitk_ws = need ? reinterpret_cast<float*>(ws) : nullptr;
  return launch_gemm_h16((hipStream_t)stream, dtype, epilogue, g);
}
// the dispatch decision of rap_gemm_h16 / rap_gemm_h16_qkvnorm / rap_gemm_h16_splitk (dtype 1, 2) and rap_x2_gemm (dtype 3: K, lda, ldw physical)
extern "C" int rap_gemm_h16_form(int32_t dtype, int32_t epilogue, int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldw, int32_t has_ws) {
  static float ws_given;      // (never dereferenced)
  GemmParamsH g = gemm_h16_params(nullptr, lda, nullptr, ldw, nullptr, N, M, N, K, nullptr, N);
  g.splitk_ws = has_ws ? &ws_given : nullptr;
  return gemm_h16_form(dtype, epilogue, g);
}
extern "C" int rap_attention_h16(int32_t dtype, const uint16_t* qk, const uint16_t* vt, int32_t vt_nblk,
                                 const int32_t* cu_seqlens, int32_t nseg, uint16_t* out, int64_t TP, int32_t heads,
                                 const float* logit_bound, void* ws, size_t ws_bytes, void* stream_) {
  if (!qk || !vt || !out) return RAP_ERR_INVALID;
  // 256-row work items, two stages -- unless tuning key 20 FORCES an item size / key groups (64, 128, 66, 130: the A/B values), which
  // then applies here as it does to a model call of the same row count (so the few-token kernels have kernel-level tests)
  const long rows = attention_h16_forced() ? (long)align_up((size_t)TP, 256) : 0;
  int bq, kg;
  attention_h16_plan(rows, &bq, &kg);
  hipStream_t stream = (hipStream_t)stream_;
  AttnWs w;
  if (int rc = attn_begin(stream, cu_seqlens, nseg, TP, 0x7fffffffLL / 8, ws, ws_bytes, bq, &w)) return rc;
  return launch_attention_h16(stream, dtype, qk, vt, vt_nblk, out, (int)TP, heads, w.items, w.max_items, logit_bound, 0, bq, kg);
}
extern "C" int rap_attention_h16_softcap(int32_t dtype, const uint16_t* qk, const uint16_t* vt, int32_t vt_nblk, const int32_t* cu_seqlens,
                                         int32_t nseg, uint16_t* out, int64_t TP, int32_t heads, float softcap, void* ws, size_t ws_bytes,
                                         void* stream_) {
  if (!qk || !vt || !out || heads <= 0 || !softcap_ok(softcap) || (dtype != RAP_DT_BF16 && dtype != RAP_DT_F16) || (int64_t)vt_nblk * 64 < TP)
    return RAP_ERR_INVALID;
  hipStream_t stream = (hipStream_t)stream_;
  AttnWs w;
  if (int rc = attn_begin(stream, cu_seqlens, nseg, TP, 0x7fffffffLL / 8, ws, ws_bytes, 256, &w)) return rc;
  return launch_attention_h16_softcap(stream, dtype, qk, vt, vt_nblk, out, (int)TP, heads, w.items, w.max_items, softcap);
}
extern "C" int rap_layernorm_mod_h16(int32_t dtype, const float* x, uint16_t* out, int64_t TP, int32_t d, const float* mod,
                                     int64_t mod_stride, const int32_t* token_row, void* stream) {
  if (!x || !out || !mod) return RAP_ERR_INVALID;
  return launch_layernorm_mod_h16((hipStream_t)stream, dtype, x, 0, out, (int)TP, d, mod, (long)mod_stride, token_row);
}
extern "C" int rap_layernorm_affine_h16(int32_t dtype, const float* x, uint16_t* out, int64_t TP, int32_t d, const float* gain,
                                        const float* shift, void* stream) {
  if (!x || !out || !gain || !shift) return RAP_ERR_INVALID;
  return launch_layernorm_affine_h16((hipStream_t)stream, dtype, x, 0, out, (int)TP, d, gain, shift);
}
// The same two kernels with the residual-stream dtype exposed, the fused combine + LayerNorm of few-token calls (tuning key 19) and the
// two stream conversions, for the parity tests.  The launchers answer RAP_OK to an empty row count before they look at anything else:
// every argument is checked HERE, whatever the row count.
static bool ln_stream_args_ok(int32_t dtype, int32_t stream_f16, int64_t rows, int32_t d) {
  if (dtype != RAP_DT_BF16 && dtype != RAP_DT_F16 && dtype != RAP_DT_F32X2) return false;
  if (stream_f16 != 0 && stream_f16 != 1) return false;
  if (dtype == RAP_DT_F32X2 && stream_f16) return false;      // the split mode keeps the residual stream in fp32
  if (d != 256 && d != 512 && d != 768 && d != 1024) return false;
  return rows >= 0 && rows <= 0x7fffffffLL - 3;                // the launchers take the row count as an int and round it up to 4
}
extern "C" int rap_layernorm_mod_h16_stream(int32_t dtype, const void* x, int32_t x_f16, uint16_t* out, int64_t TP, int32_t d,
                                            const float* mod, int64_t mod_stride, const int32_t* token_row, void* stream) {
  if (!x || !out || !mod || !ln_stream_args_ok(dtype, x_f16, TP, d)) return RAP_ERR_INVALID;
  return launch_layernorm_mod_h16((hipStream_t)stream, dtype, x, x_f16, out, (int)TP, d, mod, (long)mod_stride, token_row);
}
extern "C" int rap_layernorm_affine_h16_stream(int32_t dtype, const void* x, int32_t x_f16, uint16_t* out, int64_t TP, int32_t d,
                                               const float* gain, const float* shift, void* stream) {
  if (!x || !out || !gain || !shift || !ln_stream_args_ok(dtype, x_f16, TP, d)) return RAP_ERR_INVALID;
  return launch_layernorm_affine_h16((hipStream_t)stream, dtype, x, x_f16, out, (int)TP, d, gain, shift);
}
extern "C" int rap_resid_combine_layernorm_h16(int32_t dtype, const float* part, int32_t splits, const float* bias, void* h, int32_t h_f16,
                                               uint16_t* out, int64_t rows, int32_t d, const float* mod, int64_t mod_stride,
                                               const int32_t* token_row, const float* gain, const float* shift, void* stream) {
  if (!part || !h || !out || splits < 1 || splits > 8 || !ln_stream_args_ok(dtype, h_f16, rows, d)) return RAP_ERR_INVALID;
  if (!mod && (!gain || !shift)) return RAP_ERR_INVALID;
  return launch_resid_combine_ln_h16((hipStream_t)stream, dtype, part, splits, bias, h, h_f16, out, (int)rows, d, mod, (long)mod_stride,
                                     token_row, gain, shift);
}
extern "C" int rap_convert_f16_sat(const float* src, uint16_t* dst, int64_t n, void* stream) {
  if (!src || !dst || n < 0 || n % 4 != 0) return RAP_ERR_INVALID;
  return launch_convert_f16_sat((hipStream_t)stream, src, dst, (size_t)n);
}
extern "C" int rap_convert_f16_to_f32(const uint16_t* src, float* dst, int64_t n, void* stream) {
  if (!src || !dst || n < 0 || n % 8 != 0) return RAP_ERR_INVALID;
  return launch_convert_f16_to_f32((hipStream_t)stream, src, dst, (size_t)n);
}
extern "C" int rap_qknorm_h16(int32_t dtype, uint16_t* qk, int64_t TP, int32_t heads, const float* gamma_q,
                              const float* gamma_k, void* stream) {
  if (!qk || !gamma_q || !gamma_k || (dtype != RAP_DT_BF16 && dtype != RAP_DT_F16) || !qknorm_shape_ok(TP, heads, 32)) return RAP_ERR_INVALID;
  return launch_qknorm_h16((hipStream_t)stream, dtype, qk, (int)TP, heads, gamma_q, gamma_k, 8.0f);
}

// ---- split-precision kernel-level entry points (compute dtype 3; paired fp16 head / tail operands, see include/rapflow.h) ----
extern "C" int rap_x2_pack(const float* src, int64_t ld_src, int64_t rows, int32_t cols, float scale, uint16_t* dst, void* stream) {
  if (!src || !dst || rows < 0 || cols < 0 || cols % 32 != 0 || ld_src < cols || (ld_src & 3)) return RAP_ERR_INVALID;
  return launch_x2_pack((hipStream_t)stream, src, (long)ld_src, (long)rows, cols, scale, dst);
}
extern "C" int rap_x2_unpack(const uint16_t* src, int64_t rows, int32_t cols, float inv_scale, float* dst, void* stream) {
  if (!src || !dst || rows < 0 || cols < 0 || cols % 32 != 0) return RAP_ERR_INVALID;
  return launch_x2_unpack((hipStream_t)stream, src, (long)rows, cols, inv_scale, dst);
}
extern "C" int rap_x2_gemm(int32_t epilogue, const uint16_t* A, int32_t lda, const uint16_t* W, int32_t ldw, void* C, int32_t ldc, int32_t M,
                           int32_t N, int32_t K_physical, const float* bias, const float* resid, int32_t ldr, float acc_scale, int32_t heads,
                           const float* gamma_q, const float* gamma_k, float q_mul, uint16_t* vt, int32_t vt_nblk, void* stream) {
  if (!A || !W || !C) return RAP_ERR_INVALID;
  GemmParamsH g = gemm_h16_params(A, lda, W, ldw, C, ldc, M, N, K_physical, bias, ldr);
  g.resid = resid; g.heads = heads; g.vt = vt; g.vt_nblk = vt_nblk; g.gamma_q = gamma_q; g.gamma_k = gamma_k;
  g.q_mul = q_mul; g.acc_scale = acc_scale;
  return launch_gemm_h16((hipStream_t)stream, RAP_DT_F32X2, epilogue, g);
}
extern "C" int rap_x2_attention(const uint16_t* qk, const uint16_t* vt, int32_t vt_nblk, const int32_t* cu_seqlens, int32_t nseg,
                                uint16_t* out, int64_t TP, int32_t heads, void* ws, size_t ws_bytes, void* stream_) {
  if (!qk || !vt || !out) return RAP_ERR_INVALID;
  hipStream_t stream = (hipStream_t)stream_;
  AttnWs w;
  if (int rc = attn_begin(stream, cu_seqlens, nseg, TP, 0x7fffffffLL / 16, ws, ws_bytes, 256, &w)) return rc;
  return launch_attention_x2(stream, qk, vt, vt_nblk, out, (int)TP, heads, w.items, w.max_items);
}
extern "C" int rap_x2_attention_softcap(const uint16_t* qk, const uint16_t* vt, int32_t vt_nblk, const int32_t* cu_seqlens, int32_t nseg,
                                        uint16_t* out, int64_t TP, int32_t heads, float softcap, void* ws, size_t ws_bytes, void* stream_) {
  if (!qk || !vt || !out || heads <= 0 || !softcap_ok(softcap) || (int64_t)vt_nblk * 64 < TP) return RAP_ERR_INVALID;
  hipStream_t stream = (hipStream_t)stream_;
  AttnWs w;
  if (int rc = attn_begin(stream, cu_seqlens, nseg, TP, 0x7fffffffLL / 16, ws, ws_bytes, 256, &w)) return rc;
  return launch_attention_x2_softcap(stream, qk, vt, vt_nblk, out, (int)TP, heads, w.items, w.max_items, softcap);
}
// the same over `splits` key ranges per work item (workspace layout: carve_attn)
extern "C" int rap_x2_attention_split(const uint16_t* qk, const uint16_t* vt, int32_t vt_nblk, const int32_t* cu_seqlens, int32_t nseg,
                                      uint16_t* out, int64_t TP, int64_t n_tokens, int32_t heads, int32_t splits, void* ws, size_t ws_bytes,
                                      void* stream_) {
  if (!qk || !vt || !out || heads <= 0 || !attn_splits_ok(splits) || n_tokens < 0 || n_tokens > TP || (int64_t)vt_nblk * 64 < TP)
    return RAP_ERR_INVALID;
  hipStream_t stream = (hipStream_t)stream_;
  AttnWs w;
  if (int rc = attn_begin(stream, cu_seqlens, nseg, TP, 0x7fffffffLL / 16, ws, ws_bytes, 256, &w, heads, splits)) return rc;
  if (splits == 1) return launch_attention_x2(stream, qk, vt, vt_nblk, out, (int)TP, heads, w.items, w.max_items);
  return launch_attention_x2(stream, qk, vt, vt_nblk, out, (int)TP, heads, w.items, w.max_items, w.part_o, w.part_ml, splits, (int)n_tokens,
                             w.cu_s, nseg);
}

// ---------------------------------------------------------------------------------------------
// generation selection by rigidity
// ---------------------------------------------------------------------------------------------
struct RigWs { int32_t* off; double* partials; float* Rc; float* tc; float* per_step; size_t total; };
static RigWs carve_rig(int nparts, int S, int B, char* basep) {
  RigWs p; Carver c(basep);
  p.off = (int32_t*)c.take(((size_t)nparts + 1) * 4);
  p.partials = (double*)c.take((size_t)nparts * RAP_PROC_CHUNKS * 16 * 8);
  p.Rc = (float*)c.take((size_t)nparts * 9 * 4);
  p.tc = (float*)c.take((size_t)nparts * 3 * 4);
  p.per_step = (float*)c.take((size_t)(S > 0 ? S : 1) * B * 4);
  p.total = c.total();
  return p;
}
extern "C" size_t rap_rigidity_workspace_bytes(int32_t nparts, int32_t steps, int32_t B) {
  return (nparts < 0 || steps < 0 || B < 0) ? 0 : carve_rig(nparts, steps, B, nullptr).total;
}

extern "C" int rap_rigidity_rmse(const float* cond, const float* pred, const float* R, const float* t,
                                 const int64_t* points_per_part, int32_t B, int32_t P, const float* scales,
                                 int32_t average_per_part, float* out, void* ws, size_t ws_bytes, void* stream_) {
  if (!cond || !pred || !R || !t || !points_per_part || !out || B <= 0 || P <= 0) return RAP_ERR_INVALID;
  if ((int64_t)B * P > 65535) return RAP_ERR_INVALID;
  if (!ws) return RAP_ERR_WORKSPACE;
  RigWs w = carve_rig(B * P, 0, B, (char*)ws);
  if (w.total > ws_bytes) return RAP_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  int rc;
  if ((rc = launch_part_offsets(stream, points_per_part, B * P, w.off))) return rc;
  return launch_rigidity_rmse(stream, cond, pred, R, t, w.off, B, P, scales, average_per_part, out, w.partials);
}

extern "C" int rap_trajectory_rigidity_rmse(const float* cond, const float* traj, const int64_t* points_per_part, int32_t B,
                                            int32_t P, int64_t TP, int32_t steps, const float* scales, float* mean_out,
                                            float* per_step_out, void* ws, size_t ws_bytes, void* stream_) {
  if (!cond || !traj || !points_per_part || !mean_out || B <= 0 || P <= 0 || TP <= 0 || steps <= 0) return RAP_ERR_INVALID;
  if ((int64_t)B * P > 65535) return RAP_ERR_INVALID;
  if (!ws) return RAP_ERR_WORKSPACE;
  RigWs w = carve_rig(B * P, steps, B, (char*)ws);
  if (w.total > ws_bytes) return RAP_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  float* per_step = per_step_out ? per_step_out : w.per_step;
  int rc;
  if ((rc = launch_part_offsets(stream, points_per_part, B * P, w.off))) return rc;
  for (int s = 0; s < steps; ++s) {
    const float* x0 = traj + (size_t)s * TP * 3;
    if ((rc = launch_procrustes_fit(stream, cond, x0, w.off, B * P, w.Rc, w.tc, w.partials))) return rc;      // modeling.py:479-481
    if ((rc = launch_rigidity_rmse(stream, cond, x0, w.Rc, w.tc, w.off, B, P, scales, 0, per_step + (size_t)s * B, w.partials)))
      return rc;                                                                                              // :484-487
  }
  return launch_step_mean(stream, per_step, steps, B, mean_out);                                             // :489
}

extern "C" int rap_select_generation(const float* rmse, int32_t G, int32_t B, int32_t P, int64_t TP, const int32_t* cu_batch,
                                     const float* clouds, const float* R, const float* t, int32_t pick_largest,
                                     int32_t* best_out, float* cloud_out, float* R_out, float* t_out, void* stream) {
  if (!rmse || !best_out || G <= 0 || B <= 0) return RAP_ERR_INVALID;
  if (clouds && (!R || !t || !cu_batch || !cloud_out || !R_out || !t_out || P <= 0 || TP <= 0)) return RAP_ERR_INVALID;
  return launch_select_generation((hipStream_t)stream, rmse, G, B, P, (long)TP, cu_batch, clouds, R, t, pick_largest, best_out,
                                  cloud_out, R_out, t_out);
}

extern "C" int rap_relative_transforms(const float* R_pred, const float* t_pred, const float* R_gt, const float* t_gt,
                                       const float* scales, const int64_t* points_per_part, int32_t B, int32_t P,
                                       const float* global_rotation, const float* global_translation, float* out, void* stream) {
  if (!R_pred || !t_pred || !R_gt || !t_gt || !scales || !points_per_part || !out || B <= 0 || P <= 0) return RAP_ERR_INVALID;
  if ((global_rotation == nullptr) != (global_translation == nullptr)) return RAP_ERR_INVALID;
  return launch_relative_transforms((hipStream_t)stream, R_pred, t_pred, R_gt, t_gt, scales, points_per_part, B, P,
                                    global_rotation, global_translation, out);
}

// ---------------------------------------------------------------------------------------------
// cross-part overlap ratio
// ---------------------------------------------------------------------------------------------
// compute_transform_errors without ICP (reference eval/metrics.py:165-303): see transforms.hip
extern "C" int rap_transform_errors(const float* R_gt, const float* t_gt, const float* R_pred, const float* t_pred,
                                    const int64_t* points_per_part, const uint8_t* anchor_part, const int64_t* matched_part_ids,
                                    const float* scale, int32_t B, int32_t P, float* rot_err_per_part, float* trans_err_per_part,
                                    float* rot_err_mean, float* trans_err_mean, void* stream) {
  if (!R_gt || !t_gt || !R_pred || !t_pred || !points_per_part || !anchor_part || !rot_err_per_part || !trans_err_per_part ||
      !rot_err_mean || !trans_err_mean || B <= 0 || P <= 0)
    return RAP_ERR_INVALID;
  return launch_transform_errors((hipStream_t)stream, R_gt, t_gt, R_pred, t_pred, points_per_part, anchor_part, matched_part_ids, scale,
                                 B, P, rot_err_per_part, trans_err_per_part, rot_err_mean, trans_err_mean);
}

struct OvWs { int32_t* off; int32_t* pid; float* min_dist; void* items; size_t total; };
static OvWs carve_ov(int64_t TP, int B, int P, char* basep) {
  OvWs w; Carver c(basep);
  w.off = (int32_t*)c.take(((size_t)B * P + 1) * 4);
  w.pid = (int32_t*)c.take((size_t)TP * 4);
  w.min_dist = (float*)c.take((size_t)TP * 4);
  w.items = c.take(overlap_max_items((long)TP, B) * 16);
  w.total = c.total();
  return w;
}
extern "C" size_t rap_overlap_workspace_bytes(int64_t TP, int32_t B, int32_t P) {
  return (TP < 0 || B < 0 || P < 0) ? 0 : carve_ov(TP, B, P, nullptr).total;
}
extern "C" int rap_overlap_ratio(const float* pointclouds_pred, const int64_t* points_per_part, const int32_t* cu_batch, int32_t B,
                                 int32_t P, int64_t TP, const float* h_taus, int32_t n_taus, float* ratios_out, float* min_dist_out,
                                 void* ws, size_t ws_bytes, void* stream_) {
  if (!pointclouds_pred || !points_per_part || !cu_batch || !h_taus || !ratios_out || B <= 0 || P <= 0 || TP <= 0) return RAP_ERR_INVALID;
  if ((int64_t)B * P > 65535 || TP > 0x7fffffffLL / 8) return RAP_ERR_INVALID;
  if (!ws) return RAP_ERR_WORKSPACE;
  OvWs w = carve_ov(TP, B, P, (char*)ws);
  if (w.total > ws_bytes) return RAP_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  int rc;
  if ((rc = launch_part_offsets(stream, points_per_part, B * P, w.off))) return rc;
  return launch_overlap_ratio(stream, pointclouds_pred, cu_batch, w.off, B, P, (long)TP, h_taus, n_taus, ratios_out,
                              min_dist_out ? min_dist_out : w.min_dist, w.pid, w.items);
}

// ---------------------------------------------------------------------------------------------
// MiniSpinNet local feature extractor
// ---------------------------------------------------------------------------------------------
#include <cmath>
struct SpinLayer { int Cin, Cout, Kd, ldw; bool bn_relu; const float* W; const float* b; const float* Wt; const float* bt; };   // Wt / bt: tap-major (implicit GEMM)
struct rap_spinnet {
  float* raw = nullptr;       // the caller's blob (MiniSpinNet.state_dict() float tensors, registration order)
  float* derived = nullptr;   // folded + padded conv weights / biases, voxel table, pool weights
  float h_w1[48], h_b1[16];   // point MLP with BatchNorm folded (kernel argument)
  const float* vox;           // (420,3)
  const void* pool_w;         // SpinPoolW on the device
  SpinLayer layers[8];
  const float* zeros = nullptr;   // 256 bytes of zeros: the elevation pad of the implicit-GEMM convolutions
};
static const int kSpinCin[8] = {16, 64, 64, 128, 128, 64, 64, 32};
static const int kSpinCout[8] = {64, 64, 128, 128, 64, 64, 32, 32};

extern "C" int64_t rap_spinnet_weight_count(void) {
  int64_t n = 48 + 16 * 5 + (512 + 16 * 5 + 16 + 5);
  for (int i = 0; i < 8; ++i) {
    const int64_t kd = (int64_t)kSpinCin[i] * (i == 0 ? 27 : 9);
    n += kSpinCout[i] * kd + kSpinCout[i] + (i < 7 ? 2 * kSpinCout[i] : 0);
  }
  return n;
}

extern "C" void rap_spinnet_destroy(rap_spinnet* m) {
  if (!m) return;
  if (m->raw) (void)hipFree(m->raw);
  if (m->derived) (void)hipFree(m->derived);
  delete m;
}

extern "C" int rap_spinnet_create(const float* d_weights, int64_t n_floats, void* stream_, rap_spinnet** out) {
  if (!out) return RAP_ERR_INVALID;
  *out = nullptr;
  if (!d_weights || n_floats != rap_spinnet_weight_count()) return RAP_ERR_INVALID;
  hipStream_t stream = (hipStream_t)stream_;
  rap_spinnet* m = new (std::nothrow) rap_spinnet();
  if (!m) return RAP_ERR_ALLOC;
  auto fail = [&](int code) { rap_spinnet_destroy(m); return code; };
  if (hipMalloc((void**)&m->raw, (size_t)n_floats * 4) != hipSuccess) { delete m; return RAP_ERR_ALLOC; }
  size_t n_der = 420 * 3 + 1024;      // voxel table + pool struct (613 floats used)
  for (int i = 0; i < 8; ++i) n_der += (size_t)128 * (i == 0 ? 448 : kSpinCin[i] * 9) + 128 + (i ? (size_t)kSpinCout[i] * kSpinCin[i] * 9 + 128 : (size_t)64 * 448 + 128);
  n_der += 64;      // zero page
  if (hipMalloc((void**)&m->derived, n_der * 4) != hipSuccess) return fail(RAP_ERR_ALLOC);
  if (hipMemcpyAsync(m->raw, d_weights, (size_t)n_floats * 4, hipMemcpyDeviceToDevice, stream) != hipSuccess) return fail(RAP_ERR_HIP);
  // ---- small heads on the host: point MLP (128 floats) and attention pool (613 floats)
  std::vector<float> h(128 + 613);
  if (hipMemcpyAsync(h.data(), m->raw, h.size() * 4, hipMemcpyDeviceToHost, stream) != hipSuccess) return fail(RAP_ERR_HIP);
  if (hipStreamSynchronize(stream) != hipSuccess) return fail(RAP_ERR_HIP);
  {
    const float *W = &h[0], *b = &h[48], *g = &h[64], *be = &h[80], *rm = &h[96], *rv = &h[112];
    for (int c = 0; c < 16; ++c) {
      const float s = g[c] / std::sqrt(rv[c] + 1e-5f);
      for (int d = 0; d < 3; ++d) m->h_w1[c * 3 + d] = W[c * 3 + d] * s;
      m->h_b1[c] = (b[c] - rm[c]) * s + be[c];
    }
  }
  std::vector<float> pool(16 * 32 + 16 + 16 + 1);
  {
    const float* p0 = &h[128];
    const float *W1 = p0, *b1 = p0 + 512, *g1 = p0 + 528, *be1 = p0 + 544, *rm1 = p0 + 560, *rv1 = p0 + 576;
    const float *W2 = p0 + 592, *b2 = p0 + 608, *g2 = p0 + 609, *be2 = p0 + 610, *rm2 = p0 + 611, *rv2 = p0 + 612;
    for (int j = 0; j < 16; ++j) {
      const float s = g1[j] / std::sqrt(rv1[j] + 1e-5f);
      for (int c = 0; c < 32; ++c) pool[j * 32 + c] = W1[j * 32 + c] * s;
      pool[512 + j] = (b1[j] - rm1[j]) * s + be1[j];
    }
    const float s2 = g2[0] / std::sqrt(rv2[0] + 1e-5f);
    for (int j = 0; j < 16; ++j) pool[528 + j] = W2[j] * s2;
    pool[544] = (b2[0] - rm2[0]) * s2 + be2[0];
  }
  // ---- voxel centres: get_voxel_coordinate(radius 1, rad_n 3, azi_n 20, ele_n 7)  (utils/common.py:213-225, 338-372, 387-393)
  std::vector<float> vox(420 * 3);
  for (int r = 0; r < 3; ++r)
    for (int e = 0; e < 7; ++e)
      for (int a = 0; a < 20; ++a) {
        const double beta = M_PI * e / 7.0 + M_PI / 7.0 / 2.0, alpha = 2.0 * M_PI * a / 20.0 + M_PI / 20.0;
        const double sc = (double)r / 3.0 + 1.0 / 6.0;
        float* v = &vox[((r * 7 + e) * 20 + a) * 3];
        v[0] = (float)(sc * std::sin(beta) * std::cos(alpha));
        v[1] = (float)(sc * std::sin(beta) * std::sin(alpha));
        v[2] = (float)(sc * std::cos(beta));
      }
  float* q = m->derived;
  if (hipMemcpyAsync(q, vox.data(), vox.size() * 4, hipMemcpyHostToDevice, stream) != hipSuccess) return fail(RAP_ERR_HIP);
  m->vox = q; q += 420 * 3;
  if (hipMemcpyAsync(q, pool.data(), pool.size() * 4, hipMemcpyHostToDevice, stream) != hipSuccess) return fail(RAP_ERR_HIP);
  m->pool_w = q; q += 1024;
  if (hipStreamSynchronize(stream) != hipSuccess) return fail(RAP_ERR_HIP);   // vox / pool are stack-backed host vectors
  // ---- conv stack: fold BatchNorm (affine=False) and pad to 128 output columns / 32-multiple k
  const float* p = m->raw + 128 + 613;
  for (int i = 0; i < 8; ++i) {
    SpinLayer& L = m->layers[i];
    L.Cin = kSpinCin[i]; L.Cout = kSpinCout[i]; L.Kd = L.Cin * (i == 0 ? 27 : 9); L.ldw = i == 0 ? 448 : L.Kd; L.bn_relu = i < 7;
    const float* W = p; p += (size_t)L.Cout * L.Kd;
    const float* b = p; p += L.Cout;
    const float *rm = nullptr, *rv = nullptr;
    if (L.bn_relu) { rm = p; p += L.Cout; rv = p; p += L.Cout; }
    float* Wd = q; q += (size_t)128 * L.ldw;
    float* bd = q; q += 128;
    int rc;
    if ((rc = launch_spin_fold(stream, W, b, nullptr, nullptr, rm, rv, L.Cout, L.Kd, Wd, L.ldw, 128, bd))) return fail(rc);
    L.W = Wd; L.b = bd; L.Wt = nullptr; L.bt = nullptr;
    {
      const int ldt = i == 0 ? 448 : L.Kd;
      float* Wt = q; q += (size_t)L.Cout * ldt;
      float* bt = q; q += 128;
      if ((rc = launch_spin_fold_tapmajor(stream, W, b, rm, rv, L.Cin, L.Cout, i == 0 ? 27 : 9, ldt, Wt, bt))) return fail(rc);
      L.Wt = Wt; L.bt = bt;
    }
  }
  if (hipMemsetAsync(q, 0, 256, stream) != hipSuccess) return fail(RAP_ERR_HIP);
  m->zeros = q; q += 64;
  if ((int64_t)(p - m->raw) != n_floats) return fail(RAP_ERR_INVALID);
  *out = m;
  return RAP_OK;
}

struct SpinWs { float *x0, *A, *Y0, *Y1; size_t total; };
static SpinWs carve_spin(int Kc, char* basep) {
  SpinWs w; Carver c(basep);
  w.x0 = (float*)c.take((size_t)Kc * 420 * 16 * 4);
  w.A = (float*)c.take((size_t)Kc * 140 * 1152 * 4);
  w.Y0 = (float*)c.take((size_t)Kc * 140 * 128 * 4);
  w.Y1 = (float*)c.take((size_t)Kc * 140 * 128 * 4);
  w.total = c.total();
  return w;
}
extern "C" size_t rap_spinnet_workspace_bytes(int32_t keypoints_per_chunk) {
  return keypoints_per_chunk <= 0 ? 0 : carve_spin(keypoints_per_chunk, nullptr).total;
}

extern "C" int rap_spinnet_describe(const rap_spinnet* m, const float* pts, const int32_t* perm, int64_t N, const float* kpts,
                                    int32_t K, float des_r, int32_t flags, float* desc_out, int32_t keypoints_per_chunk, void* ws,
                                    size_t ws_bytes, void* stream_) {
  if (!m || !pts || !kpts || !desc_out || N <= 0 || K < 0 || !(des_r > 0.f) || keypoints_per_chunk <= 0) return RAP_ERR_INVALID;
  if (flags & ~(RAP_SPINNET_PATCH_LRF | RAP_SPINNET_IM2COL_PATH)) return RAP_ERR_INVALID;
  // per-call options (round 3, ADVICE r02: they used to be mutable state of the handle, a race between two callers of one model)
  const int lrf = (flags & RAP_SPINNET_PATCH_LRF) ? 1 : 0;
  const bool implicit = !(flags & RAP_SPINNET_IM2COL_PATH);
  if (K == 0) return RAP_OK;
  if (!ws) return RAP_ERR_WORKSPACE;
  SpinWs w = carve_spin(keypoints_per_chunk, (char*)ws);
  if (w.total > ws_bytes) return RAP_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  int rc;
  for (int k0 = 0; k0 < K; k0 += keypoints_per_chunk) {
    const int Kc = K - k0 < keypoints_per_chunk ? K - k0 : keypoints_per_chunk;
    const int M = Kc * 140;
    if ((rc = launch_spin_patch(stream, pts, perm, (long)N, kpts + (size_t)k0 * 3, Kc, des_r, m->vox, m->h_w1, m->h_b1, w.x0, lrf))) return rc;
    float* yin = nullptr;
    float* yout = w.Y0;
    int ld_in = 128;
    for (int i = 0; i < 8; ++i) {
      const SpinLayer& L = m->layers[i];
      if (implicit) {
        // implicit GEMM: the gather of the 3x3(x3) cylindrical neighbourhood happens in the DMA source addresses, output is dense (M, Cout)
        if (i == 0) rc = launch_spin_conv3d(stream, w.x0, L.Wt, L.bt, m->zeros, yout, M);
        else rc = launch_spin_conv3x3(stream, yin, ld_in, L.Cin, L.Wt, L.bt, m->zeros, yout, L.Cout, M, L.bn_relu);
        if (rc) return rc;
        ld_in = L.Cout;
      } else {
        if (i == 0) rc = launch_spin_im2col3d(stream, w.x0, Kc, w.A, L.ldw);
        else rc = launch_spin_im2col2d(stream, yin, 128, L.Cin, Kc, w.A);
        if (rc) return rc;
        GemmParams g{};
        g.A = w.A; g.lda = L.ldw; g.W = L.W; g.ldw = L.ldw; g.C = yout; g.ldc = 128; g.M = M; g.N = 128; g.K = L.ldw; g.bias = L.b;
        if ((rc = launch_gemm_f32(stream, L.bn_relu ? EPI_BIAS_RELU : EPI_BIAS, g))) return rc;
        ld_in = 128;
      }
      yin = yout; yout = (yout == w.Y0) ? w.Y1 : w.Y0;
    }
    if ((rc = launch_spin_pool(stream, yin, ld_in, Kc, m->pool_w, desc_out + (size_t)k0 * 32))) return rc;
  }
  return RAP_OK;
}

// ---------------------------------------------------------------------------------------------
// nearest-neighbour registration metrics
// ---------------------------------------------------------------------------------------------
struct NnWs { float* d2a; float* d2b; int32_t* nn; NnWork* items; size_t total; };
static NnWs carve_nn(int64_t n, int B, char* basep) {
  NnWs w; Carver c(basep);
  w.d2a = (float*)c.take((size_t)n * 4);
  w.d2b = (float*)c.take((size_t)n * 4);
  w.nn = (int32_t*)c.take((size_t)n * 4);
  w.items = (NnWork*)c.take(nn_max_items((long)n, B) * sizeof(NnWork));
  w.total = c.total();
  return w;
}
extern "C" size_t rap_nn_metrics_workspace_bytes(int64_t n_points, int32_t B) {
  return (n_points < 0 || B < 0) ? 0 : carve_nn(n_points, B, nullptr).total;
}
extern "C" int rap_chamfer_rmse(const float* pointclouds_gt, const float* pointclouds_pred, const int32_t* cu_batch, int32_t B,
                                int64_t TP, float* out, void* ws, size_t ws_bytes, void* stream) {
  if (!pointclouds_gt || !pointclouds_pred || !cu_batch || !out || B <= 0 || TP <= 0 || TP > 0x7fffffffLL / 8) return RAP_ERR_INVALID;
  if (!ws) return RAP_ERR_WORKSPACE;
  NnWs w = carve_nn(TP, B, (char*)ws);
  if (w.total > ws_bytes) return RAP_ERR_WORKSPACE;
  return launch_chamfer_rmse((hipStream_t)stream, pointclouds_gt, pointclouds_pred, cu_batch, B, (long)TP, out, w.d2a, w.d2b, w.items);
}
extern "C" int rap_correspondence_rmse(const float* source_gt, const float* target_gt, const float* source_pred,
                                       const float* target_pred, int32_t n_source, int32_t n_target, float distance_threshold,
                                       float* out3, void* ws, size_t ws_bytes, void* stream) {
  if (!source_gt || !target_gt || !source_pred || !target_pred || !out3 || n_source <= 0 || n_target <= 0) return RAP_ERR_INVALID;
  if (!ws) return RAP_ERR_WORKSPACE;
  NnWs w = carve_nn(n_source, 1, (char*)ws);
  if (w.total > ws_bytes) return RAP_ERR_WORKSPACE;
  return launch_correspondence_rmse((hipStream_t)stream, source_gt, target_gt, source_pred, target_pred, n_source, n_target,
                                    distance_threshold, out3, w.d2a, w.nn, w.items);
}

// part accuracy and the part matching behind matched_part_ids: see part_acc.hip
#define RAP_PART_ACC_MAX_P 256
struct PartAccWs { int32_t* seg; float* d2a; float* d2b; NnWork* items; int32_t* count; uint32_t* ge; uint32_t* lt; size_t total; };
static PartAccWs carve_part_acc(int64_t TP, int B, int P, char* basep) {
  PartAccWs w; Carver c(basep);
  const size_t words = (size_t)B * P * ((P + 31) / 32);
  w.seg = (int32_t*)c.take((size_t)B * P * 2 * 4);
  w.d2a = (float*)c.take((size_t)TP * P * 4);
  w.d2b = (float*)c.take((size_t)TP * P * 4);
  w.items = (NnWork*)c.take(part_acc_max_items((long)TP, B, P) * sizeof(NnWork));
  w.count = (int32_t*)c.take(4);
  w.ge = (uint32_t*)c.take(words * 4);
  w.lt = (uint32_t*)c.take(words * 4);
  w.total = c.total();
  return w;
}
extern "C" size_t rap_part_acc_workspace_bytes(int64_t TP, int32_t B, int32_t P) {
  return (TP < 0 || B < 0 || P < 0 || P > RAP_PART_ACC_MAX_P) ? 0 : carve_part_acc(TP, B, P, nullptr).total;
}
extern "C" int rap_part_acc(const float* pointclouds_gt, const float* pointclouds_pred, const int64_t* points_per_part, const int32_t* cu_batch,
                            int32_t B, int32_t P, int64_t TP, float threshold, float* part_acc_out, int64_t* matched_out, float* cd_out,
                            void* ws, size_t ws_bytes, void* stream) {
  if (!points_per_part || !cu_batch || !part_acc_out || !matched_out || B < 0 || P <= 0 || P > RAP_PART_ACC_MAX_P || TP < 0 ||
      threshold != threshold)
    return RAP_ERR_INVALID;
  if (TP > 0 && (!pointclouds_gt || !pointclouds_pred)) return RAP_ERR_INVALID;
  if ((int64_t)B * P > 65535 || TP > 0x7fffffffLL / 8) return RAP_ERR_INVALID;
  if (B == 0) return RAP_OK;
  if (!ws) return RAP_ERR_WORKSPACE;
  PartAccWs w = carve_part_acc(TP, B, P, (char*)ws);
  if (w.total > ws_bytes) return RAP_ERR_WORKSPACE;
  return launch_part_acc((hipStream_t)stream, pointclouds_gt, pointclouds_pred, points_per_part, cu_batch, B, P, (long)TP, threshold,
                         part_acc_out, matched_out, cd_out, w.seg, w.d2a, w.d2b, w.items, w.count, w.ge, w.lt);
}

// batched scan-pair metrics of the evaluator + compute_transform_errors_direct: see pair_metrics.hip
struct PairWs { NnWork* items; void* partials; void* ranges; size_t total; };
static PairWs carve_pair(int64_t n, int B, char* basep) {
  PairWs w; Carver c(basep);
  const size_t max_items = nn_max_items((long)n, B);
  w.items = (NnWork*)c.take(max_items * sizeof(NnWork));
  w.partials = c.take(max_items * 16);
  w.ranges = c.take((size_t)B * 16);
  w.total = c.total();
  return w;
}
extern "C" size_t rap_pair_metrics_workspace_bytes(int64_t n_points, int32_t B) {
  return (n_points < 0 || B < 0) ? 0 : carve_pair(n_points, B, nullptr).total;
}
extern "C" int rap_pair_metrics(const float* pointclouds_gt, const float* cloud, const int64_t* points_per_part, const int32_t* cu_batch,
                                const float* scales, const float* R_gt, const float* t_gt, const float* R_pred, const float* t_pred,
                                int32_t B, int64_t TP, float distance_threshold, float* out4, void* ws, size_t ws_bytes, void* stream) {
  if (!pointclouds_gt || !cloud || !points_per_part || !cu_batch || !scales || !R_gt || !t_gt || !out4 || B <= 0 || TP <= 0 ||
      TP > 0x7fffffffLL / 8 || !(distance_threshold >= 0.0f))
    return RAP_ERR_INVALID;
  if ((R_pred == nullptr) != (t_pred == nullptr)) return RAP_ERR_INVALID;
  if (!ws) return RAP_ERR_WORKSPACE;
  PairWs w = carve_pair(TP, B, (char*)ws);
  if (w.total > ws_bytes) return RAP_ERR_WORKSPACE;
  return launch_pair_metrics((hipStream_t)stream, pointclouds_gt, cloud, points_per_part, cu_batch, scales, R_gt, t_gt, R_pred, t_pred, B,
                             (long)TP, distance_threshold, out4, w.items, w.partials, w.ranges);
}
extern "C" int rap_transform_errors_direct(const float* R_gt, const float* t_gt, const float* R_pred, const float* t_pred,
                                           const int64_t* points_per_part, const int64_t* matched_part_ids, const float* scale, int32_t B,
                                           int32_t P, float* rot_err_per_part, float* trans_err_per_part, float* rot_err_mean,
                                           float* trans_err_mean, void* stream) {
  if (!R_gt || !t_gt || !R_pred || !t_pred || !points_per_part || !rot_err_per_part || !trans_err_per_part || !rot_err_mean ||
      !trans_err_mean || B <= 0 || P <= 0)
    return RAP_ERR_INVALID;
  return launch_transform_errors_direct((hipStream_t)stream, R_gt, t_gt, R_pred, t_pred, points_per_part, matched_part_ids, scale, B, P,
                                        rot_err_per_part, trans_err_per_part, rot_err_mean, trans_err_mean);
}

// batched ICP: point-to-point or point-to-plane (icp.hip, icp_plane.hip), on the tiled search or on a uniform-grid neighbour index
// (nn_grid.hip).  The four entry points are one call (IcpCall, kernels.h) with two flags: plane (Y_normals given) and grid.
#define RAP_GRID_MAX_K 65535      // the build kernels take the problem from blockIdx.y
struct IcpWs { NnWork* items; void* partials; void* ranges; double* prev; int32_t* done; double* state; size_t total; };
// plane: the larger partials of the point-to-plane estimator, and its fp64 pose after everything else
// robust: the partials of the robust point-to-plane calls, which also carry the sum of the weights
static IcpWs carve_icp(int64_t n, int K, bool plane, char* basep, bool robust = false) {
  IcpWs w; Carver c(basep);
  const size_t max_items = nn_max_items((long)n, K);
  w.items = (NnWork*)c.take(max_items * sizeof(NnWork));
  w.partials = c.take(max_items * (robust ? icp_plane_robust_partial_bytes() : plane ? icp_plane_partial_bytes() : icp_partial_bytes()));
  w.ranges = c.take((size_t)K * 16);
  w.prev = (double*)c.take((size_t)K * 8);
  w.done = (int32_t*)c.take((size_t)K * 4);
  w.state = plane ? (double*)c.take((size_t)K * 12 * 8) : nullptr;
  w.total = c.total();
  return w;
}
static size_t icp_workspace_bytes(int64_t n_x_points, int64_t n_y_points, int K, bool plane, bool grid, bool robust = false) {
  if (n_x_points <= 0 || K <= 0 || (grid && n_y_points <= 0)) return 0;
  Carver c(nullptr);
  if (grid) nn_grid_carve(c, (long)n_y_points, K);
  return carve_icp(n_x_points, K, plane, nullptr, robust).total + c.total();
}
// c: the entry point's arguments, with the caller's max_correspondence_distance in gate; the workspace pointers are filled in here
static int icp_entry(IcpCall c, bool plane, bool grid, void* ws, size_t ws_bytes, void* stream) {
  if (!c.X || !c.x_seg || !c.Y || !c.y_seg || (plane && !c.Y_normals) || !c.R || !c.T || !c.rmse || !c.iterations || !c.converged ||
      c.K <= 0 || (grid && c.K > RAP_GRID_MAX_K) || c.max_iterations <= 0 || c.NX <= 0 || c.NY <= 0 || c.NX > 0x7fffffffLL / 8 ||
      c.NY > 0x7fffffffLL / 8 || c.relative_rmse_thr != c.relative_rmse_thr || c.gate != c.gate)
    return RAP_ERR_INVALID;
  if (c.robust && (c.loss < RAP_LOSS_NONE || c.loss > RAP_LOSS_TUKEY ||
                   (c.loss != RAP_LOSS_NONE && !(c.loss_scale > 0.f && c.loss_scale < __builtin_inff()))))
    return RAP_ERR_INVALID;
  if (!ws) return RAP_ERR_WORKSPACE;
  const IcpWs w = carve_icp(c.NX, c.K, plane, (char*)ws, c.robust != 0);
  Carver gc((char*)ws + w.total);
  NnGridWs g = {};
  if (grid) g = nn_grid_carve(gc, c.NY, c.K);
  if (w.total + gc.total() > ws_bytes) return RAP_ERR_WORKSPACE;
  c.gate = c.gate > 0.f ? c.gate : 0.f;
  c.items = w.items; c.partials = w.partials; c.ranges = w.ranges; c.prev = w.prev; c.done = w.done; c.state = w.state;
  c.grid = grid ? &g : nullptr;
  return launch_icp((hipStream_t)stream, c);
}
extern "C" size_t rap_icp_workspace_bytes(int64_t n_x_points, int32_t K) { return icp_workspace_bytes(n_x_points, 0, K, false, false); }
extern "C" size_t rap_icp_grid_workspace_bytes(int64_t n_x_points, int64_t n_y_points, int32_t K) {
  return icp_workspace_bytes(n_x_points, n_y_points, K, false, true);
}
extern "C" size_t rap_icp_plane_workspace_bytes(int64_t n_x_points, int32_t K) { return icp_workspace_bytes(n_x_points, 0, K, true, false); }
extern "C" size_t rap_icp_plane_grid_workspace_bytes(int64_t n_x_points, int64_t n_y_points, int32_t K) {
  return icp_workspace_bytes(n_x_points, n_y_points, K, true, true);
}
extern "C" int rap_icp(const float* X, const int32_t* x_seg, const float* Y, const int32_t* y_seg, int32_t K, int64_t NX, int64_t NY,
                       const float* init_R, const float* init_T, int32_t max_iterations, float relative_rmse_thr,
                       float max_correspondence_distance, float* R, float* T, float* rmse, int32_t* iterations, uint8_t* converged, float* Xt,
                       void* ws, size_t ws_bytes, void* stream) {
  const IcpCall c = {X, x_seg, Y, y_seg, nullptr, K, (long)NX, (long)NY, init_R, init_T, max_iterations, relative_rmse_thr,
                     max_correspondence_distance, R, T, rmse, iterations, converged, Xt};
  return icp_entry(c, false, false, ws, ws_bytes, stream);
}
extern "C" int rap_icp_grid(const float* X, const int32_t* x_seg, const float* Y, const int32_t* y_seg, int32_t K, int64_t NX, int64_t NY,
                            const float* init_R, const float* init_T, int32_t max_iterations, float relative_rmse_thr,
                            float max_correspondence_distance, float* R, float* T, float* rmse, int32_t* iterations, uint8_t* converged,
                            float* Xt, void* ws, size_t ws_bytes, void* stream) {
  const IcpCall c = {X, x_seg, Y, y_seg, nullptr, K, (long)NX, (long)NY, init_R, init_T, max_iterations, relative_rmse_thr,
                     max_correspondence_distance, R, T, rmse, iterations, converged, Xt};
  return icp_entry(c, false, true, ws, ws_bytes, stream);
}
extern "C" int rap_icp_plane(const float* X, const int32_t* x_seg, const float* Y, const int32_t* y_seg, const float* Y_normals, int32_t K,
                             int64_t NX, int64_t NY, const float* init_R, const float* init_T, int32_t max_iterations, float relative_rmse_thr,
                             float max_correspondence_distance, float* R, float* T, float* rmse, int32_t* iterations, uint8_t* converged,
                             float* Xt, void* ws, size_t ws_bytes, void* stream) {
  const IcpCall c = {X, x_seg, Y, y_seg, Y_normals, K, (long)NX, (long)NY, init_R, init_T, max_iterations, relative_rmse_thr,
                     max_correspondence_distance, R, T, rmse, iterations, converged, Xt};
  return icp_entry(c, true, false, ws, ws_bytes, stream);
}
extern "C" int rap_icp_plane_grid(const float* X, const int32_t* x_seg, const float* Y, const int32_t* y_seg, const float* Y_normals,
                                  int32_t K, int64_t NX, int64_t NY, const float* init_R, const float* init_T, int32_t max_iterations,
                                  float relative_rmse_thr, float max_correspondence_distance, float* R, float* T, float* rmse,
                                  int32_t* iterations, uint8_t* converged, float* Xt, void* ws, size_t ws_bytes, void* stream) {
  const IcpCall c = {X, x_seg, Y, y_seg, Y_normals, K, (long)NX, (long)NY, init_R, init_T, max_iterations, relative_rmse_thr,
                     max_correspondence_distance, R, T, rmse, iterations, converged, Xt};
  return icp_entry(c, true, true, ws, ws_bytes, stream);
}
// the robust twins (robust_loss.h): the siblings' calls with IcpCall::robust set
extern "C" size_t rap_icp_plane_robust_workspace_bytes(int64_t n_x_points, int32_t K) {
  return icp_workspace_bytes(n_x_points, 0, K, true, false, true);
}
extern "C" size_t rap_icp_plane_grid_robust_workspace_bytes(int64_t n_x_points, int64_t n_y_points, int32_t K) {
  return icp_workspace_bytes(n_x_points, n_y_points, K, true, true, true);
}
extern "C" int rap_icp_plane_robust(const float* X, const int32_t* x_seg, const float* Y, const int32_t* y_seg, const float* Y_normals,
                                    int32_t K, int64_t NX, int64_t NY, const float* init_R, const float* init_T, int32_t max_iterations,
                                    float relative_rmse_thr, float max_correspondence_distance, float* R, float* T, float* rmse,
                                    int32_t* iterations, uint8_t* converged, float* Xt, int32_t loss, float loss_scale, float* weights,
                                    void* ws, size_t ws_bytes, void* stream) {
  IcpCall c = {X, x_seg, Y, y_seg, Y_normals, K, (long)NX, (long)NY, init_R, init_T, max_iterations, relative_rmse_thr,
               max_correspondence_distance, R, T, rmse, iterations, converged, Xt};
  c.robust = 1; c.loss = loss; c.loss_scale = loss_scale; c.weights = weights;
  return icp_entry(c, true, false, ws, ws_bytes, stream);
}
extern "C" int rap_icp_plane_grid_robust(const float* X, const int32_t* x_seg, const float* Y, const int32_t* y_seg, const float* Y_normals,
                                         int32_t K, int64_t NX, int64_t NY, const float* init_R, const float* init_T, int32_t max_iterations,
                                         float relative_rmse_thr, float max_correspondence_distance, float* R, float* T, float* rmse,
                                         int32_t* iterations, uint8_t* converged, float* Xt, int32_t loss, float loss_scale, float* weights,
                                         void* ws, size_t ws_bytes, void* stream) {
  IcpCall c = {X, x_seg, Y, y_seg, Y_normals, K, (long)NX, (long)NY, init_R, init_T, max_iterations, relative_rmse_thr,
               max_correspondence_distance, R, T, rmse, iterations, converged, Xt};
  c.robust = 1; c.loss = loss; c.loss_scale = loss_scale; c.weights = weights;
  return icp_entry(c, true, true, ws, ws_bytes, stream);
}

// the neighbour index as an entry point of its own (nn_grid.hip), and the normals point-to-plane ICP needs (normals.hip)
extern "C" size_t rap_nn_grid_workspace_bytes(int64_t n_x_points, int64_t n_y_points, int32_t K) {
  if (n_x_points <= 0 || n_y_points <= 0 || K <= 0) return 0;
  Carver c(nullptr);
  c.take(nn_max_items((long)n_x_points, K) * sizeof(NnWork));
  nn_grid_carve(c, (long)n_y_points, K);
  return c.total();
}
extern "C" int rap_nearest_neighbors(const float* X, const int32_t* x_seg, const float* Y, const int32_t* y_seg, int32_t K, int64_t NX,
                                     int64_t NY, const float* R, const float* T, float max_distance, int32_t* idx_out, float* d2_out, void* ws,
                                     size_t ws_bytes, void* stream) {
  if (!X || !x_seg || !Y || !y_seg || !idx_out || !d2_out || K <= 0 || K > RAP_GRID_MAX_K || NX <= 0 || NY <= 0 || NX > 0x7fffffffLL / 8 ||
      NY > 0x7fffffffLL / 8 || max_distance != max_distance || (R == nullptr) != (T == nullptr))
    return RAP_ERR_INVALID;
  if (!ws) return RAP_ERR_WORKSPACE;
  Carver c(ws);
  NnWork* items = (NnWork*)c.take(nn_max_items((long)NX, K) * sizeof(NnWork));
  const NnGridWs g = nn_grid_carve(c, (long)NY, K);
  if (c.total() > ws_bytes) return RAP_ERR_WORKSPACE;
  return launch_nearest_neighbors((hipStream_t)stream, X, x_seg, Y, y_seg, K, (long)NX, (long)NY, R, T, max_distance > 0.f ? max_distance : 0.f,
                                  idx_out, d2_out, items, g);
}

extern "C" size_t rap_normals_workspace_bytes(int64_t n_points, int32_t K) {
  return (n_points <= 0 || K <= 0) ? 0 : align_up(nn_max_items((long)n_points, K) * sizeof(NnWork), 256) + align_up((size_t)K * 4, 256);
}
extern "C" int rap_estimate_normals(const float* P, const int32_t* seg, int32_t K, int64_t n_points, int32_t max_nn, float radius,
                                    const float* viewpoint, float* normals, float* eigenvalues, void* ws, size_t ws_bytes, void* stream) {
  if (!P || !seg || !normals || K <= 0 || n_points <= 0 || n_points > 0x7fffffffLL / 8 || max_nn < 3 || max_nn > 32 || radius != radius)
    return RAP_ERR_INVALID;
  if (!ws) return RAP_ERR_WORKSPACE;
  if (rap_normals_workspace_bytes(n_points, K) > ws_bytes) return RAP_ERR_WORKSPACE;
  Carver c(ws);
  NnWork* items = (NnWork*)c.take(nn_max_items((long)n_points, K) * sizeof(NnWork));
  int32_t* repeat = (int32_t*)c.take((size_t)K * 4);
  return launch_estimate_normals((hipStream_t)stream, P, seg, K, (long)n_points, max_nn, radius, viewpoint, normals, eigenvalues, items, repeat);
}

// the k-best walk over the same index (nn_knn.hip): the k nearest rows, and the grid paths of the normal estimation and (further down)
// of the outlier removal.  Each workspace is the brute-force or 1-NN call's own terms followed by the index
extern "C" size_t rap_knn_workspace_bytes(int64_t n_x_points, int64_t n_y_points, int32_t K) {
  return rap_nn_grid_workspace_bytes(n_x_points, n_y_points, K);
}
extern "C" int rap_k_nearest_neighbors(const float* X, const int32_t* x_seg, const float* Y, const int32_t* y_seg, int32_t K, int64_t NX,
                                       int64_t NY, int32_t k, float max_distance, int32_t* idx_out, float* d2_out, int32_t* count_out,
                                       void* ws, size_t ws_bytes, void* stream) {
  if (!X || !x_seg || !Y || !y_seg || !idx_out || !d2_out || !count_out || K <= 0 || K > RAP_GRID_MAX_K || NX <= 0 || NY <= 0 ||
      NX > 0x7fffffffLL / 8 || NY > 0x7fffffffLL / 8 || k < 1 || k > 32 || max_distance != max_distance)
    return RAP_ERR_INVALID;
  if (!ws) return RAP_ERR_WORKSPACE;
  Carver c(ws);
  NnWork* items = (NnWork*)c.take(nn_max_items((long)NX, K) * sizeof(NnWork));
  const NnGridWs g = nn_grid_carve(c, (long)NY, K);
  if (c.total() > ws_bytes) return RAP_ERR_WORKSPACE;
  return launch_k_nearest_neighbors((hipStream_t)stream, X, x_seg, Y, y_seg, K, (long)NX, (long)NY, k, max_distance, idx_out, d2_out,
                                    count_out, items, g);
}

extern "C" size_t rap_normals_grid_workspace_bytes(int64_t n_points, int32_t K) {
  if (n_points <= 0 || K <= 0) return 0;
  Carver c(nullptr);
  nn_grid_carve(c, (long)n_points, K);
  return rap_normals_workspace_bytes(n_points, K) + c.total();
}
extern "C" int rap_estimate_normals_grid(const float* P, const int32_t* seg, int32_t K, int64_t n_points, int32_t max_nn, float radius,
                                         const float* viewpoint, float* normals, float* eigenvalues, void* ws, size_t ws_bytes,
                                         void* stream) {
  if (!P || !seg || !normals || K <= 0 || K > RAP_GRID_MAX_K || n_points <= 0 || n_points > 0x7fffffffLL / 8 || max_nn < 3 || max_nn > 32 ||
      radius != radius)
    return RAP_ERR_INVALID;
  if (!ws) return RAP_ERR_WORKSPACE;
  Carver c(ws);
  NnWork* items = (NnWork*)c.take(nn_max_items((long)n_points, K) * sizeof(NnWork));
  int32_t* repeat = (int32_t*)c.take((size_t)K * 4);
  const NnGridWs g = nn_grid_carve(c, (long)n_points, K);
  if (c.total() > ws_bytes) return RAP_ERR_WORKSPACE;
  return launch_estimate_normals_grid((hipStream_t)stream, P, seg, K, (long)n_points, max_nn, radius, viewpoint, normals, eigenvalues, items,
                                      repeat, g);
}

// a consistent orientation for normals that exist already (orient.hip): the lists of the k-best walk, then the spanning forest
extern "C" size_t rap_orient_normals_workspace_bytes(int64_t n_points, int32_t K) {
  if (n_points <= 0 || K <= 0) return 0;
  Carver c(nullptr);
  orient_carve(c, (long)n_points, K);
  return c.total();
}
extern "C" int rap_orient_normals(const float* P, const int32_t* seg, int32_t K, int64_t n_points, int32_t k, const float* viewpoint,
                                  float* normals, int32_t* component_out, void* ws, size_t ws_bytes, void* stream) {
  if (!P || !seg || !normals || K <= 0 || K > RAP_GRID_MAX_K || n_points <= 0 || n_points > 0x7fffffffLL / 8 || k < 2 || k > 32)
    return RAP_ERR_INVALID;
  if (!ws) return RAP_ERR_WORKSPACE;
  Carver c(ws);
  const OrientWs w = orient_carve(c, (long)n_points, K);
  if (c.total() > ws_bytes) return RAP_ERR_WORKSPACE;
  return launch_orient_normals((hipStream_t)stream, P, seg, K, (long)n_points, k, viewpoint, normals, component_out, w);
}

extern "C" int rap_farthest_point_sampling(const float* points, const int32_t* cloud_start, const int32_t* cloud_len,
                                           const int32_t* k_per_cloud, const int32_t* start_idx, int32_t n_clouds, int32_t k_max,
                                           int32_t* indices_out, float* dist_ws, void* stream) {
  if (!points || !cloud_start || !cloud_len || !k_per_cloud || !start_idx || !indices_out || !dist_ws || n_clouds <= 0 || k_max <= 0)
    return RAP_ERR_INVALID;
  return launch_fps((hipStream_t)stream, points, cloud_start, cloud_len, k_per_cloud, start_idx, n_clouds, k_max, dist_ws, indices_out);
}

// ... over a bucket index (fps_grid.hip): the same tables, the same index lists.  The workspace holds the sorted rows and their running
// distances, 20 bytes per point; the bucket tables live in LDS, so the number of clouds does not enter
extern "C" size_t rap_fps_grid_workspace_bytes(int64_t total_points, int32_t n_clouds) {
  return total_points <= 0 || total_points > 0x7fffffffLL || n_clouds <= 0 ? 0 : fps_grid_workspace_bytes(total_points);
}
extern "C" void rap_fps_grid_params(int32_t* points_per_bucket, int32_t* max_buckets) {
  int per, mb, block;
  fps_grid_params(&per, &mb, &block);
  if (points_per_bucket) *points_per_bucket = per;
  if (max_buckets) *max_buckets = mb;
}
extern "C" int rap_farthest_point_sampling_grid(const float* points, int64_t total_points, const int32_t* cloud_start, const int32_t* cloud_len,
                                                const int32_t* k_per_cloud, const int32_t* start_idx, int32_t n_clouds, int32_t k_max,
                                                int32_t* indices_out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!points || !cloud_start || !cloud_len || !k_per_cloud || !start_idx || !indices_out || total_points < 0 || total_points > 0x7fffffffLL ||
      n_clouds <= 0 || k_max <= 0)
    return RAP_ERR_INVALID;
  const size_t need = fps_grid_workspace_bytes(total_points);              // 0 without a point: every cloud is empty, every row -1
  if ((need && !workspace) || workspace_bytes < need) return RAP_ERR_WORKSPACE;
  return launch_fps_grid((hipStream_t)stream, points, (long)total_points, cloud_start, cloud_len, k_per_cloud, start_idx, n_clouds, k_max, workspace,
                         indices_out);
}

// ---------------------------------------------------------------------------------------------
// voxel down-sampling (preprocessing)
// ---------------------------------------------------------------------------------------------
extern "C" int rap_voxel_bounds(const float* points, int64_t N, float voxel_size, int64_t* bounds6_out, float* dist_max_out,
                                void* stream) {
  if (!points || !bounds6_out || !dist_max_out || N <= 0 || !(voxel_size > 0.f)) return RAP_ERR_INVALID;
  return launch_voxel_bounds((hipStream_t)stream, points, (long)N, voxel_size, (long long*)bounds6_out, (unsigned int*)dist_max_out);
}
static int64_t voxel_slots(const int64_t* b) {
  int64_t v = 0;
  for (int a = 0; a < 3; ++a) v = (b[3 + a] - b[a]) > v ? (b[3 + a] - b[a]) : v;
  if (v > 2000000) return -1;
  const __int128 s = (__int128)v + (__int128)v * v + (__int128)v * v * v + 1;      // largest key gx + gy v + gz v^2 with g <= v, plus one
  return s > ((__int128)1 << 33) ? -1 : (int64_t)s;
}
extern "C" int64_t rap_voxel_table_slots(const int64_t* h_bounds6) { return h_bounds6 ? voxel_slots(h_bounds6) : -1; }
extern "C" size_t rap_voxel_workspace_bytes(const int64_t* h_bounds6) {
  const int64_t s = h_bounds6 ? voxel_slots(h_bounds6) : -1;
  if (s < 0) return 0;
  return align_up((size_t)s * 8, 256) + align_up((size_t)((s + 4095) / 4096) * 4, 256) + 256;
}
extern "C" int rap_voxel_downsample(const float* points, int64_t N, float voxel_size, const int64_t* h_bounds6, float dist_max,
                                    int64_t* indices_out, int32_t* count_out, void* ws, size_t ws_bytes, void* stream) {
  if (!points || !h_bounds6 || !indices_out || !count_out || N <= 0 || N > 0xffffffffLL || !(voxel_size > 0.f)) return RAP_ERR_INVALID;
  const int64_t slots = voxel_slots(h_bounds6);
  if (slots < 0) return RAP_ERR_INVALID;                 // grid too large for the dense table (> 2^33 slots = 64 GiB)
  if (!ws || ws_bytes < rap_voxel_workspace_bytes(h_bounds6)) return RAP_ERR_WORKSPACE;
  char* base = (char*)ws;
  unsigned long long* table = (unsigned long long*)base;
  unsigned int* block_cnt = (unsigned int*)(base + align_up((size_t)slots * 8, 256));
  return launch_voxel_downsample((hipStream_t)stream, points, (long)N, voxel_size, (const long long*)h_bounds6,
                                 dist_max > 0.f ? dist_max : 1.f, table, (long)slots, block_cnt, (unsigned int*)count_out,
                                 (long long*)indices_out);
}

// exact number of occupied voxels (calculate_voxel_coverage, point_sampling_utils.py:11-31): h_bounds6 from rap_voxel_bounds
static int64_t coverage_slots(const int64_t* b) {
  const __int128 s = (__int128)(b[3] - b[0] + 1) * (b[4] - b[1] + 1) * (b[5] - b[2] + 1);
  return (s <= 0 || s > ((__int128)1 << 36)) ? -1 : (int64_t)s;          // 64 GiB of one-byte slots
}
extern "C" size_t rap_voxel_coverage_workspace_bytes(const int64_t* h_bounds6) {
  const int64_t s = h_bounds6 ? coverage_slots(h_bounds6) : -1;
  return s < 0 ? 0 : align_up((size_t)s, 256) + 256;
}
extern "C" int rap_voxel_coverage(const float* points, int64_t N, float voxel_size, const int64_t* h_bounds6, int64_t* count_out, void* ws,
                                  size_t ws_bytes, void* stream) {
  if (!points || !h_bounds6 || !count_out || N <= 0 || !(voxel_size > 0.f)) return RAP_ERR_INVALID;
  const int64_t slots = coverage_slots(h_bounds6);
  if (slots < 0) return RAP_ERR_INVALID;
  if (!ws || ws_bytes < rap_voxel_coverage_workspace_bytes(h_bounds6)) return RAP_ERR_WORKSPACE;
  return launch_voxel_coverage((hipStream_t)stream, points, (long)N, voxel_size, (const long long*)h_bounds6, (unsigned char*)ws, (long)slots,
                               (unsigned long long*)count_out);
}

// O(N)-memory variants of the two calls above (voxel_sort.hip): identical results from a radix sort of per-point keys.  For grids whose
// dense table is large against N or beyond its 2^33 / 2^36-slot limits (a 100 m scene at 5 cm voxels = 64 GB of table).
extern "C" size_t rap_voxel_sorted_workspace_bytes(int64_t N) { return N > 0 && N <= 0xffffffffLL ? voxel_sorted_workspace_bytes((long)N) : 0; }
extern "C" int rap_voxel_downsample_sorted(const float* points, int64_t N, float voxel_size, const int64_t* h_bounds6, float dist_max,
                                           int64_t* indices_out, int32_t* count_out, void* ws, size_t ws_bytes, void* stream) {
  if (!points || !h_bounds6 || !indices_out || !count_out || N <= 0 || N > 0xffffffffLL || !(voxel_size > 0.f)) return RAP_ERR_INVALID;
  if (!ws) return RAP_ERR_WORKSPACE;
  return launch_voxel_downsample_sorted((hipStream_t)stream, points, (long)N, voxel_size, (const long long*)h_bounds6,
                                        dist_max > 0.f ? dist_max : 1.f, ws, ws_bytes, (long long*)indices_out, count_out);
}
extern "C" int rap_voxel_coverage_sorted(const float* points, int64_t N, float voxel_size, const int64_t* h_bounds6, int64_t* count_out,
                                         void* ws, size_t ws_bytes, void* stream) {
  if (!points || !h_bounds6 || !count_out || N <= 0 || N > 0xffffffffLL || !(voxel_size > 0.f)) return RAP_ERR_INVALID;
  if (!ws) return RAP_ERR_WORKSPACE;
  return launch_voxel_coverage_sorted((hipStream_t)stream, points, (long)N, voxel_size, (const long long*)h_bounds6, ws, ws_bytes,
                                      (long long*)count_out);
}

// ---------------------------------------------------------------------------------------------
// input side of the boundary: raw parts -> the packed batch
// ---------------------------------------------------------------------------------------------
extern "C" size_t rap_collate_workspace_bytes(int32_t B, int32_t P) {
  if (B <= 0 || P <= 0) return 0;
  return collate_workspace_bytes(B, P);
}

extern "C" int rap_collate_transform(const void* points, int32_t points_are_f64, const int64_t* points_per_part, int32_t B, int32_t P,
                                     int64_t TP, const int64_t* order, const float* feat_in, int32_t F, float* cond, float* gt,
                                     float* feat_out, uint8_t* anchor_indices, int64_t* part_indices, float* rotations,
                                     float* translations, float* scales, uint8_t* anchor_parts, float* global_translation,
                                     int64_t* cu_seqlens, int32_t* order_flag, void* ws, size_t ws_bytes, void* stream) {
  if (!points || !points_per_part || !cond || !gt || !anchor_indices || !part_indices || !rotations || !translations || !scales ||
      !anchor_parts || !global_translation || !cu_seqlens)
    return RAP_ERR_INVALID;
  if (B <= 0 || P <= 0 || P > 256 || (int64_t)B * P > 65535 || TP < 0 || TP > 0x7fffffffLL / 8 || F < 0) return RAP_ERR_INVALID;
  if (F > 0 && (!feat_in || !feat_out)) return RAP_ERR_INVALID;
  if (!ws || ws_bytes < collate_workspace_bytes(B, P)) return RAP_ERR_WORKSPACE;
  return launch_collate_transform((hipStream_t)stream, points, points_are_f64 ? 1 : 0, points_per_part, B, P, (long)TP, order, feat_in, F,
                                  cond, gt, feat_out, anchor_indices, part_indices, rotations, translations, scales, anchor_parts,
                                  global_translation, cu_seqlens, order_flag, ws);
}

// Consistency of a packed batch: see check_batch_kernel.  flag_out: device int32 (0 = consistent).
extern "C" int rap_check_batch(const int64_t* points_per_part, const int32_t* cu_batch, int32_t B, int32_t P, int64_t TP,
                               int32_t* flag_out, void* stream) {
  if (!points_per_part || !cu_batch || !flag_out || B <= 0 || P <= 0 || TP < 0) return RAP_ERR_INVALID;
  return launch_check_batch((hipStream_t)stream, points_per_part, cu_batch, B, P, (long)TP, flag_out);
}

extern "C" int rap_poison_on_flag(const int32_t* flag, float* buf, int64_t n, void* stream) {
  if (!flag || !buf || n < 0) return RAP_ERR_INVALID;
  return launch_poison_on_flag((hipStream_t)stream, flag, buf, (long)n);
}

// ---------------------------------------------------------------------------------------------
// statistical outlier removal (preprocessing)
// ---------------------------------------------------------------------------------------------
extern "C" size_t rap_outlier_workspace_bytes(int64_t N) { return N <= 0 ? 0 : outlier_workspace_bytes((long)N); }

extern "C" int rap_statistical_outliers(const float* points, int64_t N, int32_t nb_neighbors, double std_ratio, int64_t* inlier_indices,
                                        int32_t* count_out, double* stats_out, void* ws, size_t ws_bytes, void* stream) {
  if (!points || !inlier_indices || !count_out || N <= 0 || N > 0x7fffffffLL / 8 || nb_neighbors < 1 || nb_neighbors > 32 || !(std_ratio > 0.0))
    return RAP_ERR_INVALID;
  if (!ws || ws_bytes < outlier_workspace_bytes((long)N)) return RAP_ERR_WORKSPACE;
  return launch_statistical_outliers((hipStream_t)stream, points, (long)N, nb_neighbors, std_ratio, inlier_indices, count_out, stats_out, ws);
}

// ... with the mean neighbour distances from the k-best walk over the grid index (nn_knn.hip): the brute-force call's workspace, then the
// cloud's one segment, the work items and the index
struct OutlierGridWs { int32_t* seg; NnWork* items; NnGridWs g; size_t total; };
static OutlierGridWs carve_outlier_grid(int64_t N, char* base) {
  OutlierGridWs w;
  Carver c(base);
  c.take(outlier_workspace_bytes((long)N));
  w.seg = (int32_t*)c.take(2 * sizeof(int32_t));
  w.items = (NnWork*)c.take(nn_max_items((long)N, 1) * sizeof(NnWork));
  w.g = nn_grid_carve(c, (long)N, 1);
  w.total = c.total();
  return w;
}
extern "C" size_t rap_outlier_grid_workspace_bytes(int64_t N) { return N <= 0 ? 0 : carve_outlier_grid(N, nullptr).total; }

extern "C" int rap_statistical_outliers_grid(const float* points, int64_t N, int32_t nb_neighbors, double std_ratio, int64_t* inlier_indices,
                                             int32_t* count_out, double* stats_out, void* ws, size_t ws_bytes, void* stream) {
  if (!points || !inlier_indices || !count_out || N <= 0 || N > 0x7fffffffLL / 8 || nb_neighbors < 1 || nb_neighbors > 32 || !(std_ratio > 0.0))
    return RAP_ERR_INVALID;
  if (!ws) return RAP_ERR_WORKSPACE;
  const OutlierGridWs w = carve_outlier_grid(N, (char*)ws);
  if (w.total > ws_bytes) return RAP_ERR_WORKSPACE;
  return launch_statistical_outliers_grid((hipStream_t)stream, points, (long)N, nb_neighbors, std_ratio, inlier_indices, count_out, stats_out,
                                          ws, w.seg, w.items, w.g);
}

// QKV projection with MultiHeadRMSNorm fused into the epilogue (EPI_H_QKV_NORM): see rapflow.h
extern "C" int rap_gemm_h16_qkvnorm(int32_t dtype, const uint16_t* A, int32_t lda, const uint16_t* W, int32_t ldw, uint16_t* qk_out,
                                    int32_t M, int32_t K, int32_t heads, const float* gamma_q, const float* gamma_k, float q_mul,
                                    uint16_t* vt, int32_t vt_nblk, void* stream) {
  if (!A || !W || !qk_out || !gamma_q || !gamma_k || !vt || heads <= 0) return RAP_ERR_INVALID;
  GemmParamsH g = gemm_h16_params(A, lda, W, ldw, qk_out, 0, M, 3 * heads * 64, K, nullptr, 0);
  g.heads = heads; g.vt = vt; g.vt_nblk = vt_nblk; g.gamma_q = gamma_q; g.gamma_k = gamma_k; g.q_mul = q_mul;
  return launch_gemm_h16((hipStream_t)stream, dtype, EPI_H_QKV_NORM, g);
}
