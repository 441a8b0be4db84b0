/* A consumer of include/rapflow.h written in plain C99 (tests/test_abi.py compiles it with gcc -std=c99 -pedantic, links it against
 * librapflow.so and runs it): what a non-Python binding of the boundary sees.  No GPU needed -- every call below is answered by the
 * host side of the library (version, workspace arithmetic, argument validation). */
#include <stdio.h>
#include <stddef.h>
#include "rapflow.h"

int main(void) {
  int fails = 0;
  char sentinel[256];
  if (rap_version() != RAPFLOW_ABI_VERSION) { printf("version %d != header %d\n", rap_version(), RAPFLOW_ABI_VERSION); ++fails; }
  if (rap_attention_workspace_bytes(262144, 64) == 0) { printf("attention workspace query\n"); ++fails; }
  if (rap_rigidity_workspace_bytes(64, 20, 32) == 0 || rap_rigidity_workspace_bytes(-1, 0, 0) != 0) { printf("rigidity workspace query\n"); ++fails; }
  if (rap_set_tuning(-1, 0) != RAP_ERR_INVALID) { printf("tuning key -1 accepted\n"); ++fails; }
  /* NULL operands and bad strides are refused before any launch */
  if (rap_x2_gemm(1, NULL, 1024, (const uint16_t*)sentinel, 1024, sentinel, 512, 256, 512, 1024, NULL, NULL, 0, 1.0f, 0, NULL, NULL, 8.0f, NULL, 0, NULL) != RAP_ERR_INVALID) { printf("x2 gemm NULL A\n"); ++fails; }
  if (rap_x2_gemm(1, (const uint16_t*)sentinel, 1024, (const uint16_t*)sentinel, 1024, sentinel, 514, 256, 512, 1024, NULL, NULL, 0, 1.0f, 0, NULL, NULL, 8.0f, NULL, 0, NULL) != RAP_ERR_INVALID) { printf("x2 gemm ldc 514\n"); ++fails; }
  /* the split-KV attention entry points: the query is host arithmetic, NULL operands / a splits value that is none of 1, 2, 4 / a split
   * without a logit bound are refused, and a short workspace is refused before anything is written */
  if (rap_attention_split_workspace_bytes(2048, 2, 8, 1) != rap_attention_workspace_bytes(2048, 2) ||
      rap_attention_split_workspace_bytes(2048, 2, 8, 4) != rap_attention_workspace_bytes(2048, 2) + (size_t)4 * 2048 * 8 * (64 + 2) * 4 ||
      rap_attention_split_workspace_bytes(2048, 2, 8, 3) != 0 || rap_attention_split_workspace_bytes(2048, 2, 0, 2) != 0) { printf("split attention workspace query\n"); ++fails; }
  if (rap_attention_f32_split(NULL, (const int32_t*)sentinel, 1, (float*)sentinel, 256, 8, (const float*)sentinel, 2, sentinel, (size_t)1 << 30, NULL) != RAP_ERR_INVALID) { printf("f32 split attention NULL qkv\n"); ++fails; }
  if (rap_attention_f32_split((const float*)sentinel, (const int32_t*)sentinel, 1, NULL, 256, 8, (const float*)sentinel, 2, sentinel, (size_t)1 << 30, NULL) != RAP_ERR_INVALID) { printf("f32 split attention NULL out\n"); ++fails; }
  if (rap_attention_f32_split((const float*)sentinel, NULL, 1, (float*)sentinel, 256, 8, (const float*)sentinel, 2, sentinel, (size_t)1 << 30, NULL) != RAP_ERR_INVALID) { printf("f32 split attention NULL cu_seqlens\n"); ++fails; }
  if (rap_attention_f32_split((const float*)sentinel, (const int32_t*)sentinel, 1, (float*)sentinel, 256, 8, NULL, 2, sentinel, (size_t)1 << 30, NULL) != RAP_ERR_INVALID) { printf("f32 split attention without a bound\n"); ++fails; }
  if (rap_attention_f32_split((const float*)sentinel, (const int32_t*)sentinel, 1, (float*)sentinel, 256, 8, (const float*)sentinel, 3, sentinel, (size_t)1 << 30, NULL) != RAP_ERR_INVALID) { printf("f32 split attention splits 3\n"); ++fails; }
  if (rap_attention_f32_split((const float*)sentinel, (const int32_t*)sentinel, 1, (float*)sentinel, 256, 8, (const float*)sentinel, 2, NULL, (size_t)1 << 30, NULL) != RAP_ERR_WORKSPACE) { printf("f32 split attention NULL workspace\n"); ++fails; }
  if (rap_attention_f32_split((const float*)sentinel, (const int32_t*)sentinel, 1, (float*)sentinel, 256, 8, (const float*)sentinel, 2, sentinel, rap_attention_split_workspace_bytes(256, 1, 8, 2) - 1, NULL) != RAP_ERR_WORKSPACE) { printf("f32 split attention short workspace\n"); ++fails; }
  if (rap_x2_attention_split(NULL, (const uint16_t*)sentinel, 4, (const int32_t*)sentinel, 1, (uint16_t*)sentinel, 256, 0, 8, 2, sentinel, (size_t)1 << 30, NULL) != RAP_ERR_INVALID) { printf("x2 split attention NULL qk\n"); ++fails; }
  if (rap_x2_attention_split((const uint16_t*)sentinel, NULL, 4, (const int32_t*)sentinel, 1, (uint16_t*)sentinel, 256, 0, 8, 2, sentinel, (size_t)1 << 30, NULL) != RAP_ERR_INVALID) { printf("x2 split attention NULL vt\n"); ++fails; }
  if (rap_x2_attention_split((const uint16_t*)sentinel, (const uint16_t*)sentinel, 4, (const int32_t*)sentinel, 1, NULL, 256, 0, 8, 2, sentinel, (size_t)1 << 30, NULL) != RAP_ERR_INVALID) { printf("x2 split attention NULL out\n"); ++fails; }
  if (rap_x2_attention_split((const uint16_t*)sentinel, (const uint16_t*)sentinel, 4, NULL, 1, (uint16_t*)sentinel, 256, 0, 8, 2, sentinel, (size_t)1 << 30, NULL) != RAP_ERR_INVALID) { printf("x2 split attention NULL cu_seqlens\n"); ++fails; }
  if (rap_x2_attention_split((const uint16_t*)sentinel, (const uint16_t*)sentinel, 4, (const int32_t*)sentinel, 1, (uint16_t*)sentinel, 256, 257, 8, 2, sentinel, (size_t)1 << 30, NULL) != RAP_ERR_INVALID) { printf("x2 split attention n_tokens above TP\n"); ++fails; }
  if (rap_x2_attention_split((const uint16_t*)sentinel, (const uint16_t*)sentinel, 3, (const int32_t*)sentinel, 1, (uint16_t*)sentinel, 256, 0, 8, 2, sentinel, (size_t)1 << 30, NULL) != RAP_ERR_INVALID) { printf("x2 split attention short V^T image\n"); ++fails; }
  if (rap_x2_attention_split((const uint16_t*)sentinel, (const uint16_t*)sentinel, 4, (const int32_t*)sentinel, 1, (uint16_t*)sentinel, 256, 0, 8, 4, sentinel, rap_attention_split_workspace_bytes(256, 1, 8, 4) - 1, NULL) != RAP_ERR_WORKSPACE) { printf("x2 split attention short workspace\n"); ++fails; }
  /* the GEMM dispatch decision and the fp32 split-K entry point: host arithmetic, refusals before any launch */
  if (rap_gemm_f32_form(0, 300, 512, 512, 512, 512, 512, 0, 0, 0) != 121 || rap_gemm_f32_form(0, 16129, 2048, 256, 256, 256, 2048, 0, 0, 0) != 201 ||
      rap_gemm_f32_form(0, 16384, 2048, 256, 256, 256, 2048, 0, 0, 0) != 301 || rap_gemm_f32_form(1, 2048, 512, 512, 512, 512, 512, 512, 1, 0) != 124 ||
      rap_gemm_f32_form(0, 300, 500, 512, 512, 512, 500, 0, 0, 0) != RAP_ERR_INVALID || rap_gemm_f32_form(0, 0, 512, 512, 512, 512, 512, 0, 0, 0) != 0) { printf("fp32 gemm form\n"); ++fails; }
  if (rap_gemm_h16_form(1, 0, 300, 256, 512, 512, 512, 0) != 141 || rap_gemm_h16_form(2, 0, 8200, 512, 64, 64, 64, 0) != 121 ||
      rap_gemm_h16_form(1, 0, 7937, 2048, 128, 128, 128, 0) != 201 || rap_gemm_h16_form(3, 1, 16384, 2048, 128, 128, 128, 0) != 301 ||
      rap_gemm_h16_form(1, 1, 2048, 512, 1024, 1024, 1024, 1) != 144 || rap_gemm_h16_form(1, 6, 300, 256, 512, 512, 512, 0) != RAP_ERR_INVALID) { printf("16-bit gemm form\n"); ++fails; }
  if (rap_gemm_f32_splitk_workspace_bytes(1, 2048, 512, 544, 0) != (size_t)4 * 2048 * 512 * 4 || rap_gemm_f32_splitk_workspace_bytes(1, 2049, 512, 544, 0) != 0 ||
      rap_gemm_f32_splitk_workspace_bytes(2, 257, 384, 576, 2) != (size_t)2 * 257 * 384 * 4 || rap_gemm_f32_splitk_workspace_bytes(2, 257, 384, 544, 2) != 0) { printf("fp32 split-K workspace query\n"); ++fails; }
  if (rap_gemm_f32_splitk(1, NULL, 512, (const float*)sentinel, 512, (float*)sentinel, 512, 100, 512, 512, NULL, (const float*)sentinel, 512, 0, sentinel, (size_t)1 << 30, NULL) != RAP_ERR_INVALID) { printf("fp32 split-K NULL A\n"); ++fails; }
  if (rap_gemm_f32_splitk(0, (const float*)sentinel, 512, (const float*)sentinel, 512, (float*)sentinel, 512, 100, 512, 512, NULL, (const float*)sentinel, 512, 0, sentinel, (size_t)1 << 30, NULL) != RAP_ERR_INVALID) { printf("fp32 split-K epilogue 0\n"); ++fails; }
  if (rap_gemm_f32_splitk(2, (const float*)sentinel, 512, (const float*)sentinel, 512, (float*)sentinel, 128, 100, 128, 512, NULL, NULL, 0, 3, sentinel, (size_t)1 << 30, NULL) != RAP_ERR_INVALID) { printf("fp32 split-K planes 3\n"); ++fails; }
  if (rap_gemm_f32_splitk(1, (const float*)sentinel, 512, (const float*)sentinel, 512, (float*)sentinel, 512, 100, 512, 512, NULL, (const float*)sentinel, 512, 0, sentinel, (size_t)4 * 100 * 512 * 4 - 1, NULL) != RAP_ERR_WORKSPACE) { printf("fp32 split-K short workspace\n"); ++fails; }
  /* the residual-stream LayerNorm / fused combine + LayerNorm / stream conversion entry points: every argument is checked before any
   * launch, an empty row count included (the launchers behind them would answer RAP_OK to 0 rows without looking at d) */
  if (rap_layernorm_mod_h16_stream(2, NULL, 1, (uint16_t*)sentinel, 4, 512, (const float*)sentinel, 0, NULL, NULL) != RAP_ERR_INVALID) { printf("stream LN NULL x\n"); ++fails; }
  if (rap_layernorm_mod_h16_stream(3, sentinel, 1, (uint16_t*)sentinel, 4, 512, (const float*)sentinel, 0, NULL, NULL) != RAP_ERR_INVALID) { printf("stream LN dtype 3 on an fp16 stream\n"); ++fails; }
  if (rap_layernorm_mod_h16_stream(2, sentinel, 1, (uint16_t*)sentinel, 0, 384, (const float*)sentinel, 0, NULL, NULL) != RAP_ERR_INVALID) { printf("stream LN d 384 at 0 rows\n"); ++fails; }
  if (rap_layernorm_affine_h16_stream(1, sentinel, 2, (uint16_t*)sentinel, 4, 512, (const float*)sentinel, (const float*)sentinel, NULL) != RAP_ERR_INVALID) { printf("stream LN x_f16 2\n"); ++fails; }
  if (rap_layernorm_affine_h16_stream(1, sentinel, 0, (uint16_t*)sentinel, 4, 512, (const float*)sentinel, NULL, NULL) != RAP_ERR_INVALID) { printf("stream LN NULL shift\n"); ++fails; }
  if (rap_layernorm_affine_h16_stream(0, sentinel, 0, (uint16_t*)sentinel, 0, 512, (const float*)sentinel, (const float*)sentinel, NULL) != RAP_ERR_INVALID) { printf("stream LN dtype 0 at 0 rows\n"); ++fails; }
  if (rap_resid_combine_layernorm_h16(2, NULL, 2, NULL, sentinel, 1, (uint16_t*)sentinel, 4, 512, (const float*)sentinel, 0, NULL, NULL, NULL, NULL) != RAP_ERR_INVALID) { printf("combine LN NULL part\n"); ++fails; }
  if (rap_resid_combine_layernorm_h16(2, (const float*)sentinel, 9, NULL, sentinel, 1, (uint16_t*)sentinel, 0, 512, (const float*)sentinel, 0, NULL, NULL, NULL, NULL) != RAP_ERR_INVALID) { printf("combine LN splits 9 at 0 rows\n"); ++fails; }
  if (rap_resid_combine_layernorm_h16(2, (const float*)sentinel, 0, NULL, sentinel, 1, (uint16_t*)sentinel, 4, 512, (const float*)sentinel, 0, NULL, NULL, NULL, NULL) != RAP_ERR_INVALID) { printf("combine LN splits 0\n"); ++fails; }
  if (rap_resid_combine_layernorm_h16(2, (const float*)sentinel, 2, NULL, sentinel, 1, (uint16_t*)sentinel, 4, 512, NULL, 0, NULL, (const float*)sentinel, NULL, NULL) != RAP_ERR_INVALID) { printf("combine LN neither mod nor gain and shift\n"); ++fails; }
  if (rap_resid_combine_layernorm_h16(3, (const float*)sentinel, 2, NULL, sentinel, 1, (uint16_t*)sentinel, 4, 512, (const float*)sentinel, 0, NULL, NULL, NULL, NULL) != RAP_ERR_INVALID) { printf("combine LN dtype 3 on an fp16 stream\n"); ++fails; }
  if (rap_resid_combine_layernorm_h16(2, (const float*)sentinel, 2, NULL, sentinel, 1, (uint16_t*)sentinel, -1, 512, (const float*)sentinel, 0, NULL, NULL, NULL, NULL) != RAP_ERR_INVALID) { printf("combine LN negative rows\n"); ++fails; }
  if (rap_convert_f16_sat(NULL, (uint16_t*)sentinel, 8, NULL) != RAP_ERR_INVALID || rap_convert_f16_sat((const float*)sentinel, (uint16_t*)sentinel, 6, NULL) != RAP_ERR_INVALID ||
      rap_convert_f16_sat((const float*)sentinel, (uint16_t*)sentinel, -4, NULL) != RAP_ERR_INVALID) { printf("saturating conversion\n"); ++fails; }
  if (rap_convert_f16_to_f32((const uint16_t*)sentinel, NULL, 8, NULL) != RAP_ERR_INVALID || rap_convert_f16_to_f32((const uint16_t*)sentinel, (float*)sentinel, 12, NULL) != RAP_ERR_INVALID ||
      rap_convert_f16_to_f32((const uint16_t*)sentinel, (float*)sentinel, -8, NULL) != RAP_ERR_INVALID) { printf("fp16 -> fp32 conversion\n"); ++fails; }
  /* the kernels between the GEMMs: a row count beyond an int is refused, never truncated (2^32 + 4 is not 4), and so is every other bad
   * argument at 0 rows; the four entry points of the small kernels check theirs the same way */
  if (rap_layernorm_mod((const float*)sentinel, (float*)sentinel, ((int64_t)1 << 32) + 4, 512, (const float*)sentinel, 0, NULL, NULL) != RAP_ERR_INVALID ||
      rap_layernorm_affine((const float*)sentinel, (float*)sentinel, 0, 384, (const float*)sentinel, (const float*)sentinel, NULL) != RAP_ERR_INVALID ||
      rap_layernorm_affine((const float*)sentinel, (float*)sentinel, 0, 768, (const float*)sentinel, (const float*)sentinel, NULL) != RAP_OK) { printf("fp32 LayerNorm arguments\n"); ++fails; }
  if (rap_qknorm((float*)sentinel, ((int64_t)1 << 32) + 4, 8, (const float*)sentinel, (const float*)sentinel, NULL) != RAP_ERR_INVALID ||
      rap_qknorm((float*)sentinel, 4, 0, (const float*)sentinel, (const float*)sentinel, NULL) != RAP_ERR_INVALID ||
      rap_qknorm_h16(1, (uint16_t*)sentinel, 0, -1, (const float*)sentinel, (const float*)sentinel, NULL) != RAP_ERR_INVALID) { printf("qk-norm arguments\n"); ++fails; }
  if (rap_posenc_x((const float*)sentinel, (float*)sentinel, ((int64_t)1 << 32) + 4, NULL) != RAP_ERR_INVALID ||
      rap_posenc_static((const float*)sentinel, (const float*)sentinel, (const int32_t*)sentinel, NULL, 8, (float*)sentinel, 4, NULL) != RAP_ERR_INVALID ||
      rap_posenc_static((const float*)sentinel, (const float*)sentinel, (const int32_t*)sentinel, NULL, 0, (float*)sentinel, 0, NULL) != RAP_OK) { printf("posenc arguments\n"); ++fails; }
  if (rap_head_out3(NULL, 256, (const float*)sentinel, (float*)sentinel, 4, 256, NULL) != RAP_ERR_INVALID ||
      rap_head_out3((const float*)sentinel, 256, (const float*)sentinel, (float*)sentinel, 4, 192, NULL) != RAP_ERR_INVALID ||
      rap_head_out3((const float*)sentinel, 128, (const float*)sentinel, (float*)sentinel, 4, 256, NULL) != RAP_ERR_INVALID ||
      rap_head_out3((const float*)sentinel, 256, (const float*)sentinel, (float*)sentinel, 0, 256, NULL) != RAP_OK) { printf("head tail arguments\n"); ++fails; }
  if (rap_max_abs(NULL, 4, (float*)sentinel, NULL) != RAP_ERR_INVALID || rap_max_abs((const float*)sentinel, -1, (float*)sentinel, NULL) != RAP_ERR_INVALID ||
      rap_max_abs((const float*)sentinel, 0, (float*)sentinel, NULL) != RAP_OK) { printf("max |x| arguments\n"); ++fails; }
  if (rap_qk_logit_bound((const float*)sentinel, (const float*)sentinel, 0, (float*)sentinel, NULL) != RAP_ERR_INVALID ||
      rap_qk_logit_bound((const float*)sentinel, NULL, 8, (float*)sentinel, NULL) != RAP_ERR_INVALID) { printf("logit bound arguments\n"); ++fails; }
  if (rap_sanitize_cu(NULL, 4, 100, (int32_t*)sentinel, NULL) != RAP_ERR_INVALID || rap_sanitize_cu((const int32_t*)sentinel, -1, 100, (int32_t*)sentinel, NULL) != RAP_ERR_INVALID ||
      rap_sanitize_cu((const int32_t*)sentinel, 4, -1, (int32_t*)sentinel, NULL) != RAP_ERR_INVALID ||
      rap_sanitize_cu((const int32_t*)sentinel, 0, 100, (int32_t*)sentinel, NULL) != RAP_OK) { printf("segment-table sanitiser arguments\n"); ++fails; }
  if (rap_model_set_compute_dtype(NULL, 3, NULL) != RAP_ERR_INVALID) { printf("NULL model\n"); ++fails; }
  printf("c consumer: %d failure(s), ABI version %d\n", fails, rap_version());
  return fails;
}
