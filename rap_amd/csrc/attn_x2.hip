// Variable-length, non-causal softmax attention with fp32-ACCURATE products on the fp16 matrix pipe (split precision, round 5).
//
// Third twin of attn_f32.hip / attn_h16.hip; replaces flash_attn.flash_attn_varlen_qkvpacked_func (flow_model/layer.py:106-111 per
// part, :123-128 per sample) for compute dtype RAP_DT_F32X2: every operand is an fp16 head + an fp16 tail (x = hi + lo, 22
// significand bits, half.h) and both contractions keep hi*hi + hi*lo + lo*hi in the MFMA's fp32 accumulators:
//     S^T = K_hi Q_hi^T + K_hi Q_lo^T + K_lo Q_hi^T        O^T += V_hi^T P_hi^T + V_hi^T P_lo^T + V_lo^T P_hi^T
// 3 x 32 cycles of v_mfma_f32_32x32x16_f16 per 16 contraction steps against 8 x 64 cycles of v_mfma_f32_32x32x2_f32 in the exact
// fp32 kernel (5.3 x fewer matrix-pipe cycles), with results at the fp32 kernel's distance from an fp64 evaluation
// (tests/test_x2_gpu.py; scripts/x2_emulation.py is the CPU model of the arithmetic).
//
// Layouts (paired, half.h): q, k [2][H][2 chunks][TP][64 physical] -- chunk c holds head dims 32c .. 32c+31 of every token as
// 32 heads | 32 tails (one 128-byte line per token and chunk), written by the QKV GEMM's fused qk-norm epilogue (gemm_h16.hip);
// v TRANSPOSED and blocked by 64 tokens, vt [H][block][2 chunks][64 d][64 physical]: chunk c holds the in-block positions
// 32c .. 32c+31 (vt_pos order) as 32 heads | 32 tails; out token-major paired (TP, 2 * H * 64) = the A operand of the out-projection.
//
// Structure = attn_h16.hip with the LDS-DMA stream (swapped products, a lane owns one query column, P fed back from the accumulator
// registers, online softmax with v_max3 row maxima and deferred rescale -- probabilities <= 2^11.5 fit fp16): every 64-key tile is
// FOUR 8 KB sub-tiles (K chunk 0 / 1, V^T chunk 0 / 1), each byte-for-byte a K or V^T tile of the 16-bit kernel (64 rows x 128 B,
// slot ^ ((row >> 1) & 7) swizzle), so a wave issues 4 LDS-DMA pieces per tile and the fragment of contraction step s lies in
// sub-tile s >> 1 at slots 2 (s & 1) + hi (heads) and 4 + 2 (s & 1) + hi (tails).  64 KB of LDS, one 8-wave block per CU.
// Few-token launches split every work item over 2 / 4 key ranges (SPLIT; attention_x2_combine_kernel merges the online-softmax partials).
#include "half.h"
#include "kernels.h"
#include "lds_dma.h"
#include "attn_tile.h"

#define XKV 64
#define XSUB (64 * 64)         // 16-bit elements of one sub-tile (8 KB)
#define XLD 72                 // row stride of the output slab (144 B)

// WPE = waves per SIMD the register allocation aims at: 2 (144 VGPRs, one block per CU) or 4 (128 VGPRs and 5 spilled, two blocks per CU
// -- the 64 KB of LDS allow both); tuning key 16 picks (A/B on the GPU: profiles/r05_*).
// SPLIT (few-token calls, round 5): gridDim.y blocks share the key tiles of a work item; each writes its UNNORMALISED partial O (fp32),
// its running maximum and its row sum, and attention_x2_combine_kernel merges them (online-softmax partials: O = sum_y O_y 2^((m_y - m) c) /
// sum_y l_y 2^((m_y - m) c)) and writes the head / tail planes.  One pair of 2 x 1024 points is 8 work items x 8 heads = 64 blocks for 256 CUs.
template <int WPE, bool SPLIT = false>
__global__ __launch_bounds__(512, WPE) void attention_x2_kernel(const u16* __restrict__ qk, const u16* __restrict__ vt, int vt_nblk,
                                                              u16* __restrict__ out, int TP, int heads,
                                                              const AttnWorkItem* __restrict__ items, float* __restrict__ part_o,
                                                              float* __restrict__ part_ml) {
  constexpr bool CAP = false;
  const float cap = 0.f;
#include "attn_x2_body.inc"
}
// CAP (the soft-capped form): unsplit
template <int WPE>
__global__ __launch_bounds__(512, WPE) void attention_x2_softcap_kernel(const u16* __restrict__ qk, const u16* __restrict__ vt, int vt_nblk,
                                                                      u16* __restrict__ out, int TP, int heads,
                                                                      const AttnWorkItem* __restrict__ items, float cap) {
  constexpr bool SPLIT = false, CAP = true;
  float* const part_o = nullptr;
  float* const part_ml = nullptr;
#include "attn_x2_body.inc"
}


// Measured and NOT kept (round 5, GPU call 2; source at commit "split-precision attention: software-pipelined kernel", numbers in
// profiles/r05_c2_x2_attention_pipelined_ab.jsonl): a software-pipelined form of this kernel -- the softmax of tile t + 1 interleaved, by
// sched_group_barrier, with the 24 P V MFMAs of tile t (K one tile ahead of V^T in the LDS ring, ping-pong P fragments, 200 VGPRs) so
// that a wave never stops issuing MFMAs for the ~180 VALU instructions of a tile's softmax: 5.99 / 11.44 ms per launch at L = 4096 /
// 8192 against 5.62 / 11.05 ms for this kernel, 43.4 k vs 45.1 k points/s for the whole call.  Two blocks per CU (WPE = 4) are no
// faster either.  As for the bf16 kernel, every schedule lands on the same ~1.2 PFLOP/s of issued fp16 MFMA work: the
// SQ counters (profiles/r05_c3_mfma_utilisation_x2.txt) show the clock the part sustains under this load, not the schedule, as the limit.
// Round 6 (GPU call 19, profiles/r06_c19_x2_attention_ring_latency.jsonl): the four-stage K / V^T ring that took the 16-bit kernel's few-token
// launches from 24.1 to 19.2 us (attn_h16.hip) was built for the SPLIT launches of this kernel too (128 KB of LDS, counted vmcnt, bit-identical)
// and changed nothing: 25.5 vs 25.4 ms per configs[0]-geometry call, 80.8 vs 80.5 at 4 096 rows.  A tile here is 48 MFMAs, ~350 VALU
// instructions and 32 ds_read_b128 per wave with all eight waves of the block working -- about 1 us each of matrix pipe, VALU and LDS
// bandwidth per tile and CU, executed phase by phase by waves that one barrier per tile keeps in step -- not the round trip of the next tile.
rap_tuning_t g_rap_attn_x2_wpe = 2;      // tuning key 16: 2 / 4 = one / two blocks per CU
extern rap_tuning_t g_rap_attn_split;    // attn_f32.hip, tuning key 5: split few-token attention launches over key ranges (1, default) or not (0)

// one thread per (token, 8 consecutive head dims): merge the key-range partials, normalise, write the head / tail planes
__global__ __launch_bounds__(256) void attention_x2_combine_kernel(const float* __restrict__ part_o, const float* __restrict__ part_ml,
                                                                   u16* __restrict__ out, int TP, int n_tokens, int heads, int splits,
                                                                   const int32_t* __restrict__ cover_cu, int cover_nseg) {
  const int dmodel = heads * 64;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)n_tokens * (dmodel / 8)) return;
  const long t = i / (dmodel / 8);
  const int c = (int)(i % (dmodel / 8)) * 8;                  // logical column: head = c >> 6, dims (c & 63) .. +7 (inside one 32-dim chunk)
  const int head = c >> 6;
  u16* dst = out + (size_t)t * (heads * 128) + head * 128 + ((c & 63) >> 5) * 64 + (c & 31);
  // a token outside every segment (an inconsistent table whose sanitised copy ends below n_tokens) has no partials: zeros, as the
  // unsplit kernel leaves such rows (the stale bytes of the aliased buffers used to be normalised by 1 / l = 1 / garbage)
  if (cover_cu && (t < cover_cu[0] || t >= cover_cu[cover_nseg])) {
    *reinterpret_cast<uint4*>(dst) = make_uint4(0, 0, 0, 0);
    *reinterpret_cast<uint4*>(dst + 32) = make_uint4(0, 0, 0, 0);
    return;
  }
  const float cexp = 0.125f * 1.44269504088896340736f;
  float m = -1e30f;
  for (int s = 0; s < splits; ++s) m = fmaxf(m, part_ml[(((size_t)s * TP + t) * heads + head) * 2]);
  float l = 0.f;
  f32x8 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < splits; ++s) {
    const float2 ml = *reinterpret_cast<const float2*>(part_ml + (((size_t)s * TP + t) * heads + head) * 2);
    const float w = __builtin_amdgcn_exp2f((ml.x - m) * cexp);       // an empty range: m_y = -1e30 -> weight 0 (and l_y = 0, O_y = 0)
    l += ml.y * w;
    const float4 a0 = *reinterpret_cast<const float4*>(part_o + ((size_t)s * TP + t) * dmodel + c);
    const float4 a1 = *reinterpret_cast<const float4*>(part_o + ((size_t)s * TP + t) * dmodel + c + 4);
    acc += f32x8{a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w} * w;
  }
  const float inv = l > 0.f ? 1.0f / l : 0.f;      // (every key range of a covered token saw at least one key: l > 0 there)
  x2_t8 h8, l8;
  x2_split8_nosat(acc * inv, h8, l8);
  *reinterpret_cast<uint4*>(dst) = __builtin_bit_cast(uint4, h8);
  *reinterpret_cast<uint4*>(dst + 32) = __builtin_bit_cast(uint4, l8);
}

// key ranges per work item of a few-token launch (1 = no split): work lists that leave most of the 256 one-block-per-CU slots empty
int attention_x2_splits(int max_items, int heads) {
  if (g_rap_attn_split == 0) return 1;
  const long blocks = (long)max_items * heads;
  return blocks <= 96 ? 4 : blocks <= 192 ? 2 : 1;
}

// part_o: splits x TP x heads*64 floats, part_ml: splits x TP x heads x 2 floats (splits > 1 only)
int launch_attention_x2(hipStream_t stream, const u16* qk, const u16* vt, int vt_nblk, u16* out, int TP, int heads,
                        const AttnWorkItem* items, int max_items, float* part_o, float* part_ml, int splits, int n_tokens,
                        const int32_t* cover_cu, int cover_nseg) {
  if (max_items <= 0 || TP <= 0) return RAP_OK;
  if (heads <= 0 || vt_nblk * 64 < TP) return RAP_ERR_INVALID;
  constexpr int LDS = 2 * 4 * XSUB * 2;      // 64 KB
  static_assert(8 * 32 * XLD * 2 <= LDS, "output slabs must fit the stages");
  if (splits > 1) {
    if (!part_o || !part_ml) return RAP_ERR_INVALID;
    if (int rc = rap_allow_dyn_lds(attention_x2_kernel<2, true>, LDS)) return rc;
    hipLaunchKernelGGL((attention_x2_kernel<2, true>), dim3(max_items * heads, splits), dim3(512), LDS, stream, qk, vt, vt_nblk, out, TP, heads, items,
                       part_o, part_ml);
    RAP_LAUNCH_CHECK();
    // only the rows that belong to a segment were written by a block: the filler rows of the padded buffers (n_tokens .. TP - 1) keep
    // the zeros prepare_static put there (they must stay finite: masked keys multiply their V column by p = 0)
    const int nt = n_tokens > 0 && n_tokens < TP ? n_tokens : TP;
    const long n8 = (long)nt * heads * 8;
    hipLaunchKernelGGL(attention_x2_combine_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, stream, part_o, part_ml, out, TP, nt, heads, splits,
                       cover_cu, cover_nseg);
    RAP_LAUNCH_CHECK();
    return RAP_OK;
  }
  float* const no = nullptr;
  const bool two = g_rap_attn_x2_wpe == 4;
  if (int rc = rap_allow_dyn_lds(two ? attention_x2_kernel<4> : attention_x2_kernel<2>, LDS)) return rc;
  if (two) hipLaunchKernelGGL(attention_x2_kernel<4>, dim3(max_items * heads), dim3(512), LDS, stream, qk, vt, vt_nblk, out, TP, heads, items, no, no);
  else hipLaunchKernelGGL(attention_x2_kernel<2>, dim3(max_items * heads), dim3(512), LDS, stream, qk, vt, vt_nblk, out, TP, heads, items, no, no);
  RAP_LAUNCH_CHECK();
  return RAP_OK;
}

// the soft-capped kernel (softcap > 0, finite: the entry points check): one form -- unsplit, one block per CU
int launch_attention_x2_softcap(hipStream_t stream, const u16* qk, const u16* vt, int vt_nblk, u16* out, int TP, int heads,
                                const AttnWorkItem* items, int max_items, float softcap) {
  if (max_items <= 0 || TP <= 0) return RAP_OK;
  if (heads <= 0 || vt_nblk * 64 < TP || !softcap_ok(softcap)) return RAP_ERR_INVALID;
  constexpr int LDS = 2 * 4 * XSUB * 2;      // 64 KB
  if (int rc = rap_allow_dyn_lds(attention_x2_softcap_kernel<2>, LDS)) return rc;
  hipLaunchKernelGGL(attention_x2_softcap_kernel<2>, dim3(max_items * heads), dim3(512), LDS, stream, qk, vt, vt_nblk, out, TP, heads, items, softcap);
  RAP_LAUNCH_CHECK();
  return RAP_OK;
}
