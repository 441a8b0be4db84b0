// Variable-length, non-causal softmax attention in fp32 on the CDNA4 matrix cores.
//
// Replaces flash_attn.flash_attn_varlen_qkvpacked_func as called by the reference at
// flow_model/layer.py:106-111 (per part) and :123-128 (per sample): for every segment of
// cu_seqlens and every head,  out = softmax(q k^T / sqrt(64)) v  with no attention across segments.
//
// Layout: q/k/v are head-major [3][H][TP][64] fp32 (written by the QKV GEMM epilogue), so each
// (segment, head) problem is three dense (L,64) matrices; out is token-major (TP, H*64).
//
// Design (gfx950 only; Dh = 64):
//  * flash-style online softmax; a block = 256 query rows of one (segment, head) -- 4 waves x 64 rows;
//    K/V are streamed in 64-key tiles through double-buffered LDS (global -> regs -> LDS).
//  * "swapped" products on v_mfma_f32_32x32x2_f32 (exact fp32):
//      S^T (key x query) = K (key x d) * Q^T (d x query)    -- A operand from LDS, B operand = Q in VGPRs
//      O^T (d x query)   = V^T (d x key) * P^T (key x query) -- A operand from LDS, B operand = P in VGPRs
//    In the 32x32 C/D layout a lane then owns ONE query column (lane & 31) and 16 of the 32 keys, so the
//    whole softmax state (running max, running sum, rescale of O) is lane-local; one cross-half
//    exchange (lane ^ 32) per 32-key tile completes the row max.
//  * No data movement between the two products: MFMA step r of P*V contracts the key pair
//    {crow(r,0), crow(r,1)} = exactly the keys whose probabilities already sit in accumulator register r
//    of the two half-waves, so P's registers are fed straight back as the B operand.
//  * d is permuted between the two O tiles (tile e holds d = 2c + e) so that one ds_read_b64 of V
//    feeds both; the permutation is undone in the store.
//  * Contraction order over d in Q*K^T is permuted as in the GEMM (one ds_read_b128 -> four MFMAs).
//  * softmax scale and log2(e) are folded into Q when it is loaded; exponentials are v_exp_f32.
//  * grid = work items x heads with head = blockIdx % H (blockIdx % 8 is the XCD on MI355X: each XCD's
//    L2 then serves the K/V of one head).
#include "kernels.h"
#include "attn_tile.h"

// Measured and NOT kept (round 3, call 22): K / V tiles by LDS-DMA (global_load_lds_dwordx4, 256-byte K rows with a slot ^ (row & 15) swizzle)
// instead of through staging registers -- bit-identical output, 196 instead of 228-242 VGPRs, and exactly the same speed (141.7 vs
// 141.8 TF per sample, 140.8 vs 141.2 per part): at 64 cycles per MFMA the 8 loads + 8 ds_write_b128 of a tile are noise.  The same
// change is worth +3.5 % in the 16-bit kernel (attn_h16.hip), where a tile is 16x shorter.
#define AQ_WAVE 64
#define AKV 64
#define KLD 68  // K LDS row stride (floats): 272 B = 17 slots -> conflict-free ds_read_b128
#define VLD 64
// scheduling fence: VALU (0x2), SALU (0x4) and transcendental (0x400) instructions may cross; DS, MFMA, VMEM may not
#define ATTN_FENCE __builtin_amdgcn_sched_barrier(0x406);

// NW = waves per block (4: 256 queries, two blocks per CU; 8: 512 queries, one block per CU).  With NW = 8 the
// two waves that share a SIMD (w and w+4) belong to the SAME block and get different static priorities: with equal
// priority two identical waves share the matrix pipe fairly, stay in lock-step and hit their softmax (VALU) phases
// together, leaving the pipe idle; with a priority split the favoured wave runs its MFMA phases at full rate and
// the other one fills its gaps (MI355X_MICROARCH.md "Two waves per SIMD", item 4).
// BOUNDED: the caller guarantees q.k/8 <= bound[head] for every pair (after the reference's qk-norm
// bound = 8 max|gamma_q| max|gamma_k|, a property of the weights).  The softmax is then evaluated with that constant as
// its offset, p = exp(s - bound): no running maximum, no rescale of O, ~1/3 of the VALU work between the two MFMA phases
// (the section that costs the online version its last 13 % of the matrix peak).  Same softmax, different rounding points.
// SPLIT (few-token calls, BOUNDED only): gridDim.y key ranges per (work item, head).  With the offset-free softmax the partial
// results of disjoint key ranges simply ADD (numerators and row sums share the common factor 1), so every range writes its
// un-normalised O and l to a scratch plane and attention_combine_kernel divides the sums: 4x the blocks for a call whose work
// list would otherwise cover a quarter of the CUs.
template <int NW, bool BOUNDED, bool SPLIT = false>
__global__ __launch_bounds__(64 * NW, 2) void attention_f32_kernel(const float* __restrict__ qkv, float* __restrict__ out,
                                                                  int TP, int heads, const AttnWorkItem* __restrict__ items,
                                                                  const float* __restrict__ bound, float* __restrict__ part_o,
                                                                  float* __restrict__ part_l) {
  constexpr bool CAP = false;
  const float cap = 0.f;
#include "attn_f32_body.inc"
}
// CAP (the soft-capped form, online softmax only): every logit s = q.k/8 becomes cap * tanh(s / cap) before the softmax sees it
// (flash-attn's softcap).  One form: 4 waves x 64 queries, never split.
template <int NW>
__global__ __launch_bounds__(64 * NW, 2) void attention_f32_softcap_kernel(const float* __restrict__ qkv, float* __restrict__ out,
                                                                          int TP, int heads, const AttnWorkItem* __restrict__ items,
                                                                          float cap) {
  constexpr bool BOUNDED = false, SPLIT = false, CAP = true;
  const float* const bound = nullptr;
  float* const part_o = nullptr;
  float* const part_l = nullptr;
#include "attn_f32_body.inc"
}

// Work list of one attention launch: one item per 256-query block of every segment, LONGEST SEGMENT FIRST (round 4).  A block's
// work is proportional to its segment's length (it streams all keys of the segment), and blocks are dispatched in blockIdx order:
// with the items in segment order the 157 x 8 blocks of a 40 000-point part at the end of a ragged batch start last and the launch
// drains on them alone; longest-processing-time-first puts the short blocks at the tail (the reference's batches are ragged:
// 200 ... 40 000 points per part, config/RAP_inference.yaml:30-36).  Items of one segment stay adjacent, so the 8 blocks x
// consecutive items that share an XCD's L2 still share K / V.  One block of 1024 threads, once per sample() call:
//   rank[s] = #{j : len_j > len_s or (len_j == len_s and j < s)}  (lengths staged through LDS, O(nseg^2 / 1024) per thread),
//   order[rank[s]] = s, exclusive scan of the item counts in rank order, then every thread emits the items of its ranks.
// sort_ws: nseg ints; nullptr = segment order (kernel-level entry points without scratch).
#define WL_THREADS 1024
#define WL_TILE 4096
#define WL_SORT_MAX 8192
// a segment's length as every stage of the kernel sees it: never negative (a decreasing table -- reachable through the kernel-level
// entry point, or under deferred validation before round 5 sanitised the tables -- made the item count negative)
__device__ __forceinline__ int wl_len(const int32_t* __restrict__ cu, int s) { const int l = cu[s + 1] - cu[s]; return l > 0 ? l : 0; }
__global__ __launch_bounds__(WL_THREADS) void build_attn_worklist_kernel(const int32_t* __restrict__ cu, int nseg, AttnWorkItem* __restrict__ items,
                                                                          int max_items, int bq, int32_t* __restrict__ sort_ws) {
  if (blockIdx.x != 0) return;
  const int tid = threadIdx.x;
  const AttnWorkItem none = {0, 0, 0, 0};
  if (!sort_ws) {
    if (tid != 0) return;
    int n = 0;
    for (int s = 0; s < nseg; ++s) {
      const int a = cu[s], len = wl_len(cu, s);
      for (int q0 = 0; q0 < len && n < max_items; q0 += bq) { const AttnWorkItem w = {a, len, q0, 0}; items[n++] = w; }
    }
    for (; n < max_items; ++n) items[n] = none;
    return;
  }
  __shared__ int lens[WL_TILE];
  __shared__ int partial[WL_THREADS];
  __shared__ int total_items;
  int32_t* order = sort_ws;            // [nseg]
  // ---- ranks.  O(nseg^2 / 1024) compares per thread on ONE CU: fine for the hundreds of parts of a real batch, ~4 M per thread at the
  // 65 535-part limit (milliseconds at the head of every call) -- above WL_SORT_MAX segments the items are emitted in
  // segment order by the same parallel scan (such batches consist of many short segments: there is no long tail to hide)
  if (nseg > WL_SORT_MAX) {
    for (int s = tid; s < nseg; s += WL_THREADS) order[s] = s;
  } else
  for (int s0 = 0; s0 < nseg; s0 += WL_THREADS) {          // segments owned by this thread in this pass: s0 + tid
    const int s = s0 + tid;
    const int my = s < nseg ? wl_len(cu, s) : -1;
    int rank = 0;
    for (int j0 = 0; j0 < nseg; j0 += WL_TILE) {
      __syncthreads();
      for (int j = tid; j < WL_TILE && j0 + j < nseg; j += WL_THREADS) lens[j] = wl_len(cu, j0 + j);
      __syncthreads();
      const int nj = nseg - j0 < WL_TILE ? nseg - j0 : WL_TILE;
      if (s < nseg)
        for (int j = 0; j < nj; ++j) rank += (lens[j] > my || (lens[j] == my && j0 + j < s)) ? 1 : 0;
    }
    if (s < nseg) order[rank] = s;
  }
  __threadfence_block();
  __syncthreads();
  // ---- exclusive scan of the item counts in rank order: thread t owns ranks [t * per, (t + 1) * per)
  const int per = (nseg + WL_THREADS - 1) / WL_THREADS;
  const int r0 = tid * per, r1 = (r0 + per) < nseg ? (r0 + per) : nseg;
  int sum = 0;
  for (int r = r0; r < r1; ++r) { const int sg = order[r]; sum += (wl_len(cu, sg) + bq - 1) / bq; }
  partial[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    int acc = 0;
    for (int t = 0; t < WL_THREADS; ++t) { const int v = partial[t]; partial[t] = acc; acc += v; }
    total_items = acc;
  }
  __syncthreads();
  // ---- emit
  int n = partial[tid];
  for (int r = r0; r < r1; ++r) {
    const int sg = order[r];
    const int a = cu[sg], len = wl_len(cu, sg);
    for (int q0 = 0; q0 < len; q0 += bq, ++n)
      if (n < max_items) { const AttnWorkItem w = {a, len, q0, 0}; items[n] = w; }
  }
  __syncthreads();                     // the padding below must not race with another thread's emit
  const int total = total_items < 0 ? 0 : total_items < max_items ? total_items : max_items;
  for (int i = total + tid; i < max_items; i += WL_THREADS) items[i] = none;
}

// One schedule ships: 4 waves x 64 queries per block (136 -> 142 TF at the C1 shapes).  The 8-wave / 512-query form (134 TF) and
// the software-pipelined v3 kernel (124 TF) of round 1 are in the history at 72efb73 (profiles/r01_run3_kernel_variant_sweep.jsonl).
rap_tuning_t g_rap_attn_variant = 1;   // kept for the ablation build's rap_set_tuning(1, .): only 1 exists
rap_tuning_t g_rap_attn_split = 1;     // tuning key 5: 0 = never split few-token calls over key ranges
static int attn_block_queries() { return RAP_ATTN_BQ; }

int launch_build_attn_worklist(hipStream_t stream, const int32_t* cu_seqlens, int nseg, AttnWorkItem* items,
                               int max_items, int block_queries, int32_t* sort_ws) {
  if (max_items <= 0) return RAP_OK;
  hipLaunchKernelGGL(build_attn_worklist_kernel, dim3(1), dim3(WL_THREADS), 0, stream, cu_seqlens, nseg, items, max_items,
                     block_queries > 0 ? block_queries : attn_block_queries(), sort_ws);
  RAP_LAUNCH_CHECK();
  return RAP_OK;
}

// out[t][c] = sum_s part_o[s][t][c] / sum_s part_l[s][t][head(c)]   (one thread per 4 columns)
__global__ __launch_bounds__(256) void attention_combine_kernel(const float* __restrict__ part_o, const float* __restrict__ part_l,
                                                                float* __restrict__ out, int TP, int heads, int splits,
                                                                const int32_t* __restrict__ cover_cu, int cover_nseg) {
  const int dmodel = heads * 64;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;           // float4 index
  if (i >= (long)TP * dmodel / 4) return;
  const long t = i / (dmodel / 4);
  const int c = (int)(i % (dmodel / 4)) * 4;
  if (cover_cu && (t < cover_cu[0] || t >= cover_cu[cover_nseg])) {      // no block wrote partials for this row (filler rows, rows outside every segment)
    *reinterpret_cast<float4*>(out + t * dmodel + c) = float4{0.f, 0.f, 0.f, 0.f};
    return;
  }
  float4 acc = {0.f, 0.f, 0.f, 0.f};
  float l = 0.f;
  for (int s = 0; s < splits; ++s) {
    const float4 v = *reinterpret_cast<const float4*>(part_o + ((size_t)s * TP + t) * dmodel + c);
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    l += part_l[((size_t)s * TP + t) * heads + (c >> 6)];
  }
  // l = NaN: a range of the main kernel refused this head (bound above 40) -- the refusal must reach out as NaN, not as zeros (l = 0,
  // a row no key contributed to, keeps its zeros)
  const float inv = (l > 0.f || l != l) ? 1.0f / l : 0.f;
  acc.x *= inv; acc.y *= inv; acc.z *= inv; acc.w *= inv;
  *reinterpret_cast<float4*>(out + t * dmodel + c) = acc;
}

// How many key ranges a few-token call is split into (1 = no split): only the bounded (offset-free) kernel can add partial
// results, and only work lists that leave most of the 2 x 256 block slots empty are worth the extra pass.
int attention_f32_splits(int max_items, int heads, bool bounded) {
  if (!bounded || g_rap_attn_split == 0) return 1;
  const long blocks = (long)max_items * heads;
  return blocks <= 160 ? 4 : blocks <= 320 ? 2 : 1;
}
// ... and whether the split launch asks for one block per CU (launch_attention_f32: the grid holds at most ~1.5 blocks per CU)
bool attention_f32_one_per_cu(int max_items, int heads, int splits) { return splits > 1 && (long)max_items * heads * splits <= 384; }

int launch_attention_f32(hipStream_t stream, const float* qkv, float* out, int TP, int heads, const AttnWorkItem* items,
                         int max_items, const float* bound, float* part_o, float* part_l, int splits, const int32_t* cover_cu,
                         int cover_nseg) {
  if (max_items <= 0 || TP <= 0) return RAP_OK;
  if (heads <= 0) return RAP_ERR_INVALID;
  if (splits > 1) {
    if (!bound || !part_o || !part_l) return RAP_ERR_INVALID;
    // At most ~one block per CU in the grid (one pair of 2 x 1024 points: 8 work items x 8 heads x 4 key ranges = 256 blocks): ask for
    // 16 KB of (unused) dynamic LDS on top of the 68 KB of tiles, so that only ONE block fits a CU.  Left to itself the dispatcher
    // doubles blocks up on some CUs while others stay empty, and two 4-wave blocks on one CU share its four matrix pipes: 102 -> 72 us
    // per launch, 62.5 -> 55.3 ms per fp32 call at that size (r03 call 36; the same trick changes nothing for the 16-bit attention
    // and GEMM launches of such a call).
    unsigned dyn = 0;
    if (attention_f32_one_per_cu(max_items, heads, splits)) {
      dyn = 16384;
      if (int rc = rap_allow_dyn_lds(attention_f32_kernel<4, true, true>, dyn)) return rc;
    }
    hipLaunchKernelGGL((attention_f32_kernel<4, true, true>), dim3(max_items * heads, splits), dim3(256), dyn, stream, qkv, out, TP,
                       heads, items, bound, part_o, part_l);
    RAP_LAUNCH_CHECK();
    const long n4 = (long)TP * heads * 16;
    hipLaunchKernelGGL(attention_combine_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream, part_o, part_l, out, TP,
                       heads, splits, cover_cu, cover_nseg);
    RAP_LAUNCH_CHECK();
    return RAP_OK;
  }
  float* const no = nullptr;
  if (bound) hipLaunchKernelGGL((attention_f32_kernel<4, true>), dim3(max_items * heads), dim3(256), 0, stream, qkv, out, TP, heads, items, bound, no, no);
  else hipLaunchKernelGGL((attention_f32_kernel<4, false>), dim3(max_items * heads), dim3(256), 0, stream, qkv, out, TP, heads, items, bound, no, no);
  RAP_LAUNCH_CHECK();
  return RAP_OK;
}

// the soft-capped online softmax (softcap > 0, finite: the entry points check): one form, 4 waves x 64 queries, never split
int launch_attention_f32_softcap(hipStream_t stream, const float* qkv, float* out, int TP, int heads, const AttnWorkItem* items,
                                 int max_items, float softcap) {
  if (max_items <= 0 || TP <= 0) return RAP_OK;
  if (heads <= 0 || !softcap_ok(softcap)) return RAP_ERR_INVALID;
  hipLaunchKernelGGL((attention_f32_softcap_kernel<4>), dim3(max_items * heads), dim3(256), 0, stream, qkv, out, TP, heads, items, softcap);
  RAP_LAUNCH_CHECK();
  return RAP_OK;
}
