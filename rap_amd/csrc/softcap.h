// Soft-capped attention logits (flash-attn's `softcap`): s <- c * tanh(s / c) in front of the softmax, shared by the capped
// instantiations of the three attention kernels (attn_f32.hip, attn_h16.hip, attn_x2.hip).
#pragma once
#include "common.h"

// host: the caps the entry points and the launchers accept -- positive and finite (NaN fails both comparisons)
static inline bool softcap_ok(float c) { return c > 0.f && c < 3.0e38f; }

// K * tanh(x) in fp32 on v_exp_f32 / v_rcp_f32, no library call; m2K = -2 K (wave-uniform, formed once per kernel).
//  * |x| >= 1/4:  K (1 - 2 / (1 + e^2x)) as ONE fma on the reciprocal.  The ends are clean: e^2x = +inf gives rcp = 0 and the result K,
//    e^2x = 0 gives rcp(1) = 1 and the result -K, both exactly; no intermediate is NaN for any finite x.  Error: about an ulp of 1
//    absolute, i.e. <= 4 ulp of tanh(x) >= 0.245.
//  * |x| < 1/4:   that form loses RELATIVE accuracy (1 - 2 / (1 + e^2x) cancels; the logit K tanh(x) would be off by K * 1e-7 whatever
//    its size -- 5e-6 at c = 50, the whole tolerance of the fp32 attention tests), so the odd Taylor polynomial through x^9 takes over:
//    truncation 1382/155925 x^10 <= 8.5e-9 relative at the seam, below half an fp32 ulp.
// Both are evaluated and selected per lane (no divergence): 2 transcendentals + 12 VALU per score.
__device__ __forceinline__ float softcap_ktanh(float x, float K, float m2K) {
  const float e = __builtin_amdgcn_exp2f(x * 2.88539008177792681472f);      // e^(2x)
  const float r = __builtin_amdgcn_rcpf(1.0f + e);
  const float big = fmaf(r, m2K, K);
  const float x2 = x * x;
  float p = fmaf(x2, 2.18694885361552028e-2f, -5.39682539682539683e-2f);   // 62/2835, -17/315
  p = fmaf(x2, p, 1.33333333333333333e-1f);                                 // 2/15
  p = fmaf(x2, p, -3.33333333333333333e-1f);
  p = fmaf(x2, p, 1.0f);
  const float small = (K * x) * p;
  return fabsf(x) < 0.25f ? small : big;
}
