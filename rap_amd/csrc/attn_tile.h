// What the three attention kernels (attn_f32.hip, attn_h16.hip, attn_x2.hip) share: the lane helpers, the deferred-rescale threshold and
// the per-tile softmax steps of the 16-bit and split-precision kernels.
//
// The tile steps are TEXT -- function-like macros that name everything they touch -- and the kernel bodies are included files
// (*_body.inc), not __device__ __forceinline__ functions: hipcc allocates registers and orders commutative operands differently for an
// inlined body (the mask + softmax + exponent step as one function moved the register allocation of all 24 kernels of attn_h16.hip), and
// every shipped kernel keeps its device code instruction for instruction across such a fold (scripts/kernel_asm_diff.py).
//
// Tile shape of the steps: s0 / s1 = the S^T accumulators (f32x16) of the two 32-key sub-tiles of one 64-key tile, o0 / o1 = the O^T
// accumulators, a lane owns one query column; mrun / lsum = its running reference and row sum, c = log2(e) / 8.  OPT: attn_h16.hip.
// The fp32 kernel has another tile shape (st[qt][r], 64 queries per wave, pre-scaled q) and takes the helpers and the threshold only.
#pragma once
#include "softcap.h"

__device__ __forceinline__ float attn_xhalf_max(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float attn_xhalf_sum(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float attn_max3(float a, float b, float c) {
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
// Deferred rescale of the online softmax, in the base-2 exponent (= 8 in natural-log units): the running reference m of a row moves only
// when a row of the wave outgrows it by more than this, so p = 2^(s - m) <= 2^11.5 = e^8 -- no overflow in bf16 / fp16 / the fp32 sums --
// and in the steady state a tile costs no alpha, no rescale of O and no l * alpha.  Softmax is invariant to the reference.
#define ATTN_DEFER_THR 11.5f

// ---- soft cap, in front of the key mask (tanh(-1e30) would un-mask a key): the fp32 scores q.k become 8 cap * tanh(q.k / (8 cap)), so
// that the exponent's FMA (x log2(e) / 8) sees cap * tanh(s / cap) of the logit s = q.k / 8
#define ATTN_SOFTCAP(s0, s1, cap)                                                                    \
  {                                                                                                  \
    const float inv_ = 0.125f / (cap), capK_ = 8.0f * (cap), capM2K_ = -16.0f * (cap);                \
    _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_) {                                              \
      s0[r_] = softcap_ktanh(s0[r_] * inv_, capK_, capM2K_);                                         \
      s1[r_] = softcap_ktanh(s1[r_] * inv_, capK_, capM2K_);                                         \
    }                                                                                                \
  }

// ---- mask the keys outside the segment [seg0, seg1) (first / last tile only); tile0 = global index of the tile's first key
#define ATTN_MASK_KEYS(s0, s1, tile0, seg0, seg1, hi)                                                \
  {                                                                                                  \
    const int tile0_ = (tile0);                                                                      \
    if (tile0_ < (seg0) || tile0_ + 64 > (seg1)) {                                                   \
      _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_) {                                            \
        const int kg_ = tile0_ + mfma32_crow(r_, hi);                                                \
        s0[r_] = (kg_ >= (seg0) && kg_ < (seg1)) ? s0[r_] : -1e30f;                                  \
        s1[r_] = (kg_ + 32 >= (seg0) && kg_ + 32 < (seg1)) ? s1[r_] : -1e30f;                        \
      }                                                                                              \
    }                                                                                                \
  }

// ---- online softmax (not OPT bit 3), lane-local except one cross-half max: the row maximum (OPT bit 0: two independent v_max3_f32
// chains) and the rescale of O and l -- deferred (OPT bit 1) while no row of the wave grew by more than ATTN_DEFER_THR.  Textbook order:
// the decision precedes this tile's exponentials and follows the previous tile's P*V.
#define ATTN_ONLINE_RESCALE(OPT, s0, s1, o0, o1, mrun, lsum, c)                                      \
  if (!((OPT) & 8)) {                                                                                \
    float mx_;                                                                                       \
    if ((OPT) & 1) {                                                                                 \
      float ma_ = attn_max3(s0[0], s0[1], s0[2]), mb_ = attn_max3(s1[0], s1[1], s1[2]);              \
      _Pragma("unroll") for (int r_ = 3; r_ < 15; r_ += 2) {                                         \
        ma_ = attn_max3(ma_, s0[r_], s0[r_ + 1]);                                                    \
        mb_ = attn_max3(mb_, s1[r_], s1[r_ + 1]);                                                    \
      }                                                                                              \
      mx_ = attn_max3(ma_, mb_, fmaxf(s0[15], s1[15]));                                              \
    } else {                                                                                         \
      mx_ = fmaxf(s0[0], s1[0]);                                                                     \
      _Pragma("unroll") for (int r_ = 1; r_ < 16; ++r_) mx_ = fmaxf(mx_, fmaxf(s0[r_], s1[r_]));     \
    }                                                                                                \
    mx_ = attn_xhalf_max(mx_);                                                                       \
    if (!((OPT) & 2) || !__all((mx_ - mrun) * (c) <= ATTN_DEFER_THR)) {                              \
      const float mnew_ = fmaxf(mrun, mx_);                                                          \
      const float alpha_ = __builtin_amdgcn_exp2f((mrun - mnew_) * (c));                             \
      mrun = mnew_;                                                                                  \
      lsum *= alpha_;                                                                                \
      _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_) { o0[r_] *= alpha_; o1[r_] *= alpha_; }      \
    }                                                                                                \
  }

// ---- p = exp2(s c - mrun c) in place (OPT bit 4: the score IS the exp2 argument) and the row sum, on the packed fp32 pipe
// (v_pk_fma_f32 / v_pk_add_f32: two lanes' worth per issue slot)
#define ATTN_EXP_ROWSUM(OPT, s0, s1, mrun, lsum, c)                                                  \
  {                                                                                                  \
    const f32x2 c2_ = {(c), (c)};                                                                    \
    const f32x2 nmc2_ = {-mrun * (c), -mrun * (c)};                                                  \
    f32x2 ps2_ = {0.f, 0.f};                                                                         \
    _Pragma("unroll") for (int k_ = 0; k_ < 8; ++k_) {                                               \
      f32x2 a_ = {s0[2 * k_], s0[2 * k_ + 1]};                                                       \
      f32x2 b_ = {s1[2 * k_], s1[2 * k_ + 1]};                                                       \
      if (!((OPT) & 16)) {                                                                           \
        a_ = __builtin_elementwise_fma(a_, c2_, nmc2_);                                              \
        b_ = __builtin_elementwise_fma(b_, c2_, nmc2_);                                              \
      }                                                                                              \
      a_.x = __builtin_amdgcn_exp2f(a_.x); a_.y = __builtin_amdgcn_exp2f(a_.y);                      \
      b_.x = __builtin_amdgcn_exp2f(b_.x); b_.y = __builtin_amdgcn_exp2f(b_.y);                      \
      s0[2 * k_] = a_.x; s0[2 * k_ + 1] = a_.y;                                                      \
      s1[2 * k_] = b_.x; s1[2 * k_ + 1] = b_.y;                                                      \
      ps2_ += a_ + b_;                                                                               \
    }                                                                                                \
    lsum += ps2_.x + ps2_.y;                                                                         \
  }
