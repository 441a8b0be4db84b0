// Epilogues of the 16-bit and split-precision GEMM kernels of gemm_h16.hip (its only user): a wave's TM x 2 accumulator tiles -> global
// memory, and H16_EPILOGUE, the one place that chooses among them.
#pragma once
#include "half.h"
#include "kernels.h"

// exact-erf GELU through the Abramowitz-Stegun 7.1.26 complementary error function (|error| <= 1.5e-7, far below
// one rounding of the 16-bit output): q = erfc(|g| / sqrt 2);  gelu(g) = g < 0 ? g q / 2 : g (1 - q / 2).
// ~15 VALU instructions instead of erff's ~45 -- at 16x the fp32 MFMA rate the GEGLU epilogue was as long as the k-loop.
__device__ __forceinline__ float gelu_erf_fast(float g) {
  const float x = fabsf(g) * 0.70710678118654752440f;
  const float t = __builtin_amdgcn_rcpf(__builtin_fmaf(0.3275911f, x, 1.0f));
  float poly = __builtin_fmaf(t, 1.061405429f, -1.453152027f);
  poly = __builtin_fmaf(t, poly, 1.421413741f);
  poly = __builtin_fmaf(t, poly, -0.284496736f);
  poly = __builtin_fmaf(t, poly, 0.254829592f);
  poly *= t;
  const float q = poly * __builtin_amdgcn_exp2f(-x * x * 1.44269504088896340736f);
  return g < 0.f ? 0.5f * g * q : g * (1.0f - 0.5f * q);
}

// Two GEGLU outputs per call on the packed fp32 pipe (r02): the epilogue is VALU-bound -- r01's ablation prices it at 0.42 ms of the
// 1.6 ms ff1 GEMM, and the disassembly showed ~24 scalar VALU instructions per output (nothing packed).  Here every multiply / FMA of
// the polynomial handles two outputs (v_pk_mul_f32 / v_pk_fma_f32: twice the fp32 rate when no MFMA is in flight), the branch of
// gelu_erf_fast becomes Phi(g) = 1/2 + copysign(1/2 - q/2, g), and the two results leave as ONE v_cvt_pk: ~13 instructions per output.
// ---------------- epilogue (shared by the kernels below) ----------------
// acc[i][j][r] = C[mw + 32 i + crow(r, hi)][nw + 32 j + l31]: a lane owns ONE column, so direct stores would be
// 2- or 4-byte scatters (measured: the out-projection ran at 147 TF, 4x its HBM floor).  Every wave therefore
// transposes its tile through a private LDS slab `stg` (the operand buffers are dead by now; the caller has
// synchronised the block) and writes whole rows with 16-byte stores; the fp32 residual is read the same way.
#define H16_STG_BYTES (64 * 144)   // largest slab: the V^T image of 64 tokens (64 d rows of 144 bytes)
// RAP_MUTATION (scripts/mutation_check.sh only, never in the shipped library): a deliberately injected extra rounding to the OPERAND type
// in the residual epilogues -- 1: of the epilogue's result (the new residual-stream value), 2: of the GEMM output before the residual is
// added -- to show that the tightened 16-bit deviation bounds of the test-suite notice a precision regression.
#ifdef RAP_MUTATION
template <int DT> __device__ __forceinline__ float rap_mut_round(float x) { return h16_to_f32<DT>(h16_from_f32<DT>(x)); }
#define RAP_MUT_OUT(DT, x) (RAP_MUTATION == 2 ? rap_mut_round<DT>(x) : (x))
#define RAP_MUT_SUM(DT, x) (RAP_MUTATION == 1 ? rap_mut_round<DT>(x) : (x))
#else
#define RAP_MUT_OUT(DT, x) (x)
#define RAP_MUT_SUM(DT, x) (x)
#endif
template <int EPI, int DT, int TM>
__device__ __forceinline__ void gemm_h16_epilogue(const GemmParamsH& p, f32x16 (&acc)[TM][2], unsigned char* stg, int mw, int nw,
                                                  int lane) {
  const int hi = lane >> 5, l31 = lane & 31;
  if constexpr (EPI == EPI_H_GEGLU) {
    u16* C = reinterpret_cast<u16*>(p.C);
    u16* sh = reinterpret_cast<u16*>(stg);       // [32 rows][32 outputs]
    const float bh = p.bias ? p.bias[nw + l31] : 0.f;
    const float bg = p.bias ? p.bias[nw + 32 + l31] : 0.f;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      f32x2 h2[8], g2[8], o2[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        h2[j] = f32x2{acc[i][0][2 * j], acc[i][0][2 * j + 1]} + f32x2{bh, bh};
        g2[j] = f32x2{acc[i][1][2 * j], acc[i][1][2 * j + 1]} + f32x2{bg, bg};
      }
      geglu_pairs<8>(h2, g2, o2);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const unsigned pk = __builtin_bit_cast(unsigned, __builtin_convertvector(o2[j], typename H16<DT>::T2));   // one v_cvt_pk for both
        sh[mfma32_crow(2 * j, hi) * 32 + l31] = (u16)(pk & 0xffffu);
        sh[mfma32_crow(2 * j + 1, hi) * 32 + l31] = (u16)(pk >> 16);
      }
#pragma unroll
      for (int it = 0; it < 2; ++it) {
        const int row = it * 16 + (lane >> 2), col = (lane & 3) * 8;
        const uint4 v = *reinterpret_cast<const uint4*>(sh + row * 32 + col);
        const int m = mw + i * 32 + row;
        if (m < p.M) *reinterpret_cast<uint4*>(C + (size_t)m * p.ldc + (nw >> 1) + col) = v;
      }
    }
    return;
  }
  if constexpr (EPI == EPI_H_BIAS_RESID_F32) {
    // (r02 call 39: requesting the residual rows of slab i + 1 while slab i is transposed and stored -- rolling through one register
    // set, or two sets -- pushes this 225-VGPR kernel over 256 and spills in the epilogue: out-projection 0.32 -> 0.33 ms, ff2 unchanged.
    // Both GEMMs are bound by this fp32 read-modify-write of the residual stream, 1.34 / 2.4 GB per call at 4.2 / 3.8 TB/s.)
    float* C = reinterpret_cast<float*>(p.C);
    float* sf = reinterpret_cast<float*>(stg);   // [32 rows][64 columns]
    const float b0 = p.bias ? p.bias[nw + l31] : 0.f;
    const float b1 = p.bias ? p.bias[nw + 32 + l31] : 0.f;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      float4 rr[8];
      if (p.resid) {
#pragma unroll
        for (int it = 0; it < 8; ++it) {
          int m = mw + i * 32 + it * 4 + (lane >> 4);
          m = m < p.M ? m : p.M - 1;
          rr[it] = *reinterpret_cast<const float4*>(p.resid + (size_t)m * p.ldr + nw + (lane & 15) * 4);
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        sf[mfma32_crow(r, hi) * 64 + l31] = RAP_MUT_OUT(DT, acc[i][0][r] + b0);
        sf[mfma32_crow(r, hi) * 64 + 32 + l31] = RAP_MUT_OUT(DT, acc[i][1][r] + b1);
      }
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        const int row = it * 4 + (lane >> 4), col = (lane & 15) * 4;
        float4 v = *reinterpret_cast<const float4*>(sf + row * 64 + col);
        if (p.resid) { v.x += rr[it].x; v.y += rr[it].y; v.z += rr[it].z; v.w += rr[it].w; }
        v.x = RAP_MUT_SUM(DT, v.x); v.y = RAP_MUT_SUM(DT, v.y); v.z = RAP_MUT_SUM(DT, v.z); v.w = RAP_MUT_SUM(DT, v.w);
        const int m = mw + i * 32 + row;
        if (m < p.M) *reinterpret_cast<float4*>(C + (size_t)m * p.ldc + nw + col) = v;
      }
    }
    return;
  }
  if constexpr (EPI == EPI_H_BIAS_RESID_H16) {
    // The residual GEMMs of the 16-bit residual stream (round 3): C fp16 = fp16(resid_h + acc + bias), the sum formed in fp32 from the
    // fp32 accumulators and rounded ONCE.  Half the bytes of the fp32 read-modify-write that bounds EPI_H_BIAS_RESID_F32.  fp32
    // transposition slab as above; a lane then owns 8 consecutive columns of a row: two float4 from the slab, one 16-byte piece of the
    // fp16 residual in, one 16-byte piece out.  ALL residual pieces of the wave tile (TM x 4 x 16 bytes per lane = 64 VGPRs, the
    // registers the operand fragments occupied during the k-loop) are requested before the first slab is transposed, so the HBM
    // latency is paid once per tile, not once per 32-row slab (the fp32 form needs 128 registers for that and spilled, r02 call 39).
    u16* C = reinterpret_cast<u16*>(p.C);
    float* sf = reinterpret_cast<float*>(stg);   // [32 rows][68 floats]: 64 columns + 4 pad (the 8-lanes-per-row reads stay off each other's banks)
    const float b0 = p.bias ? p.bias[nw + l31] : 0.f;
    const float b1 = p.bias ? p.bias[nw + 32 + l31] : 0.f;
    // the (L2-hot) bias has landed before the residual requests go out: the slab writes below then wait for nothing, and every
    // residual piece is waited for with its own counted vmcnt
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int col = (lane & 7) * 8;
    uint4 rr[TM][4];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        int m = mw + i * 32 + it * 8 + (lane >> 3);
        m = m < p.M ? m : p.M - 1;
        rr[i][it] = *reinterpret_cast<const uint4*>(p.resid_h + (size_t)m * p.ldr + nw + col);
      }
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        sf[mfma32_crow(r, hi) * 68 + l31] = RAP_MUT_OUT(DT, acc[i][0][r] + b0);
        sf[mfma32_crow(r, hi) * 68 + 32 + l31] = RAP_MUT_OUT(DT, acc[i][1][r] + b1);
      }
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int row = it * 8 + (lane >> 3);
        const float4 a0 = *reinterpret_cast<const float4*>(sf + row * 68 + col);
        const float4 a1 = *reinterpret_cast<const float4*>(sf + row * 68 + col + 4);
        float rv[8];
        h16_unpack8<RAP_DT_F16>(rr[i][it], rv);
        const typename H16<RAP_DT_F16>::T8 o8 = f16_pack8_sat(RAP_MUT_SUM(DT, a0.x + rv[0]), RAP_MUT_SUM(DT, a0.y + rv[1]), RAP_MUT_SUM(DT, a0.z + rv[2]),
                                                             RAP_MUT_SUM(DT, a0.w + rv[3]), RAP_MUT_SUM(DT, a1.x + rv[4]), RAP_MUT_SUM(DT, a1.y + rv[5]),
                                                             RAP_MUT_SUM(DT, a1.z + rv[6]), RAP_MUT_SUM(DT, a1.w + rv[7]));
        const int m = mw + i * 32 + row;
        if (m < p.M) *reinterpret_cast<uint4*>(C + (size_t)m * p.ldc + nw + col) = __builtin_bit_cast(uint4, o8);
      }
    }
    return;
  }
  if constexpr (EPI == EPI_H_BIAS || EPI == EPI_H_QKV) {
    u16* sh = reinterpret_cast<u16*>(stg);
    int c = 0, h = 0;
    if constexpr (EPI == EPI_H_QKV) {
      const int dmodel = p.heads * 64;
      c = nw / dmodel;                             // wave-uniform: the 64-column wave tile is one head of q, k or v
      h = (nw - c * dmodel) >> 6;
    }
    if (EPI == EPI_H_QKV && c == 2) {
      // V goes out TRANSPOSED and blocked by 64 tokens: vt[h][token >> 6][d][vt_pos(token & 63)].  Two 32-token slabs
      // (= one block) are staged as [64 d][64 pos] (row stride 144 B) and written as one contiguous 8 KiB block.
      // Rows >= M (tile padding) are zeros: masked keys must contribute 0 * finite in the P*V product.
#pragma unroll
      for (int ip = 0; ip < TM / 2; ++ip) {
#pragma unroll
        for (int ii = 0; ii < 2; ++ii) {
#pragma unroll
          for (int j = 0; j < 2; ++j) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              const int i = 2 * ip + ii;
              const int mb = mw + i * 32 + 8 * g + 4 * hi;          // first of 4 consecutive tokens
              float v0 = acc[i][j][4 * g + 0], v1 = acc[i][j][4 * g + 1], v2 = acc[i][j][4 * g + 2], v3 = acc[i][j][4 * g + 3];
              v0 = (mb + 0 < p.M) ? v0 : 0.f; v1 = (mb + 1 < p.M) ? v1 : 0.f;
              v2 = (mb + 2 < p.M) ? v2 : 0.f; v3 = (mb + 3 < p.M) ? v3 : 0.f;
              const int pos0 = 32 * ii + 16 * (g >> 1) + 8 * hi + 4 * (g & 1);   // = vt_pos(32 ii + 8 g + 4 hi)
              *reinterpret_cast<uint2*>(sh + (j * 32 + l31) * 72 + pos0) = h16_pack4<DT>(v0, v1, v2, v3);
            }
          }
        }
        u16* dst = p.vt + ((size_t)h * p.vt_nblk + ((mw + 64 * ip) >> 6)) * (64 * 64);
#pragma unroll
        for (int it = 0; it < 8; ++it) {
          const int d = it * 8 + (lane >> 3), ch = (lane & 7) * 8;
          *reinterpret_cast<uint4*>(dst + d * 64 + ch) = *reinterpret_cast<const uint4*>(sh + d * 72 + ch);
        }
      }
      return;
    }
    const float b0 = (EPI == EPI_H_BIAS && p.bias) ? p.bias[nw + l31] : 0.f;
    const float b1 = (EPI == EPI_H_BIAS && p.bias) ? p.bias[nw + 32 + l31] : 0.f;
    u16* C = reinterpret_cast<u16*>(p.C);
    // q / k plane [c][h][m][64]: the wave's rows are contiguous 128-byte lines; EPI_H_BIAS: row-major (M, ldc)
    const size_t row_stride = (EPI == EPI_H_QKV) ? 64 : (size_t)p.ldc;
    u16* base = (EPI == EPI_H_QKV) ? C + ((size_t)(c * p.heads + h) * p.M) * 64 : C + nw;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        sh[mfma32_crow(r, hi) * 64 + l31] = h16_from_f32<DT>(acc[i][0][r] + b0);
        sh[mfma32_crow(r, hi) * 64 + 32 + l31] = h16_from_f32<DT>(acc[i][1][r] + b1);
      }
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int row = it * 8 + (lane >> 3), col = (lane & 7) * 8;
        const uint4 v = *reinterpret_cast<const uint4*>(sh + row * 64 + col);
        const int m = mw + i * 32 + row;
        if (m < p.M) *reinterpret_cast<uint4*>(base + (size_t)m * row_stride + col) = v;
      }
    }
  }
}

// ---------------- fused q / k epilogue of EPI_H_QKV_NORM (swapped product) ----------------
// acc[i][j][r] = C[mw + 32 i + l31][nw + 32 j + crow(r, hi)]: the lane owns token row mw + 32 i + l31 and, of the head's 64 columns,
// those with bit 2 equal to hi.  MultiHeadRMSNorm (flow_model/norm.py:28-33: F.normalize(x, dim=-1) * gamma * sqrt(64)) needs the
// row's sum of squares: 32 lane-local terms + the partner lane's (lane ^ 32, one v_permlane32_swap).  q additionally carries
// q_mul / 8 (the attention kernel's pre-scaled form, see launch_qknorm_h16).  Output plane [c][h][m][64]: register groups 2t and
// 2t+1 of the two half-waves are exchanged (v_permlane32_swap) so that a lane holds 8 CONSECUTIVE columns = one 16-byte store;
// the four stores of a row tile cover whole 128-byte rows -- no LDS transpose.
template <int DT, int TM>
__device__ __forceinline__ void gemm_h16_qknorm_epilogue(const GemmParamsH& p, f32x16 (&acc)[TM][2], int mw, int nw, int lane) {
  const int hi = lane >> 5, l31 = lane & 31;
  const int dmodel = p.heads * 64;
  const int c = nw / dmodel;                      // 0 = q, 1 = k (wave-uniform)
  const int h = (nw - c * dmodel) >> 6;
  const float* gam = (c == 0 ? p.gamma_q : p.gamma_k) + h * 64;
  const float mul = c == 0 ? p.q_mul : 8.0f;
  float g[2][16];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) g[j][r] = gam[32 * j + mfma32_crow(r, hi)] * mul;
  u16* plane = reinterpret_cast<u16*>(p.C) + ((size_t)(c * p.heads + h) * p.M) * 64;
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) ss = __builtin_fmaf(acc[i][j][r], acc[i][j][r], ss);
    {
      const auto sw2 = __builtin_amdgcn_permlane32_swap(__float_as_uint(ss), __float_as_uint(ss), false, false);
      ss = __uint_as_float(sw2[0]) + __uint_as_float(sw2[1]);
    }
    const float inv = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
    const int m = mw + 32 * i + l31;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        float x[4], y[4];                          // groups 2t and 2t+1: columns 16t + 4hi + {0..3} and 16t + 8 + 4hi + {0..3}
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float vx = acc[i][j][8 * t + e] * inv * g[j][8 * t + e];
          const float vy = acc[i][j][8 * t + 4 + e] * inv * g[j][8 * t + 4 + e];
          const auto s2 = __builtin_amdgcn_permlane32_swap(__float_as_uint(vx), __float_as_uint(vy), false, false);
          x[e] = __uint_as_float(s2[0]); y[e] = __uint_as_float(s2[1]);
        }
        // hi = 0: x = own group 2t (cols 16t + 0..3), y = partner's group 2t (cols 16t + 4..7)      -> columns 16t + 0..7
        // hi = 1: x = partner's group 2t+1 (cols 16t + 8..11), y = own group 2t+1 (cols 16t + 12..15) -> columns 16t + 8..15
        const typename H16<DT>::T8 o8 = h16_pack8<DT>(x[0], x[1], x[2], x[3], y[0], y[1], y[2], y[3]);
        if (m < p.M) *reinterpret_cast<uint4*>(plane + (size_t)m * 64 + 32 * j + 16 * t + 8 * hi) = __builtin_bit_cast(uint4, o8);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Split-precision epilogues (RAP_DT_F32X2, round 5; half.h).  The accumulators hold acc_scale^-1 times the fp32-accurate product
// (weights are stored pre-multiplied by a power of two, see rap_model_set_compute_dtype); 16-bit outputs leave as fp16 head / tail
// planes in the paired layout: the 64 physical columns of a wave tile's line are [32 heads | 32 tails] of ONE 32-column chunk.
// Same transposition slabs as above (<= H16_STG_BYTES per wave).
//   EPI_H_BIAS_RESID_F32: C fp32 (M,N) = resid + acc * scale + bias                       (out-projection, ff2)
//   EPI_H_GEGLU:          C paired (M, 2 * N/2) = split((h + bh) * gelu_erf(g + bg))      (ff1; wave tile = 32 outputs = one chunk)
//   EPI_H_QKV (c == 2):   vt paired [H][blk][2 chunks][64 d][32 heads | 32 tails] in vt_pos order (chunk = bit 5 of the token index)
// ---------------------------------------------------------------------------------------------
template <int EPI, int TM>
__device__ __forceinline__ void gemm_x2_epilogue(const GemmParamsH& p, f32x16 (&acc)[TM][2], unsigned char* stg, int mw, int nw, int lane) {
  const int hi = lane >> 5, l31 = lane & 31;
  const float sc = p.acc_scale;
  if constexpr (EPI == EPI_H_GEGLU) {
    u16* C = reinterpret_cast<u16*>(p.C);
    u16* sh = reinterpret_cast<u16*>(stg);       // [32 rows][72]: heads in columns 0..31, tails in 32..63
    const float bh = p.bias ? p.bias[nw + l31] : 0.f;
    const float bg = p.bias ? p.bias[nw + 32 + l31] : 0.f;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      f32x2 h2[8], g2[8], o2[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        h2[j] = __builtin_elementwise_fma(f32x2{acc[i][0][2 * j], acc[i][0][2 * j + 1]}, f32x2{sc, sc}, f32x2{bh, bh});
        g2[j] = __builtin_elementwise_fma(f32x2{acc[i][1][2 * j], acc[i][1][2 * j + 1]}, f32x2{sc, sc}, f32x2{bg, bg});
      }
      geglu_pairs<8>(h2, g2, o2);
      const float osc = p.out_scale;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const f32x2 s2 = {f16_sat(o2[j].x * osc), f16_sat(o2[j].y * osc)};
        const typename H16<RAP_DT_F16>::T2 h16 = __builtin_convertvector(s2, typename H16<RAP_DT_F16>::T2);
        const typename H16<RAP_DT_F16>::T2 l16 = __builtin_convertvector(s2 - __builtin_convertvector(h16, f32x2), typename H16<RAP_DT_F16>::T2);
        const unsigned ph = __builtin_bit_cast(unsigned, h16), pl = __builtin_bit_cast(unsigned, l16);
        sh[mfma32_crow(2 * j, hi) * 72 + l31] = (u16)(ph & 0xffffu);
        sh[mfma32_crow(2 * j + 1, hi) * 72 + l31] = (u16)(ph >> 16);
        sh[mfma32_crow(2 * j, hi) * 72 + 32 + l31] = (u16)(pl & 0xffffu);
        sh[mfma32_crow(2 * j + 1, hi) * 72 + 32 + l31] = (u16)(pl >> 16);
      }
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int row = it * 8 + (lane >> 3), col = (lane & 7) * 8;
        const uint4 v = *reinterpret_cast<const uint4*>(sh + row * 72 + col);
        const int m = mw + i * 32 + row;
        if (m < p.M) *reinterpret_cast<uint4*>(C + (size_t)m * p.ldc + nw + col) = v;     // physical columns of chunk nw >> 6: [nw, nw + 64)
      }
    }
    return;
  }
  if constexpr (EPI == EPI_H_BIAS_RESID_F32) {
    float* C = reinterpret_cast<float*>(p.C);
    float* sf = reinterpret_cast<float*>(stg);   // [32 rows][64 columns]
    const float b0 = p.bias ? p.bias[nw + l31] : 0.f;
    const float b1 = p.bias ? p.bias[nw + 32 + l31] : 0.f;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      float4 rr[8];
      if (p.resid) {
#pragma unroll
        for (int it = 0; it < 8; ++it) {
          int m = mw + i * 32 + it * 4 + (lane >> 4);
          m = m < p.M ? m : p.M - 1;
          rr[it] = *reinterpret_cast<const float4*>(p.resid + (size_t)m * p.ldr + nw + (lane & 15) * 4);
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        sf[mfma32_crow(r, hi) * 64 + l31] = __builtin_fmaf(acc[i][0][r], sc, b0);
        sf[mfma32_crow(r, hi) * 64 + 32 + l31] = __builtin_fmaf(acc[i][1][r], sc, b1);
      }
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        const int row = it * 4 + (lane >> 4), col = (lane & 15) * 4;
        float4 v = *reinterpret_cast<const float4*>(sf + row * 64 + col);
        if (p.resid) { v.x += rr[it].x; v.y += rr[it].y; v.z += rr[it].z; v.w += rr[it].w; }
        const int m = mw + i * 32 + row;
        if (m < p.M) *reinterpret_cast<float4*>(C + (size_t)m * p.ldc + nw + col) = v;
      }
    }
    return;
  }
  if constexpr (EPI == EPI_H_QKV) {
    // the V column tiles of the fused QKV projection (normal product: a lane owns a column d and 16 of every 32 tokens)
    u16* sh = reinterpret_cast<u16*>(stg);       // [64 d][72]: one chunk (32 tokens) of one 64-token block: 32 heads | 32 tails
    const int dmodel = p.heads * 64;
    const int h = (nw - 2 * dmodel) >> 6;
    const float sc = p.acc_scale * p.out_scale;  // (shadows the function-level scale: the V planes carry out_scale, see GemmParamsH)
#pragma unroll
    for (int ip = 0; ip < TM / 2; ++ip) {
#pragma unroll
      for (int ii = 0; ii < 2; ++ii) {
        const int i = 2 * ip + ii;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int mb = mw + i * 32 + 8 * g + 4 * hi;          // first of 4 consecutive tokens
            float v0 = acc[i][j][4 * g + 0] * sc, v1 = acc[i][j][4 * g + 1] * sc, v2 = acc[i][j][4 * g + 2] * sc, v3 = acc[i][j][4 * g + 3] * sc;
            v0 = (mb + 0 < p.M) ? v0 : 0.f; v1 = (mb + 1 < p.M) ? v1 : 0.f;
            v2 = (mb + 2 < p.M) ? v2 : 0.f; v3 = (mb + 3 < p.M) ? v3 : 0.f;
            const int inpos = 16 * (g >> 1) + 8 * hi + 4 * (g & 1);   // = vt_pos(32 ii + 8 g + 4 hi) - 32 ii
            uint2 ph, pl;
            x2_split4(v0, v1, v2, v3, ph, pl);
            *reinterpret_cast<uint2*>(sh + (j * 32 + l31) * 72 + inpos) = ph;
            *reinterpret_cast<uint2*>(sh + (j * 32 + l31) * 72 + 32 + inpos) = pl;
          }
        }
        u16* dst = p.vt + (((size_t)h * p.vt_nblk + ((mw + 64 * ip) >> 6)) * 2 + ii) * (64 * 64);
#pragma unroll
        for (int it = 0; it < 8; ++it) {
          const int d = it * 8 + (lane >> 3), ch = (lane & 7) * 8;
          *reinterpret_cast<uint4*>(dst + d * 64 + ch) = *reinterpret_cast<const uint4*>(sh + d * 72 + ch);
        }
      }
    }
    return;
  }
}

// q / k column tiles of the fused QKV projection in split precision (swapped product, cf. gemm_h16_qknorm_epilogue): the row norm in
// fp32 from the (re-scaled) accumulators, then head / tail planes; plane [c][h][chunk][m][64 physical] (chunk = 32 head dims).
template <int TM>
__device__ __forceinline__ void gemm_x2_qknorm_epilogue(const GemmParamsH& p, f32x16 (&acc)[TM][2], int mw, int nw, int lane) {
  const int hi = lane >> 5, l31 = lane & 31;
  const int dmodel = p.heads * 64;
  const int c = nw / dmodel;                      // 0 = q, 1 = k (wave-uniform)
  const int h = (nw - c * dmodel) >> 6;
  const bool norm = p.gamma_q != nullptr;         // null gains (qk_norm = False, layer.py:103-104): q / k leave as projected
  const float* gam = norm ? (c == 0 ? p.gamma_q : p.gamma_k) + h * 64 : nullptr;
  const float mul = c == 0 ? p.q_mul : 8.0f;
  const float sc = p.acc_scale;
  float g[2][16];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) g[j][r] = norm ? gam[32 * j + mfma32_crow(r, hi)] * mul : 1.0f;
  u16* plane = reinterpret_cast<u16*>(p.C) + (((size_t)(c * p.heads + h) * 2) * p.M) * 64;
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) { acc[i][j][r] *= sc; ss = __builtin_fmaf(acc[i][j][r], acc[i][j][r], ss); }
    {
      const auto sw2 = __builtin_amdgcn_permlane32_swap(__float_as_uint(ss), __float_as_uint(ss), false, false);
      ss = __uint_as_float(sw2[0]) + __uint_as_float(sw2[1]);
    }
    const float inv = norm ? 1.0f / fmaxf(sqrtf(ss), 1e-12f) : 1.0f;
    const int m = mw + 32 * i + l31;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        float v8[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float vx = acc[i][j][8 * t + e] * inv * g[j][8 * t + e];
          const float vy = acc[i][j][8 * t + 4 + e] * inv * g[j][8 * t + 4 + e];
          const auto s2 = __builtin_amdgcn_permlane32_swap(__float_as_uint(vx), __float_as_uint(vy), false, false);
          v8[e] = __uint_as_float(s2[0]); v8[4 + e] = __uint_as_float(s2[1]);
        }
        x2_t8 h8, l8;
        x2_split8(v8, h8, l8);
        u16* dst = plane + ((size_t)j * p.M + m) * 64 + 16 * t + 8 * hi;      // chunk j of the head: dims 32 j + 16 t + 8 hi .. +7
        if (m < p.M) {
          *reinterpret_cast<uint4*>(dst) = __builtin_bit_cast(uint4, h8);
          *reinterpret_cast<uint4*>(dst + 32) = __builtin_bit_cast(uint4, l8);
        }
      }
    }
  }
}

// The epilogue of a wave tile at (MW, NW), chosen from the kernel's EPI, DT, TM, X2 and `swp` (EPI_H_QKV_NORM: true on the q / k column
// tiles, which ran the swapped product); `acc` and `lane` are the kernel's.  A macro on purpose: as a __forceinline__ function with
// these as parameters the choice perturbed register allocation and instruction order in 18 of the 66 kernels (one gained a VGPR).
#define H16_EPILOGUE(P, SLAB, MW, NW)                                                                         \
  if constexpr (X2) {                                                                                         \
    static_assert(!X2 || EPI == EPI_H_BIAS_RESID_F32 || EPI == EPI_H_GEGLU || EPI == EPI_H_QKV_NORM, "split precision: the three epilogues of the model path"); \
    if constexpr (EPI == EPI_H_QKV_NORM) {                                                                    \
      if (swp) gemm_x2_qknorm_epilogue<TM>(P, acc, MW, NW, lane);                                             \
      else gemm_x2_epilogue<EPI_H_QKV, TM>(P, acc, SLAB, MW, NW, lane);                                       \
    } else {                                                                                                  \
      gemm_x2_epilogue<EPI, TM>(P, acc, SLAB, MW, NW, lane);                                                  \
    }                                                                                                         \
  } else if constexpr (EPI == EPI_H_QKV_NORM) {                                                               \
    if (swp) gemm_h16_qknorm_epilogue<DT, TM>(P, acc, MW, NW, lane);                                          \
    else gemm_h16_epilogue<EPI_H_QKV, DT, TM>(P, acc, SLAB, MW, NW, lane);                                    \
  } else {                                                                                                    \
    gemm_h16_epilogue<EPI, DT, TM>(P, acc, SLAB, MW, NW, lane);                                               \
  }
