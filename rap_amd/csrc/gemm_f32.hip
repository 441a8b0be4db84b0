// fp32 GEMM on the CDNA4 matrix cores:  C (M,N) = A (M,K) * W (N,K)^T  + fused epilogue.
//
// Replaces the nn.Linear calls on the reference's velocity-network path
// (flow_model/layer.py:73-74,81-82,89 ; embedding.py:179 ; point_cloud_dit.py:111-117).
//
// Design (gfx950 only):
//  * v_mfma_f32_32x32x2_f32: exact fp32 (bitwise an fmaf chain), 64 cyc/SIMD, one VGPR per operand.
//  * Three kernels per epilogue, one tile step (GemmTile and the TG_* macros), one epilogue (gemm_f32_epilogue<EPI, TM>):
//      gemm_f32_tile_kernel<EPI, 2, 2, 2, 2>   128x128 block tile, 4 waves as 2x2, each wave 64x64 = 2x2 MFMA tiles; two blocks per CU
//      gemm_f32_tile_kernel<EPI, 2, 4, 4, 2>   256x256 block tile, 8 waves as 2x4, each wave 128x64 = 4x2 MFMA tiles; one block per CU
//      gemm_f32_persistent_kernel<EPI>         the 256x256 tile, one block per CU walking its share of the tiles
//    (gemm_f32_form below chooses; EPI_SPLITK_PART on the 128x128 kernel is the split-K partial product.)
//  * BK = 32: every A/W row contributes one full 128-byte line per k-tile.
//  * The contraction order inside a k-tile is permuted so that one ds_read_b128 feeds four MFMAs:
//    for k-group g (8 columns) lanes 0-31 read columns 8g..8g+3 and lanes 32-63 columns 8g+4..8g+7;
//    MFMA step s then contracts the column pair {8g+s, 8g+4+s}.  A sum is order independent up to
//    fp32 rounding, and the same permutation is applied to A and W.
//  * k-tiles go global -> LDS directly (global_load_lds_dwordx4, XOR slot swizzle instead of row padding), double-buffered
//    LDS, one barrier per k-tile.  (Rounds 1-2 also carried a register-staged v1 kernel and three software-pipelined
//    register-staged tilings, 12 points slower -- DESIGN.md 4.2; they are in the history at 72efb73.)
//  * 1-D grid, XCD-aware remap, n-tile fastest: all n-tiles of one 128-row A panel run back to
//    back on one XCD (A panel stays in that XCD's L2; W streams from L2 / Infinity Cache).
#include <type_traits>
#include "half.h"
#include "kernels.h"
#include "lds_dma.h"

#define GBM 128
#define GBN 128
#define GBK 32

// Fused MultiHeadRMSNorm for one 64-column wave tile (= one head of q or k) of the QKV projection: acc[mi][ni][r] is row
// m = mw + 32 mi + crow(r, hi), column 32 ni + l31.  The row norm is a sum over the 32 lanes of a half-wave and the two column
// tiles (5 xor-shuffles per row); the scaling repeats qknorm_kernel's operation order (x / nrm * gamma * 8), so the result differs
// from GEMM + qknorm only through the summation order of the 64 squares.
template <int TMI>
__device__ __forceinline__ void qkv_store_normalised(const GemmParams& p, f32x16 (&acc)[TMI][2], int mw, int nw, int hi, int l31) {
  const int dmodel = p.heads * 64;
  const int c = nw / dmodel;
  const int h = (nw - c * dmodel) >> 6;
  const float* gam = (c == 0 ? p.gamma_q : p.gamma_k) + h * 64;
  const float g0 = gam[l31], g1 = gam[32 + l31];
  float* plane = p.C + ((size_t)c * p.heads + h) * p.M * 64;
#pragma unroll
  for (int mi = 0; mi < TMI; ++mi) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float s = acc[mi][0][r] * acc[mi][0][r] + acc[mi][1][r] * acc[mi][1][r];
      // sum over the 32 lanes of the half-wave (= the 64 columns of the head): four DPP steps inside the VALU (quad xor 1, quad xor 2,
      // mirror within 8, mirror within 16 -- mirrored partners hold the same partial sums, so every lane ends with the total) and one
      // ds_swizzle across the two 16-lane rows, instead of five ds_bpermute round trips through the LDS queue (r02: 320 per wave tile)
      s += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s), 0xB1, 0xF, 0xF, true));
      s += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s), 0x4E, 0xF, 0xF, true));
      s += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s), 0x141, 0xF, 0xF, true));
      s += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s), 0x140, 0xF, 0xF, true));
      s += __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, s), 0x401F));
      const float nrm = fmaxf(sqrtf(s), 1e-12f);
      const int m = mw + mi * 32 + mfma32_crow(r, hi);
      if (m < p.M) {
        plane[(size_t)m * 64 + l31] = acc[mi][0][r] / nrm * g0 * 8.0f;
        plane[(size_t)m * 64 + 32 + l31] = acc[mi][1][r] / nrm * g1 * 8.0f;
      }
    }
  }
}

// The activations, written once: the tile epilogue, the erff GEGLU branch and the split-K combine pass share them.
#define TG_GELU_ERF(V) (0.5f * (V) * (1.0f + erff((V) * 0.70710678118654752440f)))
__device__ __forceinline__ float silu(float v) { return v / (1.0f + expf(-v)); }
__device__ __forceinline__ float gelu_erf(float v) { return TG_GELU_ERF(v); }

// Epilogue of one wave tile of TM x 2 MFMA tiles (rows mw .., columns nw .. nw + 63), straight from the accumulator registers.
template <int EPI, int TM>
__device__ __forceinline__ void gemm_f32_epilogue(const GemmParams& p, f32x16 (&acc)[TM][2], int mw, int nw, int hi, int l31) {
  constexpr int TN = 2;
  constexpr int RB = TM == 2 ? 2 : 1;              // row tiles whose residual loads are issued before the first use
  if (EPI == EPI_QKV_HEADMAJOR && p.gamma_q && nw < 2 * p.heads * 64) { qkv_store_normalised<TM>(p, acc, mw, nw, hi, l31); return; }
  if (EPI == EPI_GEGLU) {
    const int nout = (nw >> 1) + l31;
    const float bh = p.bias ? p.bias[nw + l31] : 0.f;
    const float bg = p.bias ? p.bias[nw + 32 + l31] : 0.f;
    if (p.geglu_fast) {                              // tuning key 9: packed-pair GEGLU (see half.h), stage-major over 8 pairs
#pragma unroll
      for (int mi = 0; mi < TM; ++mi) {
        f32x2 h2[8], g2[8], o2[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          h2[j] = f32x2{acc[mi][0][2 * j], acc[mi][0][2 * j + 1]} + f32x2{bh, bh};
          g2[j] = f32x2{acc[mi][1][2 * j], acc[mi][1][2 * j + 1]} + f32x2{bg, bg};
        }
        geglu_pairs<8>(h2, g2, o2);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int m = mw + mi * 32 + mfma32_crow(2 * j, hi);
          if (m < p.M) p.C[(size_t)m * p.ldc + nout] = o2[j].x;
          if (m + 1 < p.M) p.C[(size_t)(m + 1) * p.ldc + nout] = o2[j].y;
        }
      }
      return;
    }
    auto geglu = [&](auto G) {                       // G: guard rows against M (only the last row tile needs it)
#pragma unroll
      for (int mi = 0; mi < TM; ++mi) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = mw + mi * 32 + mfma32_crow(r, hi);
          if (decltype(G)::value && m >= p.M) continue;
          const float h = acc[mi][0][r] + bh;
          const float g = acc[mi][1][r] + bg;
          const float ge = TG_GELU_ERF(g);             // the macro: through gelu_erf() the persistent kernel schedules this loop differently
          p.C[(size_t)m * p.ldc + nout] = h * ge;
        }
      }
    };
    if (mw + 32 * TM <= p.M) geglu(std::false_type{}); else geglu(std::true_type{});
    return;
  }
  if (EPI == EPI_BIAS_RESID) {
    // r02: the residual rows are loaded UNCONDITIONALLY (row index clamped) and all loads of RB row tiles are issued before the
    // first use -- the per-register `if (m < M)` of the generic loop made hipcc emit load -> wait -> add -> store 64 times in a row
    // (64 exposed memory latencies per tile: the K = 512 shapes ran at 0.67-0.70 of the matrix peak against 0.84 at K = 2048).
    const bool full = mw + 32 * TM <= p.M;
#pragma unroll
    for (int mb = 0; mb < TM; mb += RB) {
      float rr[RB][TN][16];
#pragma unroll
      for (int b = 0; b < RB; ++b)
#pragma unroll
        for (int ni = 0; ni < TN; ++ni)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            int m = mw + (mb + b) * 32 + mfma32_crow(r, hi);
            m = m < p.M ? m : p.M - 1;
            rr[b][ni][r] = p.resid[(size_t)m * p.ldr + nw + ni * 32 + l31];
          }
#pragma unroll
      for (int b = 0; b < RB; ++b)
#pragma unroll
        for (int ni = 0; ni < TN; ++ni) {
          const int mi = mb + b;
          const int n = nw + ni * 32 + l31;
          const float bn = p.bias ? p.bias[n] : 0.f;
          if (full) {                                // wave-uniform: straight-line stores
#pragma unroll
            for (int r = 0; r < 16; ++r)
              p.C[(size_t)(mw + mi * 32 + mfma32_crow(r, hi)) * p.ldc + n] = rr[b][ni][r] + (acc[mi][ni][r] + bn);
          } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int m = mw + mi * 32 + mfma32_crow(r, hi);
              if (m < p.M) p.C[(size_t)m * p.ldc + n] = rr[b][ni][r] + (acc[mi][ni][r] + bn);
            }
          }
        }
    }
    return;
  }
  auto store_tile = [&](auto G) {
#pragma unroll
    for (int mi = 0; mi < TM; ++mi) {
#pragma unroll
      for (int ni = 0; ni < TN; ++ni) {
        const int n = nw + ni * 32 + l31;
        const float bn = p.bias ? p.bias[n] : 0.f;
        size_t qkv_col = 0;                            // head-major plane and column of this lane's output column (one division per column, not per element)
        if (EPI == EPI_QKV_HEADMAJOR) {
          const int dmodel = p.heads * 64;
          const int c = n / dmodel;
          const int rem = n - c * dmodel;
          qkv_col = ((size_t)c * p.heads + (rem >> 6)) * (size_t)p.M * 64 + (rem & 63);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = mw + mi * 32 + mfma32_crow(r, hi);
          if (decltype(G)::value && m >= p.M) continue;
          const float v = acc[mi][ni][r] + bn;
          if (EPI == EPI_BIAS) {
            p.C[(size_t)m * p.ldc + n] = v;
          } else if (EPI == EPI_SPLITK_PART) {         // plane blockIdx.y of the workspace: the bare partial sum
            p.splitk_ws[((size_t)blockIdx.y * p.M + m) * p.N + n] = acc[mi][ni][r];
          } else if (EPI == EPI_BIAS_SILU) {
            p.C[(size_t)m * p.ldc + n] = silu(v);
          } else if (EPI == EPI_BIAS_RELU) {
            p.C[(size_t)m * p.ldc + n] = fmaxf(v, 0.f);
          } else if (EPI == EPI_BIAS_GELU) {
            p.C[(size_t)m * p.ldc + n] = gelu_erf(v);
          } else if (EPI == EPI_BIAS_ANCHOR) {
            const int sel = p.anchor[m] ? 1 : 0;
            p.C[(size_t)m * p.ldc + n] = v + p.anchor_emb[(size_t)sel * p.N + n];
          } else if (EPI == EPI_QKV_HEADMAJOR) {
            p.C[qkv_col + (size_t)m * 64] = v;
          }
        }
      }
    }
  };
  if (mw + 32 * TM <= p.M) store_tile(std::false_type{}); else store_tile(std::true_type{});
}

// ---------------------------------------------------------------------------------------------
// The LDS-DMA kernels.  Ablation on MI355X (scripts/mfma_ablation.py) shows what cost the register-staged loop of rounds 1-2 its
// MFMA rate: a pure MFMA stream with LDS operand reads and a barrier per 64 MFMAs sustains ~141 TF, adding the 8 global_load_dwordx4
// + 8 ds_write_b128 per wave per k-tile drops it to ~122 TF.  Here the k-tiles go global -> LDS directly (global_load_lds_dwordx4: no
// VGPR round trip, no ds_write pass, 32 fewer VGPRs).  The DMA writes LDS lane-linearly (wave base + lane*16 B), so rows cannot be
// padded; bank conflicts are avoided by an XOR swizzle of the 16-byte slot index, slot' = slot ^ ((row >> 1) & 7), applied to the
// per-lane GLOBAL source address when staging and to the ds_read_b128 address when reading (conflict-free for every 16-lane group of
// ds_read_b128: rows {0-3,12-15,20-27} x one logical slot map to 16 distinct physical slots of the 256-byte bank row).
//
// What the one-tile-per-block kernel and the persistent kernel share: GemmTile, the geometry of a block tile of WM x WN waves, each
// TM x TN MFMA tiles of 32 x 32, with the fragment type and the accumulator clear; and the TG_* macros over the kernels' locals -- the
// staging swizzle, the fragment read, the DMA (inline asm), the MFMAs of a fragment and the k-tile step.  Macros, not functions: the chunk
// decode and the MFMAs as functions moved instructions of the 256 x 256 kernels, the fragment read has to name the LDS array itself.
// ---------------------------------------------------------------------------------------------
template <int WM, int WN, int TM, int TN>
struct GemmTile {
  static constexpr int NT = 64 * WM * WN;                       // threads
  static constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
  static constexpr int CA = BM * 8 / NT, CB = BN * 8 / NT;      // 16-byte chunks per thread per k-tile
  static constexpr int ABYTES = BM * 128, BBYTES = BN * 128;    // one stage of A / of W
  static constexpr int LDS_BYTES = 2 * (ABYTES + BBYTES);       // [A0 A1 B0 B1]
  struct Frag { float4 a[TM]; float4 b[TN]; };

  static __device__ __forceinline__ void clear(f32x16 (&acc)[TM][TN]) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  }
};

// What a kernel declares before it uses the macros below: the tile's constants and the lane's coordinates ...
#define TG_GEOMETRY                                                                                           \
  using T = GemmTile<WM, WN, TM, TN>;                                                                         \
  constexpr int NT = T::NT, BM = T::BM, BN = T::BN, CA = T::CA, CB = T::CB, ABYTES = T::ABYTES, BBYTES = T::BBYTES; \
  const int tid = threadIdx.x;                                                                                \
  const int lane = tid & 63;                                                                                  \
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);                                                  \
  const int hi = lane >> 5;                                                                                   \
  const int l31 = lane & 31;                                                                                  \
  const int wm = wave / WN, wn = wave % WN;
// staging: chunk id = I*NT + tid -> (row = id >> 3, physical slot = id & 7) holds logical slot lslot = slot ^ swz(row)
#define TG_CHUNK(I)                                                                                           \
  const int id = (I) * NT + tid;                                                                              \
  const int row = id >> 3;                                                                                    \
  const int lslot = (id & 7) ^ ((row >> 1) & 7);
// ... and, once `smem` is declared, the lane's LDS offsets and the read of k-group g (8 columns) of stage buf.  The DMA is issued from inline asm, not through the builtin (lds_dma.h); the
// transfer is retired by the explicit vmcnt(0) in front of the barrier that publishes the tile (TG_SYNC).
#define TG_LDS_OFFSETS                                                                                        \
  const int sw = (l31 >> 1) & 7;                                                                              \
  const int a_row = (wm * TM * 32 + l31) * 128;              /* byte offsets inside one A / B stage */        \
  const int b_row = (wn * TN * 32 + l31) * 128;                                                               \
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;             \
  const unsigned lds_wave = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)wave * 1024u);                    \
  auto read_frag = [&](typename T::Frag& f, int buf, int g) {                                                 \
    const int co = ((2 * g + hi) ^ sw) * 16;                                                                  \
    _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                            \
      f.a[i] = *reinterpret_cast<const float4*>(smem + buf * ABYTES + a_row + i * 32 * 128 + co);             \
    _Pragma("unroll") for (int j = 0; j < TN; ++j)                                                            \
      f.b[j] = *reinterpret_cast<const float4*>(smem + 2 * ABYTES + buf * BBYTES + b_row + j * 32 * 128 + co); \
  };
#define TG_LDS_A(BUF, I) (lds_wave + (unsigned)((BUF) * ABYTES + (I) * NT * 16))
#define TG_LDS_W(BUF, I) (lds_wave + (unsigned)(2 * ABYTES + (BUF) * BBYTES + (I) * NT * 16))
// k-tile KT into stage BUF from per-lane addresses.  PAIRED (the 128 x 128 form) issues the A and W chunks alternately, the
// 256 x 256 form all of A first: each as it was measured.
#define TG_DMA(KT, BUF)                                                                                       \
  _Pragma("unroll") for (int i = 0; i < CA; ++i) {                                                            \
    LDS_DMA_X4(a_src[i] + (size_t)(KT) * GBK, TG_LDS_A(BUF, i))                                               \
    if constexpr (PAIRED) LDS_DMA_X4(w_src[i] + (size_t)(KT) * GBK, TG_LDS_W(BUF, i))                         \
  }                                                                                                           \
  if constexpr (!PAIRED) {                                                                                    \
    _Pragma("unroll") for (int i = 0; i < CB; ++i)                                                            \
      LDS_DMA_X4(w_src[i] + (size_t)(KT) * GBK, TG_LDS_W(BUF, i))                                             \
  }
// the same from a scalar base per operand plus the lane's 32-bit byte offsets (the saddr form of global_load_lds)
#define TG_DMA_SADDR(ABASE, WBASE, BUF)                                                                       \
  _Pragma("unroll") for (int i = 0; i < CA; ++i)                                                              \
    LDS_DMA_X4_SADDR(a_off[i], ABASE, TG_LDS_A(BUF, i))                                                       \
  _Pragma("unroll") for (int i = 0; i < CB; ++i)                                                              \
    LDS_DMA_X4_SADDR(w_off[i], WBASE, TG_LDS_W(BUF, i))
#define TG_SYNC asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); __syncthreads();
// raw barrier (no memory fence needed: LDS-DMA arrival is confirmed by this wave's vmcnt, fragment reads of the stage that the next
// DMA overwrites by lgkmcnt -- they were issued one MFMA group earlier, so the wait is free)
#define TG_SYNC_RAW asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_sched_barrier(0); __builtin_amdgcn_s_barrier(); __builtin_amdgcn_sched_barrier(0);
#define TG_FENCE __builtin_amdgcn_sched_barrier(0);
#define TG_READ(F, BUF, G) read_frag(F, BUF, G);
#define TG_MMA_K(F, C)                                                                                  \
  _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                        \
    _Pragma("unroll") for (int j = 0; j < TN; ++j)                                                      \
      acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(F.a[i].C, F.b[j].C, acc[i][j], 0, 0, 0);
#define TG_MMA(F) TG_MMA_K(F, x) TG_MMA_K(F, y) TG_MMA_K(F, z) TG_MMA_K(F, w)
// One k-tile from stage CUR, f0 holding its k-group 0: each group's fragments are read under the MFMAs of the group before.  SYNC
// publishes the successor k-tile in front of the last group's MFMAs and NEXT reads its k-group 0 under them; both empty: the last k-tile.
#define TG_KSTEP(CUR, SYNC, NEXT)                                                                             \
  TG_READ(f1, CUR, 1)                                                                                         \
  TG_FENCE                                                                                                    \
  TG_MMA(f0)                                                                                                  \
  TG_FENCE                                                                                                    \
  TG_READ(f0, CUR, 2)                                                                                         \
  TG_FENCE                                                                                                    \
  TG_MMA(f1)                                                                                                  \
  TG_FENCE                                                                                                    \
  TG_READ(f1, CUR, 3)                                                                                         \
  TG_FENCE                                                                                                    \
  TG_MMA(f0)                                                                                                  \
  TG_FENCE                                                                                                    \
  SYNC                                                                                                        \
  NEXT                                                                                                        \
  TG_MMA(f1)

// ---------------------------------------------------------------------------------------------
// One output tile per block.  Two instantiations per epilogue:
//  <EPI, 2, 2, 2, 2>  the 128 x 128 kernel: 4 waves, 64 KB of LDS, two blocks per CU that cover each other's prologue and epilogue -- the
//                     K = 64 embedding GEMM, narrow outputs, few-token calls, and with EPI_SPLITK_PART the split-K partial products
//  <EPI, 2, 4, 4, 2>  the 256 x 256 kernel (form 32): 8 waves, wave tile 128 x 64 -- the shape of the 16-bit GEMM (gemm_h16.hip).  Per 4
//                     k-values a wave reads 6 fragments for 32 MFMAs (the 128 x 128 kernel: 4 for 16) and meets a barrier every 256 MFMAs
//                     instead of every 64; one block per CU (128 KB of LDS), so prologue and epilogue are not covered by a second block.
//                     N % 256 == 0, else the launcher takes the 128 x 128 kernel.
// ---------------------------------------------------------------------------------------------
__device__ unsigned int g_gemm_cu_arrivals[16 * 256];
template <int EPI, int WM, int WN, int TM, int TN>
__global__ __launch_bounds__(64 * WM * WN, WM * WN == 4 ? 2 : 1) void gemm_f32_tile_kernel(GemmParams p) {
  TG_GEOMETRY
  constexpr bool PAIRED = BM == 128;
  static_assert(!PAIRED || CA == CB, "TG_DMA pairs chunk i of A with chunk i of W");
  // The tile's LDS: static where it fits (64 KB: the launch needs no opt-in, two blocks share a CU), dynamic above.  Both arrays are declared
  // and `smem` is a reference to the one in use: a declaration inside an `if constexpr` branch ends with the branch, and through a pointer
  // variable hipcc folds the ds_read addresses differently (the 256 x 256 kernels changed).  The array not referenced takes no LDS.
  __shared__ __attribute__((aligned(1024))) unsigned char smem_static[T::LDS_BYTES <= 65536 ? T::LDS_BYTES : 1024];
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem_dynamic[];
  auto& smem = *[&]() { if constexpr (T::LDS_BYTES <= 65536) return &smem_static; else return &smem_dynamic; }();

  const int nt = p.N / BN;
  const int mt = (p.M + BM - 1) / BM;
  const int logical = xcd_remap(blockIdx.x, mt * nt);
  const int m0 = (logical / nt) * BM;
  const int n0 = (logical % nt) * BN;

  // Two blocks share a CU (2 waves per SIMD) and all blocks take the same time, so blocks launched together stay IN PHASE for
  // the whole kernel: both wait for their first tile, both run their epilogue at the same moment and the matrix pipe idles.  The
  // second resident block of every CU therefore starts half a block-duration late (one block = K/32 k-tiles x 64 MFMAs x 64 cycles,
  // twice that with the SIMD shared), after which each block's prologue / epilogue falls into the other's main loop.
  if (BM == 128 && p.stagger && blockIdx.x < 512) {
    bool late = blockIdx.x >= 256;                                       // 1: assume breadth-first placement of the first 512 blocks
    if (p.stagger == 2) {                                                // 2: ask the hardware which CU this is, count arrivals
      __shared__ unsigned int slot_s;
      if (tid == 0) {
        const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);   // HW_ID: CU_ID [11:8], SH_ID [12], SE_ID [15:13]
        const unsigned xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20) & 15u;
        slot_s = atomicAdd(&g_gemm_cu_arrivals[(xcc << 8) | ((hw >> 8) & 0xffu)], 1u);
      }
      __syncthreads();
      late = slot_s & 1u;
    }
    if (late) {
      const unsigned long long t0 = wall_clock64();                        // 100 MHz
      unsigned long long ticks = (unsigned long long)(p.K / GBK) * 178ull;         // 4096 cycles at ~2.3 GHz per k-tile
      ticks = ticks < 20000ull ? ticks : 20000ull;                                 // never more than 0.2 ms
      while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
    }
  }

  // DMA sources (rows past M clamped: their products are never stored)
  const float* a_src[CA];
  const float* w_src[CB];
#pragma unroll
  for (int i = 0; i < CA; ++i) {
    TG_CHUNK(i)
    int r = m0 + row;
    r = r < p.M ? r : p.M - 1;
    a_src[i] = p.A + (size_t)r * p.lda + 4 * lslot;
  }
#pragma unroll
  for (int i = 0; i < CB; ++i) {
    TG_CHUNK(i)
    w_src[i] = p.W + (size_t)(n0 + row) * p.ldw + 4 * lslot;
  }

  f32x16 acc[TM][TN];
  T::clear(acc);

  int nk = p.K / GBK;
  if (EPI == EPI_SPLITK_PART) {                      // this block's share of the k-tiles
    const int k0 = (int)((long)nk * blockIdx.y / gridDim.y), k1 = (int)((long)nk * (blockIdx.y + 1) / gridDim.y);
#pragma unroll
    for (int i = 0; i < CA; ++i) a_src[i] += (size_t)k0 * GBK;
#pragma unroll
    for (int i = 0; i < CB; ++i) w_src[i] += (size_t)k0 * GBK;
    nk = k1 - k0;
  }
  TG_LDS_OFFSETS

  typename T::Frag f0, f1;
  TG_DMA(0, 0)
  TG_SYNC
  TG_READ(f0, 0, 0)

  int kt = 0;
  for (; kt + 1 < nk; ++kt) {
    const int cur = kt & 1;
    TG_DMA(kt + 1, cur ^ 1)                 // spare stage: every wave finished reading it before the last barrier
    // TG_SYNC: tile kt+1 landed (vmcnt(0)) and visible; reads of tile kt complete
    TG_KSTEP(cur, TG_SYNC, TG_READ(f0, cur ^ 1, 0) TG_FENCE)
    TG_FENCE
  }
  TG_KSTEP(kt & 1, , )

  gemm_f32_epilogue<EPI, TM>(p, acc, m0 + wm * TM * 32, n0 + wn * TN * 32, hi, l31);
}

// ---------------------------------------------------------------------------------------------
// Persistent form of the 256 x 256 kernel (round 3; the same idea as gemm_h16_php_kernel, where scripts/gemm_ts.py itemised the per-tile
// overhead of a one-tile-per-block launch: block start-up and tile decode, the wait for the first k-tile, the gap to the next block).
// ONE block per CU walks the tiles of its XCD (virtual block id v = blockIdx.x + i * gridDim.x, gridDim.x a multiple of 8) and the
// k-tiles of consecutive output tiles form one DMA stream: the last k-tile of an output tile requests the first k-tile of the NEXT one
// into the spare stage exactly as it would request its own successor, so the next k-loop starts on landed data and the epilogue's
// stores (straight from the accumulator registers: no LDS involved) drain under it.  Sources are a scalar base (tile origin + k offset)
// plus one 32-bit per-thread byte offset per 16-byte chunk (the saddr form of global_load_lds): needs M % 256 == 0 (no row clamping).
// Same MFMA order, same epilogue: results are bit-identical to gemm_f32_tile_kernel<EPI, 2, 4, 4, 2>.
// ---------------------------------------------------------------------------------------------
template <int EPI>
__global__ __launch_bounds__(512) void gemm_f32_persistent_kernel(GemmParams p) {
  constexpr int WM = 2, WN = 4, TM = 4, TN = 2;
  TG_GEOMETRY
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];

  const int nt = p.N / BN;
  const int total = (p.M / BM) * nt;
  const int nk = p.K / GBK;

  unsigned a_off[CA], w_off[CB];           // byte offsets inside the tile's A / W panel at k = 0
#pragma unroll
  for (int i = 0; i < CA; ++i) { TG_CHUNK(i) a_off[i] = (unsigned)(row * p.lda + 4 * lslot) * 4u; }
#pragma unroll
  for (int i = 0; i < CB; ++i) { TG_CHUNK(i) w_off[i] = (unsigned)(row * p.ldw + 4 * lslot) * 4u; }

  f32x16 acc[TM][TN];
  TG_LDS_OFFSETS
  typename T::Frag f0, f1;

  auto tile_bases = [&](int v, const unsigned char*& ab, const unsigned char*& wb, int& m0, int& n0) {
    const int logical = xcd_remap(v, total);
    m0 = (logical / nt) * BM;
    n0 = (logical % nt) * BN;
    ab = reinterpret_cast<const unsigned char*>(p.A) + (size_t)m0 * p.lda * 4;
    wb = reinterpret_cast<const unsigned char*>(p.W) + (size_t)n0 * p.ldw * 4;
  };

  int v = blockIdx.x;
  const unsigned char *a_cur, *w_cur, *a_nxt = nullptr, *w_nxt = nullptr;
  int m0, n0, m0n = 0, n0n = 0;
  tile_bases(v, a_cur, w_cur, m0, n0);
  TG_DMA_SADDR(a_cur, w_cur, 0)
  TG_SYNC_RAW
  int par = 0;                              // stage of the current k-tile of the stream

  for (;;) {
    const int vn = v + (int)gridDim.x;
    const bool has_next = vn < total;
    if (has_next) tile_bases(vn, a_nxt, w_nxt, m0n, n0n);
    T::clear(acc);
    TG_READ(f0, par, 0)

    for (int kt = 0; kt < nk; ++kt) {
      const int cur = par;
      const bool in1 = kt + 1 < nk;
      if (in1) { TG_DMA_SADDR(a_cur + (size_t)(kt + 1) * (GBK * 4), w_cur + (size_t)(kt + 1) * (GBK * 4), cur ^ 1) }
      else if (has_next) { TG_DMA_SADDR(a_nxt, w_nxt, cur ^ 1) }       // the stream continues into the next output tile
      // TG_SYNC_RAW: successor k-tile landed (vmcnt(0): also this block's earlier stores) and visible; reads of `cur` complete
      TG_KSTEP(cur, TG_SYNC_RAW, if (in1) { TG_READ(f0, cur ^ 1, 0) } TG_FENCE)
      TG_FENCE
      par ^= 1;
    }
    gemm_f32_epilogue<EPI, TM>(p, acc, m0 + wm * TM * 32, n0 + wn * TN * 32, hi, l31);
    if (!has_next) break;
    v = vn; a_cur = a_nxt; w_cur = w_nxt; m0 = m0n; n0 = n0n;
  }
}
#undef TG_GEOMETRY
#undef TG_CHUNK
#undef TG_LDS_OFFSETS
#undef TG_LDS_A
#undef TG_LDS_W
#undef TG_DMA
#undef TG_DMA_SADDR
#undef TG_SYNC
#undef TG_SYNC_RAW
#undef TG_FENCE
#undef TG_READ
#undef TG_MMA
#undef TG_MMA_K
#undef TG_KSTEP
#undef TG_GELU_ERF

// C[m][n] = resid[m][n] + bias[n] + sum_s part[s][m][n]   (the split-K path of EPI_BIAS_RESID; one thread per 4 columns)
// SILU (round 6, the two hidden layers of final_mlp in few-token calls): no residual, C = silu(bias + sum of the partials)
template <bool SILU>
__global__ __launch_bounds__(256) void gemm_splitk_combine_kernel(GemmParams p, int splits) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int n4 = p.N / 4;
  if (i >= (long)p.M * n4) return;
  const long m = i / n4;
  const int n = (int)(i % n4) * 4;
  float4 acc = SILU ? float4{0.f, 0.f, 0.f, 0.f} : *reinterpret_cast<const float4*>(p.resid + m * p.ldr + n);
  if (p.bias) {
    const float4 b = *reinterpret_cast<const float4*>(p.bias + n);
    acc.x += b.x; acc.y += b.y; acc.z += b.z; acc.w += b.w;
  }
  for (int s = 0; s < splits; ++s) {
    const float4 v = *reinterpret_cast<const float4*>(p.splitk_ws + ((size_t)s * p.M + m) * p.N + n);
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
  }
  if (SILU) {
    acc.x = silu(acc.x); acc.y = silu(acc.y); acc.z = silu(acc.z); acc.w = silu(acc.w);
  }
  *reinterpret_cast<float4*>(p.C + m * p.ldc + n) = acc;
}

// Kernel choice: the LDS-DMA 256 x 256 / 8-wave kernel wherever there are at least two rounds of its tiles, N % 256 == 0 and
// K >= 256 (r02 call 40: qkv 128 vs 119 TF, ff1 132 vs 129, ff2 139 vs 131, head 125 vs 119, out-projection equal); the LDS-DMA
// 128 x 128 kernel (two blocks per CU cover each other's prologue) for the K = 64 embedding GEMM, narrow outputs and few-token calls.
// Tuning key 0, honoured by the RAP_ABLATION_BUILD library only: 16 = the 128 x 128 kernel for every shape, 32 = the 256 x 256 kernels
// wherever N % 256 == 0 (persistent as key 12 and the shape allow), 48 (default; any other value) = by shape, as above.
rap_tuning_t g_rap_gemm_variant = 48;

rap_tuning_t g_rap_gemm_f32_persistent = 1;     // tuning key 12: the persistent 256 x 256 kernel for full-tile shapes (1, default) or one tile per block (0)

// Grid of the persistent 256 x 256 kernels, here and in gemm_h16.hip (kernels.h)
int rap_persistent_blocks(int tiles) {
  static std::atomic<int> n_cu_cache[16] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  int n_cu = (dev >= 0 && dev < 16) ? n_cu_cache[dev].load() : 0;
  if (n_cu == 0) {
    if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n_cu <= 0) return 0;
    n_cu = n_cu >= 8 ? (n_cu / 8) * 8 : n_cu;     // a multiple of the XCD count: a block's virtual ids stay on its XCD
    if (dev >= 0 && dev < 16) n_cu_cache[dev] = n_cu;
  }
  return tiles < n_cu ? tiles : n_cu;
}

// One tile per block: gridDim.y blocks per tile (more than one: EPI_SPLITK_PART).  The 64 KB of the 128 x 128 form are static LDS.
template <int EPI, int WM, int WN, int TM, int TN>
static int launch_gemm_tile(hipStream_t stream, const GemmParams& p, int grid_y = 1) {
  using T = GemmTile<WM, WN, TM, TN>;
  const dim3 grid(((p.M + T::BM - 1) / T::BM) * (p.N / T::BN), grid_y);
  if (T::LDS_BYTES > 65536) return rap_launch_dyn_lds(gemm_f32_tile_kernel<EPI, WM, WN, TM, TN>, grid, dim3(T::NT), T::LDS_BYTES, stream, p);
  hipLaunchKernelGGL((gemm_f32_tile_kernel<EPI, WM, WN, TM, TN>), grid, dim3(T::NT), 0, stream, p);
  RAP_LAUNCH_CHECK();
  return RAP_OK;
}

template <int EPI>
static int launch_gemm_variant(hipStream_t stream, const GemmParams& p, int form) {
  if (rap_form_kernel(form) == RAP_FORM_256P) {
    const int blocks = rap_persistent_blocks((p.M / 256) * (p.N / 256));
    if (blocks <= 0) return RAP_ERR_HIP;
    return rap_launch_dyn_lds(gemm_f32_persistent_kernel<EPI>, dim3(blocks), dim3(512), GemmTile<2, 4, 4, 2>::LDS_BYTES, stream, p);
  }
  if (rap_form_kernel(form) == RAP_FORM_256) return launch_gemm_tile<EPI, 2, 4, 4, 2>(stream, p);
  return launch_gemm_tile<EPI, 2, 2, 2, 2>(stream, p);
}

rap_tuning_t g_rap_gemm_splitk = 1;      // tuning key 6: 0 = never split K for few-row calls
rap_tuning_t g_rap_gemm_stagger = 1;     // measured (r01 run 39): +1.3 % on the K = 512 shapes, +1.2 % at K = 2048; 2 (by CU id) is no better
// tuning key 9 (fp32 path): GEGLU's Phi(g).  1 (default since r02 call 50) = Abramowitz-Stegun 7.1.26 erfc, |error| <= 1.5e-7 absolute
// (about one fp32 ulp of Phi near 1/2), on the packed fp32 pipe, stage-major over eight output pairs (half.h: geglu_pairs) -- the
// epilogue of the largest GEMM of a layer was ~50 scalar VALU instructions per output with erff: ff1 8.35 -> 8.09 ms (131.7 -> 135.9 TF),
// headline 15 940 -> 16 049 points/s, all-step deviation from the unmodified reference unchanged (final cloud 5.4e-7 vs 6.6e-7,
// per-step maximum 9.5e-7 vs 8.3e-7: the fp32 noise floor).  0 = libm-grade erff.
rap_tuning_t g_rap_geglu_fast = 1;
// The dispatch decision as host arithmetic (kernels.h: the form codes): which kernel a call takes, and over how many blocks per tile its K
// is split.  launch_gemm_f32 switches on the result; tests/test_gemm_cases_host.py pins it through rap_gemm_f32_form.
//  * K split over 4 blocks per 128 x 128 tile, bias + residual with a workspace -- few-row calls: K >= 1024 (ff2) when the tile grid covers at
//    most half of the CUs, K >= 512 (the out-projection) when it covers at most a quarter (r03: one pair of 2 x 1024 points -- 64 tiles, a
//    chain of 16 k-tiles each); the k-tiles need not divide evenly (block y takes k-tiles [nk y / 4, nk (y + 1) / 4))
//  * K split over `splitk_planes` (2 or 4) blocks per tile, bias + SiLU with a workspace -- the hidden layers of final_mlp (fp32 in every mode)
//    of a few-token call: 64 / 32 tiles of a 16-k-tile chain on 256 CUs (r06 call 2: 39 us per launch, a fifth of a demo-size pair's per-step
//    overhead); the k-tiles must divide evenly here
//  * otherwise the 256 x 256 kernel from 512 of its tiles on (N % 256 == 0, K >= 256), persistent when every row tile is full
int gemm_f32_splits_by_shape(int epilogue, int M, int N, int K, int planes) {
  if (M <= 0 || N <= 0 || N % GBN != 0 || K <= 0 || K % GBK != 0) return 1;
  const long tiles128 = (long)((M + GBM - 1) / GBM) * (N / GBN);
  if (epilogue == EPI_BIAS_RESID) return ((K >= 1024 && tiles128 <= 128) || (K >= 512 && tiles128 <= 64)) ? 4 : 1;
  if (epilogue == EPI_BIAS_SILU) return ((planes == 2 || planes == 4) && K >= 512 && (K / GBK) % planes == 0 && tiles128 <= 64) ? planes : 1;
  return 1;
}
int gemm_f32_form(int epilogue, const GemmParams& p) {
  if (p.M <= 0) return 0;
  if (p.N % GBN != 0 || p.K % GBK != 0 || p.K <= 0) return RAP_ERR_INVALID;
  if ((p.lda & 3) || (p.ldw & 3)) return RAP_ERR_INVALID;
  if (epilogue < EPI_BIAS || epilogue > EPI_BIAS_GELU || epilogue == EPI_SPLITK_PART) return RAP_ERR_INVALID;
  int v = 48;
#ifdef RAP_ABLATION_BUILD
  v = g_rap_gemm_variant;
#endif
  if (v != 16 && v != 32) v = (p.N % 256 == 0 && p.K >= 256 && (long)((p.M + 255) / 256) * (p.N / 256) >= 512) ? 32 : 16;
  if (p.splitk_ws && g_rap_gemm_splitk && (p.ldc & 3) == 0 && (epilogue != EPI_BIAS_RESID || (p.ldr & 3) == 0)) {
    const int splits = gemm_f32_splits_by_shape(epilogue, p.M, p.N, p.K, p.splitk_planes);
    if (splits > 1) return rap_gemm_form(RAP_FORM_128, 2, splits);
  }
  if (v == 32 && p.N % 256 == 0) {
    const bool persistent = g_rap_gemm_f32_persistent && p.M % 256 == 0 && (long)(p.M / 256) * (p.N / 256) >= 512 && p.lda <= (1 << 20) &&
                            p.ldw <= (1 << 20);
    return rap_gemm_form(persistent ? RAP_FORM_256P : RAP_FORM_256, 0, 1);
  }
  return rap_gemm_form(RAP_FORM_128, 2, 1);
}

int launch_gemm_f32(hipStream_t stream, int epilogue, const GemmParams& p_in) {
  GemmParams p = p_in;
  p.geglu_fast = g_rap_geglu_fast;
  p.stagger = ((long)((p.M + GBM - 1) / GBM) * (p.N / GBN) >= 1024) ? g_rap_gemm_stagger.load() : 0;     // only when the chip is filled twice over
  const int form = gemm_f32_form(epilogue, p);
  if (form <= 0) return form;      // nothing to do (M <= 0) or a refused shape
  const int splits = rap_form_splits(form);
  if (splits > 1) {                // partial tiles to splitk_ws, then one combine pass (residual + bias + partials, or SiLU of bias + partials)
    const int rc = launch_gemm_tile<EPI_SPLITK_PART, 2, 2, 2, 2>(stream, p, splits);
    if (rc != RAP_OK) return rc;
    const dim3 grid((unsigned)(((long)p.M * (p.N / 4) + 255) / 256));
    if (epilogue == EPI_BIAS_RESID) hipLaunchKernelGGL(gemm_splitk_combine_kernel<false>, grid, dim3(256), 0, stream, p, splits);
    else hipLaunchKernelGGL(gemm_splitk_combine_kernel<true>, grid, dim3(256), 0, stream, p, splits);
    RAP_LAUNCH_CHECK();
    return RAP_OK;
  }
  switch (epilogue) {
    case EPI_BIAS: return launch_gemm_variant<EPI_BIAS>(stream, p, form);
    case EPI_BIAS_RESID: return launch_gemm_variant<EPI_BIAS_RESID>(stream, p, form);
    case EPI_BIAS_SILU: return launch_gemm_variant<EPI_BIAS_SILU>(stream, p, form);
    case EPI_GEGLU: return launch_gemm_variant<EPI_GEGLU>(stream, p, form);
    case EPI_QKV_HEADMAJOR:
      if (p.N != 3 * p.heads * 64) return RAP_ERR_INVALID;
      if (p.gamma_q && !p.gamma_k) return RAP_ERR_INVALID;
      return launch_gemm_variant<EPI_QKV_HEADMAJOR>(stream, p, form);
    case EPI_BIAS_ANCHOR: return launch_gemm_variant<EPI_BIAS_ANCHOR>(stream, p, form);
    case EPI_BIAS_RELU: return launch_gemm_variant<EPI_BIAS_RELU>(stream, p, form);
    case EPI_BIAS_GELU: return launch_gemm_variant<EPI_BIAS_GELU>(stream, p, form);
    default: return RAP_ERR_INVALID;
  }
}
