// bf16 / fp16 GEMM on the CDNA4 matrix cores:  C (M,N) = A (M,K) * W (N,K)^T  + fused epilogue, fp32 accumulate.
//
// The reduced-precision twin of gemm_f32.hip for the transformer blocks' dense layers (reference
// flow_model/layer.py:73-74,81-82,89 under Lightning "16-mixed"/"bf16-mixed" autocast, trainer/infer.yaml:6):
// qkv projection, attention out-projection, GEGLU feed-forward.  Embedding and the fp32 head stay on gemm_f32.
//
// Design (gfx950 only):
//  * v_mfma_f32_32x32x16_{bf16,f16}: 8 k-values per lane per operand, 32 cycles per instruction per SIMD.
//  * BK = 64 elements = one 128-byte line per row per k-tile -- byte-for-byte the LDS image of the fp32 kernel's
//    LDS-DMA variant: tiles go global -> LDS with global_load_lds_dwordx4 (no VGPR round trip, no ds_write pass);
//    the DMA writes LDS lane-linearly, so bank conflicts are removed by an XOR swizzle of the 16-byte slot index,
//    slot' = slot ^ ((row >> 1) & 7), applied to the per-lane GLOBAL source address when staging and to the
//    ds_read_b128 address when reading (conflict-free for every 16-lane group of ds_read_b128).
//  * one ds_read_b128 = the 8 k-values of one MFMA operand; k-step g of a tile reads slot 2g + (lane >> 5).
//  * block tile (32*TM*WM) x (32*TN*WN), WM x WN waves, each wave TM x TN MFMA tiles; double-buffered LDS, one
//    barrier per k-tile, the DMA of tile t+1 is issued before the MFMAs of tile t and retired (vmcnt(0)) in front
//    of the barrier that publishes it; operand fragments of k-step g+1 are read while step g's MFMAs issue.
//    At 16x the fp32 MFMA rate the kernel is L2->LDS bandwidth bound at 128x128 (64 B/clk/CU needed vs ~56
//    available), hence the 256x256 / 8-wave instantiation for the large shapes.
//  * 1-D grid, XCD-aware remap, n-tile fastest (A panel stays in one XCD's L2).
#include <type_traits>
#include "half.h"
#include "kernels.h"
#include "lds_dma.h"
#include "gemm_h16_epilogue.h"

// Split precision (RAP_DT_F32X2, half.h): fragments 0, 1 of a k-tile are the head and 2, 3 the tail fragments of its two k-steps.  The six
// kept products, as (A fragment, W fragment): (tail, head) and (head, tail) of both k-steps, then (head, head); OP(args..., ka, kb) each.
#define X2_PRODUCTS(OP, ...) \
  OP(__VA_ARGS__, 2, 0) OP(__VA_ARGS__, 0, 2) OP(__VA_ARGS__, 3, 1) OP(__VA_ARGS__, 1, 3) OP(__VA_ARGS__, 0, 0) OP(__VA_ARGS__, 1, 1)

// X2 (round 5, the residual GEMMs of few-token split-precision calls): the paired-operand product of the phase-split kernels (three MFMAs
// per fragment pair, see gemm_h16_ph_kernel) on this kernel's 128 x 128 tiles -- the four fragment sets of a k-tile (head k-steps 0, 1 and
// tail k-steps 0, 1) are read, then the six kept products issue.
//
// NS (round 6, few-token calls): LDS stages.  2 = the double-buffered loop above (two blocks per CU).  4 = a ring of four stages with
// the DMA of tile t + 3 issued while tile t multiplies and COUNTED waits (vmcnt(2 tiles)): when a launch has no more blocks than the part
// has CUs (one pair of 2 x 1024 points: 64 ... 512 blocks) a block has the CU to itself, the second block of the two-stage form hides
// nothing, and the k-loop is one L2 round trip (~1 us) per k-tile against 0.25-0.4 us of MFMA issue (profiles/r05_c13_*).  Three tiles
// in flight cover the latency.  Same k order per accumulator: results are bit-identical to NS = 2.
// EPI_H_QKV_NORM without X2 (round 6): the q / k column tiles run the swapped product and leave through gemm_h16_qknorm_epilogue, the
// V tiles through the EPI_H_QKV epilogue -- the fused form used to exist only in the 256 x 256 phase-split kernels.
template <int EPI, int DT, int WM, int WN, int TM, int TN, bool X2 = false, int NS = 2>
__global__ __launch_bounds__(64 * WM * WN, (NS > 2 ? 1 : 2)) void gemm_h16_kernel(GemmParamsH p) {
  typedef typename H16<DT>::T8 T8;
  constexpr int NT = 64 * WM * WN;
  constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
  constexpr int CA = BM * 8 / NT, CB = BN * 8 / NT;   // 16-byte chunks per thread per k-tile
  constexpr int ABYTES = BM * 128, BBYTES = BN * 128;
  static_assert(NS == 2 || NS == 4, "two stages (two blocks per CU) or a ring of four (one block per CU)");
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];   // [A0 .. A(NS-1) B0 .. B(NS-1)]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5;
  const int l31 = lane & 31;
  const int wm = wave / WN, wn = wave % WN;

  const int nt = p.N / BN;
  // (both QKV epilogues own the V^T image up to align_up(M, 256) token rows -- zeros beyond M, as the 256-row kernels leave it and as
  // include/rapflow.h documents; the plain one used to stop at align_up(M, 128), leaving up to 128 rows of the image unwritten)
  const int mt = (EPI == EPI_H_QKV_NORM || EPI == EPI_H_QKV) ? ((p.M + 255) / 256) * (256 / BM) : (p.M + BM - 1) / BM;
  const int logical = xcd_remap(blockIdx.x, mt * nt);
  const int m0 = (logical / nt) * BM;
  const int n0 = (logical % nt) * BN;

  // DMA sources: chunk id = i*NT + tid -> (row = id >> 3, physical slot = id & 7) holds logical slot (slot ^ swz(row))
  const u16* a_src[CA];
  const u16* w_src[CB];
#pragma unroll
  for (int i = 0; i < CA; ++i) {
    const int id = i * NT + tid;
    const int row = id >> 3;
    const int lslot = (id & 7) ^ ((row >> 1) & 7);
    int r = m0 + row;
    r = r < p.M ? r : p.M - 1;
    a_src[i] = p.A + (size_t)r * p.lda + 8 * lslot;
  }
#pragma unroll
  for (int i = 0; i < CB; ++i) {
    const int id = i * NT + tid;
    const int row = id >> 3;
    const int lslot = (id & 7) ^ ((row >> 1) & 7);
    w_src[i] = p.W + (size_t)(n0 + row) * p.ldw + 8 * lslot;
  }

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // split-K (launch_splitk below: EPI_H_BIAS_RESID_F32 without bias / residual, gridDim.y = splits): block y multiplies k-tiles
  // [y nk, (y + 1) nk) and writes plane y of the fp32 partial buffer
  const int nk = p.K / 64 / (EPI == EPI_H_BIAS_RESID_F32 ? (int)gridDim.y : 1);
  if constexpr (EPI == EPI_H_BIAS_RESID_F32) {
    const size_t koff = (size_t)blockIdx.y * nk * 64;
#pragma unroll
    for (int i = 0; i < CA; ++i) a_src[i] += koff;
#pragma unroll
    for (int i = 0; i < CB; ++i) w_src[i] += koff;
  }
  const int sw = (l31 >> 1) & 7;
  const int a_row = (wm * TM * 32 + l31) * 128;                       // byte offsets inside one A / B buffer
  const int b_row = (wn * TN * 32 + l31) * 128;

  // LDS-DMA (lds_dma.h) of the wave's 1 KiB pieces of a k-tile
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
  const unsigned lds_wave = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)wave * 1024u);
#define HG_DMA(KT, BUF)                                                                                       \
  _Pragma("unroll") for (int i = 0; i < CA; ++i)                                                              \
    LDS_DMA_X4(a_src[i] + (size_t)(KT) * 64, lds_wave + (unsigned)((BUF) * ABYTES + i * NT * 16))             \
  _Pragma("unroll") for (int i = 0; i < CB; ++i)                                                              \
    LDS_DMA_X4(w_src[i] + (size_t)(KT) * 64, lds_wave + (unsigned)(NS * ABYTES + (BUF) * BBYTES + i * NT * 16))
#define HG_SYNC asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); __syncthreads();
#define HG_FENCE __builtin_amdgcn_sched_barrier(0);

  struct Frag { uint4 a[TM]; uint4 b[TN]; };
  Frag f0, f1;
  auto read_frag = [&](Frag& f, int buf, int g) {
    const int co = ((2 * g + hi) ^ sw) * 16;
#pragma unroll
    for (int i = 0; i < TM; ++i)
      f.a[i] = *reinterpret_cast<const uint4*>(smem + buf * ABYTES + a_row + i * 32 * 128 + co);
#pragma unroll
    for (int j = 0; j < TN; ++j)
      f.b[j] = *reinterpret_cast<const uint4*>(smem + NS * ABYTES + buf * BBYTES + b_row + j * 32 * 128 + co);
  };
  // acc += A rows of fa_ x W rows of fb_, or the SWAPPED product (swp_c true: the MFMA's A operand is the weight fragment)
  auto mm = [&](auto swp_c, const Frag& fa_, const Frag& fb_) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        if constexpr (decltype(swp_c)::value) acc[i][j] = H16<DT>::mfma(__builtin_bit_cast(T8, fb_.b[j]), __builtin_bit_cast(T8, fa_.a[i]), acc[i][j]);
        else acc[i][j] = H16<DT>::mfma(__builtin_bit_cast(T8, fa_.a[i]), __builtin_bit_cast(T8, fb_.b[j]), acc[i][j]);
      }
  };
  auto mma = [&](const Frag& f) { mm(std::false_type{}, f, f); };
#define HG_X2_MM(F, KA, KB) mm(swp_c, F[KA], F[KB]);      // one of the X2_PRODUCTS of a k-tile's four fragment sets F
  constexpr bool RING = NS > 2 || (EPI == EPI_H_QKV_NORM && !X2);
  if constexpr (!RING) {      // the two-stage loops: tile 0
    HG_DMA(0, 0)
    HG_SYNC
  }
  // EPI_H_QKV_NORM: the q / k column tiles run the swapped product (a lane owns a token row: the row norm is lane-local), as in the
  // phase-split kernels; a compile-time property of the k-loop copy that runs.  Block-uniform: a 128-column tile is all q / k or all v.
  const bool swp = EPI == EPI_H_QKV_NORM && (n0 + wn * 64) < 2 * p.heads * 64;

  if constexpr (RING) {
    // ---- ring of NS stages (NS = 2: the plain double buffer, for the non-X2 fused QKV tiles), swapped product on q / k column tiles
    auto ring = [&](auto swp_c) __attribute__((always_inline)) {
#pragma unroll
      for (int s_ = 0; s_ < NS - 1; ++s_)
        if (s_ < nk) { HG_DMA(s_, s_) }
      if constexpr (NS > 2) {
        // The fragments of tile t + 1 are read while tile t multiplies (two register sets, the loop unrolled by two): with one wave per SIMD
        // and one barrier per k-tile all four waves would otherwise read (16 ds_read_b128 each) and multiply in lockstep, LDS pipe and
        // matrix pipe taking turns (r06 call 1: 0.65 us per split-precision k-tile against 0.37 us of MFMA issue).  At the barrier of
        // iteration t tile t + 1 is visible, tile t is in registers (its reads may still be in flight: its buffer is not reused before the
        // NEXT barrier), tile t - 1 is consumed and its buffer takes the DMA of tile t + NS - 1; NS - 3 younger tiles stay in flight.
        if (NS - 2 < nk) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NS - 2) * (CA + CB)) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        Frag fa[4], fb[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) read_frag(fa[g], 0, g);
        auto mul = [&](Frag (&fc)[4]) __attribute__((always_inline)) {
          if constexpr (X2) {
            X2_PRODUCTS(HG_X2_MM, fc)
          } else {
            mm(swp_c, fc[0], fc[0]); mm(swp_c, fc[1], fc[1]); mm(swp_c, fc[2], fc[2]); mm(swp_c, fc[3], fc[3]);
          }
        };
        // a step with a successor tile (the last tile is peeled off below: a step whose barrier is conditional makes the compiler's
        // waitcnt pass wait for the NEW fragment reads in front of the MFMAs on the path that has them)
        auto step = [&](Frag (&fc)[4], Frag (&fn)[4], int kt) __attribute__((always_inline)) {
          if (kt + NS - 2 < nk) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NS - 3) * (CA + CB)) : "memory");
          else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          __syncthreads();
          if (kt + NS - 1 < nk) { HG_DMA(kt + NS - 1, (kt + NS - 1) & (NS - 1)) }
#pragma unroll
          for (int g = 0; g < 4; ++g) read_frag(fn[g], (kt + 1) & (NS - 1), g);
          mul(fc);
        };
        int kt = 0;
        for (; kt + 2 < nk; kt += 2) {
          step(fa, fb, kt);
          step(fb, fa, kt + 1);
        }
        if (kt + 1 < nk) { step(fa, fb, kt); mul(fb); }
        else mul(fa);
        return;
      }
      for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & (NS - 1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // NS == 2: tile kt is the only one outstanding
        __syncthreads();                    // tile kt visible to every wave; every wave is done with tile kt - 1, whose buffer the next DMA takes
        if (kt + NS - 1 < nk) { HG_DMA(kt + NS - 1, (kt + NS - 1) & (NS - 1)) }
        static_assert(NS > 2 || !X2, "split precision on two stages runs the k_loop below");
        read_frag(f0, cur, 0);
        read_frag(f1, cur, 1);
        HG_FENCE
        mm(swp_c, f0, f0);
        HG_FENCE
        read_frag(f0, cur, 2);
        HG_FENCE
        mm(swp_c, f1, f1);
        HG_FENCE
        read_frag(f1, cur, 3);
        HG_FENCE
        mm(swp_c, f0, f0);
        HG_FENCE
        mm(swp_c, f1, f1);
      }
    };
    if constexpr (EPI == EPI_H_QKV_NORM) {
      if (swp) ring(std::true_type{}); else ring(std::false_type{});
    } else {
      ring(std::false_type{});
    }
    __syncthreads();                        // the operand buffers become the epilogue slabs
  } else if constexpr (X2) {
    auto k_loop = [&](auto swp_c) __attribute__((always_inline)) {
      Frag f[4];
      for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nk) { HG_DMA(kt + 1, cur ^ 1) }     // spare buffer: every wave finished reading it before the last barrier
#pragma unroll
        for (int g = 0; g < 4; ++g) read_frag(f[g], cur, g);
        X2_PRODUCTS(HG_X2_MM, f)
        HG_SYNC
      }
    };
    if constexpr (EPI == EPI_H_QKV_NORM) {
      if (swp) k_loop(std::true_type{}); else k_loop(std::false_type{});
    } else {
      k_loop(std::false_type{});
    }
  } else {
    read_frag(f0, 0, 0);

    int kt = 0;
    for (; kt + 1 < nk; ++kt) {
      const int cur = kt & 1;
      HG_DMA(kt + 1, cur ^ 1)                 // spare buffer: every wave finished reading it before the last barrier
      read_frag(f1, cur, 1);
      HG_FENCE
      mma(f0);
      HG_FENCE
      read_frag(f0, cur, 2);
      HG_FENCE
      mma(f1);
      HG_FENCE
      read_frag(f1, cur, 3);
      HG_FENCE
      mma(f0);
      HG_FENCE
      HG_SYNC                                 // tile kt+1 landed (vmcnt(0)) and visible; reads of tile kt complete
      read_frag(f0, cur ^ 1, 0);
      HG_FENCE
      mma(f1);
      HG_FENCE
    }
    {
      const int cur = kt & 1;
      read_frag(f1, cur, 1);
      HG_FENCE
      mma(f0);
      HG_FENCE
      read_frag(f0, cur, 2);
      HG_FENCE
      mma(f1);
      HG_FENCE
      read_frag(f1, cur, 3);
      HG_FENCE
      mma(f0);
      HG_FENCE
      mma(f1);
    }
    __syncthreads();
  }

  // ---------------- epilogue (the block is synchronised: the operand buffers become the per-wave slabs) ----------------
  static_assert(TN == 2, "wave tiles are 64 columns wide: one head / one GEGLU value+gate group");
  static_assert(WM * WN * H16_STG_BYTES + 1024 <= NS * (BM + BN) * 128, "staging slabs (+ the LN statistics) must fit the operand buffers");
  // Split-K: plane blockIdx.y of the partial buffer takes the place of C.  The rule and the choice stand once; the shapes they are applied
  // in are the ones the compiler has seen so far, because the code it emits follows them: the ring kernels hold ONE copy of their epilogue,
  // on copied parameters whatever EPI is; the two-stage kernels one on p and a second for the planes; and the plain two-stage loop forms
  // the wave tile's slab and origin inside each case, not ahead of the choice (EPI_H_BIAS_RESID_F32, 2 134 lines of assembly: 1 633 move).
#define HG_SPLITK_PLANE (reinterpret_cast<float*>(p.C) + (size_t)blockIdx.y * p.M * p.ldc)
#define HG_EPILOGUE(SLAB, MW, NW)                                                                             \
  if constexpr (RING) {                                                                                       \
    GemmParamsH q = p;                                                                                        \
    if constexpr (EPI == EPI_H_BIAS_RESID_F32) {                                                              \
      if (gridDim.y > 1) q.C = HG_SPLITK_PLANE;                                                               \
    }                                                                                                         \
    H16_EPILOGUE(q, SLAB, MW, NW)                                                                             \
  } else {                                                                                                    \
    if constexpr (EPI == EPI_H_BIAS_RESID_F32) {                                                              \
      if (gridDim.y > 1) {                                                                                    \
        GemmParamsH q = p;                                                                                    \
        q.C = HG_SPLITK_PLANE;                                                                                \
        H16_EPILOGUE(q, SLAB, MW, NW)                                                                         \
        return;                                                                                               \
      }                                                                                                       \
    }                                                                                                         \
    H16_EPILOGUE(p, SLAB, MW, NW)                                                                             \
  }
  if constexpr (RING || X2) {
    unsigned char* slab = smem + wave * H16_STG_BYTES;
    const int mw = m0 + wm * TM * 32, nw = n0 + wn * 64;
    HG_EPILOGUE(slab, mw, nw)
  } else {
    HG_EPILOGUE(smem + wave * H16_STG_BYTES, m0 + wm * TM * 32, n0 + wn * 64)
  }
}

#ifdef RAP_ABLATION_BUILD
// Ablation build only (scripts/gemm_ts.py): s_memrealtime stamps (100 MHz, one counter for the device) of thread 0 of every block of
// the phase-split kernel -- [block][8]: 0 entry, 1 prologue DMA issued, 2 first k-tile landed (first barrier passed), 3 k-loop done,
// 4 epilogue done (stores issued), 5 = (XCC_ID << 16) | HW_ID -- to itemise the per-tile overhead the K = 512 shapes lose to.
__device__ unsigned long long* g_gemm_ts = nullptr;
extern "C" int rap_debug_gemm_ts(void* p) { return hipMemcpyToSymbol(HIP_SYMBOL(g_gemm_ts), &p, sizeof(p)) == hipSuccess ? 0 : -3; }
#define GEMM_TS(I) if (g_gemm_ts && threadIdx.x == 0) { g_gemm_ts[(size_t)blockIdx.x * 8 + (I)] = __builtin_amdgcn_s_memrealtime(); \
    if ((I) == 0) g_gemm_ts[(size_t)blockIdx.x * 8 + 5] = ((unsigned long long)(__builtin_amdgcn_s_getreg((31 << 11) | 20) & 15u) << 16) | (__builtin_amdgcn_s_getreg((31 << 11) | 4) & 0xffffu); }
#else
#define GEMM_TS(I)
#endif
// ---------------------------------------------------------------------------------------------
// Phase-split kernel (r02; rap_set_tuning(2, 13 | 14 | 15)).  r02 calls 2-4 reproduce what the CDNA4 guide says about this
// structure class: every loop with ONE barrier per k-slice in which all eight waves stage, read and multiply in lockstep lands at
// the same 800-870 TF on the K = 2048 shape -- deeper rings (6-8), padded rows (no channel camping), one-piece-at-a-time issue
// (9-12) do not move it.  What is left is the structure itself: the two waves of a SIMD leave every barrier in the same role.
// This kernel splits the k-tile (BK = 64, two 64 KB stages) into four PHASES, one 64 x 32 quadrant of the wave's 128 x 64 tile
// each, every phase = [L: fragment reads (12 / 4 / 8 / 4 ds_read_b128) + two LDS-DMA pieces] barrier [M: 8 MFMAs under s_setprio]
// barrier, and runs wave row 1 one barrier behind wave row 0: in every barrier interval one wave of each SIMD is in its M part
// and its partner in its L part.  DMA is counted (vmcnt(6): three half-tile pairs in flight), never drained in the steady state:
//   phase q of tile t issues   q0: W half g0 of tile t+1,  q1: W half g1 of t+1,  q2: A half h1 of t+1,  q3: A half h0 of tile t+2
// so every piece is issued four phases before the phase that reads it and after the last read of the region it overwrites.
// LDS image of a stage: A as [h][wave row][2 x 32 rows] x 128 B and W as [g][wave column][32 rows] x 128 B (the halves are
// contiguous 16 KB blocks = 2 DMA pieces per thread); the permutation lives in the per-lane GLOBAL source address.
// ---------------------------------------------------------------------------------------------
// What the one-tile kernel and its persistent form below share, as macros over the kernels' own names (tid, smem, STAGE, ABYTES, wr, wc,
// hi, l31, sw, acc, PRIO, X2): as a function with parameters even the piece mapping moved ~40 instructions of every instantiation.
// piece j (0..7) of a stage: LDS chunk id = j * 512 + tid -> LDS row s = id >> 3 (0..255 A, 256..511 W), 16-byte slot id & 7.  Declares
// `row`, the row of the A (j < 4, counted from ROW0_A) or W (j >= 4, from ROW0_W) panel that LDS row holds, and `lslot`, the logical
// (swizzled) slot of the physical one.
#define PH_PIECE_ROW(J, ROW0_A, ROW0_W)                                                                       \
  const int id = (J) * 512 + tid;                                                                             \
  const int s = (id >> 3) & 255;                                                                              \
  const int lslot = (id & 7) ^ ((s >> 1) & 7);                                                                \
  const int row = (J) < 4 ? ROW0_A + ((s >> 6) & 1) * 128 + (s >> 7) * 64 + (s & 63)  /* [h][wr][64 rows] -> wr*128 + h*64 + row */ \
                          : ROW0_W + ((s >> 5) & 3) * 64 + (s >> 7) * 32 + (s & 31);  /* [g][wc][32 rows] -> wc*64 + g*32 + row */
// operand fragments of a phase: the A rows of half h (two row tiles), the W rows of half g; four k-steps each
#define PH_FRAGMENTS                                                                                          \
  uint4 fa[2][4], fb0[4], fb1[4];                                                                             \
  auto read_a = [&](int buf, int h) {                                                                         \
    _Pragma("unroll") for (int ii = 0; ii < 2; ++ii)                                                          \
      _Pragma("unroll") for (int ks = 0; ks < 4; ++ks)                                                        \
        fa[ii][ks] = *reinterpret_cast<const uint4*>(smem + buf * STAGE + (h * 128 + wr * 64 + ii * 32 + l31) * 128 + (((2 * ks + hi) ^ sw) * 16)); \
  };                                                                                                          \
  auto read_b = [&](uint4 (&fb)[4], int buf, int g) {                                                         \
    _Pragma("unroll") for (int ks = 0; ks < 4; ++ks)                                                          \
      fb[ks] = *reinterpret_cast<const uint4*>(smem + buf * STAGE + ABYTES + (g * 128 + wc * 32 + l31) * 128 + (((2 * ks + hi) ^ sw) * 16)); \
  };
// fragment pair (ka of A, kb of W) into quadrant (H, G), the two row tiles alternating; SWP: the swapped product C^T = W A^T
#define PH_MMA1(SWP, H, G, FB, KA, KB)                                                                        \
  if constexpr (SWP) {                                                                                        \
    acc[2 * (H)][G] = H16<DT>::mfma(__builtin_bit_cast(T8, FB[KB]), __builtin_bit_cast(T8, fa[0][KA]), acc[2 * (H)][G]);           \
    acc[2 * (H) + 1][G] = H16<DT>::mfma(__builtin_bit_cast(T8, FB[KB]), __builtin_bit_cast(T8, fa[1][KA]), acc[2 * (H) + 1][G]);   \
  } else {                                                                                                    \
    acc[2 * (H)][G] = H16<DT>::mfma(__builtin_bit_cast(T8, fa[0][KA]), __builtin_bit_cast(T8, FB[KB]), acc[2 * (H)][G]);           \
    acc[2 * (H) + 1][G] = H16<DT>::mfma(__builtin_bit_cast(T8, fa[1][KA]), __builtin_bit_cast(T8, FB[KB]), acc[2 * (H) + 1][G]);   \
  }
// the M part of a phase: 8 MFMAs (the four k-steps), 12 in split precision, under s_setprio where PRIO is set
#define PH_MMA(SWP, H, G, FB)                                                                                 \
  __builtin_amdgcn_sched_barrier(0);                                                                          \
  if (PRIO) __builtin_amdgcn_s_setprio(1);                                                                    \
  if constexpr (X2) {                                                                                         \
    X2_PRODUCTS(PH_MMA1, SWP, H, G, FB)                                                                       \
  } else {                                                                                                    \
    _Pragma("unroll") for (int ks = 0; ks < 4; ++ks) { PH_MMA1(SWP, H, G, FB, ks, ks) }                       \
  }                                                                                                           \
  if (PRIO) __builtin_amdgcn_s_setprio(0);                                                                    \
  __builtin_amdgcn_sched_barrier(0);
#define PH_BAR __builtin_amdgcn_sched_barrier(0); __builtin_amdgcn_s_barrier(); __builtin_amdgcn_sched_barrier(0);
#define PH_VM(N) asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory");
// X2 (round 5): the split-precision product on paired operands (half.h RAP_DT_F32X2; DT = fp16).  A 128-byte line of a stage is 32 heads
// followed by 32 tails of one 32-column chunk, so the fragments of "k-steps" 0, 1 are head fragments and those of 2, 3 the tail
// fragments of the same 32 logical columns; a phase multiplies head x head, head x tail and tail x head into the one accumulator:
// 12 MFMAs instead of 8 on the same fragment reads and LDS-DMA pieces (1.5 x the MFMA work per staged byte of the plain kernel).
template <int EPI, int DT, int PRIO, int STAG, bool X2 = false>
__global__ __launch_bounds__(512, 2) void gemm_h16_ph_kernel(GemmParamsH p) {
  typedef typename H16<DT>::T8 T8;
  constexpr int TM = 4;
  constexpr int ABYTES = 256 * 128, STAGE = 2 * ABYTES;
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];   // [stage 0: A B][stage 1: A B]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5;
  const int l31 = lane & 31;
  const int wr = wave >> 2, wc = wave & 3;

  GEMM_TS(0)
  const int nt = p.N / 256;
  const int mt = (p.M + 255) / 256;
  const int logical = xcd_remap(blockIdx.x, mt * nt);
  const int m0 = (logical / nt) * 256;
  const int n0 = (logical % nt) * 256;

  const u16* src[8];      // the pieces' sources at k = 0, rows clamped to M
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    PH_PIECE_ROW(j, m0, n0)
    if (j < 4) src[j] = p.A + (size_t)(row < p.M ? row : p.M - 1) * p.lda + 8 * lslot;
    else src[j] = p.W + (size_t)row * p.ldw + 8 * lslot;
  }

  f32x16 acc[TM][2];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int nk = p.K / 64;
  const int sw = (l31 >> 1) & 7;
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
  const unsigned lds_wave = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)wave * 1024u);
#define PH_PIECE(J, KT, BUF) LDS_DMA_X4(src[J] + (size_t)(KT) * 64, lds_wave + (unsigned)((BUF) * STAGE + (J) * 8192))
  PH_FRAGMENTS
  // EPI_H_QKV_NORM: the q and k column tiles run the SWAPPED product C^T = W A^T (the MFMA's A operand is the weight fragment): a lane
  // then owns one token row and 16 of every 32 columns, so the row norm of a head is lane-local up to one lane^32 exchange and the
  // 16-bit results leave as 16-byte row pieces without an LDS transpose.  The v tiles keep the normal order (the V^T image wants a
  // lane to own a column).  Wave-uniform choice: a 64-column wave tile is one head of q, k or v.
  const bool swp = EPI == EPI_H_QKV_NORM && (n0 + wc * 64) < 2 * p.heads * 64;
  // SWP is a compile-time property of the k-loop COPY that runs (round 4, as in the persistent kernel below): as a run-time flag inside
  // the phases the accumulators of the two alternatives are reconciled with register copies at every phase and the kernel spilled
  // (44 bytes of scratch in the <EPI_H_QKV_NORM> instantiations).

  // prologue: tile 0 completely, plus the A half h0 of tile 1 (what phase q3 of "tile -1" would have issued)
#pragma unroll
  for (int j = 0; j < 8; ++j) PH_PIECE(j, 0, 0)
  GEMM_TS(1)
  if (nk > 1) { PH_PIECE(0, 1, 1) PH_PIECE(1, 1, 1) PH_VM(2) } else { PH_VM(0) }
  PH_BAR
  GEMM_TS(2)
  if (STAG && wr == 1) { PH_BAR }          // wave row 1 runs one barrier behind

  auto k_tiles = [&](auto swp_c) __attribute__((always_inline)) {
    constexpr bool SWP = decltype(swp_c)::value;
    for (int t = 0; t < nk; ++t) {
      const int buf = t & 1;
      const bool last = t == nk - 1, pen = t == nk - 2;
      // ---- q0: quadrant (h0, g0)
      read_a(buf, 0); read_b(fb0, buf, 0);
      __builtin_amdgcn_sched_barrier(0);
      if (!last) { PH_PIECE(4, t + 1, buf ^ 1) PH_PIECE(5, t + 1, buf ^ 1) PH_VM(6) } else { PH_VM(2) }
      PH_BAR
      PH_MMA(SWP, 0, 0, fb0)
      PH_BAR
      // ---- q1: quadrant (h0, g1)
      read_b(fb1, buf, 1);
      __builtin_amdgcn_sched_barrier(0);
      if (!last) { PH_PIECE(6, t + 1, buf ^ 1) PH_PIECE(7, t + 1, buf ^ 1) PH_VM(6) } else { PH_VM(0) }
      PH_BAR
      PH_MMA(SWP, 0, 1, fb1)
      PH_BAR
      // ---- q2: quadrant (h1, g1)
      read_a(buf, 1);
      __builtin_amdgcn_sched_barrier(0);
      if (!last) { PH_PIECE(2, t + 1, buf ^ 1) PH_PIECE(3, t + 1, buf ^ 1) PH_VM(6) }
      PH_BAR
      PH_MMA(SWP, 1, 1, fb1)
      PH_BAR
      // ---- q3: quadrant (h1, g0)
      read_b(fb0, buf, 0);
      __builtin_amdgcn_sched_barrier(0);
      if (!last && !pen) { PH_PIECE(0, t + 2, buf) PH_PIECE(1, t + 2, buf) PH_VM(6) } else if (pen) { PH_VM(4) }
      PH_BAR
      PH_MMA(SWP, 1, 0, fb0)
      PH_BAR
    }
  };
  if constexpr (EPI == EPI_H_QKV_NORM) {
    if (swp) k_tiles(std::true_type{}); else k_tiles(std::false_type{});
  } else {
    k_tiles(std::false_type{});
  }
  GEMM_TS(3)
  if (STAG && wr == 0) { PH_BAR }          // equal barrier counts for both wave rows
  static_assert(8 * H16_STG_BYTES <= 2 * STAGE, "staging slabs must fit the operand buffers");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  H16_EPILOGUE(p, smem + wave * H16_STG_BYTES, m0 + wr * 128, n0 + wc * 64)
  GEMM_TS(4)
}

template <int EPI, int DT, int PRIO, int STAG, bool X2 = false>
static int launch_ph(hipStream_t stream, const GemmParamsH& p) {
  return rap_launch_dyn_lds(gemm_h16_ph_kernel<EPI, DT, PRIO, STAG, X2>, dim3(((p.M + 255) / 256) * (p.N / 256)), dim3(512), 4 * 256 * 128, stream, p);
}

// ---------------------------------------------------------------------------------------------
// Persistent form of the phase-split kernel (round 3).  scripts/gemm_ts.py (s_memrealtime stamps, r03 call 8) itemises a 256 x 256
// tile of the K = 512 shapes on the kernel above: 2.0-2.8 us from block entry to the first DMA (kernel arguments, tile decode,
// eight 64-bit source addresses, wave start-up), 1.0-1.2 us until the first k-tile has landed, 14-16 us of k-loop (8 k-tiles at
// ~52 % of the MFMA peak), 3.5-4.4 us of epilogue, ~1.8 us between a block's last store and the next block's entry: 9-10 us of
// every 25 us round are not k-loop.  Here ONE block per CU walks the tiles of its XCD (virtual block id v = blockIdx.x + i *
// gridDim.x, gridDim.x a multiple of 8: xcd_remap keeps its meaning) and treats the k-tiles of consecutive output tiles as ONE
// stream: the phases of an output tile's last k-tile request the FIRST k-tile of the next output tile exactly as they would request
// the next k-tile of their own, so the next k-loop starts on data that has landed, without a launch, an argument load or a prologue,
// and the epilogue's stores drain under it.  Differences from the kernel above:
//  * sources are a scalar base (tile origin + k offset, SGPRs) plus one 32-bit per-thread byte offset per piece (the saddr form of
//    global_load_lds): 8 VGPRs instead of 16, nothing to recompute at a tile switch but two scalar pointers; needs M % 256 == 0
//    (no row clamping);
//  * the epilogue's per-wave transposition slabs live where no DMA is in flight: the 48 KB behind the A half h0 of the stage that
//    was read last (that 16 KB is already receiving the k-tile after next) and 32 KB beyond the two stages (160 KB of LDS in all);
//  * vmcnt is in-order over loads AND stores, so a counted wait after an epilogue would also wait for its stores: everything
//    the first k-tile of the next output tile reads is therefore confirmed BEFORE the epilogue (vmcnt(2): all but the two pieces of
//    the k-tile after next), its phases q0-q2 wait for nothing, and q3's usual vmcnt(6) is the first point the stores must have drained.
// Measured (r03 calls 12-14, TP = 262 144 rows, bf16): qkv + qk-norm 0.653 -> 0.566 ms, out-projection 0.215 -> 0.192, ff1 + GEGLU 1.353 ->
// 1.204, ff2 0.550 -> 0.528; the layer GEMMs of a sampling call 829 -> 689 ms (796 -> 957 TF); results BIT-identical to the kernel above for
// every epilogue (tests/test_h16_gpu.py).  Stamps of the persistent kernel: tile period 18-21 us = 13.5-15 us of k-loop + 3.6-4.4 us of
// epilogue (7.4 with the residual's HBM latency; GEGLU is VALU-bound: the younger wave of each SIMD finishes 2.5 us after the older) +
// 0.5-0.8 us of turn-around.  Starting every other block half a period late (so that the CUs do not store in lockstep) changes nothing (+-1 %).
// ---------------------------------------------------------------------------------------------
template <int EPI, int DT, bool X2 = false>
__global__ __launch_bounds__(512, 2) void gemm_h16_php_kernel(GemmParamsH p) {
  typedef typename H16<DT>::T8 T8;
  constexpr int TM = 4;
  constexpr int PRIO = 0;      // (PH_MMA: no s_setprio in the M parts here)
  constexpr int ABYTES = 256 * 128, STAGE = 2 * ABYTES;
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];   // [stage 0: A B][stage 1: A B][32 KB of epilogue slabs]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5;
  const int l31 = lane & 31;
  const int wr = wave >> 2, wc = wave & 3;

  const int nt = p.N / 256;
  const int total = (p.M / 256) * nt;
  const int nk = p.K / 64;

  // voff[j] = byte offset of piece j's source inside the tile's A (j < 4) or W (j >= 4) panel at k = 0
  unsigned voff[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    PH_PIECE_ROW(j, 0, 0)
    if (j < 4) voff[j] = (unsigned)(row * p.lda + 8 * lslot) * 2u;
    else voff[j] = (unsigned)(row * p.ldw + 8 * lslot) * 2u;
  }

  f32x16 acc[TM][2];
  const int sw = (l31 >> 1) & 7;
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
  const unsigned lds_wave = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)wave * 1024u);
  // one LDS-DMA piece: scalar base (64-bit, SGPRs) + per-thread 32-bit offset; m0 carries the wave-uniform LDS byte address
#define PHP_PIECE(J, SBASE, BUF) LDS_DMA_X4_SADDR(voff[J], SBASE, lds_wave + (unsigned)((BUF) * STAGE + (J) * 8192))
  PH_FRAGMENTS
  // SWP (EPI_H_QKV_NORM, q and k column tiles): the swapped product C^T = W A^T, see the kernel above.  A compile-time property of the
  // k-loop COPY that runs (chosen per output tile): as a run-time flag inside the phases it cost 2x (r03 call 10: the accumulators of
  // the two alternatives are reconciled with register copies at every phase).

  // scalar source bases of an output tile (virtual block id v): A panel rows m0.., W panel rows n0.., at k = 0
  auto tile_bases = [&](int v, const unsigned char*& ab, const unsigned char*& wb, int& m0, int& n0) {
    const int logical = xcd_remap(v, total);
    m0 = (logical / nt) * 256;
    n0 = (logical % nt) * 256;
    ab = reinterpret_cast<const unsigned char*>(p.A) + (size_t)m0 * p.lda * 2;
    wb = reinterpret_cast<const unsigned char*>(p.W) + (size_t)n0 * p.ldw * 2;
  };

  int v = blockIdx.x;
  const unsigned char *a_cur, *w_cur, *a_nxt = nullptr, *w_nxt = nullptr;
  int m0, n0, m0n = 0, n0n = 0;
  tile_bases(v, a_cur, w_cur, m0, n0);

  // prologue of the block: the first k-tile completely, plus the A half h0 of the second (what phase q3 of "k-tile -1" would have issued)
#pragma unroll
  for (int j = 0; j < 4; ++j) PHP_PIECE(j, a_cur, 0)
#pragma unroll
  for (int j = 4; j < 8; ++j) PHP_PIECE(j, w_cur, 0)
  PHP_PIECE(0, a_cur + 128, 1) PHP_PIECE(1, a_cur + 128, 1)            // nk >= 2 (the launcher checks K >= 128)
  PH_VM(2)
  PH_BAR
  int par = 0;                                   // stage that holds the current k-tile of the stream
  bool first_tile = true;
#ifdef RAP_ABLATION_BUILD
  int ts_it = 0;                                 // [block][tile][4] stamps: 0 k-loop start, 1 k-loop end, 2 epilogue end (stores issued), 3 XCC/HW id
#define PHP_TS(I) if (g_gemm_ts && threadIdx.x == 0 && ts_it < 32) { g_gemm_ts[((size_t)blockIdx.x * 32 + ts_it) * 4 + (I)] = __builtin_amdgcn_s_memrealtime(); }
#else
#define PHP_TS(I)
#endif

  for (;;) {
    const int vn = v + (int)gridDim.x;
    const bool has_next = vn < total;
    if (has_next) tile_bases(vn, a_nxt, w_nxt, m0n, n0n);
    const bool swp = EPI == EPI_H_QKV_NORM && (n0 + wc * 64) < 2 * p.heads * 64;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    PHP_TS(0)
    if (wr == 1) { PH_BAR }                      // wave row 1 runs one barrier behind

    auto k_tiles = [&](auto swp_c) __attribute__((always_inline)) {
      constexpr bool SWP = decltype(swp_c)::value;
      for (int t = 0; t < nk; ++t) {
        const int buf = par;
        // stream successors: k-tile t + 1 / t + 2 of this output tile, or k-tile 0 / 1 of the next one
        const bool in1 = t + 1 < nk, in2 = t + 2 < nk;
        const bool ok1 = in1 || has_next, ok2 = in2 || has_next;
        const unsigned char* a1 = in1 ? a_cur + (size_t)(t + 1) * 128 : a_nxt;
        const unsigned char* w1 = in1 ? w_cur + (size_t)(t + 1) * 128 : w_nxt;
        const unsigned char* a2 = in2 ? a_cur + (size_t)(t + 2) * 128 : a_nxt + (size_t)(t + 2 - nk) * 128;
        // the first k-tile after an epilogue: everything it reads was confirmed before the epilogue; a counted wait here would wait
        // for the epilogue's stores (vmcnt is in-order over loads and stores)
        const bool nowait = t == 0 && !first_tile;
        // ---- q0: quadrant (h0, g0)
        read_a(buf, 0); read_b(fb0, buf, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (ok1) { PHP_PIECE(4, w1, buf ^ 1) PHP_PIECE(5, w1, buf ^ 1) if (!nowait) { PH_VM(6) } } else { PH_VM(2) }
        PH_BAR
        PH_MMA(SWP, 0, 0, fb0)
        PH_BAR
        // ---- q1: quadrant (h0, g1)
        read_b(fb1, buf, 1);
        __builtin_amdgcn_sched_barrier(0);
        if (ok1) { PHP_PIECE(6, w1, buf ^ 1) PHP_PIECE(7, w1, buf ^ 1) if (!nowait) { PH_VM(6) } } else { PH_VM(0) }
        PH_BAR
        PH_MMA(SWP, 0, 1, fb1)
        PH_BAR
        // ---- q2: quadrant (h1, g1)
        read_a(buf, 1);
        __builtin_amdgcn_sched_barrier(0);
        if (ok1) { PHP_PIECE(2, a1, buf ^ 1) PHP_PIECE(3, a1, buf ^ 1) if (!nowait) { PH_VM(6) } }
        PH_BAR
        PH_MMA(SWP, 1, 1, fb1)
        PH_BAR
        // ---- q3: quadrant (h1, g0)
        read_b(fb0, buf, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (ok2) { PHP_PIECE(0, a2, buf) PHP_PIECE(1, a2, buf) PH_VM(6) } else if (ok1) { PH_VM(4) }
        PH_BAR
        PH_MMA(SWP, 1, 0, fb0)
        PH_BAR
        par ^= 1;
      }
    };
    if constexpr (EPI == EPI_H_QKV_NORM) {
      if (swp) k_tiles(std::true_type{}); else k_tiles(std::false_type{});
    } else {
      k_tiles(std::false_type{});
    }
    PHP_TS(1)
    if (wr == 0) { PH_BAR }                      // equal barrier counts for both wave rows
    // Everything the next output tile's first k-tile reads has been requested during the last k-tile: confirm it NOW (all but the
    // two pieces of the k-tile after next, issued in q3), then publish with the barrier that also says "every wave has read the last stage".
    if (has_next) { PH_VM(2) } else { PH_VM(0) }
    PH_BAR
    {
      const int last = par ^ 1;                  // the stage the last k-tile was read from: its bytes [16 KB, 64 KB) are idle
      unsigned char* slab = wave < 5 ? smem + last * STAGE + 16384 + wave * H16_STG_BYTES : smem + 2 * STAGE + (wave - 5) * H16_STG_BYTES;
      static_assert(5 * H16_STG_BYTES <= STAGE - 16384 && 3 * H16_STG_BYTES <= 32768, "epilogue slabs must fit the idle regions");
      H16_EPILOGUE(p, slab, m0 + wr * 128, n0 + wc * 64)
    }
    PHP_TS(2)
#ifdef RAP_ABLATION_BUILD
    ++ts_it;
#endif
    if (!has_next) break;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    PH_BAR                                       // every wave has drained its slab: the next k-loop's DMA may overwrite the region
    v = vn; a_cur = a_nxt; w_cur = w_nxt; m0 = m0n; n0 = n0n;
    first_tile = false;
  }
}

template <int EPI, int DT, bool X2 = false>
static int launch_php(hipStream_t stream, const GemmParamsH& p) {
  const int blocks = rap_persistent_blocks((p.M / 256) * (p.N / 256));
  if (blocks <= 0) return RAP_ERR_HIP;
  return rap_launch_dyn_lds(gemm_h16_php_kernel<EPI, DT, X2>, dim3(blocks), dim3(512), 4 * 256 * 128 + 32768, stream, p);
}

// Kernel choice (round 3: the fifteen other main loops of rounds 1-2 -- rings, pipelined rings, interleaved issue, persistent,
// 128 x 512 -- all measured within +-4 % of this one and are gone from the tree; their source and numbers are in the history at
// 72efb73 and in docs/DESIGN_r01_r02.md section 4.3).  Default: the phase-split 256 x 256 kernel, persistent where the shape allows.
// Fallback for shapes it cannot tile (N % 256 != 0 or K < 128) and for calls with fewer 256 x 256 tiles than CUs: the two-stage
// 128 x 128 kernel, two blocks per CU.
// RAP_ABLATION_BUILD only: rap_set_tuning(2, 0) forces the 128 x 128 kernel, (2, 1) the two-stage 256 x 256 kernel.
rap_tuning_t g_rap_gemm_h16_variant = 14;
rap_tuning_t g_rap_gemm_h16_persistent = 1;     // tuning key 11: the persistent phase-split kernel for full-tile shapes (1, default) or one tile per block (0)

template <int EPI, int DT, int WM, int WN, int TM, int TN, bool X2 = false, int NS = 2>
static int launch_cfg(hipStream_t stream, const GemmParamsH& p, int splits = 1) {
  constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
  const int mt = (EPI == EPI_H_QKV_NORM || EPI == EPI_H_QKV) ? ((p.M + 255) / 256) * (256 / BM) : (p.M + BM - 1) / BM;
  return rap_launch_dyn_lds(gemm_h16_kernel<EPI, DT, WM, WN, TM, TN, X2, NS>, dim3(mt * (p.N / BN), splits), dim3(64 * WM * WN), NS * (BM + BN) * 128,
                            stream, p);
}

// The 128 x 128 kernel for few-token calls (round 6): a launch with at most g_rap_ring_blocks blocks (tuning key 18; 0 = never) takes the
// four-stage ring, one block per CU; larger launches keep two stages and two blocks per CU, whose second block is what hides the latency.
// (FIVE stages -- all 160 KB, three tiles in flight beside the fragment prefetch -- were measured for split precision in r06 call 14 and are
// not kept: residual GEMMs 14.5 vs 13.9 us, QKV 21.0 vs 20.4, 25.2 vs 24.9 ms per demo-pair call; profiles/r06_c14_x2_ring_five_stages_*.
// The ~1 us per split-precision k-tile that remains is not the L2 round trip.)
rap_tuning_t g_rap_ring_blocks = 256;
static int small_stages(const GemmParamsH& p, int splits) {
  const long blocks = (long)((p.M + 127) / 128) * (p.N / 128) * splits;
  return blocks <= (long)g_rap_ring_blocks ? 4 : 2;
}
template <int EPI, int DT, bool X2 = false>
static int launch_small(hipStream_t stream, const GemmParamsH& p, int stages, int splits = 1) {
  if (stages == 4) return launch_cfg<EPI, DT, 2, 2, 2, 2, X2, 4>(stream, p, splits);
  return launch_cfg<EPI, DT, 2, 2, 2, 2, X2, 2>(stream, p, splits);
}

// ---------------------------------------------------------------------------------------------
// Split-K for the residual GEMMs of few-token calls (round 3).  ff2 of one pair of 2 x 1024 points is M = 2048, N = 512, K = 2048:
// 64 tiles of 128 x 128 on 256 CUs, each a serial chain of 32 k-tiles with one tile of prefetch -- 33 us, latency-bound (r03 call 33: the
// K = 512 out-projection of the same call takes 8.8 us).  Four blocks per tile take a quarter of the k-tiles each and write fp32 partial
// tiles; the combine pass adds them in a fixed order, then bias, then the residual, and rounds once (fp16 stream) -- the unsplit
// epilogue's order of operations with the k-sum re-associated.
// ---------------------------------------------------------------------------------------------
template <bool H16OUT>
__global__ __launch_bounds__(256) void gemm_h16_splitk_combine_kernel(const float* __restrict__ part, int splits, int M, int N,
                                                                      const float* __restrict__ bias, const void* __restrict__ resid, int ldr,
                                                                      void* __restrict__ C, int ldc) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;      // one thread per 8 consecutive columns
  const int n8 = N / 8;
  if (i >= (long)M * n8) return;
  const int m = (int)(i / n8), c = (int)(i % n8) * 8;
  float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < splits; ++s) {
    const float4 a0 = *reinterpret_cast<const float4*>(part + ((size_t)s * M + m) * N + c);
    const float4 a1 = *reinterpret_cast<const float4*>(part + ((size_t)s * M + m) * N + c + 4);
    v[0] += a0.x; v[1] += a0.y; v[2] += a0.z; v[3] += a0.w; v[4] += a1.x; v[5] += a1.y; v[6] += a1.z; v[7] += a1.w;
  }
  if (bias) {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] += bias[c + e];
  }
  if constexpr (H16OUT) {
    float rv[8];
    h16_unpack8<RAP_DT_F16>(*reinterpret_cast<const uint4*>(reinterpret_cast<const u16*>(resid) + (size_t)m * ldr + c), rv);
    const typename H16<RAP_DT_F16>::T8 o8 = f16_pack8_sat(v[0] + rv[0], v[1] + rv[1], v[2] + rv[2], v[3] + rv[3], v[4] + rv[4],
                                                         v[5] + rv[5], v[6] + rv[6], v[7] + rv[7]);
    *reinterpret_cast<uint4*>(reinterpret_cast<u16*>(C) + (size_t)m * ldc + c) = __builtin_bit_cast(uint4, o8);
  } else {
    float* out = reinterpret_cast<float*>(C) + (size_t)m * ldc + c;
    if (resid) {
      const float* r = reinterpret_cast<const float*>(resid) + (size_t)m * ldr + c;
      const float4 r0 = *reinterpret_cast<const float4*>(r), r1 = *reinterpret_cast<const float4*>(r + 4);
      v[0] += r0.x; v[1] += r0.y; v[2] += r0.z; v[3] += r0.w; v[4] += r1.x; v[5] += r1.y; v[6] += r1.z; v[7] += r1.w;
    }
    *reinterpret_cast<float4*>(out) = float4{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<float4*>(out + 4) = float4{v[4], v[5], v[6], v[7]};
  }
}

extern rap_tuning_t g_rap_gemm_splitk;      // gemm_f32.hip, tuning key 6: split K for few-row calls (fp32 GEMMs and these)
int gemm_h16_splits_by_shape(int M, int N, int K) {
  if (M <= 0 || N % 128 != 0 || K < 1024 || (K / 64) % 4 != 0) return 1;
  const long tiles = (long)((M + 127) / 128) * (N / 128);
  return tiles <= 64 ? 4 : tiles <= 128 ? 2 : 1;
}
int gemm_h16_splits(int M, int N, int K) { return g_rap_gemm_splitk ? gemm_h16_splits_by_shape(M, N, K) : 1; }

template <int DT, bool X2 = false>
static int launch_splitk(hipStream_t stream, int epilogue, const GemmParamsH& p, int stages, int splits) {
  GemmParamsH q = p;      // (acc_scale stays: the split-precision partials are in true units)
  q.C = p.splitk_ws; q.ldc = p.N; q.bias = nullptr; q.resid = nullptr; q.resid_h = nullptr; q.splitk_ws = nullptr;
  if (int rc = launch_small<EPI_H_BIAS_RESID_F32, DT, X2>(stream, q, stages, splits)) return rc;
  if (p.defer_combine) return RAP_OK;      // the caller's combine + LayerNorm pass consumes the planes (launch_resid_combine_ln_h16)
  const long n8 = (long)p.M * (p.N / 8);
  const dim3 grid((unsigned)((n8 + 255) / 256));
  if (epilogue == EPI_H_BIAS_RESID_H16)
    hipLaunchKernelGGL(gemm_h16_splitk_combine_kernel<true>, grid, dim3(256), 0, stream, p.splitk_ws, splits, p.M, p.N, p.bias,
                       (const void*)p.resid_h, p.ldr, p.C, p.ldc);
  else
    hipLaunchKernelGGL(gemm_h16_splitk_combine_kernel<false>, grid, dim3(256), 0, stream, p.splitk_ws, splits, p.M, p.N, p.bias,
                       (const void*)p.resid, p.ldr, p.C, p.ldc);
  RAP_LAUNCH_CHECK();
  return RAP_OK;
}

// The persistent kernel pays where the per-tile overhead is a large share of a tile: K <= 2048 (<= 32 k-tiles per output tile) and at least
// two tiles per CU.  With long tiles a STATIC tile walk loses more to imbalance than it saves: 8192^3 (128 k-tiles, 4 tiles per block) runs at
// 1 129 TF persistent vs 1 221 one tile per block, while K = 512 gains 21-23 % and K = 2048 8.5 % (scripts/gemm_square.py, r03 call 23).
// Rows of a 256-row tile are addressed by a 32-bit byte offset from the tile's scalar base.
static bool use_persistent(const GemmParamsH& p) {
  return g_rap_gemm_h16_persistent && p.M % 256 == 0 && p.N % 256 == 0 && p.K >= 128 && p.K <= 2048 && (long)(p.M / 256) * (p.N / 256) >= 512 &&
         p.lda <= (1 << 20) && p.ldw <= (1 << 20);
}
// Split precision (RAP_DT_F32X2): p.K, lda, ldw (and ldc of the GEGLU output) are PHYSICAL fp16 counts = 2 x the logical ones; p.N and the fp32
// outputs are logical.  The three epilogues of the model path on the phase-split kernels (persistent where the shape allows); any M
// (rows are clamped by the one-tile kernel), N % 256 == 0, K_physical >= 128.
static bool use_persistent_x2(const GemmParamsH& p) {
  return g_rap_gemm_h16_persistent && p.M % 256 == 0 && p.K <= 8192 && (long)(p.M / 256) * (p.N / 256) >= 512 && p.lda <= (1 << 20) && p.ldw <= (1 << 20);
}
// Few-token calls.  Fewer 256 x 256 tiles than CUs: 128 x 128 tiles (two blocks per CU) fill the chip up to four times better -- one pair of
// 2 x 1024 points x 10 steps 26.6 -> 21.6 ms in bf16, 2 x 4096 x 20 steps 102.5 -> 94.0 ms, unchanged from 4 pairs up (r03 call 31); in split
// precision the N = 512 residual GEMMs below ~32 k tokens (64 tiles at 8 000 tokens), the QKV projection and ff1 below ~10 k / ~4 k.  The
// long-K residual GEMM (ff2) of a call with at most 128 such tiles is a latency-bound chain per block: K is split over 2 / 4 blocks per tile
// that write fp32 partial tiles (scaled, in split precision), and the combine pass forms residual + (bias + partials) in a fixed order
// (gemm_h16_splits_by_shape, on the physical K in split precision; tuning key 6).
static bool few_tiles(const GemmParamsH& p) { return (long)((p.M + 255) / 256) * (p.N / 256) < 256; }

// The dispatch decision as host arithmetic (kernels.h: the form codes).  launch_gemm_h16 switches on the result;
// tests/test_gemm_cases_host.py pins it through rap_gemm_h16_form.
static int form_small(const GemmParamsH& p, int splits) { return rap_gemm_form(RAP_FORM_128, small_stages(p, splits), splits); }
int gemm_h16_form(int dtype, int epilogue, const GemmParamsH& p, bool* planes_to_ws) {
  if (planes_to_ws) *planes_to_ws = false;
  if (p.M <= 0) return 0;
  if (p.N % 128 != 0 || p.K % 64 != 0 || p.K <= 0) return RAP_ERR_INVALID;      // K % 64: two 32-wide ring slices / one 64-wide tile
  if ((p.lda & 7) || (p.ldw & 7) || p.lda < p.K || p.ldw < p.K) return RAP_ERR_INVALID;
  const bool x2 = dtype == RAP_DT_F32X2;
  if (!x2 && dtype != RAP_DT_BF16 && dtype != RAP_DT_F16) return RAP_ERR_INVALID;
  if (x2) {
    if (p.N % 256 != 0 || p.K < 128) return RAP_ERR_INVALID;
    if (epilogue != EPI_H_BIAS_RESID_F32 && epilogue != EPI_H_GEGLU && epilogue != EPI_H_QKV_NORM) return RAP_ERR_INVALID;
  } else if (epilogue != EPI_H_BIAS && epilogue != EPI_H_BIAS_RESID_F32 && epilogue != EPI_H_BIAS_RESID_H16 && epilogue != EPI_H_GEGLU &&
             epilogue != EPI_H_QKV && epilogue != EPI_H_QKV_NORM) {
    return RAP_ERR_INVALID;
  }
  if (!x2 && epilogue == EPI_H_QKV_NORM && p.K < 128) return RAP_ERR_INVALID;
  // split K (and the partial planes left for the caller's combine + LayerNorm pass: one plane when there is no split)
  if ((epilogue == EPI_H_BIAS_RESID_F32 || epilogue == EPI_H_BIAS_RESID_H16) && p.splitk_ws) {
    const int splits = p.force_splits > 0 ? p.force_splits : gemm_h16_splits(p.M, p.N, p.K);
    if (splits < 1 || (p.K / 64) % splits != 0) return RAP_ERR_INVALID;
    if (splits > 1 || p.defer_combine) {
      if (planes_to_ws) *planes_to_ws = true;
      return form_small(p, splits);
    }
  }
  if (x2) {
    if (few_tiles(p)) return form_small(p, 1);
    return rap_gemm_form(use_persistent_x2(p) ? RAP_FORM_256P : RAP_FORM_256, 0, 1);
  }
  const bool big = p.N % 256 == 0 && p.K >= 128;
#ifdef RAP_ABLATION_BUILD
  if (epilogue != EPI_H_QKV_NORM) {
    if (g_rap_gemm_h16_variant == 0) return rap_gemm_form(RAP_FORM_128, 2, 1);
    if (g_rap_gemm_h16_variant == 1 && big) return rap_gemm_form(RAP_FORM_256_2S, 2, 1);
  }
#endif
  // persistent form when every row tile is full and there are at least two rounds of tiles for a 256-CU part; the one-tile-per-block
  // form for ragged M (it clamps rows); 128 x 128 tiles for shapes the phase-split kernel cannot tile (N % 256 != 0 or K < 128) and few tiles
  // (the fused qk-norm exists on 128 x 128 tiles since round 6; the r03 note in api.hip: GEMM + qk-norm as two kernels used to win there
  // because the fused form existed only in the 256 x 256 kernels)
  if (big && use_persistent(p)) return rap_gemm_form(RAP_FORM_256P, 0, 1);
  if (big && !few_tiles(p)) return rap_gemm_form(RAP_FORM_256, 0, 1);
  return form_small(p, 1);
}

template <int EPI, int DT, bool X2 = false>
static int launch_form(hipStream_t stream, const GemmParamsH& p, int form) {
  switch (rap_form_kernel(form)) {
    case RAP_FORM_256P: return launch_php<EPI, DT, X2>(stream, p);
    case RAP_FORM_256: return launch_ph<EPI, DT, 0, 1, X2>(stream, p);
    case RAP_FORM_128: return launch_small<EPI, DT, X2>(stream, p, rap_form_stages(form));
#ifdef RAP_ABLATION_BUILD
    case RAP_FORM_256_2S:
      if constexpr (!X2 && EPI != EPI_H_QKV_NORM) return launch_cfg<EPI, DT, 2, 4, 4, 2>(stream, p);
      return RAP_ERR_INVALID;
#endif
    default: return RAP_ERR_INVALID;
  }
}

// The fused QKV projections: N is three model widths and the V^T image is given and covers align_up(M, 256) token rows.  The q / k gains
// are the caller's rule: 16-bit EPI_H_QKV_NORM needs both, split precision both or neither (none = no qk-norm), EPI_H_QKV reads none.
static bool qkv_args_ok(const GemmParamsH& p, bool gammas_ok) {
  return p.N == 3 * p.heads * 64 && p.vt && p.vt_nblk * 64 >= (p.M + 255) / 256 * 256 && gammas_ok;
}

template <int DT>
static int launch_dt(hipStream_t stream, int epilogue, const GemmParamsH& p, int form, bool planes_to_ws) {
  if (planes_to_ws) {
    if ((p.ldc & 7) || (p.ldr & 7) || (epilogue == EPI_H_BIAS_RESID_H16 && !p.resid_h)) return RAP_ERR_INVALID;
    return launch_splitk<DT>(stream, epilogue, p, rap_form_stages(form), rap_form_splits(form));
  }
  switch (epilogue) {
    case EPI_H_BIAS: return launch_form<EPI_H_BIAS, DT>(stream, p, form);
    case EPI_H_BIAS_RESID_F32: return launch_form<EPI_H_BIAS_RESID_F32, DT>(stream, p, form);
    case EPI_H_BIAS_RESID_H16:
      if (!p.resid_h || (p.ldc & 7) || (p.ldr & 7)) return RAP_ERR_INVALID;
      return launch_form<EPI_H_BIAS_RESID_H16, DT>(stream, p, form);
    case EPI_H_GEGLU: return launch_form<EPI_H_GEGLU, DT>(stream, p, form);
    case EPI_H_QKV_NORM:
      if (!qkv_args_ok(p, p.gamma_q && p.gamma_k)) return RAP_ERR_INVALID;
      return launch_form<EPI_H_QKV_NORM, DT>(stream, p, form);
    case EPI_H_QKV:
      if (!qkv_args_ok(p, true)) return RAP_ERR_INVALID;
      return launch_form<EPI_H_QKV, DT>(stream, p, form);
    default: return RAP_ERR_INVALID;
  }
}

static int launch_x2(hipStream_t stream, int epilogue, const GemmParamsH& p, int form, bool planes_to_ws) {
  switch (epilogue) {
    case EPI_H_BIAS_RESID_F32:
      if (planes_to_ws) {
        if ((p.ldc & 7) || (p.ldr & 7)) return RAP_ERR_INVALID;
        return launch_splitk<RAP_DT_F16, true>(stream, epilogue, p, rap_form_stages(form), rap_form_splits(form));
      }
      return launch_form<EPI_H_BIAS_RESID_F32, RAP_DT_F16, true>(stream, p, form);
    case EPI_H_GEGLU: return launch_form<EPI_H_GEGLU, RAP_DT_F16, true>(stream, p, form);      // (ldc: checked by launch_gemm_h16)
    case EPI_H_QKV_NORM:
      if (!qkv_args_ok(p, (p.gamma_q == nullptr) == (p.gamma_k == nullptr))) return RAP_ERR_INVALID;
      return launch_form<EPI_H_QKV_NORM, RAP_DT_F16, true>(stream, p, form);
    default: return RAP_ERR_INVALID;
  }
}

int launch_gemm_h16(hipStream_t stream, int dtype, int epilogue, const GemmParamsH& p) {
  bool planes_to_ws = false;
  const int form = gemm_h16_form(dtype, epilogue, p, &planes_to_ws);
  if (form <= 0) return form;      // nothing to do (M <= 0) or a refused shape
  // output / residual rows are stored as whole 16-byte pieces: four fp32 or eight 16-bit columns
  if (epilogue == EPI_H_BIAS_RESID_F32 && ((p.ldc & 3) || p.ldc < p.N || (p.resid && ((p.ldr & 3) || p.ldr < p.N)))) return RAP_ERR_INVALID;
  if ((epilogue == EPI_H_BIAS || epilogue == EPI_H_GEGLU) && (p.ldc & 7)) return RAP_ERR_INVALID;
  if (dtype == RAP_DT_F32X2) return launch_x2(stream, epilogue, p, form, planes_to_ws);
  if (dtype == RAP_DT_BF16) return launch_dt<RAP_DT_BF16>(stream, epilogue, p, form, planes_to_ws);
  return launch_dt<RAP_DT_F16>(stream, epilogue, p, form, planes_to_ws);
}

// ---------------------------------------------------------------------------------------------
// fp32 -> bf16 / fp16 conversion (weights at model creation; round to nearest even)
// ---------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(256) void convert_h16_kernel(const float* __restrict__ src, u16* __restrict__ dst, size_t n4) {
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * 256;
  for (; i < n4; i += stride) {
    const float4 v = reinterpret_cast<const float4*>(src)[i];
    reinterpret_cast<uint2*>(dst)[i] = h16_pack4<DT>(v.x, v.y, v.z, v.w);
  }
}

// the fp32 embedding rounded into the fp16 residual stream: saturating (half.h f16_sat)
__global__ __launch_bounds__(256) void convert_f16_sat_kernel(const float* __restrict__ src, u16* __restrict__ dst, size_t n4) {
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * 256;
  for (; i < n4; i += stride) {
    const float4 v = reinterpret_cast<const float4*>(src)[i];
    reinterpret_cast<uint2*>(dst)[i] = h16_pack4<RAP_DT_F16>(f16_sat(v.x), f16_sat(v.y), f16_sat(v.z), f16_sat(v.w));
  }
}
int launch_convert_f16_sat(hipStream_t stream, const float* src, u16* dst, size_t n) {
  if (n == 0) return RAP_OK;
  if (n % 4 != 0) return RAP_ERR_INVALID;
  const size_t n4 = n / 4;
  const unsigned grid = (unsigned)((n4 + 255) / 256 < 65536 ? (n4 + 255) / 256 : 65536);
  hipLaunchKernelGGL(convert_f16_sat_kernel, dim3(grid), dim3(256), 0, stream, src, dst, n4);
  RAP_LAUNCH_CHECK();
  return RAP_OK;
}

int launch_convert_h16(hipStream_t stream, int dtype, const float* src, u16* dst, size_t n) {
  if (n == 0) return RAP_OK;
  if (n % 4 != 0) return RAP_ERR_INVALID;
  const size_t n4 = n / 4;
  const unsigned grid = (unsigned)((n4 + 255) / 256 < 65536 ? (n4 + 255) / 256 : 65536);
  if (dtype == RAP_DT_BF16) hipLaunchKernelGGL(convert_h16_kernel<RAP_DT_BF16>, dim3(grid), dim3(256), 0, stream, src, dst, n4);
  else if (dtype == RAP_DT_F16) hipLaunchKernelGGL(convert_h16_kernel<RAP_DT_F16>, dim3(grid), dim3(256), 0, stream, src, dst, n4);
  else return RAP_ERR_INVALID;
  RAP_LAUNCH_CHECK();
  return RAP_OK;
}

// fp16 -> fp32 (the 16-bit residual stream handed to the fp32 head / returned as transformer_features)
__global__ __launch_bounds__(256) void convert_f16_to_f32_kernel(const u16* __restrict__ src, float* __restrict__ dst, size_t n8) {
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * 256;
  for (; i < n8; i += stride) {
    float v[8];
    h16_unpack8<RAP_DT_F16>(reinterpret_cast<const uint4*>(src)[i], v);
    reinterpret_cast<float4*>(dst)[2 * i] = float4{v[0], v[1], v[2], v[3]};
    reinterpret_cast<float4*>(dst)[2 * i + 1] = float4{v[4], v[5], v[6], v[7]};
  }
}
int launch_convert_f16_to_f32(hipStream_t stream, const u16* src, float* dst, size_t n) {
  if (n == 0) return RAP_OK;
  if (n % 8 != 0) return RAP_ERR_INVALID;
  const size_t n8 = n / 8;
  const unsigned grid = (unsigned)((n8 + 255) / 256 < 65536 ? (n8 + 255) / 256 : 65536);
  hipLaunchKernelGGL(convert_f16_to_f32_kernel, dim3(grid), dim3(256), 0, stream, src, dst, n8);
  RAP_LAUNCH_CHECK();
  return RAP_OK;
}
