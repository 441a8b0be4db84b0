// The body of attention_x2_kernel and attention_x2_softcap_kernel (attn_x2.hip), included once into each: the names SPLIT, CAP
// (compile-time) and qk, vt, vt_nblk, out, TP, heads, items, part_o, part_ml, cap are the including kernel's.  Text inclusion: see attn_tile.h.
// CAP: as in attn_h16_body.inc.
  typedef x2_t8 T8;
  extern __shared__ __attribute__((aligned(1024))) u16 smem[];   // [2 stages][K c0 | K c1 | V c0 | V c1] = 64 KB; the 8 output slabs at the end
  const int tid = threadIdx.x;
  const int head = blockIdx.x % heads;
  const AttnWorkItem it = items[blockIdx.x / heads];
  const int len = it.seg_len;
  if (len <= 0) return;
  const int lane = tid & 63, wave = tid >> 6;
  const int hi = lane >> 5, l31 = lane & 31;
  const int seg0 = it.seg_start, seg1 = it.seg_start + len;

  const u16* Qg = qk + (size_t)head * 2 * TP * 64;                    // chunk c at + c * TP * 64
  const u16* Kg = qk + (size_t)(heads + head) * 2 * TP * 64;
  const u16* Vg = vt + (size_t)head * vt_nblk * (2 * XSUB);           // block b, chunk c at + (2 b + c) * XSUB

  const int qw0 = it.q0 + wave * 32;
  const bool wave_active = qw0 < len;   // waves beyond the segment still help stage K / V^T

  // ---- Q fragments (B operand of S^T): step s = dims 16 s + 8 hi .. +7 -> chunk s >> 1, in-chunk 16 (s & 1) + 8 hi
  T8 qh[4], ql[4];
  {
    int q = qw0 + l31;
    q = q < len ? q : len - 1;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const u16* qp = Qg + ((size_t)(s >> 1) * TP + seg0 + q) * 64 + 16 * (s & 1) + 8 * hi;
      qh[s] = __builtin_bit_cast(T8, *reinterpret_cast<const uint4*>(qp));
      ql[s] = __builtin_bit_cast(T8, *reinterpret_cast<const uint4*>(qp + 32));
    }
  }

  f32x16 o0, o1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }
  float mrun = -1e30f, lsum = 0.f;
  const float c = 0.125f * 1.44269504088896340736f;   // 1/sqrt(64) * log2(e)

  const int b_first0 = seg0 >> 6;
  const int ntile0 = ((seg1 - 1) >> 6) - b_first0 + 1;
  // SPLIT: this block's share of the key tiles (an empty share leaves m = -1e30, l = 0, O = 0: weight 0 in the combine pass)
  const int per = SPLIT ? (ntile0 + (int)gridDim.y - 1) / (int)gridDim.y : ntile0;
  const int t_begin = SPLIT ? (int)blockIdx.y * per : 0;
  const int b_first = b_first0 + t_begin;
  const int ntile = SPLIT ? (ntile0 - t_begin < per ? ntile0 - t_begin : per) : ntile0;      // may be <= 0
  // ---- LDS-DMA: wave w stages rows 8w .. 8w+7 of each of the four sub-tiles; lane -> (row 8w + lane/8, physical slot lane%8)
  const int drow = wave * 8 + (lane >> 3);
  const int dls = ((lane & 7) ^ ((drow >> 1) & 7)) * 8;              // logical slot (in elements) this lane fetches
  const unsigned lds_base = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) u16*)smem + (unsigned)wave * 1024u);
#define XATT_DMA(T, BUF)                                                                                      \
  {                                                                                                           \
    const int blk_ = b_first + (T);                                                                           \
    int tok_ = blk_ * 64 + drow;                                                                              \
    tok_ = tok_ < TP ? tok_ : TP - 1;                                                                         \
    const unsigned st_ = lds_base + (unsigned)(BUF) * (4 * XSUB * 2);                                         \
    LDS_DMA_X4(Kg + (size_t)tok_ * 64 + dls, st_)                                                             \
    LDS_DMA_X4(Kg + ((size_t)TP + tok_) * 64 + dls, st_ + XSUB * 2)                                           \
    LDS_DMA_X4(Vg + ((size_t)(2 * blk_) * 64 + drow) * 64 + dls, st_ + 2 * XSUB * 2)                          \
    LDS_DMA_X4(Vg + ((size_t)(2 * blk_ + 1) * 64 + drow) * 64 + dls, st_ + 3 * XSUB * 2)                      \
  }

  if (ntile > 0) { XATT_DMA(0, 0) }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  // the Q fragments have landed too -- tell the compiler (a use of every fragment), or it waits for them with vmcnt(n) inside the key
  // loop, where those waits would drain the DMA pieces of the NEXT tile it does not know about (attn_h16.hip)
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    uint4 a_ = __builtin_bit_cast(uint4, qh[s]), b_ = __builtin_bit_cast(uint4, ql[s]);
    asm volatile("" : "+v"(a_.x), "+v"(a_.y), "+v"(a_.z), "+v"(a_.w), "+v"(b_.x), "+v"(b_.y), "+v"(b_.z), "+v"(b_.w));
    qh[s] = __builtin_bit_cast(T8, a_); ql[s] = __builtin_bit_cast(T8, b_);
  }
  __syncthreads();

  const int swz = (l31 >> 1) & 7;                 // slot ^ ((row >> 1) & 7), the same for rows l31 and 32 + l31
  for (int t = 0; t < ntile; ++t) {
    const int cur = t & 1;
    const bool more = (t + 1) < ntile;
    if (more) { XATT_DMA(t + 1, cur ^ 1) }        // every wave left stage cur^1 at the last barrier

    if (wave_active) {
      const u16* stage = smem + cur * (4 * XSUB);
      // ---- S^T = K Q^T (three products): two 32-key sub-tiles x 32 queries
      f32x16 s0, s1;
#pragma unroll
      for (int r = 0; r < 16; ++r) { s0[r] = 0.f; s1[r] = 0.f; }
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const u16* kp = stage + (s >> 1) * XSUB + l31 * 64;
        const int oh = ((2 * (s & 1) + hi) ^ swz) * 8, ol = ((4 + 2 * (s & 1) + hi) ^ swz) * 8;
        const T8 k0h = __builtin_bit_cast(T8, *reinterpret_cast<const uint4*>(kp + oh));
        const T8 k0l = __builtin_bit_cast(T8, *reinterpret_cast<const uint4*>(kp + ol));
        const T8 k1h = __builtin_bit_cast(T8, *reinterpret_cast<const uint4*>(kp + 32 * 64 + oh));
        const T8 k1l = __builtin_bit_cast(T8, *reinterpret_cast<const uint4*>(kp + 32 * 64 + ol));
        s0 = H16<RAP_DT_F16>::mfma(k0l, qh[s], s0);
        s1 = H16<RAP_DT_F16>::mfma(k1l, qh[s], s1);
        s0 = H16<RAP_DT_F16>::mfma(k0h, ql[s], s0);
        s1 = H16<RAP_DT_F16>::mfma(k1h, ql[s], s1);
        s0 = H16<RAP_DT_F16>::mfma(k0h, qh[s], s0);
        s1 = H16<RAP_DT_F16>::mfma(k1h, qh[s], s1);
      }
      // ---- soft cap, key mask, online softmax with v_max3 row maxima and deferred rescale (P <= 2^ATTN_DEFER_THR fits fp16): attn_tile.h
      if constexpr (CAP) ATTN_SOFTCAP(s0, s1, cap)
      ATTN_MASK_KEYS(s0, s1, (b_first + t) * 64, seg0, seg1, hi)
      ATTN_ONLINE_RESCALE(3, s0, s1, o0, o1, mrun, lsum, c)
      ATTN_EXP_ROWSUM(3, s0, s1, mrun, lsum, c)
      // ---- O^T += V^T P^T (three products): key step ks contracts the keys held in registers 8(ks&1)..+7 of sub-tile ks>>1 =
      //      in-block positions 16 ks + 8 hi .. +7 -> V^T chunk ks >> 1, in-chunk 16 (ks & 1) + 8 hi
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const int rb = 8 * (ks & 1);
        f32x8 p8;
        if ((ks >> 1) == 0) p8 = f32x8{s0[rb + 0], s0[rb + 1], s0[rb + 2], s0[rb + 3], s0[rb + 4], s0[rb + 5], s0[rb + 6], s0[rb + 7]};
        else p8 = f32x8{s1[rb + 0], s1[rb + 1], s1[rb + 2], s1[rb + 3], s1[rb + 4], s1[rb + 5], s1[rb + 6], s1[rb + 7]};
        T8 ph, pl;
        x2_split8_nosat(p8, ph, pl);
        const u16* vp = stage + (2 + (ks >> 1)) * XSUB + l31 * 64;
        const int oh = ((2 * (ks & 1) + hi) ^ swz) * 8, ol = ((4 + 2 * (ks & 1) + hi) ^ swz) * 8;
        const T8 v0h = __builtin_bit_cast(T8, *reinterpret_cast<const uint4*>(vp + oh));
        const T8 v0l = __builtin_bit_cast(T8, *reinterpret_cast<const uint4*>(vp + ol));
        const T8 v1h = __builtin_bit_cast(T8, *reinterpret_cast<const uint4*>(vp + 32 * 64 + oh));
        const T8 v1l = __builtin_bit_cast(T8, *reinterpret_cast<const uint4*>(vp + 32 * 64 + ol));
        o0 = H16<RAP_DT_F16>::mfma(v0l, ph, o0);
        o1 = H16<RAP_DT_F16>::mfma(v1l, ph, o1);
        o0 = H16<RAP_DT_F16>::mfma(v0h, pl, o0);
        o1 = H16<RAP_DT_F16>::mfma(v1h, pl, o1);
        o0 = H16<RAP_DT_F16>::mfma(v0h, ph, o0);
        o1 = H16<RAP_DT_F16>::mfma(v1h, ph, o1);
      }
    }

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's four pieces of tile t + 1 have landed
    __syncthreads();
  }

  if (!wave_active) return;
  if constexpr (SPLIT) {
    // partial results of this key range: O^T unnormalised (relative to mrun), row-major (TP, heads * 64) fp32 per range; (m, l) per (token, head)
    const int q = qw0 + l31;
    if (q < len) {
      const size_t tok = (size_t)blockIdx.y * TP + (size_t)(seg0 + q);
      float* po = part_o + tok * ((size_t)heads * 64) + head * 64 + 4 * hi;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        *reinterpret_cast<float4*>(po + 8 * g) = float4{o0[4 * g + 0], o0[4 * g + 1], o0[4 * g + 2], o0[4 * g + 3]};
        *reinterpret_cast<float4*>(po + 32 + 8 * g) = float4{o1[4 * g + 0], o1[4 * g + 1], o1[4 * g + 2], o1[4 * g + 3]};
      }
    }
    const float lall = attn_xhalf_sum(lsum);
    if (q < len && hi == 0) *reinterpret_cast<float2*>(part_ml + (((size_t)blockIdx.y * TP + (size_t)(seg0 + q)) * heads + head) * 2) = float2{mrun, lall};
    return;
  }
  // ---- normalise, split and store.  Lane owns query l31; register r of tile e is head dim 32 e + crow(r, hi) (groups of 4 contiguous
  // dims), i.e. tile e IS chunk e of this head.  Every wave is past the last tile's barrier: the stages are free.  Slab of this wave:
  // [32 queries][72]: 32 heads | 32 tails of one chunk, written and drained once per chunk (LDS operations of a wave execute in order).
  const float inv = 1.0f / attn_xhalf_sum(lsum);
  u16* slab = smem + wave * (32 * XLD);
  u16* wp = slab + l31 * XLD + 4 * hi;
  const size_t orow = (size_t)heads * 128;
#pragma unroll
  for (int e = 0; e < 2; ++e) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 v4 = e == 0 ? f32x4{o0[4 * g + 0], o0[4 * g + 1], o0[4 * g + 2], o0[4 * g + 3]} : f32x4{o1[4 * g + 0], o1[4 * g + 1], o1[4 * g + 2], o1[4 * g + 3]};
      const f32x4 n4 = v4 * inv;
      const x2_t4 h4 = __builtin_convertvector(n4, x2_t4);
      const x2_t4 l4 = __builtin_convertvector(n4 - __builtin_convertvector(h4, f32x4), x2_t4);
      *reinterpret_cast<uint2*>(wp + 8 * g) = __builtin_bit_cast(uint2, h4);
      *reinterpret_cast<uint2*>(wp + 32 + 8 * g) = __builtin_bit_cast(uint2, l4);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = (lane >> 3) + 8 * i, piece = lane & 7;
      const uint4 v = *reinterpret_cast<const uint4*>(slab + row * XLD + piece * 8);
      if (qw0 + row < len)
        *reinterpret_cast<uint4*>(out + (size_t)(seg0 + qw0 + row) * orow + head * 128 + e * 64 + piece * 8) = v;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // the slab's reads have returned before chunk 1 overwrites it
    __builtin_amdgcn_wave_barrier();
  }
