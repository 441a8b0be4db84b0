// The body of attention_h16_kernel and attention_h16_softcap_kernel (attn_h16.hip), included once into each: the names DT, OPT, DMA, NS,
// CAP (compile-time) and qk, vt, vt_nblk, out, TP, heads, items, bound, bq, cap are the including kernel's.  Text inclusion: see
// attn_tile.h.  CAP: ATTN_SOFTCAP there.
// attention_h16_kgroup_kernel has its own LDS layout, K / V^T stream, key loop and merge, and takes the rest from here, one part per
// inclusion (#define HATT_PART n in front of each; undefined = the whole body):
//   1 = the work item, the Q fragments, the softmax state, the staging coordinates   (reads QW = query waves of the block, Ks, Vs)
//   2 = one key tile: S^T, softmax, O^T += V^T P^T   (reads cur = the tile's LDS slot, t = its index in the segment, Ks, Vs, LDR)
//   3 = normalise and store whole rows through the wave's slab   (reads smem)
#ifndef HATT_PART
  constexpr int QW = 8;                 // every wave has its own 32 query rows
  constexpr int LDR = DMA ? 64 : HLD;   // LDS row stride in 16-bit elements: 128 B swizzled (DMA) or 144 B padded
  static_assert(NS == 2 || (DMA && NS == 4), "two stages, or the four-stage LDS-DMA ring");
  // (at the full configuration -- two blocks per CU cover each other -- a ring of THREE stages was measured in r03 call 21: 1 132 vs
  // 1 141 TF in the bench; there the DMA latency is not exposed with two.)
  constexpr int SMEM_ELEMS = NS == 2 ? 4 * HKV * HLD : NS * 2 * HKV * 64;      // 36 KB (two stages / the 8 output slabs) or 64 KB (ring)
  static_assert(8 * 32 * HLD <= SMEM_ELEMS, "output slabs must fit");
  __shared__ __attribute__((aligned(16))) u16 smem[SMEM_ELEMS];
  u16* Ks = smem;                    // [NS][64 keys][LDR]
  u16* Vs = smem + NS * HKV * LDR;   // [NS][64 d][LDR]   (columns = vt_pos of the key)
#endif

#if !defined(HATT_PART) || HATT_PART == 1
  typedef typename H16<DT>::T8 T8;
  const int tid = threadIdx.x;
  const int head = blockIdx.x % heads;
  const AttnWorkItem it = items[blockIdx.x / heads];
  const int len = it.seg_len;
  if (len <= 0) return;
  const int lane = tid & 63, wave = tid >> 6;
  const int hi = lane >> 5, l31 = lane & 31;
  const int seg0 = it.seg_start, seg1 = it.seg_start + len;
  const int qwave = wave % QW;          // the wave's 32 query rows within the work item ...
  [[maybe_unused]] const int grp = wave / QW;      // ... and its key group (0 here: the key-group kernel's)

  const u16* Qg = qk + (size_t)head * TP * 64;
  const u16* Kg = qk + (size_t)(heads + head) * TP * 64;
  const u16* Vg = vt + (size_t)head * vt_nblk * (64 * 64);

  const int qw0 = it.q0 + qwave * 32;
  // waves beyond the work item's rows / the segment still help stage K/V (QW < 8: the item is 32 QW rows, every query wave lies inside)
  const bool wave_active = (QW < 8 || wave * 32 < bq) && qw0 < len;

  // ---- Q fragments (B operand of S^T): qf[s] = Q[q][16s + 8hi .. +7]
  T8 qf[4];
  {
    int q = qw0 + l31;
    q = q < len ? q : len - 1;
    const u16* qp = Qg + (size_t)(seg0 + q) * 64 + 8 * hi;
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = __builtin_bit_cast(T8, *reinterpret_cast<const uint4*>(qp + 16 * s));
  }

  f32x16 o0, o1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }
  // OPT bit 3: bounded softmax -- the caller guarantees q.k/8 <= bound[head] (after qk-norm: 8 max|gamma_q| max|gamma_k|), so
  // the fixed offset bound replaces the running maximum: p = exp(s - bound), no max chain, no rescale, no branch.
  // OPT bit 4 (with bit 3, bf16 only): q arrives pre-scaled by log2(e)/8 (the QKV epilogue, q_mul = log2 e), so a score IS the exp2
  // argument, and because |score| <= bound * log2(e) <= 58 the offset is dropped altogether: p = exp2(score) lies in
  // [2^-58, 2^58], far inside the range of fp32 and bf16, and softmax is invariant to the common factor.  No per-score FMA:
  // 848 -> 917 TF per part, 952 -> 1032 per sample (r01 run 43).  Measured and rejected on top of it (run 44): row sums from the
  // matrix pipe (a third O tile against an all-ones V^T: 4 more MFMAs instead of 16 v_pk_add_f32 per key tile) -> 903 / 969.
  float mrun = (OPT & 16) ? 0.f : (OPT & 8) ? bound[head] * 8.0f : -1e30f, lsum = 0.f;
  const float c = 0.125f * 1.44269504088896340736f;   // 1/sqrt(64) * log2(e)

  const int b_first = seg0 >> 6;
  const int ntile = ((seg1 - 1) >> 6) - b_first + 1;
  // ---- LDS-DMA (DMA = true): wave w stages rows 8w .. 8w+7 of the K tile and of the V^T tile; lane -> (row 8w + lane/8, physical slot lane%8)
  const int drow = (tid >> 6) * 8 + ((tid & 63) >> 3);
  const int dls = ((tid & 7) ^ ((drow >> 1) & 7)) * 8;              // logical slot (in elements) this lane fetches
  const unsigned lds_k = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) u16*)Ks + (unsigned)(tid >> 6) * 1024u);
  const unsigned lds_v = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) u16*)Vs + (unsigned)(tid >> 6) * 1024u);
#endif

#ifndef HATT_PART
  // ---- register staging (DMA = false): 512 threads, one 16-byte chunk of K and one of V^T per thread per tile
  const int srow = tid >> 3, sch = (tid & 7) * 8;
  const int soff = srow * HLD + sch;
  uint4 rk = make_uint4(0, 0, 0, 0), rv = rk;
#define HATT_LOAD(T)                                                                                 \
  {                                                                                                  \
    const int blk_ = b_first + (T);                                                                  \
    int tok_ = blk_ * 64 + srow;                                                                     \
    tok_ = tok_ < TP ? tok_ : TP - 1;                                                                \
    rk = *reinterpret_cast<const uint4*>(Kg + (size_t)tok_ * 64 + sch);                              \
    rv = *reinterpret_cast<const uint4*>(Vg + ((size_t)blk_ * 64 + srow) * 64 + sch);                \
  }
#define HATT_STORE(BUF)                                                                              \
  *reinterpret_cast<uint4*>(Ks + (BUF) * (HKV * HLD) + soff) = rk;                                   \
  *reinterpret_cast<uint4*>(Vs + (BUF) * (HKV * HLD) + soff) = rv;
#define HATT_DMA(T, BUF)                                                                             \
  {                                                                                                  \
    const int blk_ = b_first + (T);                                                                  \
    int tok_ = blk_ * 64 + drow;                                                                     \
    tok_ = tok_ < TP ? tok_ : TP - 1;                                                                \
    LDS_DMA_X4(Kg + (size_t)tok_ * 64 + dls, lds_k + (unsigned)(BUF) * (HKV * 64 * 2))                        \
    LDS_DMA_X4(Vg + ((size_t)blk_ * 64 + drow) * 64 + dls, lds_v + (unsigned)(BUF) * (HKV * 64 * 2))          \
  }

  if (DMA) {
#pragma unroll
    for (int s_ = 0; s_ < NS - 1; ++s_)
      if (s_ < ntile) { HATT_DMA(s_, s_) }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    HATT_Q_LANDED(qf)
  } else {
    HATT_LOAD(0)
    HATT_STORE(0)
  }
  __syncthreads();

  for (int t = 0; t < ntile; ++t) {
    const int cur = t & (NS - 1);
    const bool more = (t + 1) < ntile;
    const bool ahead = (t + NS - 1) < ntile;      // the tile this iteration requests: NS - 1 ahead, into the stage tile t - 1 left at the last barrier
    if (DMA) { if (ahead) { HATT_DMA(t + NS - 1, (t + NS - 1) & (NS - 1)) } } else if (more) { HATT_LOAD(t + 1) }

    if (wave_active) {
#endif
#if !defined(HATT_PART) || HATT_PART == 2
      // ---- S^T = K Q^T : two 32-key sub-tiles x 32 queries
      f32x16 s0, s1;
#pragma unroll
      for (int r = 0; r < 16; ++r) { s0[r] = 0.f; s1[r] = 0.f; }
      const int swz = (l31 >> 1) & 7;                 // DMA layout: slot ^ ((row >> 1) & 7), the same for rows l31 and 32 + l31
      const u16* kp = Ks + cur * (HKV * LDR) + l31 * LDR + (DMA ? 0 : 8 * hi);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int ko = DMA ? ((2 * s + hi) ^ swz) * 8 : 16 * s;
        const T8 k0 = __builtin_bit_cast(T8, *reinterpret_cast<const uint4*>(kp + ko));
        const T8 k1 = __builtin_bit_cast(T8, *reinterpret_cast<const uint4*>(kp + 32 * LDR + ko));
        s0 = H16<DT>::mfma(k0, qf[s], s0);
        s1 = H16<DT>::mfma(k1, qf[s], s1);
      }
      // ---- soft cap, key mask, softmax (lane-local except one cross-half max, online form only), exponentials and row sum: attn_tile.h
      if constexpr (CAP) ATTN_SOFTCAP(s0, s1, cap)
      ATTN_MASK_KEYS(s0, s1, (b_first + t) * 64, seg0, seg1, hi)
      ATTN_ONLINE_RESCALE(OPT, s0, s1, o0, o1, mrun, lsum, c)
      ATTN_EXP_ROWSUM(OPT, s0, s1, mrun, lsum, c)
      // ---- O^T += V^T P^T : key step ks contracts the keys held in registers 8(ks&1)..+7 of sub-tile ks>>1
      const u16* vp = Vs + cur * (HKV * LDR) + l31 * LDR + (DMA ? 0 : 8 * hi);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const int rb = 8 * (ks & 1);
        T8 pb;
        if ((ks >> 1) == 0)
          pb = h16_pack8<DT>(s0[rb + 0], s0[rb + 1], s0[rb + 2], s0[rb + 3], s0[rb + 4], s0[rb + 5], s0[rb + 6], s0[rb + 7]);
        else
          pb = h16_pack8<DT>(s1[rb + 0], s1[rb + 1], s1[rb + 2], s1[rb + 3], s1[rb + 4], s1[rb + 5], s1[rb + 6], s1[rb + 7]);
        const int vo = DMA ? ((2 * ks + hi) ^ swz) * 8 : 16 * ks;
        const T8 v0 = __builtin_bit_cast(T8, *reinterpret_cast<const uint4*>(vp + vo));
        const T8 v1 = __builtin_bit_cast(T8, *reinterpret_cast<const uint4*>(vp + 32 * LDR + vo));
        o0 = H16<DT>::mfma(v0, pb, o0);
        o1 = H16<DT>::mfma(v1, pb, o1);
      }
#endif
#ifndef HATT_PART
    }

    if (more && !DMA) { HATT_STORE(cur ^ 1) }
    if (DMA) {      // this wave's two pieces of tile t + 1 have landed: loads retire in order, the NS - 2 younger tiles may stay in flight
      if (NS > 2 && ahead) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * (NS - 2)) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
  }

  if (!wave_active) return;
#endif
#if !defined(HATT_PART) || HATT_PART == 3
  // ---- normalise and store: lane owns query l31; register r of tile e is d = 32e + crow(r, hi): groups of 4 contiguous d.
  // every wave of the block is past the last tile's barrier: the K / V^T buffers are free.  Slab of this wave: [32 queries][72]
  const float inv = 1.0f / attn_xhalf_sum(lsum);
  u16* slab = smem + wave * (32 * HLD);
  u16* wp = slab + l31 * HLD + 4 * hi;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    *reinterpret_cast<uint2*>(wp + 8 * g) =
        h16_pack4<DT>(o0[4 * g + 0] * inv, o0[4 * g + 1] * inv, o0[4 * g + 2] * inv, o0[4 * g + 3] * inv);
    *reinterpret_cast<uint2*>(wp + 32 + 8 * g) =
        h16_pack4<DT>(o1[4 * g + 0] * inv, o1[4 * g + 1] * inv, o1[4 * g + 2] * inv, o1[4 * g + 3] * inv);
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // the slab is private to the wave and LDS operations of a wave execute in order:
  __builtin_amdgcn_wave_barrier();                          // no block barrier (waves without queries have left already)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = (lane >> 3) + 8 * i, piece = lane & 7;
    const uint4 v = *reinterpret_cast<const uint4*>(slab + row * HLD + piece * 8);
    if (qw0 + row < len)
      *reinterpret_cast<uint4*>(out + (size_t)(seg0 + qw0 + row) * (heads * 64) + head * 64 + piece * 8) = v;
  }
#endif
#undef HATT_PART
