// LDS-DMA (global_load_lds_dwordx4): every lane moves 16 bytes global -> LDS without a VGPR round trip; the wave's 64 pieces land
// lane-linearly in the 1 KiB at the wave-uniform LDS byte address LDSB, which travels in m0 (saved and restored around the load).
// Issued from inline asm: through the builtin, hipcc (ROCm 7.2) treats the transfer as an LDS write that may alias every later ds_read
// and drains it (s_waitcnt vmcnt(0)) before the first fragment read of the SAME iteration, which serialises the whole pipeline.  Hidden
// in asm, the transfer is retired by the caller's explicit vmcnt wait in front of the barrier that publishes the tile.
#pragma once

// vaddr form: GSRC = the lane's 64-bit global source address
#define LDS_DMA_X4(GSRC, LDSB)                                                                                \
  {                                                                                                           \
    unsigned keep_;                                                                                           \
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0" \
                 : "=&s"(keep_) : "v"(GSRC), "s"(LDSB) : "memory");                                           \
  }
// saddr form: scalar base SBASE (64-bit, SGPRs) + the lane's 32-bit byte offset VOFF
#define LDS_DMA_X4_SADDR(VOFF, SBASE, LDSB)                                                                   \
  {                                                                                                           \
    unsigned keep_;                                                                                           \
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3\n\ts_mov_b32 m0, %0" \
                 : "=&s"(keep_) : "v"(VOFF), "s"(LDSB), "s"(SBASE) : "memory");                                \
  }
