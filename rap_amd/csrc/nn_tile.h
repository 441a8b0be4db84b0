// Device pieces of every brute-force nearest-neighbour search of the library (nn_metrics.hip, icp.hip, icp_plane.hip, pair_metrics.hip,
// part_acc.hip, normals.hip, overlap.hip) and of the grid search that has to return the same bits (nn_grid.hip): the squared distance
// every search compares, the segment clamp, the work-list emitters, and the tiled search itself -- a block owns NN_TILE queries, one per
// lane, and streams the candidates through one float4 tile[NN_TILE] in LDS, one ds_read_b128 broadcast per candidate.
#pragma once
#include "kernels.h"

#define NN_TILE 256

// |q - p|^2 in fp32 from direct differences: the one expression every search compares.  hipcc contracts it to dx*dx rounded, dy*dy fused
// onto it, dz*dz rounded, one add (v_pk_mul_f32 of dx and dz, v_fma_f32 of dy, v_add_f32 in the tiled kernels; v_mul, v_fmac, v_mul, v_add
// in the grid walk): the same chain in every kernel that calls it, checked in their disassembly.  Pinning the
// chain with explicit fma / contraction pragmas was tried and costs the tiled kernels their packed math.
__device__ __forceinline__ float nn_d2(float qx, float qy, float qz, float px, float py, float pz) {
  const float dx = qx - px, dy = qy - py, dz = qz - pz;
  return dx * dx + dy * dy + dz * dz;
}

// (start, len) of row k clamped to [0, limit): an inconsistent table cannot make a kernel index outside the array
__device__ __forceinline__ void nn_segment(const int32_t* __restrict__ seg, int k, long limit, int& start, int& len) {
  long s = seg[(size_t)k * 2], n = seg[(size_t)k * 2 + 1];
  s = s < 0 ? 0 : s > limit ? limit : s;
  n = n < 0 ? 0 : n > limit - s ? limit - s : n;
  start = (int)s; len = (int)n;
}

// ---- work lists: one thread appends items of NN_TILE queries, n = the number of items so far ----
// the items of queries [0, x_len) against candidates [y_start, y_start + y_len), while the list has room; returns the new n.  I: int, or
// long where the caller clamped in long (the values fit an int)
template <class I>
__device__ __forceinline__ int nn_emit_items(NnWork* items, int n, int max_items, I x_start, I x_len, I y_start, I y_len, int pad0, int pad1) {
  for (I q0 = 0; q0 < x_len && n < max_items; q0 += NN_TILE) {
    NnWork w = {(int)x_start, (int)x_len, (int)q0, (int)y_start, (int)y_len, pad0, pad1, 0};
    items[n++] = w;
  }
  return n;
}
// all of them or none: segments that overlap can ask for more items than the list holds, and such a problem is left out whole.
// Counts n up and returns the number of items appended
__device__ __forceinline__ int nn_emit_items_whole(NnWork* items, int& n, int max_items, int x_start, int x_len, int y_start, int y_len,
                                                   int pad0) {
  const int want = (x_len + NN_TILE - 1) / NN_TILE;
  if (x_len <= 0 || want > max_items - n) return 0;
  for (int q0 = 0; q0 < x_len; q0 += NN_TILE) { NnWork w = {x_start, x_len, q0, y_start, y_len, pad0, 0, 0}; items[n++] = w; }
  return want;
}
// the unused slots: x_len = 0, which a query block returns on
__device__ __forceinline__ void nn_zero_items(NnWork* items, int n, int max_items) {
  for (; n < max_items; ++n) { NnWork w = {0, 0, 0, 0, 0, 0, 0, 0}; items[n] = w; }
}

// ---- the tile ----
// row i of an (n,3) array as a candidate (w stays what it is)
__device__ __forceinline__ void nn_row(const float* P, size_t i, float4& c) { c.x = P[i * 3 + 0]; c.y = P[i * 3 + 1]; c.z = P[i * 3 + 2]; }

// Candidates [k0, k0 + NN_TILE) of `len` into the tile, between two barriers.  Lane t stores a copy c of `pad` after load(k0 + t, c)
// has filled in the components it sets (nn_row: x, y, z); past the end it stores `pad` itself, a slot no search compares.  The loader
// fills a float4 in place and is not asked to return one: returned whole, the zero w of a plain row costs a select.  Every thread of
// the block calls it.
template <class Load>
__device__ __forceinline__ void nn_tile_stage(float4* tile, int k0, int len, float4 pad, Load load) {
  const int k = k0 + threadIdx.x;
  float4 c = pad;
  if (k < len) load(k, c);
  __syncthreads();
  tile[threadIdx.x] = c;
  __syncthreads();
}

// The tiled search: declares best = min over the `len` candidates of nn_d2(q, candidate k) and besti = the FIRST k that attains it
// (strict <, torch.min's tie rule); inf and -1 without a candidate, or when every d2 is inf or NaN.  `load`: as nn_tile_stage.  Every
// thread of the block runs it.  A macro: as a function (tile by pointer or by array reference, best / besti by reference, the loader's
// captures by reference or by value) the unrolled loop gets another schedule, two more LDS reads in flight and an extra v_cndmask per
// candidate.
#define NN_TILE_ARGMIN(tile, len, qx, qy, qz, load, best, besti)                         \
  float best = __builtin_inff();                                                         \
  int besti = -1;                                                                        \
  for (int k0 = 0; k0 < (len); k0 += NN_TILE) {                                          \
    nn_tile_stage(tile, k0, len, make_float4(0.f, 0.f, 0.f, 0.f), load);                 \
    const int nk = min(NN_TILE, (len) - k0);                                             \
    _Pragma("unroll 8") for (int j = 0; j < nk; ++j) {                                   \
      const float4 p = (tile)[j];                                                        \
      const float d2 = nn_d2(qx, qy, qz, p.x, p.y, p.z);                                 \
      if (d2 < best) { best = d2; besti = k0 + j; }                                      \
    }                                                                                    \
  }
