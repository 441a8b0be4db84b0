// Part accuracy on device: compute_part_acc (reference rectified_point_flow/eval/metrics.py:92-163), which per sample pads every part to
// the longest one, expands to n_parts^2 padded pairs for a batched pytorch3d chamfer, copies the matrix to the host and runs
// scipy.optimize.linear_sum_assignment there (one forced synchronisation per sample, memory n_parts^2 * max_len).
//
//   cd[b,i,j]  = mean_{x in gt_i} min_{y in pred_j} |x - y|^2 + mean_{y in pred_j} min_{x in gt_i} |x - y|^2      (:140-148)
//   cost[i,j]  = cd[i,j] >= threshold over the non-empty parts, n = n_parts                                        (:152)
//   (row, col) = linear_sum_assignment(cost);  part_acc = |{ cd[row,col] < threshold }| / n;  matched[b,row] = col (:153-158)
//
// One sync-free call for the whole batch.  Two small kernels lay out a clamped (start, len) table of the part slots and the work list;
// then:
//   1. part_nn_kernel: the N^2 work, on nn_tile.h's tile.  A block owns up to 256 queries of ONE part (one per
//      lane, in registers) and streams ALL points of the other cloud of the same sample through LDS once, in tiles of 256 float4 (one
//      ds_read_b128 per candidate, broadcast to the wave); the running minimum is closed -- stored and reset -- at every candidate-part
//      boundary, wherever in a tile it falls.  Result: d2[j][x] = min over part j of the other cloud, for every point x and part slot j
//      of x's sample (P planes of TP floats: lanes write and read consecutive addresses).  blockIdx.y picks the direction.
//   2. part_cd_kernel: a block per (sample, gt part), a wave per pred part: both means in double -- lane-strided partial sums in index
//      order, then the xor tree of wave_sum_d -- so the result does not depend on scheduling.  Writes cd (optional output) and the two
//      comparisons with the threshold as bit rows.
//   3. part_assign_kernel: a block per sample, lanes across the columns: assign.h's restatement of SciPy's solver with the column
//      scan as a reduction (RapLsapPick).
// No floating-point atomics anywhere: two runs give the same bits.
#include "assign.h"
#include "nn_tile.h"

#define PA_TILE NN_TILE
#define PA_MAX_GRID 1024      // blocks per direction; a block walks the work list with this stride

// seg[(b * P + p)] = (start, len) of part p of sample b, clamped: the sample's span is [cu[b], cu[b+1]) inside [0, TP], the parts follow
// one another inside it and the last ones are cut short (or empty) if points_per_part asks for more.  Every later kernel indexes the
// clouds through this copy only, so a malformed points_per_part / cu_batch gives wrong numbers, never an access outside the arrays.
__global__ void part_acc_segments_kernel(const int64_t* __restrict__ ppp, const int32_t* __restrict__ cu, int P, long TP,
                                         int32_t* __restrict__ seg) {
  if (threadIdx.x != 0) return;
  const int b = blockIdx.x;
  long a = cu[b], e = cu[b + 1];
  a = a < 0 ? 0 : a > TP ? TP : a;
  e = e < a ? a : e > TP ? TP : e;
  long pos = a;
  for (int p = 0; p < P; ++p) {
    long n = (long)ppp[(size_t)b * P + p];
    n = n < 0 ? 0 : n > e - pos ? e - pos : n;
    seg[((size_t)b * P + p) * 2] = (int32_t)pos;
    seg[((size_t)b * P + p) * 2 + 1] = (int32_t)n;
    pos += n;
  }
}

// one thread: work items (part, 256-query tile).  x_* = the part, y_* = the span of the sample's parts, pad0 = sample, pad1 = part slot
__global__ void part_acc_worklist_kernel(const int32_t* __restrict__ seg, int B, int P, long TP, NnWork* __restrict__ items, int max_items,
                                         int32_t* __restrict__ count) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int n = 0;
  for (int b = 0; b < B; ++b) {
    int s0, l0, s1, l1;
    nn_segment(seg, b * P, TP, s0, l0);
    nn_segment(seg, b * P + P - 1, TP, s1, l1);
    const int y_len = s1 + l1 - s0;
    for (int p = 0; p < P; ++p) {
      int s, l;
      nn_segment(seg, b * P + p, TP, s, l);
      n = nn_emit_items(items, n, max_items, s, l, s0, y_len, b, p);
    }
  }
  *count = n;
}

__global__ __launch_bounds__(PA_TILE) void part_nn_kernel(const float* __restrict__ gt, const float* __restrict__ pred,
                                                          const int32_t* __restrict__ seg, const NnWork* __restrict__ items,
                                                          const int32_t* __restrict__ count, int max_items, int P, long TP,
                                                          float* __restrict__ d2a, float* __restrict__ d2b) {
  __shared__ float4 tile[PA_TILE];
  __shared__ int pend[RAP_LSAP_MAX_N];      // end of every part of the sample, relative to the sample's start
  const bool back = blockIdx.y != 0;
  const float* __restrict__ X = back ? pred : gt;
  const float* __restrict__ Y = back ? gt : pred;
  float* __restrict__ out = back ? d2b : d2a;
  const int n_items = min(*count, max_items);
  for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
    const NnWork w = items[item];
    __syncthreads();                          // the previous item's readers of pend / tile are done
    if ((int)threadIdx.x < P) {
      int s, l;
      nn_segment(seg, w.pad0 * P + threadIdx.x, TP, s, l);
      pend[threadIdx.x] = s + l - w.y_start;
    }
    const int q = w.q0 + threadIdx.x;
    const bool active = q < w.x_len;
    const size_t qi = (size_t)w.x_start + (active ? q : w.x_len - 1);
    const float qx = X[qi * 3 + 0], qy = X[qi * 3 + 1], qz = X[qi * 3 + 2];
    __syncthreads();
    int cj = 0;                               // the candidate part the running minimum belongs to (block-uniform)
    while (cj < P && pend[cj] <= (cj ? pend[cj - 1] : 0)) ++cj;
    float best = __builtin_inff();
    for (int k0 = 0; k0 < w.y_len && cj < P; k0 += PA_TILE) {
      nn_tile_stage(tile, k0, w.y_len, make_float4(0.f, 0.f, 0.f, 0.f), [&](int k, float4& c) { nn_row(Y, (size_t)w.y_start + k, c); });
      const int nk = min(PA_TILE, w.y_len - k0);
      int j = 0;
      while (j < nk && cj < P) {
        const int part_end = pend[cj] - k0;   // in tile coordinates; may lie in a later tile
        const int e = min(nk, part_end);
#pragma unroll 8
        for (; j < e; ++j) {
          const float4 p = tile[j];
          best = fminf(best, nn_d2(qx, qy, qz, p.x, p.y, p.z));
        }
        if (part_end <= nk) {                 // the part ends in this tile: close its minimum
          if (active) out[(size_t)cj * TP + qi] = best;
          best = __builtin_inff();
          ++cj;
          while (cj < P && pend[cj] <= pend[cj - 1]) ++cj;
        }
      }
    }
  }
}

// block (b, i): cd[b,i,:], and bit j of ge / lt row (b,i) = cd >= thr / cd < thr (both 0 for an empty part or a NaN)
__global__ __launch_bounds__(256) void part_cd_kernel(const float* __restrict__ d2a, const float* __restrict__ d2b,
                                                      const int32_t* __restrict__ seg, int P, long TP, float thr, float* __restrict__ cd_out,
                                                      uint32_t* __restrict__ ge_bits, uint32_t* __restrict__ lt_bits) {
  __shared__ uint8_t flag[RAP_LSAP_MAX_N];
  const int row = blockIdx.x, i = row % P, b = row / P;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int si, li;
  nn_segment(seg, row, TP, si, li);
  for (int j = wave; j < P; j += 4) {
    int sj, lj;
    nn_segment(seg, b * P + j, TP, sj, lj);
    float cd = __builtin_nanf("");
    if (li > 0 && lj > 0) {
      const float* __restrict__ pa = d2a + (size_t)j * TP + si;      // gt_i -> pred_j
      const float* __restrict__ pb = d2b + (size_t)i * TP + sj;      // pred_j -> gt_i
      double sa = 0.0, sb = 0.0;
      for (int x = lane; x < li; x += 64) sa += (double)pa[x];
      for (int y = lane; y < lj; y += 64) sb += (double)pb[y];
      sa = wave_sum_d(sa);
      sb = wave_sum_d(sb);
      cd = (float)(sa / (double)li + sb / (double)lj);
    }
    if (lane == 0) {
      if (cd_out) cd_out[(size_t)row * P + j] = cd;
      flag[j] = (cd >= thr ? 1 : 0) | (cd < thr ? 2 : 0);
    }
  }
  __syncthreads();
  const int W = (P + 31) >> 5;
  if ((int)threadIdx.x < W) {
    uint32_t ge = 0, lt = 0;
    for (int k = 0; k < 32; ++k) {
      const int j = threadIdx.x * 32 + k;
      if (j < P) { ge |= (uint32_t)(flag[j] & 1) << k; lt |= (uint32_t)((flag[j] >> 1) & 1) << k; }
    }
    ge_bits[(size_t)row * W + threadIdx.x] = ge;
    lt_bits[(size_t)row * W + threadIdx.x] = lt;
  }
}

__device__ __forceinline__ RapLsapPick pick_wave_reduce(RapLsapPick p) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    RapLsapPick q;
    q.val = __shfl_xor(p.val, o, 64);
    q.first = __shfl_xor(p.first, o, 64);
    q.last_free = __shfl_xor(p.last_free, o, 64);
    p = rap_lsap_pick_combine(p, q);
  }
  return p;
}

// block b: the assignment of sample b.  Rows and columns count the NON-EMPTY parts in order (the reference's indexing, metrics.py:128-158)
__global__ __launch_bounds__(256) void part_assign_kernel(const int32_t* __restrict__ seg, const uint32_t* __restrict__ ge_bits,
                                                          const uint32_t* __restrict__ lt_bits, int P, long TP, float* __restrict__ part_acc,
                                                          int64_t* __restrict__ matched) {
  __shared__ uint32_t ge[RAP_LSAP_MAX_N * 8], lt[RAP_LSAP_MAX_N * 8];
  __shared__ double u[RAP_LSAP_MAX_N], v[RAP_LSAP_MAX_N], spc[RAP_LSAP_MAX_N];
  __shared__ int path[RAP_LSAP_MAX_N], col4row[RAP_LSAP_MAX_N], row4col[RAP_LSAP_MAX_N], remaining[RAP_LSAP_MAX_N], slot[RAP_LSAP_MAX_N];
  __shared__ uint8_t SR[RAP_LSAP_MAX_N], SC[RAP_LSAP_MAX_N];
  __shared__ RapLsapPick wpick[4];
  __shared__ double st_min;
  __shared__ int st_i, st_sink, st_nrem, st_n, st_cnt[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int W = (P + 31) >> 5;
  for (int k = tid; k < P * W; k += 256) { ge[k] = ge_bits[(size_t)b * P * W + k]; lt[k] = lt_bits[(size_t)b * P * W + k]; }
  if (tid == 0) {
    int n = 0;
    for (int p = 0; p < P; ++p) {
      int s, l;
      nn_segment(seg, b * P + p, TP, s, l);
      if (l > 0) slot[n++] = p;
    }
    st_n = n;
  }
  __syncthreads();
  const int n = st_n;
  if (n == 0) {                               // the reference raises here (pad_sequence of an empty list)
    if (tid == 0) part_acc[b] = __builtin_nanf("");
    if (tid < P) matched[(size_t)b * P + tid] = 0;
    return;
  }
  if (tid < n) { u[tid] = 0.0; v[tid] = 0.0; path[tid] = -1; col4row[tid] = -1; row4col[tid] = -1; }
  bool feasible = true;
  for (int cur = 0; cur < n && feasible; ++cur) {
    if (tid < n) { remaining[tid] = n - tid - 1; SR[tid] = 0; SC[tid] = 0; spc[tid] = INFINITY; }
    double minVal = 0.0;
    int nrem = n, sink = -1, i = cur;
    __syncthreads();
    while (sink == -1) {
      RapLsapPick p = rap_lsap_pick_none();
      if (tid < nrem) {
        const int j = remaining[tid];
        const int si = slot[i], sj = slot[j];
        const double c = (double)((ge[si * W + (sj >> 5)] >> (sj & 31)) & 1u);
        rap_lsap_relax(minVal, c, u[i], v[j], i, &spc[j], &path[j]);
        p = rap_lsap_pick_of(spc[j], tid, row4col[j] == -1);
      }
      p = pick_wave_reduce(p);
      if (lane == 0) wpick[wave] = p;
      __syncthreads();
      if (tid == 0) {
        const RapLsapPick t = rap_lsap_pick_combine(rap_lsap_pick_combine(wpick[0], wpick[1]), rap_lsap_pick_combine(wpick[2], wpick[3]));
        SR[i] = 1;
        if (t.first < 0 || !(t.val < INFINITY)) {
          st_sink = -2;                       // no finite assignment: cannot happen with 0/1 costs
        } else {
          const int index = rap_lsap_pick_index(t);
          const int j = remaining[index];
          if (row4col[j] == -1) { st_sink = j; st_i = i; } else { st_sink = -1; st_i = row4col[j]; }
          SC[j] = 1;
          remaining[index] = remaining[nrem - 1];
          st_nrem = nrem - 1;
          st_min = t.val;
        }
      }
      __syncthreads();
      sink = st_sink;
      if (sink != -2) { i = st_i; nrem = st_nrem; minVal = st_min; }
    }
    if (sink == -2) { feasible = false; break; }
    double un = 0.0, vn = 0.0;
    if (tid < n) {
      const int c = col4row[tid];
      un = rap_lsap_dual_row(u[tid], SR[tid] != 0, tid == cur, minVal, (tid == cur || c < 0) ? 0.0 : spc[c]);
      vn = rap_lsap_dual_col(v[tid], SC[tid] != 0, minVal, spc[tid]);
    }
    __syncthreads();
    if (tid < n) { u[tid] = un; v[tid] = vn; }
    if (tid == 0) rap_lsap_augment(path, row4col, col4row, sink, cur);
    __syncthreads();
  }
  int ok = 0;
  if (feasible && tid < n) {
    const int si = slot[tid], sj = slot[col4row[tid]];
    ok = (int)((lt[si * W + (sj >> 5)] >> (sj & 31)) & 1u);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ok += __shfl_xor(ok, o, 64);
  if (lane == 0) st_cnt[wave] = ok;
  __syncthreads();
  if (tid == 0)
    part_acc[b] = feasible ? (float)((double)(st_cnt[0] + st_cnt[1] + st_cnt[2] + st_cnt[3]) / (double)n) : __builtin_nanf("");
  if (tid < P) matched[(size_t)b * P + tid] = (feasible && tid < n) ? (int64_t)col4row[tid] : 0;
}

size_t part_acc_max_items(long TP, int B, int P) { return (size_t)(TP / PA_TILE) + (size_t)B * P + 1; }

int launch_part_acc(hipStream_t stream, const float* gt, const float* pred, const int64_t* ppp, const int32_t* cu_batch, int B, int P, long TP,
                    float thr, float* part_acc, int64_t* matched, float* cd_out, int32_t* seg, float* d2a, float* d2b, NnWork* items,
                    int32_t* count, uint32_t* ge_bits, uint32_t* lt_bits) {
  if (B <= 0) return RAP_OK;
  if (P <= 0 || P > RAP_LSAP_MAX_N) return RAP_ERR_INVALID;
  hipLaunchKernelGGL(part_acc_segments_kernel, dim3(B), dim3(64), 0, stream, ppp, cu_batch, P, TP, seg);
  RAP_LAUNCH_CHECK();
  if (TP > 0) {
    const int max_items = (int)part_acc_max_items(TP, B, P);
    hipLaunchKernelGGL(part_acc_worklist_kernel, dim3(1), dim3(64), 0, stream, seg, B, P, TP, items, max_items, count);
    RAP_LAUNCH_CHECK();
    const int grid = max_items < PA_MAX_GRID ? max_items : PA_MAX_GRID;
    hipLaunchKernelGGL(part_nn_kernel, dim3(grid, 2), dim3(PA_TILE), 0, stream, gt, pred, seg, items, count, max_items, P, TP, d2a, d2b);
    RAP_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(part_cd_kernel, dim3(B * P), dim3(256), 0, stream, d2a, d2b, seg, P, TP, thr, cd_out, ge_bits, lt_bits);
  RAP_LAUNCH_CHECK();
  hipLaunchKernelGGL(part_assign_kernel, dim3(B), dim3(256), 0, stream, seg, ge_bits, lt_bits, P, TP, part_acc, matched);
  RAP_LAUNCH_CHECK();
  return RAP_OK;
}
