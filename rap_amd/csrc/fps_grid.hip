// Farthest point sampling over a bucket index: a second, exact path next to fps.hip.  For the same inputs it writes, bit for bit, the
// index lists fps_kernel writes: the same fp32 distance (nn_d2, nn_tile.h: dx*dx + dy*dy + dz*dz with dx = p - last), the same running
// minimum, the same winner (largest distance, then the lowest original index).  What changes is the work per pick: fps_kernel re-reads
// every point for every pick; here a pick touches only the buckets it can change.
//
// One block per cloud does everything; blocks never communicate, and every loop is bounded by K, the point count or the bucket count.
//
// Build, once per cloud.  Bounding box of the cloud -> a uniform grid of cubic cells aiming at `per` points per cell and at most
// FPS_GRID_MAX_BUCKETS cells (fps_grid_dims, fps_grid.h; an axis without extent gets one cell) -> counting sort of the rows into the
// workspace as float4 (x, y, z, original index), with the running distance (+inf) of every sorted row beside it.  A cell is a bucket.
// Per bucket the LDS holds: the TIGHT box of its rows (LDS atomic min / max of order-preserving keys), the largest running distance in
// it (max, +inf to begin with) and the lowest original index that attains it (arg).  An empty cell has max = -inf and is never opened
// or picked.  The order of rows inside a bucket depends on the atomics of the sort; nothing depends on that order, because every
// comparison that decides something compares original indices.
//
// Per pick.  s = the last pick.  Every thread tests its buckets and appends the open ones to a queue in LDS (at most one entry per
// bucket); barrier; wave w takes entries w, w + waves, ...: over the rows of a bucket d = min(d, d2), and the bucket's (max, arg) is
// rewritten from all of its rows; barrier; the block reduces (max, arg) over all buckets by (larger max, then lower arg); barrier; the
// winner is the next pick.  A bucket is handled by whichever wave draws it, so the stores of one iteration are ordered before the loads
// of the next by the block barriers, not by thread ownership as in fps_kernel.
//
// The skip rule, and why the path is exact.  A bucket with box [lo, hi] is skipped iff lb >= max, where
//   e_a = max(lo_a - s_a, s_a - hi_a, 0) per axis,   lb = (e_x^2 + e_y^2 + e_z^2) * (1 - 2^-16)        (fps_grid_lower_bound).
// Rounding.  For a row p of the bucket lo_a <= p_a <= hi_a.  fp32 subtraction is monotone (rounding a monotone function is monotone),
// so where s_a < lo_a, fl(p_a - s_a) >= fl(lo_a - s_a) = e_a, and likewise on the other side: |fl(p_a - s_a)| >= e_a on every axis, with
// the differences exactly as nn_d2 forms them.  Squares and sums of non-negative terms are monotone as well, so evaluated by the SAME
// chain of roundings the sum of the e_a^2 could not exceed d2; the compiler may contract the two sums differently (which product is
// fused into which add), which moves either by at most three roundings, 3 * 2^-24 relative each: the factor 1 - 2^-16 (GRID_MARGIN of
// nn_grid.h) is a thousand times that.  Hence lb <= d2 for every row of the bucket -- with overflow too: an infinite e_a makes d2
// infinite.  Every row has d <= max, so in a skipped bucket d <= max <= lb <= d2 and min(d, d2) = d: the brute-force loop would not
// have changed it either, and (max, arg) stay what they are.  An opened bucket is walked in full with nn_d2 itself.  A bound that is
// too small only opens a bucket that did not need it.
//
// The fallback.  A cloud with a row that has a non-finite coordinate (there d2 is inf or NaN and the running minimum follows fminf's
// NaN rule, which a box cannot bound), or whose box the grid arithmetic cannot take (an extent that overflows), is walked by the plain
// loop of fps_kernel inside this kernel, with its distances in the same workspace: slow, and identical.  This is the GRID_ROWS mode of
// the neighbour index (nn_grid.hip).
#include "nn_tile.h"
#include "fps_grid.h"

rap_tuning_t g_rap_fps_grid_per = FPS_GRID_PER;     // tuning key 22
rap_tuning_t g_rap_fps_grid_block = 512;            // tuning key 23

// order-preserving map of a finite float onto unsigned integers, and back (as nn_grid.hip's)
__device__ __forceinline__ unsigned fps_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float fps_unkey(unsigned k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }

// (d, i) <- the better of (d, i) and (od, oi): larger distance, then the lower index
__device__ __forceinline__ void fps_better(float& d, int& i, float od, int oi) {
  const bool take = (od > d) | ((od == d) & (oi < i));      // selects, not branches: this sits on the critical path of every pick
  d = take ? od : d;
  i = take ? oi : i;
}
// one step of the reduction inside a row of 16 lanes: every lane combines with the lane a DPP control pairs it with
template <int CTRL>
__device__ __forceinline__ void fps_dpp_step(float& d, int& i) {
  const float od = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(d), CTRL, 0xF, 0xF, false));
  const int oi = __builtin_amdgcn_update_dpp(0, i, CTRL, 0xF, 0xF, false);
  fps_better(d, i, od, oi);
}
// the best (d, i) of the wave, in every lane; all 64 lanes call it.  fps_better picks the maximum of a total order, so any reduction
// tree gives the same pair.  Lanes ^1 and ^2 (quad permutes), then the mirrored half-row and the mirrored row: after four DPP steps the
// 16 lanes of a row agree; the four rows meet through v_readlane.  (__shfl_xor compiles to ds_bpermute_b32, an LDS round trip per value
// and step; with it a pick took 2.24 us at 20 000 points and 3.39 us at 100 000, with this 1.96 and 3.21 -- DESIGN.md section 7.7.)
__device__ __forceinline__ void fps_wave_best(float& d, int& i) {
  fps_dpp_step<0xB1>(d, i);        // quad_perm [1, 0, 3, 2]
  fps_dpp_step<0x4E>(d, i);        // quad_perm [2, 3, 0, 1]
  fps_dpp_step<0x141>(d, i);       // row_half_mirror
  fps_dpp_step<0x140>(d, i);       // row_mirror
  float rd = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(d), 0));
  int ri = __builtin_amdgcn_readlane(i, 0);
  fps_better(rd, ri, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(d), 16)), __builtin_amdgcn_readlane(i, 16));
  fps_better(rd, ri, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(d), 32)), __builtin_amdgcn_readlane(i, 32));
  fps_better(rd, ri, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(d), 48)), __builtin_amdgcn_readlane(i, 48));
  d = rd; i = ri;
}
// the best of the NW per-wave partials, read by every thread (LDS broadcasts): no second barrier, no second tree
template <int NW>
__device__ __forceinline__ void fps_block_best(const float* rd, const int* ri, float& d, int& i) {
  d = rd[0]; i = ri[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) fps_better(d, i, rd[w], ri[w]);
}

template <int T>
__global__ __launch_bounds__(T) void fps_grid_kernel(const float* __restrict__ pts, const int32_t* __restrict__ cloud_start /* (C) */,
                                                     const int32_t* __restrict__ cloud_len /* (C) */, const int32_t* __restrict__ Ks,
                                                     const int32_t* __restrict__ starts, int Kmax, long total, int per,
                                                     float4* __restrict__ sorted_all /* (total) */, float* __restrict__ dist_all /* (total) */,
                                                     int32_t* __restrict__ out /* (C,Kmax) */) {
  constexpr int NW = T / 64;                              // waves: 4, 8 or 16
  constexpr int MB = FPS_GRID_MAX_BUCKETS;
  constexpr int CH = MB / T;                              // buckets per thread in the scan
  __shared__ float blo[3][MB], bhi[3][MB];                // tight boxes (as keys while they are being built)
  __shared__ float bmax[MB];                              // largest running distance of the bucket (the sort's cursors during the build)
  __shared__ int barg[MB];                                // lowest original index that attains it
  __shared__ unsigned bstart[MB + 1];                     // first sorted row of every bucket
  __shared__ __align__(16) unsigned short queue[MB];      // the open buckets of one pick (the scan's partial sums during the build)
  __shared__ float red_d[2][16];
  __shared__ int red_i[2][16];
  __shared__ float red_box[6][16];
  __shared__ int red_bad[16];
  __shared__ int qn[2];
  __shared__ FpsGrid grid;

  const int c = blockIdx.x, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  long a_l = cloud_start[c], n_l = cloud_len[c];          // clamped to the rows the workspace was sized for: an inconsistent table
  a_l = a_l < 0 ? 0 : a_l > total ? total : a_l;          // cannot make the kernel index outside it
  n_l = n_l < 0 ? 0 : n_l > total - a_l ? total - a_l : n_l;
  const int a = (int)a_l, n = (int)n_l;
  int K = Ks[c];
  K = K < n ? K : n;                                      // pytorch3d: at most `length` points are selected
  K = K < Kmax ? K : Kmax;                                // (a K above k_max would leave its row of indices_out)
  int32_t* o = out + (size_t)c * Kmax;
  for (int i = tid; i < Kmax; i += T) o[i] = -1;          // padding, as pytorch3d
  if (n <= 0 || K <= 0) return;
  const float* p = pts + (size_t)a * 3;
  float4* sorted = sorted_all + a;
  float* d = dist_all + a;
  int last = starts[c];
  last = last < 0 ? 0 : (last >= n ? n - 1 : last);
  if (tid == 0) o[0] = last;
  if (K == 1) return;
  const float inf = __builtin_inff();

  // ---- bounding box; is every coordinate finite?
  {
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    int bad = 0;
    for (int i = tid; i < n; i += T) {
      const float x = p[(size_t)i * 3 + 0], y = p[(size_t)i * 3 + 1], z = p[(size_t)i * 3 + 2];
      if (!(fabsf(x) < inf && fabsf(y) < inf && fabsf(z) < inf)) { bad = 1; continue; }
      lo[0] = fminf(lo[0], x); hi[0] = fmaxf(hi[0], x);
      lo[1] = fminf(lo[1], y); hi[1] = fmaxf(hi[1], y);
      lo[2] = fminf(lo[2], z); hi[2] = fmaxf(hi[2], z);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
      for (int ax = 0; ax < 3; ++ax) {
        lo[ax] = fminf(lo[ax], __shfl_xor(lo[ax], off, 64));
        hi[ax] = fmaxf(hi[ax], __shfl_xor(hi[ax], off, 64));
      }
      bad |= __shfl_xor(bad, off, 64);
    }
    if (lane == 0) {
#pragma unroll
      for (int ax = 0; ax < 3; ++ax) { red_box[ax][wave] = lo[ax]; red_box[3 + ax][wave] = hi[ax]; }
      red_bad[wave] = bad;
    }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < NW; ++w) {
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) { lo[ax] = fminf(lo[ax], red_box[ax][w]); hi[ax] = fmaxf(hi[ax], red_box[3 + ax][w]); }
        bad |= red_bad[w];
      }
      FpsGrid g = fps_grid_dims(lo, hi, n, per, MB);
      if (bad) g.buckets = 0;
      grid = g;
      qn[0] = 0; qn[1] = 0;
    }
    __syncthreads();
  }
  const FpsGrid g = grid;
  const int nb = g.buckets;

  if (nb == 0) {
    // ---- the plain loop of fps_kernel (fps.hip), T threads wide: same distance, same running minimum, same winner
    for (int i = tid; i < n; i += T) d[i] = inf;
    __syncthreads();
    for (int k = 1; k < K; ++k) {
      const float lx = p[(size_t)last * 3 + 0], ly = p[(size_t)last * 3 + 1], lz = p[(size_t)last * 3 + 2];
      float bd = -1.f;
      int bi = 0x7fffffff;
      for (int i = tid; i < n; i += T) {
        const float nd = fminf(d[i], nn_d2(p[(size_t)i * 3 + 0], p[(size_t)i * 3 + 1], p[(size_t)i * 3 + 2], lx, ly, lz));
        d[i] = nd;
        if (nd > bd) { bd = nd; bi = i; }                 // strided ascending i: the lane's first maximum
      }
      fps_wave_best(bd, bi);
      if (lane == 0) { red_d[k & 1][wave] = bd; red_i[k & 1][wave] = bi; }
      __syncthreads();
      float vd;
      int vi;
      fps_block_best<NW>(red_d[k & 1], red_i[k & 1], vd, vi);
      last = vi;
      if (tid == 0) o[k] = vi;
    }
    return;
  }

  // ---- counting sort into buckets, tight boxes and lowest indices on the way
  unsigned* cursor = (unsigned*)bmax;
  unsigned* part = (unsigned*)queue;                      // T partial sums: 4 T bytes <= 2 MB bytes
  unsigned* klo[3] = {(unsigned*)blo[0], (unsigned*)blo[1], (unsigned*)blo[2]};
  unsigned* khi[3] = {(unsigned*)bhi[0], (unsigned*)bhi[1], (unsigned*)bhi[2]};
  for (int b = tid; b < nb; b += T) {
    bstart[b] = 0u; barg[b] = 0x7fffffff;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) { klo[ax][b] = 0xffffffffu; khi[ax][b] = 0u; }
  }
  __syncthreads();
  for (int i = tid; i < n; i += T) {
    const float x = p[(size_t)i * 3 + 0], y = p[(size_t)i * 3 + 1], z = p[(size_t)i * 3 + 2];
    const int b = fps_grid_bucket(g, x, y, z);            // in [0, nb): every axis is clamped into the grid
    atomicAdd(&bstart[b], 1u);
    atomicMin(&barg[b], i);
    const unsigned kx = fps_key(x), ky = fps_key(y), kz = fps_key(z);
    atomicMin(&klo[0][b], kx); atomicMax(&khi[0][b], kx);
    atomicMin(&klo[1][b], ky); atomicMax(&khi[1][b], ky);
    atomicMin(&klo[2][b], kz); atomicMax(&khi[2][b], kz);
  }
  __syncthreads();
  {                                                       // exclusive scan of the counts: CH consecutive buckets per thread
    unsigned loc = 0;
#pragma unroll
    for (int j = 0; j < CH; ++j) { const int b = tid * CH + j; loc += b < nb ? bstart[b] : 0u; }
    part[tid] = loc;
    __syncthreads();
    for (int off = 1; off < T; off <<= 1) {
      const unsigned v = tid >= off ? part[tid - off] : 0u;
      __syncthreads();
      part[tid] += v;
      __syncthreads();
    }
    unsigned run = part[tid] - loc;
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const int b = tid * CH + j;
      if (b < nb) { const unsigned cnt = bstart[b]; bstart[b] = run; cursor[b] = run; run += cnt; }
    }
    if (tid == 0) bstart[nb] = (unsigned)n;
  }
  __syncthreads();
  for (int i = tid; i < n; i += T) {
    const float x = p[(size_t)i * 3 + 0], y = p[(size_t)i * 3 + 1], z = p[(size_t)i * 3 + 2];
    const unsigned pos = atomicAdd(&cursor[fps_grid_bucket(g, x, y, z)], 1u);      // < n: the cursors of a bucket end at the next one's start
    sorted[pos] = make_float4(x, y, z, __int_as_float(i));
    d[pos] = inf;
  }
  __syncthreads();
  for (int b = tid; b < nb; b += T) {
    const bool empty = bstart[b + 1] == bstart[b];
    bmax[b] = empty ? -inf : inf;                         // (the cursors are done with)
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
      const float l = fps_unkey(klo[ax][b]), h = fps_unkey(khi[ax][b]);
      blo[ax][b] = empty ? inf : l; bhi[ax][b] = empty ? -inf : h;
    }
  }
  __syncthreads();

  // ---- the picks
  for (int k = 1; k < K; ++k) {
    const int par = k & 1;
    const float sx = p[(size_t)last * 3 + 0], sy = p[(size_t)last * 3 + 1], sz = p[(size_t)last * 3 + 2];
    for (int b = tid; b < nb; b += T) {
      const float lb = fps_grid_lower_bound(blo[0][b], blo[1][b], blo[2][b], bhi[0][b], bhi[1][b], bhi[2][b], sx, sy, sz);
      if (!fps_grid_skip(lb, bmax[b])) queue[atomicAdd(&qn[par], 1)] = (unsigned short)b;      // at most nb entries
    }
    __syncthreads();
    const int nq = qn[par];
    if (tid == 0) qn[par ^ 1] = 0;                        // the next pick's counter: nobody reads or adds to it before the next barrier
    for (int q = wave; q < nq; q += NW) {
      const int b = queue[q];
      const unsigned r1 = bstart[b + 1];
      float bd = -inf;
      int bi = 0x7fffffff;
      for (unsigned r = bstart[b] + lane; r < r1; r += 64) {
        const float4 row = sorted[r];
        const float od = d[r];
        const float nd = fminf(od, nn_d2(row.x, row.y, row.z, sx, sy, sz));
        if (nd != od) d[r] = nd;
        fps_better(bd, bi, nd, __float_as_int(row.w));
      }
      fps_wave_best(bd, bi);
      if (lane == 0) { bmax[b] = bd; barg[b] = bi; }
    }
    __syncthreads();
    float bd = -inf;
    int bi = 0x7fffffff;
    for (int b = tid; b < nb; b += T) fps_better(bd, bi, bmax[b], barg[b]);
    fps_wave_best(bd, bi);
    if (lane == 0) { red_d[par][wave] = bd; red_i[par][wave] = bi; }
    __syncthreads();
    float vd;
    int vi;
    fps_block_best<NW>(red_d[par], red_i[par], vd, vi);     // every thread folds the partials: no fourth barrier
    last = vi;
    if (tid == 0) o[k] = vi;
  }
}

void fps_grid_params(int* per, int* max_buckets, int* block) {
  *per = g_rap_fps_grid_per; *max_buckets = FPS_GRID_MAX_BUCKETS; *block = g_rap_fps_grid_block;
}

int launch_fps_grid(hipStream_t stream, const float* pts, long total, const int32_t* cloud_start, const int32_t* cloud_len, const int32_t* Ks,
                    const int32_t* starts, int C, int Kmax, void* ws, int32_t* out) {
  if (C <= 0 || Kmax <= 0) return RAP_OK;
  float4* sorted = (float4*)ws;
  float* dist = (float*)((char*)ws + fps_grid_dist_offset(total));
  const int per = g_rap_fps_grid_per, block = g_rap_fps_grid_block;
  if (block == 256)
    hipLaunchKernelGGL(fps_grid_kernel<256>, dim3(C), dim3(256), 0, stream, pts, cloud_start, cloud_len, Ks, starts, Kmax, total, per, sorted, dist, out);
  else if (block == 512)
    hipLaunchKernelGGL(fps_grid_kernel<512>, dim3(C), dim3(512), 0, stream, pts, cloud_start, cloud_len, Ks, starts, Kmax, total, per, sorted, dist, out);
  else
    hipLaunchKernelGGL(fps_grid_kernel<1024>, dim3(C), dim3(1024), 0, stream, pts, cloud_start, cloud_len, Ks, starts, Kmax, total, per, sorted, dist, out);
  RAP_LAUNCH_CHECK();
  return RAP_OK;
}
