// Exact nearest neighbours over a uniform grid: a second search path for the batched ICP (icp.hip) and an entry point of its own.
// For the same inputs it returns, bit for bit, what the brute-force kernels return: the same fp32 distance (nn_d2, nn_tile.h), the same
// winner (smallest (d2, index) = "strict <, first arg-min"), and for ICP the same query head and epilogue (icp.h) over the same items.
//
// The index.  Y never moves during an ICP call, so it is built once per call for all K problems, on the device, without a host read:
//   nn_grid_plan_kernel     clamps every y segment (nn_segment); a problem whose segment equals an earlier one shares that problem's
//                           grid; the others take rows and cells from budgets of NY rows and NY + 8 K cells, in problem order.  A
//                           problem that no longer fits (overlapping but different segments can ask for more than NY rows) is searched
//                           by a plain loop over its rows instead: slow, and still exact
//   nn_grid_bbox_kernel     bounding box of the rows whose coordinates are all finite (integer atomic min / max of order-preserving keys)
//   nn_grid_dims_kernel     cubic cells of edge h ~ (volume / yn)^(1/3) (area / length for flat / collinear clouds; a degenerate axis gets
//                           one cell), h grown until every dimension is <= 1024 and the cell count <= yn + 8
//   nn_grid_count_kernel    cell of every row, integer atomic histogram
//   nn_grid_scan_*          exclusive scan of the counts -> first sorted row of every cell
//   nn_grid_scatter_kernel  float4 (x, y, z, index in the segment) of every row into its cell
// A counting sort, not a radix sort: the order of rows INSIDE a cell depends on the atomics, and nothing depends on that order (the tie
// rule below compares indices).  Its scratch is a function of NY and K alone, so the workspace query is host arithmetic.  Rows with a
// non-finite coordinate stay out: in the brute-force kernels their d2 is inf or NaN and `d2 < best` is false.
//
// The query (grid_search).  One query per lane; cell of the query's projection q_c onto the box; shells of Chebyshev radius r = 0, 1, ...
// around it; per (y, z) row of a shell the cells are consecutive, so a row is one run of sorted candidates, 16 bytes each.  After shell r
// every unvisited point p lies, on some axis a, in a cell beyond a face of the visited cube, i.e. in the part B of the box behind that
// face.  B is a box, so |p - q|^2 >= dist(q, B)^2 = (|o_a| + h s_a)^2 + sum over the other axes of o_b^2, with o = q - q_c (zero on an axis
// where q is inside the box; where it is outside, the faces that have grid behind them lie on the far side of q_c, so the two lengths
// add) and s_a the distance in cells from q_c to that face.  The bound is the smallest such value over the faces that have grid behind
// them.  For a query inside the box it is the distance to the nearest face of the cube; for one far outside it carries the cross term
// 2 |o_a| h s_a, which is what lets a bad initial pose prune as well as a good one (|p - q_c|^2 + |q - q_c|^2 alone does not).
// The walk stops when that bound exceeds the best distance found (or the gate), or when the cube covers the grid.
// Rounding.  Cells come from t = fl(fl(p - lo) / h), so a computed t is off by at most 2^-23 relative, i.e. 2^-13 cells at t <= 1024;
// "p is outside the cube" and s are statements about computed t's, so s is reduced by 2^-10 cells (GRID_SLACK: the two t's and the
// subtraction together are off by less than 2^-11).  The bound itself is then at most eight roundings away from exact and `best` six from the
// exact distance: 14 * 2^-24 < 2^-20 relative; the bound is scaled by 1 - 2^-16 (GRID_MARGIN), sixteen times that.  A smaller bound only
// costs another shell.  The comparison is strict, so a tied candidate with a lower index in an unvisited cell cannot be missed either.
// The k-best walk over the same index (the k nearest rows, normals, outlier removal) is nn_knn.hip; nn_grid.h holds what the two share.
// grid_search itself is in nn_grid_search.h, for the edge query of scene_refine.hip as well.
#include "icp.h"
#include "nn_grid_search.h"

#define GRID_MAX_DIM 1024
#define GRID_SCAN_CHUNK 2048
#define GRID_BUILD_BLOCKS 128

NnGridWs nn_grid_carve(Carver& c, long NY, int K) {
  NnGridWs w;
  w.n_cells = (size_t)NY + 8 * (size_t)K + 1;
  w.grids = c.take((size_t)K * sizeof(NnGrid));
  w.box = (unsigned*)c.take((size_t)K * 8 * sizeof(unsigned));
  w.cell_start = (unsigned*)c.take(w.n_cells * sizeof(unsigned));
  w.cursor = (unsigned*)c.take(w.n_cells * sizeof(unsigned));
  w.row_cell = (int32_t*)c.take((size_t)NY * sizeof(int32_t));
  w.sorted = c.take((size_t)NY * sizeof(float4));
  w.block_sum = (unsigned*)c.take((w.n_cells / GRID_SCAN_CHUNK + 1) * sizeof(unsigned));
  return w;
}

// order-preserving map of a finite float onto unsigned integers, and back
__device__ __forceinline__ unsigned grid_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float grid_unkey(unsigned k) { return __builtin_bit_cast(float, k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }

__global__ __launch_bounds__(256) void nn_grid_plan_kernel(const int32_t* __restrict__ y_seg, int K, long NY, NnGrid* __restrict__ grids,
                                                           unsigned* __restrict__ box) {
  if (blockIdx.x != 0) return;
  for (int k = threadIdx.x; k < K; k += 256) {
    int ys, yn;
    nn_segment(y_seg, k, NY, ys, yn);
    grids[k].y_start = ys; grids[k].y_len = yn;
#pragma unroll
    for (int a = 0; a < 3; ++a) { box[(size_t)k * 8 + a] = 0xffffffffu; box[(size_t)k * 8 + 3 + a] = 0u; }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < K; k += 256) {
    const int ys = grids[k].y_start, yn = grids[k].y_len;
    int owner = k;
    if (yn > 0)
      for (int j = 0; j < k; ++j)
        if (grids[j].y_len == yn && grids[j].y_start == ys) { owner = j; break; }
    grids[k].owner = owner;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  long used = 0;
  int rank = 0;
  for (int k = 0; k < K; ++k) {
    NnGrid g = grids[k];
    int base = 0;
    if (g.y_len <= 0) {
      g.mode = GRID_NONE; g.cell_base = 0;
    } else if (g.owner != k) {
      g.mode = grids[g.owner].mode; g.cell_base = grids[g.owner].cell_base; base = grids[g.owner].row_base;
    } else if (used + g.y_len <= NY) {
      g.mode = GRID_CELLS; g.cell_base = (int)used + 8 * rank; base = (int)used;      // at most y_len + 8 cells each: they never meet
      used += g.y_len; ++rank;
    } else {
      g.mode = GRID_ROWS; g.cell_base = 0;
    }
    g.lo[0] = g.lo[1] = g.lo[2] = g.hi[0] = g.hi[1] = g.hi[2] = 0.f;
    g.h = 1.f; g.row_base = base;
    g.dims[0] = g.dims[1] = g.dims[2] = 1;
    grids[k] = g;
  }
}

__global__ __launch_bounds__(256) void nn_grid_zero_kernel(unsigned* __restrict__ a, unsigned* __restrict__ b, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) { a[i] = 0u; b[i] = 0u; }
}

// blockIdx.y = problem; only the owner of a grid walks its rows
__global__ __launch_bounds__(256) void nn_grid_bbox_kernel(const float* __restrict__ Y, const NnGrid* __restrict__ grids, unsigned* __restrict__ box) {
  const int k = blockIdx.y;
  const int mode = grids[k].mode, owner = grids[k].owner, ys = grids[k].y_start, yn = grids[k].y_len;
  if (mode != GRID_CELLS || owner != k) return;
  unsigned lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
  for (int i = blockIdx.x * 256 + threadIdx.x; i < yn; i += gridDim.x * 256) {
    const float* p = Y + ((size_t)ys + i) * 3;
    const float x = p[0], y = p[1], z = p[2];
    if (!grid_finite(x, y, z)) continue;
    const unsigned kx = grid_key(x), ky = grid_key(y), kz = grid_key(z);
    lo[0] = min(lo[0], kx); hi[0] = max(hi[0], kx);
    lo[1] = min(lo[1], ky); hi[1] = max(hi[1], ky);
    lo[2] = min(lo[2], kz); hi[2] = max(hi[2], kz);
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo[a] = min(lo[a], (unsigned)__shfl_xor((int)lo[a], o, 64));
      hi[a] = max(hi[a], (unsigned)__shfl_xor((int)hi[a], o, 64));
    }
  }
  if ((threadIdx.x & 63) == 0 && lo[0] <= hi[0]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { atomicMin(box + (size_t)k * 8 + a, lo[a]); atomicMax(box + (size_t)k * 8 + 3 + a, hi[a]); }
  }
}

// cells along one axis of extent e at cell edge h (1 for an axis without extent), as a float: it may exceed GRID_MAX_DIM
__device__ __forceinline__ float grid_axis_cells(float e, float h) { return e > 0.f ? floorf(e / h) + 1.f : 1.f; }

__global__ __launch_bounds__(256) void nn_grid_dims_kernel(NnGrid* __restrict__ grids, const unsigned* __restrict__ box, int K) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= K) return;
  NnGrid* g = grids + k;
  if (g->mode != GRID_CELLS) return;
  const unsigned* b = box + (size_t)g->owner * 8;
  if (b[0] > b[3]) return;                           // no finite row: one cell that stays empty (set by the plan kernel)
  const float inf = __builtin_inff();
  const float lx = grid_unkey(b[0]), ly = grid_unkey(b[1]), lz = grid_unkey(b[2]);
  const float ux = grid_unkey(b[3]), uy = grid_unkey(b[4]), uz = grid_unkey(b[5]);
  const float ex = ux - lx, ey = uy - ly, ez = uz - lz;
  const float emax = fmaxf(ex, fmaxf(ey, ez));
  const int nd = (ex > 0.f) + (ey > 0.f) + (ez > 0.f);
  // cells ~ points over the axes that have an extent; then h grows by a quarter at a time until the grid fits its budget.  Once h
  // exceeds every extent all dimensions are 1, which 64 steps from emax / 1024 reach (1.25^64 > 1e6).
  const int yn = g->y_len;
  const double per = (ex > 0.f ? (double)ex : 1.0) * (ey > 0.f ? (double)ey : 1.0) * (ez > 0.f ? (double)ez : 1.0) / (double)yn;
  const float perf = (float)per;                     // a heuristic: its rounding (or its underflow: the next line) does not matter
  float h = nd == 3 ? __builtin_exp2f(__builtin_log2f(perf) * (1.f / 3.f)) : nd == 2 ? sqrtf(perf) : perf;
  h = fmaxf(h, emax / 1023.5f);
  int dx = 1, dy = 1, dz = 1;
  bool fits = false;
  if (nd > 0 && emax < inf && h > 0.f && h < inf) {
    for (int step = 0; step < 64 && !fits; ++step) {
      const float fx = grid_axis_cells(ex, h), fy = grid_axis_cells(ey, h), fz = grid_axis_cells(ez, h);
      if (fx <= (float)GRID_MAX_DIM && fy <= (float)GRID_MAX_DIM && fz <= (float)GRID_MAX_DIM) {
        dx = (int)fx; dy = (int)fy; dz = (int)fz;
        fits = (long long)dx * dy * dz <= (long long)yn + 8;
      }
      if (!fits) h *= 1.25f;
    }
  }
  if (!fits || !(h < inf)) { dx = dy = dz = 1; h = 1.f; }
  g->lo[0] = lx; g->lo[1] = ly; g->lo[2] = lz;
  g->hi[0] = ux; g->hi[1] = uy; g->hi[2] = uz;
  g->h = h;
  g->dims[0] = dx; g->dims[1] = dy; g->dims[2] = dz;
}

__global__ __launch_bounds__(256) void nn_grid_count_kernel(const float* __restrict__ Y, const NnGrid* __restrict__ grids,
                                                            unsigned* __restrict__ count,
                                                            int32_t* __restrict__ row_cell) {
  const int k = blockIdx.y;
  const NnGrid g = grids[k];
  if (g.mode != GRID_CELLS || g.owner != k) return;
  const int base = g.row_base;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < g.y_len; i += gridDim.x * 256) {
    const float* p = Y + ((size_t)g.y_start + i) * 3;
    const float x = p[0], y = p[1], z = p[2];
    int c = -1;
    if (grid_finite(x, y, z)) {
      const int cx = grid_cell(grid_t(x, g.lo[0], g.h), g.dims[0]), cy = grid_cell(grid_t(y, g.lo[1], g.h), g.dims[1]),
                cz = grid_cell(grid_t(z, g.lo[2], g.h), g.dims[2]);
      c = g.cell_base + cx + g.dims[0] * (cy + g.dims[1] * cz);
      atomicAdd(count + c, 1u);
    }
    row_cell[(size_t)base + i] = c;
  }
}

// exclusive scan of n counts in place, in chunks of GRID_SCAN_CHUNK = 256 threads x 8: chunk sums, their scan, the chunks
__global__ __launch_bounds__(256) void nn_grid_scan_sums_kernel(const unsigned* __restrict__ v, size_t n, unsigned* __restrict__ block_sum) {
  __shared__ unsigned red[4];
  const size_t i0 = (size_t)blockIdx.x * GRID_SCAN_CHUNK + (size_t)threadIdx.x * 8;
  unsigned s = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) s += i0 + j < n ? v[i0 + j] : 0u;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += (unsigned)__shfl_xor((int)s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) block_sum[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
// block-wide exclusive scan of one value per thread (256 threads); `total` receives the sum
__device__ __forceinline__ unsigned grid_block_scan(unsigned v, unsigned* sh, unsigned& total) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const unsigned add = t >= o ? sh[t - o] : 0u;
    __syncthreads();
    sh[t] += add;
    __syncthreads();
  }
  const unsigned incl = sh[t];
  total = sh[255];
  __syncthreads();
  return incl - v;
}
__global__ __launch_bounds__(256) void nn_grid_scan_blocks_kernel(unsigned* __restrict__ block_sum, int nb) {
  __shared__ unsigned sh[256];
  unsigned carry = 0;
  for (int b0 = 0; b0 < nb; b0 += 256) {
    const int b = b0 + threadIdx.x;
    unsigned total;
    const unsigned ex = grid_block_scan(b < nb ? block_sum[b] : 0u, sh, total);
    if (b < nb) block_sum[b] = carry + ex;
    carry += total;
  }
}
__global__ __launch_bounds__(256) void nn_grid_scan_chunks_kernel(unsigned* __restrict__ v, size_t n, const unsigned* __restrict__ block_sum) {
  __shared__ unsigned sh[256];
  const size_t i0 = (size_t)blockIdx.x * GRID_SCAN_CHUNK + (size_t)threadIdx.x * 8;
  unsigned c[8], s = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) { c[j] = i0 + j < n ? v[i0 + j] : 0u; s += c[j]; }
  unsigned total;
  unsigned run = block_sum[blockIdx.x] + grid_block_scan(s, sh, total);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (i0 + j < n) v[i0 + j] = run;
    run += c[j];
  }
}

__global__ __launch_bounds__(256) void nn_grid_scatter_kernel(const float* __restrict__ Y, const NnGrid* __restrict__ grids,
                                                              const int32_t* __restrict__ row_cell,
                                                              const unsigned* __restrict__ cell_start, unsigned* __restrict__ cursor,
                                                              float4* __restrict__ sorted, long NY) {
  const int k = blockIdx.y;
  const int mode = grids[k].mode, owner = grids[k].owner, ys = grids[k].y_start, yn = grids[k].y_len;
  if (mode != GRID_CELLS || owner != k) return;
  const int base = grids[k].row_base;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < yn; i += gridDim.x * 256) {
    const int c = row_cell[(size_t)base + i];
    if (c < 0) continue;
    const unsigned pos = cell_start[c] + atomicAdd(cursor + c, 1u);
    if ((long)pos >= NY) continue;                   // cannot happen (the counts were taken from the same row_cell); never write outside
    const float* p = Y + ((size_t)ys + i) * 3;
    sorted[pos] = make_float4(p[0], p[1], p[2], __int_as_float(i));
  }
}

// the two ICP query kernels with the grid search in place of the tiled one: same items, same head, same epilogue
__global__ __launch_bounds__(ICP_TILE) void icp_grid_query_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                                  const NnWork* __restrict__ items, const float* __restrict__ R,
                                                                  const float* __restrict__ T, const int32_t* __restrict__ done, float gate,
                                                                  const NnGrid* __restrict__ grids, const unsigned* __restrict__ cell_start,
                                                                  const float4* __restrict__ sorted, IcpPartial* __restrict__ partials) {
  __shared__ double red_m[ICP_TILE / 64][ICP_NMOM];
  __shared__ int red_n[ICP_TILE / 64];
  ICP_QUERY_BEGIN(X, items, R, T, done);
  float best;
  int besti;
  grid_search(grids[prob], Y, cell_start, sorted, px, py, pz, grid_gate2(gate), best, besti);
  icp_moments(active, besti, best, gate, x0, x1, x2, Y, w.y_start, red_m, red_n, partials + blockIdx.x);
}

__global__ __launch_bounds__(ICP_TILE) void icp_plane_grid_query_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                                        const float* __restrict__ Yn, const NnWork* __restrict__ items,
                                                                        const float* __restrict__ R, const float* __restrict__ T,
                                                                        const int32_t* __restrict__ done, float gate,
                                                                        const NnGrid* __restrict__ grids, const unsigned* __restrict__ cell_start,
                                                                        const float4* __restrict__ sorted, IcpPlanePartial* __restrict__ partials) {
  __shared__ double red_m[ICP_TILE / 64][ICP_PLANE_NMOM];
  __shared__ int red_n[ICP_TILE / 64];
  ICP_QUERY_BEGIN(X, items, R, T, done);
  float best;
  int besti;
  grid_search(grids[prob], Y, cell_start, sorted, px, py, pz, grid_gate2(gate), best, besti);
  icp_plane_moments<RAP_LOSS_NONE>(active, besti, best, gate, px, py, pz, Y, Yn, w.y_start, red_m, red_n, partials + blockIdx.x);
}

// ... and the robust call's (rap_icp_plane_grid_robust): the weighted epilogue, the optional per-row weights
template <int LOSS>
__global__ __launch_bounds__(ICP_TILE) void icp_plane_grid_query_robust_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                                               const float* __restrict__ Yn, const NnWork* __restrict__ items,
                                                                               const float* __restrict__ R, const float* __restrict__ T,
                                                                               const int32_t* __restrict__ done, float gate,
                                                                               const NnGrid* __restrict__ grids,
                                                                               const unsigned* __restrict__ cell_start,
                                                                               const float4* __restrict__ sorted, double scale,
                                                                               float* __restrict__ weights, IcpPlaneWPartial* __restrict__ partials) {
  __shared__ double red_m[ICP_TILE / 64][ICP_PLANE_WMOM];
  __shared__ int red_n[ICP_TILE / 64];
  ICP_QUERY_BEGIN(X, items, R, T, done);
  float best;
  int besti;
  grid_search(grids[prob], Y, cell_start, sorted, px, py, pz, grid_gate2(gate), best, besti);
  icp_plane_moments<LOSS>(active, besti, best, gate, px, py, pz, Y, Yn, w.y_start, red_m, red_n, partials + blockIdx.x, scale, weights, qi);
}

// items of 256 queries of one problem, all of a problem or none
__global__ void nn_grid_items_kernel(const int32_t* __restrict__ x_seg, const int32_t* __restrict__ y_seg, int K, long NX, long NY,
                                     NnWork* __restrict__ items, int max_items) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int n = 0;
  for (int k = 0; k < K; ++k) {
    int xs, xn, ys, yn;
    nn_segment(x_seg, k, NX, xs, xn);
    nn_segment(y_seg, k, NY, ys, yn);
    nn_emit_items_whole(items, n, max_items, xs, xn, ys, yn, k);
  }
  nn_zero_items(items, n, max_items);
}

// idx_out = row in Y of the nearest neighbour of x R + T (x where R is NULL), d2_out its squared distance; -1 / inf where there is none
__global__ __launch_bounds__(ICP_TILE) void nn_grid_query_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                                 const NnWork* __restrict__ items, const float* __restrict__ R,
                                                                 const float* __restrict__ T, float gate, const NnGrid* __restrict__ grids,
                                                                 const unsigned* __restrict__ cell_start, const float4* __restrict__ sorted,
                                                                 int32_t* __restrict__ idx_out, float* __restrict__ d2_out) {
  const NnWork w = items[blockIdx.x];
  const int q = w.q0 + threadIdx.x;
  if (q >= w.x_len) return;
  const int prob = w.pad0;
  const size_t qi = (size_t)w.x_start + q;
  float qx = X[qi * 3 + 0], qy = X[qi * 3 + 1], qz = X[qi * 3 + 2];
  if (R) icp_apply(R + (size_t)prob * 9, T + (size_t)prob * 3, qx, qy, qz, qx, qy, qz);
  float best;
  int besti;
  grid_search(grids[prob], Y, cell_start, sorted, qx, qy, qz, grid_gate2(gate), best, besti);
  const bool found = besti >= 0 && (!(gate > 0.f) || sqrtf(best) <= gate);
  idx_out[qi] = found ? w.y_start + besti : -1;
  d2_out[qi] = found ? best : __builtin_inff();
}

int launch_nn_grid_build(hipStream_t stream, const float* Y, const int32_t* y_seg, int K, long NY, const NnGridWs& g) {
  NnGrid* grids = (NnGrid*)g.grids;
  const unsigned gx = (unsigned)((NY + 255) / 256 < GRID_BUILD_BLOCKS ? (NY + 255) / 256 : GRID_BUILD_BLOCKS);
  const unsigned nb = (unsigned)((g.n_cells + GRID_SCAN_CHUNK - 1) / GRID_SCAN_CHUNK);
  hipLaunchKernelGGL(nn_grid_plan_kernel, dim3(1), dim3(256), 0, stream, y_seg, K, NY, grids, g.box);
  RAP_LAUNCH_CHECK();
  hipLaunchKernelGGL(nn_grid_zero_kernel, dim3(nb < 1024 ? nb : 1024), dim3(256), 0, stream, g.cell_start, g.cursor, g.n_cells);
  RAP_LAUNCH_CHECK();
  hipLaunchKernelGGL(nn_grid_bbox_kernel, dim3(gx, K), dim3(256), 0, stream, Y, (const NnGrid*)grids, g.box);
  RAP_LAUNCH_CHECK();
  hipLaunchKernelGGL(nn_grid_dims_kernel, dim3((K + 255) / 256), dim3(256), 0, stream, grids, (const unsigned*)g.box, K);
  RAP_LAUNCH_CHECK();
  hipLaunchKernelGGL(nn_grid_count_kernel, dim3(gx, K), dim3(256), 0, stream, Y, (const NnGrid*)grids, g.cell_start, g.row_cell);
  RAP_LAUNCH_CHECK();
  hipLaunchKernelGGL(nn_grid_scan_sums_kernel, dim3(nb), dim3(256), 0, stream, (const unsigned*)g.cell_start, g.n_cells, g.block_sum);
  RAP_LAUNCH_CHECK();
  hipLaunchKernelGGL(nn_grid_scan_blocks_kernel, dim3(1), dim3(256), 0, stream, g.block_sum, (int)nb);
  RAP_LAUNCH_CHECK();
  hipLaunchKernelGGL(nn_grid_scan_chunks_kernel, dim3(nb), dim3(256), 0, stream, g.cell_start, g.n_cells, (const unsigned*)g.block_sum);
  RAP_LAUNCH_CHECK();
  hipLaunchKernelGGL(nn_grid_scatter_kernel, dim3(gx, K), dim3(256), 0, stream, Y, (const NnGrid*)grids, (const int32_t*)g.row_cell,
                     (const unsigned*)g.cell_start, g.cursor, (float4*)g.sorted, NY);
  RAP_LAUNCH_CHECK();
  return RAP_OK;
}

template <int LOSS>
static void icp_plane_grid_query_robust(hipStream_t stream, const IcpCall& c) {
  const NnGridWs& g = *c.grid;
  hipLaunchKernelGGL(icp_plane_grid_query_robust_kernel<LOSS>, dim3((unsigned)nn_max_items(c.NX, c.K)), dim3(ICP_TILE), 0, stream, c.X, c.Y,
                     c.Y_normals, (const NnWork*)c.items, (const float*)c.R, (const float*)c.T, (const int32_t*)c.done, c.gate,
                     (const NnGrid*)g.grids, (const unsigned*)g.cell_start, (const float4*)g.sorted, (double)c.loss_scale, c.weights,
                     (IcpPlaneWPartial*)c.partials);
}

int launch_icp_grid_query(hipStream_t stream, const IcpCall& c) {
  const NnGridWs& g = *c.grid;
  const dim3 grid((unsigned)nn_max_items(c.NX, c.K));
  if (c.robust) {
    RAP_LOSS_DISPATCH(c.loss, icp_plane_grid_query_robust, stream, c);
  } else if (c.Y_normals)
    hipLaunchKernelGGL(icp_plane_grid_query_kernel, grid, dim3(ICP_TILE), 0, stream, c.X, c.Y, c.Y_normals, (const NnWork*)c.items,
                       (const float*)c.R, (const float*)c.T, (const int32_t*)c.done, c.gate, (const NnGrid*)g.grids,
                       (const unsigned*)g.cell_start, (const float4*)g.sorted, (IcpPlanePartial*)c.partials);
  else
    hipLaunchKernelGGL(icp_grid_query_kernel, grid, dim3(ICP_TILE), 0, stream, c.X, c.Y, (const NnWork*)c.items, (const float*)c.R,
                       (const float*)c.T, (const int32_t*)c.done, c.gate, (const NnGrid*)g.grids, (const unsigned*)g.cell_start,
                       (const float4*)g.sorted, (IcpPartial*)c.partials);
  RAP_LAUNCH_CHECK();
  return RAP_OK;
}

int launch_nn_grid_items(hipStream_t stream, const int32_t* x_seg, const int32_t* y_seg, int K, long NX, long NY, NnWork* items) {
  hipLaunchKernelGGL(nn_grid_items_kernel, dim3(1), dim3(64), 0, stream, x_seg, y_seg, K, NX, NY, items, (int)nn_max_items(NX, K));
  RAP_LAUNCH_CHECK();
  return RAP_OK;
}

int launch_nearest_neighbors(hipStream_t stream, const float* X, const int32_t* x_seg, const float* Y, const int32_t* y_seg, int K, long NX,
                             long NY, const float* R, const float* T, float gate, int32_t* idx_out, float* d2_out, NnWork* items,
                             const NnGridWs& g) {
  const int max_items = (int)nn_max_items(NX, K);
  int rc = launch_nn_grid_items(stream, x_seg, y_seg, K, NX, NY, items);
  if (rc) return rc;
  rc = launch_nn_grid_build(stream, Y, y_seg, K, NY, g);
  if (rc) return rc;
  hipLaunchKernelGGL(nn_grid_query_kernel, dim3(max_items), dim3(ICP_TILE), 0, stream, X, Y, (const NnWork*)items, R, T, gate,
                     (const NnGrid*)g.grids, (const unsigned*)g.cell_start, (const float4*)g.sorted, idx_out, d2_out);
  RAP_LAUNCH_CHECK();
  return RAP_OK;
}
