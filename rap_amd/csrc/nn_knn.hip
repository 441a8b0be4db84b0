// The k nearest rows over the uniform-grid index of nn_grid.hip: exact, and for the same inputs the neighbour sets of the brute-force
// kernels (normals.hip, outlier.hip) -- the k admissible rows with the smallest (d2, index), d2 = nn_d2 (nn_tile.h) and nothing else.
// Three entry points share one kernel: the k nearest rows themselves (rap_k_nearest_neighbors), the plane fit of normals.hip over them
// (rap_estimate_normals_grid) and the mean neighbour distance of outlier.hip's kernel 1 (rap_statistical_outliers_grid).
//
// The walk (grid_knn_search) is grid_search's: the query's projection onto the box, Chebyshev shells around its cell, per (y, z) row of a
// shell one run of `sorted`, and after every shell the same lower bound lb2 on the distance of every unvisited row (GRID_SLACK and
// GRID_MARGIN as there; nn_grid.hip derives them).  What differs is what it keeps: not one best but the k smallest 64-bit keys
// (bits of d2) << 32 | index in the segment, whose order for d2 >= 0 IS the order of (d2, index).  A row is admitted when its d2 is
// finite and, with a radius, sqrtf(d2) <= radius -- normals.hip's rule, word for word.
// The stop rule.  One register, `limit`, holds the radius bound radius^2 (1 + 2^-16) (inf without a radius) until the list is full and
// the d2 of the list's worst key from then on; a candidate is looked at when d2 <= limit, and the walk ends after a shell when
// lb2 > limit, or when the cube covers the grid.  Strict: at lb2 == limit an unvisited row may tie the worst key's d2 with a lower index.
// A list that never fills ends with the cube covering the grid, or beyond the radius bound.  Exactness under rounding is nn_grid.hip's
// argument with `limit` in the place of `best`: lb2 is at most eight roundings below a true lower bound, the d2 it is compared with six
// from the exact distance, and GRID_MARGIN is sixteen times their sum.
// The list lives in LDS as [slot][lane] (normals.hip's layout: the lanes of a wave read different banks whatever slot each is at),
// unsorted while the walk runs: a candidate that beats the worst key replaces it, and one pass over the slots finds the new worst.
// Canonical order.  The order of rows inside a cell depends on the atomics of the counting sort, so the order of insertion does too.
// Before anything is read from the list it is sorted ascending by key (an insertion sort in the lane's own LDS column: at most 32
// keys, mostly in order already because near shells come first).  Every sum below runs in that order, which is what makes a result
// bit-identical from call to call and independent of what else is in the batch.
// Coherence.  A self-search (normals, outliers) takes its queries in `sorted` (cell) order and writes each result to the row's own
// index: the lanes of a wave then walk the same cells and branch alike.  Rows with a non-finite coordinate are not in `sorted`; the lane
// that has such a row's number writes its empty result.  No result depends on this order.
// A GRID_ROWS problem (no index: overlapping, unequal y segments) is searched row by row with the same list.
// The index is the one ICP gets, about one row per cell: fuller cells were measured and are no faster.
// No atomics here, no host read, no allocation, capturable.  DESIGN.md section 7.6 has the measurements.
#include "nn_grid.h"
#include "kabsch.h"

#define KNN_TILE NN_TILE

enum { KNN_ROWS_OUT = 0, KNN_NORMALS = 1, KNN_MEAN_DIST = 2 };      // what a block does with its lists

struct KnnParams {
  const float* X;             // the queries; == Y for a self-search
  const float* Y;
  const NnWork* items;
  const NnGrid* grids;
  const unsigned* cell_start;
  const float4* sorted;
  float radius;               // 0: none
  float r2_limit;             // d2 above this cannot pass sqrtf(d2) <= radius (inf without a radius)
  int k;
  int self;                   // X and Y are the same rows with the same segments: queries in cell order
  int32_t* idx_out; float* d2_out; int32_t* count_out;                   // KNN_ROWS_OUT: (NX,k), (NX,k), (NX,)
  const float* viewpoint; float* normals; float* eigenvalues;            // KNN_NORMALS: (K,3) or null, (NX,3), (NX,3) or null
  double* mean_dist;                                                     // KNN_MEAN_DIST: (NX,)
};

__host__ __device__ inline int knn_slots(int k) { return (k + 3) & ~3; }

// one lane's list: its column of the block's LDS array, and what the walk keeps in registers about it
struct KnnLane {
  unsigned long long* list;   // slot s is list[s * KNN_TILE]
  unsigned long long worst;   // the largest key of a full list
  float limit;                // see the stop rule
  float radius;
  int cnt, worst_slot, k, slots4;
};

// one candidate (idx: its index in the y segment) against the list
__device__ __forceinline__ void knn_consider(KnnLane& s, float qx, float qy, float qz, float px, float py, float pz, int idx) {
  const float d2 = nn_d2(qx, qy, qz, px, py, pz);
  if (d2 <= s.limit) {                                                 // false for NaN
    if (d2 < __builtin_inff() && (!(s.radius > 0.f) || sqrtf(d2) <= s.radius)) {
      const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)idx;
      bool rescan = false;
      if (s.cnt < s.k) {
        s.list[s.cnt * KNN_TILE] = key;
        rescan = ++s.cnt == s.k;
      } else if (key < s.worst) {
        s.list[s.worst_slot * KNN_TILE] = key;
        rescan = true;
      }
      if (rescan) {                                                    // the new worst key and the new limit: four reads in flight at a time
        s.worst = 0ull; s.worst_slot = 0;                              // (the padding slots hold 0, which no other key of a full list equals)
        for (int t = 0; t < s.slots4; t += 4) {
          const unsigned long long v0 = s.list[(t + 0) * KNN_TILE], v1 = s.list[(t + 1) * KNN_TILE], v2 = s.list[(t + 2) * KNN_TILE],
                                   v3 = s.list[(t + 3) * KNN_TILE];
          if (v0 > s.worst) { s.worst = v0; s.worst_slot = t; }
          if (v1 > s.worst) { s.worst = v1; s.worst_slot = t + 1; }
          if (v2 > s.worst) { s.worst = v2; s.worst_slot = t + 2; }
          if (v3 > s.worst) { s.worst = v3; s.worst_slot = t + 3; }
        }
        s.limit = __uint_as_float((unsigned)(s.worst >> 32));
      }
    }
  }
}

// the candidates sorted[a .. b), four 16-byte loads in flight at a time
__device__ __forceinline__ void knn_scan_run(KnnLane& s, const float4* __restrict__ sorted, unsigned a, unsigned b, float qx, float qy, float qz) {
  unsigned j = a;
  for (; j + 4 <= b; j += 4) {
    const float4 p0 = sorted[j], p1 = sorted[j + 1], p2 = sorted[j + 2], p3 = sorted[j + 3];
    knn_consider(s, qx, qy, qz, p0.x, p0.y, p0.z, __float_as_int(p0.w));
    knn_consider(s, qx, qy, qz, p1.x, p1.y, p1.z, __float_as_int(p1.w));
    knn_consider(s, qx, qy, qz, p2.x, p2.y, p2.z, __float_as_int(p2.w));
    knn_consider(s, qx, qy, qz, p3.x, p3.y, p3.z, __float_as_int(p3.w));
  }
  for (; j < b; ++j) {
    const float4 p = sorted[j];
    knn_consider(s, qx, qy, qz, p.x, p.y, p.z, __float_as_int(p.w));
  }
}

// the k admissible rows of problem g nearest to (qx, qy, qz), into s (unsorted).  The shells and the bound are grid_search's (nn_grid.hip).
__device__ __forceinline__ void grid_knn_search(const NnGrid& g, const float* __restrict__ Y, const unsigned* __restrict__ cell_start,
                                                const float4* __restrict__ sorted, float qx, float qy, float qz, KnnLane& s) {
  if (g.mode == GRID_ROWS) {                          // no index for this problem: every row, in order
    for (int j = 0; j < g.y_len; ++j) {
      const float* p = Y + ((size_t)g.y_start + j) * 3;
      knn_consider(s, qx, qy, qz, p[0], p[1], p[2], j);
    }
    return;
  }
  if (g.mode != GRID_CELLS) return;
  const int nx = g.dims[0], ny = g.dims[1], nz = g.dims[2];
  const float cx = fminf(fmaxf(qx, g.lo[0]), g.hi[0]), cy = fminf(fmaxf(qy, g.lo[1]), g.hi[1]), cz = fminf(fmaxf(qz, g.lo[2]), g.hi[2]);
  const float ox = qx - cx, oy = qy - cy, oz = qz - cz;
  const float ox2 = ox * ox, oy2 = oy * oy, oz2 = oz * oz;
  const float tx = grid_t(cx, g.lo[0], g.h), ty = grid_t(cy, g.lo[1], g.h), tz = grid_t(cz, g.lo[2], g.h);
  const int ix = grid_cell(tx, nx), iy = grid_cell(ty, ny), iz = grid_cell(tz, nz);
  const unsigned* cs = cell_start + g.cell_base;
  for (int r = 0;; ++r) {
    const int x0 = max(ix - r, 0), x1 = min(ix + r, nx - 1), y0 = max(iy - r, 0), y1 = min(iy + r, ny - 1), z0 = max(iz - r, 0),
              z1 = min(iz + r, nz - 1);
    for (int z = z0; z <= z1; ++z) {
      const bool zface = z == iz - r || z == iz + r;
      for (int y = y0; y <= y1; ++y) {
        const int row = nx * (y + ny * z);
        if (zface || y == iy - r || y == iy + r) {
          knn_scan_run(s, sorted, cs[row + x0], cs[row + x1 + 1], qx, qy, qz);
        } else {                                      // inside the shell's ring: only its two end cells are new
          if (ix - r >= 0) knn_scan_run(s, sorted, cs[row + ix - r], cs[row + ix - r + 1], qx, qy, qz);
          if (ix + r < nx) knn_scan_run(s, sorted, cs[row + ix + r], cs[row + ix + r + 1], qx, qy, qz);
        }
      }
    }
    if (x0 == 0 && x1 == nx - 1 && y0 == 0 && y1 == ny - 1 && z0 == 0 && z1 == nz - 1) break;      // the cube covers the grid
    float sx = __builtin_inff(), sy = sx, sz = sx;
    if (x0 > 0) sx = tx - (float)x0;
    if (x1 < nx - 1) sx = fminf(sx, (float)(x1 + 1) - tx);
    if (y0 > 0) sy = ty - (float)y0;
    if (y1 < ny - 1) sy = fminf(sy, (float)(y1 + 1) - ty);
    if (z0 > 0) sz = tz - (float)z0;
    if (z1 < nz - 1) sz = fminf(sz, (float)(z1 + 1) - tz);
    const float mx = fabsf(ox) + fmaxf(sx - GRID_SLACK, 0.f) * g.h, my = fabsf(oy) + fmaxf(sy - GRID_SLACK, 0.f) * g.h,
                mz = fabsf(oz) + fmaxf(sz - GRID_SLACK, 0.f) * g.h;
    const float lb2 = fminf(fminf(mx * mx + (oy2 + oz2), my * my + (ox2 + oz2)), mz * mz + (ox2 + oy2)) * GRID_MARGIN;
    if (lb2 > s.limit) break;                         // the worst key's d2 once the list is full, the radius bound before
  }
}

// the lane's keys in ascending order, in place
__device__ __forceinline__ void knn_sort(unsigned long long* list, int cnt) {
  for (int i = 1; i < cnt; ++i) {
    const unsigned long long key = list[i * KNN_TILE];
    int j = i;
    while (j > 0) {
      const unsigned long long v = list[(j - 1) * KNN_TILE];
      if (v <= key) break;
      list[j * KNN_TILE] = v;
      --j;
    }
    list[j * KNN_TILE] = key;
  }
}

// normals.hip's plane fit over the cnt rows of the sorted list: fp64 mean and covariance in ascending key order, the smallest
// eigenvector, the orientation rule; zero below three neighbours
__device__ __forceinline__ void knn_plane_fit(const KnnParams& a, const unsigned long long* list, int cnt, int y_start, int prob, float qx,
                                              float qy, float qz, size_t row) {
  double nv[3] = {0.0, 0.0, 0.0}, lam[3] = {0.0, 0.0, 0.0};
  if (cnt >= 3) {
    double mu[3] = {0.0, 0.0, 0.0};
    for (int s = 0; s < cnt; ++s) {
      const float* p = a.Y + ((size_t)y_start + (unsigned)list[s * KNN_TILE]) * 3;
      mu[0] += (double)p[0]; mu[1] += (double)p[1]; mu[2] += (double)p[2];
    }
    const double inv = 1.0 / (double)cnt;
    mu[0] *= inv; mu[1] *= inv; mu[2] *= inv;
    double c00 = 0.0, c01 = 0.0, c02 = 0.0, c11 = 0.0, c12 = 0.0, c22 = 0.0;
    for (int s = 0; s < cnt; ++s) {
      const float* p = a.Y + ((size_t)y_start + (unsigned)list[s * KNN_TILE]) * 3;
      const double dx = (double)p[0] - mu[0], dy = (double)p[1] - mu[1], dz = (double)p[2] - mu[2];
      c00 += dx * dx; c01 += dx * dy; c02 += dx * dz; c11 += dy * dy; c12 += dy * dz; c22 += dz * dz;
    }
    const double C[3][3] = {{c00 * inv, c01 * inv, c02 * inv}, {c01 * inv, c11 * inv, c12 * inv}, {c02 * inv, c12 * inv, c22 * inv}};
    rap_sym_eig3_smallest(C, lam, nv);
    bool flip;
    if (a.viewpoint) {
      const float* v = a.viewpoint + (size_t)prob * 3;
      flip = nv[0] * ((double)v[0] - (double)qx) + nv[1] * ((double)v[1] - (double)qy) + nv[2] * ((double)v[2] - (double)qz) < 0.0;
    } else {                                                           // the component of largest magnitude positive, lowest index among equals
      int big = 0;
      if (fabs(nv[1]) > fabs(nv[big])) big = 1;
      if (fabs(nv[2]) > fabs(nv[big])) big = 2;
      flip = nv[big] < 0.0;
    }
    if (flip) { nv[0] = -nv[0]; nv[1] = -nv[1]; nv[2] = -nv[2]; }
  }
  a.normals[row * 3 + 0] = (float)nv[0]; a.normals[row * 3 + 1] = (float)nv[1]; a.normals[row * 3 + 2] = (float)nv[2];
  if (a.eigenvalues) {
    a.eigenvalues[row * 3 + 0] = (float)lam[0]; a.eigenvalues[row * 3 + 1] = (float)lam[1]; a.eigenvalues[row * 3 + 2] = (float)lam[2];
  }
}

// what the block writes for query row `row` from its sorted list of cnt keys (cnt = 0: a query that admits nothing)
template <int EPI>
__device__ __forceinline__ void knn_emit(const KnnParams& a, const unsigned long long* list, int cnt, int y_start, int prob, float qx, float qy,
                                         float qz, size_t row) {
  if (EPI == KNN_ROWS_OUT) {
    int32_t* io = a.idx_out + row * (size_t)a.k;
    float* dd = a.d2_out + row * (size_t)a.k;
    for (int s = 0; s < a.k; ++s) {
      const unsigned long long key = s < cnt ? list[s * KNN_TILE] : 0ull;
      io[s] = s < cnt ? y_start + (int)(unsigned)key : -1;
      dd[s] = s < cnt ? __uint_as_float((unsigned)(key >> 32)) : __builtin_inff();
    }
    a.count_out[row] = cnt;
  } else if (EPI == KNN_NORMALS) {
    knn_plane_fit(a, list, cnt, y_start, prob, qx, qy, qz, row);
  } else {                                            // outlier.hip's kernel 1: the mean of sqrtf(d2), summed in double, ascending
    double sum = 0.0;
    for (int s = 0; s < cnt; ++s) sum += (double)sqrtf(__uint_as_float((unsigned)(list[s * KNN_TILE] >> 32)));
    a.mean_dist[row] = cnt > 0 ? sum / (double)cnt : -1.0;
  }
}

template <int EPI>
__global__ __launch_bounds__(KNN_TILE) void knn_kernel(const KnnParams a) {
  extern __shared__ unsigned long long knn_list[];                     // [slots4][KNN_TILE] keys
  const NnWork w = a.items[blockIdx.x];
  if (w.x_len <= 0) return;
  const int prob = w.pad0;
  const NnGrid g = a.grids[prob];
  const int lane = threadIdx.x, q = w.q0 + lane;
  if (q >= w.x_len) return;                                            // no barrier below: a lane is on its own from here
  unsigned long long* list = knn_list + lane;
  size_t row = (size_t)w.x_start + q;
  float qx, qy, qz;
  bool has;
  if (a.self && g.mode == GRID_CELLS) {
    // cell order: lane q takes the q-th finite row of the segment as `sorted` holds them, and the empty result of row q if that
    // row is not among them
    const unsigned* cs = a.cell_start + g.cell_base;
    const unsigned first = cs[0], n_sorted = cs[g.dims[0] * g.dims[1] * g.dims[2]] - first;
    const float* p = a.X + row * 3;
    if (!grid_finite(p[0], p[1], p[2])) knn_emit<EPI>(a, list, 0, w.y_start, prob, p[0], p[1], p[2], row);
    has = (unsigned)q < n_sorted;
    if (has) {
      const float4 c = a.sorted[first + (unsigned)q];
      qx = c.x; qy = c.y; qz = c.z;
      row = (size_t)w.x_start + (unsigned)__float_as_int(c.w);
    }
  } else {
    qx = a.X[row * 3 + 0]; qy = a.X[row * 3 + 1]; qz = a.X[row * 3 + 2];
    has = grid_finite(qx, qy, qz);                                     // a non-finite query admits nothing: no walk
    if (!has) knn_emit<EPI>(a, list, 0, w.y_start, prob, qx, qy, qz, row);
  }
  if (!has) return;
  KnnLane s;
  s.list = list; s.worst = 0ull; s.limit = a.r2_limit; s.radius = a.radius; s.cnt = 0; s.worst_slot = 0; s.k = a.k; s.slots4 = knn_slots(a.k);
  for (int t = s.k; t < s.slots4; ++t) list[t * KNN_TILE] = 0ull;      // padding to a multiple of four: never the worst of a full list
  grid_knn_search(g, a.Y, a.cell_start, a.sorted, qx, qy, qz, s);
  knn_sort(list, s.cnt);
  knn_emit<EPI>(a, list, s.cnt, w.y_start, prob, qx, qy, qz, row);
}

static int knn_launch(hipStream_t stream, int epi, const KnnParams& a, int max_items) {
  const int lds = knn_slots(a.k) * KNN_TILE * 8;
  const dim3 grid(max_items), block(KNN_TILE);
  if (epi == KNN_ROWS_OUT) return rap_launch_dyn_lds(knn_kernel<KNN_ROWS_OUT>, grid, block, lds, stream, a);
  if (epi == KNN_NORMALS) return rap_launch_dyn_lds(knn_kernel<KNN_NORMALS>, grid, block, lds, stream, a);
  return rap_launch_dyn_lds(knn_kernel<KNN_MEAN_DIST>, grid, block, lds, stream, a);
}

static KnnParams knn_params(const float* X, const float* Y, const NnWork* items, const NnGridWs& g, int k, float radius, bool self) {
  KnnParams a = {};
  a.X = X; a.Y = Y; a.items = items;
  a.grids = (const NnGrid*)g.grids; a.cell_start = g.cell_start; a.sorted = (const float4*)g.sorted;
  a.radius = radius > 0.f ? radius : 0.f;
  a.r2_limit = radius > 0.f ? radius * radius * GRID_GATE_MARGIN : __builtin_inff();
  a.k = k; a.self = self ? 1 : 0;
  return a;
}

int launch_k_nearest_neighbors(hipStream_t stream, const float* X, const int32_t* x_seg, const float* Y, const int32_t* y_seg, int K, long NX,
                               long NY, int k, float radius, int32_t* idx_out, float* d2_out, int32_t* count_out, NnWork* items,
                               const NnGridWs& g) {
  int rc = launch_nn_grid_items(stream, x_seg, y_seg, K, NX, NY, items);
  if (rc) return rc;
  rc = launch_nn_grid_build(stream, Y, y_seg, K, NY, g);
  if (rc) return rc;
  KnnParams a = knn_params(X, Y, items, g, k, radius, false);
  a.idx_out = idx_out; a.d2_out = d2_out; a.count_out = count_out;
  return knn_launch(stream, KNN_ROWS_OUT, a, (int)nn_max_items(NX, K));
}

int launch_estimate_normals_grid(hipStream_t stream, const float* P, const int32_t* seg, int K, long N, int max_nn, float radius,
                                 const float* viewpoint, float* normals, float* eigenvalues, NnWork* items, int32_t* repeat, const NnGridWs& g) {
  int rc = launch_normals_items(stream, seg, K, N, items, repeat);
  if (rc) return rc;
  rc = launch_nn_grid_build(stream, P, seg, K, N, g);
  if (rc) return rc;
  KnnParams a = knn_params(P, P, items, g, max_nn, radius, true);
  a.viewpoint = viewpoint; a.normals = normals; a.eigenvalues = eigenvalues;
  return knn_launch(stream, KNN_NORMALS, a, (int)nn_max_items(N, K));
}

// the lists themselves for a self-search (orient.hip): the work list and the cell-order walk of the normal estimation, the output of
// rap_k_nearest_neighbors without a radius
int launch_knn_self_rows(hipStream_t stream, const float* P, const int32_t* seg, int K, long N, int k, int32_t* idx_out, float* d2_out,
                         int32_t* count_out, NnWork* items, int32_t* repeat, const NnGridWs& g) {
  int rc = launch_normals_items(stream, seg, K, N, items, repeat);
  if (rc) return rc;
  rc = launch_nn_grid_build(stream, P, seg, K, N, g);
  if (rc) return rc;
  KnnParams a = knn_params(P, P, items, g, k, 0.f, true);
  a.idx_out = idx_out; a.d2_out = d2_out; a.count_out = count_out;
  return knn_launch(stream, KNN_ROWS_OUT, a, (int)nn_max_items(N, K));
}

__global__ void knn_whole_segment_kernel(int32_t* __restrict__ seg, int n) {
  if (blockIdx.x == 0 && threadIdx.x == 0) { seg[0] = 0; seg[1] = n; }
}

int launch_knn_mean_dist_grid(hipStream_t stream, const float* pts, long N, int k, double* mean_dist, int32_t* seg, NnWork* items,
                              const NnGridWs& g) {
  hipLaunchKernelGGL(knn_whole_segment_kernel, dim3(1), dim3(64), 0, stream, seg, (int)N);
  RAP_LAUNCH_CHECK();
  int rc = launch_nn_grid_items(stream, seg, seg, 1, N, N, items);
  if (rc) return rc;
  rc = launch_nn_grid_build(stream, pts, seg, 1, N, g);
  if (rc) return rc;
  KnnParams a = knn_params(pts, pts, items, g, k, 0.f, true);
  a.mean_dist = mean_dist;
  return knn_launch(stream, KNN_MEAN_DIST, a, (int)nn_max_items(N, 1));
}
