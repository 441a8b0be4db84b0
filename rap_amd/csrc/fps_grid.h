// What the bucket index of farthest point sampling (fps_grid.hip) computes outside its loops: the build constants, the workspace
// arithmetic, the grid laid over a cloud and the lower bound of the skip rule.  Plain C++: the kernel compiles these lines for the
// device, and tests/host/fps_grid_host.cpp compiles the same lines with g++ into a sequential restatement of the method.  The method
// and the rounding argument are at the top of fps_grid.hip.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RAP_FPS_HD __host__ __device__ __forceinline__
#else
#define RAP_FPS_HD static inline
#endif

#define FPS_GRID_PER 32                       // points per bucket the grid aims at (rap_set_tuning key 22; sweep: DESIGN.md section 7.7)
#define FPS_GRID_MAX_BUCKETS 4096             // the bucket table lives in LDS: 32 bytes per bucket, plus the bucket starts and the queue
#define FPS_GRID_MARGIN 0.9999847412109375f   // 1 - 2^-16, GRID_MARGIN of nn_grid.h

// bytes of workspace per point: the sorted rows, float4 (x, y, z, original index), and the running distance of every sorted row
#define FPS_GRID_ROW_BYTES 16
#define FPS_GRID_DIST_BYTES 4

RAP_FPS_HD size_t fps_grid_align(size_t v) { return (v + 255) / 256 * 256; }
// sorted rows first, then the distances; both start on a 256-byte boundary
RAP_FPS_HD size_t fps_grid_dist_offset(int64_t total_points) { return fps_grid_align((size_t)total_points * FPS_GRID_ROW_BYTES); }
RAP_FPS_HD size_t fps_grid_workspace_bytes(int64_t total_points) {
  return total_points <= 0 ? 0 : fps_grid_dist_offset(total_points) + fps_grid_align((size_t)total_points * FPS_GRID_DIST_BYTES);
}

struct FpsGrid {
  float lo[3], h;
  int dims[3], buckets;       // buckets = dims[0] * dims[1] * dims[2] <= max_buckets; 0: the cloud cannot be indexed
};

// buckets the grid aims at for n points: ceil(n / per), at least 1 and at most max_buckets.  The cap is the only place a bucket grows
RAP_FPS_HD int fps_grid_target(int n, int per, int max_buckets) {
  const long long t = ((long long)n + per - 1) / per;
  return (int)(t < 1 ? 1 : t > max_buckets ? max_buckets : t);
}
// cells along one axis of extent e at cell edge h (1 for an axis without extent), as a float: it may be huge
RAP_FPS_HD float fps_grid_axis_cells(float e, float h) { return e > 0.f ? floorf(e / h) + 1.f : 1.f; }

// Cubic cells of edge h over the box [lo, hi] of n points: h ~ (volume / target)^(1/3) (area / length over the axes that have an
// extent; an axis without one gets one cell), grown by a quarter at a time until the cells number at most max_buckets.  A heuristic
// throughout: the sampling is exact for ANY assignment of rows to buckets, because every bucket carries the tight box of its rows.
// buckets = 0 when the extents are not finite numbers the loop can work with; the caller then walks the cloud row by row.
RAP_FPS_HD FpsGrid fps_grid_dims(const float lo[3], const float hi[3], int n, int per, int max_buckets) {
  FpsGrid g;
  g.lo[0] = lo[0]; g.lo[1] = lo[1]; g.lo[2] = lo[2];
  g.h = 1.f; g.dims[0] = g.dims[1] = g.dims[2] = 1; g.buckets = 0;
  if (n <= 0 || per <= 0 || max_buckets <= 0) return g;
  const float ex = hi[0] - lo[0], ey = hi[1] - lo[1], ez = hi[2] - lo[2];
  if (!(ex >= 0.f && ey >= 0.f && ez >= 0.f) || !(ex < INFINITY && ey < INFINITY && ez < INFINITY)) return g;
  const int nd = (ex > 0.f) + (ey > 0.f) + (ez > 0.f);
  g.buckets = 1;
  if (nd == 0) return g;                               // every row is the same point: one bucket
  const float emax = fmaxf(ex, fmaxf(ey, ez));
  const double vol = (ex > 0.f ? (double)ex : 1.0) * (ey > 0.f ? (double)ey : 1.0) * (ez > 0.f ? (double)ez : 1.0);
  const float per_cell = (float)(vol / (double)fps_grid_target(n, per, max_buckets));
  float h = nd == 3 ? cbrtf(per_cell) : nd == 2 ? sqrtf(per_cell) : per_cell;
  h = fmaxf(h, emax / (float)max_buckets);             // no axis starts with more cells than the table has
  if (!(h > 0.f && h < INFINITY)) return g;            // (underflow of a tiny volume: one bucket)
  // once h exceeds every extent all dimensions are 1; 64 steps from emax / max_buckets reach that (1.25^64 > 1e6 > max_buckets)
  for (int step = 0; step < 64; ++step) {
    const float fx = fps_grid_axis_cells(ex, h), fy = fps_grid_axis_cells(ey, h), fz = fps_grid_axis_cells(ez, h);
    if (fx <= (float)max_buckets && fy <= (float)max_buckets && fz <= (float)max_buckets &&
        (long long)fx * (long long)fy * (long long)fz <= (long long)max_buckets) {
      g.h = h; g.dims[0] = (int)fx; g.dims[1] = (int)fy; g.dims[2] = (int)fz;
      g.buckets = g.dims[0] * g.dims[1] * g.dims[2];
      return g;
    }
    h *= 1.25f;
    if (!(h < INFINITY)) break;
  }
  return g;                                            // one bucket
}

// the bucket of a row: position in cells per axis, floored and clamped into the grid
RAP_FPS_HD int fps_grid_axis_cell(float p, float lo, float h, int dim) { return (int)fminf(fmaxf(floorf((p - lo) / h), 0.f), (float)(dim - 1)); }
RAP_FPS_HD int fps_grid_bucket(const FpsGrid& g, float x, float y, float z) {
  return fps_grid_axis_cell(x, g.lo[0], g.h, g.dims[0]) +
         g.dims[0] * (fps_grid_axis_cell(y, g.lo[1], g.h, g.dims[1]) + g.dims[1] * fps_grid_axis_cell(z, g.lo[2], g.h, g.dims[2]));
}

// Lower bound of the squared distance from s to every row inside the box [lo, hi], scaled by 1 - 2^-16.  A bucket whose largest running
// distance is `max` is skipped iff fps_grid_lower_bound(...) >= max (fps_grid.hip, "Rounding").  An empty bucket has lo = +inf,
// hi = -inf and max = -inf: its bound is +inf and it is skipped.
RAP_FPS_HD float fps_grid_lower_bound(float lox, float loy, float loz, float hix, float hiy, float hiz, float sx, float sy, float sz) {
  const float ex = fmaxf(fmaxf(lox - sx, sx - hix), 0.f), ey = fmaxf(fmaxf(loy - sy, sy - hiy), 0.f), ez = fmaxf(fmaxf(loz - sz, sz - hiz), 0.f);
  return (ex * ex + ey * ey + ez * ez) * FPS_GRID_MARGIN;
}
RAP_FPS_HD bool fps_grid_skip(float lower_bound, float bucket_max) { return lower_bound >= bucket_max; }
