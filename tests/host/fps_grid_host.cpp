// Host build of rap_amd/csrc/fps_grid.h (the lines the device kernel compiles) for CPU unit tests: a SEQUENTIAL restatement of the
// bucket method of rap_amd/csrc/fps_grid.hip on the header's own grid, bucket and lower-bound functions.  The distance is
// (dx*dx + dy*dy) + dz*dz in fp32 without contraction, the expression of oracle/rap_oracle.py::farthest_point_sampling.
// With -DFPS_GRID_HOST_MAIN the file is a stand-alone program (its own main) that holds the method to the plain loop on small grids:
// the form to run under -fsanitize=address,undefined.
#include "../../rap_amd/csrc/fps_grid.h"
#include <algorithm>
#include <cstdio>
#include <limits>
#include <vector>

static float d2_host(const float* p, const float* s) {
  const float dx = p[0] - s[0], dy = p[1] - s[1], dz = p[2] - s[2];
  return (dx * dx + dy * dy) + dz * dz;
}

extern "C" size_t fps_host_workspace_bytes(int64_t total_points) { return fps_grid_workspace_bytes(total_points); }
extern "C" int fps_host_target(int n, int per, int max_buckets) { return fps_grid_target(n, per, max_buckets); }

// dims_out: dims[3], buckets; returns the cell edge
extern "C" float fps_host_dims(const float* lo, const float* hi, int n, int per, int max_buckets, int32_t* dims_out) {
  const FpsGrid g = fps_grid_dims(lo, hi, n, per, max_buckets);
  dims_out[0] = g.dims[0]; dims_out[1] = g.dims[1]; dims_out[2] = g.dims[2]; dims_out[3] = g.buckets;
  return g.h;
}

// pts (n,3) finite -> out (min(K, n)) picks; stats: {buckets, non-empty buckets, rows touched after the first pick, buckets opened after
// the first pick}.  order_seed != 0 permutes the rows inside every bucket (the order the device's counting sort leaves is arbitrary).
// Returns the number of picks, or -1 when the grid cannot take the cloud.
extern "C" int fps_host_sample(const float* pts, int n, int K, int start, int per, int max_buckets, unsigned order_seed, int32_t* out,
                               int64_t* stats) {
  const float inf = std::numeric_limits<float>::infinity();
  if (n <= 0 || K <= 0) return 0;
  K = std::min(K, n);
  float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
  for (int i = 0; i < n; ++i)
    for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], pts[i * 3 + a]); hi[a] = fmaxf(hi[a], pts[i * 3 + a]); }
  const FpsGrid g = fps_grid_dims(lo, hi, n, per, max_buckets);
  if (g.buckets <= 0 || g.buckets > max_buckets) return -1;
  const int nb = g.buckets;
  std::vector<std::vector<int>> rows(nb);
  for (int i = 0; i < n; ++i) {
    const int b = fps_grid_bucket(g, pts[i * 3], pts[i * 3 + 1], pts[i * 3 + 2]);
    if (b < 0 || b >= nb) return -1;
    rows[b].push_back(i);
  }
  unsigned rng = order_seed;
  if (order_seed)
    for (auto& r : rows)
      for (size_t j = r.size(); j > 1; --j) { rng = rng * 1664525u + 1013904223u; std::swap(r[j - 1], r[(rng >> 8) % j]); }
  std::vector<float> blo(nb * 3, inf), bhi(nb * 3, -inf), bmax(nb, -inf), d(n, inf);
  std::vector<int> barg(nb, std::numeric_limits<int>::max());
  int non_empty = 0;
  for (int b = 0; b < nb; ++b) {
    for (int i : rows[b]) {
      for (int a = 0; a < 3; ++a) { blo[b * 3 + a] = fminf(blo[b * 3 + a], pts[i * 3 + a]); bhi[b * 3 + a] = fmaxf(bhi[b * 3 + a], pts[i * 3 + a]); }
      barg[b] = std::min(barg[b], i);
    }
    if (!rows[b].empty()) { bmax[b] = inf; ++non_empty; }
  }
  int last = start < 0 ? 0 : start >= n ? n - 1 : start;
  out[0] = last;
  int64_t touched = 0, opened = 0;
  for (int k = 1; k < K; ++k) {
    const float* s = pts + (size_t)last * 3;
    for (int b = 0; b < nb; ++b) {
      const float lb = fps_grid_lower_bound(blo[b * 3], blo[b * 3 + 1], blo[b * 3 + 2], bhi[b * 3], bhi[b * 3 + 1], bhi[b * 3 + 2], s[0], s[1], s[2]);
      if (fps_grid_skip(lb, bmax[b])) continue;
      float m = -inf;
      int arg = std::numeric_limits<int>::max();
      for (int i : rows[b]) {
        d[i] = fminf(d[i], d2_host(pts + (size_t)i * 3, s));
        if (d[i] > m || (d[i] == m && i < arg)) { m = d[i]; arg = i; }
      }
      bmax[b] = m; barg[b] = arg;
      if (k > 1) { touched += (int64_t)rows[b].size(); ++opened; }
    }
    float m = -inf;
    int arg = std::numeric_limits<int>::max();
    for (int b = 0; b < nb; ++b)
      if (bmax[b] > m || (bmax[b] == m && barg[b] < arg)) { m = bmax[b]; arg = barg[b]; }
    out[k] = last = arg;
  }
  if (stats) { stats[0] = nb; stats[1] = non_empty; stats[2] = touched; stats[3] = opened; }
  return K;
}

// the plain loop: d = min(d, d2), first arg-max
extern "C" int fps_host_plain(const float* pts, int n, int K, int start, int32_t* out) {
  if (n <= 0 || K <= 0) return 0;
  K = std::min(K, n);
  std::vector<float> d(n, std::numeric_limits<float>::infinity());
  int last = start < 0 ? 0 : start >= n ? n - 1 : start;
  out[0] = last;
  for (int k = 1; k < K; ++k) {
    float m = -1.f;
    int arg = 0;
    for (int i = 0; i < n; ++i) {
      d[i] = fminf(d[i], d2_host(pts + (size_t)i * 3, pts + (size_t)last * 3));
      if (d[i] > m) { m = d[i]; arg = i; }
    }
    out[k] = last = arg;
  }
  return K;
}

#ifdef FPS_GRID_HOST_MAIN
int main() {
  int failures = 0;
  const int shapes[][3] = {{6, 6, 6}, {17, 13, 1}, {1, 1, 300}, {1, 1, 1}, {5, 1, 7}};
  for (const auto& sh : shapes) {
    std::vector<float> pts;
    for (int x = 0; x < sh[0]; ++x)
      for (int y = 0; y < sh[1]; ++y)
        for (int z = 0; z < sh[2]; ++z) { pts.push_back((float)x); pts.push_back((float)y); pts.push_back((float)z); }
    const int n = (int)pts.size() / 3;
    std::vector<int32_t> want(n), got(n);
    for (int start : {0, n / 2, n - 1}) {
      fps_host_plain(pts.data(), n, n, start, want.data());
      for (int per : {1, 8, 64})
        for (int cap : {1, 7, 4096}) {
          int64_t stats[4];
          const int k = fps_host_sample(pts.data(), n, n, start, per, cap, 77u, got.data(), stats);
          if (k != n || got != want) { std::printf("MISMATCH %dx%dx%d start %d per %d cap %d\n", sh[0], sh[1], sh[2], start, per, cap); ++failures; }
        }
    }
  }
  std::printf("%s\n", failures ? "FAILED" : "ok");
  return failures ? 1 : 0;
}
#endif
