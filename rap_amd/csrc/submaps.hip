// Submaps on the device: the stage of the reference's data preparation that turns a drive's LiDAR sweeps and poses into the submaps that
// become the "views" (dataset_process/utils/processing_utils.py:1927-2090): per-point deskewing (dataset_utils.py:682-747), frames ->
// world-frame submaps (submap_utils.py:26-50 over dataset_utils.py:361-407), the voxel-set Jaccard overlap of every pair of submaps
// (dataset_utils.py:603-650) and the connectivity test of candidate groups (submap_utils.py:102-164).  The reference does it one frame
// and one pair at a time on the host, with Python sets of voxel tuples; here F frames are one packed (N,3) array plus an int32 prefix
// table cu_frames (F+1), and S submaps are contiguous runs of frames, submap_frames (S+1) a prefix table over frames.
//
//   submap_tables_kernel    the caller's tables made safe to index with (running maximum of the clamped entries), the point offset of
//                           every submap, the call's status word and the cleared reduction cells.  A table that had to be changed is
//                           MALFORMED: bit 1 of the status word; every later kernel of the call then writes NaN (the deferred error).
//   deskew_minmax_kernel    min / max of ts per frame: a lane folds its four rows, a wave whose rows share a frame reduces in registers,
//                           the waves of a block meet in LDS, then ONE integer atomicMin / atomicMax per block and frame on the
//                           order-preserving encoding of the floats (no floating-point atomics; min and max do not depend on the
//                           order of arrival).
//   deskew_apply_kernel     axis and angle of every frame that the block's 1024 rows touch (16 at a time in LDS), once per block in double (log R by
//                           atan2(|v|, (tr - 1) / 2) with the series of asin(x) / x below 1e-4: theta = 0 and 1e-7 are exact), then
//                           per point in fp32  p' = p + A (u x p) + B (u x (u x p)) + s T,  u = s w, x = |s| theta,
//                           A = sin x / x = 2 sin(x/2) cos(x/2) / x,  B = (1 - cos x) / x^2 = 2 sin^2(x/2) / x^2  (no cancellation),
//                           the series 1 - x^2/6, 1/2 - x^2/24 below 1e-3.  s == 0 and an identity rel_pose copy the bits.
//   fuse_frames_kernel      world = fp32(R p + t - origin) in double, one rounding; normals R n / |R n| (|.| < 1e-8: divided by 1).
//   overlap_bounds_kernel   voxel coordinates floor((R p + t) / voxel_size) in double; call-wide per-axis min / max: registers, wave, LDS,
//                           then six integer atomics per block of a capped grid.
//   overlap_keys_kernel     3 x 21-bit offsets from the minimum in one 64-bit key, the submap number beside it; an axis whose extent
//                           does not fit 21 bits sets bit 2 of the status word.
//   two rocPRIM radix sorts by key, then (stable) by submap number: every submap's keys sorted, each submap where its points were.
//                           Not rocprim::segmented_radix_sort_keys: from its partitioning threshold on it copies the segment counts to
//                           the host and waits (this family never synchronises), and it gives a long segment to ONE block.
//   overlap_heads_kernel / rocPRIM inclusive scan / overlap_compact_kernel / overlap_offsets_kernel
//                           the first key of every run -> the unique keys of every submap, cu_unique (S+1), n_voxels, the chunk table.
//   overlap_intersect_kernel   THE HOT LOOP.  A block owns 256 consecutive unique keys of submap i and meets every submap j that is
//                           larger (or as large, with j > i): the pair is always searched from its smaller side.  Each wave narrows the
//                           window of j's sorted keys with its first and last key (an empty window, the common case for submaps far
//                           apart, costs two searches), each lane binary-searches its key in the window, the hits are counted with a
//                           ballot and added to the pair's cell with one integer atomic per wave.
//   overlap_finish_kernel   ratio = |A n B| / (|A| + |B| - |A n B|), both triangles, 0 where a set is empty, NaN under a status bit.
//   groups_connected_kernel one wave per candidate group: lane k holds the 64-bit adjacency mask of member k (lo <= ratio <= hi), the
//                           set reachable from member 0 grows by a wave-wide OR until it stops.
// No host read, no floating-point atomics, results bit-identical from call to call; every index comes from a sanitised table.
#include "../../include/rapflow.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "kernels.h"

#define SUB_ST_TABLE 1        // bits of the status word
#define SUB_ST_EXTENT 2
#define SUB_ST_GROUP 4
#define SUB_ROWS 1024         // rows of the packed array per block (256 threads x 4)
#define SUB_FCACHE 16         // frames whose axis / angle a deskew block keeps in LDS
#define SUB_CHUNK 256         // unique keys per intersection block
#define SUB_KEY_NONE 0xffffffffffffffffull      // the key of a dropped row: above every packed key (63 bits)
#define SUB_MAX_S 4096
#define SUB_MAX_F (1 << 24)

// ---- tables -------------------------------------------------------------------------------------------------------------------
// out[i] = max_{j <= i} clamp(in[j], 0, limit) by one block of 256 threads; returns (to every thread) whether an entry changed or an end
// is not where it has to be (first == 0 always wanted when need_first0, last == limit when need_last).
__device__ int sub_sanitize(const int32_t* __restrict__ in, int n, int limit, int32_t* __restrict__ out, bool need_first0, bool need_last,
                            int* part, int* bad_cell) {
  const int tid = threadIdx.x;
  const int per = (n + 255) / 256;
  const long i0l = (long)tid * per;
  const int i0 = i0l < n ? (int)i0l : n, i1 = (i0l + per) < n ? (int)(i0l + per) : n;
  int m = 0;
  for (int i = i0; i < i1; ++i) { int v = in[i]; v = v < 0 ? 0 : v > limit ? limit : v; m = v > m ? v : m; }
  part[tid] = m;
  if (tid == 0) *bad_cell = 0;
  __syncthreads();
  int acc = 0;
  for (int t = 0; t < tid; ++t) acc = part[t] > acc ? part[t] : acc;
  int bad = 0;
  m = acc;
  for (int i = i0; i < i1; ++i) {
    const int raw = in[i];
    int v = raw < 0 ? 0 : raw > limit ? limit : raw;
    m = v > m ? v : m;
    out[i] = m;
    bad |= (m != raw) || (i == 0 && need_first0 && raw != 0) || (i == n - 1 && need_last && raw != limit);
  }
  if (bad) atomicOr(bad_cell, 1);
  __syncthreads();
  const int r = *bad_cell;
  __syncthreads();
  return r;
}

struct SubTables {
  const int32_t* cu_frames;      // (F+1) the caller's
  const int32_t* submap_frames;  // (S+1) the caller's, or null
  int32_t* cu_s;                 // (F+1) sanitised
  int32_t* sf_s;                 // (S+1) sanitised, or null
  int32_t* seg_off;              // (S+1) point offset of every submap, or null
  int32_t* flag;                 // the call's status word
  int32_t* status;               // the caller's, or null
  uint32_t* minmax;              // (2F) deskew: encoded min / max of ts, or null
  unsigned long long* bounds;    // (6) overlap: biased per-axis min / max, or null
  int F, S, N;
};

__global__ __launch_bounds__(256) void submap_tables_kernel(const SubTables a) {
  if (blockIdx.x != 0) return;
  __shared__ int part[256];
  __shared__ int bad_cell;
  int bad = sub_sanitize(a.cu_frames, a.F + 1, a.N, a.cu_s, true, true, part, &bad_cell);
  if (a.submap_frames) {
    bad |= sub_sanitize(a.submap_frames, a.S + 1, a.F, a.sf_s, false, false, part, &bad_cell);
    __threadfence_block();
    __syncthreads();
    for (int s = threadIdx.x; s <= a.S; s += 256) a.seg_off[s] = a.cu_s[a.sf_s[s]];
  }
  if (a.minmax)
    for (int f = threadIdx.x; f < a.F; f += 256) { a.minmax[2 * f] = 0xffffffffu; a.minmax[2 * f + 1] = 0u; }
  if (a.bounds && threadIdx.x < 6) a.bounds[threadIdx.x] = threadIdx.x < 3 ? ~0ull : 0ull;
  if (threadIdx.x == 0) {
    *a.flag = bad ? SUB_ST_TABLE : 0;
    if (bad && a.status) atomicOr(a.status, SUB_ST_TABLE);
  }
}

// the frame (or submap) of row r: the last f with table[f] <= r, in [0, n - 1]; table has n + 1 non-decreasing entries
__device__ __forceinline__ int sub_find(const int32_t* __restrict__ table, int n, int r) {
  int lo = 0, hi = n;                      // first index in [0, n] with table[idx] > r, searched over [1, n]
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;    // in [1, n]
    if (table[mid] <= r) lo = mid; else hi = mid - 1;
  }
  return lo < n ? lo : n - 1;
}

// the same within [lo, hi] for a row whose entry is known to lie there: table[lo] <= r, and hi is the entry of a later row.  A block of
// SUB_ROWS consecutive rows looks up its first and its last row in the whole table (wave-uniform loads) and every row between the two,
// which is usually no search at all.
__device__ __forceinline__ int sub_find_in(const int32_t* __restrict__ table, int lo, int hi, int r) {
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;    // in [lo + 1, hi]
    if (table[mid] <= r) lo = mid; else hi = mid - 1;
  }
  return lo;
}
__device__ __forceinline__ void sub_chunk_range(const int32_t* __restrict__ table, int n, long row0, int N, int& f_first, int& f_last) {
  const long last = row0 + SUB_ROWS - 1 < N ? row0 + SUB_ROWS - 1 : (long)N - 1;
  f_first = sub_find(table, n, (int)row0);
  f_last = sub_find(table, n, (int)last);
}

// ---- deskew -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t f32_ordered(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float f32_unordered(uint32_t e) { return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e); }

__global__ __launch_bounds__(256) void deskew_minmax_kernel(const float* __restrict__ ts, const int32_t* __restrict__ cu_s, int F, int N,
                                                            uint32_t* __restrict__ minmax) {
  __shared__ uint32_t s_lo[4], s_hi[4];
  __shared__ int s_f[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t lo = 0xffffffffu, hi = 0u;                          // the lane's running pair, of frame fc
  int fc = -1, f_first, f_last;
  sub_chunk_range(cu_s, F, (long)blockIdx.x * SUB_ROWS, N, f_first, f_last);
  for (int k = 0; k < SUB_ROWS / 256; ++k) {
    const long rl = (long)blockIdx.x * SUB_ROWS + k * 256 + threadIdx.x;
    if (rl >= N) break;
    const int f = sub_find_in(cu_s, f_first, f_last, (int)rl);
    if (f != fc) {                                             // a frame ends inside the lane's four rows: hand the pair in
      if (fc >= 0 && lo <= hi) { atomicMin(&minmax[2 * fc], lo); atomicMax(&minmax[2 * fc + 1], hi); }
      fc = f; lo = 0xffffffffu; hi = 0u;
    }
    const float t = ts[rl];
    if (t == t) {                                              // a NaN stamp takes no part in min / max (its own row comes out NaN)
      const uint32_t e = f32_ordered(t);
      lo = e < lo ? e : lo; hi = e > hi ? e : hi;
    }
  }
  const int f0 = __shfl(fc, 0, 64);
  const bool uniform = __all(fc == f0) && f0 >= 0;             // the usual case: the wave's rows lie in one frame
  if (uniform) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const uint32_t l2 = __shfl_xor(lo, o, 64), h2 = __shfl_xor(hi, o, 64);
      lo = l2 < lo ? l2 : lo; hi = h2 > hi ? h2 : hi;
    }
  } else if (fc >= 0 && lo <= hi) {
    atomicMin(&minmax[2 * fc], lo); atomicMax(&minmax[2 * fc + 1], hi);
  }
  if (lane == 0) { s_f[wave] = uniform ? f0 : -1; s_lo[wave] = lo; s_hi[wave] = hi; }
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int w = 0; w < 4; ++w) {                                // the waves of one frame together: one pair of atomics per block and frame
    if (s_f[w] < 0) continue;
    uint32_t l = s_lo[w], h = s_hi[w];
    for (int v = w + 1; v < 4; ++v)
      if (s_f[v] == s_f[w]) { l = s_lo[v] < l ? s_lo[v] : l; h = s_hi[v] > h ? s_hi[v] : h; s_f[v] = -1; }
    if (l <= h) { atomicMin(&minmax[2 * s_f[w]], l); atomicMax(&minmax[2 * s_f[w] + 1], h); }
  }
}

struct DeskewFrame { float w[3], theta, T[3]; int identity; };

__device__ DeskewFrame deskew_frame(const double* __restrict__ M) {     // M: one (4,4) row-major rel_pose
  DeskewFrame d;
  const double vx = 0.5 * (M[9] - M[6]), vy = 0.5 * (M[2] - M[8]), vz = 0.5 * (M[4] - M[1]);
  const double sn = sqrt(vx * vx + vy * vy + vz * vz), cs = 0.5 * (M[0] + M[5] + M[10] - 1.0);
  const double th = atan2(sn, cs);
  const double sn2 = sn * sn;
  const double k = (sn < 1e-4 && cs > 0.0) ? 1.0 + sn2 * (1.0 / 6.0 + sn2 * (3.0 / 40.0)) : th / sn;      // theta / sin(theta)
  d.w[0] = (float)(vx * k); d.w[1] = (float)(vy * k); d.w[2] = (float)(vz * k);
  d.theta = (float)th;
  d.T[0] = (float)M[3]; d.T[1] = (float)M[7]; d.T[2] = (float)M[11];
  d.identity = M[0] == 1.0 && M[5] == 1.0 && M[10] == 1.0 && M[1] == 0.0 && M[2] == 0.0 && M[4] == 0.0 && M[6] == 0.0 && M[8] == 0.0 &&
               M[9] == 0.0 && M[3] == 0.0 && M[7] == 0.0 && M[11] == 0.0;
  return d;
}

__global__ __launch_bounds__(256) void deskew_apply_kernel(const float* __restrict__ P, const float* __restrict__ ts,
                                                           const int32_t* __restrict__ cu_s, int F, int N, const double* __restrict__ rel_pose,
                                                           float ts_mid, const uint32_t* __restrict__ minmax, const int32_t* __restrict__ flag,
                                                           float* __restrict__ out) {
  __shared__ DeskewFrame cache[SUB_FCACHE];
  const long row0 = (long)blockIdx.x * SUB_ROWS;                        // < N by the grid
  int f_first, f_last;
  sub_chunk_range(cu_s, F, row0, N, f_first, f_last);
  const bool poisoned = *flag != 0;
  int fr[SUB_ROWS / 256];                                               // the frame of each of the thread's rows, -1 past the end
  for (int k = 0; k < SUB_ROWS / 256; ++k) {
    const long rl = row0 + k * 256 + threadIdx.x;
    fr[k] = rl < N ? sub_find_in(cu_s, f_first, f_last, (int)rl) : -1;
  }
  // SUB_FCACHE frames at a time (one round, unless the block's rows lie in more frames than that): axis and angle into LDS, then the rows
  for (int base = f_first; base <= f_last; base += SUB_FCACHE) {        // block-uniform bounds
    __syncthreads();
    if (threadIdx.x < SUB_FCACHE && base + (int)threadIdx.x <= f_last) cache[threadIdx.x] = deskew_frame(rel_pose + (size_t)(base + threadIdx.x) * 16);
    __syncthreads();
    for (int k = 0; k < SUB_ROWS / 256; ++k) {
      const int f = fr[k];
      if (f < base || f >= base + SUB_FCACHE) continue;
      const int r = (int)(row0 + k * 256 + threadIdx.x);
      const size_t o = (size_t)r * 3;
      if (poisoned) { out[o] = out[o + 1] = out[o + 2] = __builtin_nanf(""); continue; }
      const DeskewFrame d = cache[f - base];
      const float px = P[o], py = P[o + 1], pz = P[o + 2];
      if (d.identity) { out[o] = px; out[o + 1] = py; out[o + 2] = pz; continue; }      // whatever its stamps are
      const float t = ts[r];
      const float tmin = f32_unordered(minmax[2 * f]), range = f32_unordered(minmax[2 * f + 1]) - tmin;
      float s = range > 1e-8f ? (t - tmin) / range - ts_mid : 0.5f - ts_mid;
      if (t != t) s = t;
      if (s == 0.f) { out[o] = px; out[o + 1] = py; out[o + 2] = pz; continue; }
      const float ux = s * d.w[0], uy = s * d.w[1], uz = s * d.w[2];
      const float x = fabsf(s) * d.theta;
      float A, B;
      if (x < 1e-3f) {
        A = 1.f - x * x * (1.f / 6.f); B = 0.5f - x * x * (1.f / 24.f);
      } else {
        float sh, ch;
        sincosf(0.5f * x, &sh, &ch);
        A = 2.f * sh * ch / x; B = 2.f * sh * sh / (x * x);
      }
      const float c1x = uy * pz - uz * py, c1y = uz * px - ux * pz, c1z = ux * py - uy * px;
      const float c2x = uy * c1z - uz * c1y, c2y = uz * c1x - ux * c1z, c2z = ux * c1y - uy * c1x;
      out[o] = px + A * c1x + B * c2x + s * d.T[0];
      out[o + 1] = py + A * c1y + B * c2y + s * d.T[1];
      out[o + 2] = pz + A * c1z + B * c2z + s * d.T[2];
    }
  }
}

// ---- fuse ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fuse_frames_kernel(const float* __restrict__ P, const float* __restrict__ normals,
                                                          const int32_t* __restrict__ cu_s, int F, int N, const double* __restrict__ pose,
                                                          const double* __restrict__ origin, const int32_t* __restrict__ flag,
                                                          float* __restrict__ world, float* __restrict__ world_normals) {
  const bool poisoned = *flag != 0;
  const double ox = origin ? origin[0] : 0.0, oy = origin ? origin[1] : 0.0, oz = origin ? origin[2] : 0.0;
  int f_first, f_last;
  sub_chunk_range(cu_s, F, (long)blockIdx.x * SUB_ROWS, N, f_first, f_last);
  for (int k = 0; k < SUB_ROWS / 256; ++k) {
    const long rl = (long)blockIdx.x * SUB_ROWS + k * 256 + threadIdx.x;
    if (rl >= N) return;
    const int r = (int)rl;
    const size_t o = (size_t)r * 3;
    if (poisoned) {
      world[o] = world[o + 1] = world[o + 2] = __builtin_nanf("");
      if (world_normals) world_normals[o] = world_normals[o + 1] = world_normals[o + 2] = __builtin_nanf("");
      continue;
    }
    const double* M = pose + (size_t)sub_find_in(cu_s, f_first, f_last, r) * 16;
    const double x = (double)P[o], y = (double)P[o + 1], z = (double)P[o + 2];
    world[o] = (float)(M[0] * x + M[1] * y + M[2] * z + M[3] - ox);
    world[o + 1] = (float)(M[4] * x + M[5] * y + M[6] * z + M[7] - oy);
    world[o + 2] = (float)(M[8] * x + M[9] * y + M[10] * z + M[11] - oz);
    if (world_normals) {
      const double nx = (double)normals[o], ny = (double)normals[o + 1], nz = (double)normals[o + 2];
      const double a = M[0] * nx + M[1] * ny + M[2] * nz, b = M[4] * nx + M[5] * ny + M[6] * nz, c = M[8] * nx + M[9] * ny + M[10] * nz;
      double len = sqrt(a * a + b * b + c * c);
      if (len < 1e-8) len = 1.0;
      world_normals[o] = (float)(a / len); world_normals[o + 1] = (float)(b / len); world_normals[o + 2] = (float)(c / len);
    }
  }
}

// ---- overlap ------------------------------------------------------------------------------------------------------------------
#define SUB_Q_LIMIT 4611686018427387904.0      // 2^62: a voxel coordinate beyond it is clamped (and fails the extent test)
#define SUB_Q_BIAS 0x8000000000000000ull

// voxel coordinates of row r, biased to unsigned; false for a row with a non-finite (world) coordinate.  [f_first, f_last]: the frames of
// the chunk of rows that r lies in (sub_chunk_range; not looked at without poses)
__device__ __forceinline__ bool sub_voxel(const float* __restrict__ P, const double* __restrict__ pose, const int32_t* __restrict__ cu_s,
                                          int f_first, int f_last, int r, double vs, unsigned long long q[3]) {
  const size_t o = (size_t)r * 3;
  double w[3] = {(double)P[o], (double)P[o + 1], (double)P[o + 2]};
  if (pose) {
    const double* M = pose + (size_t)sub_find_in(cu_s, f_first, f_last, r) * 16;
    const double x = w[0], y = w[1], z = w[2];
    w[0] = M[0] * x + M[1] * y + M[2] * z + M[3];
    w[1] = M[4] * x + M[5] * y + M[6] * z + M[7];
    w[2] = M[8] * x + M[9] * y + M[10] * z + M[11];
  }
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    ok = ok && fabs(w[a]) < __builtin_inf();               // false for NaN
    double g = floor(w[a] / vs);                           // a finite coordinate whose quotient overflows is clamped like any other
    g = g > SUB_Q_LIMIT ? SUB_Q_LIMIT : g < -SUB_Q_LIMIT ? -SUB_Q_LIMIT : g;
    q[a] = (unsigned long long)(long long)(ok ? g : 0.0) + SUB_Q_BIAS;
  }
  return ok;
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const unsigned long long w = __shfl_xor(v, o, 64); v = w < v ? w : v; }
  return v;
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const unsigned long long w = __shfl_xor(v, o, 64); v = w > v ? w : v; }
  return v;
}

struct OverlapParams {
  const float* P;
  const double* pose;            // (F,4,4) or null
  const int32_t *cu_s, *seg_off;
  int F, S, N;
  double vs;
  unsigned long long* bounds;    // (6)
  int32_t *flag, *status;
  unsigned long long* keys;      // (N)
  uint32_t* sid;                 // (N)
};

// a capped grid: every block walks several chunks of rows and hands in ONE set of six atomics (all blocks meet on the same six cells)
#define SUB_BOUNDS_BLOCKS 1024
__global__ __launch_bounds__(256) void overlap_bounds_kernel(const OverlapParams a) {
  __shared__ unsigned long long s_lo[4][3], s_hi[4][3];
  unsigned long long lo[3] = {~0ull, ~0ull, ~0ull}, hi[3] = {0ull, 0ull, 0ull};
  const int first = a.seg_off[0], last = a.seg_off[a.S];
  const long chunks = ((long)a.N + SUB_ROWS - 1) / SUB_ROWS;
  for (long ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
    int f_first = 0, f_last = 0;
    if (a.pose) sub_chunk_range(a.cu_s, a.F, ch * SUB_ROWS, a.N, f_first, f_last);
    for (int k = 0; k < SUB_ROWS / 256; ++k) {
      const long rl = ch * SUB_ROWS + k * 256 + threadIdx.x;
      if (rl >= a.N || rl < first || rl >= last) continue;
      unsigned long long q[3];
      if (!sub_voxel(a.P, a.pose, a.cu_s, f_first, f_last, (int)rl, a.vs, q)) continue;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        lo[c] = q[c] < lo[c] ? q[c] : lo[c]; hi[c] = q[c] > hi[c] ? q[c] : hi[c];
        // a quotient that was clamped: the axis does not fit whatever the other rows are
        if (q[c] == SUB_Q_BIAS + (1ull << 62) || q[c] == SUB_Q_BIAS - (1ull << 62)) { lo[c] = 0ull; hi[c] = ~0ull; }
      }
    }
  }
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const unsigned long long l = wave_min_u64(lo[c]), h = wave_max_u64(hi[c]);
    if ((threadIdx.x & 63) == 0) { s_lo[wave][c] = l; s_hi[wave][c] = h; }
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int c = threadIdx.x;
    unsigned long long l = s_lo[0][c], h = s_hi[0][c];
    for (int w = 1; w < 4; ++w) { l = s_lo[w][c] < l ? s_lo[w][c] : l; h = s_hi[w][c] > h ? s_hi[w][c] : h; }
    if (l <= h) { atomicMin(&a.bounds[c], l); atomicMax(&a.bounds[3 + c], h); }
  }
}

__global__ __launch_bounds__(256) void overlap_keys_kernel(const OverlapParams a) {
  const int first = a.seg_off[0], last = a.seg_off[a.S];
  bool fits = true;
#pragma unroll
  for (int c = 0; c < 3; ++c) fits = fits && (a.bounds[c] > a.bounds[3 + c] || a.bounds[3 + c] - a.bounds[c] < (1ull << 21));
  if (!fits && blockIdx.x == 0 && threadIdx.x == 0) {
    atomicOr(a.flag, SUB_ST_EXTENT);
    if (a.status) atomicOr(a.status, SUB_ST_EXTENT);
  }
  int f_first = 0, f_last = 0, s_first, s_last;
  if (a.pose) sub_chunk_range(a.cu_s, a.F, (long)blockIdx.x * SUB_ROWS, a.N, f_first, f_last);
  sub_chunk_range(a.seg_off, a.S, (long)blockIdx.x * SUB_ROWS, a.N, s_first, s_last);
  for (int k = 0; k < SUB_ROWS / 256; ++k) {
    const long rl = (long)blockIdx.x * SUB_ROWS + k * 256 + threadIdx.x;
    if (rl >= a.N) return;
    const int r = (int)rl;
    unsigned long long key = SUB_KEY_NONE;
    uint32_t sid = r < first ? 0u : (uint32_t)a.S + 1u;
    if (r >= first && r < last) {
      sid = (uint32_t)sub_find_in(a.seg_off, s_first, s_last, r) + 1u;
      unsigned long long q[3];
      if (fits && sub_voxel(a.P, a.pose, a.cu_s, f_first, f_last, r, a.vs, q))
        key = (q[0] - a.bounds[0]) | ((q[1] - a.bounds[1]) << 21) | ((q[2] - a.bounds[2]) << 42);
    }
    a.keys[r] = key;
    a.sid[r] = sid;
  }
}

// after the two sorts: sid ascending (every submap where its rows were), keys ascending within a submap, dropped rows last
__global__ __launch_bounds__(256) void overlap_heads_kernel(const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ sid, int N,
                                                            uint32_t* __restrict__ flags) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const unsigned long long k = keys[i];
  flags[i] = (k != SUB_KEY_NONE && (i == 0 || sid[i] != sid[i - 1] || k != keys[i - 1])) ? 1u : 0u;
}
__global__ __launch_bounds__(256) void overlap_compact_kernel(const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ flags,
                                                              const uint32_t* __restrict__ pos, int N, unsigned long long* __restrict__ uniq) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < N && flags[i]) uniq[pos[i] - 1] = keys[i];          // pos: inclusive scan of flags, so pos[i] - 1 < N
}
// cu_unique[s] = heads before submap s's first row; n_voxels; chunk_off[s] = 256-key chunks before submap s.  One block.
__global__ __launch_bounds__(256) void overlap_offsets_kernel(const int32_t* __restrict__ seg_off, const uint32_t* __restrict__ pos, int S,
                                                              int32_t* __restrict__ cu_unique, int32_t* __restrict__ chunk_off,
                                                              long long* __restrict__ n_voxels, const int32_t* __restrict__ flag) {
  if (blockIdx.x != 0) return;
  for (int s = threadIdx.x; s <= S; s += 256) { const int b = seg_off[s]; cu_unique[s] = b > 0 ? (int)pos[b - 1] : 0; }
  __threadfence_block();
  __syncthreads();
  const bool poisoned = *flag != 0;
  for (int s = threadIdx.x; s < S; s += 256) n_voxels[s] = poisoned ? -1ll : (long long)(cu_unique[s + 1] - cu_unique[s]);
  if (threadIdx.x == 0) {
    int acc = 0;
    for (int s = 0; s < S; ++s) { chunk_off[s] = acc; acc += (cu_unique[s + 1] - cu_unique[s] + SUB_CHUNK - 1) / SUB_CHUNK; }
    chunk_off[S] = acc;
  }
}

__global__ __launch_bounds__(SUB_CHUNK) void overlap_intersect_kernel(const unsigned long long* __restrict__ uniq,
                                                                      const int32_t* __restrict__ cu_unique,
                                                                      const int32_t* __restrict__ chunk_off, int S, uint32_t* __restrict__ inter) {
  const int b = blockIdx.x;
  if (b >= chunk_off[S]) return;                               // the grid is the host's bound N / 256 + S
  const int i = sub_find(chunk_off, S, b);
  const int ib = cu_unique[i], ni = cu_unique[i + 1] - ib;
  const int e = (b - chunk_off[i]) * SUB_CHUNK + threadIdx.x;   // this lane's key of submap i
  const bool have = e < ni;
  const int lane = threadIdx.x & 63;
  const int wave_first = (b - chunk_off[i]) * SUB_CHUNK + (threadIdx.x & ~63);
  if (wave_first >= ni) return;                                // the whole wave is past the end: wave-uniform
  const int wave_last = min(wave_first + 63, ni - 1);
  const unsigned long long key = uniq[ib + (have ? e : ni - 1)];
  const unsigned long long kfirst = uniq[ib + wave_first], klast = uniq[ib + wave_last];
  for (int j = 0; j < S; ++j) {
    const int jb = cu_unique[j], nj = cu_unique[j + 1] - jb;
    if (j == i || nj < ni || (nj == ni && j < i) || nj == 0) continue;      // the pair is searched from its smaller side, once
    const unsigned long long* __restrict__ B = uniq + jb;
    // lane 0: first element >= kfirst; lane 1: first element > klast -- the window [w0, w1) of the wave's keys
    const unsigned long long target = lane == 0 ? kfirst : klast;
    int lo = 0, hi = nj;
    if (lane < 2)
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const unsigned long long v = B[mid];
        if (lane == 0 ? v < target : v <= target) lo = mid + 1; else hi = mid;
      }
    const int w0 = __shfl(lo, 0, 64), w1 = __shfl(lo, 1, 64);
    if (w1 <= w0) continue;
    lo = w0; hi = w1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (B[mid] < key) lo = mid + 1; else hi = mid;
    }
    const bool hit = have && lo < w1 && B[lo] == key;
    const int cnt = __popcll(__ballot(hit));
    if (lane == 0 && cnt) atomicAdd(&inter[(size_t)i * S + j], (uint32_t)cnt);       // the cell of the ordered pair (smaller side, larger side)
  }
}

__global__ __launch_bounds__(256) void overlap_finish_kernel(const uint32_t* __restrict__ inter, const int32_t* __restrict__ cu_unique, int S,
                                                             const int32_t* __restrict__ flag, double* __restrict__ ratio) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long)S * S) return;
  if (*flag != 0) { ratio[t] = __builtin_nan(""); return; }
  const int i = (int)(t / S), j = (int)(t % S);
  const long ni = cu_unique[i + 1] - cu_unique[i], nj = cu_unique[j + 1] - cu_unique[j];
  double r = 0.0;
  if (ni > 0 && nj > 0) {
    // exactly one of the two cells of a pair was counted into
    const long n = i == j ? ni : (long)inter[(size_t)i * S + j] + (long)inter[(size_t)j * S + i];
    r = (double)n / (double)(ni + nj - n);
  }
  ratio[t] = r;
}

// ---- connectivity of candidate groups ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void groups_connected_kernel(const double* __restrict__ ratio, int S, const int32_t* __restrict__ groups,
                                                               const int32_t* __restrict__ group_len, int G, int n_max, double lo, double hi,
                                                               uint8_t* __restrict__ connected, int32_t* __restrict__ status) {
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= G) return;
  const int lane = threadIdx.x & 63;
  const int len = group_len[g];
  bool bad = len < 1 || len > n_max;
  const int n = bad ? 0 : len;
  const int m = lane < n ? groups[(size_t)g * n_max + lane] : 0;
  bad = bad || __any(m < 0 || m >= S);
  if (bad) {
    if (lane == 0) { connected[g] = 0; if (status) atomicOr(status, SUB_ST_GROUP); }
    return;
  }
  unsigned long long mask = 0ull;
  for (int l = 0; l < n; ++l) {
    const int ml = __shfl(m, l, 64);
    if (lane < n && l != lane) {
      const double r = lane < l ? ratio[(size_t)m * S + ml] : ratio[(size_t)ml * S + m];      // the pair in the group's order, as the reference
      if (lo <= r && r <= hi) mask |= 1ull << l;
    }
  }
  unsigned long long reach = 1ull;
  for (int it = 0; it < 64; ++it) {
    unsigned long long grow = ((reach >> lane) & 1ull) ? mask : 0ull;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) grow |= __shfl_xor(grow, o, 64);
    const unsigned long long next = reach | grow;
    if (next == reach) break;
    reach = next;
  }
  const unsigned long long full = n == 64 ? ~0ull : (1ull << n) - 1ull;
  if (lane == 0) connected[g] = reach == full ? 1 : 0;
}

// ---- workspaces and entry points --------------------------------------------------------------------------------------------------
static unsigned sub_row_blocks(int64_t N) { return (unsigned)((N + SUB_ROWS - 1) / SUB_ROWS); }

struct FrameWs { int32_t *cu_s, *flag; uint32_t* minmax; size_t total; };
static FrameWs carve_frames(void* base, int F, bool minmax) {
  FrameWs w; Carver c(base);
  w.cu_s = (int32_t*)c.take((size_t)(F + 1) * 4);
  w.flag = (int32_t*)c.take(4);
  w.minmax = minmax ? (uint32_t*)c.take((size_t)F * 8) : nullptr;
  w.total = c.total();
  return w;
}
static bool sub_sizes_ok(int64_t n_points, int32_t F) { return n_points >= 0 && n_points <= 0x7fffffffLL && F >= 0 && F <= SUB_MAX_F; }

extern "C" size_t rap_deskew_workspace_bytes(int64_t n_points, int32_t F) {
  return (!sub_sizes_ok(n_points, F) || F == 0) ? 0 : carve_frames(nullptr, F, true).total;
}
extern "C" int rap_deskew(const float* points, const float* ts, const int32_t* cu_frames, int32_t F, int64_t n_points, const double* rel_pose,
                          float ts_mid, float* out, int32_t* status, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!sub_sizes_ok(n_points, F) || ts_mid != ts_mid || (F == 0 && n_points > 0)) return RAP_ERR_INVALID;
  if (F == 0) return RAP_OK;
  if (!cu_frames || !rel_pose || (n_points > 0 && (!points || !ts || !out))) return RAP_ERR_INVALID;
  if (!ws || ws_bytes < rap_deskew_workspace_bytes(n_points, F)) return RAP_ERR_WORKSPACE;
  const FrameWs w = carve_frames(ws, F, true);
  SubTables t = {cu_frames, nullptr, w.cu_s, nullptr, nullptr, w.flag, status, w.minmax, nullptr, F, 0, (int)n_points};
  hipLaunchKernelGGL(submap_tables_kernel, dim3(1), dim3(256), 0, stream, t);
  RAP_LAUNCH_CHECK();
  if (n_points == 0) return RAP_OK;
  const unsigned nb = sub_row_blocks(n_points);
  hipLaunchKernelGGL(deskew_minmax_kernel, dim3(nb), dim3(256), 0, stream, ts, w.cu_s, F, (int)n_points, w.minmax);
  RAP_LAUNCH_CHECK();
  hipLaunchKernelGGL(deskew_apply_kernel, dim3(nb), dim3(256), 0, stream, points, ts, w.cu_s, F, (int)n_points, rel_pose, ts_mid, w.minmax, w.flag,
                     out);
  RAP_LAUNCH_CHECK();
  return RAP_OK;
}

extern "C" size_t rap_fuse_frames_workspace_bytes(int64_t n_points, int32_t F) {
  return (!sub_sizes_ok(n_points, F) || F == 0) ? 0 : carve_frames(nullptr, F, false).total;
}
extern "C" int rap_fuse_frames(const float* points, const float* normals, const int32_t* cu_frames, int32_t F, int64_t n_points,
                               const double* pose, const double* origin, float* world, float* world_normals, int32_t* status, void* ws,
                               size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!sub_sizes_ok(n_points, F) || (F == 0 && n_points > 0)) return RAP_ERR_INVALID;
  if (F == 0) return RAP_OK;
  if (!cu_frames || !pose || (n_points > 0 && (!points || !world || (normals != nullptr) != (world_normals != nullptr)))) return RAP_ERR_INVALID;
  if (!ws || ws_bytes < rap_fuse_frames_workspace_bytes(n_points, F)) return RAP_ERR_WORKSPACE;
  const FrameWs w = carve_frames(ws, F, false);
  SubTables t = {cu_frames, nullptr, w.cu_s, nullptr, nullptr, w.flag, status, nullptr, nullptr, F, 0, (int)n_points};
  hipLaunchKernelGGL(submap_tables_kernel, dim3(1), dim3(256), 0, stream, t);
  RAP_LAUNCH_CHECK();
  if (n_points == 0) return RAP_OK;
  hipLaunchKernelGGL(fuse_frames_kernel, dim3(sub_row_blocks(n_points)), dim3(256), 0, stream, points, normals, w.cu_s, F, (int)n_points, pose,
                     origin, w.flag, world, world_normals);
  RAP_LAUNCH_CHECK();
  return RAP_OK;
}

// The scratch of the rocPRIM calls is RESERVED by a rule that is host arithmetic (so that the workspace query needs no device): with
// caller-owned double buffers a radix sort keeps digit histograms and one look-back state per digit and block, an inclusive scan one
// state per block -- below 8 bytes per element plus 64 KiB for every configuration rocPRIM ships.  The call asks rocPRIM what it
// wants and refuses (RAP_ERR_WORKSPACE) if that ever exceeded the reservation.
static size_t sub_prim_bytes(int64_t N) { return (size_t)N * 8 + (64u << 10); }

struct OverlapWs {
  int32_t *cu_s, *sf_s, *seg_off, *flag, *cu_unique, *chunk_off;
  unsigned long long *bounds, *keys_a, *keys_b, *uniq;
  uint32_t *sid_a, *sid_b, *flags, *pos, *inter;
  void* prim;
  size_t prim_bytes, inter_bytes, total;
};
static OverlapWs carve_overlap(void* base, int64_t N, int F, int S) {
  OverlapWs w; Carver c(base);
  w.cu_s = (int32_t*)c.take((size_t)(F + 1) * 4);
  w.sf_s = (int32_t*)c.take((size_t)(S + 1) * 4);
  w.seg_off = (int32_t*)c.take((size_t)(S + 1) * 4);
  w.cu_unique = (int32_t*)c.take((size_t)(S + 1) * 4);
  w.chunk_off = (int32_t*)c.take((size_t)(S + 1) * 4);
  w.flag = (int32_t*)c.take(4);
  w.bounds = (unsigned long long*)c.take(6 * 8);
  w.inter_bytes = (size_t)S * S * 4;
  w.inter = (uint32_t*)c.take(w.inter_bytes);
  w.keys_a = (unsigned long long*)c.take((size_t)N * 8);
  w.keys_b = (unsigned long long*)c.take((size_t)N * 8);
  w.uniq = (unsigned long long*)c.take((size_t)N * 8);
  w.sid_a = (uint32_t*)c.take((size_t)N * 4);
  w.sid_b = (uint32_t*)c.take((size_t)N * 4);
  w.flags = (uint32_t*)c.take((size_t)N * 4);
  w.pos = (uint32_t*)c.take((size_t)N * 4);
  w.prim_bytes = sub_prim_bytes(N);
  w.prim = c.take(w.prim_bytes);
  w.total = c.total();
  return w;
}
extern "C" size_t rap_submap_overlap_workspace_bytes(int64_t n_points, int32_t F, int32_t S) {
  return (!sub_sizes_ok(n_points, F) || F <= 0 || S <= 0 || S > SUB_MAX_S) ? 0 : carve_overlap(nullptr, n_points, F, S).total;
}
extern "C" int rap_submap_overlap(const float* points, const int32_t* cu_frames, int32_t F, int64_t n_points, const double* pose,
                                  const int32_t* submap_frames, int32_t S, double voxel_size, double* ratio, int64_t* n_voxels,
                                  int32_t* status, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!sub_sizes_ok(n_points, F) || F <= 0 || S <= 0 || S > SUB_MAX_S || !(voxel_size > 0.0) || !(voxel_size < __builtin_inf())) return RAP_ERR_INVALID;
  if (!cu_frames || !submap_frames || !ratio || !n_voxels || (n_points > 0 && !points)) return RAP_ERR_INVALID;
  if (!ws || ws_bytes < rap_submap_overlap_workspace_bytes(n_points, F, S)) return RAP_ERR_WORKSPACE;
  const OverlapWs w = carve_overlap(ws, n_points, F, S);
  const int N = (int)n_points;
  SubTables t = {cu_frames, submap_frames, w.cu_s, w.sf_s, w.seg_off, w.flag, status, nullptr, w.bounds, F, S, N};
  hipLaunchKernelGGL(submap_tables_kernel, dim3(1), dim3(256), 0, stream, t);
  RAP_LAUNCH_CHECK();
  RAP_HIP_CHECK(hipMemsetAsync(w.inter, 0, w.inter_bytes, stream));
  const unsigned long long* sorted_keys = w.keys_a;
  if (N > 0) {
    const unsigned nb = sub_row_blocks(n_points), nb256 = (unsigned)((n_points + 255) / 256);
    OverlapParams a = {points, pose, w.cu_s, w.seg_off, F, S, N, voxel_size, w.bounds, w.flag, status, w.keys_a, w.sid_a};
    hipLaunchKernelGGL(overlap_bounds_kernel, dim3(nb < SUB_BOUNDS_BLOCKS ? nb : SUB_BOUNDS_BLOCKS), dim3(256), 0, stream, a);
    RAP_LAUNCH_CHECK();
    hipLaunchKernelGGL(overlap_keys_kernel, dim3(nb), dim3(256), 0, stream, a);
    RAP_LAUNCH_CHECK();
    rocprim::double_buffer<unsigned long long> keys(w.keys_a, w.keys_b);
    rocprim::double_buffer<uint32_t> sid(w.sid_a, w.sid_b);
    size_t need = 0;
    RAP_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, need, keys, sid, (size_t)N, 0, 64, stream));
    if (need > w.prim_bytes) return RAP_ERR_WORKSPACE;
    need = w.prim_bytes;
    RAP_HIP_CHECK(rocprim::radix_sort_pairs(w.prim, need, keys, sid, (size_t)N, 0, 64, stream));
    RAP_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, need, sid, keys, (size_t)N, 0, 13, stream));
    if (need > w.prim_bytes) return RAP_ERR_WORKSPACE;
    need = w.prim_bytes;
    RAP_HIP_CHECK(rocprim::radix_sort_pairs(w.prim, need, sid, keys, (size_t)N, 0, 13, stream));      // stable: key order survives
    sorted_keys = keys.current();
    hipLaunchKernelGGL(overlap_heads_kernel, dim3(nb256), dim3(256), 0, stream, sorted_keys, (const uint32_t*)sid.current(), N, w.flags);
    RAP_LAUNCH_CHECK();
    RAP_HIP_CHECK(rocprim::inclusive_scan(nullptr, need, w.flags, w.pos, (size_t)N, rocprim::plus<uint32_t>(), stream));
    if (need > w.prim_bytes) return RAP_ERR_WORKSPACE;
    need = w.prim_bytes;
    RAP_HIP_CHECK(rocprim::inclusive_scan(w.prim, need, w.flags, w.pos, (size_t)N, rocprim::plus<uint32_t>(), stream));
    hipLaunchKernelGGL(overlap_compact_kernel, dim3(nb256), dim3(256), 0, stream, sorted_keys, w.flags, w.pos, N, w.uniq);
    RAP_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(overlap_offsets_kernel, dim3(1), dim3(256), 0, stream, w.seg_off, w.pos, S, w.cu_unique, w.chunk_off, (long long*)n_voxels, w.flag);
  RAP_LAUNCH_CHECK();
  if (N > 0) {
    const unsigned max_chunks = (unsigned)(n_points / SUB_CHUNK) + (unsigned)S;      // sum over submaps of ceil(n_s / 256), n_s summing to <= N
    hipLaunchKernelGGL(overlap_intersect_kernel, dim3(max_chunks), dim3(SUB_CHUNK), 0, stream, w.uniq, w.cu_unique, w.chunk_off, S, w.inter);
    RAP_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(overlap_finish_kernel, dim3((unsigned)(((size_t)S * S + 255) / 256)), dim3(256), 0, stream, w.inter, w.cu_unique, S, w.flag, ratio);
  RAP_LAUNCH_CHECK();
  return RAP_OK;
}

extern "C" int rap_submap_groups_connected(const double* ratio, int32_t S, const int32_t* groups, const int32_t* group_len, int32_t G,
                                           int32_t n_max, double lo, double hi, uint8_t* connected, int32_t* status, void* stream_) {
  if (S <= 0 || S > SUB_MAX_S || G < 0 || n_max < 1 || n_max > 64 || lo != lo || hi != hi) return RAP_ERR_INVALID;
  if (G == 0) return RAP_OK;
  if (!ratio || !groups || !group_len || !connected) return RAP_ERR_INVALID;
  hipLaunchKernelGGL(groups_connected_kernel, dim3((unsigned)((G + 3) / 4)), dim3(256), 0, (hipStream_t)stream_, ratio, S, groups, group_len, G, n_max,
                     lo, hi, connected, status);
  RAP_LAUNCH_CHECK();
  return RAP_OK;
}
