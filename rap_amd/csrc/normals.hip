// Surface normals of packed clouds on the device: the plane fit of every point's neighbourhood, Open3D's estimate_normals with a
// hybrid search as the reference calls it (dataset_process/utils/dataset_utils.py:325-358: radius 0.5, max_nn 20).  K segments of one
// (n_points,3) array; for row i of segment k the neighbours are the rows j of the SAME segment with sqrtf(nn_d2(p_i, p_j)) <= radius
// (radius <= 0: no limit), of those the max_nn with the smallest (d2, j), the row itself included; rows with a non-finite coordinate
// are never neighbours.  Mean and centred covariance (over the count) in fp64 from the fp32 coordinates, the unit eigenvector of the
// smallest eigenvalue from an fp64 Jacobi (kabsch.h), rounded to fp32.  Fewer than three neighbours: normal and eigenvalues 0.
//
//   normals_items_kernel   segment table -> items of 256 queries of one segment (NnWork with x = y = the segment)
//   normals_kernel         a tiled brute-force search on nn_tile.h's tile: the candidates go through LDS, one ds_read_b128 broadcast
//                          per candidate.  Each lane keeps the admission limit in a register: the d2 of its current max_nn-th best
//                          once its list is full, the radius bound before.  The list of the max_nn best lives in LDS as
//                          [slot][lane], so the lanes of a wave hit different banks; max_nn x 256 x 8 bytes beside the 4 KB tile
//                          (64 KB at 32 slots: dynamic LDS).  An entry is one 64-bit key, d2's bits above j: for d2 >= 0 the order
//                          of the keys IS the order of (d2, j).  The list is not kept sorted: a candidate that beats the worst key
//                          replaces it, and max_nn reads, four in flight at a time, find the new worst (a sorted list costs a chain
//                          of dependent LDS shifts per insertion, and a wave takes the branch when any of its 64 lanes does: about
//                          k ln(n / k) insertions per lane are rare, 64 times that per wave are not; DESIGN.md section 7.3 has the
//                          numbers).  The covariance pass re-reads the winners by index, in slot order.
// No atomics, no host read, capturable; a row's bits depend on its own segment only.  The grid-index variant for clouds
// that are not voxel-downsampled first (rap_estimate_normals_grid: the same neighbour sets from the k-best walk) is nn_knn.hip, DESIGN.md
// section 7.6.
#include "nn_tile.h"
#include "kabsch.h"

#define NRM_TILE NN_TILE

struct NormalsParams {
  const float* P;
  const NnWork* items;
  const float* viewpoint;     // (K,3) or null
  float* normals;
  float* eigenvalues;         // (n_points,3) or null
  float radius;
  float r2_limit;             // d2 above this cannot pass sqrtf(d2) <= radius (inf without a radius)
  int max_nn;
};

// A segment that repeats an earlier one (the y segments of an ICP call may: several problems against one target) is worked once:
// repeat[k] = 1.  Segments that overlap without being equal stay the caller's responsibility.
__global__ __launch_bounds__(256) void normals_items_kernel(const int32_t* __restrict__ seg, int K, long N, NnWork* __restrict__ items,
                                                            int max_items, int32_t* __restrict__ repeat) {
  if (blockIdx.x != 0) return;
  for (int k = threadIdx.x; k < K; k += 256) {
    int s, len, sj, lj, r = 0;
    nn_segment(seg, k, N, s, len);
    for (int j = 0; j < k && !r; ++j) {
      nn_segment(seg, j, N, sj, lj);
      r = sj == s && lj == len;
    }
    repeat[k] = r;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  int n = 0;
  for (int k = 0; k < K; ++k) {
    int s, len;
    nn_segment(seg, k, N, s, len);
    if (repeat[k]) continue;
    nn_emit_items_whole(items, n, max_items, s, len, s, len, k);
  }
  nn_zero_items(items, n, max_items);
}

__host__ __device__ inline int normals_slots(int max_nn) { return (max_nn + 3) & ~3; }

__global__ __launch_bounds__(NRM_TILE) void normals_kernel(const NormalsParams a) {
  // two LDS objects, so that the compiler knows a store to the list cannot change the tile and keeps the tile reads of the unrolled
  // candidate loop in flight across the insertion branch
  __shared__ float4 tile[NRM_TILE];                                  // the candidates
  extern __shared__ unsigned long long nrm_list[];                   // [slots4][NRM_TILE] keys (d2 bits << 32 | j)
  unsigned long long* list = nrm_list;
  const NnWork w = a.items[blockIdx.x];
  if (w.x_len <= 0) return;
  const int lane = threadIdx.x;
  const int q = w.q0 + lane;
  const bool active = q < w.x_len;
  const size_t qi = (size_t)w.x_start + (active ? q : w.x_len - 1);
  const float qx = a.P[qi * 3 + 0], qy = a.P[qi * 3 + 1], qz = a.P[qi * 3 + 2];
  const int max_nn = a.max_nn;
  // the slots are padded to a multiple of four with the key 0, which is never the worst of a full list (keys are distinct and >= 0)
  const int slots4 = normals_slots(max_nn);
  for (int s = max_nn; s < slots4; ++s) list[s * NRM_TILE + lane] = 0ull;
  int cnt = 0, worst_slot = 0;
  unsigned long long worst = 0ull;                                   // the largest key of a full list
  float limit = active ? a.r2_limit : -1.f;                          // an inactive lane admits nothing
  for (int k0 = 0; k0 < w.y_len; k0 += NRM_TILE) {
    nn_tile_stage(tile, k0, w.y_len, make_float4(0.f, 0.f, 0.f, 0.f), [&](int k, float4& c) { nn_row(a.P, (size_t)w.y_start + k, c); });
    const int nk = min(NRM_TILE, w.y_len - k0);
#pragma unroll 8
    for (int j = 0; j < nk; ++j) {
      const float4 p = tile[j];
      const float d2 = nn_d2(qx, qy, qz, p.x, p.y, p.z);
      if (d2 <= limit) {                                             // false for NaN
        // exact rules: finite, inside the radius, and a smaller (d2, j) than the worst entry of a full list
        if (d2 < __builtin_inff() && (!(a.radius > 0.f) || sqrtf(d2) <= a.radius)) {
          const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)(k0 + j);
          bool rescan = false;
          if (cnt < max_nn) {
            list[cnt * NRM_TILE + lane] = key;
            rescan = ++cnt == max_nn;
          } else if (key < worst) {
            list[worst_slot * NRM_TILE + lane] = key;
            rescan = true;
          }
          if (rescan) {                                              // the new worst entry and the new limit: four reads in flight at a time
            worst = 0ull;
            for (int s = 0; s < slots4; s += 4) {
              const unsigned long long v0 = list[(s + 0) * NRM_TILE + lane], v1 = list[(s + 1) * NRM_TILE + lane],
                                       v2 = list[(s + 2) * NRM_TILE + lane], v3 = list[(s + 3) * NRM_TILE + lane];
              if (v0 > worst) { worst = v0; worst_slot = s; }
              if (v1 > worst) { worst = v1; worst_slot = s + 1; }
              if (v2 > worst) { worst = v2; worst_slot = s + 2; }
              if (v3 > worst) { worst = v3; worst_slot = s + 3; }
            }
            limit = __uint_as_float((unsigned)(worst >> 32));
          }
        }
      }
    }
  }
  if (!active) return;
  double nv[3] = {0.0, 0.0, 0.0}, lam[3] = {0.0, 0.0, 0.0};
  if (cnt >= 3) {
    double mu[3] = {0.0, 0.0, 0.0};
    for (int s = 0; s < cnt; ++s) {
      const float* p = a.P + ((size_t)w.y_start + (unsigned)list[s * NRM_TILE + lane]) * 3;
      mu[0] += (double)p[0]; mu[1] += (double)p[1]; mu[2] += (double)p[2];
    }
    const double inv = 1.0 / (double)cnt;
    mu[0] *= inv; mu[1] *= inv; mu[2] *= inv;
    double c00 = 0.0, c01 = 0.0, c02 = 0.0, c11 = 0.0, c12 = 0.0, c22 = 0.0;
    for (int s = 0; s < cnt; ++s) {
      const float* p = a.P + ((size_t)w.y_start + (unsigned)list[s * NRM_TILE + lane]) * 3;
      const double dx = (double)p[0] - mu[0], dy = (double)p[1] - mu[1], dz = (double)p[2] - mu[2];
      c00 += dx * dx; c01 += dx * dy; c02 += dx * dz; c11 += dy * dy; c12 += dy * dz; c22 += dz * dz;
    }
    const double C[3][3] = {{c00 * inv, c01 * inv, c02 * inv}, {c01 * inv, c11 * inv, c12 * inv}, {c02 * inv, c12 * inv, c22 * inv}};
    rap_sym_eig3_smallest(C, lam, nv);
    bool flip;
    if (a.viewpoint) {
      const float* v = a.viewpoint + (size_t)w.pad0 * 3;
      flip = nv[0] * ((double)v[0] - (double)qx) + nv[1] * ((double)v[1] - (double)qy) + nv[2] * ((double)v[2] - (double)qz) < 0.0;
    } else {                                                         // the component of largest magnitude positive, lowest index among equals
      int big = 0;
      if (fabs(nv[1]) > fabs(nv[big])) big = 1;
      if (fabs(nv[2]) > fabs(nv[big])) big = 2;
      flip = nv[big] < 0.0;
    }
    if (flip) { nv[0] = -nv[0]; nv[1] = -nv[1]; nv[2] = -nv[2]; }
  }
  a.normals[qi * 3 + 0] = (float)nv[0]; a.normals[qi * 3 + 1] = (float)nv[1]; a.normals[qi * 3 + 2] = (float)nv[2];
  if (a.eigenvalues) {
    a.eigenvalues[qi * 3 + 0] = (float)lam[0]; a.eigenvalues[qi * 3 + 1] = (float)lam[1]; a.eigenvalues[qi * 3 + 2] = (float)lam[2];
  }
}

int launch_normals_items(hipStream_t stream, const int32_t* seg, int K, long N, NnWork* items, int32_t* repeat) {
  hipLaunchKernelGGL(normals_items_kernel, dim3(1), dim3(256), 0, stream, seg, K, N, items, (int)nn_max_items(N, K), repeat);
  RAP_LAUNCH_CHECK();
  return RAP_OK;
}

int launch_estimate_normals(hipStream_t stream, const float* P, const int32_t* seg, int K, long N, int max_nn, float radius,
                            const float* viewpoint, float* normals, float* eigenvalues, NnWork* items, int32_t* repeat) {
  const int max_items = (int)nn_max_items(N, K);
  const int rc = launch_normals_items(stream, seg, K, N, items, repeat);
  if (rc) return rc;
  NormalsParams a;
  a.P = P; a.items = items; a.viewpoint = viewpoint; a.normals = normals; a.eigenvalues = eigenvalues;
  a.radius = radius > 0.f ? radius : 0.f;
  // d2 > radius^2 (1 + 2^-16) implies sqrtf(d2) > radius after rounding (the margin of the grid search's gate, nn_grid.hip)
  a.r2_limit = radius > 0.f ? radius * radius * 1.0000152587890625f : __builtin_inff();
  a.max_nn = max_nn;
  const int lds = normals_slots(max_nn) * NRM_TILE * 8;      // the list; the 4 KB tile is static
  return rap_launch_dyn_lds(normals_kernel, dim3(max_items), dim3(NRM_TILE), lds, stream, a);
}
