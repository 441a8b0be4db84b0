// Device pieces shared by the brute-force ICP (icp.hip), the grid search (nn_grid.hip) and the nearest-neighbour metrics
// (nn_metrics.hip): the squared distance every search compares, the segment clamp, the row-vector transform and the moment epilogue
// of an ICP query block.  Two search paths that share these give the same bits.
#pragma once
#include "kernels.h"

#define ICP_TILE 256
#define ICP_NMOM 17      // sum x (3), sum y (3), sum x_i y_j (9), sum |x|^2, sum |y|^2

struct IcpPartial { double m[ICP_NMOM]; long long count; };
struct IcpRange { int first, count, x_len, y_len; };

// |q - p|^2 in fp32 from direct differences: the one expression every search compares.  hipcc contracts it to dx*dx rounded, dy*dy fused
// onto it, dz*dz rounded, one add (v_pk_mul_f32 of dx and dz, v_fma_f32 of dy, v_add_f32 in the tiled kernels; v_mul, v_fmac, v_mul, v_add
// in the grid walk): the same chain in nn_query_kernel, icp_query_kernel and the grid kernels, checked in their disassembly (DESIGN.md
// section 7.2).  Pinning the chain with explicit fma / contraction pragmas was tried and costs the tiled kernels their packed math.
__device__ __forceinline__ float nn_d2(float qx, float qy, float qz, float px, float py, float pz) {
  const float dx = qx - px, dy = qy - py, dz = qz - pz;
  return dx * dx + dy * dy + dz * dz;
}

// (start, len) of row k clamped to [0, limit): an inconsistent table cannot make a kernel index outside the array
__device__ __forceinline__ void icp_segment(const int32_t* __restrict__ seg, int k, long limit, int& start, int& len) {
  long s = seg[(size_t)k * 2], n = seg[(size_t)k * 2 + 1];
  s = s < 0 ? 0 : s > limit ? limit : s;
  n = n < 0 ? 0 : n > limit - s ? limit - s : n;
  start = (int)s; len = (int)n;
}

// p R + T in fp32, row vectors (pytorch3d's _apply_similarity_transform with s = 1)
__device__ __forceinline__ void icp_apply(const float* __restrict__ R, const float* __restrict__ T, float x, float y, float z, float& ox, float& oy,
                                          float& oz) {
  ox = x * R[0] + y * R[3] + z * R[6] + T[0];
  oy = x * R[1] + y * R[4] + z * R[7] + T[1];
  oz = x * R[2] + y * R[5] + z * R[8] + T[2];
}

// Epilogue of a block of ICP_TILE queries (one per lane, in X's order): the gated count and the raw moments (double) of the ORIGINAL x
// and its neighbour y = Y[y_start + besti], summed per wave, then over the four waves in a fixed order, into the item's partial.
// Every thread of the block calls it.  red_m / red_n: shared memory of the block.
__device__ __forceinline__ void icp_moments(bool active, int besti, float best, float gate, float x0, float x1, float x2,
                                            const float* __restrict__ Y, int y_start, double (*red_m)[ICP_NMOM], int* red_n,
                                            IcpPartial* __restrict__ out) {
  double m[ICP_NMOM];
#pragma unroll
  for (int i = 0; i < ICP_NMOM; ++i) m[i] = 0.0;
  int n = 0;
  if (active && besti >= 0 && (!(gate > 0.f) || sqrtf(best) <= gate)) {
    const size_t ti = (size_t)y_start + besti;
    const double xs[3] = {(double)x0, (double)x1, (double)x2};
    const double ys[3] = {(double)Y[ti * 3 + 0], (double)Y[ti * 3 + 1], (double)Y[ti * 3 + 2]};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      m[i] = xs[i]; m[3 + i] = ys[i];
#pragma unroll
      for (int j = 0; j < 3; ++j) m[6 + 3 * i + j] = xs[i] * ys[j];
    }
    m[15] = xs[0] * xs[0] + xs[1] * xs[1] + xs[2] * xs[2];
    m[16] = ys[0] * ys[0] + ys[1] * ys[1] + ys[2] * ys[2];
    n = 1;
  }
#pragma unroll
  for (int i = 0; i < ICP_NMOM; ++i) m[i] = wave_sum_d(m[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int i = 0; i < ICP_NMOM; ++i) red_m[threadIdx.x >> 6][i] = m[i];
    red_n[threadIdx.x >> 6] = n;
  }
  __syncthreads();
  if (threadIdx.x < ICP_NMOM) out->m[threadIdx.x] = (red_m[0][threadIdx.x] + red_m[1][threadIdx.x]) + (red_m[2][threadIdx.x] + red_m[3][threadIdx.x]);
  if (threadIdx.x == ICP_NMOM) out->count = (long long)(red_n[0] + red_n[1] + red_n[2] + red_n[3]);
}

// ---- point-to-plane (icp_plane.hip; the grid path in nn_grid.hip) ----
#define ICP_PLANE_NMOM 28      // upper triangle of A = sum J J^T, row by row (21), b = sum J r (6), e = sum r^2
struct IcpPlanePartial { double m[ICP_PLANE_NMOM]; long long count; };

// the neighbour's normal counts when every component is finite and it is not the zero vector ("no estimate", normals.hip)
__device__ __forceinline__ bool icp_normal_ok(float nx, float ny, float nz) {
  const float inf = __builtin_inff();
  return fabsf(nx) < inf && fabsf(ny) < inf && fabsf(nz) < inf && (nx != 0.f || ny != 0.f || nz != 0.f);
}

// wave sum of one moment into the wave's row of red_m; the sums of a block are taken one at a time, so that no more than the seven
// doubles of J and r stay live across them, not 28 accumulators (the query kernels stay at 50 / 68 VGPRs)
__device__ __forceinline__ void icp_plane_put(double v, double* __restrict__ row, int i) {
  v = wave_sum_d(v);
  if ((threadIdx.x & 63) == 0) row[i] = v;
}

// Epilogue of a block of ICP_TILE queries for the point-to-plane step, built as icp_moments is: (px, py, pz) is the MOVED query (what
// the search saw, fp32), y = Y[y_start + besti] its neighbour, n = Yn[y_start + besti] the neighbour's normal.  In double:
// r = (p - y) . n, J = [p x n, n]; the gated pairs with a usable normal are summed per wave, then over the four waves in a fixed order.
// Every thread of the block calls it.  Both search paths end here, so they return the same bits.
__device__ __forceinline__ void icp_plane_moments(bool active, int besti, float best, float gate, float px, float py, float pz,
                                                  const float* __restrict__ Y, const float* __restrict__ Yn, int y_start,
                                                  double (*red_m)[ICP_PLANE_NMOM], int* red_n, IcpPlanePartial* __restrict__ out) {
  double J[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, r = 0.0;
  int n = 0;
  if (active && besti >= 0 && (!(gate > 0.f) || sqrtf(best) <= gate)) {
    const size_t ti = (size_t)y_start + besti;
    const float n0 = Yn[ti * 3 + 0], n1 = Yn[ti * 3 + 1], n2 = Yn[ti * 3 + 2];
    if (icp_normal_ok(n0, n1, n2)) {
      const double p[3] = {(double)px, (double)py, (double)pz};
      const double nv[3] = {(double)n0, (double)n1, (double)n2};
      const double d[3] = {p[0] - (double)Y[ti * 3 + 0], p[1] - (double)Y[ti * 3 + 1], p[2] - (double)Y[ti * 3 + 2]};
      r = d[0] * nv[0] + d[1] * nv[1] + d[2] * nv[2];
      J[0] = p[1] * nv[2] - p[2] * nv[1];
      J[1] = p[2] * nv[0] - p[0] * nv[2];
      J[2] = p[0] * nv[1] - p[1] * nv[0];
      J[3] = nv[0]; J[4] = nv[1]; J[5] = nv[2];
      n = 1;
    }
  }
  double* row = red_m[threadIdx.x >> 6];
  int at = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = i; j < 6; ++j) icp_plane_put(J[i] * J[j], row, at++);
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) icp_plane_put(J[i] * r, row, 21 + i);
  icp_plane_put(r * r, row, 27);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if ((threadIdx.x & 63) == 0) red_n[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x < ICP_PLANE_NMOM)
    out->m[threadIdx.x] = (red_m[0][threadIdx.x] + red_m[1][threadIdx.x]) + (red_m[2][threadIdx.x] + red_m[3][threadIdx.x]);
  if (threadIdx.x == ICP_PLANE_NMOM) out->count = (long long)(red_n[0] + red_n[1] + red_n[2] + red_n[3]);
}
