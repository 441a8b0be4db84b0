// Device pieces of the batched ICP that its four query kernels and two finish kernels share (icp.hip, icp_plane.hip, nn_grid.hip): the
// row-vector transform, the head of a query block, the moment epilogues of the two estimators and their partial structs, and the head
// and the stopping rule of a finish wave.  Two search paths that end in the same epilogue give the same bits.  The search pieces
// themselves (nn_d2, the segment clamp, the tile) are nn_tile.h's.
#pragma once
#include "nn_tile.h"
#include "robust_loss.h"

#define ICP_TILE NN_TILE
#define ICP_NMOM 17      // sum x (3), sum y (3), sum x_i y_j (9), sum |x|^2, sum |y|^2

struct IcpPartial { double m[ICP_NMOM]; long long count; };
struct IcpRange { int first, count, x_len, y_len; };

// p R + T in fp32, row vectors (pytorch3d's _apply_similarity_transform with s = 1)
__device__ __forceinline__ void icp_apply(const float* __restrict__ R, const float* __restrict__ T, float x, float y, float z, float& ox, float& oy,
                                          float& oz) {
  ox = x * R[0] + y * R[3] + z * R[6] + T[0];
  oy = x * R[1] + y * R[4] + z * R[7] + T[1];
  oz = x * R[2] + y * R[5] + z * R[8] + T[2];
}

// Head of a query block.  Declares w = its item, prob = the item's problem, active = the lane has a query, (x0, x1, x2) = that query
// (an inactive lane re-reads the item's last one) and (px, py, pz) = x R + T with the problem's current pose, in fp32: what the search
// sees.  The whole block returns on an unused item or a finished problem.  A macro: as a function returning "go on" (its results in a
// struct or in separate references) it moves code in the two grid query kernels.
#define ICP_QUERY_BEGIN(X, items, R, T, done)                                                                 \
  const NnWork w = items[blockIdx.x];                                                                         \
  if (w.x_len <= 0) return;                                                                                   \
  const int prob = w.pad0;                                                                                    \
  if (done[prob]) return;                                                                                     \
  const int q = w.q0 + threadIdx.x;                                                                           \
  const bool active = q < w.x_len;                                                                            \
  const size_t qi = (size_t)w.x_start + (active ? q : w.x_len - 1);                                           \
  const float x0 = X[qi * 3 + 0], x1 = X[qi * 3 + 1], x2 = X[qi * 3 + 2];                                     \
  float px, py, pz;                                                                                           \
  icp_apply(R + (size_t)prob * 9, T + (size_t)prob * 3, x0, x1, x2, px, py, pz)

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
struct IcpPlanePartial { static constexpr int NRED = ICP_PLANE_NMOM; double m[ICP_PLANE_NMOM]; long long count; };
// ... of the robust calls: A = sum w J J^T, b = sum w J r, e = sum 2 rho, and behind them W = sum w (robust_loss.h)
#define ICP_PLANE_WMOM (ICP_PLANE_NMOM + 1)
struct IcpPlaneWPartial { static constexpr int NRED = ICP_PLANE_WMOM; double m[ICP_PLANE_WMOM]; long long count; };

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

// Epilogue of a block of ICP_TILE queries for the point-to-plane step: (px, py, pz) is the MOVED query (what
// the search saw, fp32), y = Y[y_start + besti] its neighbour, n = Yn[y_start + besti] the neighbour's normal.  In double:
// r = (p - y) . n, J = [p x n, n]; the gated pairs with a usable normal are summed per wave, then over the four waves in a fixed order.
// Every thread of the block calls it.  Both search paths end here, so they return the same bits.
// Partial = IcpPlaneWPartial (the robust calls): every pair enters with its weight w(r) of loss LOSS at scale k, e sums 2 rho(r), W = sum w
// is carried as a 29th moment, and an active lane stores its weight (0 for a pair that does not count) to wrow[its row] where wrow is
// given.  LOSS none there multiplies nothing and sums the statements of the plain partial: the same bits.
template <int LOSS, class Partial>
__device__ __forceinline__ void icp_plane_moments(bool active, int besti, float best, float gate, float px, float py, float pz,
                                                  const float* __restrict__ Y, const float* __restrict__ Yn, int y_start,
                                                  double (*red_m)[Partial::NRED], int* red_n, Partial* __restrict__ out, double k = 0.0,
                                                  float* __restrict__ wrow = nullptr, size_t qi = 0) {
  constexpr bool weighted = Partial::NRED == ICP_PLANE_WMOM;
  double J[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, r = 0.0;
  double wt = 0.0, e = 0.0;
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
      if (weighted) {
        wt = 1.0;
        if (LOSS != RAP_LOSS_NONE) {
          double rho;
          rap_robust<LOSS>(r, k, wt, rho);
          e = 2.0 * rho;
        }
      }
    }
  }
  if (weighted && wrow && active) wrow[qi] = (float)wt;
  double Jw[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) Jw[i] = weighted && LOSS != RAP_LOSS_NONE ? wt * J[i] : J[i];
  double* row = red_m[threadIdx.x >> 6];
  int at = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = i; j < 6; ++j) icp_plane_put(Jw[i] * J[j], row, at++);
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) icp_plane_put(Jw[i] * r, row, 21 + i);
  icp_plane_put(weighted && LOSS != RAP_LOSS_NONE ? e : r * r, row, 27);
  if (weighted) icp_plane_put(wt, row, ICP_PLANE_NMOM);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if ((threadIdx.x & 63) == 0) red_n[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x < Partial::NRED)
    out->m[threadIdx.x] = (red_m[0][threadIdx.x] + red_m[1][threadIdx.x]) + (red_m[2][threadIdx.x] + red_m[3][threadIdx.x]);
  if (threadIdx.x == Partial::NRED) out->count = (long long)(red_n[0] + red_n[1] + red_n[2] + red_n[3]);
}

// F<loss>(args...) for the run-time loss code (checked by the entry point: 0 .. 3)
#define RAP_LOSS_DISPATCH(loss, F, ...)                       \
  switch (loss) {                                             \
    case RAP_LOSS_HUBER: F<RAP_LOSS_HUBER>(__VA_ARGS__); break;   \
    case RAP_LOSS_CAUCHY: F<RAP_LOSS_CAUCHY>(__VA_ARGS__); break; \
    case RAP_LOSS_TUKEY: F<RAP_LOSS_TUKEY>(__VA_ARGS__); break;   \
    default: F<RAP_LOSS_NONE>(__VA_ARGS__); break;                \
  }

// A finish wave (one per problem) starts here: declares m[NMOM] = the item partials of range r added lane-strided in item order, then
// over the wave, and n = the number of pairs.  A macro: as a function (the range by value or as two ints, m by reference or by pointer)
// the finish kernels get another register allocation.
#define ICP_SUM_PARTIALS(NMOM, Partial, partials, r, m, n)                                \
  double m[NMOM];                                                                         \
  _Pragma("unroll") for (int i = 0; i < NMOM; ++i) m[i] = 0.0;                            \
  long long n = 0;                                                                        \
  for (int i = threadIdx.x; i < r.count; i += 64) {                                       \
    const Partial* p = partials + r.first + i;                                            \
    _Pragma("unroll") for (int j = 0; j < NMOM; ++j) m[j] += p->m[j];                     \
    n += p->count;                                                                        \
  }                                                                                       \
  _Pragma("unroll") for (int i = 0; i < NMOM; ++i) m[i] = wave_sum_d(m[i]);               \
  _Pragma("unroll") for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);

// ... and ends here, lane 0: pytorch3d's stopping rule on the relative decrease of the rmse, and the bookkeeping of iteration `it`
__device__ __forceinline__ void icp_finish_end(int k, int it, double rmse, double rel_thr, float* __restrict__ rmse_out,
                                               int32_t* __restrict__ iterations, uint8_t* __restrict__ converged, double* __restrict__ prev,
                                               int32_t* __restrict__ done) {
  const double pv = prev[k];
  const double rel = pv < 0.0 ? 1.0 : (pv - rmse) / pv;
  const bool stop = pv == 0.0 || rel <= rel_thr;     // pv == 0: 0 / 0 in pytorch3d, which then runs to the limit with the same transform
  rmse_out[k] = (float)rmse;
  iterations[k] = it + 1;
  if (stop) { converged[k] = 1; done[k] = 1; }
  prev[k] = rmse;
}
