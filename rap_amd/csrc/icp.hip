// Batched point-to-point ICP on the device: K independent problems, each aligning a segment of X to a segment of Y, with pytorch3d's
// iterative_closest_point semantics (the reference takes it from there: eval/metrics.py:79 and :261, one problem at a time with a KNN
// launch, an SVD launch and a host read of the convergence test per iteration).  Row-vector convention Xt = X R + T, det R = +1.
//
//   icp_setup_kernel    segment tables -> items of 256 queries of one problem + every problem's item range; the state of every problem
//                       (R, T = init or identity, no previous rmse, iterations 0, done = a segment is empty)
//   per iteration, enqueued max_iterations times up front:
//   icp_query_kernel    pair_query_kernel's search (candidate tile through LDS, one ds_read_b128 broadcast per candidate, strict < so the
//                       first arg-min wins) with the problem's current R, T applied to the query when it is LOADED; epilogue: the block
//                       reduces the gated count and the raw moments (double) of the ORIGINAL x and its neighbour y into one partial per item
//   icp_finish_kernel   one wave per problem: item partials added lane-strided in item order, the 3 x 3 Kabsch solve (kabsch.h), the rmse
//                       from the same centred moments, the stopping rule, the new state
//   icp_apply_kernel    optional: Xt = X R + T of every point of a problem
//
// The convergence decision stays on the device: blocks and waves of a problem whose done flag is set return at once, so the host never
// reads anything back and the whole call can be captured into a graph.  Nothing N x M and no per-point index or distance reaches HBM.
// Deterministic (no floating-point atomics) and batch-independent: a problem's arithmetic depends on its own segments only.
#include "icp.h"
#include "kabsch.h"

size_t icp_partial_bytes() { return sizeof(IcpPartial); }

__global__ __launch_bounds__(ICP_TILE) void icp_setup_kernel(const int32_t* __restrict__ x_seg, const int32_t* __restrict__ y_seg, int K, long NX,
                                                             long NY, const float* __restrict__ init_R, const float* __restrict__ init_T,
                                                             NnWork* __restrict__ items, IcpRange* __restrict__ ranges, int max_items,
                                                             float* __restrict__ R, float* __restrict__ T, float* __restrict__ rmse,
                                                             int32_t* __restrict__ iterations, uint8_t* __restrict__ converged,
                                                             double* __restrict__ prev, int32_t* __restrict__ done) {
  if (blockIdx.x != 0) return;
  if (threadIdx.x == 0) {
    int n = 0;
    for (int k = 0; k < K; ++k) {
      int xs, xn, ys, yn;
      icp_segment(x_seg, k, NX, xs, xn);
      icp_segment(y_seg, k, NY, ys, yn);
      IcpRange r = {n, 0, xn, yn};
      // a problem with an empty Y keeps its items: icp_apply_kernel moves its points by the initial transform.  x segments that overlap
      // can ask for more items than the list holds: such a problem is left out whole (it reports as an empty one)
      const int want = (xn + ICP_TILE - 1) / ICP_TILE;
      if (xn > 0 && want <= max_items - n) {
        for (int q0 = 0; q0 < xn; q0 += ICP_TILE) { NnWork w = {xs, xn, q0, ys, yn, k, 0, 0}; items[n++] = w; }
        r.count = want;
      }
      ranges[k] = r;
    }
    for (; n < max_items; ++n) { NnWork w = {0, 0, 0, 0, 0, 0, 0, 0}; items[n] = w; }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < K; k += ICP_TILE) {
#pragma unroll
    for (int i = 0; i < 9; ++i) R[(size_t)k * 9 + i] = init_R ? init_R[(size_t)k * 9 + i] : (i % 4 == 0 ? 1.f : 0.f);
#pragma unroll
    for (int i = 0; i < 3; ++i) T[(size_t)k * 3 + i] = init_T ? init_T[(size_t)k * 3 + i] : 0.f;
    rmse[k] = __builtin_nanf("");
    iterations[k] = 0;
    converged[k] = 0;
    prev[k] = -1.0;                                  // "none": an rmse is never negative
    done[k] = ranges[k].count > 0 && ranges[k].y_len > 0 ? 0 : 1;
  }
}

__global__ __launch_bounds__(ICP_TILE) void icp_query_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                             const NnWork* __restrict__ items, const float* __restrict__ R,
                                                             const float* __restrict__ T, const int32_t* __restrict__ done, float gate,
                                                             IcpPartial* __restrict__ partials) {
  __shared__ float4 tile[ICP_TILE];
  __shared__ double red_m[ICP_TILE / 64][ICP_NMOM];
  __shared__ int red_n[ICP_TILE / 64];
  const NnWork w = items[blockIdx.x];
  if (w.x_len <= 0) return;
  const int prob = w.pad0;
  if (done[prob]) return;
  const int q = w.q0 + threadIdx.x;
  const bool active = q < w.x_len;
  const size_t qi = (size_t)w.x_start + (active ? q : w.x_len - 1);
  const float x0 = X[qi * 3 + 0], x1 = X[qi * 3 + 1], x2 = X[qi * 3 + 2];
  float qx, qy, qz;
  icp_apply(R + (size_t)prob * 9, T + (size_t)prob * 3, x0, x1, x2, qx, qy, qz);
  float best = __builtin_inff();
  int besti = -1;
  for (int k0 = 0; k0 < w.y_len; k0 += ICP_TILE) {
    const int k = k0 + threadIdx.x;
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
    if (k < w.y_len) {
      const size_t ki = (size_t)w.y_start + k;
      c.x = Y[ki * 3 + 0]; c.y = Y[ki * 3 + 1]; c.z = Y[ki * 3 + 2];
    }
    __syncthreads();
    tile[threadIdx.x] = c;
    __syncthreads();
    const int nk = min(ICP_TILE, w.y_len - k0);
#pragma unroll 8
    for (int j = 0; j < nk; ++j) {
      const float4 p = tile[j];
      const float d2 = nn_d2(qx, qy, qz, p.x, p.y, p.z);
      if (d2 < best) { best = d2; besti = k0 + j; }      // strict <: the first minimum wins, as nn_query_kernel
    }
  }
  icp_moments(active, besti, best, gate, x0, x1, x2, Y, w.y_start, red_m, red_n, partials + blockIdx.x);
}

__global__ __launch_bounds__(64) void icp_finish_kernel(const IcpPartial* __restrict__ partials, const IcpRange* __restrict__ ranges, int it,
                                                        double rel_thr, float* __restrict__ R_out, float* __restrict__ T_out,
                                                        float* __restrict__ rmse_out, int32_t* __restrict__ iterations,
                                                        uint8_t* __restrict__ converged, double* __restrict__ prev, int32_t* __restrict__ done) {
  const int k = blockIdx.x;
  if (done[k]) return;
  const IcpRange r = ranges[k];
  double m[ICP_NMOM];
#pragma unroll
  for (int i = 0; i < ICP_NMOM; ++i) m[i] = 0.0;
  long long n = 0;
  for (int i = threadIdx.x; i < r.count; i += 64) {
    const IcpPartial* p = partials + r.first + i;
#pragma unroll
    for (int j = 0; j < ICP_NMOM; ++j) m[j] += p->m[j];
    n += p->count;
  }
#pragma unroll
  for (int i = 0; i < ICP_NMOM; ++i) m[i] = wave_sum_d(m[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if (threadIdx.x != 0) return;
  if (n == 0) {                                      // the gate left no correspondence: stop with the last R, T
    rmse_out[k] = __builtin_inff();
    done[k] = 1;
    return;
  }
  // rap_kabsch_from_moments' arithmetic, with the fp64 rotation kept for the rmse.  kabsch.h solves for column vectors
  // (tgt = Rc src + t, t = mu_t - Rc mu_s); the row-vector R of this file is its transpose.
  const double inv = 1.0 / (double)n;
  const double mx[3] = {m[0] * inv, m[1] * inv, m[2] * inv};
  const double my[3] = {m[3] * inv, m[4] * inv, m[5] * inv};
  double H[3][3], Rc[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) H[i][j] = m[6 + 3 * i + j] - (double)n * mx[i] * my[j];
  rap_kabsch_from_H(H, Rc);
  double rh = 0.0;                                   // sum_i (x_i - mu_x) R . (y_i - mu_y) = sum_ij R[i][j] H[i][j]
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) {
      R_out[(size_t)k * 9 + 3 * i + j] = (float)Rc[j][i];
      rh += Rc[j][i] * H[i][j];
    }
    T_out[(size_t)k * 3 + i] = (float)(my[i] - (Rc[i][0] * mx[0] + Rc[i][1] * mx[1] + Rc[i][2] * mx[2]));
  }
  // with T = mu_y - mu_x R the residual of a pair is (x - mu_x) R - (y - mu_y):  sum |.|^2 = Sxx + Syy - 2 sum_ij R_ij H_ij  (R orthogonal)
  const double sxx = m[15] - (double)n * (mx[0] * mx[0] + mx[1] * mx[1] + mx[2] * mx[2]);
  const double syy = m[16] - (double)n * (my[0] * my[0] + my[1] * my[1] + my[2] * my[2]);
  const double rmse = sqrt(fmax((sxx + syy - 2.0 * rh) * inv, 0.0));
  const double pv = prev[k];
  const double rel = pv < 0.0 ? 1.0 : (pv - rmse) / pv;
  const bool stop = pv == 0.0 || rel <= rel_thr;     // pv == 0: 0 / 0 in pytorch3d, which then runs to the limit with the same transform
  rmse_out[k] = (float)rmse;
  iterations[k] = it + 1;
  if (stop) { converged[k] = 1; done[k] = 1; }
  prev[k] = rmse;
}

__global__ __launch_bounds__(ICP_TILE) void icp_apply_kernel(const float* __restrict__ X, const NnWork* __restrict__ items,
                                                             const float* __restrict__ R, const float* __restrict__ T, float* __restrict__ Xt) {
  const NnWork w = items[blockIdx.x];
  const int q = w.q0 + threadIdx.x;
  if (q >= w.x_len) return;
  const size_t qi = (size_t)w.x_start + q;
  float ox, oy, oz;
  icp_apply(R + (size_t)w.pad0 * 9, T + (size_t)w.pad0 * 3, X[qi * 3 + 0], X[qi * 3 + 1], X[qi * 3 + 2], ox, oy, oz);
  Xt[qi * 3 + 0] = ox; Xt[qi * 3 + 1] = oy; Xt[qi * 3 + 2] = oz;
}

int launch_icp(hipStream_t stream, const float* X, const int32_t* x_seg, const float* Y, const int32_t* y_seg, int K, long NX, long NY,
               const float* init_R, const float* init_T, int max_iterations, float relative_rmse_thr, float gate, float* R, float* T,
               float* rmse, int32_t* iterations, uint8_t* converged, float* Xt, NnWork* items, void* partials, void* ranges, double* prev,
               int32_t* done) {
  const int max_items = (int)nn_max_items(NX, K);
  hipLaunchKernelGGL(icp_setup_kernel, dim3(1), dim3(ICP_TILE), 0, stream, x_seg, y_seg, K, NX, NY, init_R, init_T, items, (IcpRange*)ranges,
                     max_items, R, T, rmse, iterations, converged, prev, done);
  RAP_LAUNCH_CHECK();
  for (int it = 0; it < max_iterations; ++it) {
    hipLaunchKernelGGL(icp_query_kernel, dim3(max_items), dim3(ICP_TILE), 0, stream, X, Y, items, R, T, done, gate, (IcpPartial*)partials);
    RAP_LAUNCH_CHECK();
    hipLaunchKernelGGL(icp_finish_kernel, dim3(K), dim3(64), 0, stream, (const IcpPartial*)partials, (const IcpRange*)ranges, it,
                       (double)relative_rmse_thr, R, T, rmse, iterations, converged, prev, done);
    RAP_LAUNCH_CHECK();
  }
  if (Xt) {
    hipLaunchKernelGGL(icp_apply_kernel, dim3(max_items), dim3(ICP_TILE), 0, stream, X, items, R, T, Xt);
    RAP_LAUNCH_CHECK();
  }
  return RAP_OK;
}

// the pieces of launch_icp that a second search path (nn_grid.hip) enqueues around its own query kernel: a kernel is launched from the
// file that defines it
int launch_icp_setup(hipStream_t stream, const int32_t* x_seg, const int32_t* y_seg, int K, long NX, long NY, const float* init_R,
                     const float* init_T, NnWork* items, void* ranges, float* R, float* T, float* rmse, int32_t* iterations,
                     uint8_t* converged, double* prev, int32_t* done) {
  hipLaunchKernelGGL(icp_setup_kernel, dim3(1), dim3(ICP_TILE), 0, stream, x_seg, y_seg, K, NX, NY, init_R, init_T, items, (IcpRange*)ranges,
                     (int)nn_max_items(NX, K), R, T, rmse, iterations, converged, prev, done);
  RAP_LAUNCH_CHECK();
  return RAP_OK;
}
int launch_icp_finish(hipStream_t stream, const void* partials, const void* ranges, int K, int it, float relative_rmse_thr, float* R, float* T,
                      float* rmse, int32_t* iterations, uint8_t* converged, double* prev, int32_t* done) {
  hipLaunchKernelGGL(icp_finish_kernel, dim3(K), dim3(64), 0, stream, (const IcpPartial*)partials, (const IcpRange*)ranges, it,
                     (double)relative_rmse_thr, R, T, rmse, iterations, converged, prev, done);
  RAP_LAUNCH_CHECK();
  return RAP_OK;
}
int launch_icp_apply(hipStream_t stream, const float* X, const NnWork* items, int max_items, const float* R, const float* T, float* Xt) {
  hipLaunchKernelGGL(icp_apply_kernel, dim3(max_items), dim3(ICP_TILE), 0, stream, X, items, R, T, Xt);
  RAP_LAUNCH_CHECK();
  return RAP_OK;
}
