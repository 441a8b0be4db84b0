// Batched point-to-point ICP on the device: K independent problems, each aligning a segment of X to a segment of Y, with pytorch3d's
// iterative_closest_point semantics (the reference takes it from there: eval/metrics.py:79 and :261, one problem at a time with a KNN
// launch, an SVD launch and a host read of the convergence test per iteration).  Row-vector convention Xt = X R + T, det R = +1.
//
//   icp_setup_kernel    segment tables -> items of 256 queries of one problem + every problem's item range; the state of every problem
//                       (R, T = init or identity, no previous rmse, iterations 0, done = a segment is empty)
//   per iteration, enqueued max_iterations times up front:
//   icp_query_kernel    the tiled search (nn_tile.h) with the problem's current R, T applied to the query when it is LOADED (icp.h);
//                       epilogue: the block reduces the gated count and the raw moments (double) of the ORIGINAL x and its neighbour y
//                       into one partial per item
//   icp_finish_kernel   one wave per problem: item partials added lane-strided in item order, the 3 x 3 Kabsch solve (kabsch.h), the rmse
//                       from the same centred moments, the stopping rule, the new state
//   icp_apply_kernel    optional: Xt = X R + T of every point of a problem
//
// The convergence decision stays on the device: blocks and waves of a problem whose done flag is set return at once, so the host never
// reads anything back and the whole call can be captured into a graph.  Nothing N x M and no per-point index or distance reaches HBM.
// Deterministic (no floating-point atomics) and batch-independent: a problem's arithmetic depends on its own segments only.
//
// launch_icp is the host driver of all four forms of the call: estimator (point, here; plane, icp_plane.hip) x search (tiled; the grid
// of nn_grid.hip).  They differ in one optional launch before the loop each and in which query and finish kernel an iteration runs.
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
      nn_segment(x_seg, k, NX, xs, xn);
      nn_segment(y_seg, k, NY, ys, yn);
      // a problem with an empty Y keeps its items: icp_apply_kernel moves its points by the initial transform.  One left out whole
      // (nn_emit_items_whole) reports as an empty one
      IcpRange r = {n, 0, xn, yn};
      r.count = nn_emit_items_whole(items, n, max_items, xs, xn, ys, yn, k);
      ranges[k] = r;
    }
    nn_zero_items(items, n, max_items);
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
  ICP_QUERY_BEGIN(X, items, R, T, done);
  NN_TILE_ARGMIN(tile, w.y_len, px, py, pz, [&](int k, float4& c) { nn_row(Y, (size_t)w.y_start + k, c); }, best, besti);
  icp_moments(active, besti, best, gate, x0, x1, x2, Y, w.y_start, red_m, red_n, partials + blockIdx.x);
}

__global__ __launch_bounds__(64) void icp_finish_kernel(const IcpPartial* __restrict__ partials, const IcpRange* __restrict__ ranges, int it,
                                                        double rel_thr, float* __restrict__ R_out, float* __restrict__ T_out,
                                                        float* __restrict__ rmse_out, int32_t* __restrict__ iterations,
                                                        uint8_t* __restrict__ converged, double* __restrict__ prev, int32_t* __restrict__ done) {
  const int k = blockIdx.x;
  if (done[k]) return;
  const IcpRange r = ranges[k];
  ICP_SUM_PARTIALS(ICP_NMOM, IcpPartial, partials, r, m, n);
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
  icp_finish_end(k, it, rmse, rel_thr, rmse_out, iterations, converged, prev, done);
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

int launch_icp(hipStream_t stream, const IcpCall& c) {
  const int max_items = (int)nn_max_items(c.NX, c.K);
  int rc = RAP_OK;
  hipLaunchKernelGGL(icp_setup_kernel, dim3(1), dim3(ICP_TILE), 0, stream, c.x_seg, c.y_seg, c.K, c.NX, c.NY, c.init_R, c.init_T, c.items,
                     (IcpRange*)c.ranges, max_items, c.R, c.T, c.rmse, c.iterations, c.converged, c.prev, c.done);
  RAP_LAUNCH_CHECK();
  if (c.Y_normals && (rc = launch_icp_plane_state(stream, c))) return rc;
  if (c.grid && (rc = launch_nn_grid_build(stream, c.Y, c.y_seg, c.K, c.NY, *c.grid))) return rc;
  for (int it = 0; it < c.max_iterations; ++it) {
    if (c.grid) {
      rc = launch_icp_grid_query(stream, c);
    } else if (c.Y_normals) {
      rc = launch_icp_plane_query(stream, c);
    } else {
      hipLaunchKernelGGL(icp_query_kernel, dim3(max_items), dim3(ICP_TILE), 0, stream, c.X, c.Y, (const NnWork*)c.items, (const float*)c.R,
                         (const float*)c.T, (const int32_t*)c.done, c.gate, (IcpPartial*)c.partials);
      RAP_LAUNCH_CHECK();
    }
    if (rc) return rc;
    if (c.Y_normals) {
      rc = launch_icp_plane_finish(stream, c, it);
    } else {
      hipLaunchKernelGGL(icp_finish_kernel, dim3(c.K), dim3(64), 0, stream, (const IcpPartial*)c.partials, (const IcpRange*)c.ranges, it,
                         (double)c.relative_rmse_thr, c.R, c.T, c.rmse, c.iterations, c.converged, c.prev, c.done);
      RAP_LAUNCH_CHECK();
    }
    if (rc) return rc;
  }
  if (c.Xt) {
    hipLaunchKernelGGL(icp_apply_kernel, dim3(max_items), dim3(ICP_TILE), 0, stream, c.X, (const NnWork*)c.items, (const float*)c.R,
                       (const float*)c.T, c.Xt);
    RAP_LAUNCH_CHECK();
  }
  return RAP_OK;
}
