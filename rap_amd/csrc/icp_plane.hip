// Batched point-to-plane ICP on the device: the second estimator of icp.hip's driver (launch_icp with Y_normals: one set-up, then a query
// and a finish launch per iteration, all enqueued up front; blocks and waves of a problem whose done flag is set return at once).  This
// file holds its kernels and the three launches the driver makes for it.  Every iteration
// linearises the motion about the CURRENT pose: with p_i = x_i R + T (fp32, what the search sees), y its nearest neighbour and n that
// neighbour's normal,
//     r_i = (p_i - y) . n,   J_i = [p_i x n, n],   A = sum J J^T,  b = sum J r,   (omega, tau) = -A^+ b,
//     dR = exp([omega]x),   R <- R dR^T,   T <- T dR^T + tau          (row vectors: p <- p dR^T + tau)
// over the gated pairs whose normal is finite and not zero.  A^+ drops eigenvalues <= 1e-12 lambda_max (fp64 6 x 6 cyclic Jacobi,
// kabsch.h): on a planar target the in-plane motion is unobservable and the step along it is zero instead of noise / 0.
//
//   icp_setup_kernel (icp.hip)   items, item ranges, R, T = init or identity, flags
//   icp_plane_state_kernel       the fp64 pose of every problem (12 doubles) = its fp32 start; the outputs R, T are always the fp32
//                                rounding of this state, so the pose does not lose a rounding per iteration
//   icp_plane_query_kernel       the tiled search (nn_tile.h) of the moved query, epilogue icp_plane_moments (icp.h): 28 doubles and a
//                                count per item
//   icp_plane_finish_kernel      one wave per problem: partials added lane-strided in item order; lane 0: rmse of the pose that ENTERED
//                                the iteration (so the reported rmse is one update behind the returned R, T), the 6 x 6 solve, the update,
//                                the stopping rule
//   icp_apply_kernel (icp.hip)   optional Xt
// No host read, no allocation, no floating-point atomics; a problem's bits depend on its own segments only.
#include "icp.h"
#include "kabsch.h"

#define ICP_PLANE_RCOND 1e-12

size_t icp_plane_partial_bytes() { return sizeof(IcpPlanePartial); }

__global__ __launch_bounds__(256) void icp_plane_state_kernel(const float* __restrict__ R, const float* __restrict__ T, int K,
                                                              double* __restrict__ state) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= K) return;
#pragma unroll
  for (int i = 0; i < 9; ++i) state[(size_t)k * 12 + i] = (double)R[(size_t)k * 9 + i];
#pragma unroll
  for (int i = 0; i < 3; ++i) state[(size_t)k * 12 + 9 + i] = (double)T[(size_t)k * 3 + i];
}

__global__ __launch_bounds__(ICP_TILE) void icp_plane_query_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                                   const float* __restrict__ Yn, const NnWork* __restrict__ items,
                                                                   const float* __restrict__ R, const float* __restrict__ T,
                                                                   const int32_t* __restrict__ done, float gate,
                                                                   IcpPlanePartial* __restrict__ partials) {
  __shared__ float4 tile[ICP_TILE];
  __shared__ double red_m[ICP_TILE / 64][ICP_PLANE_NMOM];
  __shared__ int red_n[ICP_TILE / 64];
  ICP_QUERY_BEGIN(X, items, R, T, done);
  NN_TILE_ARGMIN(tile, w.y_len, px, py, pz, [&](int k, float4& c) { nn_row(Y, (size_t)w.y_start + k, c); }, best, besti);
  icp_plane_moments(active, besti, best, gate, px, py, pz, Y, Yn, w.y_start, red_m, red_n, partials + blockIdx.x);
}

__global__ __launch_bounds__(64) void icp_plane_finish_kernel(const IcpPlanePartial* __restrict__ partials, const IcpRange* __restrict__ ranges,
                                                              int it, double rel_thr, double* __restrict__ state, float* __restrict__ R_out,
                                                              float* __restrict__ T_out, float* __restrict__ rmse_out,
                                                              int32_t* __restrict__ iterations, uint8_t* __restrict__ converged,
                                                              double* __restrict__ prev, int32_t* __restrict__ done) {
  const int k = blockIdx.x;
  if (done[k]) return;
  const IcpRange r = ranges[k];
  ICP_SUM_PARTIALS(ICP_PLANE_NMOM, IcpPlanePartial, partials, r, m, n);
  if (threadIdx.x != 0) return;
  if (n == 0) {                                      // no gated pair with a usable normal: stop with the R, T it had
    rmse_out[k] = __builtin_inff();
    done[k] = 1;
    return;
  }
  const double rmse = sqrt(fmax(m[27] / (double)n, 0.0));
  double A[6][6], b[6], xi[6];
  int at = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = i; j < 6; ++j) { A[i][j] = m[at]; A[j][i] = m[at]; ++at; }
    b[i] = m[21 + i];
  }
  rap_pinv6_step(A, b, ICP_PLANE_RCOND, xi);
  double dR[3][3], S[12];
  rap_rodrigues(xi, dR);
  double* st = state + (size_t)k * 12;
  // rows of [R; T] times dR^T: out[i][j] = sum_l in[i][l] dR[j][l]
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const double a0 = st[3 * i + 0], a1 = st[3 * i + 1], a2 = st[3 * i + 2];
#pragma unroll
    for (int j = 0; j < 3; ++j) S[3 * i + j] = a0 * dR[j][0] + a1 * dR[j][1] + a2 * dR[j][2] + (i == 3 ? xi[3 + j] : 0.0);
  }
#pragma unroll
  for (int i = 0; i < 12; ++i) st[i] = S[i];
#pragma unroll
  for (int i = 0; i < 9; ++i) R_out[(size_t)k * 9 + i] = (float)S[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) T_out[(size_t)k * 3 + i] = (float)S[9 + i];
  icp_finish_end(k, it, rmse, rel_thr, rmse_out, iterations, converged, prev, done);
}

int launch_icp_plane_state(hipStream_t stream, const IcpCall& c) {
  hipLaunchKernelGGL(icp_plane_state_kernel, dim3((c.K + 255) / 256), dim3(256), 0, stream, (const float*)c.R, (const float*)c.T, c.K, c.state);
  RAP_LAUNCH_CHECK();
  return RAP_OK;
}
int launch_icp_plane_query(hipStream_t stream, const IcpCall& c) {
  hipLaunchKernelGGL(icp_plane_query_kernel, dim3((unsigned)nn_max_items(c.NX, c.K)), dim3(ICP_TILE), 0, stream, c.X, c.Y, c.Y_normals,
                     (const NnWork*)c.items, (const float*)c.R, (const float*)c.T, (const int32_t*)c.done, c.gate, (IcpPlanePartial*)c.partials);
  RAP_LAUNCH_CHECK();
  return RAP_OK;
}
int launch_icp_plane_finish(hipStream_t stream, const IcpCall& c, int it) {
  hipLaunchKernelGGL(icp_plane_finish_kernel, dim3(c.K), dim3(64), 0, stream, (const IcpPlanePartial*)c.partials, (const IcpRange*)c.ranges, it,
                     (double)c.relative_rmse_thr, c.state, c.R, c.T, c.rmse, c.iterations, c.converged, c.prev, c.done);
  RAP_LAUNCH_CHECK();
  return RAP_OK;
}
