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
// The robust calls (rap_icp_plane_robust; IcpCall::robust) run icp_plane_query_robust_kernel<loss> and icp_plane_finish_robust_kernel in
// their place: the same statements on weighted sums (robust_loss.h, the epilogue in icp.h), a partial that also carries W = sum w, and
// icp_plane_weights_zero_kernel once before the loop where per-row weights are asked for.
// No host read, no allocation, no floating-point atomics; a problem's bits depend on its own segments only.
#include "icp.h"
#include "kabsch.h"

#define ICP_PLANE_RCOND 1e-12

size_t icp_plane_partial_bytes() { return sizeof(IcpPlanePartial); }
size_t icp_plane_robust_partial_bytes() { return sizeof(IcpPlaneWPartial); }

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
  icp_plane_moments<RAP_LOSS_NONE>(active, besti, best, gate, px, py, pz, Y, Yn, w.y_start, red_m, red_n, partials + blockIdx.x);
}

// the robust call's query: the same search, the weighted epilogue, the optional per-row weights
template <int LOSS>
__global__ __launch_bounds__(ICP_TILE) void icp_plane_query_robust_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                                          const float* __restrict__ Yn, const NnWork* __restrict__ items,
                                                                          const float* __restrict__ R, const float* __restrict__ T,
                                                                          const int32_t* __restrict__ done, float gate, double scale,
                                                                          float* __restrict__ weights, IcpPlaneWPartial* __restrict__ partials) {
  __shared__ float4 tile[ICP_TILE];
  __shared__ double red_m[ICP_TILE / 64][ICP_PLANE_WMOM];
  __shared__ int red_n[ICP_TILE / 64];
  ICP_QUERY_BEGIN(X, items, R, T, done);
  NN_TILE_ARGMIN(tile, w.y_len, px, py, pz, [&](int k, float4& c) { nn_row(Y, (size_t)w.y_start + k, c); }, best, besti);
  icp_plane_moments<LOSS>(active, besti, best, gate, px, py, pz, Y, Yn, w.y_start, red_m, red_n, partials + blockIdx.x, scale, weights, qi);
}

// weights = 0 on every row of every problem that has items (a problem that runs no iteration keeps that)
__global__ __launch_bounds__(ICP_TILE) void icp_plane_weights_zero_kernel(const NnWork* __restrict__ items, float* __restrict__ weights) {
  const NnWork w = items[blockIdx.x];
  const int q = w.q0 + threadIdx.x;
  if (q < w.x_len) weights[(size_t)w.x_start + q] = 0.f;
}

#define FINISH_KERNEL icp_plane_finish_kernel
#define FINISH_PARTIAL IcpPlanePartial
#include "icp_plane_finish.inc"
#undef FINISH_KERNEL
#undef FINISH_PARTIAL
#define FINISH_KERNEL icp_plane_finish_robust_kernel
#define FINISH_PARTIAL IcpPlaneWPartial
#include "icp_plane_finish.inc"
#undef FINISH_KERNEL
#undef FINISH_PARTIAL

int launch_icp_plane_state(hipStream_t stream, const IcpCall& c) {
  hipLaunchKernelGGL(icp_plane_state_kernel, dim3((c.K + 255) / 256), dim3(256), 0, stream, (const float*)c.R, (const float*)c.T, c.K, c.state);
  RAP_LAUNCH_CHECK();
  if (c.robust && c.weights) {
    hipLaunchKernelGGL(icp_plane_weights_zero_kernel, dim3((unsigned)nn_max_items(c.NX, c.K)), dim3(ICP_TILE), 0, stream,
                       (const NnWork*)c.items, c.weights);
    RAP_LAUNCH_CHECK();
  }
  return RAP_OK;
}
template <int LOSS>
static void icp_plane_query_robust(hipStream_t stream, const IcpCall& c) {
  hipLaunchKernelGGL(icp_plane_query_robust_kernel<LOSS>, dim3((unsigned)nn_max_items(c.NX, c.K)), dim3(ICP_TILE), 0, stream, c.X, c.Y,
                     c.Y_normals, (const NnWork*)c.items, (const float*)c.R, (const float*)c.T, (const int32_t*)c.done, c.gate,
                     (double)c.loss_scale, c.weights, (IcpPlaneWPartial*)c.partials);
}
int launch_icp_plane_query(hipStream_t stream, const IcpCall& c) {
  if (c.robust) {
    RAP_LOSS_DISPATCH(c.loss, icp_plane_query_robust, stream, c);
    RAP_LAUNCH_CHECK();
    return RAP_OK;
  }
  hipLaunchKernelGGL(icp_plane_query_kernel, dim3((unsigned)nn_max_items(c.NX, c.K)), dim3(ICP_TILE), 0, stream, c.X, c.Y, c.Y_normals,
                     (const NnWork*)c.items, (const float*)c.R, (const float*)c.T, (const int32_t*)c.done, c.gate, (IcpPlanePartial*)c.partials);
  RAP_LAUNCH_CHECK();
  return RAP_OK;
}
int launch_icp_plane_finish(hipStream_t stream, const IcpCall& c, int it) {
  if (c.robust) {
    hipLaunchKernelGGL(icp_plane_finish_robust_kernel, dim3(c.K), dim3(64), 0, stream, (const IcpPlaneWPartial*)c.partials,
                       (const IcpRange*)c.ranges, it, (double)c.relative_rmse_thr, c.state, c.R, c.T, c.rmse, c.iterations, c.converged, c.prev,
                       c.done);
    RAP_LAUNCH_CHECK();
    return RAP_OK;
  }
  hipLaunchKernelGGL(icp_plane_finish_kernel, dim3(c.K), dim3(64), 0, stream, (const IcpPlanePartial*)c.partials, (const IcpRange*)c.ranges, it,
                     (double)c.relative_rmse_thr, c.state, c.R, c.T, c.rmse, c.iterations, c.converged, c.prev, c.done);
  RAP_LAUNCH_CHECK();
  return RAP_OK;
}
