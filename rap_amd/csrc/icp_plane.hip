// Batched point-to-plane ICP on the device: icp.hip's structure (one set-up, then a query and a finish launch per iteration, all
// enqueued up front; blocks and waves of a problem whose done flag is set return at once) with a second estimator.  Every iteration
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
//   icp_plane_query_kernel       icp_query_kernel's search, epilogue icp_plane_moments (icp.h): 28 doubles and a count per item
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
  const NnWork w = items[blockIdx.x];
  if (w.x_len <= 0) return;
  const int prob = w.pad0;
  if (done[prob]) return;
  const int q = w.q0 + threadIdx.x;
  const bool active = q < w.x_len;
  const size_t qi = (size_t)w.x_start + (active ? q : w.x_len - 1);
  float qx, qy, qz;
  icp_apply(R + (size_t)prob * 9, T + (size_t)prob * 3, X[qi * 3 + 0], X[qi * 3 + 1], X[qi * 3 + 2], qx, qy, qz);
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
      if (d2 < best) { best = d2; besti = k0 + j; }      // strict <: the first minimum wins, as icp_query_kernel
    }
  }
  icp_plane_moments(active, besti, best, gate, qx, qy, qz, Y, Yn, w.y_start, red_m, red_n, partials + blockIdx.x);
}

__global__ __launch_bounds__(64) void icp_plane_finish_kernel(const IcpPlanePartial* __restrict__ partials, const IcpRange* __restrict__ ranges,
                                                              int it, double rel_thr, double* __restrict__ state, float* __restrict__ R_out,
                                                              float* __restrict__ T_out, float* __restrict__ rmse_out,
                                                              int32_t* __restrict__ iterations, uint8_t* __restrict__ converged,
                                                              double* __restrict__ prev, int32_t* __restrict__ done) {
  const int k = blockIdx.x;
  if (done[k]) return;
  const IcpRange r = ranges[k];
  double m[ICP_PLANE_NMOM];
#pragma unroll
  for (int i = 0; i < ICP_PLANE_NMOM; ++i) m[i] = 0.0;
  long long n = 0;
  for (int i = threadIdx.x; i < r.count; i += 64) {
    const IcpPlanePartial* p = partials + r.first + i;
#pragma unroll
    for (int j = 0; j < ICP_PLANE_NMOM; ++j) m[j] += p->m[j];
    n += p->count;
  }
#pragma unroll
  for (int i = 0; i < ICP_PLANE_NMOM; ++i) m[i] = wave_sum_d(m[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
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
  const double pv = prev[k];
  const double rel = pv < 0.0 ? 1.0 : (pv - rmse) / pv;
  const bool stop = pv == 0.0 || rel <= rel_thr;
  rmse_out[k] = (float)rmse;
  iterations[k] = it + 1;
  if (stop) { converged[k] = 1; done[k] = 1; }
  prev[k] = rmse;
}

int launch_icp_plane_state(hipStream_t stream, const float* R, const float* T, int K, double* state) {
  hipLaunchKernelGGL(icp_plane_state_kernel, dim3((K + 255) / 256), dim3(256), 0, stream, R, T, K, state);
  RAP_LAUNCH_CHECK();
  return RAP_OK;
}
int launch_icp_plane_finish(hipStream_t stream, const void* partials, const void* ranges, int K, int it, float relative_rmse_thr, double* state,
                            float* R, float* T, float* rmse, int32_t* iterations, uint8_t* converged, double* prev, int32_t* done) {
  hipLaunchKernelGGL(icp_plane_finish_kernel, dim3(K), dim3(64), 0, stream, (const IcpPlanePartial*)partials, (const IcpRange*)ranges, it,
                     (double)relative_rmse_thr, state, R, T, rmse, iterations, converged, prev, done);
  RAP_LAUNCH_CHECK();
  return RAP_OK;
}

int launch_icp_plane(hipStream_t stream, const float* X, const int32_t* x_seg, const float* Y, const int32_t* y_seg, const float* Y_normals,
                     int K, long NX, long NY, const float* init_R, const float* init_T, int max_iterations, float relative_rmse_thr, float gate,
                     float* R, float* T, float* rmse, int32_t* iterations, uint8_t* converged, float* Xt, NnWork* items, void* partials,
                     void* ranges, double* prev, int32_t* done, double* state) {
  const int max_items = (int)nn_max_items(NX, K);
  int rc = launch_icp_setup(stream, x_seg, y_seg, K, NX, NY, init_R, init_T, items, ranges, R, T, rmse, iterations, converged, prev, done);
  if (rc) return rc;
  if ((rc = launch_icp_plane_state(stream, R, T, K, state))) return rc;
  for (int it = 0; it < max_iterations; ++it) {
    hipLaunchKernelGGL(icp_plane_query_kernel, dim3(max_items), dim3(ICP_TILE), 0, stream, X, Y, Y_normals, (const NnWork*)items,
                       (const float*)R, (const float*)T, (const int32_t*)done, gate, (IcpPlanePartial*)partials);
    RAP_LAUNCH_CHECK();
    if ((rc = launch_icp_plane_finish(stream, partials, ranges, K, it, relative_rmse_thr, state, R, T, rmse, iterations, converged, prev, done)))
      return rc;
  }
  if (Xt) return launch_icp_apply(stream, X, items, max_items, R, T, Xt);
  return RAP_OK;
}
