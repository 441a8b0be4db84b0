// The finish kernel of point-to-plane ICP, included by icp_plane.hip once per partial type: FINISH_KERNEL = its name, FINISH_PARTIAL =
// IcpPlanePartial (rap_icp_plane) or IcpPlaneWPartial (the robust call, whose rmse is sqrt(sum 2 rho / n) and which also stops when every
// weight is zero).  A textual include and not a template: as a function called from two kernels the plain kernel gets another register
// allocation than it had (see ICP_SUM_PARTIALS, icp.h).
__global__ __launch_bounds__(64) void FINISH_KERNEL(const FINISH_PARTIAL* __restrict__ partials, const IcpRange* __restrict__ ranges,
                                                    int it, double rel_thr, double* __restrict__ state, float* __restrict__ R_out,
                                                    float* __restrict__ T_out, float* __restrict__ rmse_out,
                                                    int32_t* __restrict__ iterations, uint8_t* __restrict__ converged,
                                                    double* __restrict__ prev, int32_t* __restrict__ done) {
  const int k = blockIdx.x;
  if (done[k]) return;
  const IcpRange r = ranges[k];
  ICP_SUM_PARTIALS(FINISH_PARTIAL::NRED, FINISH_PARTIAL, partials, r, m, n);
  if (threadIdx.x != 0) return;
  // no gated pair with a usable normal (or, robust: none with a weight): stop with the R, T it had
  if (n == 0 || (FINISH_PARTIAL::NRED == ICP_PLANE_WMOM && m[FINISH_PARTIAL::NRED - 1] == 0.0)) {
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
