// Batched scan-pair metrics of the evaluator (reference eval/evaluator.py:124-248): for all B samples of a packed batch with P = 2 the
// correspondence RMSE, the correspondence ratio and the Redwood "transform error" -- compute_correspondence_rmse (eval/metrics.py:386-469)
// and compute_approximate_transform_error (:487-508) as the evaluator calls them per pair in a Python loop with host read-backs.
// Here: three launches for the whole batch, no host read, nothing of size N x M and no per-point array in HBM.
//
//   pair_worklist_kernel   points_per_part / cu -> items of 256 source points of one pair + the item range of every pair
//   pair_query_kernel      the tiled search (nn_tile.h: target tile through LDS, one ds_read_b128 broadcast per candidate, strict < so the
//                          first arg-min wins) on clouds scaled to metres when they are LOADED, with the epilogue fused: the lane that
//                          found nn(i) forms |src_i - tgt_nn(i)|^2 of the compared clouds and the block reduces {sum (double), count}
//                          into one partial per item
//   pair_finish_kernel     one wave per pair: item partials added in a fixed order, the 3 x 3 pose algebra, the four outputs
//
// Two rules:
//   * deterministic -- no floating-point atomics, the partials of a pair are combined lane-strided in item order by one wave;
//   * round before you subtract -- the reference scales the clouds in fp32 and THEN measures distances; x * s - y would be contracted
//     into one fma, a different number.  Every scaled coordinate is formed by mul_rn_nofuse, so d^2 is the direct-difference fp32 value
//     of the rounded coordinates, exactly what nn_query_kernel computes on a cloud torch scaled beforehand.
#include "nn_tile.h"

#define PM_TILE NN_TILE

struct PairPartial { double sum; long long count; };
struct PairRange { int first, count, n_source, n_target; };

__global__ void pair_worklist_kernel(const int64_t* __restrict__ ppp, const int32_t* __restrict__ cu, int B, long TP,
                                     NnWork* __restrict__ items, PairRange* __restrict__ ranges, int max_items) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int n = 0;
  for (int b = 0; b < B; ++b) {
    // clamped so that an inconsistent table cannot make a later kernel index outside [0, TP)
    long start = cu[b];
    start = start < 0 ? 0 : start > TP ? TP : start;
    long n0 = ppp[(size_t)b * 2], n1 = ppp[(size_t)b * 2 + 1];
    n0 = n0 < 0 ? 0 : n0 > TP - start ? TP - start : n0;
    n1 = n1 < 0 ? 0 : n1 > TP - start - n0 ? TP - start - n0 : n1;
    PairRange r = {n, 0, (int)n0, (int)n1};
    if (n0 > 0 && n1 > 0) {
      n = nn_emit_items(items, n, max_items, start, n0, start + n0, n1, b, 0);
      r.count = n - r.first;
    }
    ranges[b] = r;
  }
  nn_zero_items(items, n, max_items);
}

__device__ __forceinline__ void pm_load_scaled(const float* __restrict__ P, size_t i, float s, float& x, float& y, float& z) {
  x = mul_rn_nofuse(P[i * 3 + 0], s); y = mul_rn_nofuse(P[i * 3 + 1], s); z = mul_rn_nofuse(P[i * 3 + 2], s);
}
// (p s) @ R^T + t s (evaluator.py:176-184) in double from the fp32 inputs: once per correspondence, so the compared clouds carry no
// rounding of their own (at 50 m an fp32 coordinate is good to 4e-6 m, which a 1 cm error would see as 1e-3 relative per point)
__device__ __forceinline__ void pm_pose_apply(const float* __restrict__ R, const float* __restrict__ t, double s, const float* __restrict__ p,
                                              double* o) {
  const double x = p[0] * s, y = p[1] * s, z = p[2] * s;
#pragma unroll
  for (int r = 0; r < 3; ++r) o[r] = ((double)R[r * 3] * x + (double)R[r * 3 + 1] * y + (double)R[r * 3 + 2] * z) + t[r] * s;
}

// TRANSFORMED: compared clouds = (cloud s) @ R_pred^T + t_pred s per part (cloud = the inputs), formed in double; else the two parts of
// cloud s (cloud = the prediction) in the arithmetic of correspondence_finish_kernel on a cloud scaled beforehand in fp32 -- rounded
// products, fp32 differences and squares -- so that the batched and the single-pair path agree per point.
// One partial {sum of squared errors over the item's correspondences, their number} per item.
template <bool TRANSFORMED>
__global__ __launch_bounds__(PM_TILE) void pair_query_kernel(const float* __restrict__ gt, const float* __restrict__ cloud,
                                                             const float* __restrict__ scales, const float* __restrict__ R_pred,
                                                             const float* __restrict__ t_pred, const NnWork* __restrict__ items,
                                                             float thr, PairPartial* __restrict__ partials) {
  __shared__ float4 tile[PM_TILE];
  __shared__ double red_s[PM_TILE / 64];
  __shared__ int red_n[PM_TILE / 64];
  const NnWork w = items[blockIdx.x];
  if (w.x_len <= 0) return;
  const int b = w.pad0;
  const float s = scales[b];
  const int q = w.q0 + threadIdx.x;
  const bool active = q < w.x_len;
  const size_t qi = (size_t)w.x_start + (active ? q : w.x_len - 1);
  float qx, qy, qz;
  pm_load_scaled(gt, qi, s, qx, qy, qz);
  // the candidates are stored to LDS already in metres
  NN_TILE_ARGMIN(tile, w.y_len, qx, qy, qz, [&](int k, float4& c) { pm_load_scaled(gt, (size_t)w.y_start + k, s, c.x, c.y, c.z); }, best, besti);
  double se = 0.0;
  int n = 0;
  if (active && besti >= 0 && sqrtf(best) <= thr) {        // the form correspondence_finish_kernel uses
    const size_t ti = (size_t)w.y_start + besti;
    if (TRANSFORMED) {
      const size_t p0 = (size_t)b * 2, p1 = p0 + 1;
      double a[3], c[3];
      pm_pose_apply(R_pred + p0 * 9, t_pred + p0 * 3, (double)s, cloud + qi * 3, a);
      pm_pose_apply(R_pred + p1 * 9, t_pred + p1 * 3, (double)s, cloud + ti * 3, c);
      const double dx = a[0] - c[0], dy = a[1] - c[1], dz = a[2] - c[2];
      se = dx * dx + dy * dy + dz * dz;
    } else {
      float sx, sy, sz, tx, ty, tz;
      pm_load_scaled(cloud, qi, s, sx, sy, sz);
      pm_load_scaled(cloud, ti, s, tx, ty, tz);
      const float dx = sx - tx, dy = sy - ty, dz = sz - tz;
      se = (double)(dx * dx + dy * dy + dz * dz);
    }
    n = 1;
  }
  se = wave_sum_d(se);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if ((threadIdx.x & 63) == 0) { red_s[threadIdx.x >> 6] = se; red_n[threadIdx.x >> 6] = n; }
  __syncthreads();
  if (threadIdx.x == 0) {
    PairPartial p;
    p.sum = (red_s[0] + red_s[1]) + (red_s[2] + red_s[3]);
    p.count = (long long)(red_n[0] + red_n[1] + red_n[2] + red_n[3]);
    partials[blockIdx.x] = p;
  }
}

// ---- 3 x 3 pose algebra of one pair, in double from the fp32 poses (once per pair; the closest a device can get to the fp64 record) ----
__device__ __forceinline__ void pm_rel(const float* __restrict__ R, const float* __restrict__ t, double s, double* Rrel, double* trel) {
  // R_rel = R_tgt R_src^T, t_rel = s t_tgt - R_rel (s t_src)            (evaluator.py:159-168, 192-195); part 0 = source, part 1 = target
  const float* Rs = R; const float* Rt = R + 9;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c)
      Rrel[r * 3 + c] = (double)Rt[r * 3] * Rs[c * 3] + (double)Rt[r * 3 + 1] * Rs[c * 3 + 1] + (double)Rt[r * 3 + 2] * Rs[c * 3 + 2];
  const double ts[3] = {t[0] * s, t[1] * s, t[2] * s};
  for (int r = 0; r < 3; ++r)
    trel[r] = t[3 + r] * s - (Rrel[r * 3] * ts[0] + Rrel[r * 3 + 1] * ts[1] + Rrel[r * 3 + 2] * ts[2]);
}
// |q_xyz|^2 of the unit quaternion of M (Shepperd's choice of the largest of m00, m11, m22, trace -- no cancellation at small angles,
// where (3 - tr M) / 4 in fp32 would lose the value)
__device__ __forceinline__ double pm_quat_vec_sq(const double* M) {
  const double tr = M[0] + M[4] + M[8];
  double q[4];
  int i = 3; double big = tr;
  for (int d = 0; d < 3; ++d)
    if (M[d * 4] > big) { big = M[d * 4]; i = d; }
  if (i == 3) {
    q[0] = M[7] - M[5]; q[1] = M[2] - M[6]; q[2] = M[3] - M[1]; q[3] = 1.0 + tr;
  } else {
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    q[i] = 1.0 - tr + 2.0 * M[i * 4];
    q[j] = M[j * 3 + i] + M[i * 3 + j];
    q[k] = M[k * 3 + i] + M[i * 3 + k];
    q[3] = M[k * 3 + j] - M[j * 3 + k];
  }
  const double v = q[0] * q[0] + q[1] * q[1] + q[2] * q[2];
  return v / (v + q[3] * q[3]);
}

// out4[b] = {rmse, ratio, transform_error_rmse, count}; inf / 0 / inf / 0 when a part is empty (evaluator.py:233-236), inf / 0 with a finite
// transform error when no source point has a target within the threshold (metrics.py:454-455)
__global__ __launch_bounds__(64) void pair_finish_kernel(const PairPartial* __restrict__ partials, const PairRange* __restrict__ ranges,
                                                         const float* __restrict__ scales, const float* __restrict__ R_gt,
                                                         const float* __restrict__ t_gt, const float* __restrict__ R_pred,
                                                         const float* __restrict__ t_pred, float* __restrict__ out4) {
  const int b = blockIdx.x;
  const PairRange r = ranges[b];
  double s = 0.0;
  long long n = 0;
  for (int i = threadIdx.x; i < r.count; i += 64) { const PairPartial p = partials[r.first + i]; s += p.sum; n += p.count; }
  s = wave_sum_d(s);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if (threadIdx.x != 0) return;
  const float inf = __builtin_inff();
  float* o = out4 + (size_t)b * 4;
  const bool both = r.n_source > 0 && r.n_target > 0;
  o[0] = n > 0 ? (float)sqrt(s / (double)n) : inf;
  o[1] = n > 0 ? (float)((double)n / (double)r.n_source) : 0.f;
  o[3] = (float)n;
  float te = inf;
  if (both && R_pred) {
    const double sc = (double)scales[b];
    double Rg[9], tg[3], Re[9], tE[3], dR[9];
    pm_rel(R_gt + (size_t)b * 18, t_gt + (size_t)b * 6, sc, Rg, tg);
    pm_rel(R_pred + (size_t)b * 18, t_pred + (size_t)b * 6, sc, Re, tE);
    for (int rr = 0; rr < 3; ++rr)
      for (int c = 0; c < 3; ++c) dR[rr * 3 + c] = Rg[rr] * Re[c] + Rg[3 + rr] * Re[3 + c] + Rg[6 + rr] * Re[6 + c];      // R_rel_gt^T R_rel_est
    const double d0 = tE[0] - tg[0], d1 = tE[1] - tg[1], d2 = tE[2] - tg[2];
    te = (float)sqrt(d0 * d0 + d1 * d1 + d2 * d2 + pm_quat_vec_sq(dR));        // identity covariance: er^T er, then the evaluator's sqrt
  }
  o[2] = te;
}

int launch_pair_metrics(hipStream_t stream, const float* gt, const float* cloud, const int64_t* ppp, const int32_t* cu_batch,
                        const float* scales, const float* R_gt, const float* t_gt, const float* R_pred, const float* t_pred, int B, long TP,
                        float thr, float* out4, NnWork* items, void* partials, void* ranges) {
  if (B <= 0 || TP <= 0) return RAP_OK;
  const int max_items = (int)nn_max_items(TP, B);
  hipLaunchKernelGGL(pair_worklist_kernel, dim3(1), dim3(64), 0, stream, ppp, cu_batch, B, TP, items, (PairRange*)ranges, max_items);
  RAP_LAUNCH_CHECK();
  if (R_pred)
    hipLaunchKernelGGL(pair_query_kernel<true>, dim3(max_items), dim3(PM_TILE), 0, stream, gt, cloud, scales, R_pred, t_pred, items, thr,
                       (PairPartial*)partials);
  else
    hipLaunchKernelGGL(pair_query_kernel<false>, dim3(max_items), dim3(PM_TILE), 0, stream, gt, cloud, scales, R_pred, t_pred, items, thr,
                       (PairPartial*)partials);
  RAP_LAUNCH_CHECK();
  hipLaunchKernelGGL(pair_finish_kernel, dim3(B), dim3(64), 0, stream, (const PairPartial*)partials, (const PairRange*)ranges, scales, R_gt,
                     t_gt, R_pred, t_pred, out4);
  RAP_LAUNCH_CHECK();
  return RAP_OK;
}

// ---------------------------------------------------------------------------------------------
// compute_transform_errors_direct (reference eval/metrics.py:305-383): no anchor frame, every non-empty part counts.
//   delta_R = R_gt^T R_pred, delta_t = (t_pred - t_gt) scale;  RE = deg(acos(clamp((tr delta_R - 1) / 2, -1, 1))),  TE = |delta_t|;
//   means over the non-empty parts (0 / 0 = NaN for a sample without one, as the reference's division).
// One block per sample, one lane per part, the per-sample sums in part order by one lane, in double.  matched (B,P) int64 or null re-orders the
// PREDICTED poses (:341-344).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void transform_errors_direct_kernel(const float* __restrict__ R_gt, const float* __restrict__ t_gt,
                                                                     const float* __restrict__ R_pred, const float* __restrict__ t_pred,
                                                                     const int64_t* __restrict__ ppp, const int64_t* __restrict__ matched,
                                                                     const float* __restrict__ scale, int P, float* __restrict__ rot_pp,
                                                                     float* __restrict__ trans_pp, float* __restrict__ rot_mean,
                                                                     float* __restrict__ trans_mean) {
  const int b = blockIdx.x;
  const size_t row = (size_t)b * P;
  const double s = scale ? (double)scale[b] : 1.0;
  for (int p = threadIdx.x; p < P; p += 64) {
    float re = 0.f, te = 0.f;
    if (ppp[row + p] != 0) {
      long q = matched ? (long)matched[row + p] : (long)p;
      q = q < 0 ? 0 : q >= P ? P - 1 : q;              // an out-of-range match cannot index outside the sample's rows
      const float* Rg = R_gt + (row + p) * 9; const float* Rp = R_pred + (row + (size_t)q) * 9;
      const float* tg = t_gt + (row + p) * 3; const float* tp = t_pred + (row + (size_t)q) * 3;
      double tr = 0.0;
      for (int k = 0; k < 9; ++k) tr += (double)Rg[k] * (double)Rp[k];          // tr(R_gt^T R_pred) = sum of the element products
      double c = 0.5 * (tr - 1.0);
      c = c < -1.0 ? -1.0 : c > 1.0 ? 1.0 : c;
      re = (float)(acos(c) * 57.29577951308232);
      const double d0 = ((double)tp[0] - tg[0]) * s, d1 = ((double)tp[1] - tg[1]) * s, d2 = ((double)tp[2] - tg[2]) * s;
      te = (float)sqrt(d0 * d0 + d1 * d1 + d2 * d2);
    }
    rot_pp[row + p] = re; trans_pp[row + p] = te;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    // the sums in double like everything above: an fp32 running sum over P parts loses up to P / 2 ulp of the mean (3.5 ulp seen at P = 64)
    double sr = 0.0, st = 0.0; int n = 0;
    for (int p = 0; p < P; ++p) {
      sr += (double)rot_pp[row + p]; st += (double)trans_pp[row + p];
      n += ppp[row + p] != 0 ? 1 : 0;
    }
    rot_mean[b] = (float)(sr / (double)n);          // 0 / 0 = NaN for a sample without a part, as the reference's division
    trans_mean[b] = (float)(st / (double)n);
  }
}

int launch_transform_errors_direct(hipStream_t stream, const float* R_gt, const float* t_gt, const float* R_pred, const float* t_pred,
                                   const int64_t* ppp, const int64_t* matched, const float* scale, int B, int P, float* rot_pp,
                                   float* trans_pp, float* rot_mean, float* trans_mean) {
  if (B <= 0 || P <= 0) return RAP_OK;
  hipLaunchKernelGGL(transform_errors_direct_kernel, dim3(B), dim3(64), 0, stream, R_gt, t_gt, R_pred, t_pred, ppp, matched, scale, P, rot_pp,
                     trans_pp, rot_mean, trans_mean);
  RAP_LAUNCH_CHECK();
  return RAP_OK;
}
