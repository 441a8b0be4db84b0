// The robust losses of the point-to-plane estimators (rap_icp_plane_robust, rap_icp_plane_grid_robust, rap_scene_refine_robust of
// include/rapflow.h): the weight w and the cost rho of one residual r at scale k, fp64.  Shared by the device epilogue
// (icp_plane_moments, icp.h) and a host unit test (tests/host/robust_host.cpp compiles this header with g++, so both run the same
// statements).  Plain C++; the only HIP-specific token is the qualifier.
//
//   none     w = 1                                  rho = r^2 / 2
//   huber    w = 1 (|r| <= k), k / |r|              rho = r^2 / 2 (|r| <= k), k (|r| - k / 2)
//   cauchy   w = 1 / (1 + (r/k)^2)                  rho = (k^2 / 2) log1p((r/k)^2)
//   tukey    w = (1 - (r/k)^2)^2 (|r| <= k), 0      rho = (k^2 / 6) (1 - (1 - (r/k)^2)^3) (|r| <= k), k^2 / 6
//
// w = rho'(r) / r: iteratively reweighted least squares (Holland and Welsch 1977).  All three are continuous in r, so a residual at
// |r| = k takes the same value from either branch up to rounding.
#pragma once
#include <math.h>

#ifndef RAP_HD
#if defined(__HIPCC__)
#define RAP_HD __host__ __device__
#else
#define RAP_HD
#endif
#endif

#ifndef RAP_LOSS_NONE
#define RAP_LOSS_NONE 0
#define RAP_LOSS_HUBER 1
#define RAP_LOSS_CAUCHY 2
#define RAP_LOSS_TUKEY 3
#endif

template <int LOSS>
RAP_HD inline void rap_robust(double r, double k, double& w, double& rho) {
  if (LOSS == RAP_LOSS_HUBER) {
    const double a = fabs(r);
    if (a <= k) { w = 1.0; rho = 0.5 * r * r; }
    else { w = k / a; rho = k * (a - 0.5 * k); }
  } else if (LOSS == RAP_LOSS_CAUCHY) {
    const double u = r / k, u2 = u * u;
    w = 1.0 / (1.0 + u2);
    rho = 0.5 * k * k * log1p(u2);
  } else if (LOSS == RAP_LOSS_TUKEY) {
    if (fabs(r) <= k) {
      const double u = r / k, t = 1.0 - u * u;
      w = t * t;
      rho = k * k / 6.0 * (1.0 - t * t * t);
    } else {
      w = 0.0;
      rho = k * k / 6.0;
    }
  } else {
    w = 1.0;
    rho = 0.5 * r * r;
  }
}

// the same with the loss chosen at run time (host code and tests); an unknown code gives the plain loss
RAP_HD inline void rap_robust_any(int loss, double r, double k, double& w, double& rho) {
  if (loss == RAP_LOSS_HUBER) rap_robust<RAP_LOSS_HUBER>(r, k, w, rho);
  else if (loss == RAP_LOSS_CAUCHY) rap_robust<RAP_LOSS_CAUCHY>(r, k, w, rho);
  else if (loss == RAP_LOSS_TUKEY) rap_robust<RAP_LOSS_TUKEY>(r, k, w, rho);
  else rap_robust<RAP_LOSS_NONE>(r, k, w, rho);
}
