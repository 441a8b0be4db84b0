// Host build of the robust losses of rap_amd/csrc/robust_loss.h (the statements the point-to-plane epilogue runs on the device), for
// tests/test_robust_host.py: g++ -O2 -shared -fPIC.
#include "../../rap_amd/csrc/robust_loss.h"

extern "C" {

// w[i], rho[i] of r[i] under loss (a RAP_LOSS_* code) at scale k, through the compile-time instantiation the kernels use
void robust_eval(int loss, const double* r, int n, double k, double* w, double* rho) {
  for (int i = 0; i < n; ++i) rap_robust_any(loss, r[i], k, w[i], rho[i]);
}

int robust_code(int which) {
  const int codes[4] = {RAP_LOSS_NONE, RAP_LOSS_HUBER, RAP_LOSS_CAUCHY, RAP_LOSS_TUKEY};
  return which >= 0 && which < 4 ? codes[which] : -1;
}
}
