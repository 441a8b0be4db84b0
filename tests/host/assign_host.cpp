// Host build of rap_amd/csrc/assign.h (the lines the device assignment kernel compiles) for CPU unit tests.
#include "../../rap_amd/csrc/assign.h"
#include <vector>

// cost: n x n bytes (0 / 1), row-major -> col4row (n ints); returns the solver's code
extern "C" int lsap_solve01(const uint8_t* cost, int n, int32_t* col4row) {
  if (n <= 0) return 0;
  std::vector<double> u(n), v(n), spc(n);
  std::vector<int> path(n), row4col(n), remaining(n), c4r(n);
  std::vector<uint8_t> SR(n), SC(n);
  const int rc = rap_lsap_solve(n, [=](int i, int j) { return (double)cost[(size_t)i * n + j]; }, u.data(), v.data(), spc.data(), path.data(),
                                c4r.data(), row4col.data(), SR.data(), SC.data(), remaining.data());
  for (int i = 0; i < n; ++i) col4row[i] = c4r[i];
  return rc;
}

// one scan state -> the pick of SciPy's loop (out[0]) and of the combine rule folded left to right (out[1]) and as a balanced tree (out[2])
static RapLsapPick tree(const int* remaining, const double* spc, const int* row4col, int a, int e) {
  if (e - a == 1) return rap_lsap_pick_of(spc[remaining[a]], a, row4col[remaining[a]] == -1);
  const int m = a + (e - a) / 2;
  return rap_lsap_pick_combine(tree(remaining, spc, row4col, m, e), tree(remaining, spc, row4col, a, m));      // right operand first: order must not matter
}
extern "C" void lsap_picks(int num_remaining, const int32_t* remaining, const double* spc, const int32_t* row4col, int32_t* out, double* lowest) {
  out[0] = rap_lsap_pick_sequential(num_remaining, remaining, spc, row4col, &lowest[0]);
  out[1] = rap_lsap_pick_reduced(num_remaining, remaining, spc, row4col, &lowest[1]);
  if (num_remaining > 0) {
    const RapLsapPick p = tree(remaining, spc, row4col, 0, num_remaining);
    out[2] = p.first < 0 ? -1 : rap_lsap_pick_index(p);
    lowest[2] = p.val;
  } else {
    out[2] = -1; lowest[2] = INFINITY;
  }
}
