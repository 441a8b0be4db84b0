// Host build of the dense symmetric solve of rap_amd/csrc/sym_solve.h (the code scene_refine.hip runs on the device, there with 512
// threads and the block's barrier; here with one thread and a barrier that does nothing: the same statements on the same values), for
// tests/test_scene_refine_host.py: g++ -O2 -shared -fPIC.  Matrices are row-major doubles.
#include <vector>

#include "../../rap_amd/csrc/sym_solve.h"

extern "C" {

// x = -H^+ g with eigenvalues <= rcond * lambda_max dropped; n even, <= 96.  Returns the number of Jacobi sweeps, -1 for a bad n.
int sym_solve_step(const double* H, const double* g, int n, double rcond, double* x) {
  if (n < 0 || n > SYM_SOLVE_MAX_N || n % 2) return -1;
  std::vector<double> A(H, H + (size_t)n * n), V((size_t)n * n);
  SymSolveScratch w;
  return sym_solve_pinv_step(A.data(), V.data(), g, x, n, rcond, &w, 0, 1, [] {});
}

// the tournament: pair j of step `step` on n indices
void sym_solve_pair_of(int n, int step, int j, int* p, int* q) { sym_solve_pair(n, step, j, *p, *q); }

int sym_solve_max_sweeps(void) { return SYM_SOLVE_MAX_SWEEPS; }
}
