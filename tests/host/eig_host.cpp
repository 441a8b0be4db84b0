// Host build of the symmetric eigen-solvers of rap_amd/csrc/kabsch.h (the code normals.hip and icp_plane.hip run on the device), for
// tests/test_normals_host.py: g++ -O2 -shared -fPIC.  Matrices are row-major doubles.
#include "../../rap_amd/csrc/kabsch.h"

extern "C" {

// C (3x3 symmetric) -> lam[3] ascending, n[3] the unit eigenvector of lam[0]
void eig3_smallest(const double* C, double* lam, double* n) {
  double M[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) M[i][j] = C[3 * i + j];
  rap_sym_eig3_smallest(M, lam, n);
}

// A (6x6 symmetric) -> lam[6] (the diagonal after the sweeps, unordered), V[36] (columns = eigenvectors)
void eig6(const double* A, double* lam, double* V) {
  double M[6][6], W[6][6];
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) M[i][j] = A[6 * i + j];
  rap_sym_eig<6>(M, W);
  for (int i = 0; i < 6; ++i) {
    lam[i] = M[i][i];
    for (int j = 0; j < 6; ++j) V[6 * i + j] = W[i][j];
  }
}

// x = -A^+ b with eigenvalues <= rcond * lambda_max dropped
void pinv6_step(const double* A, const double* b, double rcond, double* x) {
  double M[6][6];
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) M[i][j] = A[6 * i + j];
  rap_pinv6_step(M, b, rcond, x);
}

// R (3x3) = exp([w]x)
void rodrigues(const double* w, double* R) {
  double M[3][3];
  rap_rodrigues(w, M);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R[3 * i + j] = M[i][j];
}
}
