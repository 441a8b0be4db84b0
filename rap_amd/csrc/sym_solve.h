// x = -H^+ g for a dense symmetric positive semi-definite n x n system (n even, <= 96: the block system of a scene, scene_refine.hip),
// fp64, worked on by all the threads of one block: a parallel-ordered cyclic Jacobi eigen-decomposition, then the pseudo-inverse
// without the eigenvalues <= rcond * lambda_max (the rule of rap_pinv6_step, kabsch.h).  tests/host/sym_solve_host.cpp compiles this
// header with g++ (one "thread", barriers that do nothing) against numpy.linalg.pinv.  Plain C++; the caller supplies the barrier.
//
// The ordering.  A sweep is n - 1 steps of n / 2 DISJOINT pairs (the round-robin tournament: index n - 1 stays, the others go round),
// so every pair (p, q) meets exactly once per sweep, and the n / 2 rotations of a step commute: A <- J^T A J with J their product.
// A step is three phases with a barrier after each:
//   1. pair j (one thread each): the rotation (c, s) that annihilates A[p][q], from A[p][p], A[q][q], A[p][q]; the pair's own 2 x 2
//      block gets its exact result (diagonals -+ t apq, off-diagonals 0), and no other phase touches that block.  A pair whose
//      |A[p][q]| <= 1e-18 |A|_F is skipped (c = 1, s = 0): the absolute threshold of rap_sym_eig, which is what lets the zero
//      eigenvalues of a rank-deficient H (a free gauge, a view without an edge) come out as ~1e-17 |H|, far below the relative cut
//   2. columns: for every row k outside the pair, (A[k][p], A[k][q]) <- (c akp - s akq, s akp + c akq); for every row k, the same on V
//   3. rows: for every column k outside the pair, (A[p][k], A[q][k]) likewise
// Every entry is written by one thread per phase, from values no thread writes in that phase, so the result does not depend on the
// number of threads: the host build and the device give the same statements in the same order.
// The sweep cap (SYM_SOLVE_MAX_SWEEPS) is reasoned in DESIGN.md section 7.9: the ordering converges quadratically like the row-cyclic
// one; the host test measures 6 .. 13 sweeps for n = 6 .. 96 on its matrices, rank-deficient ones included (the count grows like log n),
// and the cap is more than twice that.  At the cap the solve goes on with what it has.
#pragma once
#include <math.h>

#ifndef RAP_HD
#if defined(__HIPCC__)
#define RAP_HD __host__ __device__
#else
#define RAP_HD
#endif
#endif

#define SYM_SOLVE_MAX_N 96
#define SYM_SOLVE_MAX_SWEEPS 32

// scratch of one solve besides A and V (n x n doubles each, row stride n): rotation of every pair, the coefficients, two flags
struct SymSolveScratch {
  double c[SYM_SOLVE_MAX_N / 2], s[SYM_SOLVE_MAX_N / 2];
  double f[SYM_SOLVE_MAX_N];
  double tiny, lmax;
  int pp[SYM_SOLVE_MAX_N / 2], qq[SYM_SOLVE_MAX_N / 2];
  int rotated, sweeps;
};

// pair j of step `step` of the tournament on n (even) indices, p < q
RAP_HD inline void sym_solve_pair(int n, int step, int j, int& p, int& q) {
  const int m = n - 1;
  int a, b;
  if (j == 0) { a = m; b = step % m; }
  else { a = (step + j) % m; b = (step - j + m) % m; }
  p = a < b ? a : b;
  q = a < b ? b : a;
}

// Eigen-decomposition in place: on return the diagonal of A holds the eigenvalues and column j of V the unit eigenvector of A[j][j].
// Every thread of the block calls it with its tid in [0, nt); sync() is the block's barrier.  Returns the number of sweeps run.
template <class Sync>
RAP_HD inline int sym_solve_eig(double* A, double* V, int n, SymSolveScratch* w, int tid, int nt, Sync sync) {
  for (int i = tid; i < n * n; i += nt) V[i] = (i / n == i % n) ? 1.0 : 0.0;
  if (tid == 0) {
    double fro = 0.0;
    for (int i = 0; i < n * n; ++i) fro += A[i] * A[i];
    w->tiny = 1e-18 * sqrt(fro);
    w->rotated = 0;
    w->sweeps = 0;
  }
  sync();
  const int half = n / 2;
  for (int sweep = 0; sweep < SYM_SOLVE_MAX_SWEEPS; ++sweep) {
    for (int step = 0; step < n - 1; ++step) {
      for (int j = tid; j < half; j += nt) {                       // phase 1
        int p, q;
        sym_solve_pair(n, step, j, p, q);
        w->pp[j] = p; w->qq[j] = q;
        const double apq = A[p * n + q];
        double c = 1.0, s = 0.0;
        if (fabs(apq) > w->tiny) {
          const double theta = (A[q * n + q] - A[p * n + p]) / (2.0 * apq);
          const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(1.0 + theta * theta));
          c = 1.0 / sqrt(1.0 + t * t);
          s = c * t;
          A[p * n + p] -= t * apq;
          A[q * n + q] += t * apq;
          A[p * n + q] = 0.0;
          A[q * n + p] = 0.0;
          w->rotated = 1;                                          // every writer stores the same value
        }
        w->c[j] = c; w->s[j] = s;
      }
      sync();
      for (int i = tid; i < n * half; i += nt) {                   // phase 2: columns of A (rows outside the pair) and of V
        const int k = i / half, j = i % half;
        const double c = w->c[j], s = w->s[j];
        if (s == 0.0) continue;
        const int p = w->pp[j], q = w->qq[j];
        if (k != p && k != q) {
          const double akp = A[k * n + p], akq = A[k * n + q];
          A[k * n + p] = c * akp - s * akq;
          A[k * n + q] = s * akp + c * akq;
        }
        const double vkp = V[k * n + p], vkq = V[k * n + q];
        V[k * n + p] = c * vkp - s * vkq;
        V[k * n + q] = s * vkp + c * vkq;
      }
      sync();
      for (int i = tid; i < n * half; i += nt) {                   // phase 3: rows of A (columns outside the pair)
        const int j = i / n, k = i % n;
        const double c = w->c[j], s = w->s[j];
        if (s == 0.0) continue;
        const int p = w->pp[j], q = w->qq[j];
        if (k == p || k == q) continue;
        const double apk = A[p * n + k], aqk = A[q * n + k];
        A[p * n + k] = c * apk - s * aqk;
        A[q * n + k] = s * apk + c * aqk;
      }
      sync();
    }
    const int rotated = w->rotated;
    sync();
    if (tid == 0) { w->rotated = 0; w->sweeps = sweep + 1; }
    sync();
    if (!rotated) break;
  }
  return w->sweeps;
}

// x = -H^+ g.  A holds H on entry (row stride n, both triangles) and is destroyed; V: n x n scratch.  n == 0 does nothing.
template <class Sync>
RAP_HD inline int sym_solve_pinv_step(double* A, double* V, const double* g, double* x, int n, double rcond, SymSolveScratch* w, int tid,
                                      int nt, Sync sync) {
  if (n <= 0) return 0;
  const int sweeps = sym_solve_eig(A, V, n, w, tid, nt, sync);
  if (tid == 0) {
    double lmax = 0.0;
    for (int j = 0; j < n; ++j) lmax = fmax(lmax, A[j * n + j]);
    w->lmax = lmax;
  }
  sync();
  for (int j = tid; j < n; j += nt) {
    const double lam = A[j * n + j];
    double f = 0.0;
    if (lam > rcond * w->lmax) {
      double vb = 0.0;
      for (int i = 0; i < n; ++i) vb += V[i * n + j] * g[i];
      f = -vb / lam;
    }
    w->f[j] = f;
  }
  sync();
  for (int i = tid; i < n; i += nt) {
    double v = 0.0;
    for (int j = 0; j < n; ++j) v += w->f[j] * V[i * n + j];
    x[i] = v;
  }
  sync();
  return sweeps;
}
