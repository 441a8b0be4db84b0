// Square linear sum assignment, restated from SciPy's published rectangular_lsap (scipy/optimize/rectangular_lsap: the shortest
// augmenting path routine of Crouse 2016, "On implementing 2D rectangular assignment algorithms") so that the PERMUTATION it returns --
// not only the optimal value, which is unique -- is the one scipy.optimize.linear_sum_assignment returns (reference
// eval/metrics.py:152-158 keeps that permutation as matched_part_ids).  Plain C++: the device kernel (part_acc.hip) and the host wrapper
// of the CPU tests (tests/host/assign_host.cpp) compile the same lines.
//
// What decides the permutation, kept literally:
//   * rows are augmented in order 0 .. n-1;
//   * the scan list starts as remaining[it] = n - it - 1;
//   * every scan relaxes r = minVal + cost[i][j] - u[i] - v[j] into shortestPathCosts[j] / path[j] on a STRICT <;
//   * the scan's pick moves to position `it` when spc[j] < lowest, or when spc[j] == lowest and column j is unassigned;
//   * the picked entry is removed by overwriting it with the LAST remaining entry;
//   * duals of the visited rows / columns are updated, then the matching is flipped along `path`.
// All arithmetic is in double; with 0/1 costs every value is a small integer and exact.
//
// The part of a scan that does not depend on who runs it is its pick.  Sequentially it is a fold over the positions; as a reduction it is
// RapLsapPick with rap_lsap_pick_combine: among the positions that hold the minimum value take the LAST one whose column is unassigned,
// and if there is none the FIRST one.  (The fold sets the pick at the first position that reaches the minimum -- strict < -- and moves it
// afterwards only onto unassigned columns at the same value.)  The combine is associative and commutative, so any reduction tree gives the
// fold's answer; tests/test_part_acc_host.py holds it to the fold on random scan states.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RAP_LSAP_HD __host__ __device__ __forceinline__
#else
#define RAP_LSAP_HD static inline
#endif

#define RAP_LSAP_MAX_N 256

struct RapLsapPick {
  double val;       // the smallest shortestPathCosts seen; INFINITY: nothing seen
  int first;        // first position that holds val
  int last_free;    // last position that holds val and whose column is unassigned; -1: none
};

RAP_LSAP_HD RapLsapPick rap_lsap_pick_none() {
  RapLsapPick p; p.val = INFINITY; p.first = -1; p.last_free = -1;
  return p;
}
RAP_LSAP_HD RapLsapPick rap_lsap_pick_of(double val, int it, bool column_unassigned) {
  RapLsapPick p; p.val = val; p.first = it; p.last_free = column_unassigned ? it : -1;
  if (!(val < INFINITY) && !column_unassigned) p.first = -1;      // the fold never stops on an assigned column at INFINITY
  return p;
}
RAP_LSAP_HD RapLsapPick rap_lsap_pick_combine(const RapLsapPick& a, const RapLsapPick& b) {
  if (a.first < 0) return b;
  if (b.first < 0) return a;
  if (a.val < b.val) return a;
  if (b.val < a.val) return b;
  RapLsapPick p; p.val = a.val;
  p.first = a.first < b.first ? a.first : b.first;
  p.last_free = a.last_free > b.last_free ? a.last_free : b.last_free;
  return p;
}
// the position the sequential scan ends on
RAP_LSAP_HD int rap_lsap_pick_index(const RapLsapPick& p) { return p.last_free >= 0 ? p.last_free : p.first; }

// the pick as SciPy's loop takes it, position by position: the fold the combine rule restates.  -> index (-1: nothing remains)
RAP_LSAP_HD int rap_lsap_pick_sequential(int num_remaining, const int* remaining, const double* spc, const int* row4col, double* lowest_out) {
  int index = -1;
  double lowest = INFINITY;
  for (int it = 0; it < num_remaining; ++it) {
    const int j = remaining[it];
    if (spc[j] < lowest || (spc[j] == lowest && row4col[j] == -1)) { lowest = spc[j]; index = it; }
  }
  *lowest_out = lowest;
  return index;
}
// the same pick as a reduction over the positions, in the order a given tree visits them (here: left to right)
RAP_LSAP_HD int rap_lsap_pick_reduced(int num_remaining, const int* remaining, const double* spc, const int* row4col, double* lowest_out) {
  RapLsapPick pick = rap_lsap_pick_none();
  for (int it = 0; it < num_remaining; ++it) {
    const int j = remaining[it];
    pick = rap_lsap_pick_combine(pick, rap_lsap_pick_of(spc[j], it, row4col[j] == -1));
  }
  *lowest_out = pick.val;
  return rap_lsap_pick_index(pick);
}

// one relaxation of the scan: column j seen from row i
RAP_LSAP_HD void rap_lsap_relax(double minVal, double cost_ij, double u_i, double v_j, int i, double* spc_j, int* path_j) {
  const double r = minVal + cost_ij - u_i - v_j;
  if (r < *spc_j) { *path_j = i; *spc_j = r; }
}
// dual updates after the augmenting path of row cur ended with minVal
RAP_LSAP_HD double rap_lsap_dual_row(double u_i, bool visited, bool is_cur, double minVal, double spc_of_its_column) {
  if (is_cur) return u_i + minVal;
  return visited ? u_i + (minVal - spc_of_its_column) : u_i;
}
RAP_LSAP_HD double rap_lsap_dual_col(double v_j, bool visited, double minVal, double spc_j) {
  return visited ? v_j - (minVal - spc_j) : v_j;
}
// flip the matching along path from the sink back to row cur
RAP_LSAP_HD void rap_lsap_augment(const int* path, int* row4col, int* col4row, int sink, int cur) {
  int j = sink;
  for (;;) {
    const int i = path[j];
    row4col[j] = i;
    const int t = col4row[i]; col4row[i] = j; j = t;
    if (i == cur) break;
  }
}

// The serial solver.  cost(i, j) -> double.  Scratch: u, v, spc (n doubles each), path, row4col, remaining (n ints each), SR, SC (n bytes
// each).  col4row[i] (n ints) receives the column of row i.  Returns 0, or -1 when no finite assignment exists.
template <typename Cost>
RAP_LSAP_HD int rap_lsap_solve(int n, Cost cost, double* u, double* v, double* spc, int* path, int* col4row, int* row4col, uint8_t* SR,
                               uint8_t* SC, int* remaining) {
  for (int k = 0; k < n; ++k) { u[k] = 0.0; v[k] = 0.0; path[k] = -1; col4row[k] = -1; row4col[k] = -1; }
  for (int cur = 0; cur < n; ++cur) {
    double minVal = 0.0;
    int num_remaining = n, sink = -1, i = cur;
    for (int it = 0; it < n; ++it) { remaining[it] = n - it - 1; SR[it] = 0; SC[it] = 0; spc[it] = INFINITY; }
    while (sink == -1) {
      SR[i] = 1;
      for (int it = 0; it < num_remaining; ++it) {          // (a relaxation touches column remaining[it] only: relaxing first, then
        const int j = remaining[it];                         //  picking, is SciPy's single loop)
        rap_lsap_relax(minVal, cost(i, j), u[i], v[j], i, &spc[j], &path[j]);
      }
      const int index = rap_lsap_pick_sequential(num_remaining, remaining, spc, row4col, &minVal);
      if (index < 0 || minVal == INFINITY) return -1;
      const int j = remaining[index];
      if (row4col[j] == -1) sink = j; else i = row4col[j];
      SC[j] = 1;
      remaining[index] = remaining[--num_remaining];
    }
    for (int k = 0; k < n; ++k) {
      const int c = col4row[k];                              // a visited row other than cur is matched: c >= 0 wherever it is read
      u[k] = rap_lsap_dual_row(u[k], SR[k] != 0, k == cur, minVal, (k == cur || c < 0) ? 0.0 : spc[c]);
    }
    for (int k = 0; k < n; ++k) v[k] = rap_lsap_dual_col(v[k], SC[k] != 0, minVal, spc[k]);
    rap_lsap_augment(path, row4col, col4row, sink, cur);
  }
  return 0;
}
