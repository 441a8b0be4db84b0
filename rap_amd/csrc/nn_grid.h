// What the two searches over the uniform-grid index share (nn_grid.hip: the build and the 1-NN walk; nn_knn.hip: the k-best walk): the
// per-problem grid record, the margins of the lower bound, and the ONE definition of "position in cells" and "cell" that the build and
// every query use.  The index itself and the reasoning behind the margins are described at the top of nn_grid.hip.
#pragma once
#include "nn_tile.h"

#define GRID_SLACK 0.0009765625f          // 2^-10 cells
#define GRID_MARGIN 0.9999847412109375f   // 1 - 2^-16
#define GRID_GATE_MARGIN 1.0000152587890625f   // 1 + 2^-16: d2 > gate^2 (1 + 2^-16) implies sqrtf(d2) > gate after rounding

enum { GRID_NONE = 0, GRID_CELLS = 1, GRID_ROWS = 2 };      // empty y segment; indexed; searched row by row (no budget left)

struct NnGrid {                     // 64 bytes per problem
  float lo[3], h;
  float hi[3];
  int row_base;                     // first entry of this grid's rows in row_cell
  int dims[3], cell_base;           // first cell of this grid in the tables of the call
  int y_start, y_len, owner, mode;  // owner: the problem whose build kernels fill this grid (itself, or an earlier one with the same rows)
};

__device__ __forceinline__ bool grid_finite(float x, float y, float z) {
  const float inf = __builtin_inff();
  return fabsf(x) < inf && fabsf(y) < inf && fabsf(z) < inf;
}
// position in cells along one axis, and the cell it falls into: the ONE definition the build and the query share
__device__ __forceinline__ float grid_t(float p, float lo, float h) { return (p - lo) / h; }
__device__ __forceinline__ int grid_cell(float t, int dim) { return (int)fminf(fmaxf(floorf(t), 0.f), (float)(dim - 1)); }

__device__ __forceinline__ float grid_gate2(float gate) { return gate > 0.f ? gate * gate * GRID_GATE_MARGIN : __builtin_inff(); }
