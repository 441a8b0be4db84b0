// The 1-NN walk over the uniform-grid index (grid_search), for the kernels that query it: the ICP and nearest-neighbour kernels of
// nn_grid.hip and the edge query of scene_refine.hip.  The index, the lower bound of the walk and its rounding margins are described
// at the top of nn_grid.hip.
#pragma once
#include "nn_grid.h"

// one candidate against the best so far: smallest (d2, index in the segment) wins
__device__ __forceinline__ void grid_consider(const float4 p, float qx, float qy, float qz, float& best, int& besti) {
  const float d2 = nn_d2(qx, qy, qz, p.x, p.y, p.z);
  const int idx = __float_as_int(p.w);
  if (d2 < best || (d2 == best && idx < besti)) { best = d2; besti = idx; }
}
// the candidates sorted[a .. b), four 16-byte loads in flight at a time (the loop is bound by their latency, not by the arithmetic)
__device__ __forceinline__ void grid_scan_run(const float4* __restrict__ sorted, unsigned a, unsigned b, float qx, float qy, float qz, float& best,
                                              int& besti) {
  unsigned j = a;
  for (; j + 4 <= b; j += 4) {
    const float4 p0 = sorted[j], p1 = sorted[j + 1], p2 = sorted[j + 2], p3 = sorted[j + 3];
    grid_consider(p0, qx, qy, qz, best, besti);
    grid_consider(p1, qx, qy, qz, best, besti);
    grid_consider(p2, qx, qy, qz, best, besti);
    grid_consider(p3, qx, qy, qz, best, besti);
  }
  for (; j < b; ++j) grid_consider(sorted[j], qx, qy, qz, best, besti);
}

// nearest row of problem g to (qx, qy, qz): best = its d2 (inf: none), besti = its index in the y segment (-1: none).  gate2 = inf: no gate.
__device__ __forceinline__ void grid_search(const NnGrid& g, const float* __restrict__ Y, const unsigned* __restrict__ cell_start,
                                            const float4* __restrict__ sorted, float qx, float qy, float qz, float gate2, float& best, int& besti) {
  best = __builtin_inff();
  besti = -1;
  if (g.mode == GRID_ROWS) {                          // no index for this problem: every row, in order
    for (int j = 0; j < g.y_len; ++j) {
      const float* p = Y + ((size_t)g.y_start + j) * 3;
      const float d2 = nn_d2(qx, qy, qz, p[0], p[1], p[2]);
      if (d2 < best) { best = d2; besti = j; }
    }
    return;
  }
  if (g.mode != GRID_CELLS) return;
  const int nx = g.dims[0], ny = g.dims[1], nz = g.dims[2];
  // projection onto the box (a NaN coordinate projects onto lo: such a query never wins a comparison anyway)
  const float cx = fminf(fmaxf(qx, g.lo[0]), g.hi[0]), cy = fminf(fmaxf(qy, g.lo[1]), g.hi[1]), cz = fminf(fmaxf(qz, g.lo[2]), g.hi[2]);
  const float ox = qx - cx, oy = qy - cy, oz = qz - cz;
  const float ox2 = ox * ox, oy2 = oy * oy, oz2 = oz * oz;
  const float tx = grid_t(cx, g.lo[0], g.h), ty = grid_t(cy, g.lo[1], g.h), tz = grid_t(cz, g.lo[2], g.h);
  const int ix = grid_cell(tx, nx), iy = grid_cell(ty, ny), iz = grid_cell(tz, nz);
  const unsigned* cs = cell_start + g.cell_base;
  for (int r = 0;; ++r) {
    const int x0 = max(ix - r, 0), x1 = min(ix + r, nx - 1), y0 = max(iy - r, 0), y1 = min(iy + r, ny - 1), z0 = max(iz - r, 0),
              z1 = min(iz + r, nz - 1);
    for (int z = z0; z <= z1; ++z) {
      const bool zface = z == iz - r || z == iz + r;
      for (int y = y0; y <= y1; ++y) {
        const int row = nx * (y + ny * z);
        if (zface || y == iy - r || y == iy + r) {
          grid_scan_run(sorted, cs[row + x0], cs[row + x1 + 1], qx, qy, qz, best, besti);
        } else {                                      // inside the shell's ring: only its two end cells are new
          if (ix - r >= 0) grid_scan_run(sorted, cs[row + ix - r], cs[row + ix - r + 1], qx, qy, qz, best, besti);
          if (ix + r < nx) grid_scan_run(sorted, cs[row + ix + r], cs[row + ix + r + 1], qx, qy, qz, best, besti);
        }
      }
    }
    if (x0 == 0 && x1 == nx - 1 && y0 == 0 && y1 == ny - 1 && z0 == 0 && z1 == nz - 1) break;      // the cube covers the grid
    // per axis: cells from q_c to the nearer face of the cube that has grid behind it (inf: none), then the distance from q to the
    // part of the box behind that face
    float sx = __builtin_inff(), sy = sx, sz = sx;
    if (x0 > 0) sx = tx - (float)x0;
    if (x1 < nx - 1) sx = fminf(sx, (float)(x1 + 1) - tx);
    if (y0 > 0) sy = ty - (float)y0;
    if (y1 < ny - 1) sy = fminf(sy, (float)(y1 + 1) - ty);
    if (z0 > 0) sz = tz - (float)z0;
    if (z1 < nz - 1) sz = fminf(sz, (float)(z1 + 1) - tz);
    const float mx = fabsf(ox) + fmaxf(sx - GRID_SLACK, 0.f) * g.h, my = fabsf(oy) + fmaxf(sy - GRID_SLACK, 0.f) * g.h,
                mz = fabsf(oz) + fmaxf(sz - GRID_SLACK, 0.f) * g.h;
    const float lb2 = fminf(fminf(mx * mx + (oy2 + oz2), my * my + (ox2 + oz2)), mz * mz + (ox2 + oy2)) * GRID_MARGIN;
    if (lb2 > best || lb2 > gate2) break;
  }
}
