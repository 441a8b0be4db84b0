// Joint multi-view point-to-plane refinement of registered scenes on the device (rap_scene_refine, include/rapflow.h): one Gauss-Newton
// problem per scene over the poses of all its views, every directed edge (source view a, target view b) contributing the point-to-plane
// moments of a's rows against their nearest rows of b.  The pairwise estimator (icp_plane.hip) is the special case of two views, one
// edge and the target fixed; what is new here is the work list over (edge, 256 rows of the source view), the block system of a scene and
// its dense solve.  Unpinned: the reference has no counterpart (it runs pytorch3d's pairwise ICP only); tests/scene_refine_oracle.py
// restates the header in fp64.
//
//   scene_setup_kernel     clamped view table, view -> scene, fixed flags, the live edges and their items (all of an edge or none, while
//                          the row budget lasts), every scene's edge list (a stable counting sort by scene), the fp64 pose of every
//                          view = its fp32 start, outputs and flags
//   launch_nn_grid_build   the uniform-grid index of nn_grid.hip with y_seg = view_seg: one grid per view, built once per call
//   per iteration, enqueued max_iterations times up front:
//   scene_edge_pose_kernel  R_e = R_a R_b^T, T_e = (T_a - T_b) R_b^T in double from the fp64 state, rounded to fp32; the edge's done flag
//   scene_query_kernel      the ICP query head (icp.h) with the edge's pose, grid_search on the TARGET view's grid, icp_plane_moments
//   scene_edge_kernel       one wave per edge: item partials added lane-strided in item order; the edge's rmse and count; the moments
//                           carried into the world frame, A_w = M_b^T A_e M_b and g_w = M_b^T b_e (36 + 6 lanes)
//   scene_solve_kernel      one block of 512 threads per scene: total count and rmse; the 6 Vf x 6 Vf system over the Vf free views,
//                           every entry summed by its one owner thread in ascending edge order; x = -H^+ g (sym_solve.h, parallel-ordered
//                           cyclic Jacobi in LDS); the update of every free view; the stopping rule (icp_finish_end)
// H, the eigenvectors, g and x live in LDS: two (6 max_views)^2 fp64 matrices are 147 KB at max_views = 16, inside the 160 KB of a
// CDNA4 compute unit, and a Jacobi step is three barrier-separated passes over them, each entry read and written once -- from the
// workspace every pass would be a round trip to L2.  One block per compute unit is no loss: a scene has one block.
// No host read, no allocation, no floating-point atomics; a scene's bits depend on its own views and edges only.
#include "icp.h"
#include "kabsch.h"
#include "nn_grid_search.h"
#include "sym_solve.h"

#define SCENE_RCOND 1e-12          // ICP_PLANE_RCOND
#define SCENE_THREADS 512
#define SCENE_CHUNK 256            // edges of a scene staged in LDS at a time
#define SCENE_MAX_VIEWS 16
#define SCENE_EDGE_W 42            // A_w (6 x 6, both triangles) and g_w per edge

struct SceneEdge { int first, count, a, b; };        // the edge's items (count 0: ignored), source and target view
struct SceneView { int start, len, scene, fixed; };  // clamped rows; scene -1: outside every scene, or in one that is left out
struct SceneTab { int first, count, edge_first, edge_count; };      // views (count -1: left out) and the range in edge_order

struct SceneWs {
  NnWork* items; IcpPlanePartial* partials; SceneEdge* edges; int32_t* edge_scene; int32_t* edge_order; int32_t* edone;
  float* edge_R; float* edge_T; IcpPlanePartial* edge_mom; double* edge_w; SceneView* views; double* state; SceneTab* scenes;
  double* prev; int32_t* done; NnGridWs grid; size_t total;
};

static long scene_max_items(int64_t row_budget, int E) { return (long)(row_budget / NN_TILE) + E + 1; }

// robust: partials and edge_mom hold IcpPlaneWPartial (the moments and W = sum w) behind the same pointers
static SceneWs scene_carve(void* base, int64_t n_points, int V, int S, int E, int64_t row_budget, bool robust = false) {
  const size_t partial = robust ? sizeof(IcpPlaneWPartial) : sizeof(IcpPlanePartial);
  SceneWs w; Carver c(base);
  const size_t max_items = (size_t)scene_max_items(row_budget, E);
  w.items = (NnWork*)c.take(max_items * sizeof(NnWork));
  w.partials = (IcpPlanePartial*)c.take(max_items * partial);
  w.edges = (SceneEdge*)c.take((size_t)E * sizeof(SceneEdge));
  w.edge_scene = (int32_t*)c.take((size_t)E * 4);
  w.edge_order = (int32_t*)c.take((size_t)E * 4);
  w.edone = (int32_t*)c.take((size_t)E * 4);
  w.edge_R = (float*)c.take((size_t)E * 9 * 4);
  w.edge_T = (float*)c.take((size_t)E * 3 * 4);
  w.edge_mom = (IcpPlanePartial*)c.take((size_t)E * partial);
  w.edge_w = (double*)c.take((size_t)E * SCENE_EDGE_W * 8);
  w.views = (SceneView*)c.take((size_t)V * sizeof(SceneView));
  w.state = (double*)c.take((size_t)V * 12 * 8);
  w.scenes = (SceneTab*)c.take((size_t)S * sizeof(SceneTab));
  w.prev = (double*)c.take((size_t)S * 8);
  w.done = (int32_t*)c.take((size_t)S * 4);
  w.grid = nn_grid_carve(c, (long)n_points, V);
  w.total = c.total();
  return w;
}

// LDS of the solve kernel for systems of up to n = 6 max_views unknowns: A, V, g, x, the solver's scratch, the edge chunk, the rest
struct SceneShared {
  SymSolveScratch solve;
  int chunk_e[SCENE_CHUNK], chunk_n[SCENE_CHUNK];
  double chunk_err[SCENE_CHUNK];
  short chunk_a[SCENE_CHUNK], chunk_b[SCENE_CHUNK];
  int slot[SCENE_MAX_VIEWS];
  double tot_err;
  long long tot_n;
  int n;
};
// ... of the robust call: the weight sums beside the counts
struct SceneSharedW : SceneShared {
  double chunk_w[SCENE_CHUNK];
  double tot_w;
};
static size_t scene_lds_bytes(int max_views, bool robust = false) {
  const size_t n = 6 * (size_t)max_views;
  return align_up(robust ? sizeof(SceneSharedW) : sizeof(SceneShared), 16) + (2 * n * n + 2 * n) * sizeof(double);
}

__global__ __launch_bounds__(256) void scene_setup_kernel(const int32_t* __restrict__ view_seg, int V, long N, const int32_t* __restrict__ scene_seg,
                                                          int S, const int32_t* __restrict__ edge_tab, int E, long row_budget, int max_views,
                                                          const uint8_t* __restrict__ fixed, const float* __restrict__ init_R,
                                                          const float* __restrict__ init_T, int max_items, SceneWs w, float* __restrict__ R,
                                                          float* __restrict__ T, float* __restrict__ rmse, int32_t* __restrict__ iterations,
                                                          uint8_t* __restrict__ converged, float* __restrict__ edge_rmse,
                                                          int32_t* __restrict__ edge_count) {
  if (blockIdx.x != 0) return;
  for (int v = threadIdx.x; v < V; v += 256) {
    SceneView sv;
    nn_segment(view_seg, v, N, sv.start, sv.len);
    sv.scene = -1;
    sv.fixed = fixed ? (fixed[v] != 0) : 0;
    w.views[v] = sv;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int s = 0; s < S; ++s) {
      SceneTab st;
      nn_segment(scene_seg, s, (long)V, st.first, st.count);
      st.edge_first = 0; st.edge_count = 0;
      if (st.count > max_views) {
        st.count = -1;                               // left out
      } else {
        for (int v = st.first; v < st.first + st.count; ++v) w.views[v].scene = s;
        if (!fixed && st.count > 0) w.views[st.first].fixed = 1;
      }
      w.scenes[s] = st;
    }
    int n = 0;
    long rows = 0;
    for (int e = 0; e < E; ++e) {
      const int a = edge_tab[(size_t)e * 2], b = edge_tab[(size_t)e * 2 + 1];
      SceneEdge se = {n, 0, a, b};
      int sc = -1;
      if (a >= 0 && a < V && b >= 0 && b < V && a != b) {
        const SceneView va = w.views[a], vb = w.views[b];
        const int want = (va.len + NN_TILE - 1) / NN_TILE;
        if (va.scene >= 0 && va.scene == vb.scene && va.len > 0 && vb.len > 0 && rows + va.len <= row_budget && want <= max_items - n) {
          for (int q0 = 0; q0 < va.len; q0 += NN_TILE) { NnWork it = {va.start, va.len, q0, vb.start, vb.len, e, b, 0}; w.items[n++] = it; }
          se.count = want;
          rows += va.len;
          sc = va.scene;
          ++w.scenes[sc].edge_count;
        }
      }
      w.edges[e] = se;
      w.edge_scene[e] = sc;
    }
    nn_zero_items(w.items, n, max_items);
    int at = 0;
    for (int s = 0; s < S; ++s) { w.scenes[s].edge_first = at; at += w.scenes[s].edge_count; w.scenes[s].edge_count = 0; }
    for (int e = 0; e < E; ++e) {
      const int sc = w.edge_scene[e];
      if (sc >= 0) w.edge_order[w.scenes[sc].edge_first + w.scenes[sc].edge_count++] = e;
    }
  }
  __syncthreads();
  for (int v = threadIdx.x; v < V; v += 256) {
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      const float r = init_R ? init_R[(size_t)v * 9 + i] : (i % 4 == 0 ? 1.f : 0.f);
      R[(size_t)v * 9 + i] = r;
      w.state[(size_t)v * 12 + i] = (double)r;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const float t = init_T ? init_T[(size_t)v * 3 + i] : 0.f;
      T[(size_t)v * 3 + i] = t;
      w.state[(size_t)v * 12 + 9 + i] = (double)t;
    }
  }
  for (int s = threadIdx.x; s < S; s += 256) {
    rmse[s] = __builtin_nanf("");
    iterations[s] = 0;
    converged[s] = 0;
    w.prev[s] = -1.0;
    w.done[s] = w.scenes[s].count < 0 ? 1 : 0;
  }
  for (int e = threadIdx.x; e < E; e += 256) {
    if (edge_rmse) edge_rmse[e] = __builtin_nanf("");
    if (edge_count) edge_count[e] = 0;
    w.edone[e] = 1;
  }
}

__global__ __launch_bounds__(256) void scene_edge_pose_kernel(const SceneEdge* __restrict__ edges, const int32_t* __restrict__ edge_scene, int E,
                                                              const double* __restrict__ state, const int32_t* __restrict__ done,
                                                              float* __restrict__ edge_R, float* __restrict__ edge_T,
                                                              int32_t* __restrict__ edone) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  const int sc = edge_scene[e];
  if (sc < 0) return;                                // edone stays 1
  const int d = done[sc];
  edone[e] = d;
  if (d) return;
  const double* sa = state + (size_t)edges[e].a * 12;
  const double* sb = state + (size_t)edges[e].b * 12;
  // R_e[i][j] = sum_l R_a[i][l] R_b[j][l];  T_e[j] = sum_l (T_a - T_b)[l] R_b[j][l]
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double r0, r1, r2;
    if (i < 3) { r0 = sa[3 * i]; r1 = sa[3 * i + 1]; r2 = sa[3 * i + 2]; }
    else { r0 = sa[9] - sb[9]; r1 = sa[10] - sb[10]; r2 = sa[11] - sb[11]; }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double v = r0 * sb[3 * j] + r1 * sb[3 * j + 1] + r2 * sb[3 * j + 2];
      if (i < 3) edge_R[(size_t)e * 9 + 3 * i + j] = (float)v;
      else edge_T[(size_t)e * 3 + j] = (float)v;
    }
  }
}

// item: pad0 = the edge (its pose and done flag), pad1 = the target view (its grid)
__global__ __launch_bounds__(ICP_TILE) void scene_query_kernel(const float* __restrict__ P, const float* __restrict__ Pn,
                                                               const NnWork* __restrict__ items, const float* __restrict__ R,
                                                               const float* __restrict__ T, const int32_t* __restrict__ done, float gate,
                                                               const NnGrid* __restrict__ grids, const unsigned* __restrict__ cell_start,
                                                               const float4* __restrict__ sorted, IcpPlanePartial* __restrict__ partials) {
  __shared__ double red_m[ICP_TILE / 64][ICP_PLANE_NMOM];
  __shared__ int red_n[ICP_TILE / 64];
  ICP_QUERY_BEGIN(P, items, R, T, done);
  float best;
  int besti;
  grid_search(grids[w.pad1], P, cell_start, sorted, px, py, pz, grid_gate2(gate), best, besti);
  icp_plane_moments<RAP_LOSS_NONE>(active, besti, best, gate, px, py, pz, P, Pn, w.y_start, red_m, red_n, partials + blockIdx.x);
}

// the robust call's query (rap_scene_refine_robust): the weighted epilogue of icp.h
template <int LOSS>
__global__ __launch_bounds__(ICP_TILE) void scene_query_robust_kernel(const float* __restrict__ P, const float* __restrict__ Pn,
                                                                      const NnWork* __restrict__ items, const float* __restrict__ R,
                                                                      const float* __restrict__ T, const int32_t* __restrict__ done, float gate,
                                                                      const NnGrid* __restrict__ grids, const unsigned* __restrict__ cell_start,
                                                                      const float4* __restrict__ sorted, double scale,
                                                                      IcpPlaneWPartial* __restrict__ partials) {
  __shared__ double red_m[ICP_TILE / 64][ICP_PLANE_WMOM];
  __shared__ int red_n[ICP_TILE / 64];
  ICP_QUERY_BEGIN(P, items, R, T, done);
  float best;
  int besti;
  grid_search(grids[w.pad1], P, cell_start, sorted, px, py, pz, grid_gate2(gate), best, besti);
  icp_plane_moments<LOSS>(active, besti, best, gate, px, py, pz, P, Pn, w.y_start, red_m, red_n, partials + blockIdx.x, scale);
}

struct SceneSolveArgs {
  const SceneTab* scenes; const SceneView* views; const SceneEdge* edges; const int32_t* edge_order; const IcpPlanePartial* edge_mom;
  const double* edge_w; double* state; float* R; float* T; float* rmse; int32_t* iterations; uint8_t* converged; double* prev;
  int32_t* done; int it; double rel_thr;
};

#define SCENE_IF_WEIGHTED(...)
#define SCENE_EDGE_KERNEL scene_edge_kernel
#define SCENE_SOLVE_KERNEL scene_solve_kernel
#define SCENE_PARTIAL IcpPlanePartial
#define SCENE_SHARED SceneShared
#include "scene_refine_sums.inc"
#undef SCENE_IF_WEIGHTED
#undef SCENE_EDGE_KERNEL
#undef SCENE_SOLVE_KERNEL
#undef SCENE_PARTIAL
#undef SCENE_SHARED
#define SCENE_IF_WEIGHTED(...) __VA_ARGS__
#define SCENE_EDGE_KERNEL scene_edge_robust_kernel
#define SCENE_SOLVE_KERNEL scene_solve_robust_kernel
#define SCENE_PARTIAL IcpPlaneWPartial
#define SCENE_SHARED SceneSharedW
#include "scene_refine_sums.inc"
#undef SCENE_IF_WEIGHTED
#undef SCENE_EDGE_KERNEL
#undef SCENE_SOLVE_KERNEL
#undef SCENE_PARTIAL
#undef SCENE_SHARED

extern "C" size_t rap_scene_refine_workspace_bytes(int64_t n_points, int32_t V, int32_t S, int32_t E, int64_t row_budget, int32_t max_views) {
  if (n_points <= 0 || n_points > 0x7fffffffLL / 8 || V <= 0 || V > 65535 || S <= 0 || E <= 0 || E > 65535 || row_budget <= 0 ||
      row_budget / NN_TILE > 0x7fffffffLL / 64 || max_views < 2 || max_views > SCENE_MAX_VIEWS)
    return 0;
  return scene_carve(nullptr, n_points, V, S, E, row_budget).total;
}

extern "C" size_t rap_scene_refine_robust_workspace_bytes(int64_t n_points, int32_t V, int32_t S, int32_t E, int64_t row_budget,
                                                          int32_t max_views) {
  if (!rap_scene_refine_workspace_bytes(n_points, V, S, E, row_budget, max_views)) return 0;
  return scene_carve(nullptr, n_points, V, S, E, row_budget, true).total;
}

template <int LOSS>
static void scene_query_robust(hipStream_t stream, unsigned max_items, const float* P, const float* normals, const SceneWs& w, float gate,
                               double scale) {
  hipLaunchKernelGGL(scene_query_robust_kernel<LOSS>, dim3(max_items), dim3(ICP_TILE), 0, stream, P, normals, (const NnWork*)w.items,
                     (const float*)w.edge_R, (const float*)w.edge_T, (const int32_t*)w.edone, gate, (const NnGrid*)w.grid.grids,
                     (const unsigned*)w.grid.cell_start, (const float4*)w.grid.sorted, scale, (IcpPlaneWPartial*)w.partials);
}

// both entry points; robust: the weighted kernels with loss (a RAP_LOSS_* code, checked here) at loss_scale
static int scene_entry(const float* P, const float* normals, const int32_t* view_seg, int32_t V, int64_t n_points, const int32_t* scene_seg,
                       int32_t S, const int32_t* edges, int32_t E, int64_t row_budget, int32_t max_views, const uint8_t* fixed,
                       const float* init_R, const float* init_T, int32_t max_iterations, float relative_rmse_thr,
                       float max_correspondence_distance, float* R, float* T, float* rmse, int32_t* iterations, uint8_t* converged,
                       float* edge_rmse, int32_t* edge_count, bool robust, int32_t loss, float loss_scale, void* ws, size_t ws_bytes,
                       void* stream_) {
  if (!P || !normals || !view_seg || !scene_seg || !edges || !R || !T || !rmse || !iterations || !converged || n_points <= 0 ||
      n_points > 0x7fffffffLL / 8 || V <= 0 || V > 65535 || S <= 0 || E <= 0 || E > 65535 || row_budget <= 0 ||
      row_budget / NN_TILE > 0x7fffffffLL / 64 || max_views < 2 || max_views > SCENE_MAX_VIEWS || max_iterations <= 0 ||
      relative_rmse_thr != relative_rmse_thr || max_correspondence_distance != max_correspondence_distance)
    return RAP_ERR_INVALID;
  if (robust && (loss < RAP_LOSS_NONE || loss > RAP_LOSS_TUKEY || (loss != RAP_LOSS_NONE && !(loss_scale > 0.f && loss_scale < __builtin_inff()))))
    return RAP_ERR_INVALID;
  if (!ws) return RAP_ERR_WORKSPACE;
  const SceneWs w = scene_carve(ws, n_points, V, S, E, row_budget, robust);
  if (w.total > ws_bytes) return RAP_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  const int max_items = (int)scene_max_items(row_budget, E);
  const float gate = max_correspondence_distance > 0.f ? max_correspondence_distance : 0.f;
  hipLaunchKernelGGL(scene_setup_kernel, dim3(1), dim3(256), 0, stream, view_seg, V, (long)n_points, scene_seg, S, edges, E, (long)row_budget,
                     max_views, fixed, init_R, init_T, max_items, w, R, T, rmse, iterations, converged, edge_rmse, edge_count);
  RAP_LAUNCH_CHECK();
  int rc = launch_nn_grid_build(stream, P, view_seg, V, (long)n_points, w.grid);
  if (rc) return rc;
  const int lds = (int)scene_lds_bytes(max_views, robust);
  for (int it = 0; it < max_iterations; ++it) {
    hipLaunchKernelGGL(scene_edge_pose_kernel, dim3((E + 255) / 256), dim3(256), 0, stream, (const SceneEdge*)w.edges,
                       (const int32_t*)w.edge_scene, E, (const double*)w.state, (const int32_t*)w.done, w.edge_R, w.edge_T, w.edone);
    RAP_LAUNCH_CHECK();
    if (robust) {
      RAP_LOSS_DISPATCH(loss, scene_query_robust, stream, (unsigned)max_items, P, normals, w, gate, (double)loss_scale);
      RAP_LAUNCH_CHECK();
      hipLaunchKernelGGL(scene_edge_robust_kernel, dim3(E), dim3(64), 0, stream, (const IcpPlaneWPartial*)w.partials,
                         (const SceneEdge*)w.edges, (const int32_t*)w.edone, (const double*)w.state, (IcpPlaneWPartial*)w.edge_mom, w.edge_w,
                         edge_rmse, edge_count);
      RAP_LAUNCH_CHECK();
    } else {
      hipLaunchKernelGGL(scene_query_kernel, dim3((unsigned)max_items), dim3(ICP_TILE), 0, stream, P, normals, (const NnWork*)w.items,
                         (const float*)w.edge_R, (const float*)w.edge_T, (const int32_t*)w.edone, gate, (const NnGrid*)w.grid.grids,
                         (const unsigned*)w.grid.cell_start, (const float4*)w.grid.sorted, w.partials);
      RAP_LAUNCH_CHECK();
      hipLaunchKernelGGL(scene_edge_kernel, dim3(E), dim3(64), 0, stream, (const IcpPlanePartial*)w.partials, (const SceneEdge*)w.edges,
                         (const int32_t*)w.edone, (const double*)w.state, w.edge_mom, w.edge_w, edge_rmse, edge_count);
      RAP_LAUNCH_CHECK();
    }
    const SceneSolveArgs a = {w.scenes, w.views, w.edges, w.edge_order, w.edge_mom, w.edge_w, w.state, R, T, rmse, iterations, converged,
                              w.prev, w.done, it, (double)relative_rmse_thr};
    rc = robust ? rap_launch_dyn_lds(scene_solve_robust_kernel, dim3(S), dim3(SCENE_THREADS), lds, stream, a)
                : rap_launch_dyn_lds(scene_solve_kernel, dim3(S), dim3(SCENE_THREADS), lds, stream, a);
    if (rc) return rc;
  }
  return RAP_OK;
}

extern "C" int rap_scene_refine(const float* P, const float* normals, const int32_t* view_seg, int32_t V, int64_t n_points,
                                const int32_t* scene_seg, int32_t S, const int32_t* edges, int32_t E, int64_t row_budget, int32_t max_views,
                                const uint8_t* fixed, const float* init_R, const float* init_T, int32_t max_iterations,
                                float relative_rmse_thr, float max_correspondence_distance, float* R, float* T, float* rmse,
                                int32_t* iterations, uint8_t* converged, float* edge_rmse, int32_t* edge_count, void* ws, size_t ws_bytes,
                                void* stream) {
  return scene_entry(P, normals, view_seg, V, n_points, scene_seg, S, edges, E, row_budget, max_views, fixed, init_R, init_T, max_iterations,
                     relative_rmse_thr, max_correspondence_distance, R, T, rmse, iterations, converged, edge_rmse, edge_count, false, 0, 0.f,
                     ws, ws_bytes, stream);
}
extern "C" int rap_scene_refine_robust(const float* P, const float* normals, const int32_t* view_seg, int32_t V, int64_t n_points,
                                       const int32_t* scene_seg, int32_t S, const int32_t* edges, int32_t E, int64_t row_budget,
                                       int32_t max_views, const uint8_t* fixed, const float* init_R, const float* init_T,
                                       int32_t max_iterations, float relative_rmse_thr, float max_correspondence_distance, float* R, float* T,
                                       float* rmse, int32_t* iterations, uint8_t* converged, float* edge_rmse, int32_t* edge_count, int32_t loss,
                                       float loss_scale, void* ws, size_t ws_bytes, void* stream) {
  return scene_entry(P, normals, view_seg, V, n_points, scene_seg, S, edges, E, row_budget, max_views, fixed, init_R, init_T, max_iterations,
                     relative_rmse_thr, max_correspondence_distance, R, T, rmse, iterations, converged, edge_rmse, edge_count, true, loss,
                     loss_scale, ws, ws_bytes, stream);
}
