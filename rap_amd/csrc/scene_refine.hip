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

static SceneWs scene_carve(void* base, int64_t n_points, int V, int S, int E, int64_t row_budget) {
  SceneWs w; Carver c(base);
  const size_t max_items = (size_t)scene_max_items(row_budget, E);
  w.items = (NnWork*)c.take(max_items * sizeof(NnWork));
  w.partials = (IcpPlanePartial*)c.take(max_items * sizeof(IcpPlanePartial));
  w.edges = (SceneEdge*)c.take((size_t)E * sizeof(SceneEdge));
  w.edge_scene = (int32_t*)c.take((size_t)E * 4);
  w.edge_order = (int32_t*)c.take((size_t)E * 4);
  w.edone = (int32_t*)c.take((size_t)E * 4);
  w.edge_R = (float*)c.take((size_t)E * 9 * 4);
  w.edge_T = (float*)c.take((size_t)E * 3 * 4);
  w.edge_mom = (IcpPlanePartial*)c.take((size_t)E * sizeof(IcpPlanePartial));
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
static size_t scene_lds_bytes(int max_views) {
  const size_t n = 6 * (size_t)max_views;
  return align_up(sizeof(SceneShared), 16) + (2 * n * n + 2 * n) * sizeof(double);
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
  icp_plane_moments(active, besti, best, gate, px, py, pz, P, Pn, w.y_start, red_m, red_n, partials + blockIdx.x);
}

__global__ __launch_bounds__(64) void scene_edge_kernel(const IcpPlanePartial* __restrict__ partials, const SceneEdge* __restrict__ edges,
                                                        const int32_t* __restrict__ edone, const double* __restrict__ state,
                                                        IcpPlanePartial* __restrict__ edge_mom, double* __restrict__ edge_w,
                                                        float* __restrict__ edge_rmse, int32_t* __restrict__ edge_count) {
  __shared__ double sA[36], sM[36], sb[6];
  const int e = blockIdx.x;
  if (edone[e]) return;
  const SceneEdge r = edges[e];
  ICP_SUM_PARTIALS(ICP_PLANE_NMOM, IcpPlanePartial, partials, r, m, n);
  const int t = threadIdx.x;
  if (t == 0) {
    IcpPlanePartial* o = edge_mom + e;
#pragma unroll
    for (int i = 0; i < ICP_PLANE_NMOM; ++i) o->m[i] = m[i];
    o->count = n;
    if (edge_rmse) edge_rmse[e] = n > 0 ? (float)sqrt(fmax(m[27] / (double)n, 0.0)) : __builtin_nanf("");
    if (edge_count) edge_count[e] = (int32_t)n;
    // M^T = [[C, [t]x C], [0, C]] with C = R_b^T (the column form of the target's rotation) and t = T_b:
    // J_w = [p_w x n_w, n_w] = M^T [q x n, n] for p_w = C q + t, n_w = C n
    const double* s = state + (size_t)r.b * 12;
    const double tx[3][3] = {{0.0, -s[11], s[10]}, {s[11], 0.0, -s[9]}, {-s[10], s[9], 0.0}};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const double c = s[3 * j + i];
        sM[6 * i + j] = c;
        sM[6 * (i + 3) + (j + 3)] = c;
        sM[6 * (i + 3) + j] = 0.0;
        sM[6 * i + (j + 3)] = tx[i][0] * s[3 * j + 0] + tx[i][1] * s[3 * j + 1] + tx[i][2] * s[3 * j + 2];
      }
    }
    int at = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
      for (int j = i; j < 6; ++j) { sA[6 * i + j] = m[at]; sA[6 * j + i] = m[at]; ++at; }
      sb[i] = m[21 + i];
    }
  }
  __syncthreads();
  double* out = edge_w + (size_t)e * SCENE_EDGE_W;
  if (t < 36) {
    // A_w[i][j] = sum_k M^T[i][k] (sum_l A[k][l] M^T[j][l]); entry (i, j) with i > j repeats the statements of (j, i): the same bits
    const int i0 = t / 6, j0 = t % 6, i = i0 < j0 ? i0 : j0, j = i0 < j0 ? j0 : i0;
    double acc = 0.0;
    for (int k = 0; k < 6; ++k) {
      double row = 0.0;
      for (int l = 0; l < 6; ++l) row += sA[6 * k + l] * sM[6 * j + l];
      acc += sM[6 * i + k] * row;
    }
    out[t] = acc;
  } else if (t < SCENE_EDGE_W) {
    const int i = t - 36;
    double acc = 0.0;
    for (int k = 0; k < 6; ++k) acc += sM[6 * i + k] * sb[k];
    out[t] = acc;
  }
}

struct SceneSolveArgs {
  const SceneTab* scenes; const SceneView* views; const SceneEdge* edges; const int32_t* edge_order; const IcpPlanePartial* edge_mom;
  const double* edge_w; double* state; float* R; float* T; float* rmse; int32_t* iterations; uint8_t* converged; double* prev;
  int32_t* done; int it; double rel_thr;
};

__global__ __launch_bounds__(SCENE_THREADS) void scene_solve_kernel(SceneSolveArgs p) {
  extern __shared__ __align__(16) unsigned char scene_lds[];
  const int sc = blockIdx.x;
  if (p.done[sc]) return;
  SceneShared* sh = (SceneShared*)scene_lds;
  double* mem = (double*)(scene_lds + ((sizeof(SceneShared) + 15) / 16) * 16);
  const int tid = threadIdx.x;
  const SceneTab st = p.scenes[sc];
  if (tid == 0) {
    int nf = 0;
    for (int l = 0; l < st.count; ++l) sh->slot[l] = p.views[st.first + l].fixed ? -1 : nf++;
    sh->n = 6 * nf;
    sh->tot_err = 0.0;
    sh->tot_n = 0;
  }
  __syncthreads();
  const int n = sh->n;
  double* A = mem;
  double* V = A + n * n;
  double* g = V + n * n;
  double* x = g + n;
  for (int i = tid; i < n * n + n; i += SCENE_THREADS) A[i < n * n ? i : i + n * n] = 0.0;      // A, then g behind V
  for (int c0 = 0; c0 < st.edge_count; c0 += SCENE_CHUNK) {
    const int nc = min(SCENE_CHUNK, st.edge_count - c0);
    __syncthreads();
    if (tid < nc) {
      const int e = p.edge_order[st.edge_first + c0 + tid];
      const SceneEdge se = p.edges[e];
      const long long ne = p.edge_mom[e].count;
      sh->chunk_e[tid] = e;
      sh->chunk_n[tid] = (int)ne;
      sh->chunk_err[tid] = p.edge_mom[e].m[27];
      sh->chunk_a[tid] = (short)sh->slot[se.a - st.first];
      sh->chunk_b[tid] = (short)sh->slot[se.b - st.first];
    }
    __syncthreads();
    if (tid == 0) {
      double err = sh->tot_err;
      long long cnt = sh->tot_n;
      for (int c = 0; c < nc; ++c) { err += sh->chunk_err[c]; cnt += sh->chunk_n[c]; }
      sh->tot_err = err; sh->tot_n = cnt;
    }
    for (int idx = tid; idx < n * n + n; idx += SCENE_THREADS) {
      double acc;
      if (idx < n * n) {
        const int i = idx / n, j = idx % n, vi = i / 6, vj = j / 6, off = (i % 6) * 6 + j % 6;
        acc = A[idx];
        for (int c = 0; c < nc; ++c) {
          if (sh->chunk_n[c] == 0) continue;
          const int a = sh->chunk_a[c], b = sh->chunk_b[c];
          if (vi == vj) {
            if (a == vi || b == vi) acc += p.edge_w[(size_t)sh->chunk_e[c] * SCENE_EDGE_W + off];
          } else if ((a == vi && b == vj) || (a == vj && b == vi)) {
            acc -= p.edge_w[(size_t)sh->chunk_e[c] * SCENE_EDGE_W + off];
          }
        }
        A[idx] = acc;
      } else {
        const int i = idx - n * n, vi = i / 6;
        acc = g[i];
        for (int c = 0; c < nc; ++c) {
          if (sh->chunk_n[c] == 0) continue;
          const double gw = p.edge_w[(size_t)sh->chunk_e[c] * SCENE_EDGE_W + 36 + i % 6];
          if (sh->chunk_a[c] == vi) acc += gw;
          if (sh->chunk_b[c] == vi) acc -= gw;
        }
        g[i] = acc;
      }
    }
  }
  __syncthreads();
  const long long cnt = sh->tot_n;
  if (cnt == 0) {                                    // no pair with a usable normal in the whole scene: stop with the poses it had
    if (tid == 0) { p.rmse[sc] = __builtin_inff(); p.done[sc] = 1; }
    return;
  }
  sym_solve_pinv_step(A, V, g, x, n, SCENE_RCOND, &sh->solve, tid, SCENE_THREADS, [] { __syncthreads(); });
  if (tid < st.count && sh->slot[tid] >= 0) {
    const double* xi = x + 6 * sh->slot[tid];
    if (xi[0] != 0.0 || xi[1] != 0.0 || xi[2] != 0.0 || xi[3] != 0.0 || xi[4] != 0.0 || xi[5] != 0.0) {      // a zero step keeps every bit
      const int v = st.first + tid;
      double dR[3][3], S[12];
      rap_rodrigues(xi, dR);
      double* s = p.state + (size_t)v * 12;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double a0 = s[3 * i + 0], a1 = s[3 * i + 1], a2 = s[3 * i + 2];
#pragma unroll
        for (int j = 0; j < 3; ++j) S[3 * i + j] = a0 * dR[j][0] + a1 * dR[j][1] + a2 * dR[j][2] + (i == 3 ? xi[3 + j] : 0.0);
      }
#pragma unroll
      for (int i = 0; i < 12; ++i) s[i] = S[i];
#pragma unroll
      for (int i = 0; i < 9; ++i) p.R[(size_t)v * 9 + i] = (float)S[i];
#pragma unroll
      for (int i = 0; i < 3; ++i) p.T[(size_t)v * 3 + i] = (float)S[9 + i];
    }
  }
  if (tid == 0) {
    const double rmse = sqrt(fmax(sh->tot_err / (double)cnt, 0.0));
    icp_finish_end(sc, p.it, rmse, p.rel_thr, p.rmse, p.iterations, p.converged, p.prev, p.done);
  }
}

extern "C" size_t rap_scene_refine_workspace_bytes(int64_t n_points, int32_t V, int32_t S, int32_t E, int64_t row_budget, int32_t max_views) {
  if (n_points <= 0 || n_points > 0x7fffffffLL / 8 || V <= 0 || V > 65535 || S <= 0 || E <= 0 || E > 65535 || row_budget <= 0 ||
      row_budget / NN_TILE > 0x7fffffffLL / 64 || max_views < 2 || max_views > SCENE_MAX_VIEWS)
    return 0;
  return scene_carve(nullptr, n_points, V, S, E, row_budget).total;
}

extern "C" int rap_scene_refine(const float* P, const float* normals, const int32_t* view_seg, int32_t V, int64_t n_points,
                                const int32_t* scene_seg, int32_t S, const int32_t* edges, int32_t E, int64_t row_budget, int32_t max_views,
                                const uint8_t* fixed, const float* init_R, const float* init_T, int32_t max_iterations,
                                float relative_rmse_thr, float max_correspondence_distance, float* R, float* T, float* rmse,
                                int32_t* iterations, uint8_t* converged, float* edge_rmse, int32_t* edge_count, void* ws, size_t ws_bytes,
                                void* stream_) {
  if (!P || !normals || !view_seg || !scene_seg || !edges || !R || !T || !rmse || !iterations || !converged || n_points <= 0 ||
      n_points > 0x7fffffffLL / 8 || V <= 0 || V > 65535 || S <= 0 || E <= 0 || E > 65535 || row_budget <= 0 ||
      row_budget / NN_TILE > 0x7fffffffLL / 64 || max_views < 2 || max_views > SCENE_MAX_VIEWS || max_iterations <= 0 ||
      relative_rmse_thr != relative_rmse_thr || max_correspondence_distance != max_correspondence_distance)
    return RAP_ERR_INVALID;
  if (!ws) return RAP_ERR_WORKSPACE;
  const SceneWs w = scene_carve(ws, n_points, V, S, E, row_budget);
  if (w.total > ws_bytes) return RAP_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  const int max_items = (int)scene_max_items(row_budget, E);
  const float gate = max_correspondence_distance > 0.f ? max_correspondence_distance : 0.f;
  hipLaunchKernelGGL(scene_setup_kernel, dim3(1), dim3(256), 0, stream, view_seg, V, (long)n_points, scene_seg, S, edges, E, (long)row_budget,
                     max_views, fixed, init_R, init_T, max_items, w, R, T, rmse, iterations, converged, edge_rmse, edge_count);
  RAP_LAUNCH_CHECK();
  int rc = launch_nn_grid_build(stream, P, view_seg, V, (long)n_points, w.grid);
  if (rc) return rc;
  const int lds = (int)scene_lds_bytes(max_views);
  for (int it = 0; it < max_iterations; ++it) {
    hipLaunchKernelGGL(scene_edge_pose_kernel, dim3((E + 255) / 256), dim3(256), 0, stream, (const SceneEdge*)w.edges,
                       (const int32_t*)w.edge_scene, E, (const double*)w.state, (const int32_t*)w.done, w.edge_R, w.edge_T, w.edone);
    RAP_LAUNCH_CHECK();
    hipLaunchKernelGGL(scene_query_kernel, dim3((unsigned)max_items), dim3(ICP_TILE), 0, stream, P, normals, (const NnWork*)w.items,
                       (const float*)w.edge_R, (const float*)w.edge_T, (const int32_t*)w.edone, gate, (const NnGrid*)w.grid.grids,
                       (const unsigned*)w.grid.cell_start, (const float4*)w.grid.sorted, w.partials);
    RAP_LAUNCH_CHECK();
    hipLaunchKernelGGL(scene_edge_kernel, dim3(E), dim3(64), 0, stream, (const IcpPlanePartial*)w.partials, (const SceneEdge*)w.edges,
                       (const int32_t*)w.edone, (const double*)w.state, w.edge_mom, w.edge_w, edge_rmse, edge_count);
    RAP_LAUNCH_CHECK();
    const SceneSolveArgs a = {w.scenes, w.views, w.edges, w.edge_order, w.edge_mom, w.edge_w, w.state, R, T, rmse, iterations, converged,
                              w.prev, w.done, it, (double)relative_rmse_thr};
    rc = rap_launch_dyn_lds(scene_solve_kernel, dim3(S), dim3(SCENE_THREADS), lds, stream, a);
    if (rc) return rc;
  }
  return RAP_OK;
}
