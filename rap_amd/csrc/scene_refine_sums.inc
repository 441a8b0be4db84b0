// The two kernels of rap_scene_refine that read the moment partials, included by scene_refine.hip once per partial type:
// SCENE_EDGE_KERNEL / SCENE_SOLVE_KERNEL = their names, SCENE_PARTIAL = IcpPlanePartial with SCENE_SHARED = SceneShared (rap_scene_refine),
// or IcpPlaneWPartial with SceneSharedW (rap_scene_refine_robust: weighted sums, e = sum 2 rho, W carried; the solve also totals W and
// stops a scene whose every weight is zero).  SCENE_IF_WEIGHTED(statements): those of the robust call only.  A textual include and not
// a template: as functions called from two kernels the plain kernels get another register allocation than they had.
#define SCENE_MOM(p, e) (((const SCENE_PARTIAL*)(p).edge_mom)[e])

__global__ __launch_bounds__(64) void SCENE_EDGE_KERNEL(const SCENE_PARTIAL* __restrict__ partials, const SceneEdge* __restrict__ edges,
                                                        const int32_t* __restrict__ edone, const double* __restrict__ state,
                                                        SCENE_PARTIAL* __restrict__ edge_mom, double* __restrict__ edge_w,
                                                        float* __restrict__ edge_rmse, int32_t* __restrict__ edge_count) {
  __shared__ double sA[36], sM[36], sb[6];
  const int e = blockIdx.x;
  if (edone[e]) return;
  const SceneEdge r = edges[e];
  ICP_SUM_PARTIALS(SCENE_PARTIAL::NRED, SCENE_PARTIAL, partials, r, m, n);
  const int t = threadIdx.x;
  if (t == 0) {
    SCENE_PARTIAL* o = edge_mom + e;
#pragma unroll
    for (int i = 0; i < SCENE_PARTIAL::NRED; ++i) o->m[i] = m[i];
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

__global__ __launch_bounds__(SCENE_THREADS) void SCENE_SOLVE_KERNEL(SceneSolveArgs p) {
  extern __shared__ __align__(16) unsigned char scene_lds[];
  const int sc = blockIdx.x;
  if (p.done[sc]) return;
  SCENE_SHARED* sh = (SCENE_SHARED*)scene_lds;
  double* mem = (double*)(scene_lds + ((sizeof(SCENE_SHARED) + 15) / 16) * 16);
  const int tid = threadIdx.x;
  const SceneTab st = p.scenes[sc];
  if (tid == 0) {
    int nf = 0;
    for (int l = 0; l < st.count; ++l) sh->slot[l] = p.views[st.first + l].fixed ? -1 : nf++;
    sh->n = 6 * nf;
    sh->tot_err = 0.0;
    sh->tot_n = 0;
    SCENE_IF_WEIGHTED(sh->tot_w = 0.0;)
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
      const long long ne = SCENE_MOM(p, e).count;
      sh->chunk_e[tid] = e;
      sh->chunk_n[tid] = (int)ne;
      sh->chunk_err[tid] = SCENE_MOM(p, e).m[27];
      SCENE_IF_WEIGHTED(sh->chunk_w[tid] = SCENE_MOM(p, e).m[ICP_PLANE_NMOM];)
      sh->chunk_a[tid] = (short)sh->slot[se.a - st.first];
      sh->chunk_b[tid] = (short)sh->slot[se.b - st.first];
    }
    __syncthreads();
    if (tid == 0) {
      double err = sh->tot_err;
      long long cnt = sh->tot_n;
      for (int c = 0; c < nc; ++c) { err += sh->chunk_err[c]; cnt += sh->chunk_n[c]; }
      sh->tot_err = err; sh->tot_n = cnt;
      SCENE_IF_WEIGHTED(double tw = sh->tot_w; for (int c = 0; c < nc; ++c) tw += sh->chunk_w[c]; sh->tot_w = tw;)
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
  bool none = cnt == 0;                              // no pair with a usable normal in the whole scene: stop with the poses it had
  SCENE_IF_WEIGHTED(none = none || sh->tot_w == 0.0;)      // ... or none with a weight
  if (none) {
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

#undef SCENE_MOM
