// Consistent orientation of the normals of packed clouds: the minimum spanning forest of the Riemannian graph (Hoppe et al. 1992, Open3D's
// orient_normals_consistent_tangent_plane as the reference calls it after its plane fit, dataset_process/utils/dataset_utils.py:325-358),
// restated so that the result is a pure function of integers and signs.  include/rapflow.h (rap_orient_normals) has the semantics,
// DESIGN.md section 7.8 the arguments; this is how it is computed.
//
// Graph.  The vertices are the rows with finite coordinates and a finite non-zero normal.  The k-best walk of nn_knn.hip writes every
// row's k nearest rows of its own segment (itself included) into the workspace; slot (i, s) holding row j is an edge {i, j} when both are
// vertices and i != j.  An edge that sits in both ends' lists is simply met twice.  Its weight is w = 1 - |d|, d = orient_dot of the two
// input normals, and edges are ordered by (w, lo, hi), lo < hi its rows: a total order, so the minimum spanning forest is unique and
// every way of computing it gives the same tree.
//
// Forest: Boruvka rounds, every step its own launch (no kernel waits for another block).  `lab` holds for every vertex its component's
// root and its sign relative to that root, packed as root << 1 | parity, flat at the start of a round.
//   orient_offer_kernel<0>  every live slot whose ends lie in different components offers (key(w) << 32 | lo) to both components: integer
//                           64-bit atomicMin into best[root].  A slot whose ends share a component is dead for good and is struck out
//   orient_offer_kernel<1>  the slots that tie a component's winning (w, lo) settle hi: atomicMin into besthi[root]
//   orient_hook_kernel      every root with a winning edge hooks onto the root at its other end: ptr[root] = other << 1 | parity, the
//                           parity of u -> root_u, of the edge (d < 0) and of v -> root_v composed.  When two roots won the SAME edge the
//                           lower one stays root.  Under a total order these pairs are the only cycles of the "won edge" relation
//   orient_jump_kernel      pointer jumping on ptr, in place: a word is always a true (ancestor, parity to it) pair, so a reader that
//                           meets a half-finished neighbour composes a shorter but correct hop, and a launch at least doubles what
//                           every pointer spans.  The last launch of a round copies ptr into lab and clears the offers; a launch
//                           that follows one in which no pointer moved has nothing to do and leaves
// Because the parity travels with the union-find and a tree path is unique, no traversal of the tree follows, and its depth never
// enters: a chain of n points costs the same launches as a ball of n points.
// Counts.  A component that can still grow merges with at least one other per round, so at most n >> t such components start round t:
// floor(log2 n) rounds, and ceil(log2 (n >> t)) jump launches (at least one) after the hooks of round t.  Both are host arithmetic in
// n_points, so the call is capturable; a round that finds the previous round's `hooked` flag clear leaves at its first instruction.
//
// Seed and write.  orient_seed_kernel: integer atomicMax of key(z) << 32 | ~row into the root's slot: the largest z, the lowest row
// among equals.  orient_seed_sign_kernel: the seed decides its own sign (n_z < 0, or the viewpoint rule of normals.hip) and leaves
// sign ^ its parity with the root.  orient_write_kernel: every vertex flips its sign bits when parity(v) ^ that word is set.
// No loop here is longer than four steps or than the slots of a block's rows; no floating-point atomics; the integer minima and maxima do
// not depend on arrival order, so the bits are the same from call to call and for a segment whatever else is in the batch.
#include "nn_grid.h"

#define ORI_TILE NN_TILE
#define ORI_NONE 0xffffffffu      // lab / ptr of a row that is no vertex
#define ORI_JUMPS 4               // hops a thread tries per jump launch; the launch counts rely on the first one only
#define ORI_ROUNDS 32             // more than the rounds of 2^28 rows, and than the jump launches of a round

struct OrientParams {
  const float* P;
  const NnWork* items;
  const float* viewpoint;     // (K,3) or null
  float* normals;
  int32_t* component_out;     // (n_points) or null
  int32_t* idx;               // (n_points, k): the neighbour lists, -1 where a slot gives no (live) edge
  unsigned* wkey;             // (n_points, k): key(w) of every edge slot
  unsigned* lab;              // the flat labels of the round
  unsigned* ptr;              // the labels being hooked and flattened
  unsigned long long* best;   // per root: the smallest key(w) << 32 | lo offered
  unsigned* besthi;           // per root: the smallest hi among the offers that tie best; at the end the seed's word
  unsigned long long* seed;   // per root: the largest key(z) << 32 | ~row
  int32_t* flags;             // flags[t]: a root hooked in round t; flags[32 + 32 t + j]: jump launch j of round t moved a pointer
  int k;
};

OrientWs orient_carve(Carver& c, long N, int K) {
  OrientWs w;
  w.items = (NnWork*)c.take(nn_max_items(N, K) * sizeof(NnWork));
  w.repeat = (int32_t*)c.take((size_t)K * 4);
  w.g = nn_grid_carve(c, N, K);
  w.idx = (int32_t*)c.take((size_t)N * 32 * 4);
  w.wkey = (unsigned*)c.take((size_t)N * 32 * 4);
  w.count = (int32_t*)c.take((size_t)N * 4);
  w.lab = (unsigned*)c.take((size_t)N * 4);
  w.ptr = (unsigned*)c.take((size_t)N * 4);
  w.best = (unsigned long long*)c.take((size_t)N * 8);
  w.besthi = (unsigned*)c.take((size_t)N * 4);
  w.seed = (unsigned long long*)c.take((size_t)N * 8);
  w.flags = (int32_t*)c.take((ORI_ROUNDS + ORI_ROUNDS * ORI_ROUNDS) * 4);
  return w;
}

// the ONE expression for d: the x product rounded, y and z fused onto it.  Products commute, so both ends get the same bits
__device__ __forceinline__ float orient_dot(const float* __restrict__ a, const float* __restrict__ b) {
  return __fmaf_rn(a[2], b[2], __fmaf_rn(a[1], b[1], a[0] * b[0]));
}
// order-preserving map of a float onto unsigned integers (nn_grid.hip's grid_key)
__device__ __forceinline__ unsigned orient_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// the rows of this block's item: false when there are none
__device__ __forceinline__ bool orient_item(const OrientParams& a, size_t& base, int& rows) {
  const NnWork w = a.items[blockIdx.x];
  if (w.x_len <= 0) return false;
  base = (size_t)w.x_start + w.q0;
  rows = min(ORI_TILE, w.x_len - w.q0);
  return true;
}

__global__ __launch_bounds__(ORI_TILE) void orient_init_kernel(const OrientParams a) {
  if (blockIdx.x == 0)
    for (int t = threadIdx.x; t < ORI_ROUNDS + ORI_ROUNDS * ORI_ROUNDS; t += ORI_TILE) a.flags[t] = 0;
  size_t base; int rows;
  if (!orient_item(a, base, rows) || (int)threadIdx.x >= rows) return;
  const size_t row = base + threadIdx.x;
  const float* p = a.P + row * 3;
  const float* n = a.normals + row * 3;
  const bool vertex = grid_finite(p[0], p[1], p[2]) && grid_finite(n[0], n[1], n[2]) && (n[0] != 0.f || n[1] != 0.f || n[2] != 0.f);
  const unsigned self = vertex ? (unsigned)row << 1 : ORI_NONE;
  a.lab[row] = self; a.ptr[row] = self;
  a.best[row] = ~0ull; a.besthi[row] = ~0u; a.seed[row] = 0ull;
}

// slot by slot: the lists of a block's rows are one contiguous run of rows * k entries
__global__ __launch_bounds__(ORI_TILE) void orient_edges_kernel(const OrientParams a) {
  size_t base; int rows;
  if (!orient_item(a, base, rows)) return;
  const int k = a.k, n = rows * k;
  for (int e = threadIdx.x; e < n; e += ORI_TILE) {
    const size_t row = base + e / k, slot = base * k + e;
    const int j = a.idx[slot];
    if (j < 0) continue;
    if ((size_t)j == row || a.lab[row] == ORI_NONE || a.lab[j] == ORI_NONE) { a.idx[slot] = -1; continue; }
    const float d = orient_dot(a.normals + row * 3, a.normals + (size_t)j * 3);
    a.wkey[slot] = orient_key(1.f - fabsf(d));
  }
}

template <bool HI>
__global__ __launch_bounds__(ORI_TILE) void orient_offer_kernel(const OrientParams a, int round) {
  if (round > 0 && a.flags[round - 1] == 0) return;
  size_t base; int rows;
  if (!orient_item(a, base, rows)) return;
  const int k = a.k, n = rows * k;
  for (int e = threadIdx.x; e < n; e += ORI_TILE) {
    const size_t row = base + e / k, slot = base * k + e;
    const int j = a.idx[slot];
    if (j < 0) continue;
    const unsigned ri = a.lab[row] >> 1, rj = a.lab[j] >> 1;
    if (ri == rj) { if (!HI) a.idx[slot] = -1; continue; }
    const unsigned lo = min((unsigned)row, (unsigned)j), hi = max((unsigned)row, (unsigned)j);
    const unsigned long long key = ((unsigned long long)a.wkey[slot] << 32) | lo;
    if (!HI) {                                                         // best only falls: a stale read costs an atomic, never a miss
      if (key < a.best[ri]) atomicMin(&a.best[ri], key);
      if (key < a.best[rj]) atomicMin(&a.best[rj], key);
    } else {
      if (key == a.best[ri] && hi < a.besthi[ri]) atomicMin(&a.besthi[ri], hi);
      if (key == a.best[rj] && hi < a.besthi[rj]) atomicMin(&a.besthi[rj], hi);
    }
  }
}

__global__ __launch_bounds__(ORI_TILE) void orient_hook_kernel(const OrientParams a, int round) {
  if (round > 0 && a.flags[round - 1] == 0) return;
  size_t base; int rows;
  if (!orient_item(a, base, rows) || (int)threadIdx.x >= rows) return;
  const unsigned v = (unsigned)(base + threadIdx.x);
  if (a.lab[v] != v << 1) return;                                      // roots only (a root's parity is 0)
  const unsigned long long key = a.best[v];
  if (key == ~0ull) return;
  const unsigned lo = (unsigned)key, hi = a.besthi[v];
  if (hi == ~0u) return;                                               // cannot happen: the slot that won (w, lo) offers its hi
  const unsigned ll = a.lab[lo], lh = a.lab[hi];
  const unsigned other = (ll >> 1) == v ? lh >> 1 : ll >> 1;
  if (a.best[other] == key && a.besthi[other] == hi && v < other) return;      // both won this edge: the lower root stays
  const unsigned flip = orient_dot(a.normals + (size_t)lo * 3, a.normals + (size_t)hi * 3) < 0.f ? 1u : 0u;
  a.ptr[v] = other << 1 | ((ll ^ lh ^ flip) & 1u);
  a.flags[round] = 1;
}

__global__ __launch_bounds__(ORI_TILE) void orient_jump_kernel(const OrientParams a, int round, int step, int last) {
  if ((round > 0 && a.flags[round - 1] == 0) || a.flags[round] == 0) return;      // no hook in this round: no offer either, lab is current
  int32_t* moved = a.flags + ORI_ROUNDS + round * ORI_ROUNDS;
  const bool flat = step > 0 && moved[step - 1] == 0;                  // a launch in which nothing moved saw every pointer at a root
  if (flat && !last) return;
  size_t base; int rows;
  if (!orient_item(a, base, rows) || (int)threadIdx.x >= rows) return;
  const size_t row = base + threadIdx.x;
  unsigned w = a.ptr[row];
  if (w != ORI_NONE && !flat) {
    bool hop = false;
    for (int it = 0; it < ORI_JUMPS; ++it) {
      const unsigned up = a.ptr[w >> 1];
      if (up >> 1 == w >> 1) break;                                    // w points at a root
      w = (up & ~1u) | ((w ^ up) & 1u);
      hop = true;
    }
    if (hop) { a.ptr[row] = w; moved[step] = 1; }
  }
  if (last) { a.lab[row] = w; a.best[row] = ~0ull; a.besthi[row] = ~0u; }
}

// one atomic per wave where the wave's vertices share a root (the usual case: a block's rows are neighbours in the array), one per
// vertex otherwise; a plain read first either way (the word only rises)
__global__ __launch_bounds__(ORI_TILE) void orient_seed_kernel(const OrientParams a) {
  size_t base = 0; int rows = 0;
  const bool item = orient_item(a, base, rows);
  const size_t row = base + threadIdx.x;
  const unsigned w = item && (int)threadIdx.x < rows ? a.lab[row] : ORI_NONE;
  const bool vertex = w != ORI_NONE;
  const unsigned root = w >> 1;
  unsigned long long key = 0ull;
  if (vertex) key = ((unsigned long long)orient_key(a.P[row * 3 + 2] + 0.f) << 32) | (0xffffffffu - (unsigned)row);      // -0 is 0
  const unsigned long long mask = __ballot(vertex);
  if (mask == 0ull) return;
  const int leader = __ffsll((long long)mask) - 1;
  const unsigned root0 = (unsigned)__shfl((int)root, leader, 64);
  if (__all(!vertex || root == root0)) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long other = __shfl_xor(key, o, 64);
      key = other > key ? other : key;
    }
    if ((int)(threadIdx.x & 63) == leader && key > a.seed[root0]) atomicMax(&a.seed[root0], key);
  } else if (vertex && key > a.seed[root]) {
    atomicMax(&a.seed[root], key);
  }
}

__global__ __launch_bounds__(ORI_TILE) void orient_seed_sign_kernel(const OrientParams a) {
  size_t base; int rows;
  if (!orient_item(a, base, rows) || (int)threadIdx.x >= rows) return;
  const size_t row = base + threadIdx.x;
  const unsigned w = a.lab[row];
  if (w == ORI_NONE || 0xffffffffu - (unsigned)a.seed[w >> 1] != (unsigned)row) return;
  const float* n = a.normals + row * 3;
  bool flip;
  if (a.viewpoint) {                                                   // normals.hip's test, on the fp32 normal
    const float* v = a.viewpoint + (size_t)a.items[blockIdx.x].pad0 * 3;
    const float* p = a.P + row * 3;
    flip = (double)n[0] * ((double)v[0] - (double)p[0]) + (double)n[1] * ((double)v[1] - (double)p[1]) +
           (double)n[2] * ((double)v[2] - (double)p[2]) < 0.0;
  } else {
    flip = n[2] < 0.f;
  }
  a.besthi[w >> 1] = (flip ? 1u : 0u) ^ (w & 1u);
}

__global__ __launch_bounds__(ORI_TILE) void orient_write_kernel(const OrientParams a) {
  size_t base; int rows;
  if (!orient_item(a, base, rows) || (int)threadIdx.x >= rows) return;
  const size_t row = base + threadIdx.x;
  const unsigned w = a.lab[row];
  if (w == ORI_NONE) {
    if (a.component_out) a.component_out[row] = -1;
    return;
  }
  if ((w ^ a.besthi[w >> 1]) & 1u) {
    unsigned* n = (unsigned*)(a.normals + row * 3);
    n[0] ^= 0x80000000u; n[1] ^= 0x80000000u; n[2] ^= 0x80000000u;
  }
  if (a.component_out) a.component_out[row] = (int32_t)(0xffffffffu - (unsigned)a.seed[w >> 1]);
}

static int orient_log2_ceil(long n) { int b = 0; while ((1L << b) < n) ++b; return b; }

int orient_rounds(long N) { int r = 0; while ((N >> r) >= 2) ++r; return r; }
int orient_jumps(long N, int round) { const int j = orient_log2_ceil(N >> round); return j < 1 ? 1 : j; }

int launch_orient_normals(hipStream_t stream, const float* P, const int32_t* seg, int K, long N, int k, const float* viewpoint, float* normals,
                          int32_t* component_out, const OrientWs& w) {
  int rc = launch_knn_self_rows(stream, P, seg, K, N, k, w.idx, (float*)w.wkey, w.count, w.items, w.repeat, w.g);
  if (rc) return rc;
  OrientParams a;
  a.P = P; a.items = w.items; a.viewpoint = viewpoint; a.normals = normals; a.component_out = component_out;
  a.idx = w.idx; a.wkey = w.wkey; a.lab = w.lab; a.ptr = w.ptr; a.best = w.best; a.besthi = w.besthi; a.seed = w.seed; a.flags = w.flags;
  a.k = k;
  const dim3 grid((unsigned)nn_max_items(N, K)), block(ORI_TILE);
  hipLaunchKernelGGL(orient_init_kernel, grid, block, 0, stream, a);
  RAP_LAUNCH_CHECK();
  hipLaunchKernelGGL(orient_edges_kernel, grid, block, 0, stream, a);
  RAP_LAUNCH_CHECK();
  const int rounds = orient_rounds(N);
  for (int t = 0; t < rounds; ++t) {
    hipLaunchKernelGGL(orient_offer_kernel<false>, grid, block, 0, stream, a, t);
    RAP_LAUNCH_CHECK();
    hipLaunchKernelGGL(orient_offer_kernel<true>, grid, block, 0, stream, a, t);
    RAP_LAUNCH_CHECK();
    hipLaunchKernelGGL(orient_hook_kernel, grid, block, 0, stream, a, t);
    RAP_LAUNCH_CHECK();
    const int jumps = orient_jumps(N, t);
    for (int j = 0; j < jumps; ++j) {
      hipLaunchKernelGGL(orient_jump_kernel, grid, block, 0, stream, a, t, j, j == jumps - 1 ? 1 : 0);
      RAP_LAUNCH_CHECK();
    }
  }
  hipLaunchKernelGGL(orient_seed_kernel, grid, block, 0, stream, a);
  RAP_LAUNCH_CHECK();
  hipLaunchKernelGGL(orient_seed_sign_kernel, grid, block, 0, stream, a);
  RAP_LAUNCH_CHECK();
  hipLaunchKernelGGL(orient_write_kernel, grid, block, 0, stream, a);
  RAP_LAUNCH_CHECK();
  return RAP_OK;
}
