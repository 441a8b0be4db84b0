// C ABI of librapflow (see include/rapflow.h): model packing, workspace carving and the launch
// sequences of one velocity-network forward and of the whole Euler sampling loop.  Host code only;
// every kernel lives in the sibling .hip files, the kernel-level and metric / preprocessing entry points in api_ops.hip.
#include "../../include/rapflow.h"
#include "half.h"
#include "kernels.h"

#include <mutex>
#include <new>
#include <vector>

static thread_local int g_last_hip_error = 0;
void rap_set_last_hip_error(int e) { g_last_hip_error = e; }

// ---------------------------------------------------------------------------------------------
// optional per-kernel-class timing with HIP events on the launch stream (bench.py's roofline leg).
// Off by default; when on, every attention / GEMM launch of forward_step is bracketed by two events.
// ---------------------------------------------------------------------------------------------
// classes: 0 = attention per part, 1 = attention per sample, 2 = layer GEMMs (the MFMA-bound kernels), and since round 5 the HBM-bound
// ring: 3 = LayerNorm, 4 = posenc(x_t), 5 = Euler update, 6 = Procrustes moments + solve, 7 = rigid apply / blend
#define RAP_PROF_CLASSES 8
struct ProfRec { hipEvent_t a, b; int cls; };
// process-global state behind one mutex (round 5: the enable flag was a plain bool and the vectors unsynchronised): two
// threads enqueueing on two models may record concurrently; the flag is an atomic so that the off path costs one relaxed load
static std::atomic<bool> g_prof_on{false};
static std::mutex g_prof_mu;
static std::vector<ProfRec> g_prof_recs;
static std::vector<hipEvent_t> g_prof_pool;
static size_t g_prof_pool_used = 0;
static const size_t RAP_PROF_MAX_EVENTS = 1u << 19;   // 20 sample calls of rap_12 at 20 flow steps = 38 400 scopes = 76 800 events (r01: 32768 truncated the log)

static hipEvent_t prof_event() {      // caller holds g_prof_mu
  if (g_prof_pool_used < g_prof_pool.size()) return g_prof_pool[g_prof_pool_used++];
  if (g_prof_pool.size() >= RAP_PROF_MAX_EVENTS) return nullptr;
  hipEvent_t e = nullptr;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  g_prof_pool.push_back(e);
  g_prof_pool_used++;
  return e;
}
struct ProfScope {
  hipStream_t s; hipEvent_t a = nullptr, b = nullptr; int cls;
  ProfScope(hipStream_t s_, int cls_) : s(s_), cls(cls_) {
    if (!g_prof_on.load(std::memory_order_relaxed)) return;
    std::lock_guard<std::mutex> lock(g_prof_mu);
    a = prof_event(); b = prof_event();
    if (a && b) (void)hipEventRecord(a, s); else a = b = nullptr;
  }
  ~ProfScope() {
    if (a && b) {
      std::lock_guard<std::mutex> lock(g_prof_mu);
      (void)hipEventRecord(b, s); g_prof_recs.push_back({a, b, cls});
    }
  }
};
extern "C" int rap_profile_enable(int on) { g_prof_on.store(on != 0); return RAP_OK; }
extern "C" int rap_profile_reset(void) { std::lock_guard<std::mutex> lock(g_prof_mu); g_prof_recs.clear(); g_prof_pool_used = 0; return RAP_OK; }
// Synchronises on the recorded events.  h_ms_out / h_count_out have n_classes entries (classes >= n_classes are dropped).
extern "C" int rap_profile_collect_ex(float* h_ms_out, int64_t* h_count_out, int32_t n_classes) {
  if (!h_ms_out || !h_count_out || n_classes <= 0) return RAP_ERR_INVALID;
  std::lock_guard<std::mutex> lock(g_prof_mu);
  for (int c = 0; c < n_classes; ++c) { h_ms_out[c] = 0.f; h_count_out[c] = 0; }
  for (const ProfRec& r : g_prof_recs) {
    if (r.cls >= n_classes) continue;
    if (hipEventSynchronize(r.b) != hipSuccess) return RAP_ERR_HIP;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) return RAP_ERR_HIP;
    h_ms_out[r.cls] += ms; h_count_out[r.cls] += 1;
  }
  return RAP_OK;
}
// the three MFMA-bound classes (ABI <= 4 form)
extern "C" int rap_profile_collect(float* h_ms_out, int64_t* h_count_out) { return rap_profile_collect_ex(h_ms_out, h_count_out, 3); }

// ---------------------------------------------------------------------------------------------
// model
// ---------------------------------------------------------------------------------------------
struct LayerW {
  const float* Wqkv[2];   // (3d,d)  [0]=self (per part), [1]=global (per sample)
  const float* Wout[2];   // (d,d)
  const float* bout[2];   // (d)
  const float* gq[2];     // (H,64)
  const float* gk[2];
  const float* ffn_g;     // (d)
  const float* ffn_b;
  const float* Wff1p;     // (8d,d) value/gate interleaved
  const float* bff1p;     // (8d)
  const float* Wff2;      // (d,4d)
  const float* bff2;      // (d)
};

// 16-bit copies of the transformer-block GEMM weights (one set per reduced-precision dtype, built on demand)
struct LayerWH {
  const u16* Wqkv[2];
  const u16* Wout[2];
  const u16* Wff1p;   // value/gate interleaved, as the fp32 packing
  const u16* Wff2;
  // split precision (RAP_DT_F32X2): the planes hold w * 2^e per tensor; s_* = 2^-e, the factor the epilogue applies to the accumulators
  float s_qkv[2] = {1.f, 1.f}, s_out[2] = {1.f, 1.f}, s_ff1 = 1.f, s_ff2 = 1.f;
  // ... and the powers of two the ACTIVATIONS those weights produce are stored with (round 6, GemmParamsH::out_scale): g_v for the V^T image
  // (2^(e_qkv - 16): 1 for a tensor whose largest weight lies in (2^-5, 2^-4], the nn.Linear default range at d = 512), g_ff1 for the GEGLU
  // output (value x gate: 2^(2 (e_ff1 - 16))).  The consuming GEMM (out-projection, ff2) divides its accumulator scale by it (exact).
  float g_v[2] = {1.f, 1.f}, g_ff1 = 1.f;
};
struct HalfWeights {
  u16* blob = nullptr;
  std::vector<LayerWH> layers;
};
#define RAP_MAX_LOGIT_BOUND 40.0f   // exp(-2*40) is still a normal fp32 / bf16 number

struct rap_model {
  rap_model_desc desc;
  int d, L, H, F, E;
  int Din = 0;                // in_dim: width of the latent point features concatenated into the embedding (embedding.py:163-166; 0 in every shipped config)
  int Ks = 128;               // columns of the step-invariant embedding input: 128 + align_up(Din, 32)
  int dtype = RAP_DT_F32;     // arithmetic type of the transformer blocks (rap_model_set_compute_dtype)
  bool qk_norm = true;        // MultiHeadRMSNorm on q / k (rap_model_set_qk_norm; every shipped configuration has it on)
  int resid_dtype = RAP_DT_F32;   // storage type of the residual stream in the 16-bit modes (rap_model_set_residual_dtype): fp32 or fp16
  float softcap = 0.f;        // > 0: every attention logit s becomes softcap * tanh(s / softcap) (rap_model_set_softcap); 0 = off
  int final_act = 0;          // activation of the head's hidden layers (rap_model_set_final_act): 0 SiLU, 1 GELU (erf), 2 ReLU
  HalfWeights half[4];        // indexed by dtype (slot 0 unused; 3 = the paired head / tail planes of the split-precision mode)
  float* logit_bound = nullptr;   // (L, 2, H) per-head bounds on q.k/8 after qk-norm; null until a 16-bit dtype is selected
  // bounded[2 * layer + branch]: every head of THAT attention has a bound <= RAP_MAX_LOGIT_BOUND, so that launch may use the
  // bounded (offset-free) softmax kernel; the others take the online-softmax kernel.  Decided per launch since round 3 (VERDICT
  // r02 item 4): one hot head in a trained checkpoint costs its own (layer, branch) the fast kernel, not the whole model.
  std::vector<uint8_t> bounded;
  int n_bounded = 0;
  float* raw = nullptr;       // copy of the caller's blob
  float* derived = nullptr;   // packed arrays
  const float* anchor_emb;    // (2,d)
  const float* emb_bias;      // (d)
  const float* Wstatic;       // (d,Ks): [cond PE63 | scale PE21 | feat F | 0 .. 128 | latent Din | 0]
  const float* Wx;            // (d,64):  [x_t PE63 | 0]
  const float *adaW1, *adab1, *adaW2, *adab2, *adaW3, *adab3;  // stacked over j = 2*layer + {0 self, 1 global}
  std::vector<LayerW> layers;
  const float *hW0, *hb0, *hW2, *hb2, *hW4;
  // Configuration (compute / residual dtype) is read on the HOST while a call is being enqueued (workspace layout, kernel choice):
  // the setters and the enqueueing entry points take this mutex, so a setter on one thread cannot change the layout of a call another
  // thread is in the middle of enqueueing.  Work that is already enqueued is not affected by a later change.
  mutable std::mutex cfg_mu;
};

static bool desc_ok(const rap_model_desc* d) {
  if (!d) return false;
  if (d->embed_dim <= 0 || d->embed_dim % 256 != 0 || d->embed_dim > 1024) return false;
  if (d->num_heads * 64 != d->embed_dim) return false;
  if (d->num_layers <= 0 || d->num_layers > 64) return false;
  if (d->local_feat_dim < 0 || d->local_feat_dim % 4 != 0 || d->local_feat_dim > 40) return false;
  return true;
}

extern rap_tuning_t g_rap_gemm_variant;   // gemm_f32.hip
extern rap_tuning_t g_rap_gemm_stagger;   // gemm_f32.hip
extern rap_tuning_t g_rap_gemm_splitk;    // gemm_f32.hip
extern rap_tuning_t g_rap_geglu_fast;     // gemm_f32.hip
extern rap_tuning_t g_rap_attn_split;     // attn_f32.hip
extern rap_tuning_t g_rap_gemm_h16_variant;   // gemm_h16.hip
extern rap_tuning_t g_rap_attn_h16_variant;   // attn_h16.hip
extern rap_tuning_t g_rap_gemm_h16_persistent;   // gemm_h16.hip
extern rap_tuning_t g_rap_attn_h16_dma;          // attn_h16.hip
extern rap_tuning_t g_rap_gemm_f32_persistent;   // gemm_f32.hip
extern rap_tuning_t g_rap_attn_x2_wpe;           // attn_x2.hip
extern rap_tuning_t g_rap_attn_h16_small;        // attn_h16.hip, tuning key 20
extern rap_tuning_t g_rap_fps_grid_per, g_rap_fps_grid_block;      // fps_grid.hip, tuning keys 22 and 23
rap_tuning_t g_rap_attn_lpt = 1;               // tuning key 15: attention work lists longest-segment-first (1, default) or in segment order (0)
// tuning key 17: split precision takes over from this many token rows (align_up(TP, 256)) per call; SMALLER calls of a model in compute
// dtype 3 run the exact-fp32 kernels -- both are fp32-accurate, and below a few thousand tokens every kernel of a layer sits at the launch
// floor, where the fp32 path's few-token forms (128 x 128 tiles, split-K, split-KV) are the faster ones (r05 call 3: configs[0] geometry,
// one pair of 2 x 1024 points: 48.3 ms fp32 vs 52.6 ms on the 256 x 256-tile split kernels; call 4, one sample of 8 views, 20 steps:
// 1 024 tokens 71 vs 89 ms, 2 048: 92 vs 99, 4 096: 197 vs 124, 8 000: 459 vs 197; call 5, with the residual GEMMs of few-token calls on
// 128 x 128 split-precision tiles: 2 048 tokens 92 vs 81 ms, 2 560: 149 vs 86, 3 072: 169 vs 91; call 9, with every few-token GEMM on
// 128 x 128 tiles, split-K of ff2 and split-KV attention: 1 024 tokens 71 vs 46 ms, 2 048: 92 vs 54, configs[0] geometry 48.4 vs 28.0 ms --
// split precision wins at every size measured; calls below 1 024 rows (not measured) stay on the fp32 kernels).  rap_workspace_bytes of a
// split-precision model covers both layouts, so the key may change between the size query and the call.
rap_tuning_t g_rap_x2_min_rows = 1024;
rap_tuning_t g_rap_small_fused = 1;            // tuning key 19: few-token 16-bit / split-precision calls fold every residual GEMM's combine pass into the following LayerNorm (1, default)
extern rap_tuning_t g_rap_ring_blocks;         // gemm_h16.hip, tuning key 18: launches of the 128 x 128 16-bit GEMM with at most this many blocks take the four-stage ring
rap_tuning_t g_rap_fuse_qknorm = 1;            // tuning key 7: qk-norm fused into the QKV GEMM epilogue (1, default; both precisions) or as its own kernel (0)
// Production switches (process-global, atomics): each selects between two SHIPPED code paths that produce the same result up to
// fp32 summation order -- 5 split-KV for few-token calls (fp32 attention), 6 split-K for few-row calls (fp32 GEMMs and the 16-bit
// residual GEMMs), 7 fused qk-norm, 9 GEGLU's Phi by the
// 1.5e-7 erfc polynomial (1) or erff (0), 11 / 12 persistent 16-bit / fp32 GEMM, 15 the order of the attention work lists (identical results).  Keys 0-4 (kernel-variant A/B of the round-1/2 experiments) exist
// only in a library built with -DRAP_ABLATION_BUILD; the shipped library refuses them.
// One row per key: the values it accepts (n_values < 0: every value >= 0) and the switch it stores them in.
struct TuningRow { int32_t key; rap_tuning_t* var; int n_values; int32_t values[7]; };
static const TuningRow kTuning[] = {
#ifdef RAP_ABLATION_BUILD
  {0, &g_rap_gemm_variant, 3, {16, 32, 48}},
  {2, &g_rap_gemm_h16_variant, 3, {0, 1, 14}},
  {3, &g_rap_attn_h16_variant, 2, {0, 5}},
  {4, &g_rap_gemm_stagger, 3, {0, 1, 2}},
#endif
  {5, &g_rap_attn_split, 2, {0, 1}},
  {6, &g_rap_gemm_splitk, 2, {0, 1}},
  {7, &g_rap_fuse_qknorm, 2, {0, 1}},
  {9, &g_rap_geglu_fast, 2, {0, 1}},
  {11, &g_rap_gemm_h16_persistent, 2, {0, 1}},
  {12, &g_rap_gemm_f32_persistent, 2, {0, 1}},
  {13, &g_rap_attn_h16_dma, 2, {0, 1}},
  {15, &g_rap_attn_lpt, 2, {0, 1}},
  {16, &g_rap_attn_x2_wpe, 2, {2, 4}},           // split-precision attention: 1 / 2 blocks per CU
  {17, &g_rap_x2_min_rows, -1, {}},              // split precision from this many token rows per call (smaller calls: exact fp32)
  {18, &g_rap_ring_blocks, -1, {}},              // four-stage ring of the 128 x 128 16-bit GEMM up to this many blocks per launch (0 = never)
  {19, &g_rap_small_fused, 2, {0, 1}},           // combine + LayerNorm fusion of few-token calls
  {20, &g_rap_attn_h16_small, 7, {0, 1, 2, 64, 128, 66, 130}},   // 16-bit attention of few-token calls: 64 / 128-row work items + four-stage ring
  {22, &g_rap_fps_grid_per, 7, {1, 8, 16, 32, 48, 64, 128}},     // bucket index of farthest point sampling: points per bucket (identical results)
  {23, &g_rap_fps_grid_block, 3, {256, 512, 1024}},              // ... and threads of its one block per cloud (identical results)
};
extern "C" int rap_set_tuning(int32_t key, int32_t value) {
  for (const TuningRow& r : kTuning) {
    if (r.key != key) continue;
    bool ok = r.n_values < 0 && value >= 0;
    for (int i = 0; i < r.n_values; ++i) ok = ok || r.values[i] == value;
    if (ok) *r.var = value;
    return ok ? RAP_OK : RAP_ERR_INVALID;
  }
  return RAP_ERR_INVALID;
}

extern "C" int rap_version(void) { return RAPFLOW_ABI_VERSION; }
extern "C" int rap_last_hip_error(void) { return g_last_hip_error; }

static bool in_dim_ok(int32_t in_dim) { return in_dim >= 0 && in_dim <= 512 && in_dim % 4 == 0; }
extern "C" int64_t rap_weight_count(const rap_model_desc* desc) { return rap_weight_count_latent(desc, 0); }
extern "C" int64_t rap_weight_count_latent(const rap_model_desc* desc, int32_t in_dim) {
  if (!desc_ok(desc) || !in_dim_ok(in_dim)) return -1;
  const int64_t d = desc->embed_dim, L = desc->num_layers, H = desc->num_heads, E = 147 + desc->local_feat_dim + in_dim;
  int64_t n = 2 * d + d * E + d;
  const int64_t attn = (d * 256 + d) + (d * d + d) + (2 * d * d + 2 * d) + 3 * d * d + (d * d + d) + 2 * H * 64;
  const int64_t layer = 2 * attn + 2 * d + (8 * d * d + 8 * d) + (4 * d * d + d);
  n += L * layer;
  n += (d * d + d) + (d / 2 * d + d / 2) + 3 * (d / 2);
  return n;
}

static int ensure_logit_bounds(rap_model* m, hipStream_t stream);

extern "C" int rap_model_create(const rap_model_desc* desc, const float* d_weights, int64_t n_floats, void* stream_,
                                rap_model** out) {
  return rap_model_create_latent(desc, 0, d_weights, n_floats, stream_, out);
}
extern "C" int rap_model_create_latent(const rap_model_desc* desc, int32_t in_dim, const float* d_weights, int64_t n_floats, void* stream_,
                                       rap_model** out) {
  if (!out) return RAP_ERR_INVALID;
  *out = nullptr;
  if (!desc_ok(desc) || !in_dim_ok(in_dim) || !d_weights) return RAP_ERR_INVALID;
  if (n_floats != rap_weight_count_latent(desc, in_dim)) return RAP_ERR_INVALID;
  hipStream_t stream = (hipStream_t)stream_;
  rap_model* m = new (std::nothrow) rap_model();
  if (!m) return RAP_ERR_ALLOC;
  m->desc = *desc;
  const int d = m->d = desc->embed_dim, L = m->L = desc->num_layers, H = m->H = desc->num_heads;
  m->F = desc->local_feat_dim;
  m->Din = in_dim;
  const int Ks = m->Ks = 128 + (in_dim + 31) / 32 * 32;
  const int E = m->E = 147 + m->F + m->Din;      // native column order: [cond 63 | x_t 63 | scale 21 | feat F | latent Din]
  if (hipMalloc((void**)&m->raw, (size_t)n_floats * sizeof(float)) != hipSuccess) { delete m; return RAP_ERR_ALLOC; }
  const size_t n_ada = (size_t)2 * L * ((size_t)d * 256 + d + (size_t)d * d + d + (size_t)2 * d * d + 2 * d);
  const size_t n_ff1 = (size_t)L * ((size_t)8 * d * d + 8 * d);
  const size_t n_derived = (size_t)d * Ks + (size_t)d * 64 + n_ada + n_ff1;
  if (hipMalloc((void**)&m->derived, n_derived * sizeof(float)) != hipSuccess) {
    (void)hipFree(m->raw); delete m; return RAP_ERR_ALLOC;
  }
  int rc = RAP_OK;
  auto fail = [&](int code) { rap_model_destroy(m); return code; };
  if (hipMemcpyAsync(m->raw, d_weights, (size_t)n_floats * sizeof(float), hipMemcpyDeviceToDevice, stream) != hipSuccess)
    return fail(RAP_ERR_HIP);

  // ---- walk the raw blob in state_dict order
  const float* p = m->raw;
  auto take = [&](size_t n) { const float* r = p; p += n; return r; };
  m->anchor_emb = take((size_t)2 * d);
  const float* embW = take((size_t)d * E);
  m->emb_bias = take(d);

  float* q = m->derived;
  auto carve = [&](size_t n) { float* r = q; q += n; return r; };
  float* Wstatic = carve((size_t)d * Ks);
  float* Wx = carve((size_t)d * 64);
  float* aW1 = carve((size_t)2 * L * d * 256); float* ab1 = carve((size_t)2 * L * d);
  float* aW2 = carve((size_t)2 * L * d * d);   float* ab2 = carve((size_t)2 * L * d);
  float* aW3 = carve((size_t)2 * L * 2 * d * d); float* ab3 = carve((size_t)2 * L * 2 * d);
  m->Wstatic = Wstatic; m->Wx = Wx;
  m->adaW1 = aW1; m->adab1 = ab1; m->adaW2 = aW2; m->adab2 = ab2; m->adaW3 = aW3; m->adab3 = ab3;

  // embedding projection columns (embedding.py:161-177): [0,63) cond | [63,126) x_t | [126,147) scale | [147,E) feat
  if ((rc = launch_fill_zero(stream, Wstatic, (size_t)d * Ks))) return fail(rc);
  if ((rc = launch_fill_zero(stream, Wx, (size_t)d * 64))) return fail(rc);
  if ((rc = launch_copy_cols(stream, embW, E, 0, Wstatic, Ks, 0, d, 63))) return fail(rc);
  if ((rc = launch_copy_cols(stream, embW, E, 126, Wstatic, Ks, 63, d, 21))) return fail(rc);
  if ((rc = launch_copy_cols(stream, embW, E, 147, Wstatic, Ks, 84, d, m->F))) return fail(rc);
  if ((rc = launch_copy_cols(stream, embW, E, 147 + m->F, Wstatic, Ks, 128, d, m->Din))) return fail(rc);      // latent columns: one more k-range of the hoisted GEMM
  if ((rc = launch_copy_cols(stream, embW, E, 63, Wx, 64, 0, d, 63))) return fail(rc);

  m->layers.resize(L);
  for (int i = 0; i < L; ++i) {
    LayerW& lw = m->layers[i];
    for (int a = 0; a < 2; ++a) {
      const int j = 2 * i + a;
      const float* W1 = take((size_t)d * 256); const float* b1 = take(d);
      const float* W2 = take((size_t)d * d);   const float* b2 = take(d);
      const float* W3 = take((size_t)2 * d * d); const float* b3 = take((size_t)2 * d);
      if ((rc = launch_copy_cols(stream, W1, 256, 0, aW1 + (size_t)j * d * 256, 256, 0, d, 256))) return fail(rc);
      if ((rc = launch_copy_cols(stream, b1, d, 0, ab1 + (size_t)j * d, d, 0, 1, d))) return fail(rc);
      if ((rc = launch_copy_cols(stream, W2, d, 0, aW2 + (size_t)j * d * d, d, 0, d, d))) return fail(rc);
      if ((rc = launch_copy_cols(stream, b2, d, 0, ab2 + (size_t)j * d, d, 0, 1, d))) return fail(rc);
      if ((rc = launch_copy_cols(stream, W3, d, 0, aW3 + (size_t)j * 2 * d * d, d, 0, 2 * d, d))) return fail(rc);
      if ((rc = launch_copy_cols(stream, b3, 2 * d, 0, ab3 + (size_t)j * 2 * d, 2 * d, 0, 1, 2 * d))) return fail(rc);
      lw.Wqkv[a] = take((size_t)3 * d * d);
      lw.Wout[a] = take((size_t)d * d);
      lw.bout[a] = take(d);
      lw.gq[a] = take((size_t)H * 64);
      lw.gk[a] = take((size_t)H * 64);
    }
    lw.ffn_g = take(d);
    lw.ffn_b = take(d);
    const float* Wff1 = take((size_t)8 * d * d);
    const float* bff1 = take((size_t)8 * d);
    float* Wp = carve((size_t)8 * d * d);
    float* bp = carve((size_t)8 * d);
    if ((rc = launch_geglu_interleave(stream, Wff1, bff1, Wp, bp, 4 * d, d))) return fail(rc);
    lw.Wff1p = Wp; lw.bff1p = bp;
    lw.Wff2 = take((size_t)d * 4 * d);
    lw.bff2 = take(d);
  }
  m->hW0 = take((size_t)d * d); m->hb0 = take(d);
  m->hW2 = take((size_t)(d / 2) * d); m->hb2 = take(d / 2);
  m->hW4 = take((size_t)3 * (d / 2));
  if ((int64_t)(p - m->raw) != n_floats || (size_t)(q - m->derived) != n_derived) return fail(RAP_ERR_INVALID);
  if ((rc = ensure_logit_bounds(m, stream))) return fail(rc);
  *out = m;
  return RAP_OK;
}

extern "C" void rap_model_destroy(rap_model* m) {
  if (!m) return;
  if (m->raw) (void)hipFree(m->raw);
  if (m->derived) (void)hipFree(m->derived);
  for (int i = 0; i < 4; ++i)
    if (m->half[i].blob) (void)hipFree(m->half[i].blob);
  if (m->logit_bound) (void)hipFree(m->logit_bound);
  delete m;
}

// Per-head bounds on the attention logits from the qk-norm gains (a property of the weights): (L, 2, H) floats on the
// device; read back once (model creation may synchronise) to decide whether the bounded-softmax kernels are admissible.
static int ensure_logit_bounds(rap_model* m, hipStream_t stream) {
  if (m->logit_bound) return RAP_OK;
  const int n = m->L * 2 * m->H;
  if (hipMalloc((void**)&m->logit_bound, (size_t)n * sizeof(float)) != hipSuccess) { m->logit_bound = nullptr; return RAP_ERR_ALLOC; }
  for (int i = 0; i < m->L; ++i)
    for (int a = 0; a < 2; ++a) {
      const int rc = launch_qk_logit_bound(stream, m->layers[i].gq[a], m->layers[i].gk[a], m->H, m->logit_bound + (size_t)(2 * i + a) * m->H);
      if (rc) return rc;
    }
  std::vector<float> hb(n);
  RAP_HIP_CHECK(hipMemcpyAsync(hb.data(), m->logit_bound, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, stream));
  RAP_HIP_CHECK(hipStreamSynchronize(stream));
  m->bounded.assign((size_t)2 * m->L, 1);
  for (int j = 0; j < 2 * m->L; ++j)
    for (int h = 0; h < m->H; ++h)
      if (!(hb[(size_t)j * m->H + h] <= RAP_MAX_LOGIT_BOUND)) m->bounded[j] = 0;
  m->n_bounded = 0;
  for (uint8_t b : m->bounded) m->n_bounded += b;
  return RAP_OK;
}

// Split precision: paired fp16 head / tail planes of the six GEMM weights of every layer, each tensor multiplied by a power of two
// chosen from its largest magnitude (x2_pack.hip).  Model configuration may synchronise (as model creation does for the logit bounds).
static int build_x2_weights(rap_model* m, hipStream_t stream) {
  HalfWeights& hw = m->half[RAP_DT_F32X2];
  const size_t d = m->d, L = m->L;
  const size_t per_layer = 2 * (2 * (3 * d * d + d * d) + 8 * d * d + 4 * d * d);      // twice the 16-bit copy: heads and tails
  const int nt = (int)(6 * L);
  float* d_max = nullptr;
  if (hipMalloc((void**)&d_max, (size_t)nt * sizeof(float)) != hipSuccess) return RAP_ERR_ALLOC;
  if (hipMalloc((void**)&hw.blob, per_layer * L * sizeof(u16)) != hipSuccess) { hw.blob = nullptr; (void)hipFree(d_max); return RAP_ERR_ALLOC; }
  int rc = RAP_OK;
  auto fail = [&](int code) { (void)hipFree(hw.blob); hw.blob = nullptr; hw.layers.clear(); (void)hipFree(d_max); return code; };
  if (hipMemsetAsync(d_max, 0, (size_t)nt * sizeof(float), stream) != hipSuccess) return fail(RAP_ERR_HIP);
  struct Item { const float* src; size_t rows, cols; };
  std::vector<Item> items;
  for (size_t i = 0; i < L; ++i) {
    const LayerW& lw = m->layers[i];
    for (int a = 0; a < 2; ++a) { items.push_back({lw.Wqkv[a], 3 * d, d}); items.push_back({lw.Wout[a], d, d}); }
    items.push_back({lw.Wff1p, 8 * d, d});
    items.push_back({lw.Wff2, d, 4 * d});
  }
  for (int k = 0; k < nt && rc == RAP_OK; ++k) rc = launch_max_abs(stream, items[k].src, items[k].rows * items[k].cols, d_max + k);
  if (rc) return fail(rc);
  std::vector<float> hmax(nt);
  if (hipMemcpyAsync(hmax.data(), d_max, (size_t)nt * sizeof(float), hipMemcpyDeviceToHost, stream) != hipSuccess) return fail(RAP_ERR_HIP);
  if (hipStreamSynchronize(stream) != hipSuccess) return fail(RAP_ERR_HIP);
  u16* q = hw.blob;
  std::vector<const u16*> planes(nt);
  std::vector<float> inv(nt);
  std::vector<int> expo(nt);
  for (int k = 0; k < nt && rc == RAP_OK; ++k) {
    // largest magnitude * 2^e in (2^11, 2^12]; an all-zero tensor keeps e = 0
    // a NaN / Inf weight would silently become +-65 504 in the planes (saturating split): refuse the model instead
    if (!(hmax[k] < 3.0e38f)) return fail(RAP_ERR_INVALID);
    int e = 0;
    if (hmax[k] > 0.f) { int ex; (void)frexpf(hmax[k], &ex); e = 12 - ex; }
    e = e > 60 ? 60 : e < -60 ? -60 : e;
    expo[k] = hmax[k] > 0.f ? e : 16;
    inv[k] = ldexpf(1.0f, -e);
    planes[k] = q;
    rc = launch_x2_pack(stream, items[k].src, (long)items[k].cols, (long)items[k].rows, (int)items[k].cols, ldexpf(1.0f, e), q);
    q += 2 * items[k].rows * items[k].cols;
  }
  if (rc) return fail(rc);
  hw.layers.resize(L);
  for (size_t i = 0; i < L; ++i) {
    LayerWH& lh = hw.layers[i];
    const int k0 = (int)(6 * i);
    for (int a = 0; a < 2; ++a) {
      lh.Wqkv[a] = planes[k0 + 2 * a]; lh.s_qkv[a] = inv[k0 + 2 * a];
      { int g = expo[k0 + 2 * a] - 16; g = g > 12 ? 12 : g < -12 ? -12 : g; lh.g_v[a] = ldexpf(1.0f, g); }
      lh.Wout[a] = planes[k0 + 2 * a + 1]; lh.s_out[a] = inv[k0 + 2 * a + 1];
    }
    lh.Wff1p = planes[k0 + 4]; lh.s_ff1 = inv[k0 + 4];
    { int g = 2 * (expo[k0 + 4] - 16); g = g > 24 ? 24 : g < -24 ? -24 : g; lh.g_ff1 = ldexpf(1.0f, g); }
    lh.Wff2 = planes[k0 + 5]; lh.s_ff2 = inv[k0 + 5];
  }
  (void)hipFree(d_max);
  return RAP_OK;
}

extern "C" int rap_model_set_compute_dtype(rap_model* m, int32_t dtype, void* stream_) {
  if (!m) return RAP_ERR_INVALID;
  std::lock_guard<std::mutex> lock(m->cfg_mu);
  if (dtype == RAP_DT_F32) { m->dtype = dtype; return RAP_OK; }
  if (dtype != RAP_DT_BF16 && dtype != RAP_DT_F16 && dtype != RAP_DT_F32X2) return RAP_ERR_INVALID;
  HalfWeights& hw = m->half[dtype];
  if (!hw.blob && dtype == RAP_DT_F32X2) {
    const int rcx = build_x2_weights(m, (hipStream_t)stream_);
    if (rcx) return rcx;
  }
  if (!hw.blob) {
    hipStream_t stream = (hipStream_t)stream_;
    const size_t d = m->d, L = m->L;
    const size_t per_layer = 2 * (3 * d * d + d * d) + 8 * d * d + 4 * d * d;
    if (hipMalloc((void**)&hw.blob, per_layer * L * sizeof(u16)) != hipSuccess) { hw.blob = nullptr; return RAP_ERR_ALLOC; }
    u16* q = hw.blob;
    int rc = RAP_OK;
    auto conv = [&](const float* src, size_t n) -> const u16* {
      u16* dst = q; q += n;
      if (rc == RAP_OK) rc = launch_convert_h16(stream, dtype, src, dst, n);
      return dst;
    };
    hw.layers.resize(L);
    for (size_t i = 0; i < L; ++i) {
      const LayerW& lw = m->layers[i];
      LayerWH& lh = hw.layers[i];
      for (int a = 0; a < 2; ++a) {
        lh.Wqkv[a] = conv(lw.Wqkv[a], 3 * d * d);
        lh.Wout[a] = conv(lw.Wout[a], d * d);
      }
      lh.Wff1p = conv(lw.Wff1p, 8 * d * d);
      lh.Wff2 = conv(lw.Wff2, 4 * d * d);
    }
    if (rc != RAP_OK) { (void)hipFree(hw.blob); hw.blob = nullptr; hw.layers.clear(); return rc; }
  }
  { const int rcb = ensure_logit_bounds(m, (hipStream_t)stream_); if (rcb) return rcb; }
  m->dtype = dtype;
  return RAP_OK;
}
extern "C" int rap_model_compute_dtype(const rap_model* m) { return m ? m->dtype : RAP_ERR_INVALID; }
// Residual stream of the 16-bit modes: fp32 (default) or fp16 -- what the reference's autocast inference holds (nn.Linear outputs
// are 16-bit under Lightning "16-mixed", layer.py:155-164 adds them).  Ignored while the compute dtype is fp32.
extern "C" int rap_model_set_residual_dtype(rap_model* m, int32_t dtype) {
  if (!m || (dtype != RAP_DT_F32 && dtype != RAP_DT_F16)) return RAP_ERR_INVALID;
  std::lock_guard<std::mutex> lock(m->cfg_mu);
  m->resid_dtype = dtype;
  return RAP_OK;
}
extern "C" int rap_model_residual_dtype(const rap_model* m) { return m ? m->resid_dtype : RAP_ERR_INVALID; }
extern "C" int rap_model_bounded_attention_launches(const rap_model* m) {
  return m ? ((m->qk_norm && !(m->softcap > 0.f)) ? m->n_bounded : 0) : RAP_ERR_INVALID;
}
// qk_norm = False of the reference's constructor (point_cloud_dit.py:28, layer.py:75-83,103-104): q and k go to the attention as projected.
// Without the norm there is no bound on the logits, so every attention launch takes the online-softmax kernel; the gains in the blob are ignored.
extern "C" int rap_model_set_qk_norm(rap_model* m, int32_t on) {
  if (!m) return RAP_ERR_INVALID;
  std::lock_guard<std::mutex> lock(m->cfg_mu);
  m->qk_norm = on != 0;
  return RAP_OK;
}
extern "C" int rap_model_qk_norm(const rap_model* m) { return m ? (m->qk_norm ? 1 : 0) : RAP_ERR_INVALID; }
// softcap of the reference's constructor (point_cloud_dit.py:27, layer.py:33,64,106-128): s <- c tanh(s / c) in front of the softmax.  A capped
// model runs one attention plan (plan_call / plan_attention): the soft-capped online kernels, unsplit, 256-row items.  The cap is itself a
// logit bound (|s| <= c), so the bounded, offset-free softmax with min(bound, c) would apply -- those instantiations are not opened here.
extern "C" int rap_model_set_softcap(rap_model* m, float c) {
  if (!m || !(c >= 0.f) || !(c < 3.0e38f)) return RAP_ERR_INVALID;      // (NaN fails the first comparison)
  std::lock_guard<std::mutex> lock(m->cfg_mu);
  m->softcap = c;
  return RAP_OK;
}
extern "C" float rap_model_softcap(const rap_model* m) { return m ? m->softcap : (float)RAP_ERR_INVALID; }
// final_mlp_act of the reference's constructor (point_cloud_dit.py:30,111-117): the epilogue of the head's two hidden GEMMs
extern "C" int rap_model_set_final_act(rap_model* m, int32_t act) {
  if (!m || act < 0 || act > 2) return RAP_ERR_INVALID;
  std::lock_guard<std::mutex> lock(m->cfg_mu);
  m->final_act = act;
  return RAP_OK;
}
extern "C" int rap_model_final_act(const rap_model* m) { return m ? m->final_act : RAP_ERR_INVALID; }

// ---------------------------------------------------------------------------------------------
// workspace
// ---------------------------------------------------------------------------------------------
// the arithmetic a call of `rows` token rows actually runs in (see g_rap_x2_min_rows)
static int eff_dtype(int model_dtype, size_t rows) {
  return (model_dtype == RAP_DT_F32X2 && (long)rows < (long)g_rap_x2_min_rows) ? RAP_DT_F32 : model_dtype;
}

// ---------------------------------------------------------------------------------------------
// The plan of a model call: EVERY decision that follows from the call's shape, the model's configuration and the tuning keys -- the
// arithmetic, the padded row count, the attention work-list geometry, the split-K planes the layout reserves, the combine + LayerNorm
// fusion, and the shape fields (with "workspace given or not") of each of the eight GEMMs of a forward.  plan_call is the one place that
// states them: carve_workspace lays the buffers out by it, prepare_static / block_f32 / block_h16 / forward_step fill their GemmParams from
// it (gemm_into), and rap_call_plan reports it, so that a test can hold a call of a given size to the kernels it is meant to reach.
// The tuning keys are read once, when the call is planned.
// ---------------------------------------------------------------------------------------------
struct CallShape {
  int dtype, resid_dtype;      // the MODEL's compute / residual dtype (the call's arithmetic: CallPlan::dtype)
  int d, H, L, Ks;
  bool qk_norm;
  float softcap;               // the model's cap on the attention logits (0 = off)
  int final_act;               // the head's activation (0 SiLU, 1 GELU, 2 ReLU)
  int64_t TP;
  int B, nseg_part, rows;      // rows: rows of the adaLN table (flow steps of rap_sample, B of rap_dit_forward)
};
enum PlanGemm { PG_STATIC = 0, PG_EMBED, PG_QKV, PG_OUT, PG_FF1, PG_FF2, PG_HEAD0, PG_HEAD1, PG_COUNT };
struct GemmShape {
  int epi = 0, M = 0, N = 0, K = 0, lda = 0, ldw = 0, ldc = 0, ldr = 0;
  bool ws = false;             // a split-K workspace is handed in (which buffer: the launch site's business)
  int planes = 0;              // GemmParams::splitk_planes
  int defer = 0, force_splits = 0;      // GemmParamsH::defer_combine / force_splits
};
struct CallPlan {
  int dtype;                   // the arithmetic this call runs in (eff_dtype)
  bool x2, h16_stream;         // split precision; the residual stream is held in fp16
  bool capped;                 // soft-capped logits: every attention launch is the capped online kernel, unsplit, on 256-row items
  int TQ;                      // align_up(TP, 256): rows of every token-row buffer
  int attn_bq, attn_kg;        // query rows per attention work item; key groups per block of the 16-bit attention
  int max_items_part, max_items_batch;
  int splitk_planes;           // (TQ, d) fp32 planes reserved for the 16-bit / split-precision residual GEMMs (0: no buffer)
  bool fused;                  // every residual GEMM leaves its planes to the combine + LayerNorm kernel
  GemmShape g[PG_COUNT];       // PG_QKV .. PG_FF2 in the call's arithmetic (GemmParams or GemmParamsH), the others fp32
};

static CallPlan plan_call(const CallShape& s, int force_dtype = -1) {
  CallPlan p{};
  const int d = s.d, TP = (int)s.TP;
  const size_t Tz = align_up((size_t)s.TP, 256);
  const int T = p.TQ = (int)Tz;
  const int dtype = p.dtype = force_dtype >= 0 ? force_dtype : eff_dtype(s.dtype, Tz);
  const bool f32 = dtype == RAP_DT_F32, x2 = p.x2 = dtype == RAP_DT_F32X2;
  const bool half = dtype == RAP_DT_BF16 || dtype == RAP_DT_F16;
  p.h16_stream = half && s.resid_dtype == RAP_DT_F16;
  // query rows per attention work item: 256, or 64 / 128 for few-token calls of the 16-bit modes (attention_h16_plan)
  // (a capped model: the one form the soft-capped kernels have -- full-size items, one key group)
  p.capped = s.softcap > 0.f;
  p.attn_bq = RAP_ATTN_BQ; p.attn_kg = 1;
  if (half && !p.capped) attention_h16_plan((long)T, &p.attn_bq, &p.attn_kg);
  p.max_items_batch = (int)(s.TP / p.attn_bq) + s.B + 1;
  p.max_items_part = (int)(s.TP / p.attn_bq) + s.nseg_part + 1;
  // ff2: the one layer GEMM with K >= 1024.  Reserved by SHAPE alone (tuning key 6 only gates the launch), so that the size
  // rap_workspace_bytes reports cannot change between the query and the call
  if (!f32) {
    const int splits = gemm_h16_splits_by_shape(T, d, (x2 ? 8 : 4) * d);   // (split precision: the physical K of ff2 is 8 d)
    p.splitk_planes = splits > 1 ? splits : 0;
  }
  // Few-token calls of the 16-bit / split-precision blocks (round 6; the reference's everyday batch_size: 1, RAP_inference.yaml:30-36): every
  // residual GEMM leaves fp32 partial planes (split-K where gemm_h16_splits says so, one plane otherwise) and ONE kernel forms the new
  // residual-stream value and the LayerNorm that follows it (launch_resid_combine_ln_h16) -- 11 launches per layer instead of 14.  The planes
  // live in the split-K buffer, which exists exactly for the calls this is meant for (<= 128 tiles of 128 x 128 in the N = d GEMMs).
  p.fused = g_rap_small_fused && !f32 && p.splitk_planes > 0 && g_rap_gemm_splitk;

  auto shape = [](int epi, int M, int N, int K, int lda, int ldw, int ldc, int ldr) {
    GemmShape g; g.epi = epi; g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldw = ldw; g.ldc = ldc; g.ldr = ldr; return g;
  };
  // (the count is fixed HERE: the GEMM and the pass that reads its planes cannot disagree)
  auto defer_combine = [](GemmShape& g) { const int sp = gemm_h16_splits(g.M, g.N, g.K); g.defer = 1; g.force_splits = sp > 1 ? sp : 1; };
  // fp32 in every mode: the step-invariant embedding part over the TP real rows, PE(x_t) Wx^T + base and the head over TQ rows
  p.g[PG_STATIC] = shape(EPI_BIAS_ANCHOR, TP, d, s.Ks, s.Ks, s.Ks, d, 0);
  p.g[PG_EMBED] = shape(EPI_BIAS_RESID, T, d, 64, 64, 64, d, d);
  // few-token calls: K of the two hidden layers of the head over 2 / 4 blocks per tile (gemm_f32_form decides by the tile count); the partial
  // planes live in the FFN buffer of the fp32 layout (4 T d floats, idle there) resp. the split-K planes of the 16-bit layouts
  // final_mlp_act: the epilogue of the model's activation; only SiLU has the split-K form (a GELU / ReLU head runs unsplit: no workspace, no planes)
  const int head_epi = s.final_act == 1 ? EPI_BIAS_GELU : s.final_act == 2 ? EPI_BIAS_RELU : EPI_BIAS_SILU;
  p.g[PG_HEAD0] = shape(head_epi, T, d, d, d, d, d, 0);
  p.g[PG_HEAD1] = shape(head_epi, T, d / 2, d, d, d, d / 2, 0);
  if (head_epi == EPI_BIAS_SILU)
    for (int k = PG_HEAD0; k <= PG_HEAD1; ++k) { p.g[k].ws = f32 || p.splitk_planes > 0; p.g[k].planes = f32 ? 4 : p.splitk_planes; }
  if (f32) {
    p.g[PG_QKV] = shape(EPI_QKV_HEADMAJOR, T, 3 * d, d, d, d, 0, 0);
    p.g[PG_OUT] = shape(EPI_BIAS_RESID, T, d, d, d, d, d, d);
    p.g[PG_OUT].ws = true;       // the FFN buffer, idle between the FFNs (the split attention's partial planes are consumed by then): 4 (T,d) planes
    p.g[PG_FF1] = shape(EPI_GEGLU, T, 8 * d, d, d, d, 4 * d, 0);
    p.g[PG_FF2] = shape(EPI_BIAS_RESID, T, d, 4 * d, 4 * d, 4 * d, d, d);
    p.g[PG_FF2].ws = true;       // qkv (3 T d) and att (T d), idle during the FFN and adjacent: 4 (T,d) planes
  } else {
    const int pl = x2 ? 2 : 1;   // planes per value: K, lda, ldw (and ldc of the GEGLU output) are physical 16-bit counts
    const int epi_resid = p.h16_stream ? EPI_H_BIAS_RESID_H16 : EPI_H_BIAS_RESID_F32;
    // qk-norm in the QKV epilogue (tuning key 7; always in split precision): one kernel, q / k normalised from the fp32 accumulators
    p.g[PG_QKV] = shape((x2 || (g_rap_fuse_qknorm && s.qk_norm)) ? EPI_H_QKV_NORM : EPI_H_QKV, T, 3 * d, pl * d, pl * d, pl * d, 0, 0);
    p.g[PG_OUT] = shape(epi_resid, T, d, pl * d, pl * d, pl * d, d, d);
    if (p.fused) { p.g[PG_OUT].ws = true; defer_combine(p.g[PG_OUT]); }
    p.g[PG_FF1] = shape(EPI_H_GEGLU, T, 8 * d, pl * d, pl * d, pl * d, pl * 4 * d, 0);
    p.g[PG_FF2] = shape(epi_resid, T, d, pl * 4 * d, pl * 4 * d, pl * 4 * d, d, d);
    p.g[PG_FF2].ws = p.splitk_planes > 0;      // few-token calls: K = 4d (physical 8d in split precision) over 2 / 4 blocks per tile
    // ... and its combine pass is the first LayerNorm of the next layer (the last layer's ff2 combines itself: block_h16)
    if (p.fused && s.L > 1) defer_combine(p.g[PG_FF2]);
  }
  return p;
}
static float g_ws_given;      // (never dereferenced: a form only asks whether a workspace was handed in)
static void gemm_into(const GemmShape& s, GemmParams& g, float* ws) {
  g.M = s.M; g.N = s.N; g.K = s.K; g.lda = s.lda; g.ldw = s.ldw; g.ldc = s.ldc; g.ldr = s.ldr;
  g.splitk_ws = s.ws ? ws : nullptr; g.splitk_planes = s.planes;
}
static void gemm_into(const GemmShape& s, GemmParamsH& g, float* ws) {
  g.M = s.M; g.N = s.N; g.K = s.K; g.lda = s.lda; g.ldw = s.ldw; g.ldc = s.ldc; g.ldr = s.ldr;
  g.splitk_ws = s.ws ? ws : nullptr; g.defer_combine = s.defer; g.force_splits = s.force_splits;
}
// the form code (kernels.h) of GEMM k of the plan
static int plan_form(const CallPlan& p, int k) {
  if (p.dtype == RAP_DT_F32 || k < PG_QKV || k > PG_FF2) { GemmParams g{}; gemm_into(p.g[k], g, &g_ws_given); return gemm_f32_form(p.g[k].epi, g); }
  GemmParamsH g{}; gemm_into(p.g[k], g, &g_ws_given); return gemm_h16_form(p.dtype, p.g[k].epi, g);
}
// the key ranges of one attention launch (branch 0: per part, 1: per sample) and whether the split launch keeps every CU to one block.
// bounded: every head of that launch has a logit bound (fp32: only the bounded kernel can add partial results; 16-bit: never split)
struct AttnPlan { int splits; bool one_per_cu; };
static AttnPlan plan_attention(const CallPlan& p, int H, int branch, bool bounded) {
  const int max_items = branch == 0 ? p.max_items_part : p.max_items_batch;
  if (p.capped) return {1, false};
  if (p.dtype == RAP_DT_F32) { const int sp = attention_f32_splits(max_items, H, bounded); return {sp, attention_f32_one_per_cu(max_items, H, sp)}; }
  if (p.x2) return {attention_x2_splits(max_items, H), false};
  return {1, false};
}

struct Workspace {
  float *base, *h, *xn, *qkv, *att, *ffmid, *ax, *v, *mod, *ada_scratch, *xt, *Rc, *tc, *tgrid;
  u16* h16;                            // the residual stream when it is held in fp16 (16-bit modes with resid_dtype = fp16; h is then null)
  float *hid1, *hid2, *astatic;        // head hidden layers (T,d), (T,d/2) and the static feature matrix (T,Ks), Ks = 128 + align_up(in_dim, 32): aliases
  u16 *xnh, *qkh, *vth, *atth, *ffmidh; // reduced-precision mode: 16-bit activations (xn/qkv/att/ffmid are then unused)
  float* splitk_h;                      // reduced-precision mode, few-token calls only: fp32 partial planes of the split-K ff2 GEMM (else null)
  int splitk_planes;                    // ... and how many (T, d) planes were reserved there (2 or 4; 0 without the buffer)
  int vt_nblk;
  int rows;                             // TQ = align_up(TP, 256): rows of every token-row buffer
  int dtype;                            // the arithmetic this call runs in (eff_dtype: the model's, or fp32 for a small split-precision call)
  bool qk_norm;                         // snapshot of the model's switch (the configuration mutex is held only while the layout is carved)
  float softcap;                        // ... and of its cap on the attention logits (0 = off)
  double* proc_partials;
  int32_t *token_sample, *part_offsets, *attn_sort;
  int32_t *cu_batch_s, *cu_part_s;      // sanitised copies of the caller's segment tables (clamped to [0, TP], non-decreasing)
  const int32_t* cu_part_live;          // the part table the attention work lists were built from (part_offsets in rap_sample, cu_part_s in rap_dit_forward)
  int nseg_part, nseg_batch;            // segments in the two tables
  AttnWorkItem *items_batch, *items_part;
  int max_items_batch, max_items_part;
  int attn_bq;                          // query rows per work item of this call's attention lists
  int attn_kg;                          // key groups per block of the 16-bit attention (1, or 2 / 4 for few-token calls)
  CallPlan plan;                        // what the fields above were laid out by, and what the launches of this call follow
  size_t total;
};

static CallShape call_shape(const rap_model* m, int64_t TP, int B, int nseg_part, int rows) {
  CallShape s{};
  s.dtype = m->dtype; s.resid_dtype = m->resid_dtype; s.d = m->d; s.H = m->H; s.L = m->L; s.Ks = m->Ks; s.qk_norm = m->qk_norm;
  s.softcap = m->softcap; s.final_act = m->final_act;
  s.TP = TP; s.B = B; s.nseg_part = nseg_part; s.rows = rows;
  return s;
}
static Workspace carve_workspace(const CallShape& s, char* basep, int force_dtype = -1) {
  Workspace w;
  const CallPlan& plan = w.plan = plan_call(s, force_dtype);
  const size_t d = s.d, L = s.L;
  const int64_t TP = s.TP;
  const int B = s.B, nseg_part = s.nseg_part, rows = s.rows;
  Carver c(basep);
  // Every token-row buffer is carved at TQ = align_up(TP, 256) rows (round 4): the layer kernels run over TQ rows, so the persistent
  // 256-row-tile GEMMs serve ANY token count (ragged batches are the reference's real regime, RAP_inference.yaml:30-36); rows
  // TP .. TQ-1 are finite filler nobody reads (rows are independent in every kernel but attention, whose work lists and key
  // ranges stop at the true segment ends).  See forward_step.
  const size_t T = (size_t)plan.TQ;
  w.rows = plan.TQ;
  const int dtype = w.dtype = plan.dtype;
  w.qk_norm = s.qk_norm;
  w.softcap = s.softcap;
  w.base = (float*)c.take(T * d * 4);
  const bool x2 = plan.x2;                  // split precision: fp32 residual stream, every 16-bit activation buffer holds heads AND tails
  const bool h16 = plan.h16_stream;
  w.h = h16 ? nullptr : (float*)c.take(T * d * 4);
  w.h16 = h16 ? (u16*)c.take(T * d * 2) : nullptr;
  w.xn = w.qkv = w.att = w.ffmid = nullptr;
  w.xnh = w.qkh = w.vth = w.atth = w.ffmidh = nullptr;
  w.splitk_h = nullptr;
  w.splitk_planes = 0;
  w.vt_nblk = 0;
  if (dtype == RAP_DT_F32) {
    w.xn = (float*)c.take(T * d * 4);            // also head hidden 1 (TP,d)
    w.qkv = (float*)c.take(T * 3 * d * 4);
    w.att = (float*)c.take(T * d * 4);           // also head hidden 2 (TP,d/2)
    w.ffmid = (float*)c.take(T * 4 * d * 4);     // also the static feature matrix (TP,Ks) during prepare (16 T d >= 4 T Ks bytes for d >= 256)
    w.hid1 = w.xn; w.hid2 = w.att; w.astatic = w.ffmid;
  } else {
    const size_t pl = x2 ? 2 : 1;              // planes per value
    w.vt_nblk = (int)(T / 64);                 // V^T image: whole 64-token blocks over the padded rows
    w.xnh = (u16*)c.take(T * d * 2 * pl);
    w.qkh = (u16*)c.take(T * 2 * d * 2 * pl);    // q,k [2][H][T][64]   (x2: [2][H][2 chunks][T][64 physical])
    w.vth = (u16*)c.take((size_t)w.vt_nblk * 64 * d * 2 * pl);   // [H][vt_nblk][64][64]   (x2: [H][vt_nblk][2 chunks][64][64 physical])
    w.atth = (u16*)c.take(T * d * 2 * pl);
    // >= 8*T*d bytes: also hosts the fp32 head hidden layers and the static feature matrix (T,Ks) fp32 = 4*T*Ks bytes, which is the
    // larger of the two at d = 256 with in_dim > 384 in the 16-bit modes (pl = 1)
    const size_t ffmid_bytes = T * 4 * d * 2 * pl, static_bytes = T * (size_t)s.Ks * 4;
    w.ffmidh = (u16*)c.take(ffmid_bytes > static_bytes ? ffmid_bytes : static_bytes);
    w.hid1 = (float*)w.ffmidh;                 // (T,d) fp32   = 4*T*d bytes
    w.hid2 = w.hid1 + T * d;                   // (T,d/2) fp32 = 2*T*d bytes
    w.astatic = (float*)w.ffmidh;
    // the fp32 partial planes of few-token calls (plan_call: by the shape of ff2 alone)
    if (plan.splitk_planes > 0) { w.splitk_h = (float*)c.take((size_t)plan.splitk_planes * T * d * 4); w.splitk_planes = plan.splitk_planes; }
  }
  w.ax = (float*)c.take(T * 64 * 4);
  w.v = (float*)c.take(T * 3 * 4);
  w.xt = (float*)c.take(T * 3 * 4);
  w.mod = (float*)c.take((size_t)rows * 2 * L * 2 * d * 4);
  w.ada_scratch = (float*)c.take((size_t)rows * (256 + 4 * L * d) * 4);
  w.tgrid = (float*)c.take((size_t)rows * 4);
  w.token_sample = (int32_t*)c.take(T * 4);
  w.part_offsets = (int32_t*)c.take(((size_t)nseg_part + 1) * 4);
  w.cu_batch_s = (int32_t*)c.take(((size_t)B + 1) * 4);
  w.cu_part_s = (int32_t*)c.take(((size_t)nseg_part + 1) * 4);
  w.cu_part_live = w.part_offsets; w.nseg_part = nseg_part; w.nseg_batch = B;
  w.attn_bq = plan.attn_bq; w.attn_kg = plan.attn_kg;
  w.max_items_batch = plan.max_items_batch; w.max_items_part = plan.max_items_part;
  // (reserved for the smallest work items whatever tuning key 20 says: the size rap_workspace_bytes reports does not depend on the key)
  w.items_batch = (AttnWorkItem*)c.take(((size_t)(TP / 64) + B + 1) * sizeof(AttnWorkItem));
  w.items_part = (AttnWorkItem*)c.take(((size_t)(TP / 64) + nseg_part + 1) * sizeof(AttnWorkItem));
  w.attn_sort = (int32_t*)c.take(((size_t)(nseg_part > B ? nseg_part : B) + 1) * 4);   // scratch of the longest-first work-list order
  w.proc_partials = (double*)c.take((size_t)nseg_part * RAP_PROC_CHUNKS * 16 * 8);
  w.Rc = (float*)c.take((size_t)nseg_part * 9 * 4);
  w.tc = (float*)c.take((size_t)nseg_part * 3 * 4);
  w.total = c.total();
  return w;
}

static size_t workspace_bytes_of(const CallShape& s) {
  if (s.dtype == RAP_DT_F32X2) {      // both layouts: see rap_workspace_bytes
    const size_t a = carve_workspace(s, nullptr, RAP_DT_F32).total;
    const size_t b = carve_workspace(s, nullptr, RAP_DT_F32X2).total;
    return a > b ? a : b;
  }
  return carve_workspace(s, nullptr).total;
}
extern "C" size_t rap_workspace_bytes(const rap_model* m, int64_t TP, int32_t B, int32_t nseg_part, int32_t rows) {
  if (!m || TP < 0 || B < 0 || nseg_part < 0 || rows < 0) return 0;
  std::lock_guard<std::mutex> lock(m->cfg_mu);
  // A split-precision model runs calls below tuning key 17's threshold on the exact-fp32 kernels, and the two layouts differ in size (the
  // split layout adds the split-K planes of few-token calls).  The size reported covers BOTH, so that a change of the process-global
  // threshold between this query and the call -- __graft_entry__.smoke() and the tests do toggle it -- cannot turn a valid call into
  // RAP_ERR_WORKSPACE (the comment here used to claim the two layouts need the same bytes).
  return workspace_bytes_of(call_shape(m, TP, B, nseg_part, rows));
}

// What a model call of this shape does (include/rapflow.h): plan_call's own answer -- the function the launch path runs by -- plus the form
// code of each GEMM and the workspace size.  Host arithmetic only: no model handle, no device.
extern "C" int rap_call_plan(int32_t compute_dtype, int32_t resid_dtype, int32_t d, int32_t heads, int32_t num_layers, int32_t in_dim, int64_t TP,
                             int32_t B, int32_t nseg_part, int32_t rows, int32_t bounded, int64_t* out, int32_t n_out) {
  if (!out || n_out < RAP_CALL_PLAN_FIELDS) return RAP_ERR_INVALID;
  if (compute_dtype < RAP_DT_F32 || compute_dtype > RAP_DT_F32X2 || (resid_dtype != RAP_DT_F32 && resid_dtype != RAP_DT_F16)) return RAP_ERR_INVALID;
  rap_model_desc desc{};
  desc.embed_dim = d; desc.num_heads = heads; desc.num_layers = num_layers;
  if (!desc_ok(&desc) || !in_dim_ok(in_dim)) return RAP_ERR_INVALID;
  if (TP <= 0 || TP > 0x7fffffffLL / 8 || B <= 0 || nseg_part < 0 || nseg_part > 65535 || rows <= 0) return RAP_ERR_INVALID;
  CallShape s{};
  s.dtype = compute_dtype; s.resid_dtype = resid_dtype; s.d = d; s.H = heads; s.L = num_layers; s.Ks = 128 + (int)align_up((size_t)in_dim, 32);
  s.softcap = 0.f; s.final_act = 0;      // (rapflow.h: the plan of an uncapped model with the SiLU head)
  s.qk_norm = true;      // (every shipped configuration; without it no launch is bounded and the QKV epilogue of the 16-bit modes is the plain one)
  s.TP = TP; s.B = B; s.nseg_part = nseg_part; s.rows = rows;
  const CallPlan p = plan_call(s);
  const AttnPlan ap = plan_attention(p, heads, 0, bounded != 0), ab = plan_attention(p, heads, 1, bounded != 0);
  int64_t* o = out;
  *o++ = p.dtype; *o++ = p.TQ; *o++ = p.attn_bq; *o++ = p.attn_kg; *o++ = p.max_items_part; *o++ = p.max_items_batch;
  *o++ = ap.splits; *o++ = ab.splits; *o++ = ap.one_per_cu ? 1 : 0; *o++ = ab.one_per_cu ? 1 : 0;
  *o++ = p.fused ? 1 : 0; *o++ = p.splitk_planes;
  for (int k = 0; k < PG_COUNT; ++k) *o++ = plan_form(p, k);
  *o++ = (int64_t)workspace_bytes_of(s);
  static_assert(12 + PG_COUNT + 1 == RAP_CALL_PLAN_FIELDS, "rapflow.h: the fields of rap_call_plan");
  return RAP_OK;
}

// ---------------------------------------------------------------------------------------------
// prepare (step-invariant work) and one forward
// ---------------------------------------------------------------------------------------------
static int zero_rows(hipStream_t stream, void* base, size_t row_bytes, int row0, int row1) {
  if (row1 <= row0) return RAP_OK;
  if (hipMemsetAsync((char*)base + (size_t)row0 * row_bytes, 0, (size_t)(row1 - row0) * row_bytes, stream) != hipSuccess) {
    rap_set_last_hip_error((int)hipGetLastError());
    return RAP_ERR_HIP;
  }
  return RAP_OK;
}

static int prepare_static(const rap_model* m, const Workspace& w, hipStream_t stream, const float* cond, const float* feat,
                          const float* scales, const uint8_t* anchor, const int32_t* cu_batch, const int32_t* cu_part,
                          int B, int nseg_part, int TP, const float* latent = nullptr) {
  int rc;
  // the caller's tables are only ever read through sanitised copies: every index derived from them stays inside [0, TP]
  if ((rc = launch_sanitize_cu(stream, cu_batch, B + 1, TP, w.cu_batch_s))) return rc;
  cu_batch = w.cu_batch_s;
  if (cu_part != w.part_offsets) {          // rap_dit_forward: the caller's part table (rap_sample builds its own, clamped, from points_per_part)
    if ((rc = launch_sanitize_cu(stream, cu_part, nseg_part + 1, TP, w.cu_part_s))) return rc;
    cu_part = w.cu_part_s;
  }
  if ((rc = launch_token_sample(stream, cu_batch, B, w.token_sample))) return rc;
  const int bq = w.dtype == RAP_DT_F32 ? 0 : w.dtype == RAP_DT_F32X2 ? 256 : w.attn_bq;
  int32_t* sort_ws = g_rap_attn_lpt ? w.attn_sort : nullptr;
  if ((rc = launch_build_attn_worklist(stream, cu_batch, B, w.items_batch, w.max_items_batch, bq, sort_ws))) return rc;
  if ((rc = launch_build_attn_worklist(stream, cu_part, nseg_part, w.items_part, w.max_items_part, bq, sort_ws))) return rc;
  // Filler rows TP .. TQ-1 (TQ = align_up(TP, 256), see carve_workspace): every value a layer kernel reads there has to be FINITE,
  // because the 16-bit attention's V^T image is blocked by 64 tokens and a masked key still multiplies its V column by p = 0
  // (0 x NaN = NaN).  Zero the filler rows of the four buffers no kernel writes beyond row TP -- the step-invariant embedding
  // part, PE(x_t), the attention output, the sample index of a token -- once per call; everything else in rows TP .. TQ-1 is then
  // computed from those by row-independent kernels (LayerNorm, GEMMs) and stays finite.
  const int TQ = w.rows, d = m->d;
  if ((rc = zero_rows(stream, w.base, (size_t)d * 4, TP, TQ))) return rc;
  if ((rc = zero_rows(stream, w.ax, 64 * 4, TP, TQ))) return rc;
  if ((rc = zero_rows(stream, w.token_sample, 4, TP, TQ))) return rc;
  if (w.dtype == RAP_DT_F32) { if ((rc = zero_rows(stream, w.att, (size_t)d * 4, TP, TQ))) return rc; }
  else if ((rc = zero_rows(stream, w.atth, (size_t)d * 2 * (w.dtype == RAP_DT_F32X2 ? 2 : 1), TP, TQ))) return rc;
  // base = [PE63(cond) | PE21(scale) | feat | 0] Wstatic^T + emb bias + anchor embedding   (embedding.py:155-179,
  // point_cloud_dit.py:119-139) -- everything in the embedding that does not depend on x_t.
  float* astatic = w.astatic;
  const int Ks = m->Ks;
  if ((rc = launch_posenc_static(stream, cond, scales, w.token_sample, feat, m->F, astatic, TP, Ks))) return rc;
  if (m->Din > 0) {
    // latent point features (embedding.py:163-166: concatenated between the coordinate and the scale embeddings): step-invariant, so
    // they are Din more columns of the hoisted K = Ks GEMM; columns 128 + Din .. Ks - 1 are zero padding up to the k-tile
    if (Ks > 128 + m->Din &&
        hipMemset2DAsync(astatic + 128 + m->Din, (size_t)Ks * 4, 0, (size_t)(Ks - 128 - m->Din) * 4, (size_t)TP, stream) != hipSuccess) {
      rap_set_last_hip_error((int)hipGetLastError());
      return RAP_ERR_HIP;
    }
    if ((rc = launch_copy_cols(stream, latent, m->Din, 0, astatic, Ks, 128, TP, m->Din))) return rc;
  }
  GemmParams g{};
  gemm_into(w.plan.g[PG_STATIC], g, nullptr);      // M = TP rows, K = Ks
  g.A = astatic; g.W = m->Wstatic; g.C = w.base; g.bias = m->emb_bias; g.anchor = anchor; g.anchor_emb = m->anchor_emb;
  return launch_gemm_f32(stream, w.plan.g[PG_STATIC].epi, g);
}

// ---- one transformer block in exact fp32 (layer i).  mod: see forward_step.
static int block_f32(const rap_model* m, const Workspace& w, hipStream_t stream, int i, const float* mod, long mod_stride,
                     const int32_t* token_row) {
  const int d = m->d, H = m->H, TP = w.rows;
  const CallPlan& plan = w.plan;
  const LayerW& lw = m->layers[i];
  int rc;
  for (int a = 0; a < 2; ++a) {   // a = 0: per-part attention, a = 1: per-sample attention (layer.py:152-160)
    const int j = 2 * i + a;
    { ProfScope ps(stream, 3); rc = launch_layernorm_mod(stream, w.h, w.xn, TP, d, mod + (size_t)j * 2 * d, mod_stride, token_row); }
    if (rc) return rc;
    GemmParams g{};
    gemm_into(plan.g[PG_QKV], g, nullptr);
    g.A = w.xn; g.W = lw.Wqkv[a]; g.C = w.qkv; g.heads = H;
    const bool fuse_qk = g_rap_fuse_qknorm != 0 && w.qk_norm;
    if (fuse_qk) { g.gamma_q = lw.gq[a]; g.gamma_k = lw.gk[a]; }        // qk-norm in the QKV epilogue (tuning key 7)
    { ProfScope ps(stream, 2); rc = launch_gemm_f32(stream, plan.g[PG_QKV].epi, g); }
    if (rc) return rc;
    if (!fuse_qk && w.qk_norm && (rc = launch_qknorm(stream, w.qkv, TP, H, lw.gq[a], lw.gk[a]))) return rc;
    {
      ProfScope ps(stream, a);
      const float* bound = (w.qk_norm && m->bounded[j] && !plan.capped) ? m->logit_bound + (size_t)j * H : nullptr;
      // few-token calls: split the keys of every work item over up to 4 blocks; the partial O planes live in the (idle) FFN
      // buffer (4 x TP x d floats), the partial row sums in the (idle) LN-output buffer
      const int max_items = a == 0 ? w.max_items_part : w.max_items_batch;
      const int splits = plan_attention(plan, H, a, bound != nullptr).splits;
      if (plan.capped)
        rc = launch_attention_f32_softcap(stream, w.qkv, w.att, TP, H, a == 0 ? w.items_part : w.items_batch, max_items, w.softcap);
      else
      rc = launch_attention_f32(stream, w.qkv, w.att, TP, H, a == 0 ? w.items_part : w.items_batch, max_items, bound, w.ffmid, w.xn,
                                splits, a == 0 ? w.cu_part_live : w.cu_batch_s, a == 0 ? w.nseg_part : w.nseg_batch);
    }
    if (rc) return rc;
    GemmParams o{};
    gemm_into(plan.g[PG_OUT], o, w.ffmid);     // idle between the FFNs (the split attention's partial planes are consumed by now): 4 partial (T,d) planes
    o.A = w.att; o.W = lw.Wout[a]; o.C = w.h; o.bias = lw.bout[a]; o.resid = w.h;
    { ProfScope ps(stream, 2); rc = launch_gemm_f32(stream, plan.g[PG_OUT].epi, o); }
    if (rc) return rc;
  }
  { ProfScope ps(stream, 3); rc = launch_layernorm_affine(stream, w.h, w.xn, TP, d, lw.ffn_g, lw.ffn_b); }
  if (rc) return rc;
  GemmParams f1{};
  gemm_into(plan.g[PG_FF1], f1, nullptr);
  f1.A = w.xn; f1.W = lw.Wff1p; f1.C = w.ffmid; f1.bias = lw.bff1p;
  { ProfScope ps(stream, 2); rc = launch_gemm_f32(stream, plan.g[PG_FF1].epi, f1); }
  if (rc) return rc;
  GemmParams f2{};
  gemm_into(plan.g[PG_FF2], f2, w.qkv);      // idle during the FFN; qkv (3 T d) and att (T d) are adjacent: 4 partial (T,d) planes
  f2.A = w.ffmid; f2.W = lw.Wff2; f2.C = w.h; f2.bias = lw.bff2; f2.resid = w.h;
  { ProfScope ps(stream, 2); rc = launch_gemm_f32(stream, plan.g[PG_FF2].epi, f2); }
  return rc;
}

// ---- one reduced-precision transformer block (layer i): 16-bit MFMA operands, fp32 accumulate, fp32 LN / softmax; ONE kernel sequence
// for the three modes.  bf16 / fp16: one plane per value, residual stream in fp32 or fp16 (w.h16).  Split precision (RAP_DT_F32X2, round 5):
// fp32-accurate products on the fp16 matrix pipe -- the same sequence on paired head / tail operands (pl = 2: physical K = 2 d resp. 8 d),
// per-tensor power-of-two scales, fp32 residual stream, qk-norm always fused, online softmax (probabilities must fit fp16).
// fused: few-token calls (see forward_step) -- every LayerNorm but the first of the forward is then part of the combine pass before it.
static int block_h16(const rap_model* m, const Workspace& w, hipStream_t stream, int i, const float* mod, long mod_stride,
                     const int32_t* token_row, int TP_valid) {
  const int d = m->d, H = m->H, TP = w.rows, dt = w.dtype;
  const CallPlan& plan = w.plan;
  const bool x2 = plan.x2, fused = plan.fused;
  const LayerW& lw = m->layers[i];
  // the 16-bit modes leave every s_* / g_* of LayerWH at 1.f, which are GemmParamsH's own defaults: the scales below are split precision's
  const LayerWH& lh = m->half[dt].layers[i];
  void* const hres = w.h16 ? (void*)w.h16 : (void*)w.h;      // the residual stream as the 16-bit LayerNorms and the residual GEMMs see it
  const int hres_f16 = w.h16 ? 1 : 0;
  auto onto_resid = [&](GemmParamsH& g) { g.C = hres; if (w.h16) g.resid_h = w.h16; else g.resid = w.h; };
  int rc = RAP_OK;
  for (int a = 0; a < 2; ++a) {
    const int j = 2 * i + a;
    if (!fused || j == 0) { ProfScope ps(stream, 3); rc = launch_layernorm_mod_h16(stream, dt, hres, hres_f16, w.xnh, TP, d, mod + (size_t)j * 2 * d, mod_stride, token_row); }
    if (rc) return rc;
    GemmParamsH g{};
    gemm_into(plan.g[PG_QKV], g, nullptr);
    g.A = w.xnh; g.W = lh.Wqkv[a]; g.C = w.qkh; g.heads = H;
    g.vt = w.vth; g.vt_nblk = w.vt_nblk; g.acc_scale = lh.s_qkv[a]; g.out_scale = lh.g_v[a];
    const bool bnd = !x2 && w.qk_norm && m->bounded[j] != 0 && !plan.capped;      // this launch's softmax kernel (per layer and branch)
    const bool prescale = attention_h16_wants_prescaled_q(dt, bnd);
    const float q_mul = prescale ? RAP_QMUL_PRESCALED : 8.0f;
    // (few-token calls: the fused epilogue exists on 128 x 128 tiles too since round 6 -- launch_gemm_h16 picks the tile; until then
    // such calls ran the projection and qk-norm as two kernels, r03 call 32)
    if (plan.g[PG_QKV].epi == EPI_H_QKV_NORM) {
      // qk-norm in the QKV epilogue: one kernel, q / k normalised from the fp32 accumulators (no 16-bit round trip through HBM)
      if (w.qk_norm) { g.gamma_q = lw.gq[a]; g.gamma_k = lw.gk[a]; }      // (split precision) null gains: the epilogue splits q / k as projected
      g.q_mul = q_mul;
      { ProfScope ps(stream, 2); rc = launch_gemm_h16(stream, dt, EPI_H_QKV_NORM, g); }
      if (rc) return rc;
    } else {
      { ProfScope ps(stream, 2); rc = launch_gemm_h16(stream, dt, EPI_H_QKV, g); }
      if (rc) return rc;
      if (w.qk_norm && (rc = launch_qknorm_h16(stream, dt, w.qkh, TP, H, lw.gq[a], lw.gk[a], q_mul))) return rc;
    }
    {
      ProfScope ps(stream, a);
      const AttnWorkItem* items = a == 0 ? w.items_part : w.items_batch;
      const int max_items = a == 0 ? w.max_items_part : w.max_items_batch;
      if (plan.capped) {      // unprescaled q (bnd is false), 256-row items, unsplit
        rc = x2 ? launch_attention_x2_softcap(stream, w.qkh, w.vth, w.vt_nblk, w.atth, TP, H, items, max_items, w.softcap)
                : launch_attention_h16_softcap(stream, dt, w.qkh, w.vth, w.vt_nblk, w.atth, TP, H, items, max_items, w.softcap);
      } else if (x2) {
        // few-token calls: the keys of every work item over 2 / 4 blocks; the partial O planes (4 x TQ x d floats) live in the idle FFN
        // buffer (16 TQ d bytes in this mode), the partial (max, row sum) pairs in the idle LayerNorm-output buffer
        rc = launch_attention_x2(stream, w.qkh, w.vth, w.vt_nblk, w.atth, TP, H, items, max_items, reinterpret_cast<float*>(w.ffmidh),
                                 reinterpret_cast<float*>(w.xnh), plan_attention(plan, H, a, bnd).splits, TP_valid,
                                 a == 0 ? w.cu_part_live : w.cu_batch_s, a == 0 ? w.nseg_part : w.nseg_batch);
      } else {
        rc = launch_attention_h16(stream, dt, w.qkh, w.vth, w.vt_nblk, w.atth, TP, H, items, max_items,
                                  bnd ? m->logit_bound + (size_t)j * H : nullptr, prescale ? 1 : 0, w.attn_bq, w.attn_kg);
      }
    }
    if (rc) return rc;
    GemmParamsH o{};
    gemm_into(plan.g[PG_OUT], o, w.splitk_h);      // (fused: its planes stay in the split-K buffer for the pass below)
    o.A = w.atth; o.W = lh.Wout[a];
    o.bias = lw.bout[a]; o.acc_scale = lh.s_out[a] / lh.g_v[a];      // (the attention output carries V's activation scale)
    onto_resid(o);
    { ProfScope ps(stream, 2); rc = launch_gemm_h16(stream, dt, plan.g[PG_OUT].epi, o); }
    if (rc) return rc;
    if (fused) {      // combine pass + the NEXT LayerNorm in one kernel: adaLN of the per-sample branch after a = 0, the FFN's affine LN after a = 1
      ProfScope ps(stream, 3);
      rc = launch_resid_combine_ln_h16(stream, dt, w.splitk_h, o.force_splits, o.bias, hres, hres_f16, w.xnh, TP, d,
                                       a == 0 ? mod + (size_t)(j + 1) * 2 * d : nullptr, mod_stride, token_row, lw.ffn_g, lw.ffn_b);
      if (rc) return rc;
    }
  }
  if (!fused) { ProfScope ps(stream, 3); rc = launch_layernorm_affine_h16(stream, dt, hres, hres_f16, w.xnh, TP, d, lw.ffn_g, lw.ffn_b); }
  if (rc) return rc;
  GemmParamsH f1{};
  gemm_into(plan.g[PG_FF1], f1, nullptr);
  f1.A = w.xnh; f1.W = lh.Wff1p; f1.C = w.ffmidh;
  f1.bias = lw.bff1p; f1.acc_scale = lh.s_ff1; f1.out_scale = lh.g_ff1;
  { ProfScope ps(stream, 2); rc = launch_gemm_h16(stream, dt, plan.g[PG_FF1].epi, f1); }
  if (rc) return rc;
  GemmParamsH f2{};
  gemm_into(plan.g[PG_FF2], f2, w.splitk_h);      // few-token calls: K split over 2 / 4 blocks per tile (no buffer otherwise)
  f2.A = w.ffmidh; f2.W = lh.Wff2;
  f2.bias = lw.bff2; f2.acc_scale = lh.s_ff2 / lh.g_ff1;
  onto_resid(f2);
  const bool f2_fused = fused && i + 1 < m->L;      // its combine pass is the first LayerNorm of the next layer; the last layer's ff2 combines itself
  if (!f2_fused) { f2.defer_combine = 0; f2.force_splits = 0; }
  { ProfScope ps(stream, 2); rc = launch_gemm_h16(stream, dt, plan.g[PG_FF2].epi, f2); }
  if (rc) return rc;
  if (f2_fused) {
    ProfScope ps(stream, 3);
    rc = launch_resid_combine_ln_h16(stream, dt, w.splitk_h, f2.force_splits, f2.bias, hres, hres_f16, w.xnh, TP, d,
                                     mod + (size_t)(2 * i + 2) * 2 * d, mod_stride, token_row, nullptr, nullptr);
  }
  return rc;
}

// mod: (scale|shift) rows for this forward: row r at mod + r*mod_stride, LN j at + j*2d.
static int forward_step(const rap_model* m, const Workspace& w, hipStream_t stream, const float* x_t, const float* mod,
                        long mod_stride, const int32_t* token_row, int TP_valid, float* v_out, float* feats_out) {
  const int d = m->d;
  int rc;
  // embed = PE63(x_t) Wx^T + base
  { ProfScope ps(stream, 4); rc = launch_posenc_x(stream, x_t, w.ax, TP_valid); }
  if (rc) return rc;
  // From here to the head every kernel runs over TQ = align_up(TP, 256) rows of the workspace (filler rows: prepare_static):
  // the GEMMs see M % 256 == 0 whatever the batch, i.e. the persistent 256 x 256 kernels; the attention launches take TQ as the
  // row count of the head-major planes and their work lists (true segment ends) for everything else.
  const int TP = w.rows;
  {
    GemmParams g{};
    gemm_into(w.plan.g[PG_EMBED], g, nullptr);
    // 16-bit residual stream: the fp32 embedding lands in the (idle) FFN buffer and is rounded to fp16 once
    g.A = w.ax; g.W = m->Wx; g.C = w.h16 ? w.hid1 : w.h; g.resid = w.base;
    if ((rc = launch_gemm_f32(stream, w.plan.g[PG_EMBED].epi, g))) return rc;
    if (w.h16 && (rc = launch_convert_f16_sat(stream, w.hid1, w.h16, (size_t)TP * d))) return rc;
  }
  // (few-token calls of the 16-bit / split-precision blocks fold every combine pass into the following LayerNorm: plan_call, CallPlan::fused)
  for (int i = 0; i < m->L; ++i) {
    rc = w.dtype == RAP_DT_F32 ? block_f32(m, w, stream, i, mod, mod_stride, token_row)
                               : block_h16(m, w, stream, i, mod, mod_stride, token_row, TP_valid);
    if (rc) return rc;
  }
  // 16-bit residual stream: the fp32 head (and the caller's transformer_features) read an fp32 image of it -- written into the
  // caller's feature buffer when there is one, else into the q / k planes (T x 2d 16-bit values = T x d floats, dead after the last attention)
  const float* h_final = w.h;
  int head_rows = TP;                       // the head's first GEMM reads TQ rows of a workspace buffer, TP_valid rows of a caller's
  if (w.h16) {
    float* img = feats_out ? feats_out : reinterpret_cast<float*>(w.qkh);
    if (feats_out) head_rows = TP_valid;
    if ((rc = launch_convert_f16_to_f32(stream, w.h16, img, (size_t)head_rows * d))) return rc;
    h_final = img;
  } else if (feats_out) {
    if (hipMemcpyAsync(feats_out, w.h, (size_t)TP_valid * d * sizeof(float), hipMemcpyDeviceToDevice, stream) != hipSuccess) {
      rap_set_last_hip_error((int)hipGetLastError());
      return RAP_ERR_HIP;
    }
  }
  // final_mlp (point_cloud_dit.py:111-117): Lin+act, Lin+act, Lin(no bias); act = final_mlp_act (SiLU unless rap_model_set_final_act says otherwise)
  // few-token calls: K of the two hidden layers over 2 / 4 blocks per tile; the partial planes live in the FFN buffer of the fp32 layout
  // (4 T d floats, idle here) resp. the split-K planes of the 16-bit layouts (plan_call).  The plan's M is TQ; head_rows differs from it only
  // for a caller's feature buffer of the fp16 stream (ragged M = TP_valid on planes sized for TQ)
  float* const head_ws = w.dtype == RAP_DT_F32 ? w.ffmid : w.splitk_h;
  GemmParams h0{};
  gemm_into(w.plan.g[PG_HEAD0], h0, head_ws);
  h0.A = h_final; h0.W = m->hW0; h0.C = w.hid1; h0.M = head_rows; h0.bias = m->hb0;
  if ((rc = launch_gemm_f32(stream, w.plan.g[PG_HEAD0].epi, h0))) return rc;
  GemmParams h2{};
  gemm_into(w.plan.g[PG_HEAD1], h2, head_ws);
  h2.A = w.hid1; h2.W = m->hW2; h2.C = w.hid2; h2.M = head_rows; h2.bias = m->hb2;
  if ((rc = launch_gemm_f32(stream, w.plan.g[PG_HEAD1].epi, h2))) return rc;
  return launch_head_out3(stream, w.hid2, d / 2, m->hW4, v_out, TP_valid, d / 2);
}

extern "C" int rap_dit_forward(const rap_model* m, const float* x_t, const float* timesteps, const float* cond,
                               const float* feat, const float* scales, const uint8_t* anchor, const int32_t* cu_batch,
                               const int32_t* cu_part, int32_t B, int32_t VP, int64_t TP, float* v_out, float* feats_out,
                               void* ws, size_t ws_bytes, void* stream_) {
  return rap_dit_forward_latent(m, x_t, timesteps, cond, feat, nullptr, scales, anchor, cu_batch, cu_part, B, VP, TP, v_out, feats_out, ws, ws_bytes, stream_);
}
extern "C" int rap_dit_forward_latent(const rap_model* m, const float* x_t, const float* timesteps, const float* cond,
                                      const float* feat, const float* latent, const float* scales, const uint8_t* anchor, const int32_t* cu_batch,
                                      const int32_t* cu_part, int32_t B, int32_t VP, int64_t TP, float* v_out, float* feats_out,
                                      void* ws, size_t ws_bytes, void* stream_) {
  if (!m || !x_t || !timesteps || !cond || !scales || !anchor || !cu_batch || !cu_part || !v_out) return RAP_ERR_INVALID;
  if (m->F > 0 && !feat) return RAP_ERR_INVALID;
  if ((m->Din > 0) != (latent != nullptr)) return RAP_ERR_INVALID;      // a model built with in_dim > 0 needs its latent features, one without takes none
  if (B <= 0 || VP < 0 || TP < 0 || TP > 0x7fffffffLL / 8) return RAP_ERR_INVALID;
  if (TP == 0) return RAP_OK;
  if (!ws) return RAP_ERR_WORKSPACE;
  // the configuration (compute / residual dtype, qk_norm) is snapshotted into the workspace descriptor under the model's mutex; the enqueue
  // itself runs unlocked, so threads sharing a model do not serialise on a (possibly queue-bound) enqueue
  Workspace w;
  { std::lock_guard<std::mutex> lock(m->cfg_mu); w = carve_workspace(call_shape(m, TP, B, VP, B), (char*)ws); }
  if (w.total > ws_bytes) return RAP_ERR_WORKSPACE;
  w.cu_part_live = w.cu_part_s;             // prepare_static sanitises the caller's part table into it
  hipStream_t stream = (hipStream_t)stream_;
  int rc;
  if ((rc = prepare_static(m, w, stream, cond, feat, scales, anchor, cu_batch, cu_part, B, VP, (int)TP, latent))) return rc;
  if ((rc = launch_adaln_table(stream, timesteps, B, 2 * m->L, m->d, m->adaW1, m->adab1, m->adaW2, m->adab2, m->adaW3,
                               m->adab3, w.ada_scratch, w.mod)))
    return rc;
  return forward_step(m, w, stream, x_t, w.mod, (long)2 * m->L * 2 * m->d, w.token_sample, (int)TP, v_out, feats_out);
}

// kernel-level: the adaLN modulation table of this model for `rows` timesteps
extern "C" int rap_adaln_table(const rap_model* m, const float* t, int32_t rows, float* scratch, float* out, void* stream) {
  if (!m || !t || !scratch || !out || rows < 0) return RAP_ERR_INVALID;
  return launch_adaln_table((hipStream_t)stream, t, rows, 2 * m->L, m->d, m->adaW1, m->adab1, m->adaW2, m->adab2, m->adaW3,
                            m->adab3, scratch, out);
}

extern "C" int rap_euler_step(const float* x_t, const float* v, float t, float dt, float* x0_hat, float* x_next,
                              float* traj_xt_slot, int64_t n, void* stream) {
  if (!x_t || !v || !x0_hat || !x_next || n < 0) return RAP_ERR_INVALID;
  return launch_euler_step((hipStream_t)stream, x_t, v, t, dt, x0_hat, x_next, traj_xt_slot, (long)n);
}

// ---------------------------------------------------------------------------------------------
// procrustes entry points
// ---------------------------------------------------------------------------------------------
struct ProcWs { int32_t* off; double* partials; float* Rc; float* tc; size_t total; };
static ProcWs carve_proc(int nparts, char* basep) {
  ProcWs p; Carver c(basep);
  p.off = (int32_t*)c.take(((size_t)nparts + 1) * 4);
  p.partials = (double*)c.take((size_t)nparts * RAP_PROC_CHUNKS * 16 * 8);
  p.Rc = (float*)c.take((size_t)nparts * 9 * 4);
  p.tc = (float*)c.take((size_t)nparts * 3 * 4);
  p.total = c.total();
  return p;
}
extern "C" size_t rap_procrustes_workspace_bytes(int32_t nparts) { return nparts < 0 ? 0 : carve_proc(nparts, nullptr).total; }

// what the three entry points below start with: shape checks, the carved workspace, the parts' point offsets
static int proc_begin(hipStream_t stream, const int64_t* points_per_part, int32_t B, int32_t P, void* ws, size_t ws_bytes, ProcWs* p) {
  if (B <= 0 || P <= 0 || (int64_t)B * P > 65535) return RAP_ERR_INVALID;
  if (!ws) return RAP_ERR_WORKSPACE;
  *p = carve_proc(B * P, (char*)ws);
  if (p->total > ws_bytes) return RAP_ERR_WORKSPACE;
  return launch_part_offsets(stream, points_per_part, B * P, p->off);
}

extern "C" int rap_fit_transformations(const float* src, const float* tgt, const int64_t* points_per_part, int32_t B,
                                       int32_t P, float* R_out, float* t_out, void* ws, size_t ws_bytes, void* stream_) {
  if (!src || !tgt || !points_per_part || !R_out || !t_out) return RAP_ERR_INVALID;
  hipStream_t stream = (hipStream_t)stream_;
  ProcWs p;
  int rc;
  if ((rc = proc_begin(stream, points_per_part, B, P, ws, ws_bytes, &p))) return rc;
  return launch_procrustes_fit(stream, src, tgt, p.off, B * P, R_out, t_out, p.partials);
}

extern "C" int rap_rigidify(const float* prediction, const float* condition, const int64_t* points_per_part, int32_t B,
                            int32_t P, float* out, void* ws, size_t ws_bytes, void* stream_) {
  if (!prediction || !condition || !points_per_part || !out) return RAP_ERR_INVALID;
  hipStream_t stream = (hipStream_t)stream_;
  ProcWs p;
  int rc;
  if ((rc = proc_begin(stream, points_per_part, B, P, ws, ws_bytes, &p))) return rc;
  if ((rc = launch_procrustes_fit(stream, condition, prediction, p.off, B * P, p.Rc, p.tc, p.partials))) return rc;
  return launch_rigid_apply(stream, condition, p.Rc, p.tc, p.off, B * P, out, nullptr, 0.f, 0.f, nullptr, 0);
}

extern "C" int rap_rigidify_blend(const float* x0_hat, const float* condition, const int64_t* points_per_part, int32_t B,
                                  int32_t P, const float* x_1, float w0, float w1, float* x_t_out, void* ws, size_t ws_bytes,
                                  void* stream_) {
  if (!x0_hat || !condition || !points_per_part || !x_1 || !x_t_out) return RAP_ERR_INVALID;
  hipStream_t stream = (hipStream_t)stream_;
  ProcWs p;
  int rc;
  if ((rc = proc_begin(stream, points_per_part, B, P, ws, ws_bytes, &p))) return rc;
  if ((rc = launch_procrustes_fit(stream, condition, x0_hat, p.off, B * P, p.Rc, p.tc, p.partials))) return rc;
  return launch_rigid_apply(stream, condition, p.Rc, p.tc, p.off, B * P, x_t_out, x_1, w0, w1, nullptr, 1);
}

// ---------------------------------------------------------------------------------------------
// the whole sampling loop
// ---------------------------------------------------------------------------------------------
__global__ void tgrid_kernel(float* t, int steps, double dt) {
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s < steps) t[s] = (float)(1.0 - (double)s * dt);   // t = 1 - step*dt in double (sampler.py:42,55), cast at torch.full
}

extern "C" int rap_sample(const rap_model* m, const float* cond, const float* feat, const float* scales,
                          const uint8_t* anchor, const int64_t* points_per_part, const int32_t* cu_batch, const float* x_1,
                          int32_t B, int32_t P, int64_t TP, int32_t num_steps, int32_t rigidity_forcing, float* traj_x0,
                          float* traj_xt, float* R_out, float* t_out, float* feats_out, void* ws, size_t ws_bytes,
                          void* stream_) {
  return rap_sample_latent(m, cond, feat, nullptr, scales, anchor, points_per_part, cu_batch, x_1, B, P, TP, num_steps, rigidity_forcing, traj_x0,
                           traj_xt, R_out, t_out, feats_out, ws, ws_bytes, stream_);
}
extern "C" int rap_sample_latent(const rap_model* m, const float* cond, const float* feat, const float* latent, const float* scales,
                                 const uint8_t* anchor, const int64_t* points_per_part, const int32_t* cu_batch, const float* x_1,
                                 int32_t B, int32_t P, int64_t TP, int32_t num_steps, int32_t rigidity_forcing, float* traj_x0,
                                 float* traj_xt, float* R_out, float* t_out, float* feats_out, void* ws, size_t ws_bytes,
                                 void* stream_) {
  if (!m || !cond || !scales || !anchor || !points_per_part || !cu_batch || !x_1 || !traj_x0 || !traj_xt || !R_out || !t_out)
    return RAP_ERR_INVALID;
  if (m->F > 0 && !feat) return RAP_ERR_INVALID;
  if ((m->Din > 0) != (latent != nullptr)) return RAP_ERR_INVALID;
  if (B <= 0 || P <= 0 || TP <= 0 || num_steps <= 0 || TP > 0x7fffffffLL / 8 || (int64_t)B * P > 65535) return RAP_ERR_INVALID;
  const int np = B * P;
  if (!ws) return RAP_ERR_WORKSPACE;
  Workspace w;
  { std::lock_guard<std::mutex> lock(m->cfg_mu); w = carve_workspace(call_shape(m, TP, B, np, num_steps), (char*)ws); }      // see rap_dit_forward
  if (w.total > ws_bytes) return RAP_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  const int T = (int)TP;
  const long n3 = (long)TP * 3;
  int rc;
  if ((rc = launch_part_offsets(stream, points_per_part, np, w.part_offsets, (long)TP))) return rc;
  if ((rc = prepare_static(m, w, stream, cond, feat, scales, anchor, cu_batch, w.part_offsets, B, np, T, latent))) return rc;
  // t is uniform over the batch inside the sampler (modeling.py:674), so the adaLN table is computed once for
  // ALL flow steps (row s = step s) instead of per sample per step.
  const double dt = 1.0 / (double)num_steps;
  hipLaunchKernelGGL(tgrid_kernel, dim3((num_steps + 63) / 64), dim3(64), 0, stream, w.tgrid, num_steps, dt);
  RAP_LAUNCH_CHECK();
  if ((rc = launch_adaln_table(stream, w.tgrid, num_steps, 2 * m->L, m->d, m->adaW1, m->adab1, m->adaW2, m->adab2,
                               m->adaW3, m->adab3, w.ada_scratch, w.mod)))
    return rc;
  RAP_HIP_CHECK(hipMemcpyAsync(w.xt, x_1, (size_t)n3 * sizeof(float), hipMemcpyDeviceToDevice, stream));
  const size_t mod_step = (size_t)2 * m->L * 2 * m->d;
  for (int s = 0; s < num_steps; ++s) {
    const double t = 1.0 - (double)s * dt;
    float* x0_slot = traj_x0 + (size_t)s * n3;
    float* xt_slot = traj_xt + (size_t)s * n3;
    float* feats = (feats_out && s == num_steps - 1) ? feats_out : nullptr;
    if ((rc = forward_step(m, w, stream, w.xt, w.mod + (size_t)s * mod_step, 0, nullptr, T, w.v, feats))) return rc;
    { ProfScope ps(stream, 5); rc = launch_euler_step(stream, w.xt, w.v, (float)t, (float)dt, x0_slot, w.xt, rigidity_forcing ? nullptr : xt_slot, n3); }
    if (rc) return rc;
    if (rigidity_forcing) {
      { ProfScope ps(stream, 6); rc = launch_procrustes_fit(stream, cond, x0_slot, w.part_offsets, np, w.Rc, w.tc, w.proc_partials); }
      if (rc) return rc;
      const float w0 = (float)(1.0 - t + dt), w1 = (float)(t - dt);
      { ProfScope ps(stream, 7); rc = launch_rigid_apply(stream, cond, w.Rc, w.tc, w.part_offsets, np, w.xt, x_1, w0, w1, xt_slot, 1); }
      if (rc) return rc;
    }
  }
  // final poses (modeling.py:389-391): fit_transformations(cond, trajs[-1])
  return launch_procrustes_fit(stream, cond, traj_x0 + (size_t)(num_steps - 1) * n3, w.part_offsets, np, R_out, t_out,
                               w.proc_partials);
}

