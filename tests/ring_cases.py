"""The cases and the CPU references that the host and the GPU tests of the kernels BETWEEN the GEMMs share
(tests/test_ring_cases_host.py, tests/test_ring_edges_gpu.py): the fp32 LayerNorm, both qk-norms, the positional-encoding builders, the
adaLN table, the head tail, the Euler update, the 16-bit and split-precision conversions, max |x|, the segment-table sanitiser, the logit
bound of the bounded softmax and the GEGLU interleave.  Pure torch, seeded, cached: nothing here touches a GPU.

Every size-dependent path of these kernels is launch arithmetic, restated below next to the kernel it belongs to (rows per block, grid
caps, lanes per row, rows per chunk); the host test computes from it that every case reaches what it is listed for.

References are fp64 evaluations of the oracle's formula on the same fp32 (or 16-bit) inputs, or exact (bitwise) where the operation is.
The bounds are the suite's own (tests/test_kernels_gpu.py, tests/test_h16_gpu.py, tests/test_x2_gpu.py; restated here, the host test
asserts they are the same numbers) -- with one addition, for the LayerNorm rows whose mean dwarfs their spread (ln_bound).
"""
import collections
import functools
import math
import zlib

import torch
import torch.nn.functional as F

import ln_stream_cases as L
from oracle import rap_oracle as O

# restated from tests/test_kernels_gpu.py
GEMM_BOUND = 2e-5
NORM_BOUND = 1e-5
POSENC_BOUND = 1e-6
ADALN_BOUND = 2e-6
# restated from tests/test_h16_gpu.py (through ln_stream_cases, which restates them too)
ULP, ONE_ROUNDING, NORM_SLACK, TORCH_DT = L.ULP, L.ONE_ROUNDING, L.NORM_SLACK, L.TORCH_DT
F16_MAX = 65504.0
INT32_MAX = 2 ** 31 - 1
_I = float("inf")


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def bits32(t):
    return t.contiguous().view(torch.int32)


def same_bits_or_both_nan(a, b):
    """bitwise equality of two float tensors of one type, a NaN on both sides counting as equal whatever its payload"""
    ia, ib = (t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32) for t in (a, b))
    return bool(((ia == ib) | (torch.isnan(a) & torch.isnan(b))).all())


# ---------------------------------------------------------------------------------------------
# fp32 LayerNorm (norm.hip layernorm_kernel<NV>: one wave per row, 4 rows per block, NV = d / 256 float4 per lane)
# ---------------------------------------------------------------------------------------------
LN_WIDTHS = [256, 512, 768, 1024]
LN_ROWS = L.ROWS                                  # every tail of the 4-rows-per-block launch, one and several blocks
LN_FORMS = L.FORMS                                # mod_rows (token_row given), mod (token_row NULL), affine
LN_FAMILIES = ["benign", "mean50", "mean1000", "const", "zero", "tiny", "huge", "outlier"]
LN_CONST = 3.25
LN_EXACT = ("const", "zero")                      # x - mean is exactly 0 in fp32: the output IS the shift
# How far inside ln_bound torch's own fp32 LayerNorm has to sit, per family (the host test).  2 everywhere but on the outlier rows: there
# the error of ANY fp32 evaluation is the rounding of an output of sqrt(d) |multiplier| = 43 (three roundings and rstd's own, about 3 ulp
# of 3.8e-6 = 1.1e-5), which the bound's second term (the cancellation in x - mean: 1.0e-5 there) does not model.  Measured: 0.52 of the
# bound at (d 1024, 5 rows), 0.46 at most on every other family.  The GPU test holds the kernel to the bound itself on every family.
LN_YARDSTICK_MARGIN = {f: 2.0 for f in LN_FAMILIES}
LN_YARDSTICK_MARGIN["outlier"] = 1.5


@functools.lru_cache(maxsize=16)
def ln_input(d, rows, family):
    """(rows, d) fp32, every row of one family"""
    if family == "benign":
        return L.stream_input(d, rows)            # randn * 3 + 0.5: the distribution the suite ran before
    z = torch.randn(rows, d, generator=_gen("ln", d, rows, family))
    if family == "mean50":
        return z + 50.0
    if family == "mean1000":
        return z + 1000.0                         # E[x^2] - mean^2 in fp32 is off by 3 % here
    if family == "const":
        return torch.full((rows, d), LN_CONST)
    if family == "zero":
        return torch.zeros(rows, d)
    if family == "tiny":
        return z * 1e-4                           # var 1e-8 << eps 1e-5
    if family == "huge":
        return z * 1e6
    assert family == "outlier"
    z[torch.arange(rows), ln_outlier_column(d, torch.arange(rows))] = 1e4
    return z


def ln_outlier_column(d, row):
    """another column in every row, over all lanes and all float4 slots of a lane"""
    return (row * 37 + 5) % d


@functools.lru_cache(maxsize=None)
def ln_params(d):
    """-> (mod (3, 4, 2 d), gain (d), shift (d)), distinct per column; the table has the shape of ln_stream_cases.ln_params.  Multipliers
    stay within 1 +- 0.4 (table randn * 0.1, gain 0.75 + rand / 2): an outlier row normalises to sqrt(d) = 32 at d = 1024, and the three fp32
    roundings of an output of 32 |multiplier| (ulp 3.8e-6) are no part of ln_bound's cancellation term -- see LN_YARDSTICK_MARGIN."""
    g = _gen("ln params", d)
    mod = torch.randn(L.TABLE_ROWS, L.TABLE_SLOTS, 2 * d, generator=g) * 0.1
    return mod, torch.rand(d, generator=g) * 0.5 + 0.75, torch.randn(d, generator=g)


def ln_modulation(form, d, rows, dt=torch.float32):
    """-> (multiplier, shift) of the normalised rows, (rows, d) or (d), formed in `dt` from the fp32 tables"""
    mod, gain, shift = (t.to(dt) for t in ln_params(d))
    if form == "affine":
        return gain, shift
    t = L.token_rows(rows).long() if form == "mod_rows" else torch.zeros(rows, dtype=torch.long)
    return 1 + mod[t, L.MOD_SLOT, :d], mod[t, L.MOD_SLOT, d:]


def ln_ref64(x, form):
    rows, d = x.shape
    mul, add = ln_modulation(form, d, rows, torch.float64)
    return F.layer_norm(x.double(), (d,), eps=1e-5) * mul + add


def ln_ref32(x, form):
    """the yardstick of the host test: torch's fp32 LayerNorm (two passes over the row) with fp32 modulation"""
    rows, d = x.shape
    mul, add = ln_modulation(form, d, rows)
    return F.layer_norm(x, (d,), eps=1e-5) * mul + add


def ln_one_pass32(x, form):
    """what the sweep is there to catch: var = E[x^2] - mean^2 in fp32"""
    rows, d = x.shape
    mul, add = ln_modulation(form, d, rows)
    mean = x.mean(dim=1, keepdim=True)
    var = ((x * x).mean(dim=1, keepdim=True) - mean * mean).clamp_min(0)
    return (x - mean) * (1.0 / torch.sqrt(var + 1e-5)) * mul + add


def ln_bound(x, form):
    """NORM_BOUND + 4 * 2^-24 * max|x| * max rstd * max|multiplier|: the second term is the cancellation in x - mean (mean carries a relative
    error of a few 2^-24, so x - mean an absolute one of that times |x|, which rstd and the multiplier scale) and nothing else.  It is below
    NORM_BOUND / 10 on the benign rows."""
    rows, d = x.shape
    mul, _ = ln_modulation(form, d, rows, torch.float64)
    rstd = 1.0 / torch.sqrt(x.double().var(dim=1, unbiased=False) + 1e-5)
    return NORM_BOUND + 4 * 2.0 ** -24 * float(x.abs().max()) * float(rstd.max()) * float(mul.abs().max())


def ln_shift_rows(form, d, rows):
    """(rows, d) fp32: what a row with x - mean == 0 must come out as"""
    _, add = ln_modulation(form, d, rows)
    return add.expand(rows, d).contiguous()


# ---------------------------------------------------------------------------------------------
# qk-norm (norm.hip qknorm_kernel: 16 lanes per row of 64, 16 rows per block; norm_h16.hip qknorm_h16_kernel: 8 lanes, 32 rows per block;
# both over the 2 * H * TP rows of the q and k planes, head = (row in plane) / TP)
# ---------------------------------------------------------------------------------------------
QK_HEADS = [1, 3, 8, 16]
QK_ROWS = [1, 15, 16, 17, 31, 33, 1027]
QK_ROWS_PER_BLOCK = {0: 16, 1: 32, 2: 32}         # mode 0 = fp32, 1 = bf16, 2 = fp16
QK_KINDS = ["plain", "zero", "onehot", "plain", "tiny", "plain", "huge", "plain", "plain", "plain", "plain"]
# scale of the tiny / huge rows.  fp32 and bf16: 1e-15 and 1e15 (the squares stay inside fp32; below 1e-12 the row norm meets the eps
# clamp).  fp16 cannot hold either: its rows sit at the two ends of ITS range (subnormals at 2^-20; 2^11 times |N(0, 2)| < 65504).
QK_SCALES = {0: (1e-15, 1e15), 1: (1e-15, 1e15), 2: (2.0 ** -20, 2.0 ** 11)}


def qk_kind(plane, flat_row):
    return QK_KINDS[(flat_row * 7 + plane * 3) % len(QK_KINDS)]


@functools.lru_cache(maxsize=None)
def qk_gammas(H):
    """-> (gamma_q, gamma_k) (H, 64): distinct per head, plane and column, every third column negative"""
    g = _gen("qk gamma", H)
    sign = torch.where(torch.arange(64) % 3 == 1, -1.0, 1.0)
    return (torch.rand(H, 64, generator=g) + 0.5) * sign, (torch.rand(H, 64, generator=g) + 0.5) * sign.flip(0)


@functools.lru_cache(maxsize=8)
def qk_input(H, TP, mode):
    """(3, H, TP, 64) in the type of `mode`: q and k planes with the special rows, and a third plane no kernel may touch (fp32: v)"""
    x = torch.randn(3, H, TP, 64, generator=_gen("qk", H, TP)) * 2
    tiny, huge = QK_SCALES[mode]
    for plane in range(2):
        flat = x[plane].view(H * TP, 64)
        for r in range(H * TP):
            kind = qk_kind(plane, r)
            if kind == "zero":
                flat[r] = 0.0
            elif kind == "onehot":
                flat[r] = 0.0
                flat[r, (r * 5 + 1) % 64] = -3.0 if r % 2 else 3.0
            elif kind == "tiny":
                flat[r] *= tiny
            elif kind == "huge":
                flat[r] *= huge
    return x if mode == 0 else x.to(TORCH_DT[mode])


def qk_ref64(x):
    """fp64 MultiHeadRMSNorm of the q and k planes of qk_input (the oracle's formula: normalize(eps 1e-12) * gamma * 8)"""
    H = x.shape[1]
    gq, gk = qk_gammas(H)
    xd = x.double()
    q = O.multi_head_rms_norm(xd[0].permute(1, 0, 2), gq.double()).permute(1, 0, 2)
    k = O.multi_head_rms_norm(xd[1].permute(1, 0, 2), gk.double()).permute(1, 0, 2)
    return torch.stack([q, k])


def qk_ref32(x, mode):
    """plain fp32 evaluation of the kernel's formula on the stored inputs, rounded once into the type -> fp64"""
    H = x.shape[1]
    g = torch.stack(qk_gammas(H))[:, :, None, :]
    xf = x[:2].float()
    nrm = torch.sqrt((xf * xf).sum(dim=-1, keepdim=True)).clamp_min(1e-12)
    o = xf / nrm * g * 8.0
    return (o if mode == 0 else o.to(TORCH_DT[mode])).double()


def qk_error(mode, got, ref, H):
    """-> (worst error, bound) in the measure the suite holds this output to"""
    if mode == 0:
        gmax = max(float(g.abs().max()) for g in qk_gammas(H))
        return float((got.double() - ref).abs().max()), NORM_BOUND * gmax
    return float(((got.double() - ref).abs() / (ref.abs() + 1e-2)).max()), ONE_ROUNDING * ULP[mode] + NORM_SLACK


def qk_blocks_straddling(H, TP, mode):
    """-> (some block holds rows of two heads of one plane, some block holds rows of the q AND the k plane), from the launch arithmetic"""
    rb, rows = QK_ROWS_PER_BLOCK[mode], H * TP
    two_heads = two_planes = False
    for b0 in range(0, 2 * rows, rb):
        owners = {(r // rows, (r % rows) // TP) for r in range(b0, min(b0 + rb, 2 * rows))}
        two_planes |= len({p for p, _ in owners}) > 1
        two_heads |= any(len({h for p, h in owners if p == plane}) > 1 for plane in (0, 1))
    return two_heads, two_planes


# ---------------------------------------------------------------------------------------------
# positional encodings (embed.hip: posenc_x_kernel 16 threads per token = 16 tokens per block, posenc_static_kernel 32 threads per token
# = 8 tokens per block; thread 31 also writes columns 124..127, every feature float4 is predicated on fc < F)
# ---------------------------------------------------------------------------------------------
PE_ROWS = [1, 7, 8, 9, 15, 16, 17, 1027]
PE_MAGNITUDES = [1e-3, 1.0, 6.0, 100.0]           # 2^9 * 100 = 51 200 rad
PE_FEAT_DIMS = [0, 4, 8, 32, 36, 40]
PE_SAMPLES = 3
PE_SCALES = torch.tensor([5.0, 50.0, 23.456789])  # in [5, 50], both ends


@functools.lru_cache(maxsize=None)
def pe_coords(TP, which):
    """(TP, 3) fp32: row r at magnitude PE_MAGNITUDES[r % 4] (signed, uniform), with exact +0 and -0 coordinates"""
    g = _gen("pe", TP, which)
    x = (torch.rand(TP, 3, generator=g) * 2 - 1) * torch.tensor(PE_MAGNITUDES)[torch.arange(TP) % 4][:, None]
    for r in range(0, TP, 5):
        x[r, r % 3] = 0.0 if (r // 5) % 2 == 0 else -0.0
    return x


def pe_token_sample(TP):
    """2, 1, 0, 2, ...: not monotone over the 3 samples"""
    return ((2 - torch.arange(TP)) % PE_SAMPLES).to(torch.int32)


@functools.lru_cache(maxsize=None)
def pe_feat(TP, Fd):
    return torch.randn(TP, Fd, generator=_gen("pe feat", TP, Fd)) if Fd else None


def pe_x_ref64(x):
    """(TP, 64) fp64: O.posenc on the exact fp32 argument (2^k x is exact), pad column 63 zero"""
    return torch.cat([O.posenc(x.double()), torch.zeros(x.shape[0], 1, dtype=torch.float64)], dim=1)


def pe_static_ref64(cond, Fd):
    TP = cond.shape[0]
    sc = PE_SCALES[pe_token_sample(TP).long()]
    parts = [O.posenc(cond.double()), O.posenc(sc.double().unsqueeze(-1))] + ([pe_feat(TP, Fd).double()] if Fd else [])
    ref = torch.cat(parts, dim=1)
    return torch.cat([ref, torch.zeros(TP, 128 - ref.shape[1], dtype=torch.float64)], dim=1)


def pe_x_ref32(x):
    return torch.cat([O.posenc(x), torch.zeros(x.shape[0], 1)], dim=1)


def pe_static_ref32(cond, Fd):
    TP = cond.shape[0]
    sc = PE_SCALES[pe_token_sample(TP).long()]
    parts = [O.posenc(cond), O.posenc(sc.unsqueeze(-1))] + ([pe_feat(TP, Fd)] if Fd else [])
    ref = torch.cat(parts, dim=1)
    return torch.cat([ref, torch.zeros(TP, 128 - ref.shape[1])], dim=1)


def pe_raw_columns_x():
    return [0, 1, 2]


def pe_raw_columns_static(Fd):
    return [0, 1, 2, 63] + list(range(84, 84 + Fd))


def pe_columns_of_component(c):
    """the columns of a PE63 block that depend on coordinate c: the raw value, and sin / cos at every frequency"""
    return [c] + [3 + 6 * j + c for j in range(10)] + [3 + 6 * j + 3 + c for j in range(10)]


# ---------------------------------------------------------------------------------------------
# adaLN table (adaln.hip small_linear_kernel: one wave per output feature, rows in chunks of 8 with per-row predicates)
# ---------------------------------------------------------------------------------------------
ADALN_MODELS = [(256, 1), (256, 2), (1024, 1), (1024, 2)]      # (d, L)
ADALN_ROWS = [1, 7, 8, 9, 16, 17, 33]
ADALN_CHUNK = 8
ADALN_T8 = [1.0, 1e-3, 0.0, 0.5, 0.5, 0.95, 0.05, 0.3]          # tiled: row i and row i + 8 carry the same t


def adaln_t(rows):
    return torch.tensor([ADALN_T8[i % ADALN_CHUNK] for i in range(rows)])


def adaln_cfg(d, L_):
    from rap_amd import synthetic as S
    cfg = dict(S.RAP_12)
    cfg.update(embed_dim=d, num_heads=d // 64, num_layers=L_, local_feat_dim=8)
    return cfg


@functools.lru_cache(maxsize=1)
def adaln_weights(d, L_):
    from rap_amd import synthetic as S
    return S.make_weights(adaln_cfg(d, L_), 4)


def adaln_ref(sd, L_, t, dt=torch.float64):
    """(rows, 2 L, 2 d) in `dt`: O.adaln_scale_shift for every adaptive LayerNorm, in the table's order"""
    sdt = {k: v.to(dt) for k, v in sd.items() if "prenorm" in k}
    out = []
    for i in range(L_):
        for which in ("self", "global"):
            out.append(torch.cat(O.adaln_scale_shift(sdt, f"transformer_layers.{i}.{which}_prenorm.", t), dim=-1))
    return torch.stack(out, dim=1)


# ---------------------------------------------------------------------------------------------
# head tail (sampler_kernels.hip head_out3_kernel: one wave per token, k = lane * 4; k < K; k += 256; at most 8192 blocks of 4 waves)
# ---------------------------------------------------------------------------------------------
HEAD_KS = [128, 256, 384, 512]
HEAD_LD_EXTRA = [0, 64]
HEAD_ROWS = [1, 3, 4, 5, 32768, 32769, 40001]
HEAD_WAVES = 8192 * 4


@functools.lru_cache(maxsize=1)
def _head_base(TP):
    return torch.randn(TP, max(HEAD_KS) + max(HEAD_LD_EXTRA), generator=_gen("head", TP))


def head_inputs(TP, K, extra):
    """-> (y (TP, K + extra) whose columns beyond K are NaN -- nothing may read them, W (3, K) with distinct rows)"""
    y = _head_base(TP)[:, :K + extra].clone()
    y[:, K:] = float("nan")
    return y, torch.randn(3, K, generator=_gen("head W", K)) / K ** 0.5


def head_ref64(y, W):
    K = W.shape[1]
    return y[:, :K].double() @ W.double().T


def head_lane_trips(K):
    """-> sorted set of loop trip counts over the 64 lanes"""
    return sorted({len(range(lane * 4, K, 256)) for lane in range(64)})


# ---------------------------------------------------------------------------------------------
# Euler update (euler_step_kernel: grid-stride, at most 2048 blocks of 256)
# ---------------------------------------------------------------------------------------------
EULER_NS = [1, 255, 256, 257, 524288, 524289, 786432]
EULER_THREADS = 2048 * 256
EULER_FORMS = ["separate", "in_place", "trajectory"]     # in_place: x_next == x_t and no trajectory slot, as rap_sample calls it
EULER_T, EULER_DT = 1 - 3 * (1.0 / 20), 1.0 / 20


@functools.lru_cache(maxsize=2)
def euler_inputs(n):
    g = _gen("euler", n)
    return torch.randn(n, generator=g), torch.randn(n, generator=g)


def euler_ref(x, v):
    """-> (x_next, x0_hat), bitwise: fp32 tensor ops with separate multiply and subtract roundings"""
    return O.euler_step(x, EULER_T, EULER_DT, lambda a, b: v)


# ---------------------------------------------------------------------------------------------
# fp32 -> 16 bit (gemm_h16.hip convert_h16_kernel: 4 values per thread, at most 65 536 blocks of 256)
# ---------------------------------------------------------------------------------------------
CONVERT_PASS = 65536 * 256                                # threads of one pass of the three capped conversion / pack grids
CONVERT_WRAP_N = CONVERT_PASS * 4 + 4 * 256 * 3 + 4


@functools.lru_cache(maxsize=2)
def convert_table(dt):
    """fp32 inputs of the conversion to type dt (1 bf16, 2 fp16): every 16-bit pattern widened (NaNs, infinities and the type's subnormals
    included), its fp32 neighbours either side, every exact half-way point between neighbouring values of the type (ties: to the even one),
    values that overflow fp16, fp32 subnormals; a multiple of 4 long"""
    h = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(TORCH_DT[dt]).float()
    fin = h[torch.isfinite(h)].sort().values
    mid = ((fin[:-1].double() + fin[1:].double()) / 2).float()           # exact: neighbours differ in the last bit of a short significand
    up, dn = torch.nextafter(h, torch.full_like(h, _I)), torch.nextafter(h, torch.full_like(h, -_I))
    mup, mdn = torch.nextafter(mid, torch.full_like(mid, _I)), torch.nextafter(mid, torch.full_like(mid, -_I))
    edge = torch.tensor([65504.0, 65519.996, 65520.0, 65536.0, 1e5, 3.4e38, _I, -65504.0, -65519.996, -65520.0, -1e5, -3.4e38, -_I,
                         float("nan"), 0.0, -0.0, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * 1.0000001, 2.0 ** -133, 2.0 ** -134, 3e-6, -3e-6,
                         1e-45, -1e-45, 3.3895e38, 3.3961e38, 1e-40])
    x = torch.cat([h, up, dn, mid, mup, mdn, edge])
    return x[: x.numel() // 4 * 4].contiguous()


def convert_ref(x, dt):
    """torch's CPU conversion of the WHOLE table (sliced afterwards, never converted in pieces: see ln_stream_cases.widen_ref)"""
    return x.to(TORCH_DT[dt])


# ---------------------------------------------------------------------------------------------
# split precision pack / unpack (x2_pack.hip: 4 / 1 values per thread, at most 65 536 blocks of 256)
# ---------------------------------------------------------------------------------------------
X2_COLS = [32, 512, 2048]
X2_ROWS = 37
X2_LD_EXTRA = 32
X2_PACK_WRAP = (32769, 2048)                              # rows * cols / 4 threads > one pass
X2_UNPACK_WRAP = (32769, 512)                             # rows * cols threads > one pass


@functools.lru_cache(maxsize=None)
def x2_source(cols):
    """(37, cols + 32) fp32 over 10 decades with the edges of the fp16 range, values beyond it, NaN, zeros and subnormal tails"""
    g = _gen("x2", cols)
    x = torch.randn(X2_ROWS, cols + X2_LD_EXTRA, generator=g) * 10.0 ** torch.randint(-6, 4, (X2_ROWS, cols + X2_LD_EXTRA), generator=g).float()
    x[0, :12] = torch.tensor([0.0, -0.0, 1.0, 1.00048828125, 65504.0, 1e6, -3e5, 6.1e-5, 65519.996, 65520.0, _I, -_I])
    x[1, 0], x[5, cols - 1], x[36, 17] = float("nan"), float("nan"), -70000.0
    return x


def x2_clipped(x):
    return torch.where(torch.isnan(x), x, x.clamp(-F16_MAX, F16_MAX))


def x2_pack_ref(x):
    """(rows, K) fp32 -> (rows, 2 K) fp16, paired layout; the model of tests/test_x2_gpu.py pack_ref (the host test asserts they agree)"""
    hi, lo = L.x2_split(x)
    out = torch.empty(x.shape[0], 2 * x.shape[1], dtype=torch.float16)
    k = torch.arange(x.shape[1])
    out[:, L.x2_col(k)], out[:, L.x2_col(k) + 32] = hi, lo
    return out


def x2_unpack_ref(p, cols):
    """fp32 head + tail, the kernel's one add (exact in fp64, rounded once)"""
    k = torch.arange(cols)
    return p[:, L.x2_col(k)].float() + p[:, L.x2_col(k) + 32].float()


def x2_pair_bound(x):
    """|head + tail - clipped x| in fp64: 2^-22 relative (normal tails) or 2^-25 absolute (subnormal tails) -- the bound of
    test_pack_is_head_plus_tail_in_the_paired_layout"""
    return x.double().abs() * 2.0 ** -22 + 2.0 ** -25


# ---------------------------------------------------------------------------------------------
# max |x| (x2_pack.hip max_abs_kernel: grid-stride, at most 1024 blocks of 256, atomicMax on the bits of a non-negative float)
# ---------------------------------------------------------------------------------------------
MAXABS_NS = [1, 63, 64, 65, 255, 256, 257, 262144, 262145, 1000003]
MAXABS_THREADS = 1024 * 256
MAXABS_PLACES = ["first", "last", "second_pass"]
MaxAbsCase = collections.namedtuple("MaxAbsCase", "n place negative")


def maxabs_index(n, place):
    if place == "first":
        return 0
    if place == "last":
        return n - 1
    return MAXABS_THREADS + (n - MAXABS_THREADS) // 2 if n > MAXABS_THREADS else None


def maxabs_cases():
    out = []
    for i, n in enumerate(MAXABS_NS):
        for j, place in enumerate(MAXABS_PLACES):
            if maxabs_index(n, place) is not None:
                out.append(MaxAbsCase(n, place, (i + j) % 2 == 0))
    return out


@functools.lru_cache(maxsize=2)
def _maxabs_base(n):
    x = torch.randn(n, generator=_gen("maxabs", n))
    x[3::17] = float("nan")                                   # NaN entries are ignored
    return x


def maxabs_input(c):
    x = _maxabs_base(c.n).clone()
    x[maxabs_index(c.n, c.place)] = -77.5 if c.negative else 77.5
    return x


MAXABS_SPECIALS = collections.OrderedDict([            # name -> (values, tiled to 300 entries; the result as fp32 bits)
    ("plus_inf", ([1.0, _I, -2.0], 0x7F800000)),
    ("minus_inf", ([1.0, -_I, float("nan")], 0x7F800000)),
    ("zeros", ([0.0, -0.0, -0.0], 0x00000000)),
    ("all_nan", ([float("nan")] * 3, 0x00000000)),
    ("subnormal", ([1e-45, -3e-45, 0.0], 0x00000002)),
])


def maxabs_ref_bits(x):
    a = x.abs()
    a = a[~torch.isnan(a)]
    return int(bits32(a.max().reshape(1))[0]) if a.numel() else 0


# ---------------------------------------------------------------------------------------------
# segment-table sanitiser (sampler_kernels.hip sanitize_cu_kernel: one block of 1024 threads, thread t owns the chunk
# [t * per, (t + 1) * per) with per = ceil(n / 1024); prefix maximum over the chunk maxima, then within the chunk)
# ---------------------------------------------------------------------------------------------
SAN_NS = [1, 2, 1023, 1024, 1025, 2048, 2049, 5001]
SAN_THREADS = 1024
SAN_TABLES = ["consistent", "dip_in_chunk", "dip_on_boundary", "negative", "above_limit", "limit0"]
SAN_LIMIT = 100000


def san_per(n):
    return -(-n // SAN_THREADS)


def san_dip(n, table):
    """-> (index of a spike, index of the entry after it that falls back), or None where n has no room for it.  dip_on_boundary: the spike
    is the LAST entry of a chunk, so every later chunk learns of it through the prefix over chunk maxima alone; dip_in_chunk: spike and dip
    lie in one chunk"""
    per = san_per(n)
    if table == "dip_on_boundary":
        k = (n // per) // 2 * per          # a chunk start in the middle of the table
        return (k - 1, k) if 1 <= k < n else None
    if table == "dip_in_chunk":
        k = (n // per) // 2 * per          # the first entry of a chunk; the entry after it is in the same chunk when per >= 2
        return (k, k + 1) if per >= 2 and k + 1 < n else None
    return None


def san_table(n, table):
    """-> (cu int32 (n), limit)"""
    g = _gen("san", n, table)
    limit = 0 if table == "limit0" else SAN_LIMIT
    cu = torch.sort(torch.randint(0, SAN_LIMIT // 2, (n,), generator=g)).values
    cu[0] = 0
    if table == "negative":
        cu[torch.arange(n) % 7 == 3] = -5
        cu[n // 2] = -(2 ** 31)
    elif table == "above_limit":
        cu[n // 3:] += SAN_LIMIT          # the tail runs past the limit, and goes on rising there
        cu[n - 1] = INT32_MAX
    elif table == "limit0":
        cu[n // 2] = -3
    dip = san_dip(n, table)
    if dip is not None:
        cu[dip[0]] = SAN_LIMIT - 7         # far above everything behind it: the running maximum holds it to the end
    return cu.to(torch.int32), limit


def san_ref(cu, limit):
    return torch.cummax(cu.clamp(0, limit), dim=0).values.to(torch.int32)


# ---------------------------------------------------------------------------------------------
# logit bound of the bounded softmax (norm_h16.hip qk_logit_bound_kernel: one wave per head, a lane per column)
# ---------------------------------------------------------------------------------------------
BOUND_HEADS = [1, 4, 8, 12, 16]
BOUND_SLACK = 1.001
BOUND_LANES = [0, 63, 17, 32]
# (sign of the largest |gamma_q|, sign of the largest |gamma_k|) of head h: BOUND_SIGNS[h % 4]
BOUND_SIGNS = [(1, 1), (-1, -1), (1, -1), (-1, 1)]


# 1 + u + 2^-20 for the unit roundoff u of the type: 8 gamma lies 2^-17 above the midpoint of 8 and its upper neighbour
BOUND_WORST_GAMMA = {1: 1.0 + 2.0 ** -8 + 2.0 ** -20, 2: 1.0 + 2.0 ** -11 + 2.0 ** -20}


@functools.lru_cache(maxsize=None)
def bound_gammas(H, aligned):
    """-> (gamma_q, gamma_k) (H, 64), |gamma| < 1 but for one column per head and plane that holds the largest, at lane 0, 63, 17, 32 in
    turn, positive or negative.  aligned: the two maxima sit in the SAME column (the tight case of q.k / 8 <= B: one-hot rows on it)."""
    g = _gen("bound", H, aligned)
    gq, gk = torch.rand(H, 64, generator=g) * 1.8 - 0.9, torch.rand(H, 64, generator=g) * 1.8 - 0.9
    top = 1.0 + torch.rand(2, H, generator=g)                   # in [1, 2): no exact bf16 / fp16 value, the operand roundings are live
    if aligned:
        # the worst case of the two operand roundings: 8 gamma just above the midpoint of two neighbouring 16-bit values, in both planes
        top[:, 0] = BOUND_WORST_GAMMA[1]                          # head 0: bf16 rounds 8 gamma UP by 2^-8 (1 - 2^-8) relative
        if H > 1:
            top[:, 1] = BOUND_WORST_GAMMA[2]                      # head 1: the same for fp16, 2^-11
    for h in range(H):
        lq = BOUND_LANES[h % 4]
        lk = lq if aligned else BOUND_LANES[(h + 1) % 4]
        sq, sk = BOUND_SIGNS[h % 4]
        gq[h, lq], gk[h, lk] = sq * top[0, h], sk * top[1, h]
    return gq, gk


def bound_lane(h):
    return BOUND_LANES[h % 4]


def bound_ref64(gq, gk):
    """8 max|gamma_q| max|gamma_k| per head, fp64 on the fp32 gammas (without the slack)"""
    return 8.0 * gq.double().abs().amax(dim=1) * gk.double().abs().amax(dim=1)


def bound_ref32(gq, gk):
    """the kernel's fp32 chain"""
    return torch.tensor(8.0) * gq.abs().amax(dim=1) * gk.abs().amax(dim=1) * torch.tensor(BOUND_SLACK)


def ulp32(v):
    return 2.0 ** (math.floor(math.log2(abs(v))) - 23)


def bound_onehot_rows(H, TP=5):
    """(2, H, TP, 64) fp32: q and k rows that are one-hot on the column of head h's largest gammas (aligned set), at magnitudes that
    normalise away, signed so that q.k > 0"""
    gq, gk = bound_gammas(H, True)
    x = torch.zeros(2, H, TP, 64)
    mags = torch.tensor([3.0, 0.7, 1.0, 12.5, 0.011])[:TP]
    for h in range(H):
        c = bound_lane(h)
        s = float(torch.sign(gq[h, c]) * torch.sign(gk[h, c]))
        x[0, h, :, c], x[1, h, :, c] = mags, s * mags.flip(0)
    return x


# What q.k / 8 <= B[h] means per path.  The kernels write q = rn(8 gamma_q) and k = rn(8 gamma_k) on the one-hot rows, so with the unit
# roundoff u of the output type (TH.ULP: 2^-8 bf16, 2^-11 fp16; fp32 2^-24) s = q.k / 8 <= (B / 1.001) (1 + u)^2:
#   fp32, fp16: (1 + 2^-11)^2 = 1.00098 < 1.001 -- s <= B holds, in fp16 with 2e-5 to spare;
#   bf16:       (1 + 2^-8)^2 / 1.001 = 1.0068 -- s may exceed B, by less than 2^-7.  Harmless to exp(s - B) (the excess is 0.31 in the
#               exponent at B = 40), and what include/rapflow.h states for bf16.
# Worst measured s / B on the MI355X (head 0 / head 1 of the aligned set are the worst cases above; the GPU test prints every path):
#   rap_qknorm (fp32)                       0.99900
#   rap_qknorm_h16 / rap_gemm_h16_qkvnorm   fp16 0.99997      bf16 1.00679   (both paths alike)
BOUND_EXCESS = {0: 1.0, 2: 1.0, 1: 1.0 + 2.0 ** -7}


# ---------------------------------------------------------------------------------------------
# GEGLU interleave (geglu_interleave_kernel: a block per packed row, k = threadIdx.x; k < K; k += 256)
# ---------------------------------------------------------------------------------------------
GEGLU_INNERS = [32, 64, 96, 1024]
GEGLU_KS = [1, 64, 255, 256, 257, 1024]


def geglu_inputs(inner, K):
    """W (2 inner, K) and b (2 inner): every element another value (integers below 2^24, exact in fp32)"""
    W = torch.arange(2 * inner * K, dtype=torch.float32).reshape(2 * inner, K) + 1.0
    return W, -(torch.arange(2 * inner, dtype=torch.float32) + 1.0)


def geglu_source_rows(inner):
    """packed row 64 g + c = value row 32 g + c (c < 32) or gate row inner + 32 g + c - 32"""
    rp = torch.arange(2 * inner)
    g, c = rp // 64, rp % 64
    return torch.where(c < 32, 32 * g + c, inner + 32 * g + c - 32)


# ---------------------------------------------------------------------------------------------
# grid caps: (name, threads or rows one pass covers, the work items per case) -- both sides of every cap are in the tables
# ---------------------------------------------------------------------------------------------
def passes(items, per_pass):
    return -(-items // per_pass)
