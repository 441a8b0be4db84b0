"""The cases and the CPU references that the host and the GPU tests of the residual-stream LayerNorm kernels share
(tests/test_ln_stream_cases_host.py, tests/test_ln_stream_gpu.py).  Pure torch, seeded, cached: nothing here touches a GPU.

The kernels (rap_amd/csrc/norm_h16.hip): layernorm_h16_kernel<NV, DT, XH, COMB> and layernorm_x2_kernel<NV, COMB>, one wave per row, four
rows per block, NV = d / 256 float4 per lane.  XH: the residual stream is fp16; COMB: the kernel first forms the new stream value from the
partial planes of a split-K residual GEMM, stores it, and normalises the STORED value.  With XH and an even NV (d = 512, 1024) a lane owns 8
consecutive columns, otherwise 4 -- two column maps in one kernel, which every load and store of a row has to agree on.  The inputs below
are distinct per column (x, gains, shifts, bias, every plane), so a load through the other map is an O(1) error in identifiable columns.

References:
  * stream value: the kernel's own fp32 adds in the kernel's own order, as sequential tensor adds -- (0 + p0 + p1 + ...) + bias, then + h --
    and for an fp16 stream clamp(+-65504) and ONE .to(float16).  torch.clamp keeps NaN and maps +-inf to +-65504, which is half.h f16_sat.
    Compared BITWISE;
  * LayerNorm output: fp64 LayerNorm (eps 1e-5) of the STORED stream value, fp64 modulation, at the bounds the suite already holds the same
    outputs to (tests/test_h16_gpu.py, tests/test_x2_gpu.py; restated here, tests/test_ln_stream_cases_host.py asserts they are the same
    numbers and that a plain fp32 torch LayerNorm rounded once into the output type meets them on every case).
"""
import collections
import functools
import zlib

import torch
import torch.nn.functional as F

# (compute dtype, residual stream): dtype 1 = bf16, 2 = fp16 operands, 3 = split precision (fp32 stream only)
MODES = [(1, "f32"), (1, "f16"), (2, "f32"), (2, "f16"), (3, "f32")]
WIDTHS = [256, 512, 768, 1024]                  # NV = 1 .. 4
# every tail of the 4-rows-per-block launch (1, 2, 3 rows in the last block, none), one and several blocks; 1027 = 256 blocks + a 3-row tail.
# The kernels have no other size-dependent path.
SMALL_ROWS = [1, 2, 3, 4, 5, 8, 9]
ROWS = SMALL_ROWS + [1027]
FORMS = ["mod_rows", "mod", "affine"]           # adaLN through token_row; adaLN with token_row = NULL (table row 0); gain / shift
SPLITS = [1, 2, 3, 4, 8]
# one magnitude per plane: a dropped, repeated or exchanged plane (or a plane stride that lands in a neighbour) moves the fp32 sum by far
# more than an ulp
PLANE_SCALES = [1.0, 1e-3, 30.0, 0.25, 3e-2, 7.0, 1e-2, 2.0]
TABLE_ROWS, TABLE_SLOTS = 3, 4                  # the modulation table: (3, 4, 2 d) as in the model, the LayerNorm reads slot MOD_SLOT
MOD_SLOT = 2
F16_MAX = 65504.0

TORCH_DT = {1: torch.bfloat16, 2: torch.float16}
# restated from tests/test_h16_gpu.py (ULP, ONE_ROUNDING, NORM_SLACK) and tests/test_x2_gpu.py (X2_NORM_BOUND)
ULP = {1: 2.0 ** -8, 2: 2.0 ** -11}
ONE_ROUNDING = 1.01
NORM_SLACK = 1e-4
X2_NORM_BOUND = 5e-7


def wide_map(stream, d):
    """the kernel's 8-columns-per-lane map: fp16 stream and an even number of float4 per lane"""
    return stream == "f16" and (d // 256) % 2 == 0


def column_of(stream, d, lane, i, j):
    """column of element j (0 .. 3) of a lane's i-th float4, as norm_h16.hip indexes it"""
    if wide_map(stream, d):
        return (i // 2) * 512 + lane * 8 + (i % 2) * 4 + j
    return (i * 64 + lane) * 4 + j


def row_tail(rows):
    return rows % 4


def blocks(rows):
    return -(-rows // 4)


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ln_params(d):
    """-> (mod (3, 4, 2 d), gain (d), shift (d)): distinct per column, shared by every case of a width"""
    g = _gen("params", d)
    mod = torch.randn(TABLE_ROWS, TABLE_SLOTS, 2 * d, generator=g) * 0.3
    return mod, torch.randn(d, generator=g), torch.randn(d, generator=g)


def token_rows(rows):
    """2, 1, 0, 2, 1, 0, ...: not monotone, and the first row reads the LAST table row"""
    return ((2 - torch.arange(rows)) % TABLE_ROWS).to(torch.int32)


@functools.lru_cache(maxsize=None)
def bias_of(d):
    return torch.randn(d, generator=_gen("bias", d))


@functools.lru_cache(maxsize=16)
def stream_input(d, rows):
    """the residual stream before the call, fp32: (rows, d)"""
    return torch.randn(rows, d, generator=_gen("x", d, rows)) * 3 + 0.5


@functools.lru_cache(maxsize=8)
def planes(d, rows):
    """(8, rows, d) fp32: plane s at magnitude PLANE_SCALES[s]; a case with `splits` planes takes the first `splits`"""
    p = torch.randn(len(PLANE_SCALES), rows, d, generator=_gen("part", d, rows))
    return p * torch.tensor(PLANE_SCALES)[:, None, None]


def as_stream(x, stream):
    """an fp32 tensor as the stream holds it before the call"""
    return x.to(torch.float16) if stream == "f16" else x.clone()


# ---------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------
def combine_sum(part, bias, h):
    """the fp32 value the kernel forms: (0 + part[0] + part[1] + ...) + bias, then + h (h widened from fp16 where the stream is fp16)"""
    acc = torch.zeros_like(part[0])
    for s in range(part.shape[0]):
        acc = acc + part[s]
    if bias is not None:
        acc = acc + bias
    return acc + h.float()


def store(v, stream):
    """the stored stream value: the fp32 sum itself, or its saturating round to fp16"""
    return v.clamp(-F16_MAX, F16_MAX).to(torch.float16) if stream == "f16" else v


def modulation(form, d, rows, dt=torch.float32):
    """-> (multiplier, shift) of the normalised rows, (rows, d) or (d), formed in `dt` from the fp32 tables"""
    mod, gain, shift = (t.to(dt) for t in ln_params(d))
    if form == "affine":
        return gain, shift
    t = token_rows(rows).long() if form == "mod_rows" else torch.zeros(rows, dtype=torch.long)
    return 1 + mod[t, MOD_SLOT, :d], mod[t, MOD_SLOT, d:]


def ln_ref64(stored, form):
    """fp64 LayerNorm of the stored stream value with fp64 modulation"""
    rows, d = stored.shape
    mul, add = modulation(form, d, rows, torch.float64)
    return F.layer_norm(stored.double(), (d,), eps=1e-5) * mul + add


def x2_col(k):
    return ((k >> 5) << 6) | (k & 31)


def x2_split(v):
    """torch model of half.h x2_split4 -> (head, tail) fp16"""
    s = torch.where(torch.isnan(v), v, v.clamp(-F16_MAX, F16_MAX))
    hi = s.to(torch.float16)
    return hi, (s - hi.float()).to(torch.float16)


def ln_ref32_rounded(stored, form, dtype):
    """the yardstick: a plain fp32 torch LayerNorm of the stored value, fp32 modulation, rounded ONCE into the output type -> fp64"""
    rows, d = stored.shape
    mul, add = modulation(form, d, rows)
    o = F.layer_norm(stored.float(), (d,), eps=1e-5) * mul + add
    if dtype == 3:
        hi, lo = x2_split(o)
        return hi.double() + lo.double()
    return o.to(TORCH_DT[dtype]).double()


def ln_error(dtype, got, ref):
    """-> (worst error, bound) in the measure the suite holds this output to.  Rows whose reference is NaN are the caller's to check."""
    ok = ~torch.isnan(ref).any(dim=1)
    got, ref = got[ok].double(), ref[ok]
    if dtype == 3:
        return float((got - ref).abs().max()) / float(ref.abs().max()), X2_NORM_BOUND
    return float(((got - ref).abs() / (ref.abs() + 1e-2)).max()), ONE_ROUNDING * ULP[dtype] + NORM_SLACK


# ---------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------
PlainCase = collections.namedtuple("PlainCase", "dtype stream d rows form")
FusedCase = collections.namedtuple("FusedCase", "dtype stream d rows form splits bias")


def plain_cases(dtype, stream, d, rows_list=ROWS):
    return [PlainCase(dtype, stream, d, rows, form) for rows in rows_list for form in FORMS]


def fused_cases(dtype, stream, d, rows_list=ROWS):
    """every row count with every split count; bias and LN form rotate so that, for one (mode, d), every split count occurs with and without
    a bias and every row count with all three LN forms"""
    out = []
    for ri, rows in enumerate(rows_list):
        for si, splits in enumerate(SPLITS):
            out.append(FusedCase(dtype, stream, d, rows, FORMS[(ri + si) % 3], splits, (ri + si) % 2 == 0))
    return out


def fused_inputs(c):
    """-> (part (splits, rows, d), bias or None, h as the stream holds it)"""
    return planes(c.d, c.rows)[:c.splits], (bias_of(c.d) if c.bias else None), as_stream(stream_input(c.d, c.rows), c.stream)


def fused_stored(c):
    part, bias, h = fused_inputs(c)
    return store(combine_sum(part, bias, h), c.stream)


# ---------------------------------------------------------------------------------------------
# special rows (fp16 stream): every value below is PRODUCED BY THE SUM of two planes, the bias and the residual
# ---------------------------------------------------------------------------------------------
SPECIAL_ROWS, SPECIAL_SPLITS = 9, 2
# name -> (row, column, plane 0, plane 1, h, what the stream must hold afterwards as fp16 bits).  The bias is zero in these columns.
# Rows 0, 2, 3 and 5 hold specials; rows 1, 4, 6, 7, 8 -- a neighbour in the same block, a whole block, the tail block -- hold none.
_H, _I = 2.0 ** -11, float("inf")
SPECIALS = collections.OrderedDict([
    ("above",       (0, 5,   60000.0,   5000.0, 1000.0, 0x7BFF)),      # 66 000: finite, above 65 504 only once the residual is added
    ("below",       (0, 130, -60000.0, -5000.0, -1000.0, 0xFBFF)),
    ("rounds_max",  (0, 251, 65000.0,   500.0,  0.0,    0x7BFF)),      # 65 500 < 65 504: the clamp is idle, the ROUNDING gives 65 504
    ("just_above",  (0, 77,  65000.0,   519.0,  0.0,    0x7BFF)),      # 65 519: would round to 65 504 anyway; 65 520 would round to inf
    ("round_inf",   (0, 200, 65000.0,   520.0,  0.0,    0x7BFF)),      # 65 520: an unsaturated conversion gives +inf
    ("plus_inf",    (2, 9,   3e38,      3e38,   1.0,    0x7BFF)),      # two finite planes overflow fp32
    ("minus_inf",   (2, 190, -_I,       1.0,    2.0,    0xFBFF)),
    ("nan",         (3, 66,  _I,        -_I,    1.0,    None)),        # inf - inf; checked with isnan
    ("subnormal",   (5, 3,   2e-6,      1e-6,   0.0,    None)),        # 3e-6 < 2^-14: checked as 0 < |v| < 2^-14
    ("minus_zero",  (5, 100, -1e-9,     0.0,    0.0,    0x8000)),      # (0 + -0 is +0 in every rounding mode: -0 comes from a tiny negative sum)
    ("half_even",   (5, 161, 1.0,       _H,     0.0,    0x3C00)),      # 1 + 2^-11, halfway between 1 and 1 + 2^-10: to the even one, 1
    ("half_odd",    (5, 255, 1.0,       3 * _H, 0.0,    0x3C02)),      # 1 + 3 * 2^-11, halfway between 1 + 2^-10 and 1 + 2^-9: to 1 + 2^-9
])
SPECIAL_CLEAN_ROWS = [1, 4, 6, 7, 8]
SATURATED = {"above": F16_MAX, "below": -F16_MAX, "rounds_max": F16_MAX, "just_above": F16_MAX, "round_inf": F16_MAX, "plus_inf": F16_MAX,
             "minus_inf": -F16_MAX}


def special_column(name, d):
    """the columns above lie in 0 .. 255; at wider rows they move into the last 256 columns (the second 512-column group of the 8-column map
    at d = 1024, the third float4 of the 4-column map at d = 768)"""
    return SPECIALS[name][1] + d - 256


def special_inputs(d, with_specials=True):
    """-> (part (2, 9, d), bias (d), h fp16 (9, d)): the base case, and the same with the special elements set"""
    part = planes(d, SPECIAL_ROWS)[:SPECIAL_SPLITS].clone()
    bias = bias_of(d).clone()
    h = as_stream(stream_input(d, SPECIAL_ROWS), "f16")
    for name, (r, _, p0, p1, hv, _) in SPECIALS.items():
        bias[special_column(name, d)] = 0.0          # in both runs: the clean rows see the same bias
    if with_specials:
        for name, (r, _, p0, p1, hv, _) in SPECIALS.items():
            c = special_column(name, d)
            part[0, r, c], part[1, r, c], h[r, c] = p0, p1, hv
    return part, bias, h


# ---------------------------------------------------------------------------------------------
# conversions
# ---------------------------------------------------------------------------------------------
def all_f16_patterns():
    """all 65 536 bit patterns as an fp16 tensor (int16 view: -32768 .. 32767)"""
    return torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(torch.float16)


@functools.lru_cache(maxsize=1)
def widen_ref():
    """.float() of all 65 536 patterns (a signalling NaN leaves quiet, its payload kept).  Always converted as ONE whole table and sliced
    afterwards: torch converts the last elements of a tensor whose length is no multiple of its vector width one by one, and that path
    writes another NaN for a NaN"""
    return all_f16_patterns().float()


@functools.lru_cache(maxsize=1)
def sat_table():
    """fp32 inputs of the saturating conversion: every fp16 value widened (NaNs included), every midpoint between neighbouring fp16 values
    and one fp32 step either side of it (round to nearest even, both directions), the edges of the range, seeded values over 22 decades;
    a multiple of 4 long"""
    h = all_f16_patterns().float()
    fin = h[torch.isfinite(h)].sort().values
    mid = (fin[:-1].double() + fin[1:].double()) / 2
    mid = mid.float()                                   # exact: neighbouring fp16 values differ in one bit of an 11-bit significand
    up, dn = torch.nextafter(mid, torch.full_like(mid, _I)), torch.nextafter(mid, torch.full_like(mid, -_I))
    g = _gen("sat")
    rnd = torch.randn(4096, generator=g) * 10.0 ** torch.randint(-12, 10, (4096,), generator=g).float()
    edge = torch.tensor([65504.0, 65519.996, 65520.0, 65536.0, 1e5, 3.4e38, _I, -65504.0, -65519.996, -65520.0, -1e5, -3.4e38, -_I, float("nan"),
                         0.0, -0.0, 1e-9, -1e-9, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * 1.0000001, 3e-6, -3e-6, 1e-45, -1e-45])
    x = torch.cat([h, mid, up, dn, rnd, edge])
    return x[: x.numel() // 4 * 4].contiguous()


def sat_ref(x):
    return x.clamp(-F16_MAX, F16_MAX).to(torch.float16)


# one element more than a grid of 65 536 blocks of 256 threads covers in one pass: 4 values (sat) / 8 values (to_f32) per thread
SAT_WRAP_N = 65536 * 256 * 4 + 4 * 256 * 3 + 4
WIDEN_WRAP_N = 65536 * 256 * 8 + 8 * 256 * 3 + 8
