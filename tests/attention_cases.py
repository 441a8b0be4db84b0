"""Segment tables, operands and the key-range arithmetic that the host and the GPU tests of the attention kernels' edges share
(tests/test_attention_cases_host.py, tests/test_attention_edges_gpu.py).  Pure Python / torch on the CPU: nothing here touches a GPU.

The sweep: the split-precision and the 16-bit kernels tile the keys of a segment by ABSOLUTE 64-token blocks of the transposed-V image,
the fp32 kernel by 64-key tiles RELATIVE to the segment start, and real few-token batches have arbitrary part lengths -- so every
(start mod 64, length) pair of STARTS x LENS is a segment of one of six tables, and the fillers that realign the starts are ordinary
segments that are checked like the rest."""
import functools

import torch
import torch.nn.functional as F

STARTS = [0, 1, 31, 32, 33, 63]                    # start offsets mod 64
LENS = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 320, 513]      # 257, 320, 513: further work items, partial waves
H = 2                                              # heads of every case (head-count coverage is in the kernels' own files)
WIDE_START, WIDE_HEADS = 33, 4                     # but one: the fp32 split launch has another form above 384 blocks (f32_split_blocks)

# The two fp32 split cases with extreme logits (test_attention_edges_gpu.py, "sharp softmax across key ranges") are held to
# max(ATTN_BOUND, FP32_SHARP_FACTOR x the error of a plain fp32 evaluation -- torch CPU float32 matmul + softmax -- against fp64 on the
# same inputs): the factor is for the different association order of the MFMA chains and of the partial sums, not for a looser kernel.
# Measured (yardstick = the plain fp32 evaluation, kernel = rap_attention_f32_split on an MI355X, worst over both geometries, every
# spike position and 2 / 4 key ranges; max abs error against fp64):
#   spike (logit 36):        yardstick up to 3.6e-6 (per case 1.4e-6 .. 3.6e-6)   kernel up to 4.0e-6 (2 ranges), 3.4e-6 (4 ranges)
#   all logits near -bound:  yardstick 6.9e-7 (700 rows), 2.1e-6 (129 rows)        kernel 6.6e-7, 1.9e-6 (the same at 2 and 4 ranges)
# -- the kernel is at the plain evaluation's own distance from fp64 in every case; the bound of a case is 4 x ITS yardstick (or ATTN_BOUND).
FP32_SHARP_FACTOR = 4.0


def align_up(n, a):
    return -(-n // a) * a


@functools.lru_cache(maxsize=None)
def sweep_table(start):
    """cu_seqlens (a list) in which every length of LENS is a segment whose first row is = start (mod 64); a filler segment of 1 .. 63
    tokens goes in front of a segment wherever the running position is not there already"""
    assert 0 <= start < 64
    cu = [0]
    for n in LENS:
        fill = (start - cu[-1]) % 64
        if fill:
            cu.append(cu[-1] + fill)
        assert cu[-1] % 64 == start
        cu.append(cu[-1] + n)
    return cu


def segments(cu):
    return [(a, b - a) for a, b in zip(cu[:-1], cu[1:])]


# ---- the two kernels' split of a segment's key tiles over `splits` key ranges, restated (attn_f32.hip: SPLIT; attn_x2.hip: SPLIT) ----
def f32_range_tiles(length, splits):
    """tiles of 64 keys RELATIVE to the segment start; range y takes tiles [n y / splits, n (y + 1) / splits) -> tiles per range"""
    n = (length + 63) // 64
    return [n * (y + 1) // splits - n * y // splits for y in range(splits)]


def x2_range_tiles(start, length, splits):
    """ABSOLUTE 64-token tiles that the segment touches; range y takes `per` = ceil(n / splits) tiles from tile y * per -> tiles per range"""
    n = ((start + length - 1) >> 6) - (start >> 6) + 1
    per = (n + splits - 1) // splits
    return [max(0, min(per, n - y * per)) for y in range(splits)]


def f32_split_blocks(TP, nseg, heads, splits):
    """blocks of the fp32 split launch: the entry point reserves TP / 256 + nseg + 1 work items.  At most 384 blocks take the
    one-block-per-CU launch (16 KB of unused dynamic LDS), more take the plain one (attn_f32.hip: launch_attention_f32)."""
    return (TP // 256 + nseg + 1) * heads * splits


# ---- operands ----
def operands(TP, seed, heads=H):
    """q, k, v (heads, TP, 64) fp32 in the style of the kernels' ragged tests: |q|, |k| between 4 and 12 (per-dimension gains), v ~ N(0, 1)"""
    g = torch.Generator().manual_seed(seed)
    q = F.normalize(torch.randn(heads, TP, 64, generator=g), dim=-1) * 8 * (0.5 + torch.rand(heads, 1, 64, generator=g))
    k = F.normalize(torch.randn(heads, TP, 64, generator=g), dim=-1) * 8 * (0.5 + torch.rand(heads, 1, 64, generator=g))
    v = torch.randn(heads, TP, 64, generator=g)
    return q, k, v


@functools.lru_cache(maxsize=None)
def sweep_operands(start):
    return operands(sweep_table(start)[-1], 100 + start)


# one segment of 700 rows from row 0 (11 tiles -> 3, 3, 3, 2 at four key ranges in the split-precision kernel, 2, 3, 3, 3 in the fp32
# kernel); one of 129 rows from row 63 behind a 63-token filler (rows 63 .. 191: three absolute tiles of 1, 64 and 64 keys, three
# relative ones of 64, 64 and 1)
SHARP_TABLES = {"700-from-0": [0, 700], "129-from-63": [0, 63, 192]}


def sharp_spikes(L):
    """positions (relative to the segment) of the dominant key: the first and the last key and the interior of every key range at four
    ranges of the 700-row segment in the split-precision kernel (0, 191 | 192, 350, 383 | 384, 575 | 576, 699) and in the fp32 kernel
    (0, 127 | 128, 319 | 320, 511 | 512, 699), and either side of every tile edge of the 129-row one (0 | 1, 64 | 65, 128 absolute,
    63 | 64, 127 | 128 relative)"""
    return sorted({p for p in (0, 1, 63, 64, 65, 127, 128, 191, 192, 319, 320, 350, 383, 384, 511, 512, 575, 576, L - 1) if p < L})


def sharp_case_x2(cu, spike, seed):
    """test_x2_attention_sharp_softmax_and_late_maximum's operands: k = randn / 10 with one key = 4 q[5] (logit |q5|^2 / 2 ~ 32 for query 5
    of the LAST segment of cu, far above every other).  -> q, k, v, the absolute rows of query 5 and of the spike"""
    g = torch.Generator().manual_seed(seed)
    TP, a = cu[-1], cu[-2]
    q = torch.randn(H, TP, 64, generator=g); k = torch.randn(H, TP, 64, generator=g) * 0.1; v = torch.randn(H, TP, 64, generator=g)
    k[:, a + spike] = q[:, a + 5] * 4.0
    return q, k, v, a + 5, a + spike


def sharp_case_f32(cu, spike, seed):
    """the same for the BOUNDED fp32 kernel, which needs logits <= 40: |q| = 12, k = randn / 10 except k[spike] = 2 q[5] -> logit 36"""
    g = torch.Generator().manual_seed(seed)
    TP, a = cu[-1], cu[-2]
    q = F.normalize(torch.randn(H, TP, 64, generator=g), dim=-1) * 12
    k = torch.randn(H, TP, 64, generator=g) * 0.1
    v = torch.randn(H, TP, 64, generator=g)
    k[:, a + spike] = q[:, a + 5] * 2.0
    return q, k, v, a + 5, a + spike


def far_apart_case_x2(cu, spike, seed):
    """partial maxima further apart than fp32's exponent range: every logit of the last segment is about -44 (all queries within a few
    degrees of one direction u, |q| = 8, k = -45 u + noise) except one key = +50 u, about +49 for every query -- 93 apart, and
    exp2(93 log2 e) = 2^135 is infinite in fp32.  The combine pass of the split form has to measure every range's maximum against the
    LARGEST one (weights <= 1, the far ranges flush to 0); against any other range's maximum the spike's weight overflows.  Every row
    of that segment is one-hot on the spike.  -> q, k, v, the absolute row of the spike"""
    g = torch.Generator().manual_seed(seed)
    TP, a = cu[-1], cu[-2]
    u = F.normalize(torch.randn(H, 1, 64, generator=g), dim=-1)
    q = F.normalize(u + 0.02 * torch.randn(H, TP, 64, generator=g), dim=-1) * 8
    k = -45.0 * u + 0.05 * torch.randn(H, TP, 64, generator=g)
    v = torch.randn(H, TP, 64, generator=g)
    k[:, a + spike] = 50.0 * u[:, 0]
    return q, k, v, a + spike


NEAR_BOUND = 39.5


def near_bound_case(cu, seed):
    """every logit of every segment close to MINUS the bound: all queries of a head within a few degrees of one direction u (|q| = 8),
    k = -35 x (the mean query direction) + small noise, so every q.k/8 lies in [-39, -30] under the declared bound 39.5.  The bounded fp32
    kernel takes p = exp(logit) with no offset: every numerator is about e^-35 = 1e-15 and every row sum about 1e-13 -- far below 1,
    normal numbers, and the common factor has to cancel in O / l."""
    g = torch.Generator().manual_seed(seed)
    TP = cu[-1]
    u = F.normalize(torch.randn(H, 1, 64, generator=g), dim=-1)
    q = F.normalize(u + 0.02 * torch.randn(H, TP, 64, generator=g), dim=-1) * 8
    qbar = F.normalize(q.mean(dim=1, keepdim=True), dim=-1)
    k = -35.0 * qbar + 0.05 * torch.randn(H, TP, 64, generator=g)
    v = torch.randn(H, TP, 64, generator=g)
    return q, k, v


def logits_range(q, k, cu):
    lo, hi = float("inf"), float("-inf")
    for a, n in segments(cu):
        if n:
            s = q[:, a:a + n].double() @ k[:, a:a + n].double().transpose(1, 2) / 8.0
            lo, hi = min(lo, float(s.min())), max(hi, float(s.max()))
    return lo, hi


def attention_f32_plain(q, k, v, cu):
    """the yardstick of the fp32 sharp cases: softmax attention per segment in plain float32 on the CPU (matmul + softmax) -> (TP, H * 64)"""
    heads, TP, _ = q.shape
    out = torch.zeros(TP, heads * 64, dtype=torch.float32)
    for a, n in segments(cu):
        if n:
            p = torch.softmax(q[:, a:a + n] @ k[:, a:a + n].transpose(1, 2) / 8.0, dim=-1)
            out[a:a + n] = (p @ v[:, a:a + n]).permute(1, 0, 2).reshape(n, heads * 64)
    return out
