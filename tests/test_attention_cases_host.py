"""CPU: the cases of tests/test_attention_edges_gpu.py are what they are there for -- the six segment tables hold every (start mod 64,
length) pair, stay below the row count up to which tuning key 20 is honoured, and reach every empty-range pattern of the two split
kernels; the fp64 references of the GPU tests agree with torch's own attention in float64; the extreme-logit operands keep the bounded
kernel's contract; and the split entry points refuse bad arguments before anything touches the device."""
import ctypes
import itertools

import torch
import torch.nn.functional as F

import attention_cases as A
import test_h16_gpu as TH
import test_x2_gpu as TX
from rap_amd import _lib

N, ONE = ctypes.c_void_p(0), ctypes.c_void_p(256)      # NULL; a non-NULL sentinel -- every call below fails before a pointer is used


def test_the_six_tables_hold_every_start_and_length_and_stay_small():
    seen = set()
    for start in A.STARTS:
        cu = A.sweep_table(start)
        assert cu[0] == 0 and all(b > a for a, b in zip(cu, cu[1:]))                     # fillers have 1 .. 63 tokens, nothing is empty
        segs = A.segments(cu)
        seen |= {(a % 64, n) for a, n in segs}
        assert {(start, n) for n in A.LENS} <= {(a % 64, n) for a, n in segs}              # every length at THIS table's start offset
        assert all(1 <= n <= 63 for a, n in segs if (a % 64, n) not in set(itertools.product([start], A.LENS)))      # the rest are fillers
        # attention_h16_plan ignores a forced key-20 value above 8 192 rows: the sweep would then run the 256-row kernel five times over
        assert A.align_up(cu[-1], 256) <= 8192, (start, cu[-1])
        assert 2852 <= cu[-1] <= 4200
    assert set(itertools.product(A.STARTS, A.LENS)) <= seen
    assert sum(A.LENS) == 2852


def test_the_lengths_reach_every_empty_range_pattern_of_both_split_kernels():
    # fp32 kernel, tiles relative to the segment start: 1, 2, 3 and >= 4 tiles leave 3, 2, 1 and 0 of four ranges empty
    empties = {A.f32_range_tiles(n, 4).count(0) for n in A.LENS}
    assert empties == {3, 2, 1, 0}
    for n in A.LENS:
        t = A.f32_range_tiles(n, 4)
        assert sum(t) == (n + 63) // 64
    assert A.f32_range_tiles(64, 4) == [0, 0, 0, 1] and A.f32_range_tiles(65, 4) == [0, 1, 0, 1] and A.f32_range_tiles(192, 4) == [0, 1, 1, 1]
    # split-precision kernel, absolute tiles: 1 .. 6 tiles and more; its empty ranges come LAST (5 tiles -> 2, 2, 1, 0)
    shapes = set()
    for start in A.STARTS:
        for a, n in A.segments(A.sweep_table(start)):
            t = A.x2_range_tiles(a, n, 4)
            assert sum(t) == ((a + n - 1) >> 6) - (a >> 6) + 1
            shapes.add(tuple(t))
    assert {sum(s) for s in shapes} >= {1, 2, 3, 4, 5, 6, 9}
    assert {(1, 0, 0, 0), (1, 1, 0, 0), (1, 1, 1, 0), (1, 1, 1, 1), (2, 2, 1, 0), (2, 2, 2, 0), (3, 3, 3, 0)} <= shapes
    # two ranges: an empty one in both kernels at lengths <= 64 (the split-precision kernel only where the segment stays inside one tile)
    assert all(A.f32_range_tiles(n, 2) == [0, 1] for n in A.LENS if n <= 64)
    assert A.x2_range_tiles(0, 64, 2) == [1, 0] and A.x2_range_tiles(63, 2, 2) == [1, 1] and A.x2_range_tiles(33, 31, 2) == [1, 0]
    # the sharp-softmax segments: 11 tiles -> 3, 3, 3, 2 (absolute) and 2, 3, 3, 3 (relative); 129 rows from row 63 -> three tiles either way
    assert A.x2_range_tiles(0, 700, 4) == [3, 3, 3, 2] and A.f32_range_tiles(700, 4) == [2, 3, 3, 3]
    assert A.x2_range_tiles(63, 129, 4) == [1, 1, 1, 0] and A.f32_range_tiles(129, 4) == [0, 1, 1, 1]
    assert A.x2_range_tiles(63, 129, 2) == [2, 1] and A.f32_range_tiles(129, 2) == [1, 2]
    for L, edges in ((700, (191, 192, 383, 384, 575, 576, 127, 128, 319, 320, 511, 512)), (129, (0, 1, 63, 64, 65, 127, 128))):
        assert set(edges) <= set(A.sharp_spikes(L)) and {0, L - 1} <= set(A.sharp_spikes(L))


def test_both_launch_forms_of_the_fp32_split_kernel_are_taken():
    """launch_attention_f32 gives grids of at most 384 blocks 16 KB of unused dynamic LDS (one block per CU), larger grids none.  With
    two heads every table of the sweep stays below that, at two and at four key ranges (like the one pair of 2 x 1024 points the launch
    form was made for); the sweep's extra call with WIDE_HEADS heads on the WIDE_START table is the one that takes the plain launch."""
    for start in A.STARTS:
        cu = A.sweep_table(start)
        assert all(A.f32_split_blocks(cu[-1], len(cu) - 1, A.H, splits) <= 384 for splits in (2, 4))
    for cu in A.SHARP_TABLES.values():
        assert A.f32_split_blocks(cu[-1], len(cu) - 1, A.H, 4) <= 384
    cu = A.sweep_table(A.WIDE_START)
    assert A.f32_split_blocks(cu[-1], len(cu) - 1, A.WIDE_HEADS, 4) > 384


def test_fp64_segment_references_equal_torch_attention_in_float64():
    start = 33
    cu = A.sweep_table(start)
    q, k, v = A.sweep_operands(start)
    TP = cu[-1]

    def sdpa64(q, k, v):
        out = torch.zeros(TP, A.H * 64, dtype=torch.float64)
        for a, n in A.segments(cu):
            o = F.scaled_dot_product_attention(q[:, a:a + n].double(), k[:, a:a + n].double(), v[:, a:a + n].double())
            out[a:a + n] = o.permute(1, 0, 2).reshape(n, A.H * 64)
        return out
    want = sdpa64(q, k, v)
    assert float(want.abs().max()) > 1.0
    assert float((TX.attention_ref64(q, k, v, torch.tensor(cu)) - want).abs().max()) < 1e-13
    for dt in (1, 2):
        qh, kh, vh = (TH.to_h(x, dt).float() for x in (q, k, v))
        assert float((TH.attention_ref64(q, k, v, torch.tensor(cu), dt) - sdpa64(qh, kh, vh)).abs().max()) < 1e-13
    # and the plain-fp32 yardstick is that function in float32
    assert float((A.attention_f32_plain(q, k, v, cu).double() - want).abs().max()) < 5e-6


def test_extreme_logit_operands_keep_the_bounded_kernels_contract():
    for name, cu in A.SHARP_TABLES.items():
        L = cu[-1] - cu[-2]
        for spike in A.sharp_spikes(L):
            q, k, v, row5, at = A.sharp_case_f32(cu, spike, 9)
            bound = TH.logit_bound(q, k)
            assert float(bound.max()) <= 40.0
            lo, hi = A.logits_range(q, k, cu)
            assert 35.9 < hi <= float(bound.min()), (name, spike, hi)
            q, k, v, row5, at = A.sharp_case_x2(cu, spike, 9)
            s = (q[:, row5].double().unsqueeze(1) * k[:, cu[-2]:].double()).sum(-1) / 8.0            # (H, L): query 5 against every key of its segment
            top = s.topk(2, dim=-1).values
            assert (s.argmax(dim=-1) == spike).all() and float((top[:, 0] - top[:, 1]).min()) > 15.0, (name, spike)
        for spike in (0, L // 2, L - 1):
            q, k, v, at = A.far_apart_case_x2(cu, spike, 9)
            s = q[:, cu[-2]:].double() @ k[:, cu[-2]:].double().transpose(1, 2) / 8.0            # (H, L, L)
            others = torch.cat([s[:, :, :spike], s[:, :, spike + 1:]], dim=-1)
            gap = float((s[:, :, spike] - others.amax(dim=-1)).min())
            assert gap * 1.4426950408889634 > 128.0, (name, spike, gap)                         # exp2 of the gap is infinite in fp32
            assert float(k.abs().max()) < 60.0                                                  # far inside fp16: the operands split exactly as usual
        q, k, v = A.near_bound_case(cu, 9)
        lo, hi = A.logits_range(q, k, cu)
        assert -39.0 <= lo and hi <= -30.0 and hi < A.NEAR_BOUND, (name, lo, hi)


def test_split_attention_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = _lib.load()
    q = lib.rap_attention_split_workspace_bytes
    base = lib.rap_attention_workspace_bytes
    up = lambda n: -(-n // 256) * 256
    for TP, nseg, heads in ((1, 1, 1), (200, 3, 2), (3500, 38, 2), (2048, 2, 8)):
        assert q(TP, nseg, heads, 1) == base(TP, nseg)
        for s in (2, 4):
            assert q(TP, nseg, heads, s) == base(TP, nseg) + s * TP * heads * 64 * 4 + up(s * TP * heads * 2 * 4), (TP, nseg, heads, s)
    for bad in ((-1, 1, 2, 2), (10, -1, 2, 2), (10, 1, 0, 2), (10, 1, 2, 0), (10, 1, 2, 3), (10, 1, 2, 8)):
        assert q(*bad) == 0, bad
    assert base(262144, 64) == up((262144 // 64 + 65) * 16) + up(65 * 4)                  # unchanged: the exact-workspace guard tests depend on it

    def f32(qkv=ONE, cu=ONE, nseg=1, out=ONE, TP=256, heads=2, bound=ONE, splits=2, ws=ONE, wsb=1 << 30):
        return lib.rap_attention_f32_split(qkv, cu, nseg, out, TP, heads, bound, splits, ws, wsb, N)

    def x2(qk=ONE, vt=ONE, nblk=4, cu=ONE, nseg=1, out=ONE, TP=256, nt=0, heads=2, splits=2, ws=ONE, wsb=1 << 30):
        return lib.rap_x2_attention_split(qk, vt, nblk, cu, nseg, out, TP, nt, heads, splits, ws, wsb, N)
    assert f32(qkv=N) == -1 and f32(cu=N) == -1 and f32(out=N) == -1 and f32(nseg=-1) == -1 and f32(TP=-1) == -1 and f32(heads=0) == -1
    assert f32(bound=N) == -1 and f32(bound=N, splits=4) == -1                            # only the bounded softmax can add partial results
    assert f32(splits=0) == -1 and f32(splits=3) == -1 and f32(splits=8) == -1
    assert x2(qk=N) == -1 and x2(vt=N) == -1 and x2(cu=N) == -1 and x2(out=N) == -1 and x2(heads=0) == -1 and x2(splits=3) == -1
    assert x2(nt=-1) == -1 and x2(nt=257) == -1 and x2(nblk=3) == -1
    for s in (1, 2, 4):
        need = q(256, 1, 2, s)
        assert f32(ws=N, splits=s) == -2 and f32(wsb=need - 1, splits=s) == -2 and f32(wsb=0, splits=s) == -2
        assert x2(ws=N, splits=s) == -2 and x2(wsb=need - 1, splits=s) == -2
    assert f32(wsb=base(256, 1)) == -2 and x2(wsb=base(256, 1)) == -2                     # the unsplit entry points' workspace is not enough
