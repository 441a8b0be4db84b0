"""The cases and the restated arithmetic that the host and the GPU tests of the WHOLE-CALL dispatch share (tests/test_plan_cases_host.py,
tests/test_plan_edges_gpu.py).  Pure torch and Python, seeded: nothing here touches a GPU.

A model call decides, from its shape alone, which arithmetic runs, which form each of its eight GEMMs takes, how many split-K planes the
workspace reserves, whether the combine + LayerNorm fusion is on, the attention work-list geometry and the key ranges of each branch, and
which idle buffer hosts which partial planes (rap_amd/csrc/api.hip: plan_call, which the launch path runs by and rap_call_plan reports).
The kernel-level sweeps cannot see a wrong threshold there, a plane count two call sites compute differently, or a buffer that stops
being idle at some size.  The sweep here puts one call on each side of every row count and every work-list size at which the plan of a
rap_12-width model (d = 512, 8 heads) changes: TP = TQ_low exactly (no filler rows) and TP = TQ_low + 1 (255 filler rows, the most
prepare_static ever zeroes).

The plan arithmetic is restated below next to the kernel file it belongs to; the host test holds rap_call_plan to it on every case and on
a dense grid, and computes from it that every pair changes exactly the fields it is listed for.
"""
import collections
import contextlib
import ctypes
import functools

import torch

from rap_amd import synthetic as S

# ---------------------------------------------------------------------------------------------
# modes: name -> (compute dtype, residual dtype) as rap_amd.PointCloudDiT takes them, and as the C ABI numbers them
# ---------------------------------------------------------------------------------------------
MODES = {"f32": ("float32", "float32"), "x2": ("float32x2", "float32"), "bf16h": ("bfloat16", "float16"), "f16": ("float16", "float32")}
DT = {"float32": 0, "bfloat16": 1, "float16": 2, "float32x2": 3}
FAMILY = {"f32": "f32", "x2": "x2", "bf16h": "h16", "f16": "h16"}
D, HEADS, LAYERS, STEPS = 512, 8, 2, 2          # rap_12 widths, 2 layers, 2 flow steps, rigidity forcing on
WIDTHS = [(256, 4), (512, 8), (768, 12), (1024, 16)]

FIELDS = ("dtype", "TQ", "attn_bq", "attn_kg", "items_part", "items_batch", "ranges_part", "ranges_batch", "percu_part", "percu_batch",
          "fused", "planes", "f_static", "f_embed", "f_qkv", "f_out", "f_ff1", "f_ff2", "f_head0", "f_head1", "ws_bytes")
ALWAYS = {"TQ", "ws_bytes"}                     # what a row pair changes besides what it is listed for
Plan = collections.namedtuple("Plan", FIELDS)

# the tuning keys the plan reads, at their defaults (gemm_cases.tuned.DEFAULTS holds the same numbers for the ones it knows)
KEYS = {5: 1, 6: 1, 7: 1, 11: 1, 12: 1, 13: 1, 17: 1024, 18: 256, 19: 1, 20: 1}


def _cdiv(a, b):
    return -(-a // b)


def _up(a, b):
    return _cdiv(a, b) * b


# ---- gemm_f32.hip: gemm_f32_splits_by_shape, gemm_f32_form (epilogues: 1 bias + residual, 2 bias + SiLU; tiles of 128 x 128, k-tiles of 32)
def f32_form(epi, M, N, K, ws, planes, keys):
    if M <= 0:
        return 0
    if ws and keys[6]:
        tiles = _cdiv(M, 128) * (N // 128)
        sp = 1
        if epi == 1:
            sp = 4 if (K >= 1024 and tiles <= 128) or (K >= 512 and tiles <= 64) else 1
        elif epi == 2:
            sp = planes if planes in (2, 4) and K >= 512 and (K // 32) % planes == 0 and tiles <= 64 else 1
        if sp > 1:
            return 120 + sp
    if N % 256 == 0 and K >= 256 and _cdiv(M, 256) * (N // 256) >= 512:
        return 301 if keys[12] and M % 256 == 0 and (M // 256) * (N // 256) >= 512 else 201
    return 121


# ---- gemm_h16.hip: gemm_h16_splits_by_shape / gemm_h16_splits, small_stages, few_tiles, use_persistent[_x2], gemm_h16_form
def h16_splits_by_shape(M, N, K):
    if M <= 0 or N % 128 or K < 1024 or (K // 64) % 4:
        return 1
    tiles = _cdiv(M, 128) * (N // 128)
    return 4 if tiles <= 64 else 2 if tiles <= 128 else 1


def h16_form(x2, resid, M, N, K, ws, defer, force, keys):
    def small(sp):
        return 100 + 10 * (4 if _cdiv(M, 128) * (N // 128) * sp <= keys[18] else 2) + sp
    if resid and ws:
        sp = force if force > 0 else (h16_splits_by_shape(M, N, K) if keys[6] else 1)
        if sp > 1 or defer:
            return small(sp)
    few = _cdiv(M, 256) * (N // 256) < 256
    full = M % 256 == 0 and (M // 256) * (N // 256) >= 512
    if x2:
        if few:
            return small(1)
        return 301 if keys[11] and full and K <= 8192 else 201
    big = N % 256 == 0 and K >= 128
    if big and keys[11] and full and K <= 2048:
        return 301
    if big and not few:
        return 201
    return small(1)


# ---- attn_h16.hip: attention_h16_plan (tuning keys 20 and 13) -> (query rows per work item, key groups per block)
def attn_h16_plan(rows, keys):
    mode = keys[20]
    if not mode or not keys[13] or rows <= 0 or rows > 8192:
        return 256, 1
    if mode in (64, 128):
        return mode, 1
    if mode == 66:
        return 64, 4
    if mode == 130:
        return 128, 2
    if rows > 4096:
        return 256, 1
    if mode == 2:
        return 128, 1
    return (64, 4) if rows <= 2048 else (128, 2)


# ---- attn_f32.hip: attention_f32_splits, attention_f32_one_per_cu; attn_x2.hip: attention_x2_splits (tuning key 5)
def attn_f32_ranges(items, heads, bounded, keys):
    if not bounded or not keys[5]:
        return 1, 0
    blocks = items * heads
    sp = 4 if blocks <= 160 else 2 if blocks <= 320 else 1
    return sp, int(sp > 1 and blocks * sp <= 384)


def attn_x2_ranges(items, heads, keys):
    if not keys[5]:
        return 1, 0
    blocks = items * heads
    return (4 if blocks <= 96 else 2 if blocks <= 192 else 1), 0


# ---- api.hip: carve_workspace (every buffer rounded up to 256 bytes; work items of 16 bytes; 16 Procrustes chunks of 16 doubles per part)
def workspace_bytes(dtype, h16_stream, planes, d, L, Ks, TP, T, B, nseg, rows):
    a = lambda n: _up(n, 256)
    tot = a(T * d * 4) + (a(T * d * 2) if h16_stream else a(T * d * 4))
    if dtype == 0:
        tot += a(T * d * 4) + a(T * 3 * d * 4) + a(T * d * 4) + a(T * 4 * d * 4)
    else:
        pl = 2 if dtype == 3 else 1
        tot += a(T * d * 2 * pl) + a(T * 2 * d * 2 * pl) + a((T // 64) * 64 * d * 2 * pl) + a(T * d * 2 * pl)
        tot += a(max(T * 4 * d * 2 * pl, T * Ks * 4))
        if planes:
            tot += a(planes * T * d * 4)
    tot += a(T * 64 * 4) + 2 * a(T * 12) + a(rows * 2 * L * 2 * d * 4) + a(rows * (256 + 4 * L * d) * 4) + a(rows * 4) + a(T * 4)
    tot += 2 * a((nseg + 1) * 4) + a((B + 1) * 4)
    tot += a((TP // 64 + B + 1) * 16) + a((TP // 64 + nseg + 1) * 16) + a((max(nseg, B) + 1) * 4)
    tot += a(nseg * 16 * 16 * 8) + a(nseg * 36) + a(nseg * 12)
    return tot


# ---- api.hip: plan_call, plan_attention, rap_call_plan
def plan(mode, TP, B, nseg, d=D, heads=HEADS, L=LAYERS, rows=STEPS, in_dim=0, bounded=True, keys=KEYS, force_dtype=None):
    cdt, rdt = (DT[x] for x in MODES[mode])
    T = _up(TP, 256)
    dtype = force_dtype if force_dtype is not None else (0 if cdt == 3 and T < keys[17] else cdt)
    f32, x2, half = dtype == 0, dtype == 3, dtype in (1, 2)
    h16_stream = half and rdt == 2
    bq, kg = attn_h16_plan(T, keys) if half else (256, 1)
    items_b, items_p = TP // bq + B + 1, TP // bq + nseg + 1
    planes = 0
    if not f32:
        sp = h16_splits_by_shape(T, d, (8 if x2 else 4) * d)
        planes = sp if sp > 1 else 0
    fused = int(bool(keys[19]) and not f32 and planes > 0 and bool(keys[6]))
    if f32:
        rp, rb = attn_f32_ranges(items_p, heads, bounded, keys), attn_f32_ranges(items_b, heads, bounded, keys)
    elif x2:
        rp, rb = attn_x2_ranges(items_p, heads, keys), attn_x2_ranges(items_b, heads, keys)
    else:
        rp = rb = (1, 0)
    Ks = 128 + _up(in_dim, 32)
    head_ws, head_planes = (True, 4) if f32 else (planes > 0, planes)
    forms = [f32_form(5, TP, d, Ks, False, 0, keys), f32_form(1, T, d, 64, False, 0, keys)]
    if f32:
        forms += [f32_form(4, T, 3 * d, d, False, 0, keys), f32_form(1, T, d, d, True, 0, keys), f32_form(3, T, 8 * d, d, False, 0, keys),
                  f32_form(1, T, d, 4 * d, True, 0, keys)]
    else:
        pl = 2 if x2 else 1

        def deferred(M, N, K):          # (defer_combine: the count is gemm_h16_splits at planning time, at least one plane)
            return max(1, h16_splits_by_shape(M, N, K) if keys[6] else 1)
        forms += [h16_form(x2, False, T, 3 * d, pl * d, False, 0, 0, keys),
                  h16_form(x2, True, T, d, pl * d, bool(fused), fused, deferred(T, d, pl * d) if fused else 0, keys),
                  h16_form(x2, False, T, 8 * d, pl * d, False, 0, 0, keys)]
        f2_defer = bool(fused) and L > 1
        forms += [h16_form(x2, True, T, d, pl * 4 * d, planes > 0, int(f2_defer), deferred(T, d, pl * 4 * d) if f2_defer else 0, keys)]
    forms += [f32_form(2, T, d, d, head_ws, head_planes, keys), f32_form(2, T, d // 2, d, head_ws, head_planes, keys)]
    if cdt == 3 and force_dtype is None:      # rap_workspace_bytes of a split-precision model covers both layouts (tuning key 17 may change)
        ws = max(plan(mode, TP, B, nseg, d, heads, L, rows, in_dim, bounded, keys, force_dtype=fd).ws_bytes for fd in (0, 3))
    else:
        ws = workspace_bytes(dtype, h16_stream, planes, d, L, Ks, TP, T, B, nseg, rows)
    return Plan(dtype, T, bq, kg, items_p, items_b, rp[0], rb[0], rp[1], rb[1], fused, planes, *forms, ws)


def lib_plan(lib, mode, TP, B, nseg, d=D, heads=HEADS, L=LAYERS, rows=STEPS, in_dim=0, bounded=True):
    """rap_call_plan with the library's CURRENT tuning keys -> Plan"""
    out = (ctypes.c_int64 * len(FIELDS))()
    cdt, rdt = (DT[x] for x in MODES[mode])
    rc = lib.rap_call_plan(cdt, rdt, d, heads, L, in_dim, TP, B, nseg, rows, int(bounded), ctypes.cast(out, ctypes.c_void_p), len(FIELDS))
    assert rc == 0, (rc, mode, TP, B, nseg, d)
    return Plan(*out)


def row_signature(p):
    """what of a plan depends on the row count alone (given the mode): the arithmetic, the attention item geometry, the fusion, the
    planes, the eight forms (bf16 and fp16 operands count as one arithmetic: their forms are the same function)"""
    return ({2: 1}.get(p.dtype, p.dtype), p.attn_bq, p.attn_kg, p.fused, p.planes) + tuple(p[FIELDS.index("f_static"):FIELDS.index("ws_bytes")])


def branch_states(p):
    """(key ranges, one block per CU) of the per-part and of the per-sample branch"""
    return (p.ranges_part, p.percu_part), (p.ranges_batch, p.percu_batch)


@contextlib.contextmanager
def tuned(lib, pairs):
    """gemm_cases.tuned (the keys are back at their defaults afterwards) together with the key table the restated plan takes"""
    import gemm_cases as GC
    keys = dict(KEYS)
    keys.update(dict(pairs))
    with GC.tuned(lib, pairs):
        yield keys


# ---------------------------------------------------------------------------------------------
# geometries
# ---------------------------------------------------------------------------------------------
MIN_PART = 24
SAMPLE_TOKENS = 3600          # samples of a many-token geometry average this and stay below ~4 150 (weights 0.85 .. 1.15)


def _ragged(total, n, lo, key, spread=0.5):
    """n seeded sizes >= lo that sum to total, within a factor (1 +- spread) of each other's share"""
    assert total >= n * lo, (total, n, lo)
    g = torch.Generator().manual_seed(hash_key(key))
    w = 1.0 - spread + 2.0 * spread * torch.rand(n, generator=g, dtype=torch.float64)
    extra = ((total - n * lo) * w / w.sum()).floor().to(torch.int64)
    sizes = [lo + int(e) for e in extra]
    sizes[int(torch.argmax(w))] += total - sum(sizes)
    return sizes


def hash_key(key):
    import zlib
    return zlib.crc32(repr(key).encode())


def row_geometry(TP):
    """-> part-size lists of TP tokens: samples of at most about 4 100 tokens with 3 and 2 ragged parts in turn (P = 3: every second
    sample has an EMPTY trailing part, counted in nseg_part = B x P), two samples at least"""
    B = max(2, _cdiv(TP, SAMPLE_TOKENS))
    samples = _ragged(TP, B, MIN_PART * 3, ("samples", TP), spread=0.15)
    return [_ragged(n, 3 if b % 2 == 0 else 2, MIN_PART, ("parts", TP, b)) for b, n in enumerate(samples)]


def worklist_geometry(TP, parts_per_sample):
    """-> part-size lists of TP tokens for samples of the given REAL part counts (P = the largest: the others end in empty parts)"""
    B = len(parts_per_sample)
    samples = _ragged(TP, B, MIN_PART * max(parts_per_sample), ("wl-samples", TP, tuple(parts_per_sample)), spread=0.2)
    return [_ragged(n, k, MIN_PART, ("wl-parts", TP, tuple(parts_per_sample), b), spread=0.3) for b, (n, k) in enumerate(zip(samples, parts_per_sample))]


Member = collections.namedtuple("Member", "name parts TP B P nseg")
Pair = collections.namedtuple("Pair", "name kind low high modes")      # modes: {mode: the set of FIELDS that differ between low and high}


def member(name, parts, P=None):
    P = P if P is not None else max(len(p) for p in parts)
    assert all(n >= MIN_PART for p in parts for n in p), name
    return Member(name, parts, sum(sum(p) for p in parts), len(parts), P, len(parts) * P)


@functools.lru_cache(maxsize=None)
def inputs(m):
    """the seeded packed batch of a member (rap_amd.synthetic.make_inputs; P = m.P, so short samples end in empty parts)"""
    return S.make_inputs([list(p) for p in m.parts], seed=hash_key(("inputs", m.name)) % 100000, max_parts=m.P)


def _freeze(parts):
    return tuple(tuple(p) for p in parts)


def _row_pair(low, modes, kind="rows"):
    return Pair(f"rows-{low}", kind, member(f"rows-{low}", _freeze(row_geometry(low)), 3), member(f"rows-{low + 1}", _freeze(row_geometry(low + 1)), 3), modes)


_H16_ITEMS = {"attn_bq", "attn_kg", "items_part", "items_batch"}
_SMALL = ("f32", "x2", "bf16h", "f16")
# Row boundaries (TQ low | high = low + 256) of a d = 512 model at the default tuning keys, and per mode the fields that change there.
ROW_PAIRS = [
    # a split-precision model switches from the exact-fp32 kernels to split precision (tuning key 17)
    _row_pair(768, {"x2": {"dtype", "percu_part", "percu_batch", "fused", "planes", "f_qkv", "f_out", "f_ff1", "f_ff2"}}),
    # 16-bit and split precision: ff1 leaves the four-stage ring (tuning key 18: more than 256 blocks of 128 x 128)
    _row_pair(1024, {"x2": {"f_ff1"}, "bf16h": {"f_ff1"}, "f16": {"f_ff1"}}),
    # fp32: out-projection and head layer 0 lose their 4-way split K.  16-bit: attention 64 rows x 4 key groups -> 128 x 2, planes 4 -> 2,
    # head layer 1 takes 2 planes, head layer 0 none.  Split precision: out-projection and ff2 4 -> 2 (its attention ranges are a matter of
    # the work list, not of the rows)
    _row_pair(2048, {"f32": {"f_out", "f_head0"}, "x2": {"planes", "f_out", "f_ff2", "f_head0", "f_head1"},
                     "bf16h": _H16_ITEMS | {"planes", "f_ff2", "f_head0", "f_head1"}, "f16": _H16_ITEMS | {"planes", "f_ff2", "f_head0", "f_head1"}}),
    # 16-bit and split precision: QKV leaves the four-stage ring
    _row_pair(2560, {"x2": {"f_qkv"}, "bf16h": {"f_qkv"}, "f16": {"f_qkv"}}),
    # 16-bit and split precision: ff1 moves from 128 x 128 tiles to the 256 x 256 kernel while the planes and the fusion stay on
    _row_pair(3840, {"x2": {"f_ff1"}, "bf16h": {"f_ff1"}, "f16": {"f_ff1"}}),
    # fp32: ff2 and head layer 1 lose split K.  16-bit and split precision: no planes, fusion off, attention 256 x 1
    _row_pair(4096, {"f32": {"f_ff2", "f_head1"}, "x2": {"fused", "planes", "f_out", "f_ff2", "f_head1"},
                     "bf16h": _H16_ITEMS | {"fused", "planes", "f_ff2", "f_head1"}, "f16": _H16_ITEMS | {"fused", "planes", "f_ff2", "f_head1"}}),
    # ff1 goes persistent (all modes)
    _row_pair(7936, {"f32": {"f_ff1"}, "x2": {"f_ff1"}, "bf16h": {"f_ff1"}}),
    # 16-bit and split precision: the unsplit out-projection and ff2 leave the four-stage ring
    _row_pair(8192, {"x2": {"f_out", "f_ff2"}, "f16": {"f_out", "f_ff2"}}),
    # 16-bit and split precision: QKV 128 x 128 -> 256 x 256
    _row_pair(10752, {"x2": {"f_qkv"}, "f16": {"f_qkv"}}),
    # QKV goes persistent (all modes)
    _row_pair(21760, {"f32": {"f_qkv"}, "x2": {"f_qkv"}, "bf16h": {"f_qkv"}}),
    # 16-bit and split precision: out-projection and ff2 leave the 128 x 128 tiles
    _row_pair(32512, {"x2": {"f_out", "f_ff2"}, "f16": {"f_out", "f_ff2"}}),
]

# Work-list boundaries: calls of about 1 100 tokens (TP / 256 = 4, TQ = 1 280: above tuning key 17's default), max_items = 4 + segments + 1.
WL_TOKENS = 1100


def _wl_pair(name, low_parts, high_parts, modes, P_low=None, P_high=None, tokens=WL_TOKENS):
    lo = member(f"{name}-low", _freeze(worklist_geometry(tokens, low_parts)), P_low)
    hi = member(f"{name}-high", _freeze(worklist_geometry(tokens, high_parts)), P_high)
    return Pair(name, "worklist", lo, hi, modes)


WORKLIST_PAIRS = [
    # nseg_part 7 | 8 (max_items 12 | 13): fp32 4 ranges one block per CU -> 4 ranges plain launch; split precision 4 -> 2 ranges
    _wl_pair("nseg-7-8", [6], [4, 3], {"f32": {"percu_part"}, "x2": {"ranges_part"}}, P_low=7, P_high=4),
    # 15 | 16 (20 | 21): fp32 4 ranges plain -> 2 ranges one block per CU
    _wl_pair("nseg-15-16", [5, 4, 5], [4, 4, 3, 4], {"f32": {"ranges_part", "percu_part"}}),
    # 19 | 20 (24 | 25): fp32 2 ranges one per CU -> 2 ranges plain; split precision 2 -> 1
    _wl_pair("nseg-19-20", [18], [5, 5, 4, 5], {"f32": {"percu_part"}, "x2": {"ranges_part"}}, P_low=19, P_high=5),
    # 35 | 36 (40 | 41): fp32 2 ranges plain -> unsplit
    _wl_pair("nseg-35-36", [7, 7, 6, 7, 7], [6, 6, 5, 6, 6, 6], {"f32": {"ranges_part"}}),
    # the per-sample branch instead: B = 15 | 16 (max_items_batch 20 | 21).  One-part samples have nseg_part = B, so there both branches
    # move together; with ONE two-part sample (P = 2: every other sample ends in an empty part) the part branch sits at 2 plain ranges on both
    # sides and only the per-sample branch goes 4 ranges plain -> 2 ranges one per CU
    _wl_pair("batch-15-16-one-part", [1] * 15, [1] * 16, {"f32": {"ranges_part", "percu_part", "ranges_batch", "percu_batch"}}),
    _wl_pair("batch-15-16", [2] + [1] * 14, [2] + [1] * 15, {"f32": {"ranges_batch", "percu_batch"}}),
]
WL_ALWAYS = {"items_part", "items_batch", "ws_bytes"}      # (whichever of the two item counts moves; the bytes follow the tables)
PAIRS = ROW_PAIRS + WORKLIST_PAIRS


def cases():
    """-> [(pair, 'low' | 'high', member, mode)] in a stable order"""
    return [(p, side, getattr(p, side), mode) for p in PAIRS for side in ("low", "high") for mode in p.modes]


def case_id(pair, side, mode):
    return f"{getattr(pair, side).name}-{mode}"


def members():
    seen = {}
    for p in PAIRS:
        for m in (p.low, p.high):
            seen[m.name] = m
    return list(seen.values())


# ---------------------------------------------------------------------------------------------
# bounds (restated; the host test asserts they are the numbers of the tests they come from)
# ---------------------------------------------------------------------------------------------
# tests/test_fullconfig_gpu.py: TOL_CLOUD, TOL_R, TOL_T and the two "what an exact-fp32 path achieves" bounds of _assert_fp32
FP32_TOL_CLOUD, FP32_TOL_R, FP32_TOL_T, FP32_SAMPLE_CLOUD, FP32_SHARP_R = 5e-4, 1e-3, 1e-3, 5e-5, 1e-4


def assert_fp32(e, inside=1.0):
    """test_fullconfig_gpu._assert_fp32 on an _errors(...) row, `inside` times tighter"""
    assert inside * e["worst_step_cloud"] <= FP32_TOL_CLOUD and inside * e["worst_step_x_t"] <= FP32_TOL_CLOUD, e
    assert inside * e["final_cloud"] <= FP32_TOL_CLOUD and inside * e["R_frob"] <= FP32_TOL_R and inside * e["t"] <= FP32_TOL_T, e
    assert inside * e["per_sample_final_cloud_max"] < FP32_SAMPLE_CLOUD and inside * e["R_frob"] < FP32_SHARP_R, e


# Measured on one MI355X over all 76 sampling cases (the GPU test records every case in plan_edges.jsonl): fp32 and split precision -- worst step
# cloud 8.0e-7, |dR|_F 1.7e-6, t 3.4e-7, per-sample final cloud 8.0e-7 (the plain fp32 device oracle on the same inputs: up to 2.3e-6 /
# 4.3e-6: the kernels sit closer to float64 than torch's fp32 does, so no bound here needed the yardstick rule); bf16 operands on the fp16
# stream -- cloud 1.1e-3, |dR|_F 2.3e-3; fp16 operands -- cloud 1.2e-4, |dR|_F 1.5e-4.  Forward calls: fp32-accurate modes velocity 4.0e-7 and
# features 4.3e-6 (max |f| 7.5), bf16 1.4e-3 / 2.1e-3 of the maxima, fp16 1.3e-4 / 1.8e-4.
YARDSTICK_MARGIN = 4.0      # the fp32 oracle has to sit this far inside the fp32 bounds on the ~1 100-token geometries (the host test)
# tests/test_h16_gpu.py (test_baseline_geometries_h16_agrees_with_fp32_path): final cloud and |dR|_F of a sampling call in 16-bit arithmetic;
# tests/test_small_call_gpu.py holds every flow step's end points to 2e-2 in both
H16_SAMPLE_BOUND = {"bfloat16": 2e-2, "float16": 3e-3}
H16_STEP_BOUND = 2e-2
# tests/test_widths_gpu.py (forward): fp32-accurate modes -- velocity 1e-4 of max|v| and 2e-5 absolute, features 2e-4; 16-bit modes --
# FWD_REL_BOUND of tests/test_h16_gpu.py on the velocity (x 2 for fp16 operands on the fp16 stream), 4 x that on the features
FWD_FP32_V_REL, FWD_FP32_V_ABS, FWD_FP32_F_ABS = 1e-4, 2e-5, 2e-4
FWD_REL_BOUND = {"bfloat16": 8e-3, "float16": 1e-3}
FWD_PAIRS = ("rows-2048", "rows-4096")
BITID_MEMBERS = ("rows-2049", "rows-3841")      # two planes, fusion on (the neighbouring 2 048 and 4 096 are tests/test_small_call_gpu.py's)
BITID_MODES = ("bf16h", "x2")
BITID_X2_TOL = 5e-6                             # tests/test_small_call_gpu.py: split precision re-associates the out-projection's k-sum

