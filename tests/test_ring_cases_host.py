"""CPU: the cases of tests/test_ring_edges_gpu.py are what they are there for, and its references stand on their own.

  * the restated bounds are the suite's own numbers;
  * every case reaches what it is listed for, computed from the launch arithmetic restated in tests/ring_cases.py: row tails, blocks that
    straddle a head or the q / k plane boundary, the second pass of every capped grid (with the sizes just inside and just past the cap
    both in the table), lanes that idle or take a second trip, chunk counts of the sanitiser and of the adaLN rows;
  * a plain fp32 torch evaluation of the same formula meets every bound on every case with a factor 2 to spare (the kernels sum in another
    order than torch; both are O(eps) algorithms, so a factor 2 separates an order change from a wrong formula).  Two places where that
    factor cannot exist, stated where they are asserted: an output rounded ONCE into a 16-bit type sits AT one rounding by construction
    (there the fp32 value before the rounding is held to half of the slack, and the rounded one to the bound), and the LayerNorm rows with
    a 1e4 outlier (ring_cases.LN_YARDSTICK_MARGIN);
  * the wrong kernels the sweep is there for -- a one-pass variance, head = r / (TP + 1), a dropped second grid pass, swapped sin / cos,
    a sanitiser that loses the prefix at a chunk boundary -- move the references by far more than the bounds;
  * every refusal of the entry points, through the library loaded on the CPU: RAP_ERR_INVALID before any launch.
"""
import ctypes

import pytest
import torch

import ln_stream_cases as L
import ring_cases as C
import test_h16_gpu as TH
import test_kernels_gpu as TK
import test_x2_gpu as TX
from rap_amd import _lib

N, X = ctypes.c_void_p(0), ctypes.c_void_p(256)      # NULL; a non-NULL pointer value that is never dereferenced
BIG = 2 ** 32 + 4                                    # a row count an unchecked cast to int turns into 4


def test_the_bounds_are_the_suites_own():
    assert (C.GEMM_BOUND, C.NORM_BOUND, C.POSENC_BOUND, C.ADALN_BOUND) == (TK.GEMM_BOUND, TK.NORM_BOUND, TK.POSENC_BOUND, TK.ADALN_BOUND)
    assert C.ULP == TH.ULP and C.ONE_ROUNDING == TH.ONE_ROUNDING and C.NORM_SLACK == TH.NORM_SLACK and C.TORCH_DT == TH.TORCH_DT
    x = C.x2_source(32)[:, :32].contiguous()
    assert C.same_bits_or_both_nan(C.x2_pack_ref(x), TX.pack_ref(x))
    assert C.LN_ROWS is L.ROWS and C.LN_FORMS is L.FORMS


# ---------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------
def test_layernorm_table_reaches_every_tail_and_every_family_is_what_it_says():
    assert C.LN_WIDTHS == [256, 512, 768, 1024]
    assert {r % 4 for r in C.LN_ROWS if r <= 4} == {0, 1, 2, 3} and {r % 4 for r in C.LN_ROWS if r > 4} >= {0, 1, 3}
    assert C.LN_FAMILIES == ["benign", "mean50", "mean1000", "const", "zero", "tiny", "huge", "outlier"]
    t = L.token_rows(9).tolist()
    assert t != sorted(t) and t != sorted(t, reverse=True) and set(t) == set(range(L.TABLE_ROWS))
    for d in C.LN_WIDTHS:
        mod, gain, shift = C.ln_params(d)
        assert mod.shape == L.ln_params(d)[0].shape
        for v in (gain, shift, mod[0, L.MOD_SLOT, :d], mod[2, L.MOD_SLOT, d:]):
            assert v.unique().numel() == d                                 # a column read through another map is another value
        x = {f: C.ln_input(d, 1027, f) for f in C.LN_FAMILIES}
        assert torch.equal(x["benign"], L.stream_input(d, 1027))
        for f, m in (("mean50", 50.0), ("mean1000", 1000.0)):
            assert (x[f].mean(1) - m).abs().max() < 0.3 and (x[f].std(1) - 1).abs().max() < 0.3
        assert bool((x["const"] == 3.25).all()) and bool((x["zero"] == 0).all())
        assert x["tiny"].var(1).max() < 1e-5 / 300 and x["huge"].abs().max() > 3e6
        col = x["outlier"].abs().argmax(1)
        assert bool((x["outlier"][torch.arange(1027), col] == 1e4).all()) and bool((col[1:] != col[:-1]).all())
        assert int((x["outlier"] == 1e4).sum()) == 1027
        lanes, slots = (col // 4) % 64, col // 256
        assert lanes.unique().numel() == 64 and slots.unique().numel() == d // 256


@pytest.mark.parametrize("d", C.LN_WIDTHS)
def test_fp32_layernorm_meets_every_bound_and_a_one_pass_variance_does_not(d):
    worst = {f: 0.0 for f in C.LN_FAMILIES}
    err32 = {f: 0.0 for f in C.LN_FAMILIES}
    for f in C.LN_FAMILIES:
        for rows in C.LN_ROWS:
            x = C.ln_input(d, rows, f)
            for form in C.LN_FORMS:
                ref, bound = C.ln_ref64(x, form), C.ln_bound(x, form)
                err = float((C.ln_ref32(x, form).double() - ref).abs().max())
                assert err * C.LN_YARDSTICK_MARGIN[f] < bound, (f, rows, form, err, bound)
                worst[f], err32[f] = max(worst[f], err / bound), max(err32[f], err)
                if f in ("benign", "tiny", "huge", "zero"):
                    assert bound < 1.5 * C.NORM_BOUND, (f, bound)         # the cancellation term vanishes on the benign rows
                if f in C.LN_EXACT:
                    assert torch.equal(ref.float(), C.ln_shift_rows(form, d, rows))
                if f == "mean1000":
                    bad = float((C.ln_one_pass32(x, form).double() - ref).abs().max())
                    assert bad > 20 * bound, (rows, form, bad, bound)      # E[x^2] - mean^2 in fp32: percent-level
                if f == "benign":
                    assert float((C.ln_one_pass32(x, form).double() - ref).abs().max()) < bound     # ... and invisible to the old input
    print(f"d {d}: torch fp32 LayerNorm, worst error per family " + ", ".join(f"{f} {err32[f]:.1e} ({worst[f]:.2f} of the bound)" for f in C.LN_FAMILIES))


# ---------------------------------------------------------------------------------------------
# qk-norm
# ---------------------------------------------------------------------------------------------
def test_qknorm_table_straddles_heads_and_planes_and_holds_every_special_row():
    assert C.QK_HEADS == [1, 3, 8, 16] and C.QK_ROWS == [1, 15, 16, 17, 31, 33, 1027]
    for mode, rb in C.QK_ROWS_PER_BLOCK.items():
        st = {(H, TP): C.qk_blocks_straddling(H, TP, mode) for H in C.QK_HEADS for TP in C.QK_ROWS}
        assert all(planes == (H * TP % rb != 0) for (H, TP), (_, planes) in st.items())
        assert all(not heads for (H, TP), (heads, _) in st.items() if H == 1)
        for H in C.QK_HEADS[1:]:
            assert any(heads for (h, TP), (heads, _) in st.items() if h == H)
        assert any(planes for _, planes in st.values()) and any(not planes for _, planes in st.values())
        assert st[(3, 16)] == (rb == 32, rb == 32) and st[(3, 17)] == (True, True)
    for H in C.QK_HEADS:
        gq, gk = C.qk_gammas(H)
        assert torch.cat([gq, gk]).flatten().unique().numel() == 2 * H * 64 and bool((gq < 0).any()) and bool((gk < 0).any())
    # every kind of special row, in both planes, in a case whose blocks straddle
    for plane in (0, 1):
        kinds = {C.qk_kind(plane, r) for r in range(3 * 17)}
        assert kinds == {"plain", "zero", "onehot", "tiny", "huge"}
    x = C.qk_input(3, 17, 0)
    flat = x[0].reshape(-1, 64)
    r0 = [r for r in range(51) if C.qk_kind(0, r) == "zero"][0]
    r1 = [r for r in range(51) if C.qk_kind(0, r) == "onehot"][0]
    assert bool((flat[r0] == 0).all()) and int((flat[r1] != 0).sum()) == 1
    for mode in (0, 1, 2):
        tiny, huge = C.QK_SCALES[mode]
        xm = C.qk_input(3, 17, mode).float()
        assert torch.isfinite(xm).all() and torch.isfinite(xm * xm).all()       # squares inside fp32 (and the values inside the type)
        rt = [r for r in range(51) if C.qk_kind(1, r) == "tiny"][0]
        rh = [r for r in range(51) if C.qk_kind(1, r) == "huge"][0]
        k = xm[1].reshape(-1, 64)
        assert 0 < k[rt].abs().max() < 10 * tiny and k[rh].abs().max() > huge / 4


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["f32", "bf16", "f16"])
def test_fp32_qknorm_meets_the_bound_and_a_wrong_head_index_does_not(mode):
    worst = 0.0
    for H in C.QK_HEADS:
        for TP in C.QK_ROWS:
            x = C.qk_input(H, TP, mode)
            ref = C.qk_ref64(x)
            assert torch.isfinite(ref).all()
            err, bound = C.qk_error(mode, C.qk_ref32(x, mode), ref, H)
            if mode == 0:
                assert 2 * err < bound, (H, TP, err, bound)
            else:
                # one rounding into the type IS the bound: the rounded value meets it, the fp32 value before the rounding half of the slack
                assert err < bound, (H, TP, err, bound)
                pre = float(((C.qk_ref32(x.float(), 0) - ref).abs() / (ref.abs() + 1e-2)).max())
                assert 2 * pre < C.NORM_SLACK, (H, TP, pre)
            worst = max(worst, err / bound)
            if H > 1:
                # head = r / (TP + 1): the gammas of the neighbouring head from row TP on
                g = torch.stack(C.qk_gammas(H))
                r = torch.arange(H * TP)
                wrong = ref.reshape(2, H * TP, 64) / g[:, r // TP] * g[:, r // (TP + 1)]
                e_wrong, _ = C.qk_error(mode, wrong.reshape(ref.shape), ref, H)
                assert e_wrong > 100 * bound, (H, TP, e_wrong)
    print(f"mode {mode}: fp32 torch qk-norm, worst error {worst:.2f} of the bound")


# ---------------------------------------------------------------------------------------------
# positional encodings
# ---------------------------------------------------------------------------------------------
def test_posenc_table_reaches_every_block_tail_feature_width_and_magnitude():
    assert C.PE_ROWS == [1, 7, 8, 9, 15, 16, 17, 1027] and C.PE_FEAT_DIMS == [0, 4, 8, 32, 36, 40]
    assert {r % 8 for r in C.PE_ROWS} >= {0, 1, 7} and {r % 16 for r in C.PE_ROWS} >= {0, 1, 15}       # 8 / 16 tokens per block
    # threads 22 .. 31 own the float4 at columns 84 + 4 (j - 22): the table has a width at which the fc < F test of the first, of an inner
    # and of the last of them goes either way, and thread 31 writes a feature float4 (120 .. 123) AND the zero float4 124 .. 127 at F = 40
    for j, Fs in ((22, (0, 4)), (23, (4, 8)), (30, (32, 36)), (31, (36, 40))):
        fc = 4 * (j - 22)
        assert [fc < F for F in Fs] == [False, True]
    tok = C.pe_token_sample(9).tolist()
    assert tok != sorted(tok) and tok != sorted(tok, reverse=True) and set(tok) == {0, 1, 2}
    assert C.PE_SCALES.min() == 5.0 and C.PE_SCALES.max() == 50.0
    x = C.pe_coords(1027, "x")
    for m in C.PE_MAGNITUDES:
        rows = x[torch.tensor(C.PE_MAGNITUDES)[torch.arange(1027) % 4] == m]
        assert m / 2 < rows.abs().max() <= m
    assert float(x.abs().max()) * 512 > 50000
    zeros = x == 0
    assert int((zeros & ~torch.signbit(x)).sum()) > 50 and int((zeros & torch.signbit(x)).sum()) > 50           # +0 and -0
    ref = C.pe_x_ref64(x)
    assert bool((ref[:, :3] == x.double()).all()) and bool((ref[:, 63] == 0).all())
    assert sorted(sum((C.pe_columns_of_component(c) for c in range(3)), [])) == list(range(63))


def test_fp32_sin_cos_meets_the_posenc_bound_and_a_swapped_column_does_not():
    worst = 0.0
    for TP in C.PE_ROWS:
        x = C.pe_coords(TP, "x")
        e = float((C.pe_x_ref32(x).double() - C.pe_x_ref64(x)).abs().max())
        assert 2 * e < C.POSENC_BOUND, (TP, e)
        worst = max(worst, e)
        cond = C.pe_coords(TP, "cond")
        for Fd in C.PE_FEAT_DIMS:
            ref = C.pe_static_ref64(cond, Fd)
            e = float((C.pe_static_ref32(cond, Fd).double() - ref).abs().max())
            assert 2 * e < C.POSENC_BOUND, (TP, Fd, e)
            worst = max(worst, e)
            assert bool((ref[:, 84 + Fd:] == 0).all()) and ref.shape == (TP, 128)
            for c in C.pe_raw_columns_static(Fd):
                assert bool((ref[:, c] == ref[:, c].float().double()).all())      # raw columns are fp32 values: compared bitwise
    print(f"fp32 torch sin / cos against fp64: {worst:.2e}")
    ref = C.pe_x_ref64(C.pe_coords(17, "x"))
    swapped = ref.clone()
    swapped[:, 3:6], swapped[:, 6:9] = ref[:, 6:9], ref[:, 3:6]                  # cos where sin belongs, at one frequency
    assert float((swapped - ref).abs().max()) > 0.1


# ---------------------------------------------------------------------------------------------
# adaLN table
# ---------------------------------------------------------------------------------------------
def test_adaln_rows_reach_one_chunk_two_chunks_and_a_tail_and_fp32_meets_the_bound():
    chunks = {rows: divmod(rows, C.ADALN_CHUNK) for rows in C.ADALN_ROWS}
    assert chunks == {1: (0, 1), 7: (0, 7), 8: (1, 0), 9: (1, 1), 16: (2, 0), 17: (2, 1), 33: (4, 1)}
    t = C.adaln_t(33)
    assert {1.0, 0.0}.issubset(set(t.tolist())) and float(t[1]) == pytest.approx(1e-3) and float(t[3]) == float(t[4])     # a repeated value
    assert torch.equal(t[:8], t[8:16]) and torch.equal(t[:8], t[16:24]) and float(t[32]) == float(t[0])
    assert C.ADALN_MODELS == [(256, 1), (256, 2), (1024, 1), (1024, 2)]
    for d, L_ in C.ADALN_MODELS:
        sd = C.adaln_weights(d, L_)
        ref = C.adaln_ref(sd, L_, t)
        assert ref.shape == (33, 2 * L_, 2 * d)
        err = float((C.adaln_ref(sd, L_, t, torch.float32).double() - ref).abs().max())
        print(f"adaLN d {d} L {L_}: fp32 torch against fp64 {err:.2e}")
        assert 2 * err < C.ADALN_BOUND, (d, L_, err)
        assert torch.equal(ref[0], ref[8]) and float((ref[0] - ref[1]).abs().max()) > 100 * C.ADALN_BOUND      # rows differ where t does


# ---------------------------------------------------------------------------------------------
# head tail, Euler, the capped grids
# ---------------------------------------------------------------------------------------------
def test_head_tail_reaches_idle_lanes_second_trips_and_the_second_grid_pass():
    assert {K: C.head_lane_trips(K) for K in C.HEAD_KS} == {128: [0, 1], 256: [1], 384: [1, 2], 512: [2]}
    assert C.HEAD_LD_EXTRA == [0, 64] and C.HEAD_WAVES == 32768
    p = {TP: C.passes(TP, C.HEAD_WAVES) for TP in C.HEAD_ROWS}
    assert p[32768] == 1 and p[32769] == 2 and p[40001] == 2 and {TP % 4 for TP in C.HEAD_ROWS if TP < 8} == {0, 1, 3}
    for K in C.HEAD_KS:
        y, W = C.head_inputs(40001, K, 64)
        assert y.shape == (40001, K + 64) and bool(torch.isnan(y[:, K:]).all()) and torch.isfinite(y[:, :K]).all()
        ref = C.head_ref64(y, W)
        err = float(((y[:, :K] @ W.T).double() - ref).abs().max())
        assert 2 * err < C.GEMM_BOUND, (K, err)
        assert float((ref[:, [1, 0, 2]] - ref).abs().max()) > 1.0 and float((ref[32768:] - ref[:7233]).abs().max()) > 1.0      # a swapped column; a first-pass row in a second-pass slot
        print(f"head tail K {K}: fp32 torch against fp64 {err:.2e}")


def test_every_grid_cap_has_a_size_just_inside_and_just_past_it():
    p = {n: C.passes(n, C.EULER_THREADS) for n in C.EULER_NS}
    assert p[524288] == 1 and p[524289] == 2 and p[786432] == 2 and {1, 255, 256, 257} <= set(C.EULER_NS)
    p = {n: C.passes(n, C.MAXABS_THREADS) for n in C.MAXABS_NS}
    assert p[262144] == 1 and p[262145] == 2 and p[1000003] == 4 and {63, 64, 65} <= set(C.MAXABS_NS)
    # the three conversion grids are capped at 2^24 threads: the sizes just inside the cap are the whole rest of each table, the wrap case
    # is one block row past it (a case AT the cap would be another 0.5 GB for one more block of the same pass)
    assert C.CONVERT_WRAP_N % 4 == 0 and C.passes(C.CONVERT_WRAP_N // 4, C.CONVERT_PASS) == 2
    for dt in (1, 2):
        n = C.convert_table(dt).numel()
        assert n % 4 == 0 and C.passes(n // 4, C.CONVERT_PASS) == 1 and (C.CONVERT_PASS * 4) % n != 0      # tiled, it does not repeat with the grid's period
    rows, cols = C.X2_PACK_WRAP
    assert C.passes(rows * cols // 4, C.CONVERT_PASS) == 2 and C.passes((rows - 1) * cols // 4, C.CONVERT_PASS) == 1
    assert (C.CONVERT_PASS // (cols // 4)) % C.X2_ROWS != 0                      # the second pass starts on another row of the tiled source
    rows, cols = C.X2_UNPACK_WRAP
    assert C.passes(rows * cols, C.CONVERT_PASS) == 2 and C.passes((rows - 1) * cols, C.CONVERT_PASS) == 1
    assert (C.CONVERT_PASS // cols) % C.X2_ROWS != 0
    # a dropped second pass leaves the NaN / sentinel of the output: every GPU case compares the WHOLE output
    x, v = C.euler_inputs(524289)
    xn, x0 = C.euler_ref(x, v)
    assert torch.isfinite(xn).all() and torch.isfinite(x0).all() and not torch.equal(xn, x) and not torch.equal(x0, xn)
    assert C.EULER_FORMS == ["separate", "in_place", "trajectory"]


# ---------------------------------------------------------------------------------------------
# conversions
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [1, 2], ids=["bf16", "f16"])
def test_conversion_table_holds_every_pattern_tie_and_edge(dt):
    x = C.convert_table(dt)
    ref = C.convert_ref(x, dt)
    T = C.TORCH_DT[dt]
    pat = x[:65536]
    assert pat.to(T).view(torch.int16).to(torch.int32).unique().numel() > 65536 - 2100         # every pattern (NaN payloads may merge)
    assert int(torch.isnan(x).sum()) > 100 and int(torch.isinf(x).sum()) >= 4
    fin = torch.isfinite(x)
    back = ref.float()
    tie = fin & torch.isfinite(back) & ((x.double() - back.double()).abs() * 2 == (torch.nextafter(ref, torch.full_like(ref, C._I)).double() - back.double()).abs())
    assert int(tie.sum()) > 30000                                                # exact half-way points ...
    assert bool(((ref[tie].view(torch.int16) & 1) == 0).all())                  # ... go to the even neighbour
    assert int((fin & torch.isinf(back)).sum()) > 0                              # finite values that overflow the type
    tiny = torch.finfo(T).tiny
    assert int(((back != 0) & (back.abs() < tiny)).sum()) > 100                  # the type's subnormals
    assert int((fin & (x != 0) & (x.abs() < 2.0 ** -126)).sum()) > 0             # fp32 subnormals
    assert torch.equal(torch.isnan(ref), torch.isnan(x))


def test_split_precision_references_hold_their_bound_and_clip():
    assert C.X2_COLS == [32, 512, 2048]
    for cols in C.X2_COLS:
        src = C.x2_source(cols)
        assert src.shape == (C.X2_ROWS, cols + C.X2_LD_EXTRA)
        x = src[:, :cols].contiguous()
        p = C.x2_pack_ref(x)
        back = TX.unpack_ref(p, cols)
        clip = C.x2_clipped(x)
        ok = ~torch.isnan(x)
        assert bool(((back - clip.double()).abs()[ok] <= C.x2_pair_bound(clip)[ok]).all())
        assert bool(torch.isnan(back[~ok]).all()) and int((~ok).sum()) >= 2
        big = ok & (x.abs() > C.F16_MAX)
        assert int(big.sum()) >= 4 and bool((back[big] == torch.sign(x[big]).double() * C.F16_MAX).all())
        assert bool((C.x2_unpack_ref(p, cols).double()[ok] == back.float().double()[ok]).all())


# ---------------------------------------------------------------------------------------------
# max |x|, sanitiser, logit bound, interleave
# ---------------------------------------------------------------------------------------------
def test_max_abs_cases_place_the_maximum_first_last_and_in_the_second_pass():
    cases = C.maxabs_cases()
    assert {c.n for c in cases} == set(C.MAXABS_NS) and {c.place for c in cases} == set(C.MAXABS_PLACES)
    assert {c.negative for c in cases} == {True, False}
    for c in cases:
        i = C.maxabs_index(c.n, c.place)
        assert 0 <= i < c.n
        if c.place == "second_pass":
            assert c.n > C.MAXABS_THREADS and C.MAXABS_THREADS <= i < c.n
    assert {c.n for c in cases if c.place == "second_pass"} == {262145, 1000003}
    c = [c for c in cases if c.n == 1000003 and c.place == "second_pass"][0]
    x = C.maxabs_input(c)
    assert int(torch.isnan(x).sum()) > 1000 and C.maxabs_ref_bits(x) == int(C.bits32(torch.tensor([77.5]))[0])
    assert C.maxabs_ref_bits(x[:C.MAXABS_THREADS]) != C.maxabs_ref_bits(x)       # a dropped second pass misses it
    for name, (vals, want) in C.MAXABS_SPECIALS.items():
        assert C.maxabs_ref_bits(torch.tensor(vals)) == want, name


def test_sanitiser_tables_reach_one_and_several_chunk_entries_and_a_boundary_slip_shows():
    assert C.SAN_NS == [1, 2, 1023, 1024, 1025, 2048, 2049, 5001]
    assert {n: C.san_per(n) for n in C.SAN_NS} == {1: 1, 2: 1, 1023: 1, 1024: 1, 1025: 2, 2048: 2, 2049: 3, 5001: 5}
    for n in C.SAN_NS:
        per = C.san_per(n)
        for table in C.SAN_TABLES:
            cu, limit = C.san_table(n, table)
            ref = C.san_ref(cu, limit)
            assert cu.dtype == torch.int32 and cu.numel() == n and 0 <= int(ref.min()) and int(ref.max()) <= limit
            assert bool((ref[1:] >= ref[:-1]).all())
            if table == "consistent":
                assert torch.equal(ref, cu)
            if table == "limit0":
                assert limit == 0 and bool((ref == 0).all())
            if table == "negative":
                assert int((cu < 0).sum()) >= 1
            if table == "above_limit" and n > 2:
                assert int((cu > limit).sum()) >= 1 and int(ref[-1]) == limit
            dip = C.san_dip(n, table)
            if dip is not None:
                i, j = dip
                assert j == i + 1 and int(cu[j]) < int(cu[i]) and int(ref[-1]) == int(cu[i])
                if table == "dip_on_boundary":
                    assert j % per == 0 and i // per != j // per
                    # a sanitiser that drops the prefix over the chunk maxima (each chunk on its own) differs from the chunk after the spike on
                    alone = torch.cat([torch.cummax(cu[k:k + per].clamp(0, limit), 0).values for k in range(0, n, per)])
                    assert not torch.equal(alone.to(torch.int32), ref)
                else:
                    assert per >= 2 and i // per == j // per
    assert all(C.san_dip(n, "dip_on_boundary") is not None for n in C.SAN_NS if n >= 2)
    assert {n for n in C.SAN_NS if C.san_dip(n, "dip_in_chunk") is not None} == {1025, 2048, 2049, 5001}


def test_logit_bound_cases_and_the_fp32_chain():
    assert C.BOUND_HEADS == [1, 4, 8, 12, 16]
    for H in C.BOUND_HEADS:
        for aligned in (False, True):
            gq, gk = C.bound_gammas(H, aligned)
            for h in range(H):
                lq, lk = int(gq[h].abs().argmax()), int(gk[h].abs().argmax())
                assert lq == C.bound_lane(h) and lk == (lq if aligned else C.BOUND_LANES[(h + 1) % 4])
                assert (float(torch.sign(gq[h, lq])), float(torch.sign(gk[h, lk]))) == tuple(float(s) for s in C.BOUND_SIGNS[h % 4])
            ref, b32 = C.bound_ref64(gq, gk), C.bound_ref32(gq, gk)
            for h in range(H):
                want = float(ref[h]) * C.BOUND_SLACK
                assert float(b32[h]) >= float(ref[h]) and abs(float(b32[h]) - want) <= 2 * C.ulp32(want)
    assert {0, 63} <= {C.bound_lane(h) for h in range(4)} and {s for h in range(4) for s in C.BOUND_SIGNS[h]} == {1, -1}
    # the one-hot rows are the tight case: in exact arithmetic q.k / 8 IS 8 max|gamma_q| max|gamma_k|
    for H in C.BOUND_HEADS:
        gq, gk = C.bound_gammas(H, True)
        x = C.bound_onehot_rows(H)
        g = torch.stack([gq, gk]).double()[:, :, None, :]
        qk = torch.nn.functional.normalize(x.double(), dim=-1) * g * 8.0
        s = (qk[0][:, :, None, :] * qk[1][:, None, :, :]).sum(-1) / 8.0           # (H, TP, TP): every query against every key
        ref = C.bound_ref64(gq, gk)
        assert float((s / ref[:, None, None] - 1).abs().max()) < 1e-12
    # two operand roundings of unit roundoff u: (1 + u)^2 fits the 0.1 % slack in fp16 (and fp32), and 1 + 2^-7 times it in bf16
    assert C.BOUND_EXCESS == {0: 1.0, 2: 1.0, 1: 1 + 2.0 ** -7}
    assert (1 + C.ULP[2]) ** 2 < C.BOUND_SLACK < (1 + C.ULP[1]) ** 2 < C.BOUND_SLACK * (1 + 2.0 ** -7)
    for dt in (1, 2):                                                             # the worst-case gammas round UP by nearly a whole u
        g8 = torch.tensor([8 * C.BOUND_WORST_GAMMA[dt]])
        assert float(g8) == 8 * C.BOUND_WORST_GAMMA[dt] and float(g8.to(C.TORCH_DT[dt])) == 8 * (1 + 2 * C.ULP[dt])
        gq, gk = C.bound_gammas(4, True)
        assert float(gq[dt - 1].abs().max()) == C.BOUND_WORST_GAMMA[dt] == float(gk[dt - 1].abs().max())


def test_geglu_interleave_reference_is_a_permutation():
    assert C.GEGLU_INNERS == [32, 64, 96, 1024] and C.GEGLU_KS == [1, 64, 255, 256, 257, 1024]
    for inner in C.GEGLU_INNERS:
        src = C.geglu_source_rows(inner)
        assert sorted(src.tolist()) == list(range(2 * inner))
        assert src[:32].tolist() == list(range(32)) and src[32:64].tolist() == list(range(inner, inner + 32))
        W, b = C.geglu_inputs(inner, 257)
        assert W.flatten().unique().numel() == W.numel() and b.unique().numel() == b.numel() and float(W.max()) < 2 ** 24


# ---------------------------------------------------------------------------------------------
# refusals: RAP_ERR_INVALID before any launch (there is no device here to launch on)
# ---------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = _lib.load()

    def ln_mod(x=X, out=X, TP=4, d=512, mod=X):
        return lib.rap_layernorm_mod(x, out, TP, d, mod, 0, N, N)

    def ln_aff(x=X, out=X, TP=4, d=512, gain=X, shift=X):
        return lib.rap_layernorm_affine(x, out, TP, d, gain, shift, N)

    def qkn(qkv=X, TP=4, heads=8, gq=X, gk=X):
        return lib.rap_qknorm(qkv, TP, heads, gq, gk, N)

    def qkh(dtype=1, qk=X, TP=4, heads=8, gq=X, gk=X):
        return lib.rap_qknorm_h16(dtype, qk, TP, heads, gq, gk, N)

    def pex(x=X, ax=X, TP=4):
        return lib.rap_posenc_x(x, ax, TP, N)

    def pes(cond=X, scales=X, tok=X, feat=X, Fd=8, out=X, TP=4):
        return lib.rap_posenc_static(cond, scales, tok, feat, Fd, out, TP, N)

    def head(y=X, ldy=256, W=X, v=X, TP=4, K=256):
        return lib.rap_head_out3(y, ldy, W, v, TP, K, N)

    def euler(x=X, v=X, x0=X, xn=X, n=4):
        return lib.rap_euler_step(x, v, 0.5, 0.05, x0, xn, N, n, N)

    def conv(dtype=1, src=X, dst=X, n=8):
        return lib.rap_convert_h16(dtype, src, dst, n, N)

    def pack(src=X, ld=64, rows=4, cols=64, dst=X):
        return lib.rap_x2_pack(src, ld, rows, cols, 1.0, dst, N)

    def unpack(src=X, rows=4, cols=64, dst=X):
        return lib.rap_x2_unpack(src, rows, cols, 1.0, dst, N)

    def maxabs(x=X, n=4, out=X):
        return lib.rap_max_abs(x, n, out, N)

    def bound(gq=X, gk=X, heads=8, out=X):
        return lib.rap_qk_logit_bound(gq, gk, heads, out, N)

    def san(cu=X, n=4, limit=100, out=X):
        return lib.rap_sanitize_cu(cu, n, limit, out, N)

    def glu(W=X, b=X, Wp=X, bp=X, inner=64, K=64):
        return lib.rap_geglu_interleave(W, b, Wp, bp, inner, K, N)

    # a NULL required operand of each, at a positive row count and at none
    required = [(ln_mod, "TP", ("x", "out", "mod")), (ln_aff, "TP", ("x", "out", "gain", "shift")), (qkn, "TP", ("qkv", "gq", "gk")),
                (qkh, "TP", ("qk", "gq", "gk")), (pex, "TP", ("x", "ax")), (pes, "TP", ("cond", "scales", "tok", "out")),
                (head, "TP", ("y", "W", "v")), (euler, "n", ("x", "v", "x0", "xn")), (conv, "n", ("src", "dst")),
                (pack, "rows", ("src", "dst")), (unpack, "rows", ("src", "dst")), (maxabs, "n", ("x", "out")), (san, "n", ("cu", "out"))]
    for f, count, names in required:
        for k in names:
            for rows in (4, 0):
                assert f(**{k: N, count: rows}) == -1, (f.__name__, k, rows)
        assert f(**{count: -1}) == -1, f.__name__                              # a negative row count or n
        assert f(**{count: 0}) == 0, f.__name__                                # zero rows with valid arguments: RAP_OK, nothing launched
    for k in ("gq", "gk", "out"):
        assert bound(**{k: N}) == -1
    for k in ("W", "b", "Wp", "bp"):
        assert glu(**{k: N}) == -1
    assert lib.rap_adaln_table(N, X, 4, X, X, N) == -1
    # a row count above INT32_MAX where the launcher takes an int: refused, never truncated (2^32 + 4 is not 4 rows)
    for f in (ln_mod, ln_aff, qkn, qkh, pex, pes, head):
        assert f(TP=BIG) == -1 and f(TP=2 ** 31) == -1, f.__name__
    assert ln_mod(TP=2 ** 31 - 1) == -1 and head(TP=2 ** 31 - 2) == -1          # (rows are rounded up to the 4 of a block)
    assert qkn(TP=2 ** 31 - 1, heads=16) == -1                                  # 2 * 16 * TP / 16 blocks: beyond the grid limit
    # feat == NULL with feat_dim > 0; feature widths outside {0, 4, ..., 40}
    assert pes(feat=N, Fd=8) == -1 and pes(feat=N, Fd=8, TP=0) == -1 and pes(feat=N, Fd=0, TP=0) == 0
    for Fd in (-4, 2, 6, 44, 48):
        assert pes(Fd=Fd) == -1 and pes(Fd=Fd, TP=0) == -1, Fd
    # heads <= 0
    for h in (0, -1):
        assert qkn(heads=h) == -1 and qkh(heads=h) == -1 and qkn(heads=h, TP=0) == -1 and qkh(heads=h, TP=0) == -1 and bound(heads=h) == -1
    for dt in (0, 3, -1):
        assert qkh(dtype=dt) == -1 and qkh(dtype=dt, TP=0) == -1 and conv(dtype=dt) == -1 and conv(dtype=dt, n=0) == -1
    # d or K outside the accepted set
    for d in (0, 128, 384, 500, 1280, 2048, -256):
        assert ln_mod(d=d) == -1 and ln_aff(d=d) == -1 and ln_mod(d=d, TP=0) == -1 and ln_aff(d=d, TP=0) == -1, d
    for K in (0, 64, 192, 320, 500, 640, 1024, -128):
        assert head(K=K, ldy=1024) == -1 and head(K=K, ldy=1024, TP=0) == -1, K
    assert head(K=256, ldy=192) == -1 and head(K=256, ldy=258) == -1 and head(K=256, ldy=320, TP=0) == 0      # ldy >= K, rows move as float4
    # the interleave
    for inner, K in ((0, 64), (-32, 64), (48, 64), (64, 0), (64, -1)):
        assert glu(inner=inner, K=K) == -1, (inner, K)
    for n in (1, 2, 3, 6):
        assert conv(n=n) == -1
    assert pack(cols=48) == -1 and pack(ld=32) == -1 and pack(ld=66) == -1 and pack(cols=-32) == -1 and unpack(cols=48) == -1 and unpack(cols=48, rows=0) == -1
    assert san(limit=-1) == -1 and san(limit=2 ** 31) == -1 and san(limit=0, n=0) == 0
    assert lib.rap_version() == _lib.ABI_VERSION == 6                           # additive: the ABI version stays
