"""CPU: the cases of tests/test_ln_stream_gpu.py are what they are there for, and its references stand on their own -- the tables hold
every (mode, width) with every row tail, both column maps, every split count with and without a bias; every special value is produced by the
fp32 sum; a plain fp32 torch LayerNorm of the stored value, rounded once into the output type, meets the stated bound against the fp64
reference on EVERY case (so the bounds can be met before anything runs on a GPU); a dropped, repeated or exchanged plane changes every
fused case's stream value; and the new entry points refuse bad arguments before anything touches the device."""
import ctypes
import itertools

import pytest
import torch

import ln_stream_cases as C
import test_h16_gpu as TH
import test_x2_gpu as TX
from rap_amd import _lib

N, X = ctypes.c_void_p(0), ctypes.c_void_p(256)      # NULL; a non-NULL pointer value that is never dereferenced
MODE_D = list(itertools.product(C.MODES, C.WIDTHS))


def test_the_bounds_are_the_suites_own():
    assert C.ULP == TH.ULP and C.ONE_ROUNDING == TH.ONE_ROUNDING and C.NORM_SLACK == TH.NORM_SLACK and C.TORCH_DT == TH.TORCH_DT
    assert C.X2_NORM_BOUND == TX.X2_NORM_BOUND
    assert all(C.x2_col(k) == TX.x2_col(k) for k in range(1024))


def test_tables_cover_every_mode_width_row_tail_split_count_and_bias():
    assert C.MODES == [(1, "f32"), (1, "f16"), (2, "f32"), (2, "f16"), (3, "f32")] and C.WIDTHS == [256, 512, 768, 1024]
    assert {C.row_tail(r) for r in C.ROWS} == {0, 1, 2, 3}
    assert {C.row_tail(r) for r in C.ROWS if C.blocks(r) == 1} == {0, 1, 2, 3}       # every tail in a block of its own ...
    assert {C.row_tail(r) for r in C.ROWS if C.blocks(r) > 1} >= {0, 1, 3}           # ... and behind full blocks
    assert max(C.ROWS) == 1027 and C.ROWS[:-1] == [1, 2, 3, 4, 5, 8, 9]
    for (dtype, stream), d in MODE_D:
        plain, fused = C.plain_cases(dtype, stream, d), C.fused_cases(dtype, stream, d)
        assert {(c.rows, c.form) for c in plain} == set(itertools.product(C.ROWS, C.FORMS))
        assert {(c.rows, c.splits) for c in fused} == set(itertools.product(C.ROWS, C.SPLITS))
        assert {(c.splits, c.bias) for c in fused} == set(itertools.product(C.SPLITS, (False, True)))
        assert {(c.rows, c.form) for c in fused} == set(itertools.product(C.ROWS, C.FORMS))
        assert {(C.row_tail(c.rows), c.bias) for c in fused} == set(itertools.product(range(4), (False, True)))
        assert all(c.dtype == dtype and c.stream == stream and c.d == d for c in plain + fused)
    assert C.SPLITS == [1, 2, 3, 4, 8] and len(C.PLANE_SCALES) == max(C.SPLITS)
    # the token rows: not monotone, the last table row in use (by the very first row), and a table wider than the slot that is read
    t = C.token_rows(9).tolist()
    assert t[0] == C.TABLE_ROWS - 1 and t != sorted(t) and t != sorted(t, reverse=True) and set(t) == set(range(C.TABLE_ROWS))
    assert 0 < C.MOD_SLOT < C.TABLE_SLOTS


def test_both_column_maps_occur_for_the_fp16_stream_and_differ_where_it_matters():
    wide = {d for d in C.WIDTHS if C.wide_map("f16", d)}
    assert wide == {512, 1024} and not any(C.wide_map("f32", d) for d in C.WIDTHS)
    for d in C.WIDTHS:
        nv = d // 256
        for stream in ("f32", "f16"):
            cols = sorted(C.column_of(stream, d, lane, i, j) for lane in range(64) for i in range(nv) for j in range(4))
            assert cols == list(range(d)), (stream, d)                     # each map is a permutation of the row
        moved = sum(C.column_of("f16", d, lane, i, 0) != C.column_of("f32", d, lane, i, 0) for lane in range(64) for i in range(nv))
        assert (moved > 0) == (d in wide)
        # a gain (shift, bias, plane) read through the other map is another column's value: the inputs are distinct per column
        mod, gain, shift = C.ln_params(d)
        for v in (gain, shift, C.bias_of(d), mod[0, C.MOD_SLOT, :d], mod[2, C.MOD_SLOT, d:], C.stream_input(d, 3)[1], C.planes(d, 3)[2, 1]):
            assert v.unique().numel() == d


def test_every_special_value_is_produced_by_the_sum():
    for d in C.WIDTHS:
        part, bias, h = C.special_inputs(d)
        base = C.special_inputs(d, with_specials=False)
        v = C.combine_sum(part, bias, h)
        st = C.store(v, "f16")
        bits = st.view(torch.int16).to(torch.int32) & 0xFFFF
        rows_with = sorted({r for r, *_ in C.SPECIALS.values()})
        assert sorted(rows_with + C.SPECIAL_CLEAN_ROWS) == list(range(C.SPECIAL_ROWS))
        for name, (r, _, p0, p1, hv, want) in C.SPECIALS.items():
            c = C.special_column(name, d)
            assert d - 256 <= c < d and float(bias[c]) == 0.0
            assert all(torch.isfinite(t[..., r, c]).all() for t in (part[:, None], h[None])) or name in ("minus_inf", "nan"), name
            if want is not None:
                assert int(bits[r, c]) == want, (name, hex(int(bits[r, c])))
            if name in C.SATURATED:
                assert float(st[r, c]) == C.SATURATED[name]
        at = lambda name: float(v[C.SPECIALS[name][0], C.special_column(name, d)])
        assert 65504 < at("above") < float("inf") and float("-inf") < at("below") < -65504
        p_above = float(part[0, 0, C.special_column("above", d)] + part[1, 0, C.special_column("above", d)])
        assert p_above < 65504                                          # only the residual carries it over the edge
        assert 65488 < at("rounds_max") < 65504 and 65504 < at("just_above") < 65520 and at("round_inf") == 65520
        assert torch.isinf(torch.tensor(at("round_inf")).to(torch.float16))      # what an unsaturated conversion would store
        assert at("plus_inf") == float("inf") and at("minus_inf") == float("-inf")
        assert torch.isfinite(part[:, 2, C.special_column("plus_inf", d)]).all()  # +inf by overflow of two finite planes
        assert at("nan") != at("nan")
        r, c = C.SPECIALS["nan"][0], C.special_column("nan", d)
        assert torch.isnan(st[r, c]) and int(torch.isnan(st).sum()) == 1 and int(torch.isnan(v).sum()) == 1
        r, c = C.SPECIALS["subnormal"][0], C.special_column("subnormal", d)
        assert 0 < float(st[r, c]) < 2.0 ** -14 and at("subnormal") > 0
        assert at("minus_zero") < 0 and at("half_even") == 1 + 2.0 ** -11 and at("half_odd") == 1 + 3 * 2.0 ** -11
        # the clean rows are the base case's rows, input for input
        for a, b in zip((part, bias, h), base):
            assert torch.equal(a[..., C.SPECIAL_CLEAN_ROWS, :] if a.dim() > 1 else a, b[..., C.SPECIAL_CLEAN_ROWS, :] if b.dim() > 1 else b)
        assert torch.equal(st[C.SPECIAL_CLEAN_ROWS], C.store(C.combine_sum(*base), "f16")[C.SPECIAL_CLEAN_ROWS])


def test_clamp_then_one_rounding_is_the_saturating_conversion():
    """the reference of the fp16 stream value on the conversion table: NaN stays NaN, +-inf and everything beyond +-65504 becomes +-65504,
    everything else is torch's round to nearest even"""
    x = C.sat_table()
    assert x.numel() % 4 == 0 and (65536 * 256 * 4) % x.numel() != 0       # tiled, the wrap case does not repeat with the grid's period
    r = C.sat_ref(x)
    assert torch.equal(torch.isnan(r), torch.isnan(x)) and int(torch.isnan(x).sum()) > 2000
    assert not torch.isinf(r).any() and int(torch.isinf(x).sum()) >= 4
    big = x.abs() >= 65504
    assert torch.equal(r[big].float(), torch.sign(x[big]) * 65504)
    inside = x.abs() < 65504
    assert torch.equal(r[inside].view(torch.int16), x[inside].to(torch.float16).view(torch.int16))
    assert int(torch.isinf(x[x.abs() < float("inf")].to(torch.float16)).sum()) > 0     # finite inputs a plain conversion sends to inf
    h = C.all_f16_patterns()
    assert h.numel() == 65536 and h.view(torch.int16).to(torch.int32).unique().numel() == 65536
    assert torch.equal(C.sat_ref(h.float()).view(torch.int16)[torch.isfinite(h)], h.view(torch.int16)[torch.isfinite(h)])   # a round trip is exact
    assert C.SAT_WRAP_N % 4 == 0 and C.SAT_WRAP_N // 4 > 65536 * 256 and C.WIDEN_WRAP_N % 8 == 0 and C.WIDEN_WRAP_N // 8 > 65536 * 256
    assert (65536 * 256 * 8) % 65528 != 0                                  # the period the widening wrap case tiles its patterns with


@pytest.mark.parametrize("mode,d", MODE_D, ids=lambda v: str(v).replace(" ", ""))
def test_an_fp32_layernorm_rounded_once_meets_every_bound(mode, d):
    """The references agree with each other: fp32 torch LayerNorm of the stored value + one rounding vs the fp64 reference, every plain and
    every fused case, and the special rows.  Nothing here is measured against the kernels."""
    dtype, stream = mode
    worst = 0.0
    for c in C.plain_cases(dtype, stream, d):
        stored = C.as_stream(C.stream_input(d, c.rows), stream)
        err, bound = C.ln_error(dtype, C.ln_ref32_rounded(stored, c.form, dtype), C.ln_ref64(stored, c.form))
        assert err < bound, (c, err, bound)
        worst = max(worst, err)
    for c in C.fused_cases(dtype, stream, d):
        stored = C.fused_stored(c)
        assert torch.isfinite(stored.float()).all()
        err, bound = C.ln_error(dtype, C.ln_ref32_rounded(stored, c.form, dtype), C.ln_ref64(stored, c.form))
        assert err < bound, (c, err, bound)
        worst = max(worst, err)
    if stream == "f16":
        stored = C.store(C.combine_sum(*C.special_inputs(d)), "f16")
        for form in C.FORMS:
            ref = C.ln_ref64(stored, form)
            nan_row = C.SPECIALS["nan"][0]
            assert torch.isnan(ref[nan_row]).all() and int(torch.isnan(ref).any(dim=1).sum()) == 1
            err, bound = C.ln_error(dtype, C.ln_ref32_rounded(stored, form, dtype), ref)     # rows holding +-65504 included
            assert err < bound, (form, err, bound)
            worst = max(worst, err)
    print(f"dtype {dtype} stream {stream} d {d}: fp32 torch LayerNorm + one rounding, worst error {worst:.3e} (bound {bound:.3e})")


def test_a_dropped_repeated_or_exchanged_plane_changes_every_fused_stream_value():
    for stream in ("f32", "f16"):
        for d in C.WIDTHS:
            for c in C.fused_cases(2, stream, d, rows_list=C.SMALL_ROWS):
                part, bias, h = C.fused_inputs(c)
                good = C.combine_sum(part, bias, h)
                ref = C.store(good, stream)
                wrong = [part[1:] if c.splits > 1 else part * 0,                          # the loop starts at plane 1
                         torch.cat([part, part[-1:]]),                                    # one plane twice
                         C.planes(c.d, c.rows)[1:c.splits + 1]]                           # planes read one plane further (a wrong stride)
                wrong = [C.combine_sum(w, bias, h) for w in wrong] + ([C.combine_sum(part, None, h)] if bias is not None else [])
                for v in wrong:
                    assert (v != good).float().mean() > 0.9, c                            # the fp32 sum: nearly every element moves ...
                    assert (C.store(v, stream) != ref).float().mean() > 0.25, c           # ... and what reaches a 16-bit stream still does
                if c.splits > 2:
                    # exchanged planes: fp32 addition is not associative, the sum moves in the last bits of some elements
                    perm = torch.cat([part[1:], part[:1]])
                    assert not torch.equal(C.combine_sum(perm, bias, h), C.combine_sum(part, bias, h)), c
                # and the order (partials + bias) + residual, against partials + (bias + residual)
                if bias is not None and stream == "f32" and c.rows >= 4:
                    acc = torch.zeros_like(part[0])
                    for s in range(c.splits):
                        acc = acc + part[s]
                    assert not torch.equal(acc + (bias + h.float()), ref), c


def test_stream_entry_points_validate_arguments_without_a_gpu():
    """Every refusal of include/rapflow.h for the five entry points, at a positive row count AND at none (the launchers behind them answer
    RAP_OK to an empty call before they look at d)."""
    lib = _lib.load()
    mod_args = dict(dtype=2, x=X, f16=1, out=X, TP=4, d=512, mod=X, stride=0, tok=N)

    def ln_mod(**kw):
        a = {**mod_args, **kw}
        return lib.rap_layernorm_mod_h16_stream(a["dtype"], a["x"], a["f16"], a["out"], a["TP"], a["d"], a["mod"], a["stride"], a["tok"], N)

    aff_args = dict(dtype=1, x=X, f16=0, out=X, TP=4, d=768, gain=X, shift=X)

    def ln_aff(**kw):
        a = {**aff_args, **kw}
        return lib.rap_layernorm_affine_h16_stream(a["dtype"], a["x"], a["f16"], a["out"], a["TP"], a["d"], a["gain"], a["shift"], N)

    comb_args = dict(dtype=2, part=X, splits=2, bias=N, h=X, f16=1, out=X, rows=4, d=1024, mod=X, stride=0, tok=N, gain=N, shift=N)

    def comb(**kw):
        a = {**comb_args, **kw}
        return lib.rap_resid_combine_layernorm_h16(a["dtype"], a["part"], a["splits"], a["bias"], a["h"], a["f16"], a["out"], a["rows"], a["d"],
                                                   a["mod"], a["stride"], a["tok"], a["gain"], a["shift"], N)

    for rows in (4, 0):
        for k in ("x", "out", "mod"):
            assert ln_mod(TP=rows, **{k: N}) == -1, k
        for k in ("x", "out", "gain", "shift"):
            assert ln_aff(TP=rows, **{k: N}) == -1, k
        for k in ("part", "h", "out"):
            assert comb(rows=rows, **{k: N}) == -1, k
        for f, rk in ((ln_mod, "TP"), (ln_aff, "TP"), (comb, "rows")):
            for dt in (0, 4, -1):
                assert f(dtype=dt, **{rk: rows}) == -1, dt
            assert f(dtype=3, f16=1, **{rk: rows}) == -1                       # the split mode keeps its stream in fp32
            for v in (2, -1):
                assert f(f16=v, **{rk: rows}) == -1, v
            for d in (0, 128, 384, 500, 1280, 2048, -256):
                assert f(d=d, **{rk: rows}) == -1, d
        for s in (0, 9, -1):
            assert comb(rows=rows, splits=s) == -1, s
        assert comb(rows=rows, mod=N) == -1 and comb(rows=rows, mod=N, gain=X) == -1 and comb(rows=rows, mod=N, shift=X) == -1
    assert ln_mod(TP=-1) == -1 and ln_aff(TP=-4) == -1 and comb(rows=-1) == -1
    # valid arguments and no rows: RAP_OK, and nothing is launched (there is no device here to launch on)
    assert ln_mod(TP=0) == 0 and ln_aff(TP=0) == 0 and comb(rows=0) == 0 and comb(rows=0, mod=N, gain=X, shift=X) == 0
    assert ln_mod(TP=0, dtype=3, f16=0) == 0 and comb(rows=0, dtype=3, f16=0, splits=8) == 0
    sat, wid = lib.rap_convert_f16_sat, lib.rap_convert_f16_to_f32
    assert sat(N, X, 8, N) == -1 and sat(X, N, 8, N) == -1 and wid(N, X, 8, N) == -1 and wid(X, N, 8, N) == -1
    assert sat(X, X, -4, N) == -1 and wid(X, X, -8, N) == -1
    for n in (1, 2, 3, 6, 9):
        assert sat(X, X, n, N) == -1, n
    for n in (1, 4, 7, 12, 20):
        assert wid(X, X, n, N) == -1, n
    assert sat(N, X, 0, N) == -1 and wid(X, N, 0, N) == -1                      # NULL is refused at n = 0 too
    assert sat(X, X, 0, N) == 0 and wid(X, X, 0, N) == 0
