"""CPU: the whole-call dispatch sweep (tests/plan_cases.py) reaches what it is listed for, computed from the library's own plan query
(rap_call_plan: the function the launch path runs by, as host arithmetic) and from its restatement in Python: the two agree on every
case and on a dense grid, each pair differs in exactly the fields it is listed for, the union of the cases reaches every plan the grid
shows for d = 512 up to 32 768 rows, the plan follows the tuning keys, and the inputs of the work-list cases are well conditioned."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import plan_cases as PC
from conftest import ROOT
from oracle import rap_oracle as O
from rap_amd import _lib
from rap_amd import synthetic as S


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _diff(a, b):
    return {f for f, x, y in zip(PC.FIELDS, a, b) if x != y}


def test_plan_query_equals_the_restated_plan_on_every_case(lib):
    for pair, side, m, mode in PC.cases():
        assert PC.lib_plan(lib, mode, m.TP, m.B, m.nseg) == PC.plan(mode, m.TP, m.B, m.nseg), (m.name, mode)
        # ... and a launch that cannot use the bounded softmax never splits the fp32 attention
        p = PC.lib_plan(lib, mode, m.TP, m.B, m.nseg, bounded=False)
        assert p == PC.plan(mode, m.TP, m.B, m.nseg, bounded=False)
        if p.dtype == 0:
            assert (p.ranges_part, p.ranges_batch, p.percu_part, p.percu_batch) == (1, 1, 0, 0)


def _grid_points():
    for TQ in range(256, 70000, 256):
        for nseg in range(1, 49):
            yield TQ, nseg


def test_plan_query_equals_the_restated_plan_on_a_dense_grid(lib):
    """TQ 256 .. 70 000 in steps of 256 x nseg_part 1 .. 48 x the four modes x the four widths, TP = TQ (and, on a thinner set, the
    ragged TP = TQ - 255 and other batch sizes / layer counts / latent widths: the workspace arithmetic)."""
    out = (ctypes.c_int64 * len(PC.FIELDS))()
    po = ctypes.cast(out, ctypes.c_void_p)
    n = 0
    for d, H in PC.WIDTHS:
        for mode in PC.MODES:
            cdt, rdt = (PC.DT[x] for x in PC.MODES[mode])
            for TQ, nseg in _grid_points():
                B = 1 + (nseg * 7 + TQ // 256) % 16
                assert lib.rap_call_plan(cdt, rdt, d, H, 2, 0, TQ, B, nseg, 2, 1, po, len(PC.FIELDS)) == 0
                assert tuple(out) == tuple(PC.plan(mode, TQ, B, nseg, d=d, heads=H)), (d, mode, TQ, nseg, B)
                n += 1
    assert n == 4 * 4 * 273 * 48
    for d, H in PC.WIDTHS:
        for mode in PC.MODES:
            for TQ in list(range(256, 12000, 256)) + [21760, 22016, 32768, 65536]:
                for L, rows, in_dim, B, nseg in ((1, 1, 0, 1, 1), (12, 20, 0, 32, 64), (3, 7, 64, 5, 40), (2, 3, 512, 16, 16)):
                    kw = dict(d=d, heads=H, L=L, rows=rows, in_dim=in_dim)
                    assert PC.lib_plan(lib, mode, TQ - 255, B, nseg, **kw) == PC.plan(mode, TQ - 255, B, nseg, **kw), (d, mode, TQ, L, rows, in_dim)


def test_each_pair_differs_in_exactly_the_fields_it_is_listed_for(lib):
    for pair in PC.PAIRS:
        lo, hi = pair.low, pair.high
        if pair.kind == "rows":
            assert hi.TP == lo.TP + 1 and lo.TP % 256 == 0 and (lo.B, lo.P) == (hi.B, hi.P), pair.name      # no filler | 255 filler rows
        else:
            assert lo.TP // 256 == hi.TP // 256 == 4 and hi.nseg + hi.B > lo.nseg + lo.B, pair.name
        for mode in PC.MODES:
            a, b = (PC.lib_plan(lib, mode, m.TP, m.B, m.nseg) for m in (lo, hi))
            diff = _diff(a, b)
            if pair.kind == "rows":
                # listed for exactly the modes whose plan changes there (above 4 097 tokens one 16-bit variant stands for both)
                listed = pair.modes.get(mode)
                if listed is None and PC.FAMILY[mode] == "h16" and lo.TP > 4097:
                    listed = next((v for k, v in pair.modes.items() if PC.FAMILY[k] == "h16"), None)
                assert diff == (listed or set()) | PC.ALWAYS, (pair.name, mode, sorted(diff))
                if lo.TP <= 4097:
                    assert (mode in pair.modes) == bool(diff - PC.ALWAYS), (pair.name, mode)
            elif mode in pair.modes:
                assert pair.modes[mode] <= diff <= pair.modes[mode] | PC.WL_ALWAYS, (pair.name, mode, sorted(diff))
                assert a.TQ == 1280 and a.dtype == PC.DT[PC.MODES[mode][0]]          # above tuning key 17's default: split precision runs
        if pair.kind == "worklist":
            # the branch the pair does not move stays at 4 key ranges on both sides (the mixed state) -- except where the issue's own
            # geometry rules it out: one-part samples have nseg_part = B, so both branches move; the two-part variant next to it keeps the
            # part branch at 2 plain ranges while the per-sample branch moves
            for mode, listed in pair.modes.items():
                a, b = (PC.lib_plan(lib, mode, m.TP, m.B, m.nseg) for m in (lo, hi))
                if pair.name == "batch-15-16-one-part":
                    assert PC.branch_states(a) == ((4, 0), (4, 0)) and PC.branch_states(b) == ((2, 1), (2, 1))
                elif pair.name == "batch-15-16":
                    assert PC.branch_states(a) == ((2, 0), (4, 0)) and PC.branch_states(b) == ((2, 0), (2, 1))
                else:
                    assert a.ranges_batch == b.ranges_batch == 4 and not {"ranges_batch", "percu_batch"} & listed, (pair.name, mode)


def test_geometries_are_what_the_sweep_asks_for():
    for m in PC.members():
        inp = PC.inputs(m)
        ppp = inp["points_per_part"]
        assert tuple(ppp.shape) == (m.B, m.P) and int(ppp.sum()) == m.TP == inp["pointclouds"].shape[0] and m.nseg == m.B * m.P
        assert int(ppp[ppp > 0].min()) >= PC.MIN_PART                                  # no near-degenerate Procrustes fit
        assert all(len(p) in (2, 3) for p in m.parts) or not m.name.startswith("rows")
        if m.name.startswith("rows"):
            assert max(sum(p) for p in m.parts) <= 4200                                # the fp64 attention stays cheap
        if not m.name.startswith("batch-15-16-one-part"):
            assert bool((ppp[:, -1] == 0).any()) and bool((ppp[:, -1] > 0).any()) or m.B == 1 and int(ppp[0, -1]) == 0, m.name      # an empty trailing part
        lens = [n for p in m.parts for n in p]
        assert len(set(lens)) > 1 or len(lens) == 1                                    # ragged


def test_the_cases_reach_every_plan_of_the_grid_up_to_32768_rows(lib):
    """Per family (fp32, split precision, 16-bit): every row signature (arithmetic, attention item geometry, fusion, planes, the eight forms) the
    d = 512 grid shows up to 32 768 rows is the signature of some case, and so is every (key ranges, one block per CU) state of either
    attention branch."""
    want_rows, want_branch = set(), set()
    for mode in PC.MODES:
        fam = PC.FAMILY[mode]
        for TQ in range(256, 32768 + 1, 256):
            for nseg in range(1, 49):
                for B in (1, min(nseg, 16)):
                    p = PC.plan(mode, TQ, B, nseg)
                    if mode == "x2" and p.dtype == 0:
                        continue                                                       # (a small split-precision call IS an fp32 call: counted there)
                    want_rows.add((fam, PC.row_signature(p)))
                    for br, st in zip(("part", "batch"), PC.branch_states(p)):
                        want_branch.add((fam, br, st))
    have_rows, have_branch = set(), set()
    for pair, side, m, mode in PC.cases():
        p = PC.lib_plan(lib, mode, m.TP, m.B, m.nseg)
        fam = "f32" if p.dtype == 0 else PC.FAMILY[mode]
        have_rows.add((fam, PC.row_signature(p)))
        for br, st in zip(("part", "batch"), PC.branch_states(p)):
            have_branch.add((fam, br, st))
    assert want_rows <= have_rows, sorted(want_rows - have_rows)
    assert want_branch <= have_branch, sorted(want_branch - have_branch)
    # the two 16-bit variants share every row signature (they differ in the residual epilogue, not in a form): one stands for both
    for TQ in range(256, 32768 + 1, 256):
        assert PC.row_signature(PC.plan("bf16h", TQ, 2, 6)) == PC.row_signature(PC.plan("f16", TQ, 2, 6))


def test_plan_follows_the_tuning_keys_and_the_defaults_come_back(lib):
    probe = [(mode, TP, B, nseg) for mode in PC.MODES for TP, B, nseg in ((768, 2, 6), (769, 2, 6), (1100, 1, 7), (1100, 4, 20), (2048, 2, 6), (2049, 2, 6), (4096, 2, 6),
                                                                         (4097, 2, 6), (7937, 3, 9))]
    before = [PC.lib_plan(lib, *q) for q in probe]
    changed = {}
    for pairs in ([(5, 0)], [(6, 0)], [(17, 0)], [(17, 4096)], [(19, 0)], [(20, 0)], [(20, 2)], [(20, 64)], [(20, 130)], [(6, 0), (19, 0)], [(18, 0)]):
        with PC.tuned(lib, pairs) as keys:
            got = [PC.lib_plan(lib, *q) for q in probe]
            assert got == [PC.plan(*q, keys=keys) for q in probe], pairs
            changed[tuple(pairs)] = set().union(*(_diff(a, b) for a, b in zip(before, got)))
    assert {"ranges_part", "percu_part"} <= changed[((5, 0),)]
    assert {"fused", "f_out", "f_ff2", "f_head0"} <= changed[((6, 0),)] and "planes" not in changed[((6, 0),)] and "ws_bytes" not in changed[((6, 0),)]
    assert "dtype" in changed[((17, 0),)] and "dtype" in changed[((17, 4096),)]
    assert "fused" in changed[((19, 0),)] and "planes" not in changed[((19, 0),)]
    assert {"attn_bq", "attn_kg", "items_part"} <= changed[((20, 0),)] and "attn_kg" in changed[((20, 2),)]
    assert "ws_bytes" not in set().union(*changed.values())                           # the size never depends on a key
    assert [PC.lib_plan(lib, *q) for q in probe] == before


def test_workspace_bytes_of_a_split_precision_model_cover_both_layouts(lib):
    for TP, B, nseg in ((769, 2, 6), (768, 2, 6), (2049, 2, 6), (4097, 2, 6), (1100, 4, 20)):
        both = [PC.plan("x2", TP, B, nseg, force_dtype=fd).ws_bytes for fd in (0, 3)]
        assert PC.lib_plan(lib, "x2", TP, B, nseg).ws_bytes == max(both)
        with PC.tuned(lib, [(17, 0)]):
            assert PC.lib_plan(lib, "x2", TP, B, nseg).ws_bytes == max(both)
        # the fp32 layout is the fp32 model's own
        assert both[0] == PC.lib_plan(lib, "f32", TP, B, nseg).ws_bytes
    assert PC.plan("x2", 769, 2, 6, force_dtype=3).ws_bytes > PC.plan("x2", 769, 2, 6, force_dtype=0).ws_bytes      # (the split-K planes)
    assert PC.plan("x2", 4097, 2, 6, force_dtype=3).ws_bytes == PC.plan("x2", 4097, 2, 6, force_dtype=0).ws_bytes   # (none: the same bytes)


def test_bad_arguments_are_refused_before_anything_else_happens(lib):
    out = (ctypes.c_int64 * 21)(*([-7] * 21))
    po = ctypes.cast(out, ctypes.c_void_p)
    good = [1, 2, 512, 8, 2, 0, 1100, 2, 6, 2, 1]
    for i, v in ((0, 4), (0, -1), (1, 1), (2, 0), (2, 128), (2, 1280), (3, 4), (4, 0), (4, 65), (5, 2), (5, 516), (6, 0), (6, -1), (7, 0), (8, -1), (9, 0)):
        a = list(good); a[i] = v
        assert lib.rap_call_plan(*a, po, 21) == -1 and list(out) == [-7] * 21, (i, v)
    assert lib.rap_call_plan(*good, None, 21) == -1 and lib.rap_call_plan(*good, po, 20) == -1 and list(out) == [-7] * 21
    assert lib.rap_call_plan(*good, po, 21) == 0 and list(out) != [-7] * 21


def test_bounds_are_the_numbers_of_the_tests_they_come_from():
    import test_fullconfig_gpu as TF
    assert (TF.TOL_CLOUD, TF.TOL_R, TF.TOL_T) == (PC.FP32_TOL_CLOUD, PC.FP32_TOL_R, PC.FP32_TOL_T)
    src = inspect.getsource(TF._assert_fp32)
    assert 'e["per_sample_final_cloud_max"] < 5e-5 and e["R_frob"] < 1e-4' in src and (PC.FP32_SAMPLE_CLOUD, PC.FP32_SHARP_R) == (5e-5, 1e-4)
    # PC.assert_fp32 at inside = 1 IS TF._assert_fp32: both pass just inside every bound and both fail just outside each one
    ok = {"worst_step_cloud": 5e-4, "worst_step_x_t": 5e-4, "final_cloud": 5e-4, "R_frob": 9.99e-5, "t": 1e-3, "per_sample_final_cloud_max": 4.99e-5}
    TF._assert_fp32(ok); PC.assert_fp32(ok)
    for k, v in (("worst_step_cloud", 5.01e-4), ("worst_step_x_t", 5.01e-4), ("final_cloud", 5.01e-4), ("R_frob", 1e-4), ("t", 1.01e-3),
                 ("per_sample_final_cloud_max", 5e-5)):
        for f in (TF._assert_fp32, PC.assert_fp32):
            with pytest.raises(AssertionError):
                f({**ok, k: v})
    tests = os.path.join(ROOT, "tests")
    h16 = open(os.path.join(tests, "test_h16_gpu.py")).read()
    assert 'bound = {"bfloat16": 2e-2, "float16": 3e-3}[cdt]' in h16 and PC.H16_SAMPLE_BOUND == {"bfloat16": 2e-2, "float16": 3e-3}
    assert re.search(r'^FWD_REL_BOUND = \{"bfloat16": 8e-3, "float16": 1e-3\}$', h16, flags=re.M) and PC.FWD_REL_BOUND == {"bfloat16": 8e-3, "float16": 1e-3}
    small = open(os.path.join(tests, "test_small_call_gpu.py")).read()
    assert 'assert err < (5e-5 if cdt == "float32x2" else 2e-2)' in small and PC.H16_STEP_BOUND == 2e-2
    assert 'assert float((outs[tag][k] - v).abs().max()) < 5e-6, (tag, k)' in small and PC.BITID_X2_TOL == 5e-6
    widths = open(os.path.join(tests, "test_widths_gpu.py")).read()
    assert "assert ev <= 1e-4 * v_ref.abs().max().item(), ev" in widths and "assert ev < 2e-5 and ef < 2e-4, (ev, ef)" in widths
    assert (PC.FWD_FP32_V_REL, PC.FWD_FP32_V_ABS, PC.FWD_FP32_F_ABS) == (1e-4, 2e-5, 2e-4)
    assert 'bound = FWD_REL_BOUND[cdt] * (2.0 if (cdt, rdt) == ("float16", "float16") else 1.0)' in widths and "assert frel < 4 * bound, frel" in widths


_WL_MEMBERS = [m for p in PC.WORKLIST_PAIRS for m in (p.low, p.high)]


@pytest.mark.parametrize("m", _WL_MEMBERS, ids=[m.name for m in _WL_MEMBERS])
def test_worklist_inputs_are_well_conditioned(m):
    """the float32 oracle sits at least 4 x inside the fp32 bounds of the float64 oracle on every ~1 100-token geometry: the bounds the GPU
    test holds the fp32 and split-precision kernels to are not a matter of luck with these inputs, and no Procrustes fit of a small part is
    near-degenerate"""
    from test_fullconfig_gpu import _errors
    cfg = dict(S.RAP_12); cfg["num_layers"] = PC.LAYERS
    sd = S.make_weights(cfg, 0)
    inp = PC.inputs(m)
    r32 = O.sample(sd, cfg, inp, PC.STEPS, True)
    r64 = O.sample(sd, cfg, inp, PC.STEPS, True, dtype=torch.float64)
    keys = ("end_point_trajectory", "trajectory", "R", "t")
    e = _errors({k: r32[k].double() for k in keys}, {k: r64[k] for k in keys}, inp["cu_seqlens"], inp["points_per_part"])
    print(m.name, {k: e[k] for k in ("worst_step_cloud", "worst_step_x_t", "R_frob", "t", "per_sample_final_cloud_max")})
    PC.assert_fp32(e, inside=PC.YARDSTICK_MARGIN)
