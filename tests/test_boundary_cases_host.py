"""CPU: the inputs of tests/boundary_cases.py are what tests/test_boundary_edges_gpu.py takes them for, every new float64 restatement
agrees with the committed oracle on a small case, and the bounds that are measured rather than derived (the fp32 transform errors) are
re-measured here: the committed oracle in float32 against itself in float64."""
import os

import numpy as np
import torch

import boundary_cases as BC
from oracle import rap_oracle as O


# ---------------------------------------------------------------------------------------------
# collate
# ---------------------------------------------------------------------------------------------
def _wrapper_batches():
    out = {"sizes": BC.collate_sizes_batch(), "primary": BC.collate_primary_batch(), "single_point": BC.collate_single_point_batch()}
    out.update({f"P{P}_B{B}": b for (P, B), b in BC.collate_part_count_batches().items()})
    out.update(BC.collate_dtype_batches())
    return out


def test_every_part_size_is_once_primary_and_once_not():
    b = BC.collate_sizes_batch()
    primary, other = set(), set()
    for row in b["counts"]:
        a = BC.primary_of(row)
        primary.add(int(row[a]))
        other |= {int(n) for p, n in enumerate(row) if p != a and n > 0}
    assert primary >= set(BC.COLLATE_SIZES) and other >= set(BC.COLLATE_SIZES)
    assert b["P"] == 3 and any((row > 0).sum() < 3 for row in b["counts"])                    # trailing padding
    assert int(b["counts"].sum()) % 256 != 0


def test_primary_part_cases_are_what_they_are_named_for():
    b = BC.collate_primary_batch()
    c = b["counts"]
    assert [BC.primary_of(c[i]) for i in range(6)] == [0, 1, 4, 0, 0, 1]
    assert (c[2] > 0).sum() == b["P"] and BC.primary_of(c[2]) == b["P"] - 1                    # the largest part in the LAST column
    assert c[3, 0] == c[3, 1] and c[4, 0] == c[4, 1] == c[4, 2] and c[5, 1] == c[5, 2] > c[5, 0]
    exp = BC.collate_expected(b)
    assert [bool(exp["anchor_parts"][i, p]) for i, p in enumerate([0, 1, 4, 0, 0, 1])] == [True] * 6
    assert exp["anchor_parts"].sum(1).tolist() == [1] * len(c)
    # the extent-defining point: the unique maximum of |p - centroid| over the primary part, the runner-up far behind
    k = int((c[:6] > 0).sum())
    assert sorted(i for _, i, _, _ in b["extent"]) == [0, 63, 64, 255, 256, BC.EXTENT_N - 1]
    assert {s for _, _, _, s in b["extent"]} == {-1.0, 1.0}
    for (sample, idx, axis, sign), j in zip(b["extent"], range(len(b["extent"]))):
        assert BC.primary_of(c[sample]) == 1
        part = b["parts"][k + 2 * j + 1]
        d = part - part.mean(0)
        flat = np.abs(d).reshape(-1)
        order = np.argsort(flat)
        assert order[-1] == 3 * idx + axis and np.sign(d[idx, axis]) == sign
        assert flat[order[-1]] > 3.0 * flat[order[-2]]                                           # ~2 against ~0.5
        assert abs(float(exp["scales"][sample]) - 1.5 * flat[order[-1]]) <= BC.F32_ULP * 3.0


def test_part_count_batches_reach_the_block_edges():
    bs = BC.collate_part_count_batches()
    assert {P for P, _ in bs} == {1, 2, 3, 64, 255, 256} and {B for _, B in bs} == {1, 2, 65}
    assert any(int(b["counts"].sum()) % 256 for b in bs.values())
    for (P, B), b in bs.items():
        assert b["counts"].shape == (B, P) and B * P <= 65535
        if P > 1:
            assert any((row > 0).sum() < P for row in b["counts"]) or B == 1
        if P >= 64:
            assert (b["counts"][0] > 0).all()                                                    # thread P-1 of the frame kernel has a real part
    assert any((b["counts"][-1] > 0).sum() < P for (P, B), b in bs.items() if P == 256)


def test_collate_oracle_is_stable_to_the_summation_order():
    """both sides of the GPU comparison round one float64 value to fp32; they differ in float64 summation order only.  The oracle with
    every part's points in reverse order (same outputs, other order of every sum) moves by no more than the bound itself."""
    for name, b in _wrapper_batches().items():
        a, f = BC.collate_expected(b), BC.collate_expected(b, flip=True)
        for k in BC.COLLATE_EXACT_KEYS:
            assert np.array_equal(a[k], f[k]), (name, k)
        for k in BC.COLLATE_FLOAT_KEYS:
            fin = np.isfinite(a[k])
            assert np.array_equal(fin, np.isfinite(f[k])), (name, k)
            d = np.abs(a[k].astype(np.float64) - f[k].astype(np.float64))[fin]
            assert (d <= BC.collate_tolerance(a[k])[fin]).all(), (name, k, d.max())


def test_empty_part_expectation_keeps_columns_and_zero_rows():
    b = BC.collate_empty_parts_batch()
    c, e = b["counts"], BC.collate_expected(b)
    assert c[0, 0] == 0 and c[0, 1] == 0 and c[0, 3] == 0 and c[2].sum() == 0 and c[1].sum() > 0 and c[3].sum() > 0
    empty = c == 0
    assert not e["rotations"][empty].any() and not e["translations"][empty].any() and not e["anchor_parts"][empty].any()
    assert (e["rotations"][~empty] == np.eye(3, dtype=np.float32)).all()
    assert e["cu_seqlens"][2] == e["cu_seqlens"][3] and e["scales"][2] == 0 and not e["global_translation"][2].any()
    cu = e["cu_seqlens"]
    for s in range(len(c)):
        assert set(e["part_indices"][cu[s]:cu[s + 1]].tolist()) == {p for p in range(c.shape[1]) if c[s, p] > 0}
    assert [int(np.argmax(r)) for r in e["anchor_parts"][[0, 1, 3, 4]]] == [4, 1, 4, 0]
    # the neighbours of the empty sample are what they are alone
    for s in (1, 3):
        k0, k1 = int((c[:s] > 0).sum()), int((c[:s + 1] > 0).sum())
        alone = dict(b, counts=c[s:s + 1], parts=b["parts"][k0:k1], feats=b["feats"][k0:k1], perms=b["perms"][k0:k1])
        ea = BC.collate_expected(alone)
        assert np.array_equal(ea["pointclouds"], e["pointclouds"][cu[s]:cu[s + 1]]) and np.array_equal(ea["translations"][0], e["translations"][s])


def test_single_point_primary_divides_by_zero_in_the_oracle_only_there():
    b = BC.collate_single_point_batch()
    e = BC.collate_expected(b)
    cu = e["cu_seqlens"]
    assert e["scales"][1] == 0 and not np.isfinite(e["pointclouds_gt"][cu[1]:cu[2]]).any() and not np.isfinite(e["translations"][1]).any()
    assert np.isfinite(e["global_translation"]).all() and np.isfinite(e["rotations"]).all()
    for s in (0, 2):
        assert np.isfinite(e["pointclouds"][cu[s]:cu[s + 1]]).all() and np.isfinite(e["translations"][s]).all() and e["scales"][s] > 0


def test_dtype_batches_are_far_out_and_mixed():
    d = BC.collate_dtype_batches()
    assert all(x.dtype == np.float64 for x in d["f64_far"]["parts"]) and min(np.abs(x.mean(0)).max() for x in d["f64_far"]["parts"]) > 5e4
    assert all(x.dtype == np.float32 for x in d["f32"]["parts"]) and min(np.abs(x.mean(0)).max() for x in d["f32"]["parts"]) > 1.5e2
    kinds = [x.dtype for x in d["mixed"]["parts"]]
    assert kinds.count(np.dtype(np.float64)) == 1 and kinds.count(np.dtype(np.float32)) == len(kinds) - 1
    x = d["mixed"]["parts"][3]
    assert not np.array_equal(x, x.astype(np.float32).astype(np.float64))                       # casting the batch down would show


def test_orders_and_feature_widths_are_all_covered():
    bs = dict(_wrapper_batches(), empty=BC.collate_empty_parts_batch())
    assert {b["order"] for b in bs.values()} == {"none", "identity", "reverse", "random", "numpy"}
    assert {b["F"] for b in bs.values()} == {0, 1, 3, 32}
    b = BC.collate_primary_batch()
    np.random.seed(b["np_seed"])
    drawn = [np.random.permutation(int(n)) for n in b["counts"].reshape(-1) if n > 0]
    assert all(np.array_equal(x, y) for x, y in zip(drawn, b["perms"]))
    for b in bs.values():
        if b["perms"] is not None:
            assert all(np.array_equal(np.sort(o), np.arange(len(x))) for o, x in zip(b["perms"], b["parts"]))


# ---------------------------------------------------------------------------------------------
# output transforms
# ---------------------------------------------------------------------------------------------
def test_relative_cases_put_an_empty_part_on_one_side_of_lane_64():
    seen = set()
    for B, P in BC.REL_SHAPES:
        c = BC.relative_case(B, P)
        flat = c["ppp"].reshape(-1)
        assert int((flat > 0).sum()) > 0
        if B * P > 64:
            assert (int(flat[63]) == 0) != (int(flat[64]) == 0)
            seen.add(int(flat[63]) == 0)
        assert float(c["scales"][0]) == np.float32(0.02) and (B == 1 or float(c["scales"][-1]) == 80.0)
        Gg = c["G_general"].double()
        sv = torch.linalg.svdvals(Gg)
        assert (sv[:, 0] - 2.0).abs().max() < 1e-5 and (sv[:, 2] - 0.5).abs().max() < 1e-5 and (c["g_general"].norm(dim=1) - 300).abs().max() < 1e-3
        assert (c["G_rigid"].double() @ c["G_rigid"].double().transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs().max() < 1e-6
    assert seen == {True, False}
    assert BC.relative_case(1, 64)["ppp"][0, 63] == 0


def test_float64_relative_transforms_agree_with_the_committed_oracle():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transform_files.npz"))
    T = lambda k: torch.from_numpy(z[k])
    args = (T("R_pred"), T("t_pred"), T("in_rotations"), T("in_translations"), T("in_scales"), T("in_points_per_part"))
    for gr, gt in ((None, None), (T("global_rotation"), T("global_translation"))):
        ref, bound = BC.relative_transforms_f64(*args, gr, gt)
        old = O.relative_transforms(*args, gr, gt).double().numpy()
        assert np.abs(ref - old).max() < 1e-5 * max(1.0, np.abs(ref).max())
        assert (bound[ref != 0] > 0).all()
    # ... and on a case of this file's, in the frame the reference is conditioned for (a rotation)
    c = BC.relative_case(5, 13)
    args = (c["R_pred"], c["t_pred"], c["R_gt"], c["t_gt"], c["scales"], c["ppp"], c["G_rigid"], c["g_rigid"])
    ref, _ = BC.relative_transforms_f64(*args)
    assert np.abs(ref - O.relative_transforms(*args).double().numpy()).max() < 1e-5 * max(1.0, np.abs(ref).max())
    assert not ref[(c["ppp"] == 0).numpy()].any()


# ---------------------------------------------------------------------------------------------
# transform errors
# ---------------------------------------------------------------------------------------------
def test_transform_error_cases_reach_their_edges():
    roles, kinds_of_bad = set(), set()
    for B, P, m, _ in BC.transform_error_cases():
        c = BC.transform_error_case(B, P, m)
        roles |= set(c["roles"])
        valid = (c["ppp"] != 0) & ~c["anchor"]
        if P == 130:                                            # every angle class on both sides of column 64, on parts that count
            for half in (slice(0, 64), slice(64, 130)):
                assert {int(x) for x in c["cls"][:, half][valid[:, half]].tolist()} >= set(range(len(BC.TE_ANGLES))) or m == "out_of_range"
        if P > 64:
            assert {(int(r[63]) == 0, int(r[64]) == 0) for r in c["ppp"] if int((r != 0).sum()) > 1} <= {(True, False), (False, True), (False, False)}
            assert any(int(r[63]) == 0 for r in c["ppp"]) or any(int(r[64]) == 0 for r in c["ppp"])
        for b, role in enumerate(c["roles"]):
            n_anchor = int(c["anchor"][b].sum())
            assert n_anchor == {"no_anchor": 0, "two_anchors": 2 if P > 2 else 1}.get(role, 1)
            if role == "anchor_only":
                assert int(valid[b].sum()) == 0
            if role == "anchor_on_empty":
                assert int(c["ppp"][b][c["anchor"][b]].sum()) == 0
        if m == "out_of_range":
            ids, cl = c["matched"], c["clamped"]
            assert torch.equal(cl, ids.clamp(0, P - 1)) and bool(((ids < 0) | (ids >= P)).any())
            kinds_of_bad |= {int(x) if int(x) in (-1, 2 ** 40) else "P" for x in ids[(ids < 0) | (ids >= P)].tolist()}
            if P > 2:
                assert bool((cl != torch.arange(P)[None, :]).any())                              # some part is redirected, not merely clamped onto itself
            # the expectation IS the oracle on the clamped ids: the oracle rejects the raw ones
            r = BC.transform_errors_oracle(c, torch.float64, True)
            bi = torch.arange(B)[:, None]
            again = O.compute_transform_errors(c["R_gt"].double(), c["t_gt"].double(), c["R_pred"].double()[bi, cl], c["t_pred"].double()[bi, cl],
                                               c["ppp"], c["anchor"], None, c["scale"].double())
            assert all(torch.equal(torch.nan_to_num(x, nan=-1.0), torch.nan_to_num(y, nan=-1.0)) for x, y in zip(r, again))
        if m == "permuted" and P > 2:
            assert bool((c["matched"] != torch.arange(P)[None, :]).any())
    assert roles == set(BC.TE_ROLES) and kinds_of_bad == {-1, "P", 2 ** 40}
    c = BC.transform_error_case(3, 130, "identity")
    assert c["cls"].min() == 0 and torch.equal(c["R_pred"][c["cls"] == 0], c["R_gt"][c["cls"] == 0])      # angle 0 exactly


def test_float64_direct_restatement_agrees_with_the_committed_oracle_without_an_anchor():
    """without an anchor the frame of compute_transform_errors is the identity, and the function is the direct variant"""
    for m in ("none", "permuted"):
        c = dict(BC.transform_error_case(3, 65, m))
        c["anchor"] = torch.zeros_like(c["anchor"])
        a = BC.transform_errors_oracle(c, torch.float64, True)
        d = BC.transform_errors_direct_f64(c, True)
        for x, y in zip(a, d):
            assert torch.equal(torch.isnan(x), torch.isnan(y))
            assert float((torch.nan_to_num(x) - torch.nan_to_num(y)).abs().max()) < 1e-9


def measure_transform_error_deviation():
    """-> (rot per class (8,), trans, rot mean, trans mean): max |float32 oracle - float64 oracle| over every case"""
    rot = np.zeros(len(BC.TE_ANGLES))
    trans = rot_mean = trans_mean = 0.0
    for B, P, m, with_scale in BC.transform_error_cases():
        c = BC.transform_error_case(B, P, m)
        r64 = BC.transform_errors_oracle(c, torch.float64, with_scale)
        r32 = BC.transform_errors_oracle(c, torch.float32, with_scale)
        assert all(torch.equal(torch.isnan(x), torch.isnan(y)) for x, y in zip(r64, r32))
        cls = BC.angle_class_of(c["cls"], r64[2])
        d = (r32[2].double() - r64[2]).abs()
        valid = (c["ppp"] != 0) & ~c["anchor"]
        for k in range(len(BC.TE_ANGLES)):
            sel = valid & (cls == k)
            if bool(sel.any()):
                rot[k] = max(rot[k], float(d[sel].max()))
        trans = max(trans, float((r32[3].double() - r64[3]).abs().max()))
        ok = ~torch.isnan(r64[0])
        if bool(ok.any()):
            rot_mean = max(rot_mean, float((r32[0].double() - r64[0])[ok].abs().max()))
            trans_mean = max(trans_mean, float((r32[1].double() - r64[1])[ok].abs().max()))
    return rot, trans, rot_mean, trans_mean


def test_transform_error_bounds_are_the_measured_ones():
    rot, trans, rot_mean, trans_mean = measure_transform_error_deviation()
    print("float32 oracle vs float64 oracle: rot per class", " ".join(f"{x:.3e}" for x in rot), f"trans {trans:.3e} rot mean {rot_mean:.3e} "
          f"trans mean {trans_mean:.3e}")
    assert BC.TE_MARGIN == 4.0
    for k in range(len(BC.TE_ANGLES)):
        assert BC.TE_ROT_BOUND[k] >= 4.0 * rot[k], (BC.TE_ANGLES[k], rot[k])
        assert BC.TE_ROT_BOUND[k] <= 4.0 * 1.5 * rot[k] + 1e-30, (BC.TE_ANGLES[k], rot[k])      # ... and are not padded either
    for const, got in ((BC.TE_TRANS_BOUND, trans), (BC.TE_ROT_MEAN_BOUND, rot_mean), (BC.TE_TRANS_MEAN_BOUND, trans_mean)):
        assert 4.0 * got <= const <= 4.0 * 1.5 * got, (const, got)
    # d(theta) = d(cos) / sin(theta): the well-conditioned classes are orders of magnitude tighter than the ends
    assert max(rot[3], rot[4]) < 0.05 * min(rot[0], rot[7])


# ---------------------------------------------------------------------------------------------
# generation selection
# ---------------------------------------------------------------------------------------------
def test_selection_specials_sit_on_both_sides_of_sample_64():
    for G in BC.SEL_G:
        v = BC.selection_values(G, 200)
        for side in (BC.SEL_LEFT, BC.SEL_RIGHT):
            assert bool((v[:, side["tie"]] == v[0, side["tie"]]).all())
            assert bool(torch.isinf(v[:, side["inf"]]).any()) and float(v[:, side["inf"]].max()) == float("inf")
            assert float(v[:, side["neg_inf"]].min()) == float("-inf")
            assert int(torch.isnan(v[:, side["nan"]]).sum()) == (2 if G > 1 else 1)
        assert max(BC.SEL_LEFT.values()) == 63 and min(BC.SEL_RIGHT.values()) == 64
        assert bool(torch.isnan(BC.selection_values(G, 65)[:, 60]).any()) and bool((BC.selection_values(G, 65)[:, 64] == 2.0).all())
    for G in BC.SEL_G:
        for B in BC.SEL_B:
            v = BC.selection_values(G, B)
            assert v.shape == (G, B)
            assert torch.equal(torch.argmin(v, dim=0), BC.first_extremum(v, False)), (G, B)      # torch's rule is the documented rule
            assert torch.equal(torch.argmax(v, dim=0), BC.first_extremum(v, True)), (G, B)
    v = BC.selection_values(17, 200)
    assert int(torch.argmin(v, dim=0)[67]) == 8 and int(torch.argmin(v, dim=0)[66]) == 8 and int(torch.argmax(v, dim=0)[66]) != 16


def test_gather_cases_cross_the_strides():
    assert any(3 * n < 256 for n in BC.GATHER_COUNTS if n) and 3 * 85 < 256 <= 3 * 86 and 3 * 1365 < 16 * 256 <= 3 * 1366 and 0 in BC.GATHER_COUNTS
    assert 28 * 9 < 256 <= 29 * 9 and 85 * 3 < 256 <= 86 * 3
    for P in BC.GATHER_P:
        c = BC.gather_case(P)
        for k in ("clouds", "R", "t"):
            assert c[k].unique().numel() == c[k].numel()                                        # a wrong source index is a wrong value
        assert len(set(torch.argmin(c["rmse"], dim=0).tolist())) > 1


# ---------------------------------------------------------------------------------------------
# batch tables
# ---------------------------------------------------------------------------------------------
def test_token_tables_hold_the_named_lengths_and_empty_runs():
    t = BC.token_tables()
    lens = (t["many"][1:] - t["many"][:-1]).tolist()
    assert len(lens) == 1000 and int(t["many"][0]) == 7
    assert lens[0] == lens[1] == 0 and lens[500:503] == [0, 0, 0] and lens[998:] == [0, 0] and lens[2] > 0 and lens[997] >= 0
    assert set(BC.TOKEN_LENGTHS) <= set(lens)
    assert [int(v[-1] - v[0]) for k, v in t.items() if k != "many"] == [40000, 1, 16385]


def test_check_batch_bit_table_and_which_bits_can_stand_alone():
    want = {"consistent": 0, "sum": 1 | 8, "ends": 1 | 2, "first_entry": 2 | 8, "ends_alone": 2, "decreasing": 4 | 8, "span_alone": 8, "negative_alone": 16,
            "negative_and_sum": 1 | 8 | 16, "everything": 31}
    cases = BC.check_batch_cases()
    assert set(cases) == set(want)
    for name, (ppp, cu, TP, bit) in cases.items():
        f = BC.check_batch_bits(ppp, cu, TP)
        assert f == want[name] and (f & bit) == bit, (name, f)
    seen = {BC.check_batch_bits(*t) for t in BC.small_check_tables()}
    assert {0, 2, 8, 16} <= seen and not ({1, 4} & seen)                     # bits 0 and 2 never come alone
    assert all(any(f & bit for f in seen) for bit in (1, 2, 4, 8, 16))
