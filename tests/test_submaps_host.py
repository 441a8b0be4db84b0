"""CPU: the yardstick of the submap stage (tests/submap_oracle.py) against the reference's recorded outputs (tests/golden/submaps.npz) and
against scipy; the argument checks and workspace arithmetic of rap_deskew, rap_fuse_frames, rap_submap_overlap and
rap_submap_groups_connected; and what the GPU test (tests/test_submaps_gpu.py) relies on, measured from the yardstick and not from the
code under test: the margin rule of every overlap input, and the deskew bound.

THE DESKEW BOUND.  The oracle's formula run in numpy float32 against float64 on the GPU test's inputs (submap_oracle.deskew_case
and deskew_short_case, every ts_mid of TS_MIDS) deviates by at most 4.66e-7 of max(1, |p|_inf + |T|_inf) per point (measured here, printed by
test_deskew_bound_is_the_measured_fp32_deviation; submap_oracle.DESKEW_F32_DEVIATION is that figure, held to the measurement's three
digits).  The GPU test allows 4 times that constant: the kernel contracts to fma and its sincosf differs from numpy's by a few ulp,
which moves single roundings, not the order of magnitude; a wrong branch (the series taken for a large angle, the 1e-8 rule missed, the
wrong sign of s) is off by 1e-3 or more."""
import ctypes
import os

import numpy as np
import pytest
import torch

import submap_oracle as O
from conftest import ROOT
from rap_amd import _lib

N, ONE = ctypes.c_void_p(0), ctypes.c_void_p(256)      # NULL; a non-NULL sentinel -- every call below fails before a pointer is used
up = lambda n: -(-n // 256) * 256


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "submaps.npz"))


# ---- the oracle against the reference's outputs ----------------------------------------------------------------------------------------
def test_oracle_reproduces_the_reference_fixture(golden):
    g = golden
    pts, nrm, poses = [p.astype(np.float64) for p in g["points"]], [v.astype(np.float64) for v in g["normals"]], list(g["poses"])
    vs = float(g["voxel_size"])
    subs = []
    for k, (a, b) in enumerate(g["boundaries"]):
        fp, fn = O.create_submap_from_frames(pts, poses, int(a), int(b - a + 1), nrm)
        scale = np.abs(g[f"fused_points_{k}"]).max()
        assert np.abs(fp - g[f"fused_points_{k}"]).max() <= 4 * np.finfo(np.float64).eps * scale           # double rounding
        assert np.abs(fn - g[f"fused_normals_{k}"]).max() <= 4 * np.finfo(np.float64).eps
        zero = ~g[f"fused_normals_{k}"].any(axis=1)
        assert zero.sum() >= 1 and not fn[zero].any()                                                      # the zero normals stay zero
        subs.append(fp)
        assert O.voxel_margin(fp, vs) >= 1e-6
    ratios = [O.overlap_ratio(subs[i], subs[j], vs) for i, j in g["pairs"]]
    assert ratios == list(g["pair_ratio"])                                                                # exactly
    assert O.overlap_ratio(np.zeros((0, 3)), subs[0], vs) == float(g["empty_ratio"]) == 0.0
    matrix, _ = O.overlap_matrix(subs, vs)
    assert all(matrix[i, j] == r for (i, j), r in zip(g["pairs"], g["pair_ratio"]))
    for sel, (lo, hi), want in zip(g["verdict_groups"], g["verdict_lo_hi"], g["verdicts"]):
        sel = [int(s) for s in sel if s >= 0]
        assert O.groups_connected(matrix, sel, lo, hi) == bool(want), sel
    assert g["verdicts"].any() and not g["verdicts"].all()


def test_slerp_rotation_is_scipys_rotvec_scaling():
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(1)
    s = np.array([-1.5, -0.5, -1e-9, 0.0, 1e-9, 0.25, 0.5, 1.0, 1.7, 2.5])
    for th in (0.0, 1e-9, 1e-7, 1e-5, 9.9e-5, 1.01e-4, 1e-3, 0.3, 1.0, 3.0, 3.1415):
        R = np.eye(3) if th == 0.0 else O.rotation(rng.normal(size=3), th)
        w = O.rotvec(R)
        ref = Rotation.from_matrix(R).as_rotvec()
        assert np.abs(w - ref).max() <= 1e-12 * max(th, 1e-3) + 1e-10 * (th > 3.1), (th, w, ref)
        assert abs(np.linalg.norm(w) - th) <= 1e-12 + 1e-9 * (th > 3.1), th
        got = O.slerp_rotation(R, s)
        want = Rotation.from_rotvec(s[:, None] * ref[None]).as_matrix()
        assert np.abs(got - want).max() <= 1e-12 + 1e-8 * (th > 3.1), th
    # the per-point vector form of deskew() is that rotation
    p = rng.normal(size=(s.shape[0], 3)).astype(np.float32)
    M = O.make_pose(rng, 0.7)
    ts = np.linspace(0, 1, s.shape[0]).astype(np.float32)
    sp = ts.astype(np.float64) - 0.5
    want = np.einsum("nij,nj->ni", O.slerp_rotation(M[:3, :3], sp), p.astype(np.float64)) + sp[:, None] * M[:3, 3][None]
    assert np.abs(O.deskew(p, ts, M, 0.5) - want).max() <= 1e-14


def test_deskew_oracle_rules():
    rng = np.random.default_rng(2)
    p, M = O.frame_points(rng, 50), O.make_pose(rng, 0.4)
    const = np.full(50, 0.3, np.float32)
    assert np.array_equal(O.deskew(p, const, M, 0.5), p.astype(np.float64))                     # the 1e-8 rule: s = 0
    half = O.transform_points(p.astype(np.float64), np.block([[O.slerp_rotation(M[:3, :3], [0.5])[0], 0.5 * M[:3, 3:4]], [np.zeros((1, 3)), np.ones((1, 1))]]))
    assert np.abs(O.deskew(p, const, M, 0.0) - half).max() <= 1e-13                             # s = 0.5 - ts_mid
    ts = rng.uniform(0, 1, 50).astype(np.float32)
    assert np.array_equal(O.deskew(p, ts, np.eye(4), 0.5), p.astype(np.float64))                # identity: untouched
    ts[0], ts[-1] = 1.0, 0.0
    full = O.deskew(p, ts, M, 0.0)
    assert np.abs(full[0] - O.transform_points(p[:1].astype(np.float64), M)[0]).max() <= 1e-13  # s = 1: the whole rel_pose
    assert np.array_equal(full[-1], p[-1].astype(np.float64))                                   # s = 0


def test_deskew_bound_is_the_measured_fp32_deviation():
    P, ts, cu, rel, names = O.deskew_case()
    assert set(np.diff(cu)) >= set(O.DESKEW_LENGTHS)
    assert {0.0, 1e-7, 1e-3, 0.3, 3.0} == set(O.DESKEW_THETAS)
    for k in range(len(cu) - 1):                                     # the largest stamp first and the smallest last
        t = ts[cu[k]:cu[k + 1]]
        if t.shape[0] >= 2 and names[k] != "constant_ts":
            assert t[0] == t.max() > t.min() == t[-1]
    worst = 0.0
    for what, (P, ts, cu, rel) in (("case", (P, ts, cu, rel)), ("short frames", O.deskew_short_case())):
        scale = O.deskew_scale(P, cu, rel)
        for mid in O.TS_MIDS:
            d = np.abs(O.deskew_packed(P, ts, cu, rel, mid, np.float32).astype(np.float64) - O.deskew_packed(P, ts, cu, rel, mid)).max(axis=1) / scale
            print(f"{what}, ts_mid {mid}: fp32 formula within {d.max():.3e} of the fp64 one (relative to max(1, |p| + |T|))")
            worst = max(worst, d.max())
    assert f"{worst:.2e}" == f"{O.DESKEW_F32_DEVIATION:.2e}", worst                  # the constant IS the measurement, to three digits
    assert len(O.deskew_short_case()[2]) - 1 == 40 and O.deskew_short_case()[0].shape[0] <= 1024      # one block, more than two rounds of 16 frames


# ---- the margin rule ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", O.OVERLAP_CASES)
def test_overlap_inputs_keep_the_margin_rule(name):
    c = O.overlap_case(name)
    world = O.case_world(c)
    margin = min(O.voxel_margin(w, c["voxel_size"]) for w in world)
    print(f"{name}: smallest margin {margin:.2e}, n_voxels {O.overlap_matrix(world, c['voxel_size'])[1]}")
    assert margin >= 1e-6 or O.exact_quotient(c)
    assert O.exact_quotient(c) == (name == "extent_max")
    ratio, nv = O.overlap_matrix(world, c["voxel_size"])
    S = len(world)
    assert S == {"one": 1, "two": 2, "three": 3, "extent_max": 2, "rows_100k": 3}.get(name.replace("_posed", ""), 5)
    assert (c["pose"] is not None) == name.endswith("_posed")
    assert min(w[np.isfinite(w).all(axis=1)].min() for w in world if w.size) < 0          # floor is not truncation
    if name.startswith("counts"):
        assert list(nv) == [255, 256, 257, 5, 3000] and (ratio[np.triu_indices(5, 1)] > 0).sum() >= 8
    if name == "rows_100k":
        assert c["points"].shape[0] == 99_000 and list(nv) == [11000] * 3 and (ratio[np.triu_indices(3, 1)] > 0.1).all()
    if name.startswith("edge"):
        assert [int(c["cu"][c["submap_frames"][s + 1]] - c["cu"][c["submap_frames"][s]]) for s in range(2)] == [0, 1]      # no row; ONE row
        assert list(nv) == [0, 1, 257, 257, 100] and ratio[2, 3] == 1.0 and ratio[2, 4] == 100 / 257 and ratio[0, 0] == 0.0 and ratio[1, 2] == 0.0
    if name == "three":
        assert list(nv) == [320, 320, 1] and ratio[0, 1] == 0.0 and not np.isfinite(world[0]).all()
    if name == "two":
        assert 0.0 < ratio[0, 1] < 1.0
    if name == "extent_max":
        q = np.floor(np.concatenate(world)[:, 0])
        assert q.max() - q.min() == (1 << 21) - 1
    over = O.extent_case(1 << 21)
    q = np.floor(over["points"].astype(np.float64)[:, 0])
    assert q.max() - q.min() == 1 << 21 and O.exact_quotient(over)


def test_e2e_scene_is_on_its_plane_and_keeps_the_margin():
    P, ts, cu, rel, pose, world, sf = O.e2e_case()
    q = world / O.E2E_VOXEL
    assert np.abs(q - np.round(q)).min() >= 0.09 and np.abs(q).max() < 40          # 0.09 of a voxel (18 cm) from every voxel face
    assert O.voxel_margin(world, O.E2E_VOXEL) >= 1e-3
    back, _ = O.fuse_packed(O.deskew_packed(P, ts, cu, rel, 0.5), cu, pose)           # float64 deskew of the fp32 points, fused in float64
    assert np.abs(back - world).max() <= 2.0 ** -23 * np.abs(P).max() * 3                # only the fp32 rounding of the skewed points is left
    raw, _ = O.fuse_packed(P.astype(np.float64), cu, pose)
    assert np.abs(raw - world)[cu[1]:].max() > 0.3                                       # without deskewing the sweeps are visibly smeared
    assert np.array_equal(rel[0], np.eye(4))
    ratio, nv = O.overlap_matrix([world[cu[sf[s]]:cu[sf[s + 1]]] for s in range(3)], O.E2E_VOXEL)
    assert (ratio[np.triu_indices(3, 1)] > 0.1).all() and (ratio[np.triu_indices(3, 1)] < 1.0).all()


def test_connectivity_case_has_both_verdicts_and_exact_bounds():
    ratio, groups, lo, hi = O.connectivity_case()
    verdicts = [O.groups_connected(ratio, g, lo, hi) for g in groups]
    assert {len(g) for g in groups} >= {1, 2, 3, 64}
    named = dict(zip(map(tuple, groups), verdicts))
    assert named[(0, 1)] and named[(1, 2)]                       # ratio == lo and ratio == hi exactly: inclusive
    assert not named[(0, 2)] and not named[(1, 3)]               # 1/8 and 7/8: outside
    assert named[(0, 1, 2)] and named[(0, 2, 1)] and named[(2, 0, 1)]      # 0-2 only through 1, in any order
    assert not named[(0, 1, 64, 65)] and named[(64, 66, 65)] and not named[(64, 66)]
    assert named[tuple(range(64))] and not named[tuple(range(1, 64)) + (64,)]
    assert sum(verdicts) >= 5 and sum(not v for v in verdicts) >= 5


# ---- the inputs at table scale (tests/test_table_scale_gpu.py) ------------------------------------------------------------------------------
@pytest.mark.parametrize("F", O.SCALE_F)
def test_scale_frames_case_spans_hundreds_of_frames_per_chunk_and_has_both_kinds_of_chunk(F):
    c = O.scale_frames_case(F)
    cu, n = c["cu"], np.diff(c["cu"])
    assert len(cu) == F + 1 and set(n) == set(range(8)) | {O.SCALE_LONG} and n[c["long"]] == O.SCALE_LONG
    frame_of = lambda r: int(np.searchsorted(cu, r, side="right") - 1)
    frames_of = lambda a, b: frame_of(min(b, cu[-1]) - 1) - frame_of(a) + 1       # first to last frame of the rows, the empty ones between them included
    per_chunk = [frames_of(a, a + 1024) for a in range(0, int(cu[-1]), 1024)]
    print(f"F {F}: {cu[-1]} rows, frames per 1024-row chunk {min(per_chunk)} .. {max(per_chunk)}")
    assert max(per_chunk) > 16 * (17 if F == 4099 else 5)                   # a chunk of rows in that many rounds of 16 cached frames
    if F == 4099:
        assert min(per_chunk) < max(per_chunk) // 4                         # and one that lies mostly in the long frame
    assert len(c["identity"]) >= 6 and all(np.array_equal(c["rel_pose"][k], np.eye(4)) for k in c["identity"])
    assert any(n[k] >= 2 for k in c["identity"]) and c["long"] not in c["identity"]
    th = [np.linalg.norm(O.rotvec(M[:3, :3])) for M in c["rel_pose"][:40]]
    assert all(any(abs(t - want) <= 1e-9 + 1e-6 * want for t in th) for want in O.DESKEW_THETAS)
    assert np.abs(np.linalg.norm(c["normals"], axis=1) - 1.0).max() < 1e-6
    four = np.arange(0, int(cu[-1]) - 768, 1)                                # a lane's four rows (256 apart) in four different frames
    f_of = np.searchsorted(cu, np.stack([four + 256 * k for k in range(4)]), side="right") - 1
    assert (np.diff(f_of, axis=0) > 0).any(axis=0).sum() > 500               # the frame switches inside a lane's four rows ...
    assert F != 4099 or (np.diff(f_of, axis=0) > 0).all(axis=0).any()        # ... three times


def test_malformed_scale_tables_are_single_edits_away_from_a_threads_first_entry():
    c = O.scale_frames_case(4099)
    cu, N = c["cu"], c["points"].shape[0]
    per = O.table_per(len(cu))
    assert per == 17
    edits = O.malformed_tables(cu, 3001, N)
    assert [name for name, _ in edits] == ["decreasing", "past the limit", "short of the end"]
    for name, bad in edits:
        at = np.flatnonzero(bad != cu)
        assert at.size == 1 and at[0] % per != 0 and at[0] // per > 0, name      # one entry; not a thread's first; not thread 0's
    sf = O.overlap_scale_case(1025)["submap_frames"]
    per = O.table_per(len(sf))
    assert per == 5
    for name, bad in O.malformed_tables(sf, 1023, int(sf[-1]), need_last=False):
        at = np.flatnonzero(bad != sf)
        assert at.size == 1 and at[0] % per != 0 and at[0] // per > 0, name
    o = O.overlap_scale_case(1025)
    assert len(O.malformed_tables(o["cu"], 2001, o["points"].shape[0])) == 3 and 2001 % O.table_per(len(o["cu"])) != 0
    P, ts, cu, rel = O.boundary_repeats_case()
    assert (np.diff(cu) >= 0).all() and cu[0] == 0 and cu[-1] == P.shape[0] == ts.shape[0] and len(cu) == 4100


def test_incidence_oracle_equals_the_set_oracle():
    cases = [(name, O.overlap_case(name)) for name in O.OVERLAP_CASES] + [("scale 257", O.overlap_scale_case(257))]
    for name, c in cases:
        world = O.case_world(c)
        a, an = O.overlap_matrix(world, c["voxel_size"])
        b, bn = O.overlap_matrix_incidence(world, c["voxel_size"])
        assert np.array_equal(a, b) and np.array_equal(an, bn) and b.dtype == np.float64, name      # as doubles
    r, n = O.overlap_matrix_incidence([np.zeros((0, 3)), np.zeros((0, 3))], 1.0)
    assert not r.any() and not n.any()


@pytest.mark.parametrize("S", O.SCALE_S)
def test_overlap_scale_inputs_keep_the_margin_rule_and_tie_in_size(S):
    c = O.overlap_scale_case(S)
    world = O.case_world(c)
    margin = min(O.voxel_margin(w, c["voxel_size"]) for w in world)
    ratio, nv = O.overlap_scale_oracle(S)
    pairs = np.triu_indices(S, 1)
    both = ((nv[:, None] > 0) & (nv[None, :] > 0))[pairs]
    share = (ratio[pairs] > 0).sum() / both.sum()
    print(f"S {S}: {c['points'].shape[0]} rows in {len(c['cu']) - 1} frames, smallest margin {margin:.2e}, {share:.0%} of the pairs intersect, "
          f"sizes {dict(zip(*np.unique(nv, return_counts=True)))}")
    assert margin >= 1e-6 and not O.exact_quotient(c)
    assert (c["pose"] is not None) == (S != 4096)
    assert len(world) == S and np.array_equal(nv, c["counts"])
    assert set(np.diff(c["submap_frames"])) == {1, 2, 3, 4}
    for rare in O.SCALE_RARE:
        assert (nv == rare).sum() >= 2
    for tie in O.SCALE_COUNTS:                                           # the ordering rule decides among many submaps of equal size
        assert (nv == tie).sum() >= S // 5
    assert share > 0.5 and np.array_equal(ratio, ratio.T) and (np.diag(ratio) == (nv > 0)).all()
    assert min(w.min() for w in world if w.size) < 0
    if S == 4096:                                                        # rows before the first and after the last submap, far outside the grid
        sf, cu = c["submap_frames"], c["cu"]
        assert sf[0] == 1 and sf[-1] == len(cu) - 2 and cu[1] > 256 and cu[-1] - cu[-2] > 0
        assert np.abs(c["points"][0]).min() >= 1e7 and np.abs(c["points"][cu[-2]]).min() >= 1e7
        assert np.abs(np.concatenate(world)).max() < 100


def test_connectivity_scale_case_has_both_verdicts_in_a_quarter_of_the_groups_each():
    ratio, groups, lo, hi, bad = O.connectivity_scale_case()
    assert ratio.shape == (O.CONN_S, O.CONN_S) and len(groups) == O.CONN_G == 1027 and O.CONN_G % 4
    good = [g for k, g in enumerate(groups) if k not in bad]
    assert {len(g) for g in good} == set(range(1, 65))
    assert min(min(g) for g in good) < 8 and max(max(g) for g in good) >= O.CONN_S - 8
    verdicts = [O.groups_connected(ratio, g, lo, hi) for g in good]
    print(f"{sum(verdicts)} of {len(verdicts)} groups connected at lo = {lo}")
    assert sum(verdicts) >= len(groups) // 4 and len(verdicts) - sum(verdicts) >= len(groups) // 4
    assert [len(groups[k]) for k in bad] == [0, 4, 0] and groups[bad[1]][-1] == O.CONN_S
    assert len({k // 4 for k in bad}) == 3 and bad[-1] == O.CONN_G - 1      # three different blocks of four groups, the last one partial


# ---- the C ABI without a GPU ----------------------------------------------------------------------------------------------------------------
def test_workspace_queries_are_host_arithmetic():
    lib = _lib.load()
    for n, F in ((0, 1), (1, 1), (1000, 9), (12_000_000, 200), ((1 << 31) - 1, 1 << 24)):
        assert lib.rap_deskew_workspace_bytes(n, F) == up((F + 1) * 4) + 256 + up(F * 8), (n, F)
        assert lib.rap_fuse_frames_workspace_bytes(n, F) == up((F + 1) * 4) + 256, (n, F)
        for S in (1, 20, 4096):
            want = up((F + 1) * 4) + 4 * up((S + 1) * 4) + 256 + 256 + up(S * S * 4) + 3 * up(8 * n) + 4 * up(4 * n) + up(8 * n + 65536)
            assert lib.rap_submap_overlap_workspace_bytes(n, F, S) == want, (n, F, S)
    for q in (lib.rap_deskew_workspace_bytes, lib.rap_fuse_frames_workspace_bytes):
        assert q(-1, 4) == 0 and q(1 << 31, 4) == 0 and q(10, -1) == 0 and q(10, (1 << 24) + 1) == 0 and q(0, 0) == 0
    q = lib.rap_submap_overlap_workspace_bytes
    assert q(-1, 4, 2) == 0 and q(1 << 31, 4, 2) == 0 and q(10, 0, 2) == 0 and q(10, 4, 0) == 0 and q(10, 4, 4097) == 0


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = _lib.load()
    big = 1 << 40

    def deskew(**kw):
        a = dict(P=ONE, ts=ONE, cu=ONE, F=3, n=100, rel=ONE, mid=0.5, out=ONE, st=N, ws=ONE, wsb=big)
        a.update(kw)
        return lib.rap_deskew(*a.values(), N)
    for name in ("P", "ts", "cu", "rel", "out"):
        assert deskew(**{name: N}) == -1, name
    assert deskew(n=-1) == -1 and deskew(n=1 << 31) == -1 and deskew(F=-1) == -1 and deskew(F=(1 << 24) + 1) == -1 and deskew(mid=float("nan")) == -1
    assert deskew(F=0) == -1 and deskew(F=0, n=0, P=N, ts=N, cu=N, rel=N, out=N, ws=N, wsb=0) == 0        # points without a frame; nothing at all
    need = lib.rap_deskew_workspace_bytes(100, 3)
    assert deskew(ws=N) == -2 and deskew(wsb=need - 1) == -2 and deskew(wsb=0) == -2

    def fuse(**kw):
        a = dict(P=ONE, nrm=N, cu=ONE, F=3, n=100, pose=ONE, org=N, world=ONE, wn=N, st=N, ws=ONE, wsb=big)
        a.update(kw)
        return lib.rap_fuse_frames(*a.values(), N)
    for name in ("P", "cu", "pose", "world"):
        assert fuse(**{name: N}) == -1, name
    assert fuse(nrm=ONE) == -1 and fuse(wn=ONE) == -1                                   # normals in and out: both or neither
    assert fuse(n=-1) == -1 and fuse(n=1 << 31) == -1 and fuse(F=-1) == -1 and fuse(F=0) == -1
    assert fuse(F=0, n=0, P=N, cu=N, pose=N, world=N, ws=N, wsb=0) == 0
    need = lib.rap_fuse_frames_workspace_bytes(100, 3)
    assert fuse(ws=N) == -2 and fuse(wsb=need - 1) == -2

    def overlap(**kw):
        a = dict(P=ONE, cu=ONE, F=3, n=100, pose=N, sf=ONE, S=2, vs=2.0, ratio=ONE, nv=ONE, st=N, ws=ONE, wsb=big)
        a.update(kw)
        return lib.rap_submap_overlap(*a.values(), N)
    for name in ("P", "cu", "sf", "ratio", "nv"):
        assert overlap(**{name: N}) == -1, name
    assert overlap(F=0) == -1 and overlap(S=0) == -1 and overlap(S=4097) == -1 and overlap(n=-1) == -1 and overlap(n=1 << 31) == -1
    assert overlap(vs=0.0) == -1 and overlap(vs=-1.0) == -1 and overlap(vs=float("nan")) == -1 and overlap(vs=float("inf")) == -1
    need = lib.rap_submap_overlap_workspace_bytes(100, 3, 2)
    assert overlap(ws=N) == -2 and overlap(wsb=need - 1) == -2 and overlap(wsb=0) == -2

    def groups(**kw):
        a = dict(ratio=ONE, S=5, groups=ONE, glen=ONE, G=3, n_max=4, lo=0.1, hi=0.9, out=ONE, st=N)
        a.update(kw)
        return lib.rap_submap_groups_connected(*a.values(), N)
    for name in ("ratio", "groups", "glen", "out"):
        assert groups(**{name: N}) == -1, name
    assert groups(S=0) == -1 and groups(S=4097) == -1 and groups(G=-1) == -1 and groups(n_max=0) == -1 and groups(n_max=65) == -1
    assert groups(lo=float("nan")) == -1 and groups(hi=float("nan")) == -1
    assert groups(G=0, ratio=N, groups=N, glen=N, out=N) == 0
    assert lib.rap_version() == _lib.ABI_VERSION == 6


def test_python_entry_points_refuse_cpu_tensors_and_bad_arguments():
    import rap_amd
    from rap_amd import submaps
    pts, cu, eye = torch.zeros(8, 3), torch.tensor([0, 8]), torch.eye(4, dtype=torch.float64).reshape(1, 4, 4)
    with pytest.raises(_lib.RapError):
        rap_amd.deskew_packed(pts, torch.zeros(8), cu, eye)
    with pytest.raises(_lib.RapError):
        rap_amd.fuse_frames_packed(pts, cu, eye)
    with pytest.raises(_lib.RapError):
        rap_amd.submap_overlap_matrix(pts, cu, torch.tensor([0, 1]))
    with pytest.raises(_lib.RapError):
        rap_amd.groups_connected(torch.zeros(2, 2, dtype=torch.float64), torch.zeros(1, 2, dtype=torch.int32), torch.tensor([2]), 0.1, 0.9)
    with pytest.raises(_lib.RapError):
        rap_amd.deskewing(pts, torch.zeros(8), torch.eye(4))
    with pytest.raises(_lib.RapError):
        rap_amd.create_submap_from_frames([pts], [torch.eye(4)], 0, 1)
    with pytest.raises(_lib.RapError):
        rap_amd.calculate_point_cloud_overlap_ratio_fast(pts, pts)
    with pytest.raises(_lib.RapError):
        rap_amd.check_submap_validity([0], [(0, 0)], None, [pts], [torch.eye(4)], [0], 0, 1, 0.1, 0.9, "voxel")
    with pytest.raises(ValueError):
        rap_amd.deskew_packed(torch.zeros(8, 2), torch.zeros(8), cu, eye)
    assert rap_amd.deskewing(pts, None, torch.eye(4)) is pts                              # ts is None: the input, as the reference
    assert rap_amd.check_submap_validity.__doc__ and "generator" in rap_amd.calculate_point_cloud_overlap_ratio_fast.__doc__
    submaps.check_pending(block=False)                                                    # nothing pending, nothing raised
