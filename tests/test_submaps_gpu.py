"""GPU: rap_deskew, rap_fuse_frames, rap_submap_overlap and rap_submap_groups_connected through the C ABI against the float64 yardstick
(tests/submap_oracle.py), on the smallest shapes at which each kernel can go wrong; then the Python mirrors against the reference's own
recorded outputs (tests/golden/submaps.npz) and a small end-to-end scene.

Bounds.  Deskew: 4 x submap_oracle.DESKEW_F32_DEVIATION (= 4 x 4.66e-7, the measured distance of the fp32 formula from the fp64 one on
these very inputs; tests/test_submaps_host.py measures it and says why 4) of max(1, |p|_inf + |T|_inf) per point.  Fuse: the points are
fp32(oracle) up to 1 ulp, the normals within 2e-6.  Overlap: every input keeps the margin rule (asserted on the host, from the oracle), so
n_voxels and every ratio are demanded EXACTLY.  Connectivity: the oracle's verdicts."""
import ctypes
import os

import numpy as np
import pytest
import torch

import submap_oracle as O
from conftest import ROOT
from rap_amd import _lib

pytestmark = pytest.mark.gpu

F32, F64, I32, I64, U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8
DESKEW_TOL, ulps = O.DESKEW_TOL, O.ulps


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def stream(dev):
    return _lib.current_stream(dev)


def d(a, dev, dtype=None):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(dev)


# ---- the four entry points, raw ---------------------------------------------------------------------------------------------------------
def run_deskew(lib, dev, P, ts, cu, rel, mid):
    N, F = P.shape[0], len(cu) - 1
    out = torch.full((N, 3), float("nan"), dtype=F32, device=dev)
    st = torch.zeros(1, dtype=I32, device=dev)
    need = lib.rap_deskew_workspace_bytes(N, F)
    ws = torch.empty(max(need, 1), dtype=U8, device=dev)
    a = [d(P, dev), d(ts, dev), d(cu, dev, I32), d(rel, dev, F64)]              # held until the call has run
    rc = lib.rap_deskew(_lib.ptr(a[0]), _lib.ptr(a[1]), _lib.ptr(a[2]), F, N, _lib.ptr(a[3]), mid, _lib.ptr(out), _lib.ptr(st), _lib.ptr(ws), need,
                        stream(dev))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(st.item())


def run_fuse(lib, dev, P, nrm, cu, pose, origin):
    N, F = P.shape[0], len(cu) - 1
    world = torch.full((N, 3), float("nan"), dtype=F32, device=dev)
    wn = torch.full((N, 3), float("nan"), dtype=F32, device=dev) if nrm is not None else None
    st = torch.zeros(1, dtype=I32, device=dev)
    need = lib.rap_fuse_frames_workspace_bytes(N, F)
    ws = torch.empty(max(need, 1), dtype=U8, device=dev)
    a = [d(P, dev), d(nrm, dev), d(cu, dev, I32), d(pose, dev, F64), d(origin, dev, F64)]
    rc = lib.rap_fuse_frames(_lib.ptr(a[0]), _lib.ptr(a[1]), _lib.ptr(a[2]), F, N, _lib.ptr(a[3]), _lib.ptr(a[4]), _lib.ptr(world), _lib.ptr(wn),
                             _lib.ptr(st), _lib.ptr(ws), need, stream(dev))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return world.cpu().numpy(), (wn.cpu().numpy() if wn is not None else None), int(st.item())


def run_overlap(lib, dev, c):
    N, F, S = c["points"].shape[0], len(c["cu"]) - 1, len(c["submap_frames"]) - 1
    ratio = torch.full((S, S), -7.0, dtype=F64, device=dev)
    nv = torch.full((S,), -7, dtype=I64, device=dev)
    st = torch.zeros(1, dtype=I32, device=dev)
    need = lib.rap_submap_overlap_workspace_bytes(N, F, S)
    ws = torch.empty(need, dtype=U8, device=dev)
    a = [d(c["points"], dev), d(c["cu"], dev, I32), d(c["pose"], dev, F64), d(c["submap_frames"], dev, I32)]
    rc = lib.rap_submap_overlap(_lib.ptr(a[0]), _lib.ptr(a[1]), F, N, _lib.ptr(a[2]), _lib.ptr(a[3]), S, float(c["voxel_size"]), _lib.ptr(ratio),
                                _lib.ptr(nv), _lib.ptr(st), _lib.ptr(ws), need, stream(dev))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return ratio.cpu().numpy(), nv.cpu().numpy(), int(st.item())


def run_groups(lib, dev, ratio, groups, lo, hi, n_max=64):
    G, S = len(groups), ratio.shape[0]
    g = np.full((G, n_max), -99, np.int32)                      # the entries past a group's length are never read as members
    for k, m in enumerate(groups):
        g[k, :len(m)] = m
    out = torch.full((G,), 9, dtype=U8, device=dev)
    st = torch.zeros(1, dtype=I32, device=dev)
    a = [d(ratio, dev, F64), d(g, dev), d([len(m) for m in groups], dev, I32)]
    rc = lib.rap_submap_groups_connected(_lib.ptr(a[0]), S, _lib.ptr(a[1]), _lib.ptr(a[2]), G, n_max, lo, hi, _lib.ptr(out), _lib.ptr(st), stream(dev))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(st.item())


# ---- deskew -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def deskew_case():
    return O.deskew_case()


@pytest.mark.parametrize("mid", O.TS_MIDS)
def test_deskew_matches_the_oracle_on_every_frame_length_and_angle(lib, dev, deskew_case, mid):
    P, ts, cu, rel, names = deskew_case
    got, status = run_deskew(lib, dev, P, ts, cu, rel, mid)
    assert status == 0 and np.isfinite(got).all()
    want = O.deskew_packed(P, ts, cu, rel, mid)
    err = np.abs(got.astype(np.float64) - want).max(axis=1) / O.deskew_scale(P, cu, rel)
    for k, name in enumerate(names):
        e = err[cu[k]:cu[k + 1]]
        print(f"ts_mid {mid} {name}: worst deviation {e.max() if e.size else 0.0:.2e} (bound {DESKEW_TOL:.2e})")
    assert err.max() <= DESKEW_TOL
    moved = np.abs(got - P).max(axis=1)
    k = names.index("identity")
    assert np.array_equal(got[cu[k]:cu[k + 1]].view(np.uint32), P[cu[k]:cu[k + 1]].view(np.uint32))      # identity rel_pose: bit for bit
    k = names.index("constant_ts")
    if mid == 0.5:                                                                                       # the 1e-8 rule: s = 0, bit for bit
        assert np.array_equal(got[cu[k]:cu[k + 1]].view(np.uint32), P[cu[k]:cu[k + 1]].view(np.uint32))
        assert np.array_equal(got[cu[1]:cu[2]].view(np.uint32), P[cu[1]:cu[2]].view(np.uint32))          # the one-point frame likewise
    else:
        assert moved[cu[k]:cu[k + 1]].min() > 1e-3                                                       # s = 0.5 - ts_mid: everything moves
    assert moved[cu[8]:cu[9]].max() > 1.0                                                                # the 1025-row frame is really deskewed


def test_deskew_single_frame_no_frame_and_repeatability(lib, dev, deskew_case):
    P, ts, cu, rel, names = deskew_case
    a, b = int(cu[8]), int(cu[9])                                  # F = 1: the 1025-row frame alone
    one, status = run_deskew(lib, dev, P[a:b], ts[a:b], np.array([0, b - a]), rel[8:9], 0.5)
    full, _ = run_deskew(lib, dev, P, ts, cu, rel, 0.5)
    assert status == 0 and np.array_equal(one.view(np.uint32), full[a:b].view(np.uint32))      # a frame's bits do not depend on its neighbours
    again, _ = run_deskew(lib, dev, P, ts, cu, rel, 0.5)
    assert np.array_equal(full.view(np.uint32), again.view(np.uint32))                          # two calls, the same bits
    assert lib.rap_deskew(None, None, None, 0, 0, None, 0.5, None, None, None, 0, stream(dev)) == 0      # F = 0: valid, nothing to do
    empty, status = run_deskew(lib, dev, np.zeros((0, 3), np.float32), np.zeros(0, np.float32), np.array([0, 0, 0]), rel[:2], 0.5)
    assert status == 0 and empty.shape == (0, 3)                                                # only empty frames


def test_deskew_block_with_more_frames_than_one_round(lib, dev):
    P, ts, cu, rel = O.deskew_short_case()                          # 40 frames in one block of rows: three rounds of 16 frames
    for mid in O.TS_MIDS:
        got, status = run_deskew(lib, dev, P, ts, cu, rel, mid)
        err = np.abs(got.astype(np.float64) - O.deskew_packed(P, ts, cu, rel, mid)).max(axis=1) / O.deskew_scale(P, cu, rel)
        print(f"40 short frames, ts_mid {mid}: worst deviation {err.max():.2e} (bound {DESKEW_TOL:.2e})")
        assert status == 0 and err.max() <= DESKEW_TOL


def test_deskew_nan_stamp_gives_nan_except_in_an_identity_frame(lib, dev, deskew_case):
    P, ts, cu, rel, names = deskew_case
    ts = ts.copy()
    k, i = names.index("identity"), 5
    ts[cu[i] + 3] = ts[cu[k] + 3] = np.nan
    got, status = run_deskew(lib, dev, P, ts, cu, rel, 0.5)
    assert status == 0 and np.isnan(got[cu[i] + 3]).all() and np.isnan(got).any(axis=1).sum() == 1       # that row, and no other
    assert np.array_equal(got[cu[k]:cu[k + 1]].view(np.uint32), P[cu[k]:cu[k + 1]].view(np.uint32))        # the identity frame is copied
    clean, _ = run_deskew(lib, dev, P, deskew_case[1], cu, rel, 0.5)
    rest = np.ones(len(P), bool)
    rest[cu[i] + 3] = False
    assert np.array_equal(got[rest].view(np.uint32), clean[rest].view(np.uint32))                          # min and max ignore a NaN stamp


def test_deskew_malformed_table_gives_nan_and_the_status_bit(lib, dev, deskew_case):
    P, ts, cu, rel, _ = deskew_case
    for bad in (np.where(np.arange(len(cu)) == 3, cu[5], cu), np.concatenate([cu[:-1], [cu[-1] + 7]]), np.concatenate([[2], cu[1:]]),
                np.concatenate([cu[:-1], [cu[-1] - 1]])):              # decreasing; past the end; not from 0; short of the end
        got, status = run_deskew(lib, dev, P, ts, bad.astype(np.int32), rel, 0.5)
        assert status == 1 and np.isnan(got).all()


# ---- fuse ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_origin", [False, True], ids=["no_origin", "origin"])
def test_fuse_frames_is_the_rounded_float64_transform(lib, dev, with_origin):
    P, nrm, cu, pose = O.fuse_case()
    origin = np.array(O.FUSE_FAR) + np.array([3.0, -2.0, 1.0]) if with_origin else None
    world, wn, status = run_fuse(lib, dev, P, nrm, cu, pose, origin)
    want, want_n = O.fuse_packed(P, cu, pose, nrm, origin)
    assert status == 0
    assert (np.sign(world) == np.sign(want.astype(np.float32))).all()              # so that the integer distance below is in ulp
    print(f"origin {with_origin}: points within {ulps(world, want)} ulp of fp32(oracle), |coordinates| up to {np.abs(want).max():.0f}; "
          f"normals within {np.abs(wn - want_n).max():.2e}")
    assert ulps(world, want) <= 1
    assert np.abs(wn.astype(np.float64) - want_n).max() <= 2e-6
    zero = ~nrm.any(axis=1)
    assert zero.sum() == 7 and not wn[zero].any()                                   # a zero normal comes back unchanged
    assert np.abs(want).max() > 9_000 if not with_origin else np.abs(want).max() < 200
    # an empty submap, and a submap of the empty frame plus the next two: the caller's indexing of the packed output
    sf = np.array([0, 0, 3, 9])
    for s in range(3):
        a, b = cu[sf[s]], cu[sf[s + 1]]
        sub, _ = O.create_submap_from_frames([P[cu[k]:cu[k + 1]].astype(np.float64) for k in range(9)], list(pose), int(sf[s]), int(sf[s + 1] - sf[s]))
        sub = sub.reshape(-1, 3) - (origin if with_origin else 0.0)
        assert sub.shape[0] == b - a and ulps(world[a:b], sub) <= 1
    world2, wn2, _ = run_fuse(lib, dev, P, nrm, cu, pose, origin)
    assert np.array_equal(world.view(np.uint32), world2.view(np.uint32)) and np.array_equal(wn.view(np.uint32), wn2.view(np.uint32))
    only, none, _ = run_fuse(lib, dev, P, None, cu, pose, origin)                   # without normals
    assert none is None and np.array_equal(only.view(np.uint32), world.view(np.uint32))


def test_fuse_frames_malformed_table_gives_nan_and_the_status_bit(lib, dev):
    P, nrm, cu, pose = O.fuse_case()
    bad = cu.copy()
    bad[4] = -3
    world, wn, status = run_fuse(lib, dev, P, nrm, bad, pose, None)
    assert status == 1 and np.isnan(world).all() and np.isnan(wn).all()
    assert lib.rap_fuse_frames(None, None, None, 0, 0, None, None, None, None, None, None, 0, stream(dev)) == 0


# ---- overlap ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", O.OVERLAP_CASES)
def test_overlap_matrix_is_exactly_the_oracles(lib, dev, name):
    c = O.overlap_case(name)
    want, want_n = O.overlap_matrix(O.case_world(c), c["voxel_size"])
    ratio, nv, status = run_overlap(lib, dev, c)
    print(f"{name}: n_voxels {nv}, ratios {ratio[np.triu_indices(len(nv), 1)]}")
    assert status == 0
    assert np.array_equal(nv, want_n)
    assert np.array_equal(ratio, want)                              # exactly, as doubles
    assert np.array_equal(ratio, ratio.T)
    again = run_overlap(lib, dev, c)
    assert np.array_equal(again[0], ratio) and np.array_equal(again[1], nv)


def test_overlap_one_voxel_too_wide_gives_nan_and_the_status_bit(lib, dev):
    ratio, nv, status = run_overlap(lib, dev, O.extent_case(1 << 21))
    assert status == 2 and np.isnan(ratio).all() and (nv == -1).all()
    ratio, nv, status = run_overlap(lib, dev, O.extent_case((1 << 21) - 1))
    assert status == 0 and np.array_equal(ratio, np.eye(2)) and list(nv) == [1, 1]
    # finite coordinates whose quotient overflows (a voxel of 1e-300): not dropped, not one shared voxel -- the extent error
    tiny = {**O.extent_case(5), "voxel_size": 1e-300}
    ratio, nv, status = run_overlap(lib, dev, tiny)
    assert status == 2 and np.isnan(ratio).all() and (nv == -1).all()


def test_overlap_malformed_tables_give_nan_and_the_status_bit(lib, dev):
    c = O.overlap_case("two")
    for key, bad in (("submap_frames", [0, 3, 2]), ("submap_frames", [0, 2, 9]), ("cu", np.concatenate([c["cu"][:-1], [c["cu"][-1] + 1]]))):
        ratio, nv, status = run_overlap(lib, dev, {**c, key: np.asarray(bad, np.int32)})
        assert status == 1 and np.isnan(ratio).all() and (nv == -1).all(), key
    # submaps need not cover every frame: the first and the last frame left out
    part = {**c, "submap_frames": np.array([1, 2, 3], np.int32)}
    want, want_n = O.overlap_matrix(O.case_world(part), c["voxel_size"])
    ratio, nv, status = run_overlap(lib, dev, part)
    assert status == 0 and np.array_equal(ratio, want) and np.array_equal(nv, want_n)


# ---- connectivity -------------------------------------------------------------------------------------------------------------------------
def test_groups_connected_gives_the_oracles_verdicts(lib, dev):
    ratio, groups, lo, hi = O.connectivity_case()
    want = [O.groups_connected(ratio, g, lo, hi) for g in groups]
    got, status = run_groups(lib, dev, ratio, groups, lo, hi)
    assert status == 0 and list(got) == [int(v) for v in want]
    small = [g for g in groups if len(g) <= 3]                       # n_max = 3: the row pitch of the group table
    got3, _ = run_groups(lib, dev, ratio, small, lo, hi, n_max=3)
    assert list(got3) == [int(O.groups_connected(ratio, g, lo, hi)) for g in small]
    again, _ = run_groups(lib, dev, ratio, groups, lo, hi)
    assert np.array_equal(again, got)
    # an asymmetric matrix: the pair is read in the group's order, as the reference computes it
    lop = ratio.copy()
    lop[1, 0] = 0.0
    assert list(run_groups(lib, dev, lop, [[0, 1], [1, 0]], lo, hi)[0]) == [1, 0]
    nan = ratio.copy()
    nan[0, 1] = nan[1, 0] = np.nan
    assert list(run_groups(lib, dev, nan, [[0, 1]], lo, hi)[0]) == [0]


def test_groups_connected_malformed_groups_give_zero_and_the_status_bit(lib, dev):
    ratio, _, lo, hi = O.connectivity_case()
    got, status = run_groups(lib, dev, ratio, [[0, 1], [], [0, 80], [0, -1], [1, 2]], lo, hi)
    assert status == 4 and list(got) == [1, 0, 0, 0, 1]


# ---- the Python layer: packed forms, mirrors, the reference's recorded outputs -----------------------------------------------------------
def test_mirrors_reproduce_the_reference_fixture(dev):
    import rap_amd
    g = np.load(os.path.join(ROOT, "tests", "golden", "submaps.npz"))
    pts, nrm, poses = list(g["points"]), list(g["normals"]), list(g["poses"])
    vs = float(g["voxel_size"])
    subs = []
    for k, (a, b) in enumerate(g["boundaries"]):
        fp, fn = rap_amd.create_submap_from_frames(pts, poses, int(a), int(b - a + 1), nrm)
        assert isinstance(fp, np.ndarray) and ulps(fp, g[f"fused_points_{k}"]) <= 1 and np.abs(fn - g[f"fused_normals_{k}"]).max() <= 2e-6
        subs.append(fp)
    tp, tn = rap_amd.create_submap_from_frames([torch.from_numpy(p).to(dev) for p in pts], poses, 2, 2)
    assert tn is None and tp.is_cuda and np.array_equal(tp.cpu().numpy(), subs[1])
    for (i, j), want in zip(g["pairs"], g["pair_ratio"]):
        assert rap_amd.calculate_point_cloud_overlap_ratio_fast(subs[i], subs[j], voxel_size=vs) == want       # exactly the reference's float
    assert rap_amd.calculate_point_cloud_overlap_ratio_fast(np.zeros((0, 3)), subs[0], voxel_size=vs) == 0.0
    gen = torch.Generator(device=dev).manual_seed(3)
    cut = rap_amd.calculate_point_cloud_overlap_ratio_fast(subs[0], subs[4], voxel_size=vs, max_points_per_cloud=30, generator=gen)
    gen.manual_seed(3)
    assert cut == rap_amd.calculate_point_cloud_overlap_ratio_fast(subs[0], subs[4], voxel_size=vs, max_points_per_cloud=30, generator=gen)
    assert 0.0 <= cut < 1.0 and cut != g["pair_ratio"][1]                                                      # a subset of 30 of 80 points
    bounds = [tuple(int(v) for v in b) for b in g["boundaries"]]
    for sel, (lo, hi), want in zip(g["verdict_groups"], g["verdict_lo_hi"], g["verdicts"]):
        sel = [int(s) for s in sel if s >= 0]
        assert rap_amd.check_submap_validity(sel, bounds, None, pts, poses, list(range(8)), 0.0, 1e9, lo, hi, "voxel", 0, vs) == bool(want), sel


def test_deskewing_mirror_and_the_deferred_error(dev, deskew_case):
    import rap_amd
    from rap_amd import submaps
    P, ts, cu, rel, names = deskew_case
    a, b = int(cu[8]), int(cu[9])
    want = O.deskew(P[a:b], ts[a:b], rel[8], 0.5)
    p4 = np.concatenate([P[a:b], np.arange(b - a, dtype=np.float32)[:, None]], axis=1)            # (N,4): intensity kept
    got = rap_amd.deskewing(p4, ts[a:b, None], rel[8])
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and np.array_equal(got[:, 3], p4[:, 3])
    assert (np.abs(got[:, :3] - want).max(axis=1) / O.deskew_scale(P[a:b], [0, b - a], rel[8:9])).max() <= DESKEW_TOL
    t = rap_amd.deskewing(torch.from_numpy(P[a:b]).to(dev), torch.from_numpy(ts[a:b]).to(dev), torch.from_numpy(rel[8]).to(dev))
    assert t.is_cuda and np.array_equal(t.cpu().numpy(), got[:, :3])
    # the packed form does not wait; a malformed table surfaces later, as NaN results and a ValueError
    bad = cu.copy()
    bad[2] = 10_000
    out = rap_amd.deskew_packed(torch.from_numpy(P).to(dev), torch.from_numpy(ts).to(dev), torch.from_numpy(bad).to(dev), torch.from_numpy(rel).to(dev))
    with pytest.raises(ValueError, match="prefix table"):
        submaps.synchronize()
    assert torch.isnan(out).all()
    submaps.synchronize()                                                                        # reported once
    mine = torch.zeros(1, dtype=I32, device=dev)                                                 # the caller's own status word: not followed
    rap_amd.deskew_packed(torch.from_numpy(P).to(dev), torch.from_numpy(ts).to(dev), torch.from_numpy(bad).to(dev), torch.from_numpy(rel).to(dev),
                          status=mine)
    submaps.synchronize()
    assert int(mine.item()) == 1


def test_end_to_end_plane_scene(dev):
    """6 sweeps of 2000 points of a horizontal plane, skewed in float64 by the inverse of the motion model: deskew, then fuse, puts every
    point back on the plane, and the overlap matrix of the three two-frame submaps is the oracle's.  Distance allowed to a point:
    sqrt(3) x (the deskew bound x max(1, |p| + |T|) + the fp32 rounding of the skewed input, 2^-24 |p|) + one fp32 ulp of the fused
    coordinate (2^-23 |X|) -- a rigid pose does not stretch the first two."""
    import rap_amd
    P, ts, cu, rel, pose, world, sf = O.e2e_case()
    tP, tcu = torch.from_numpy(P).to(dev), torch.from_numpy(cu).to(dev)
    desk = rap_amd.deskew_packed(tP, torch.from_numpy(ts).to(dev), tcu, torch.from_numpy(rel).to(dev))
    fused = rap_amd.fuse_frames_packed(desk, tcu, torch.from_numpy(pose).to(dev))
    ratio, nv = rap_amd.submap_overlap_matrix(desk, tcu, torch.from_numpy(sf).to(dev), O.E2E_VOXEL, pose=torch.from_numpy(pose).to(dev))
    ok = rap_amd.groups_connected(ratio, torch.tensor([[0, 1, 2], [2, 0, 1]], dtype=I32, device=dev), torch.tensor([3, 3], dtype=I32, device=dev), 0.05, 0.99)
    rap_amd.submaps.synchronize()
    got = fused.cpu().numpy().astype(np.float64)
    scale = O.deskew_scale(P, cu, rel)
    allowed = np.sqrt(3.0) * (DESKEW_TOL * scale + 2.0 ** -24 * np.abs(P).max(axis=1)) + 2.0 ** -23 * np.abs(world).max(axis=1)
    off = np.abs(got[:, 2] - O.E2E_PLANE_Z)
    print(f"worst distance from the plane {off.max():.2e} (allowed there {allowed[off.argmax()]:.2e}); worst |X - truth| {np.abs(got - world).max():.2e}")
    assert (off <= allowed).all()
    assert (np.abs(got - world).max(axis=1) <= allowed).all()                     # and at the right place on it
    assert np.array_equal(desk[:cu[1]].cpu().numpy().view(np.uint32), P[:cu[1]].view(np.uint32))       # frame 0: identity rel_pose, untouched
    # the oracle on the very points the device deskewed; their voxels are those of the truth (0.09 of a voxel from every face)
    dw, _ = O.fuse_packed(desk.cpu().numpy(), cu, pose)
    assert O.voxel_margin(dw, O.E2E_VOXEL) >= 1e-3
    want, want_n = O.overlap_matrix([dw[cu[sf[s]]:cu[sf[s + 1]]] for s in range(3)], O.E2E_VOXEL)
    truth, _ = O.overlap_matrix([world[cu[sf[s]]:cu[sf[s + 1]]] for s in range(3)], O.E2E_VOXEL)
    assert np.array_equal(ratio.cpu().numpy(), want) and np.array_equal(nv.cpu().numpy(), want_n) and np.array_equal(want, truth)
    assert list(ok.cpu().numpy()) == [int(O.groups_connected(want, [0, 1, 2], 0.05, 0.99))] * 2
