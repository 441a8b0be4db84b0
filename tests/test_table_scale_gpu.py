"""GPU: caller's tables of hundreds and thousands of entries -- past the first round of the block or wave that walks them.

Submaps.  tests/test_submaps_gpu.py stops at F = 40 frames and S = 5 submaps, where every thread of the table kernel has one entry, the
`s += 256` loops run once and the intersect kernel meets four partners; a drive has thousands of sweeps and hundreds of submaps.  Here
F goes to 4099 and S to 4096 (the limit), G to 1027 groups, on arrays of a few rows per entry.

ICP and normals.  No other test has more than 6 problems or segments, or (against the yardstick) more than 64 items of 256 queries.  Here
K = 300 problems of both estimators and both searches, one problem of 66 and of 129 items, and K = 300 segments for the normals, at the
bound of tests/test_icp_gpu.py, tests/test_icp_plane_gpu.py and tests/test_normals_gpu.py: 2e-6.  R, T, rmse and `converged` are
compared for every problem, and so is the iteration count, for both estimators.  For point-to-point a run stops when the
correspondences repeat, and then the rmse repeats bit for bit.  For point-to-plane the stop compares successive rmse values that the fp32
moved points move by 1e-6 of themselves, so that estimator gets a variant of the batch whose inputs are chosen, from the yardstick
alone, so that no stopping decision is a matter of rounding: lattice problems with a residual, and relative_rmse_thr = 1e-3 (see BATCH_THR in
tests/icp_plane_oracle.py and BATCH_PLANE_STEPS in tests/icp_oracle.py; tests/test_icp_plane_host.py proves it for at least 98 % of
the problems, and the tests here fail below that share).

Yardsticks and bounds are those of tests/test_submaps_gpu.py, none new: deskew within DESKEW_TOL, fused points within 1 ulp of
fp32(oracle) and normals within 2e-6, n_voxels and every ratio exact (the margin rule, asserted on the host for every input here), the
oracle's verdicts.  The inputs live in tests/submap_oracle.py; tests/test_submaps_host.py proves what they are meant to contain.  Every
parity test prints its worst deviation before it asserts (run with -s to see them)."""
import numpy as np
import pytest
import torch

import icp_oracle as I
import icp_plane_oracle as PO
import rap_amd
import submap_oracle as O
from rap_amd import _lib
from test_submaps_gpu import run_deskew, run_fuse, run_groups, run_overlap

pytestmark = pytest.mark.gpu

DESKEW_TOL, ulps = O.DESKEW_TOL, O.ulps
u32 = lambda a: a.view(np.uint32)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def solo_frames(c):
    """frames to run alone: the long one, an identity one, the first and the last non-empty one, and one that a 1024-row chunk boundary cuts"""
    cu = c["cu"]
    full = [k for k in range(len(cu) - 1) if cu[k + 1] > cu[k]]
    cut = [k for k in full if cu[k] % 1024 > cu[k + 1] % 1024 and k != c["long"]]
    return sorted({c["long"], next(k for k in c["identity"] if cu[k + 1] - cu[k] >= 2), full[0], full[-1], *cut[:2]})


# ---- deskew and fuse ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", O.SCALE_F)
def test_deskew_over_thousands_of_short_frames(lib, dev, F):
    c = O.scale_frames_case(F)
    P, ts, cu, rel = c["points"], c["ts"], c["cu"], c["rel_pose"]
    scale = O.deskew_scale(P, cu, rel)
    for mid in (0.5, 0.0):
        got, status = run_deskew(lib, dev, P, ts, cu, rel, mid)
        assert status == 0 and np.isfinite(got).all()
        err = np.abs(got.astype(np.float64) - O.deskew_packed(P, ts, cu, rel, mid)).max(axis=1) / scale
        print(f"F {F}, {P.shape[0]} rows, ts_mid {mid}: worst deviation {err.max():.2e} at row {err.argmax()} (bound {DESKEW_TOL:.2e})")
        assert err.max() <= DESKEW_TOL
        for k in c["identity"]:                                              # identity rel_pose: bit for bit
            assert np.array_equal(u32(got[cu[k]:cu[k + 1]]), u32(P[cu[k]:cu[k + 1]])), k
        a, b = cu[c["long"]], cu[c["long"] + 1]
        assert np.abs(got[a:b] - P[a:b]).max() > 1.0                         # the long frame is really deskewed
    full, _ = run_deskew(lib, dev, P, ts, cu, rel, 0.5)
    again, _ = run_deskew(lib, dev, P, ts, cu, rel, 0.5)
    assert np.array_equal(u32(full), u32(again))
    for k in solo_frames(c):                                                 # a frame's bits do not depend on its thousands of neighbours
        a, b = int(cu[k]), int(cu[k + 1])
        one, status = run_deskew(lib, dev, P[a:b], ts[a:b], np.array([0, b - a]), rel[k:k + 1], 0.5)
        assert status == 0 and np.array_equal(u32(one), u32(full[a:b])), k


@pytest.mark.parametrize("F", O.SCALE_F)
def test_fuse_over_thousands_of_short_frames(lib, dev, F):
    c = O.scale_frames_case(F)
    P, nrm, cu, pose = c["points"], c["normals"], c["cu"], c["pose"]
    origin = np.array([3.0, -2.0, 1.0])
    world, wn, status = run_fuse(lib, dev, P, nrm, cu, pose, origin)
    want, want_n = O.fuse_packed(P, cu, pose, nrm, origin)
    assert status == 0 and (np.sign(world) == np.sign(want.astype(np.float32))).all()
    print(f"F {F}: points within {ulps(world, want)} ulp of fp32(oracle), normals within {np.abs(wn - want_n).max():.2e}")
    assert ulps(world, want) <= 1
    assert np.abs(wn.astype(np.float64) - want_n).max() <= 2e-6
    world2, wn2, _ = run_fuse(lib, dev, P, nrm, cu, pose, origin)
    assert np.array_equal(u32(world), u32(world2)) and np.array_equal(u32(wn), u32(wn2))
    for k in solo_frames(c):
        a, b = int(cu[k]), int(cu[k + 1])
        one, one_n, status = run_fuse(lib, dev, P[a:b], nrm[a:b], np.array([0, b - a]), pose[k:k + 1], origin)
        assert status == 0 and np.array_equal(u32(one), u32(world[a:b])) and np.array_equal(u32(one_n), u32(wn[a:b])), k


def test_one_bad_entry_deep_in_a_table_of_thousands_is_found(lib, dev):
    c = O.scale_frames_case(4099)
    P, ts, cu, rel, N = c["points"], c["ts"], c["cu"], c["rel_pose"], c["points"].shape[0]
    for name, bad in O.malformed_tables(cu, 3001, N):                        # entry 3001: the tenth of the seventeen of thread 176
        got, status = run_deskew(lib, dev, P, ts, bad, rel, 0.5)
        assert status == 1 and np.isnan(got).all(), name
        world, wn, status = run_fuse(lib, dev, P, c["normals"], bad, c["pose"], None)
        assert status == 1 and np.isnan(world).all() and np.isnan(wn).all(), name
    o = O.overlap_scale_case(1025)
    sf = o["submap_frames"]
    # (no "last entry short of the end" here: submaps need not cover every frame, so the kernel does not hold this table's end to anything)
    for name, bad in O.malformed_tables(sf, 1023, int(sf[-1]), need_last=False):
        ratio, nv, status = run_overlap(lib, dev, {**o, "submap_frames": bad})
        assert status == 1 and np.isnan(ratio).all() and (nv == -1).all(), name
    for name, bad in O.malformed_tables(o["cu"], 2001, o["points"].shape[0]):
        ratio, nv, status = run_overlap(lib, dev, {**o, "cu": bad})
        assert status == 1 and np.isnan(ratio).all() and (nv == -1).all(), name


def test_repeated_entries_on_thread_boundaries_are_not_an_error(lib, dev):
    P, ts, cu, rel = O.boundary_repeats_case()
    got, status = run_deskew(lib, dev, P, ts, cu, rel, 0.0)
    err = np.abs(got.astype(np.float64) - O.deskew_packed(P, ts, cu, rel, 0.0)).max(axis=1) / O.deskew_scale(P, cu, rel)
    print(f"empty frames on every thread boundary: status {status}, worst deviation {err.max():.2e} (bound {DESKEW_TOL:.2e})")
    assert status == 0 and err.max() <= DESKEW_TOL
    world, _, status = run_fuse(lib, dev, P, None, cu, rel, None)
    assert status == 0 and ulps(world, O.fuse_packed(P, cu, rel)[0]) <= 1


# ---- overlap --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", O.SCALE_S)
def test_overlap_matrix_of_hundreds_of_submaps_is_exactly_the_oracles(lib, dev, S):
    c = O.overlap_scale_case(S)
    want, want_n = O.overlap_scale_oracle(S)
    ratio, nv, status = run_overlap(lib, dev, c)
    wrong = np.argwhere(ratio != want)
    print(f"S {S}: {c['points'].shape[0]} rows, {len(c['cu']) - 1} frames; n_voxels wrong at {np.flatnonzero(nv != want_n)[:8]}, "
          f"{wrong.shape[0]} ratios differ{'' if not wrong.size else f', the first at {wrong[0]}'}")
    assert status == 0
    assert np.array_equal(nv, want_n)
    assert np.array_equal(ratio, want)                                       # exactly, as doubles
    assert np.array_equal(ratio, ratio.T)
    again = run_overlap(lib, dev, c)
    assert np.array_equal(again[0], ratio) and np.array_equal(again[1], nv) and again[2] == 0


# ---- connectivity ---------------------------------------------------------------------------------------------------------------------------
def test_a_thousand_groups_on_a_real_matrix_get_the_oracles_verdicts(lib, dev):
    ratio, groups, lo, hi, bad = O.connectivity_scale_case()
    want = np.array([0 if k in bad else int(O.groups_connected(ratio, g, lo, hi)) for k, g in enumerate(groups)], np.uint8)
    good = [g for k, g in enumerate(groups) if k not in bad]
    clean, status = run_groups(lib, dev, ratio, good, lo, hi)
    print(f"{len(good)} groups: {int(clean.sum())} connected, {np.flatnonzero(clean != np.delete(want, bad)).size} verdicts differ")
    assert status == 0 and np.array_equal(clean, np.delete(want, bad))
    got, status = run_groups(lib, dev, ratio, groups, lo, hi)               # the malformed ones among them: their neighbours are not disturbed
    assert status == 4 and np.array_equal(got, want)
    # the device's own matrix gives the same verdicts as the oracle's: the two are equal as doubles
    dev_ratio, _, _ = run_overlap(lib, dev, O.overlap_scale_case(O.CONN_S))
    again, _ = run_groups(lib, dev, dev_ratio, groups, lo, hi)
    assert np.array_equal(again, got)


# ---- ICP: 300 problems in one call ----------------------------------------------------------------------------------------------------------
TOL = 2e-6
SOLO = (0, 5, 129, 255, 256, 261, 271, 293, 299)          # lattice, surface and shared-target problems on both sides of problem 256


def t(dev, a, dtype=None):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(dev)


def icp_bits(sol, with_xt=True):
    out = [sol.converged.to(torch.uint8), sol.rmse, sol.R, sol.T, sol.iterations] + ([sol.Xt] if with_xt else [])
    return [x.contiguous().cpu().view(torch.uint8).clone() for x in out]


def same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def run_batch300(dev, search, estimation, init):
    b = I.batch300(estimation == "point_to_plane")
    kw = dict(search=search, estimation=estimation)
    if estimation == "point_to_plane":
        kw.update(y_normals=t(dev, PO.batch300_normals()[0]), relative_rmse_thr=PO.BATCH_THR)
    if init:
        kw.update(init_R=t(dev, b["init_R"]), init_T=t(dev, b["init_T"]))
    return rap_amd.icp_packed(t(dev, b["X"]), t(dev, b["x_seg"]), t(dev, b["Y"]), t(dev, b["y_seg"]), **kw)


def check_batch300(sol, ref, stable, what, init):
    """R, T, rmse within TOL of the yardstick and `converged` equal for every compared problem; the iteration count equal for `stable`,
    which has to be 98 % of them"""
    b = I.batch300()                                                  # (the starts are those of both variants)
    R, T, rmse = sol.R.double().cpu().numpy(), sol.T.double().cpu().numpy(), sol.rmse.double().cpu().numpy()
    its, conv = sol.iterations.cpu().numpy(), sol.converged.cpu().numpy().astype(bool)
    compared = [k for k in range(I.BATCH_K) if ref[k] is not None]
    dR = np.array([np.abs(R[k] - ref[k].R).max() for k in compared])
    dT = np.array([np.abs(T[k] - ref[k].T).max() for k in compared])
    dr = np.array([abs(rmse[k] - ref[k].rmse) for k in compared])
    off = [k for k in stable if its[k] != ref[k].iterations]
    print(f"{what}: {len(compared)} problems, worst |dR| {dR.max():.2e} (problem {compared[dR.argmax()]}) |dT| {dT.max():.2e} |drmse| {dr.max():.2e}; "
          f"iteration counts {sorted(set(int(v) for v in its[compared]))}, {len(off)} of {len(stable)} differ from the yardstick's {off[:8]}")
    assert len(compared) >= 0.98 * I.BATCH_K                          # no more than 2 % of the problems are left out
    assert len(stable) >= 0.98 * len(compared) and sum(k >= 256 for k in stable) >= 30      # ... nor of the iteration counts
    assert dR.max() <= TOL and dT.max() <= TOL and dr.max() <= TOL
    assert all(conv[k] == ref[k].converged for k in compared) and not off
    assert max(abs(np.linalg.det(R[k]) - 1.0) for k in compared) < 1e-6
    eye = np.eye(3)
    for k in I.BATCH_EMPTY_X + I.BATCH_EMPTY_Y:                       # the rules for empty problems hold at numbers >= 256: R, T = init or identity
        assert np.isnan(rmse[k]) and its[k] == 0 and not conv[k]
        assert np.array_equal(sol.R[k].cpu().numpy(), b["init_R"][k] if init else np.eye(3, dtype=np.float32)), k
        assert np.array_equal(sol.T[k].cpu().numpy(), b["init_T"][k] if init else np.zeros(3, np.float32)), k
    for k in I.BATCH_ONE_POINT:
        assert np.isfinite(R[k]).all() and np.isfinite(T[k]).all() and np.isfinite(rmse[k]) and np.abs(R[k] @ R[k].T - eye).max() < 1e-6
    return compared


@pytest.mark.parametrize("init", [False, True], ids=["identity", "init_transform"])
def test_point_to_point_batch_of_300_matches_the_yardstick_in_both_searches(dev, init):
    b, ref = I.batch300(), I.batch300_solved(init)
    sol = run_batch300(dev, "brute", "point_to_point", init)
    compared = check_batch300(sol, ref, [k for k in range(I.BATCH_K) if ref[k] is not None], f"point to point, init {init}", init)
    assert same_bits(icp_bits(run_batch300(dev, "grid", "point_to_point", init)), icp_bits(sol))
    if not init:
        Xt = sol.Xt.cpu().numpy()
        covered = np.zeros(b["X"].shape[0], bool)
        for k in compared + list(I.BATCH_ONE_POINT):
            covered[b["x_seg"][k, 0]:b["x_seg"][k, 0] + b["x_seg"][k, 1]] = True
        assert (~covered).sum() > 100 and np.array_equal(Xt[~covered], b["X"][~covered])      # junk rows and the x of an empty-Y problem pass through


@pytest.mark.parametrize("init", [False, True], ids=["identity", "init_transform"])
def test_point_to_plane_batch_of_300_matches_the_yardstick_in_both_searches(dev, init):
    ref = PO.batch300_solved(init)
    sol = run_batch300(dev, "brute", "point_to_plane", init)
    check_batch300(sol, ref, PO.batch300_decided(init), f"point to plane, init {init}", init)
    assert same_bits(icp_bits(run_batch300(dev, "grid", "point_to_plane", init)), icp_bits(sol))


@pytest.mark.parametrize("search", ["brute", "grid"])
@pytest.mark.parametrize("estimation", ["point_to_point", "point_to_plane"])
def test_problems_of_the_batch_of_300_equal_their_solo_runs_bit_for_bit(dev, search, estimation):
    b = I.batch300(estimation == "point_to_plane")
    sol = run_batch300(dev, search, estimation, False)
    per = PO.batch300_normals()[1]
    for k in SOLO:
        X, Y = b["parts"][k]
        kw = dict(Y_normals=t(dev, per[k]), relative_rmse_thr=PO.BATCH_THR) if estimation == "point_to_plane" else {}
        solo = rap_amd.iterative_closest_point(t(dev, X), t(dev, Y), search=search, estimation=estimation, **kw)
        for name in ("R", "T", "rmse", "iterations", "converged"):
            assert torch.equal(getattr(sol, name)[k].cpu().view(-1), getattr(solo, name)[0].cpu().view(-1)), (k, name)
        a = int(b["x_seg"][k, 0])
        assert torch.equal(sol.Xt[a:a + X.shape[0]].cpu(), solo.Xt.cpu()), k


# ---- ICP: one problem of more than 64 items ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", I.BIG_NX)
@pytest.mark.parametrize("estimation", ["point_to_point", "point_to_plane"])
def test_problem_of_more_than_64_items_matches_the_yardstick(dev, estimation, nx):
    plane = estimation == "point_to_plane"
    X, Y, xs, ys, parts = I.big_batch(nx, plane)
    ref = PO.big_solved(nx) if plane else I.big_solved(nx)
    kw = dict(y_normals=t(dev, PO.big_normals(nx)[0]), relative_rmse_thr=PO.BATCH_THR) if plane else {}
    sol = rap_amd.icp_packed(t(dev, X), t(dev, xs), t(dev, Y), t(dev, ys), estimation=estimation, **kw)
    for k in range(3):
        R, T = sol.R[k].double().cpu().numpy(), sol.T[k].double().cpu().numpy()
        dR, dT, dr = np.abs(R - ref[k].R).max(), np.abs(T - ref[k].T).max(), abs(float(sol.rmse[k]) - ref[k].rmse)
        print(f"{estimation}, problem {k} of {X.shape[0]} rows ({xs[k, 1]} x {ys[k, 1]}): |dR| {dR:.2e} |dT| {dT:.2e} |drmse| {dr:.2e}; "
              f"iterations {int(sol.iterations[k])} (yardstick {ref[k].iterations})")
        assert dR <= TOL and dT <= TOL and dr <= TOL and bool(sol.converged[k]) == ref[k].converged and int(sol.iterations[k]) == ref[k].iterations
    grid = rap_amd.icp_packed(t(dev, X), t(dev, xs), t(dev, Y), t(dev, ys), estimation=estimation, search="grid", **kw)
    assert same_bits(icp_bits(grid), icp_bits(sol))
    solo = rap_amd.iterative_closest_point(t(dev, parts[1][0]), t(dev, parts[1][1]), estimation=estimation,
                                           **(dict(Y_normals=t(dev, PO.big_normals(nx)[1][1]), relative_rmse_thr=PO.BATCH_THR) if plane else {}))
    for name in ("R", "T", "rmse", "iterations", "converged"):      # items 1 .. 66 of a batch give what items 0 .. 65 of a solo run give
        assert torch.equal(getattr(sol, name)[1].cpu().view(-1), getattr(solo, name)[0].cpu().view(-1)), name


# ---- normals: 300 segments --------------------------------------------------------------------------------------------------------------------
def normals_deviation(n, e, ref, signed):
    ref_n, ref_e = ref[0], ref[1]
    dn = np.abs(n - ref_n).max(axis=1)
    if not signed:
        dn = np.minimum(dn, np.abs(n + ref_n).max(axis=1))
    return float(dn.max(initial=0.0)), float((np.abs(e - ref_e) / np.maximum(ref_e[:, 2:3], 1e-300)).max(initial=0.0))


@pytest.mark.parametrize("max_nn", PO.NORMALS_MAX_NN)
def test_normals_of_300_segments_match_the_yardstick(dev, max_nn):
    b = PO.normals_batch300()
    seg, K = b["seg"], PO.NORMALS_K
    Pd, sd = t(dev, b["P"]), t(dev, seg)
    run = lambda **kw: [x.cpu() for x in rap_amd.estimate_normals_packed(Pd, sd, max_nn=max_nn, radius=0.0, return_eigenvalues=True, **kw)]
    n0, e0 = run()
    nv, ev = run(viewpoint=t(dev, b["viewpoint"]))
    assert torch.equal(e0.view(torch.int32), ev.view(torch.int32))
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(run(), (n0, e0)))
    worst = [0.0, 0.0, 0.0]
    for k in range(K):
        a, m = int(seg[k, 0]), int(seg[k, 1])
        if m == 0:
            continue
        ref0, refv = PO.normals_batch300_solved(max_nn, False)[k], PO.normals_batch300_solved(max_nn, True)[k]
        dn, de = normals_deviation(n0[a:a + m].double().numpy(), e0[a:a + m].double().numpy(), ref0, signed=False)
        dv, _ = normals_deviation(nv[a:a + m].double().numpy(), ev[a:a + m].double().numpy(), refv, signed=True)      # every sign: the viewpoints keep clear
        worst = [max(worst[0], dn), max(worst[1], de), max(worst[2], dv)]
        assert dn <= TOL and de <= TOL and dv <= TOL, (k, m, dn, de, dv)
        if m < 3:
            assert not n0[a:a + m].any() and not e0[a:a + m].any()
    print(f"max_nn {max_nn}, {K} segments: worst |dn| up to sign {worst[0]:.2e}, |d lambda| / lambda_max {worst[1]:.2e}, towards the viewpoint {worst[2]:.2e}")
    # rows outside every segment are not written: through the C ABI, into buffers that hold a pattern
    lib = _lib.load()
    N = b["P"].shape[0]
    out = torch.full((N, 3), 7.5, dtype=torch.float32, device=dev)
    eig = torch.full((N, 3), -3.25, dtype=torch.float32, device=dev)
    ws = torch.empty(lib.rap_normals_workspace_bytes(N, K), dtype=torch.uint8, device=dev)
    rc = lib.rap_estimate_normals(_lib.ptr(Pd), _lib.ptr(sd), K, N, max_nn, 0.0, None, _lib.ptr(out), _lib.ptr(eig), _lib.ptr(ws), ws.numel(),
                                  _lib.current_stream(dev))
    torch.cuda.synchronize()
    covered = torch.from_numpy(b["covered"])
    out, eig = out.cpu(), eig.cpu()
    assert rc == 0 and (out[~covered] == 7.5).all() and (eig[~covered] == -3.25).all()
    assert torch.equal(out[covered].view(torch.int32), n0[covered].view(torch.int32))
    for k in (1, 100, 255, 256, 258, 264, 296, 299):                  # solo runs, repeats and their originals among them
        a, m = int(seg[k, 0]), int(seg[k, 1])
        sn, se = rap_amd.estimate_normals_packed(t(dev, b["clouds"][k]), t(dev, np.array([[0, m]], np.int32)), max_nn=max_nn, radius=0.0,
                                                 viewpoint=t(dev, b["viewpoint"][k]), return_eigenvalues=True)
        assert torch.equal(sn.cpu().view(torch.int32), nv[a:a + m].view(torch.int32)) and torch.equal(se.cpu().view(torch.int32), ev[a:a + m].view(torch.int32)), k
