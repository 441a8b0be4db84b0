"""CPU: the point-to-plane ICP's entry points refuse bad arguments before anything touches the device, their workspace queries are host
arithmetic, and the inputs the GPU tests (tests/test_icp_plane_gpu.py) hold the kernels to are fit for it -- margins measured from the
yardstick (tests/icp_plane_oracle.py), not from the code under test."""
import ctypes

import numpy as np
import pytest
import torch

import icp_oracle as O
import icp_plane_oracle as P
from rap_amd import _lib

N, ONE = ctypes.c_void_p(0), ctypes.c_void_p(256)      # NULL; a non-NULL sentinel -- every call below fails before a pointer is used


def call(lib, grid=False, **kw):
    a = dict(X=ONE, xs=ONE, Y=ONE, ys=ONE, Yn=ONE, K=2, NX=1000, NY=900, iR=N, iT=N, it=10, thr=1e-6, gate=0.0, R=ONE, T=ONE, rmse=ONE,
             iters=ONE, conv=ONE, Xt=N, ws=ONE, wsb=1 << 30)
    a.update(kw)
    fn = lib.rap_icp_plane_grid if grid else lib.rap_icp_plane
    return fn(a["X"], a["xs"], a["Y"], a["ys"], a["Yn"], a["K"], a["NX"], a["NY"], a["iR"], a["iT"], a["it"], a["thr"], a["gate"], a["R"],
              a["T"], a["rmse"], a["iters"], a["conv"], a["Xt"], a["ws"], a["wsb"], N)


@pytest.mark.parametrize("grid", [False, True], ids=["brute", "grid"])
def test_rap_icp_plane_refuses_bad_arguments_without_a_gpu(grid):
    lib = _lib.load()
    for name in ("X", "xs", "Y", "ys", "Yn", "R", "T", "rmse", "iters", "conv"):
        assert call(lib, grid, **{name: N}) == -1, name
    assert call(lib, grid, K=0) == -1 and call(lib, grid, K=-3) == -1
    assert call(lib, grid, it=0) == -1 and call(lib, grid, it=-1) == -1
    assert call(lib, grid, NX=0) == -1 and call(lib, grid, NY=0) == -1 and call(lib, grid, NX=1 << 31) == -1 and call(lib, grid, NY=1 << 31) == -1
    assert call(lib, grid, thr=float("nan")) == -1 and call(lib, grid, gate=float("nan")) == -1
    if grid:
        assert call(lib, grid, K=65536) == -1
    need = lib.rap_icp_plane_grid_workspace_bytes(1000, 900, 2) if grid else lib.rap_icp_plane_workspace_bytes(1000, 2)
    assert call(lib, grid, ws=N) == -2 and call(lib, grid, wsb=need - 1) == -2 and call(lib, grid, wsb=0) == -2


def test_icp_plane_workspace_queries_are_host_arithmetic():
    lib = _lib.load()
    q, qg = lib.rap_icp_plane_workspace_bytes, lib.rap_icp_plane_grid_workspace_bytes
    assert q(0, 4) == 0 and q(-1, 4) == 0 and q(1000, 0) == 0 and q(1000, -2) == 0
    assert qg(0, 5, 1) == 0 and qg(5, 0, 1) == 0 and qg(5, 5, 0) == 0
    up = lambda n: -(-n // 256) * 256
    for n, K in ((1, 1), (256, 1), (1000, 6), (100_000, 1), (131072, 32)):
        items = n // 256 + K + 1
        # work items (32 bytes), one partial of 28 fp64 moments + a count per item, and per problem: item range, previous rmse, done flag,
        # the fp64 pose (12 doubles)
        assert q(n, K) == up(items * 32) + up(items * 232) + up(K * 16) + up(K * 8) + up(K * 4) + up(K * 96), (n, K)
        # the grid's scratch is what it is for rap_icp_grid
        assert qg(n, 777, K) - q(n, K) == lib.rap_icp_grid_workspace_bytes(n, 777, K) - lib.rap_icp_workspace_bytes(n, K)
    assert q(1 << 40, 1) > 1 << 39


def test_python_entry_points_refuse_cpu_tensors_and_unknown_estimations():
    import rap_amd
    X, Y = torch.zeros(8, 3), torch.zeros(9, 3)
    with pytest.raises(ValueError):
        rap_amd.iterative_closest_point(X, Y, estimation="plane")
    with pytest.raises(ValueError):
        rap_amd.icp_packed(X, torch.tensor([[0, 8]]), Y, torch.tensor([[0, 9]]), estimation="point-to-plane")
    with pytest.raises(_lib.RapError):
        rap_amd.iterative_closest_point(X, Y, estimation="point_to_plane")
    with pytest.raises(ValueError):
        rap_amd.iterative_closest_point(X, Y, Y_normals=Y)             # normals without the estimator that reads them


@pytest.mark.parametrize("seed,nx,ny", P.PLANE_PAIRS)
def test_margin_checked_pairs_keep_a_neighbour_margin_and_a_well_conditioned_step(seed, nx, ny):
    r = P.solved(seed, nx, ny, margins=True)
    print(f"seed {seed}: smallest nearest / second-nearest gap {r.nn_margin:.2e} over {r.iterations} iterations, "
          f"smallest lambda_min / lambda_max {r.cond:.2e}")
    assert r.converged and r.nn_margin >= 1e-5
    assert r.cond > 1e-6                                                 # nowhere near the 1e-12 cut of the pseudo-inverse
    assert P.solved(seed, nx, ny, f32=True).iterations == r.iterations


@pytest.mark.parametrize("seed,nx,ny", P.PLANE_PAIRS)
def test_fp32_search_run_of_the_yardstick_stays_within_1e_7_of_its_fp64_run(seed, nx, ny):
    a, b = P.solved(seed, nx, ny), P.solved(seed, nx, ny, f32=True)
    dR, dT, dr = np.abs(a.R - b.R).max(), np.abs(a.T - b.T).max(), abs(a.rmse - b.rmse)
    print(f"fp32 vs fp64 moved points: |dR| {dR:.2e} |dT| {dT:.2e} |drmse| {dr:.2e}")
    assert dR < 1e-7 and dT < 1e-7 and dr < 1e-7


@pytest.mark.parametrize("seed,nx,ny", P.PLANE_PAIRS)
def test_plane_beats_point_to_point_in_iterations_and_pose_error(seed, nx, ny):
    plane, point = P.solved(seed, nx, ny), O.solved(seed, nx, ny)
    e_plane, e_point = np.abs(plane.R - O.R0).max(), np.abs(point.R - O.R0).max()
    print(f"seed {seed}: plane {plane.iterations} iterations, |R - R0| {e_plane:.2e}; point {point.iterations} iterations, |R - R0| {e_point:.2e}")
    assert plane.iterations < point.iterations and e_plane < e_point


def test_gated_input_keeps_a_gate_margin():
    g = P.GATE_CASE
    r = P.solved(g["seed"], g["nx"], g["ny"], x_range=g["x_range"], y_range=g["y_range"], gate=P.GATE, margins=True)
    free = P.solved(g["seed"], g["nx"], g["ny"], x_range=g["x_range"], y_range=g["y_range"])
    print(f"smallest |nearest distance - gate| {r.gate_margin:.2e}, neighbour gap {r.nn_margin:.2e} over {r.iterations} iterations; "
          f"{r.count} of {g['nx']} pairs inside the gate")
    assert r.converged and r.gate_margin >= 2e-5 and r.nn_margin >= 1e-5
    assert 0 < r.count < g["nx"] and np.abs(free.R - r.R).max() > 1e-3      # the gate matters on this pair
    assert P.solved(g["seed"], g["nx"], g["ny"], x_range=g["x_range"], y_range=g["y_range"], gate=P.GATE, f32=True).iterations == r.iterations


@pytest.mark.parametrize("seed,nx,ny", P.ESTIMATED_PAIRS)
def test_estimated_normals_run_keeps_its_margins(seed, nx, ny):
    X, Y, Yn = P.pair(seed, nx, ny)
    _, eig, counts, gap = P.estimate_normals(Y, 20, 0.0)
    sep = ((eig[:, 1] - eig[:, 0]) / eig[:, 2]).min()
    r = P.solved(seed, nx, ny, estimated=True, margins=True)
    print(f"seed {seed}: normals' neighbour gap {gap.min():.2e}, (l1 - l0) / l2 {sep:.3f}; ICP neighbour gap {r.nn_margin:.2e}, "
          f"{r.iterations} iterations")
    assert (counts == 20).all() and r.converged
    assert gap.min() >= 1e-5 and sep >= 0.05 and r.nn_margin >= 1e-5


def test_yardstick_rules_for_empty_unusable_and_coplanar_targets():
    X, Y, Yn = P.pair(3, 256, 256)
    for r in (P.icp_plane(X[:0], Y, Yn), P.icp_plane(X, Y[:0], Yn[:0])):
        assert np.isnan(r.rmse) and r.iterations == 0 and not r.converged and np.array_equal(r.R, np.eye(3)) and not r.T.any()
    none = P.icp_plane(X, Y, np.zeros_like(Yn))
    assert np.isinf(none.rmse) and not none.converged and none.iterations == 0 and np.array_equal(none.R, np.eye(3))
    bad = Yn.copy()
    bad[::3] = 0.0
    bad[1::3, 1] = np.nan
    part = P.icp_plane(X, Y, bad, max_iterations=1)
    assert 0 < part.count < X.shape[0]
    Xp, Yp, Np = P.coplanar_case()
    flat = P.icp_plane(Xp, Yp, Np)
    assert flat.converged and np.abs(flat.R[2, :2]).max() > 1e-3 and flat.rmse < 1e-6      # the tilt is found
    # one step moves along nothing the data do not observe: no rotation about z (R - R^T has no z part), no translation in the plane
    # (over several steps T dR^T turns the lift into the plane at second order, so the rule is a statement about a step)
    one = P.icp_plane(Xp, Yp, Np, max_iterations=1)
    assert abs(one.R[0, 1] - one.R[1, 0]) < 1e-12 and np.abs(one.T[:2]).max() < 1e-12 and abs(one.T[2]) > 1e-3
    lim = P.icp_plane(X, Y, Yn, max_iterations=1)
    assert lim.iterations == 1 and not lim.converged


# ---- the inputs at table scale (tests/test_table_scale_gpu.py) ---------------------------------------------------------------------------
@pytest.mark.parametrize("init", [False, True], ids=["identity", "init_transform"])
def test_batch_of_300_with_normals_keeps_its_margins_and_every_count_is_decided(init):
    b, p2p, (Yn, per) = O.batch300(True), O.batch300(), P.batch300_normals()
    ref, f32 = P.batch300_solved(init), P.batch300_solved(init, f32=True)
    compared = [k for k in range(O.BATCH_K) if ref[k] is not None]
    assert Yn.shape == b["Y"].shape and len(compared) == O.BATCH_K - 6
    # the variant differs from the point-to-point batch in the points alone: the same kinds, the same starts, lattices of the same sizes
    assert b["kinds"] == p2p["kinds"] and np.array_equal(b["init_R"], p2p["init_R"]) and np.array_equal(b["init_T"], p2p["init_T"])
    assert all(b["x_seg"][k, 1] == p2p["x_seg"][k, 1] for k in compared if b["kinds"][k] != "surface")
    assert set(O.BATCH_PLANE_SURFACES) == set(O.BATCH_SURFACES) and len(O.BATCH_PLANE_STEPS) == O.BATCH_K
    for k in compared:
        a, n = b["y_seg"][k]
        assert np.array_equal(Yn[a:a + n], per[k]) and np.abs(np.linalg.norm(per[k], axis=1) - 1.0).max() < 1e-6
    margin, cond = min(ref[k].nn_margin for k in compared), min(ref[k].cond for k in compared)
    counts = sorted({ref[k].iterations for k in compared})
    print(f"{len(compared)} problems: smallest neighbour gap {margin:.2e} (required {O.BATCH_MARGIN:.0e}), smallest lambda_min / lambda_max {cond:.2e}, "
          f"iteration counts {counts}, smallest final rmse {min(ref[k].rmse for k in compared):.1e}")
    assert margin >= O.BATCH_MARGIN and cond > 1e-6 and all(ref[k].converged and f32[k].converged for k in compared)
    worst = max(max(np.abs(f32[k].R - ref[k].R).max(), np.abs(f32[k].T - ref[k].T).max(), abs(f32[k].rmse - ref[k].rmse)) for k in compared)
    print(f"fp32 moved points vs fp64: worst deviation {worst:.2e}")
    assert worst < 1e-7
    # the iteration count of a problem is compared where no rounding decides it (icp_plane_oracle.BATCH_THR): that has to be (all but) all
    decided = P.batch300_decided(init)
    moved = max(abs(x - y) for k in decided for x, y in zip(ref[k].rels, f32[k].rels))      # what the fp32 moved points make of a relative decrease
    print(f"{len(decided)} of {len(compared)} problems have a decided count, iterations {sorted({ref[k].iterations for k in decided})}, "
          f"{sum(k >= 256 for k in decided)} of them at numbers >= 256; fp32 moved points move a relative decrease by up to "
          f"{moved:.1e} (threshold {P.BATCH_THR:.0e})")
    assert len(decided) >= 0.98 * len(compared) and sum(k >= 256 for k in decided) >= 30
    assert len({ref[k].iterations for k in decided}) >= 3 and len({ref[k].iterations for k in decided if k >= 256}) >= 2
    assert moved < P.BATCH_THR / 100                                  # a factor of 10 from the threshold is far out of its reach


@pytest.mark.parametrize("nx", O.BIG_NX)
def test_big_problem_with_normals_keeps_its_margin_and_decided_counts(nx):
    ref, f32 = P.big_solved(nx), P.big_solved(nx, f32=True)
    print(f"{nx}: gap {ref[1].nn_margin:.2e}, iterations {[r.iterations for r in ref]}, rmse {ref[1].rmse:.2e}, lambda_min / lambda_max {ref[1].cond:.2e}")
    assert all(r.converged and r.nn_margin >= O.BATCH_MARGIN and r.cond > 1e-6 for r in ref)
    assert all(P.decided(r, f) for r, f in zip(ref, f32)) and ref[1].rmse > 1e-3      # the two small neighbours too: they carry a residual
    assert max(np.abs(f32[1].R - ref[1].R).max(), np.abs(f32[1].T - ref[1].T).max(), abs(f32[1].rmse - ref[1].rmse)) < 1e-7
