"""GPU: the point-to-plane ICP (rap_amd/csrc/icp_plane.hip, the grid path in nn_grid.hip, rap_amd/icp.py) against its fp64 yardstick
(tests/icp_plane_oracle.py).

Bound: R, T and rmse within 2e-6 absolute of the yardstick, the bound of rap_icp (tests/test_icp_gpu.py).  The device searches and forms
the residuals from fp32 moved points and solves in fp64; the yardstick's own run with fp32 moved points stays within 1e-8 of its fp64
run on these inputs, and no neighbour or gate decision comes within 1e-5 of flipping (tests/test_icp_plane_host.py), so iteration
counts are compared exactly.  Every parity test prints its worst deviation before it asserts (run with -s to see them)."""
import numpy as np
import pytest
import torch

import icp_oracle as O
import icp_plane_oracle as P
import rap_amd

pytestmark = pytest.mark.gpu

TOL = 2e-6
PLANE = dict(estimation="point_to_plane")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def t(dev, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def solve(dev, X, Y, Yn, **kw):
    return rap_amd.iterative_closest_point(t(dev, X), t(dev, Y), Y_normals=t(dev, Yn), **PLANE, **kw)


def assert_parity(sol, ref, what, k=0):
    R, T = sol.R[k].double().cpu().numpy(), sol.T[k].double().cpu().numpy()
    dR, dT, dr = np.abs(R - ref.R).max(), np.abs(T - ref.T).max(), abs(float(sol.rmse[k]) - ref.rmse)
    print(f"{what}: |dR| {dR:.2e} |dT| {dT:.2e} |drmse| {dr:.2e}; iterations {int(sol.iterations[k])} (yardstick {ref.iterations})")
    assert dR <= TOL and dT <= TOL and dr <= TOL, (what, dR, dT, dr)
    assert abs(np.linalg.det(R) - 1.0) < 1e-6
    assert int(sol.iterations[k]) == ref.iterations and bool(sol.converged[k]) == ref.converged


def bits(sol):
    return [x.contiguous().cpu().view(torch.uint8).clone() for x in (sol.converged.to(torch.uint8), sol.rmse, sol.Xt, sol.R, sol.T, sol.iterations)]


def same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# 1. parity with the yardstick, both searches ---------------------------------------------------------
@pytest.mark.parametrize("seed,nx,ny", P.PLANE_PAIRS)
def test_margin_checked_pairs_match_the_yardstick_and_grid_equals_brute(dev, seed, nx, ny):
    X, Y, Yn = P.pair(seed, nx, ny)
    ref = P.solved(seed, nx, ny)
    sol = solve(dev, X, Y, Yn)
    assert_parity(sol, ref, f"seed {seed} {nx} x {ny}")
    Xt = sol.Xt.double().cpu().numpy()
    assert Xt.shape == X.shape and np.abs(Xt - ref.Xt).max() <= TOL * (np.abs(X).sum(axis=1).max() + 1.0) + 4e-7      # |x|_1 |dR| + |dT| + fp32 rounding
    grid = solve(dev, X, Y, Yn, search="grid")
    assert same_bits(bits(grid), bits(sol))
    for limit in (1, 2):                                              # the update of the last iteration is applied; rmse is one update behind
        lim = solve(dev, X, Y, Yn, max_iterations=limit)
        assert_parity(lim, P.solved(seed, nx, ny, max_iterations=limit), f"seed {seed} limit {limit}")
        assert not bool(lim.converged[0])
    one, two = P.solved(seed, nx, ny, max_iterations=1), P.solved(seed, nx, ny, max_iterations=2)
    assert np.abs(one.R - np.eye(3)).max() > 1e-3 and two.rmse < 0.5 * one.rmse


def test_gated_partial_overlap_matches_the_gated_yardstick(dev):
    g = P.GATE_CASE
    X, Y, Yn = P.pair(g["seed"], g["nx"], g["ny"], g["x_range"], g["y_range"])
    ref = P.solved(g["seed"], g["nx"], g["ny"], x_range=g["x_range"], y_range=g["y_range"], gate=P.GATE, margins=True)
    assert ref.gate_margin >= 2e-5 and 0 < ref.count < g["nx"]      # asserted on the host side of this test too
    sol = solve(dev, X, Y, Yn, max_correspondence_distance=P.GATE)
    assert_parity(sol, ref, "gated 256 x 256")
    assert same_bits(bits(solve(dev, X, Y, Yn, max_correspondence_distance=P.GATE, search="grid")), bits(sol))
    none = solve(dev, X, Y, Yn, max_correspondence_distance=1e-5)      # a gate below every distance
    assert torch.isinf(none.rmse[0]) and float(none.rmse[0]) > 0 and not bool(none.converged[0]) and int(none.iterations[0]) == 0
    assert torch.equal(none.R[0].cpu(), torch.eye(3)) and not none.T[0].cpu().any()


# 2. ragged batch -----------------------------------------------------------------------------------------
def ragged(dev):
    (sa, na, ma), (sb, nb, mb) = P.PLANE_PAIRS
    Xa, Ya, Na = P.pair(sa, na, ma)
    Xb, Yb, Nb = P.pair(sb, nb, mb)
    rng = np.random.default_rng(11)
    junk = lambda n: rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    # X: [junk 5 | B | junk 3 | one point | A | two points | junk 40 (the "x" of the empty-Y problem)], Y likewise out of order
    X = np.concatenate([junk(5), Xb, junk(3), Xa[:1], Xa, Xa[5:7], junk(40)])
    Y = np.concatenate([Ya, junk(7), Yb, junk(9)])
    Yn = np.concatenate([Na, junk(7), Nb, junk(9)])
    xb = 5
    x1 = xb + nb + 3
    xa = x1 + 1
    x2 = xa + na
    xe = x2 + 2
    ya, yb = 0, ma + 7
    #            empty X      real A        1 point      empty Y      real B        2 points
    x_seg = [[17, 0],     [xa, na],     [x1, 1],     [xe, 40],    [xb, nb],     [x2, 2]]
    y_seg = [[ya, ma],    [ya, ma],     [yb, mb],    [40, -3],    [yb, mb],     [ya, ma]]
    seg = lambda rows: torch.tensor(rows, dtype=torch.int32, device=dev)
    return X, Y, Yn, seg(x_seg), seg(y_seg), ((1, Xa, Ya, Na, xa), (4, Xb, Yb, Nb, xb)), ((0, 5), (xb + nb, xb + nb + 3), (xe, xe + 40))


@pytest.mark.parametrize("search", ["brute", "grid"])
def test_ragged_batch_is_bit_identical_to_solo_runs(dev, search):
    X, Y, Yn, xs, ys, real, untouched = ragged(dev)
    sol = rap_amd.icp_packed(t(dev, X), xs, t(dev, Y), ys, y_normals=t(dev, Yn), search=search, **PLANE)
    for k, Xs, Ys, Ns, start in real:
        solo = solve(dev, Xs, Ys, Ns, search=search)
        for name in ("R", "T", "rmse", "iterations", "converged"):
            assert torch.equal(getattr(sol, name)[k].cpu().view(-1), getattr(solo, name)[0].cpu().view(-1)), (k, name)
        assert torch.equal(sol.Xt[start:start + Xs.shape[0]].cpu(), solo.Xt.cpu()), k
        assert bool(sol.converged[k])
    eye = torch.eye(3)
    for k in (0, 3):                                               # an empty X, an empty Y
        assert torch.equal(sol.R[k].cpu(), eye) and not sol.T[k].cpu().any()
        assert torch.isnan(sol.rmse[k]) and int(sol.iterations[k]) == 0 and not bool(sol.converged[k])
    for k in (2, 5):                                               # one point, two points: rank-deficient steps, a finite proper rotation
        R = sol.R[k].double().cpu().numpy()
        assert np.isfinite(R).all() and np.isfinite(sol.T[k].cpu().numpy()).all() and np.isfinite(float(sol.rmse[k]))
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(R) - 1.0) < 1e-6
    Xt = sol.Xt.cpu().numpy()
    for a, b in untouched:                                         # rows outside every segment and the rows of the empty-Y problem
        assert np.array_equal(Xt[a:b], X[a:b])


# 3. degenerate targets and unusable normals -----------------------------------------------------------------
def test_coplanar_target_takes_no_step_along_the_unobservable_motion(dev):
    X, Y, Yn = P.coplanar_case()
    sol = solve(dev, X, Y, Yn)
    R = sol.R[0].double().cpu().numpy()
    print(f"coplanar: iterations {int(sol.iterations[0])}, rmse {float(sol.rmse[0]):.2e}, tilt {np.abs(R[2, :2]).max():.2e}")
    assert np.isfinite(R).all() and np.abs(R @ R.T - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(R) - 1.0) < 1e-6
    assert bool(sol.converged[0]) and float(sol.rmse[0]) < 1e-5 and np.abs(R[2, :2]).max() > 1e-3
    one = solve(dev, X, Y, Yn, max_iterations=1)                    # a single step: no rotation about the normal, no translation in the plane
    R1, T1 = one.R[0].double().cpu().numpy(), one.T[0].double().cpu().numpy()
    print(f"coplanar, one step: |R01 - R10| {abs(R1[0, 1] - R1[1, 0]):.2e}, in-plane |T| {np.abs(T1[:2]).max():.2e}, lift {T1[2]:.2e}")
    assert abs(R1[0, 1] - R1[1, 0]) <= 1.2e-7 and np.abs(T1[:2]).max() <= 1e-9 and abs(T1[2]) > 1e-3      # one fp32 rounding of entries < 1
    ref = P.icp_plane(X, Y, Yn, max_iterations=1)
    assert np.abs(R1 - ref.R).max() <= TOL and np.abs(T1 - ref.T).max() <= TOL


def test_zero_and_nan_normals_are_left_out_and_an_all_zero_problem_reports_inf(dev):
    seed, nx, ny = P.PLANE_PAIRS[0]
    X, Y, Yn = P.pair(seed, nx, ny)
    bad = Yn.copy()
    bad[::3] = 0.0
    bad[1::3, 1] = np.nan
    ref = P.icp_plane(X, Y, bad, max_iterations=1)
    assert 0 < ref.count < nx
    sol = solve(dev, X, Y, bad, max_iterations=1)
    R, T = sol.R[0].double().cpu().numpy(), sol.T[0].double().cpu().numpy()
    print(f"{ref.count} of {nx} pairs usable: |dR| {np.abs(R - ref.R).max():.2e} |dT| {np.abs(T - ref.T).max():.2e} "
          f"|drmse| {abs(float(sol.rmse[0]) - ref.rmse):.2e}")
    # the rmse is the root MEAN over the counted pairs: a wrong count would show in it at once
    assert np.abs(R - ref.R).max() <= TOL and np.abs(T - ref.T).max() <= TOL and abs(float(sol.rmse[0]) - ref.rmse) <= TOL
    full = P.solved(seed, nx, ny, max_iterations=1)
    assert abs(full.rmse - ref.rmse) > 100 * TOL or np.abs(full.R - ref.R).max() > 100 * TOL
    for search in ("brute", "grid"):
        none = solve(dev, X, Y, np.zeros_like(Yn), search=search)
        assert torch.isinf(none.rmse[0]) and float(none.rmse[0]) > 0 and not bool(none.converged[0]) and int(none.iterations[0]) == 0
        assert torch.equal(none.R[0].cpu(), torch.eye(3)) and not none.T[0].cpu().any()
        assert torch.equal(none.Xt.cpu(), torch.from_numpy(X))


# 4. normals estimated in the same call ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed,nx,ny", P.ESTIMATED_PAIRS)
def test_missing_normals_are_estimated_in_the_call(dev, seed, nx, ny):
    X, Y, _ = P.pair(seed, nx, ny)
    ref = P.solved(seed, nx, ny, estimated=True)
    sol = solve(dev, X, Y, None)
    assert_parity(sol, ref, f"seed {seed}, estimated normals")
    assert same_bits(bits(solve(dev, X, Y, None, search="grid")), bits(sol))
    given = solve(dev, X, Y, rap_amd.estimate_point_normals(t(dev, Y), k_neighbors=20, radius=0.0).cpu().numpy())
    assert same_bits(bits(given), bits(sol))


# 5. execution properties -----------------------------------------------------------------------------------------
def batch_call(dev, search="brute", normals=True):
    X, Y, Yn, xs, ys, _, _ = ragged(dev)
    Xd, Yd, Nd = t(dev, X), t(dev, Y), t(dev, Yn) if normals else None
    return lambda: rap_amd.icp_packed(Xd, xs, Yd, ys, y_normals=Nd, max_correspondence_distance=0.2, search=search, **PLANE)


@pytest.mark.parametrize("search", ["brute", "grid"])
def test_two_calls_are_bitwise_equal_without_a_host_synchronisation_and_replay_from_a_graph(dev, search):
    for normals in (True, False):
        call = batch_call(dev, search, normals)
        want = bits(call())                                          # (also sizes the workspace: growing it is an allocation, not a sync)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            sol = call()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert same_bits(bits(sol), want)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):                                # one capture stream: the call's launches form a single chain
            sol = call()
        for _ in range(2):
            for x in (sol.rmse, sol.R, sol.T, sol.Xt):
                x.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            assert same_bits(bits(sol), want)


def test_point_to_point_is_unchanged_by_the_new_argument(dev):
    X, Y = O.pair(O.SINGLE_SEED, 300, 257)
    Xd, Yd = t(dev, X), t(dev, Y)
    for search in ("brute", "grid"):
        a = rap_amd.iterative_closest_point(Xd, Yd, search=search)
        b = rap_amd.iterative_closest_point(Xd, Yd, search=search, estimation="point_to_point")
        assert same_bits(bits(a), bits(b))
    ref = O.solved(O.SINGLE_SEED, 300, 257)
    assert np.abs(a.R[0].double().cpu().numpy() - ref.R).max() <= TOL and int(a.iterations[0]) > P.solved(*P.PLANE_PAIRS[0]).iterations
