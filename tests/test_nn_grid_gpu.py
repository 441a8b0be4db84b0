"""GPU: the grid neighbour search (rap_amd/csrc/nn_grid.hip) against the brute-force search it stands in for.

The contract is equality of bits: ``search="grid"`` must return what ``search="brute"`` returns -- R, T, rmse, iterations, converged and
Xt -- on the inputs of tests/test_icp_gpu.py and on the shapes where a grid can go wrong; and ``nearest_neighbors_packed`` must return
numpy's first arg-min on a lattice whose distances are exact in fp32 and tie across cells (tests/nn_grid_cases.py).  Where the fp64
yardstick of tests/icp_oracle.py exists the grid run is also held to the 2e-6 the brute-force run is held to, and prints its deviation."""
import numpy as np
import pytest
import torch

import icp_oracle as O
import nn_grid_cases as C
import rap_amd
from test_icp_gpu import assert_parity, bits, init_tensors, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def t(a, dev, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(dev)


def both(dev, X, Y, **kw):
    """-> (grid solution, brute solution) of one problem, asserted equal in every bit"""
    Xd, Yd = t(X, dev), t(Y, dev)
    brute = rap_amd.iterative_closest_point(Xd, Yd, search="brute", **kw)
    grid = rap_amd.iterative_closest_point(Xd, Yd, search="grid", **kw)
    assert same_bits(bits(grid), bits(brute)), [n for n, a, b in zip(("converged", "rmse", "Xt", "R", "T", "iterations"), bits(grid), bits(brute))
                                                 if not torch.equal(a, b)]
    return grid, brute


def both_packed(dev, X, xs, Y, ys, **kw):
    Xd, Yd = t(X, dev), t(Y, dev)
    xs, ys = t(xs, dev, torch.int32), t(ys, dev, torch.int32)
    brute = rap_amd.icp_packed(Xd, xs, Yd, ys, search="brute", **kw)
    grid = rap_amd.icp_packed(Xd, xs, Yd, ys, search="grid", **kw)
    assert same_bits(bits(grid), bits(brute)), [n for n, a, b in zip(("converged", "rmse", "Xt", "R", "T", "iterations"), bits(grid), bits(brute))
                                                 if not torch.equal(a, b)]
    return grid, brute


def nearest(dev, X, Y, **kw):
    xs = torch.tensor([[0, X.shape[0]]], dtype=torch.int32, device=dev)
    ys = torch.tensor([[0, Y.shape[0]]], dtype=torch.int32, device=dev)
    idx, d2 = rap_amd.nearest_neighbors_packed(t(X, dev), xs, t(Y, dev), ys, **kw)
    return idx.cpu().numpy(), d2.cpu().numpy()


# 1. ties across cells --------------------------------------------------------------------------------
def test_lattice_ties_resolve_to_the_first_arg_min_with_exact_distances(dev):
    Y, X, kind = C.lattice()
    want_i, want_d, _ = C.first_argmin(X, Y)
    idx, d2 = nearest(dev, X, Y)
    assert np.array_equal(idx, want_i), (kind[idx != want_i], np.flatnonzero(idx != want_i)[:8])
    assert np.array_equal(d2, want_d)
    for gate in (np.nextafter(C.HALF, np.float32(0)), np.nextafter(C.HALF, np.float32(1))):      # just below / above half a spacing
        gi, gd = C.gated(want_i, want_d, gate)
        idx, d2 = nearest(dev, X, Y, max_distance=float(gate))
        assert np.array_equal(idx, gi) and np.array_equal(d2, gd), float(gate)
        assert (gi[kind == "edge"] >= 0).all() == (gate > C.HALF) and (gi[kind == "point"] >= 0).all() and (gi[kind == "face"] < 0).all()
    # R, T on load: a quarter turn about z and a shift by eighths are exact in fp32, so X' R + T == X bit for bit
    R = np.array([[0, 1, 0], [-1, 0, 0], [0, 0, 1]], np.float32)
    T = np.array([0.375, -1.125, 0.25], np.float32)
    Xp = (X - T) @ R.T
    assert np.array_equal(Xp @ R + T, X)
    idx, d2 = nearest(dev, Xp, Y, R=t(R[None], dev), T=t(T[None], dev))
    assert np.array_equal(idx, want_i) and np.array_equal(d2, want_d)


# 2. ICP, bit for bit, on the inputs of the existing suite -------------------------------------------
@pytest.mark.parametrize("nx,ny", O.SINGLE_SIZES)
def test_single_problems_are_bit_identical_and_within_the_yardstick_bound(dev, nx, ny):
    X, Y = O.pair(O.SINGLE_SEED, nx, ny)
    grid, _ = both(dev, X, Y)
    assert_parity(grid, O.solved(O.SINGLE_SEED, nx, ny), f"grid {nx} x {ny}")
    assert bool(grid.converged[0])


@pytest.mark.parametrize("seed,nx,ny", O.EXACT_COUNT)
def test_exact_count_inputs_are_bit_identical(dev, seed, nx, ny):
    X, Y = O.pair(seed, nx, ny)
    ref = O.solved(seed, nx, ny)
    grid, _ = both(dev, X, Y)
    assert_parity(grid, ref, f"grid seed {seed} {nx} x {ny}")
    assert int(grid.iterations[0]) == ref.iterations and bool(grid.converged[0])


def ragged_batch():
    """the batch of six of tests/test_icp_gpu.py: empty X, real A, one point, empty Y, real B, two points; segments neither contiguous
    nor ordered"""
    Xa, Ya = O.pair(O.SINGLE_SEED, 300, 257)
    Xb, Yb = O.pair(O.SINGLE_SEED, 513, 1000)
    rng = np.random.default_rng(11)
    junk = lambda n: rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    X = np.concatenate([junk(5), Xb, junk(3), Xa[:1], Xa, Xa[5:7], junk(40)])
    Y = np.concatenate([Ya, junk(7), Yb, junk(9)])
    xa, xb, x1, x2, xe = 5 + 513 + 3 + 1, 5, 5 + 513 + 3, 5 + 513 + 3 + 1 + 300, 5 + 513 + 3 + 1 + 300 + 2
    ya, yb = 0, 257 + 7
    x_seg = np.array([[17, 0], [xa, 300], [x1, 1], [xe, 40], [xb, 513], [x2, 2]], np.int32)
    y_seg = np.array([[ya, 257], [ya, 257], [yb, 1000], [40, -3], [yb, 1000], [ya, 257]], np.int32)
    return X, x_seg, Y, y_seg, ((1, Xa, Ya, xa), (4, Xb, Yb, xb))


def test_ragged_batch_is_bit_identical_and_a_problem_gives_the_same_bits_alone(dev):
    X, x_seg, Y, y_seg, real = ragged_batch()
    grid, _ = both_packed(dev, X, x_seg, Y, y_seg)
    for k, Xs, Ys, xs in real:
        solo = rap_amd.iterative_closest_point(t(Xs, dev), t(Ys, dev), search="grid")
        for name in ("R", "T", "rmse", "iterations", "converged"):
            assert torch.equal(getattr(grid, name)[k].cpu().view(-1), getattr(solo, name)[0].cpu().view(-1)), (k, name)
        assert torch.equal(grid.Xt[xs:xs + Xs.shape[0]].cpu(), solo.Xt.cpu()), k
        assert bool(grid.converged[k])
    for k in (0, 3):                                                 # an empty X, an empty Y
        assert torch.isnan(grid.rmse[k]) and int(grid.iterations[k]) == 0 and not bool(grid.converged[k])
    assert_parity(grid, O.solved(O.SINGLE_SEED, 300, 257), "grid, ragged batch, problem A", k=1)
    assert_parity(grid, O.solved(O.SINGLE_SEED, 513, 1000), "grid, ragged batch, problem B", k=4)


def test_init_transform_is_bit_identical(dev):
    X, Y = O.pair(O.SINGLE_SEED, 513, 1000)
    grid, _ = both(dev, X, Y, init_transform=init_tensors(dev))
    assert_parity(grid, O.solved(O.SINGLE_SEED, 513, 1000, init=True), "grid 513 x 1000 with init_transform")
    one, _ = both(dev, X, Y, init_transform=init_tensors(dev), max_iterations=1)
    assert_parity(one, O.solved(O.SINGLE_SEED, 513, 1000, init=True, max_iterations=1), "grid, one iteration from init_transform")


def test_gated_partial_overlap_and_an_empty_gate_are_bit_identical(dev):
    g = O.GATE_CASE
    X, Y = O.pair(g["seed"], g["nx"], g["ny"], g["x_range"], g["y_range"])
    grid, _ = both(dev, X, Y, max_correspondence_distance=O.GATE)
    assert_parity(grid, O.solved(g["seed"], g["nx"], g["ny"], x_range=g["x_range"], y_range=g["y_range"], gate=O.GATE), "grid gated 700 x 900")
    assert bool(grid.converged[0])
    none, _ = both(dev, X, Y, max_correspondence_distance=1e-4)      # a gate below every distance: rmse inf, nothing moved
    assert torch.isinf(none.rmse[0]) and float(none.rmse[0]) > 0 and not bool(none.converged[0]) and int(none.iterations[0]) == 0
    assert torch.equal(none.Xt.cpu(), torch.from_numpy(X))


@pytest.mark.parametrize("limit", [1, 5])
def test_iteration_limits_are_bit_identical(dev, limit):
    seed, nx, ny = O.EXACT_COUNT[0]
    X, Y = O.pair(seed, nx, ny)
    grid, _ = both(dev, X, Y, max_iterations=limit)
    assert int(grid.iterations[0]) == limit and not bool(grid.converged[0])
    assert_parity(grid, O.solved(seed, nx, ny, max_iterations=limit), f"grid limit {limit}")


# 3. shapes where a grid goes wrong ----------------------------------------------------------------------
@pytest.mark.parametrize("ny", [1, 2, 1000, 4099])
@pytest.mark.parametrize("nx", [1, 255, 256, 257])
def test_item_and_cell_edges_are_bit_identical(dev, nx, ny):
    X, Y = O.pair(O.SINGLE_SEED, nx, ny)
    both(dev, X, Y, max_iterations=20)


def degenerate(name):
    X, Y = (a.copy() for a in O.pair(O.SINGLE_SEED, 300, 257))
    if name == "coplanar":
        Y[:, 2] = 0.0
    elif name == "collinear":
        Y[:, 1] = 0.25
        Y[:, 2] = -0.5
    elif name == "identical":
        Y[:] = Y[7]
    return X, Y


@pytest.mark.parametrize("name", ["coplanar", "collinear", "identical"])
def test_flat_and_degenerate_targets_are_bit_identical(dev, name):
    X, Y = degenerate(name)
    both(dev, X, Y, max_iterations=20)
    idx, d2 = nearest(dev, X, Y)                                     # every query finds a neighbour, and it is a nearest one
    D = ((X[:, None, :].astype(np.float64) - Y[None].astype(np.float64)) ** 2).sum(axis=2)
    assert (idx >= 0).all() and np.allclose(D[np.arange(X.shape[0]), idx], D.min(axis=1), rtol=1e-6, atol=0)
    if name == "identical":
        assert (idx == 0).all()                                      # all rows tie: the first one


def test_queries_ten_box_lengths_outside_are_bit_identical(dev):
    X, Y = O.pair(O.SINGLE_SEED, 513, 1000)
    far = (torch.eye(3, device=dev), torch.tensor([10.0, -10.0, 10.0], device=dev))      # the box of Y is about one unit long
    both(dev, X, Y, init_transform=far, max_iterations=10)
    both(dev, X, Y, init_transform=far, max_iterations=3, max_correspondence_distance=0.5)      # ... and gated: nothing within reach


def test_non_finite_rows_are_never_neighbours_and_bit_identical(dev):
    X, Y = (a.copy() for a in O.pair(O.SINGLE_SEED, 300, 257))
    Y[11] = (np.nan, 0.1, 0.2)
    Y[200] = (0.1, np.inf, -0.2)
    X[5, 2] = np.nan
    idx, d2 = nearest(dev, X, Y)
    assert idx[5] == -1 and np.isinf(d2[5])                          # a NaN query has no neighbour
    ok = np.arange(300) != 5
    assert (idx[ok] >= 0).all() and not np.isin(idx[ok], (11, 200)).any() and np.isfinite(d2[ok]).all()
    # ICP with the NaN query: the moments take in whatever the search returns for it (nothing), so both paths agree bit for bit
    both(dev, X, Y, max_iterations=10)
    X[5, 2] = 0.0
    grid, _ = both(dev, X, Y, max_iterations=30)
    assert np.isfinite(grid.R.cpu().numpy()).all() and np.isfinite(float(grid.rmse[0]))


def test_problems_that_share_their_y_rows_are_bit_identical(dev):
    Xa, Y = O.pair(O.SINGLE_SEED, 300, 257)
    Xb = O.pair(O.EXACT_COUNT[0][0], 256, 256)[0]
    Yj = np.concatenate([Y, O.pair(3, 256, 256)[1][:100]])
    X = np.concatenate([Xa, Xb, Xa[:40]])
    x_seg = np.array([[0, 300], [300, 256], [556, 40]], np.int32)
    # two problems on the same rows (one grid serves both), and a third whose rows overlap them without being equal: with 357 rows of Y
    # and 257 + 300 asked for, it is the one searched row by row
    y_seg = np.array([[0, 257], [0, 257], [57, 300]], np.int32)
    grid, _ = both_packed(dev, X, x_seg, Yj, y_seg, max_iterations=20)
    solo = rap_amd.iterative_closest_point(t(Xa, dev), t(Y, dev), search="grid", max_iterations=20)
    assert torch.equal(grid.R[0].cpu(), solo.R[0].cpu()) and torch.equal(grid.rmse[0].cpu(), solo.rmse[0].cpu())


# 4. one larger problem -------------------------------------------------------------------------------------
def test_twenty_thousand_points_are_bit_identical(dev):
    X, Y = O.make_pair(21, 20_000, 20_000)
    grid, _ = both(dev, X, Y, max_iterations=10)
    assert int(grid.iterations[0]) >= 1 and np.isfinite(float(grid.rmse[0]))


# 5. repeatability and graph capture ---------------------------------------------------------------------------
def batch_call(dev):
    Xa, Ya = O.pair(O.SINGLE_SEED, 300, 257)
    Xb, Yb = O.pair(O.EXACT_COUNT[0][0], 256, 256)
    X = torch.from_numpy(np.concatenate([Xa, Xb])).to(dev)
    Y = torch.from_numpy(np.concatenate([Yb, Ya])).to(dev)
    xs = torch.tensor([[0, 300], [300, 256]], dtype=torch.int32, device=dev)
    ys = torch.tensor([[256, 257], [0, 256]], dtype=torch.int32, device=dev)

    def call():
        sol = rap_amd.icp_packed(X, xs, Y, ys, max_correspondence_distance=0.2, search="grid")
        idx, d2 = rap_amd.nearest_neighbors_packed(X, xs, Y, ys, max_distance=0.2)
        return sol, idx, d2
    return call


def all_bits(out):
    sol, idx, d2 = out
    return bits(sol) + [idx.cpu().view(torch.uint8).clone(), d2.cpu().view(torch.uint8).clone()]


def test_two_grid_calls_are_bitwise_equal(dev):
    call = batch_call(dev)
    assert same_bits(all_bits(call()), all_bits(call()))


def test_grid_calls_make_no_host_synchronisation(dev):
    call = batch_call(dev)
    want = all_bits(call())                                          # (also sizes the workspace: growing it is an allocation, not a sync)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = call()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert same_bits(all_bits(out), want)


def test_single_stream_captured_graph_of_grid_calls_replays_to_the_eager_bits(dev):
    call = batch_call(dev)
    want = all_bits(call())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                    # one capture stream: the calls' launches form a single chain
        out = call()
    sol, idx, d2 = out
    for _ in range(2):
        for x in (sol.rmse, sol.R, sol.T, sol.Xt, d2):
            x.fill_(float("nan"))
        idx.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(all_bits(out), want)
