"""GPU: the batched ICP (rap_amd/csrc/icp.hip, rap_amd/icp.py) against its fp64 yardstick (tests/icp_oracle.py) at the smallest sizes that
cross each edge of the kernels, and the two metrics built on it.

Bound: R, T and rmse within 2e-6 absolute of the fp64 yardstick -- what the project holds fit_transformations to (tests/test_kernels_gpu.py).
The device searches in fp32 and fits in fp64 from raw moments; the yardstick's own fp32 run stays within 1.6e-7 / 5e-8 / 2e-9 on these
inputs (tests/test_icp_host.py).  Every parity test prints its worst deviation before it asserts (run with -s to see them)."""
import numpy as np
import pytest
import torch

import icp_oracle as O
import rap_amd

pytestmark = pytest.mark.gpu

TOL = 2e-6


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def solve(dev, X, Y, **kw):
    return rap_amd.iterative_closest_point(torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev), **kw)


def init_tensors(dev):
    return torch.from_numpy(O.INIT[0]).float().to(dev), torch.from_numpy(O.INIT[1]).float().to(dev)


def deviation(sol, ref, what, k=0):
    R, T = sol.R[k].double().cpu().numpy(), sol.T[k].double().cpu().numpy()
    dR, dT, dr = np.abs(R - ref.R).max(), np.abs(T - ref.T).max(), abs(float(sol.rmse[k]) - ref.rmse)
    print(f"{what}: |dR| {dR:.2e} |dT| {dT:.2e} |drmse| {dr:.2e}; iterations {int(sol.iterations[k])} (yardstick {ref.iterations})")
    return dR, dT, dr


def assert_parity(sol, ref, what, k=0):
    dR, dT, dr = deviation(sol, ref, what, k)
    assert dR <= TOL and dT <= TOL and dr <= TOL, (what, dR, dT, dr)
    assert abs(np.linalg.det(sol.R[k].double().cpu().numpy()) - 1.0) < 1e-6


def bits(sol):
    return [t.contiguous().cpu().view(torch.uint8).clone() for t in (sol.converged.to(torch.uint8), sol.rmse, sol.Xt, sol.R, sol.T, sol.iterations)]


def same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# 1. single problems -------------------------------------------------------------------------
@pytest.mark.parametrize("nx,ny", O.SINGLE_SIZES)
def test_single_problem_matches_the_yardstick(dev, nx, ny):
    X, Y = O.pair(O.SINGLE_SEED, nx, ny)
    ref = O.solved(O.SINGLE_SEED, nx, ny)
    sol = solve(dev, X, Y)
    assert_parity(sol, ref, f"{nx} x {ny}")
    assert bool(sol.converged[0]) and ref.converged
    Xt = sol.Xt.double().cpu().numpy()
    assert Xt.shape == X.shape and np.abs(Xt - ref.Xt).max() <= TOL * (np.abs(X).sum(axis=1).max() + 1.0) + 4e-7      # |x|_1 |dR| + |dT| + fp32 rounding


# 2. exact iteration count where no neighbour decision is close --------------------------------
@pytest.mark.parametrize("seed,nx,ny", O.EXACT_COUNT)
def test_iteration_count_equals_the_yardstick_on_margin_checked_inputs(dev, seed, nx, ny):
    X, Y = O.pair(seed, nx, ny)
    ref = O.solved(seed, nx, ny)
    sol = solve(dev, X, Y)
    assert_parity(sol, ref, f"seed {seed} {nx} x {ny}")
    assert int(sol.iterations[0]) == ref.iterations and bool(sol.converged[0])


# 3. ragged batch --------------------------------------------------------------------------------
def test_ragged_batch_is_bit_identical_to_solo_runs_and_follows_the_rules_for_empty_and_tiny_problems(dev):
    Xa, Ya = O.pair(O.SINGLE_SEED, 300, 257)
    Xb, Yb = O.pair(O.SINGLE_SEED, 513, 1000)
    rng = np.random.default_rng(11)
    junk = lambda n: rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    # X: [junk 5 | B 513 | junk 3 | one point | A 300 | two points | junk 40 (the "x" of the empty-Y problem)], Y likewise out of order
    X = np.concatenate([junk(5), Xb, junk(3), Xa[:1], Xa, Xa[5:7], junk(40)])
    Y = np.concatenate([Ya, junk(7), Yb, junk(9)])
    xa, xb, x1, x2, xe = 5 + 513 + 3 + 1, 5, 5 + 513 + 3, 5 + 513 + 3 + 1 + 300, 5 + 513 + 3 + 1 + 300 + 2
    ya, yb = 0, 257 + 7
    #            empty X        real A          1 point       empty Y      real B           2 points
    x_seg = [[17, 0],       [xa, 300],      [x1, 1],      [xe, 40],    [xb, 513],       [x2, 2]]
    y_seg = [[ya, 257],     [ya, 257],      [yb, 1000],   [40, -3],    [yb, 1000],      [ya, 257]]
    Xd, Yd = torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev)
    sol = rap_amd.icp_packed(Xd, torch.tensor(x_seg, dtype=torch.int32, device=dev), Yd, torch.tensor(y_seg, dtype=torch.int32, device=dev))
    for k, (Xs, Ys, xs) in ((1, (Xa, Ya, xa)), (4, (Xb, Yb, xb))):
        solo = solve(dev, Xs, Ys)
        for name in ("R", "T", "rmse", "iterations", "converged"):
            assert torch.equal(getattr(sol, name)[k].cpu().view(-1), getattr(solo, name)[0].cpu().view(-1)), (k, name)
        assert torch.equal(sol.Xt[xs:xs + Xs.shape[0]].cpu(), solo.Xt.cpu()), k
        assert bool(sol.converged[k])
    eye = torch.eye(3)
    for k in (0, 3):                                               # an empty X, an empty Y
        assert torch.equal(sol.R[k].cpu(), eye) and not sol.T[k].cpu().any()
        assert torch.isnan(sol.rmse[k]) and int(sol.iterations[k]) == 0 and not bool(sol.converged[k])
    for k in (2, 5):                                               # one point, two points: a finite proper rotation
        R = sol.R[k].double().cpu().numpy()
        assert np.isfinite(R).all() and np.isfinite(sol.T[k].cpu().numpy()).all() and np.isfinite(float(sol.rmse[k]))
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(R) - 1.0) < 1e-6
    assert bool(sol.converged[2]) and float(sol.rmse[2]) < 1e-6      # one pair is fitted exactly, and a zero rmse counts as converged
    # rows outside every segment and the rows of the empty-Y problem (moved by the identity) pass through
    Xt = sol.Xt.cpu().numpy()
    for a, b in ((0, 5), (5 + 513, 5 + 513 + 3), (xe, xe + 40)):
        assert np.array_equal(Xt[a:b], X[a:b])


# 4. init_transform ------------------------------------------------------------------------------
def test_init_transform_matches_the_yardstick_started_from_the_same_transform(dev):
    X, Y = O.pair(O.SINGLE_SEED, 513, 1000)
    ref = O.solved(O.SINGLE_SEED, 513, 1000, init=True)
    sol = solve(dev, X, Y, init_transform=init_tensors(dev))
    assert_parity(sol, ref, "513 x 1000 with init_transform")
    assert bool(sol.converged[0])
    one = solve(dev, X, Y, init_transform=init_tensors(dev), max_iterations=1)      # the first fit depends on the start: not the identity's
    ref1, ref0 = O.solved(O.SINGLE_SEED, 513, 1000, init=True, max_iterations=1), O.solved(O.SINGLE_SEED, 513, 1000, max_iterations=1)
    assert_parity(one, ref1, "one iteration from init_transform")
    assert np.abs(ref1.R - ref0.R).max() > 1e-3


# 5. gate --------------------------------------------------------------------------------------------
def test_gated_partial_overlap_matches_the_gated_yardstick_and_an_empty_gate_reports_inf(dev):
    g = O.GATE_CASE
    X, Y = O.pair(g["seed"], g["nx"], g["ny"], g["x_range"], g["y_range"])
    ref = O.solved(g["seed"], g["nx"], g["ny"], x_range=g["x_range"], y_range=g["y_range"], gate=O.GATE)
    sol = solve(dev, X, Y, max_correspondence_distance=O.GATE)
    assert_parity(sol, ref, "gated 700 x 900")
    assert bool(sol.converged[0])
    free = O.solved(g["seed"], g["nx"], g["ny"], x_range=g["x_range"], y_range=g["y_range"])
    assert np.abs(free.R - ref.R).max() > 1e-3                      # the gate matters on this pair
    none = solve(dev, X, Y, max_correspondence_distance=1e-4)      # a gate below every distance (tests/test_icp_host.py)
    assert torch.isinf(none.rmse[0]) and float(none.rmse[0]) > 0 and not bool(none.converged[0]) and int(none.iterations[0]) == 0
    assert torch.equal(none.R[0].cpu(), torch.eye(3)) and not none.T[0].cpu().any()
    assert torch.equal(none.Xt.cpu(), torch.from_numpy(X))


# 6. exact rigid recovery ----------------------------------------------------------------------------
def test_exact_rigid_motion_of_a_permuted_lattice_is_recovered(dev):
    X, Y, R, T = O.make_lattice_pair(0)
    sol = solve(dev, X, Y)
    dR, dT = np.abs(sol.R[0].double().cpu().numpy() - R).max(), np.abs(sol.T[0].double().cpu().numpy() - T).max()
    print(f"lattice: |dR| {dR:.2e} |dT| {dT:.2e} rmse {float(sol.rmse[0]):.2e} iterations {int(sol.iterations[0])}")
    assert dR <= TOL and dT <= TOL
    assert float(sol.rmse[0]) < 1e-6 and bool(sol.converged[0])


# 7. iteration limit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("limit", [1, 5])
def test_iteration_limit_stops_without_convergence(dev, limit):
    seed, nx, ny = O.EXACT_COUNT[0]
    assert O.solved(seed, nx, ny).iterations > limit
    X, Y = O.pair(seed, nx, ny)
    sol = solve(dev, X, Y, max_iterations=limit)
    assert int(sol.iterations[0]) == limit and not bool(sol.converged[0])
    assert_parity(sol, O.solved(seed, nx, ny, max_iterations=limit), f"limit {limit}")


# 8. metrics ---------------------------------------------------------------------------------------------
def metrics_tensors(dev):
    d = O.metrics_batch()
    return d, {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in d.items()}


def test_align_anchor_matches_the_restated_reference(dev):
    d, t = metrics_tensors(dev)
    want = O.align_anchor(d["gt"], d["pred"], d["ppp"], d["anchor"])
    got = rap_amd.align_anchor(t["gt"], t["pred"], t["ppp"], t["anchor"], t["cu"])
    err = np.abs(got.double().cpu().numpy() - want).max()
    bound = TOL * (np.abs(d["pred"]).sum(axis=1).max() + 1.0) + 4e-7      # |x|_1 |dR| + |dT| + the fp32 rounding of x R + T
    print(f"align_anchor: worst point deviation {err:.2e} (bound {bound:.2e})")
    assert err <= bound
    a = int(d["cu"][2])
    assert torch.equal(got[a:].cpu(), t["pred"][a:].cpu())          # the sample without an anchor is returned unchanged
    assert np.abs(want[:a] - d["pred"][:a]).max() > 1e-3            # ... and the others are moved
    # the padded (B,N,3) layout gives the same points
    B, n_b = 3, d["ppp"].sum(axis=1)
    Nmax = int(n_b.max())
    pad = lambda x: torch.stack([torch.nn.functional.pad(x[int(d["cu"][b]):int(d["cu"][b + 1])], (0, 0, 0, Nmax - int(n_b[b]))) for b in range(B)])
    got_p = rap_amd.align_anchor(pad(t["gt"]), pad(t["pred"]), t["ppp"], t["anchor"])
    for b in range(B):
        assert torch.equal(got_p[b, :int(n_b[b])].cpu(), got[int(d["cu"][b]):int(d["cu"][b + 1])].cpu()), b


def test_transform_errors_icp_match_the_restated_reference(dev):
    d, t = metrics_tensors(dev)
    rot_m, trans_m, rot, trans = O.transform_errors_icp(d["cond"], d["gt"], d["R_pred"], d["t_pred"], d["ppp"], d["anchor"], d["scale"])
    valid = (d["ppp"] != 0) & ~d["anchor"]
    assert rot[valid].min() >= 0.3                                  # the rotation bound below is derived for errors of that size
    g_rot_m, g_trans_m, g_rot, g_trans = rap_amd.compute_transform_errors_icp(
        t["cond"], t["gt"], t["R_gt"], t["t_gt"], t["R_pred"], t["t_pred"], t["ppp"], t["anchor"], None, t["scale"], t["cu"], return_per_part=True)
    e_rot = np.abs(g_rot.double().cpu().numpy() - rot).max()
    e_trans = np.abs(g_trans.double().cpu().numpy() - trans).max()
    e_rot_m = np.abs(g_rot_m.double().cpu().numpy() - rot_m).max()
    e_trans_m = np.abs(g_trans_m.double().cpu().numpy() - trans_m).max()
    print(f"transform errors with ICP: rotation {e_rot:.2e} deg (mean {e_rot_m:.2e}), translation {e_trans:.2e} (mean {e_trans_m:.2e})")
    assert e_rot <= 5e-3 and e_rot_m <= 5e-3                        # tests/test_sample_gpu.py's rotation bound
    assert e_trans <= 1e-5 and e_trans_m <= 1e-5
    assert not g_rot.cpu().numpy()[~valid].any() and not g_trans.cpu().numpy()[~valid].any()
    # matched_part_ids re-orders the predicted poses: the identity permutation changes nothing
    ident = torch.arange(3, device=dev).repeat(3, 1)
    again = rap_amd.compute_transform_errors_icp(t["cond"], t["gt"], t["R_gt"], t["t_gt"], t["R_pred"], t["t_pred"], t["ppp"], t["anchor"], ident,
                                                 t["scale"], t["cu"])
    assert torch.equal(again[0], g_rot_m) and torch.equal(again[1], g_trans_m)


# 9. execution properties -----------------------------------------------------------------------------------
def batch_call(dev):
    Xa, Ya = O.pair(O.SINGLE_SEED, 300, 257)
    Xb, Yb = O.pair(O.EXACT_COUNT[0][0], 256, 256)
    X = torch.from_numpy(np.concatenate([Xa, Xb])).to(dev)
    Y = torch.from_numpy(np.concatenate([Yb, Ya])).to(dev)
    xs = torch.tensor([[0, 300], [300, 256]], dtype=torch.int32, device=dev)
    ys = torch.tensor([[256, 257], [0, 256]], dtype=torch.int32, device=dev)
    return lambda: rap_amd.icp_packed(X, xs, Y, ys, max_correspondence_distance=0.2)


def test_two_calls_are_bitwise_equal(dev):
    call = batch_call(dev)
    a, b = bits(call()), bits(call())
    assert same_bits(a, b)


def test_call_makes_no_host_synchronisation(dev):
    call = batch_call(dev)
    want = bits(call())                                              # (also sizes the workspace: growing it is an allocation, not a sync)
    d, t = metrics_tensors(dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        sol = call()
        al = rap_amd.align_anchor(t["gt"], t["pred"], t["ppp"], t["anchor"], t["cu"])
        te = rap_amd.compute_transform_errors_icp(t["cond"], t["gt"], t["R_gt"], t["t_gt"], t["R_pred"], t["t_pred"], t["ppp"], t["anchor"], None,
                                                  t["scale"], t["cu"])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert same_bits(bits(sol), want)
    assert bool(torch.isfinite(al).all()) and bool(torch.isfinite(te[0]).all())


def test_single_stream_captured_graph_replays_to_the_eager_bits(dev):
    call = batch_call(dev)
    want = bits(call())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                    # one capture stream: the call's launches form a single chain
        sol = call()
    for _ in range(2):
        for t in (sol.rmse, sol.R, sol.T, sol.Xt):
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(bits(sol), want)
