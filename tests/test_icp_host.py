"""CPU: the batched ICP's entry points refuse bad arguments before anything touches the device, its workspace query is host arithmetic,
and the inputs the GPU tests (tests/test_icp_gpu.py) hold the kernels to are fit for it: on each of them the yardstick's own fp32 run stays
within 1e-6 of its fp64 run, and where an exact iteration count or a gated result is demanded no neighbour / gate decision comes within
1e-5 of flipping at any iteration."""
import ctypes

import numpy as np
import pytest
import torch

import icp_oracle as O
from rap_amd import _lib

N, ONE = ctypes.c_void_p(0), ctypes.c_void_p(256)      # NULL; a non-NULL sentinel -- every call below fails before a pointer is used


def call(lib, **kw):
    a = dict(X=ONE, xs=ONE, Y=ONE, ys=ONE, K=2, NX=1000, NY=900, iR=N, iT=N, it=10, thr=1e-6, gate=0.0, R=ONE, T=ONE, rmse=ONE, iters=ONE,
             conv=ONE, Xt=N, ws=ONE, wsb=1 << 30)
    a.update(kw)
    return lib.rap_icp(a["X"], a["xs"], a["Y"], a["ys"], a["K"], a["NX"], a["NY"], a["iR"], a["iT"], a["it"], a["thr"], a["gate"], a["R"],
                       a["T"], a["rmse"], a["iters"], a["conv"], a["Xt"], a["ws"], a["wsb"], N)


def test_rap_icp_refuses_bad_arguments_without_a_gpu():
    lib = _lib.load()
    for name in ("X", "xs", "Y", "ys", "R", "T", "rmse", "iters", "conv"):
        assert call(lib, **{name: N}) == -1, name
    assert call(lib, K=0) == -1 and call(lib, K=-3) == -1
    assert call(lib, it=0) == -1 and call(lib, it=-1) == -1
    assert call(lib, NX=0) == -1 and call(lib, NY=0) == -1 and call(lib, NX=1 << 31) == -1 and call(lib, NY=1 << 31) == -1
    assert call(lib, thr=float("nan")) == -1 and call(lib, gate=float("nan")) == -1
    need = lib.rap_icp_workspace_bytes(1000, 2)
    assert call(lib, ws=N) == -2 and call(lib, wsb=need - 1) == -2 and call(lib, wsb=0) == -2


def test_icp_workspace_query_is_host_arithmetic():
    q = _lib.load().rap_icp_workspace_bytes
    assert q(0, 4) == 0 and q(-1, 4) == 0 and q(1000, 0) == 0 and q(1000, -2) == 0
    up = lambda n: -(-n // 256) * 256
    for n, K in ((1, 1), (256, 1), (1000, 6), (100_000, 1), (131072, 32)):
        items = n // 256 + K + 1                                     # items of 256 queries: at most n / 256 full ones and one partial per problem
        # work items (32 bytes), one partial of 17 fp64 moments + a count per item, and per problem: item range, previous rmse, done flag
        assert q(n, K) == up(items * 32) + up(items * 144) + up(K * 16) + up(K * 8) + up(K * 4), (n, K)
    assert q(1 << 40, 1) > 1 << 39                                     # 64-bit arithmetic (the call itself refuses such an n)


def test_python_entry_points_refuse_cpu_tensors_and_bad_shapes():
    import rap_amd
    X, Y = torch.zeros(8, 3), torch.zeros(9, 3)
    with pytest.raises(_lib.RapError):
        rap_amd.iterative_closest_point(X, Y)
    with pytest.raises(_lib.RapError):
        rap_amd.align_anchor(X, X, torch.tensor([[8]]), torch.tensor([[True]]))
    with pytest.raises(_lib.RapError):
        rap_amd.compute_transform_errors_icp(X, X, torch.eye(3).reshape(1, 1, 3, 3), torch.zeros(1, 1, 3), torch.eye(3).reshape(1, 1, 3, 3),
                                             torch.zeros(1, 1, 3), torch.tensor([[8]]), torch.tensor([[False]]))
    assert rap_amd.ICPSolution._fields == ("converged", "rmse", "Xt", "R", "T", "iterations")


def gpu_test_inputs():
    cases = [(O.SINGLE_SEED, nx, ny, {}) for nx, ny in O.SINGLE_SIZES] + [(s, nx, ny, {}) for s, nx, ny in O.EXACT_COUNT]
    cases.append((O.SINGLE_SEED, 513, 1000, dict(init=True)))
    g = O.GATE_CASE
    cases.append((g["seed"], g["nx"], g["ny"], dict(x_range=g["x_range"], y_range=g["y_range"], gate=O.GATE)))
    return cases


@pytest.mark.parametrize("seed,nx,ny,kw", gpu_test_inputs(), ids=lambda v: str(v).replace(" ", "") if not isinstance(v, dict) else "-".join(v) or "plain")
def test_fp32_run_of_the_yardstick_stays_within_1e_6_of_its_fp64_run(seed, nx, ny, kw):
    a, b = O.solved(seed, nx, ny, **kw), O.solved(seed, nx, ny, f32=True, **kw)
    dR, dT, dr = np.abs(a.R - b.R).max(), np.abs(a.T - b.T).max(), abs(a.rmse - b.rmse)
    print(f"fp32 vs fp64 yardstick: |dR| {dR:.2e} |dT| {dT:.2e} |drmse| {dr:.2e}; iterations {a.iterations} / {b.iterations}")
    assert a.converged and b.converged
    assert dR < 1e-6 and dT < 1e-6 and dr < 1e-6


@pytest.mark.parametrize("seed,nx,ny", O.EXACT_COUNT)
def test_exact_count_inputs_keep_a_neighbour_margin(seed, nx, ny):
    r = O.solved(seed, nx, ny, margins=True)
    print(f"seed {seed}: smallest nearest / second-nearest gap {r.nn_margin:.2e} over {r.iterations} iterations")
    assert r.converged and r.nn_margin >= 1e-5
    assert O.solved(seed, nx, ny, f32=True).iterations == r.iterations


def test_gated_input_keeps_a_gate_margin():
    g = O.GATE_CASE
    r = O.solved(g["seed"], g["nx"], g["ny"], x_range=g["x_range"], y_range=g["y_range"], gate=O.GATE)
    print(f"smallest |nearest distance - gate| {r.gate_margin:.2e} over {r.iterations} iterations")
    assert r.converged and r.gate_margin >= 1e-5
    X, Y = O.pair(g["seed"], g["nx"], g["ny"], g["x_range"], g["y_range"])
    lo = float(np.sqrt(O.nearest(X.astype(np.float64), Y.astype(np.float64), second=False)[1].min()))
    assert lo > 2e-4                                                  # the gate of 1e-4 the GPU test uses for the `inf` rule is below every distance
    none = O.icp(X, Y, max_correspondence_distance=1e-4)
    assert np.isinf(none.rmse) and not none.converged and none.iterations == 0 and np.array_equal(none.R, np.eye(3))


def test_yardstick_rules_for_empty_and_tiny_problems():
    X, Y = O.pair(0, 256, 256)
    for r in (O.icp(X[:0], Y), O.icp(X, Y[:0])):
        assert np.isnan(r.rmse) and r.iterations == 0 and not r.converged and np.array_equal(r.R, np.eye(3)) and not r.T.any()
    one = O.icp(X[:1], Y)                                             # rmse 0 after the first fit: prev == 0 counts as converged
    assert one.converged and one.iterations == 2 and one.rmse < 1e-12
    lim = O.icp(X, Y, max_iterations=1)
    assert lim.iterations == 1 and not lim.converged


# ---- the inputs at table scale (tests/test_table_scale_gpu.py) ---------------------------------------------------------------------------
def test_batch_of_300_problems_is_what_the_gpu_test_takes_it_for():
    b = O.batch300()
    K, kinds, xs, ys = O.BATCH_K, b["kinds"], b["x_seg"], b["y_seg"]
    assert K == 300 and xs.shape == ys.shape == (K, 2) and b["init_R"].shape == (K, 3, 3) and b["init_T"].shape == (K, 3)
    count = {name: kinds.count(name) for name in set(kinds)}
    print(f"X {b['X'].shape[0]} rows, Y {b['Y'].shape[0]} rows: {count}")
    assert count["lattice"] >= 250 and count["surface"] >= 30
    for special in (O.BATCH_EMPTY_X, O.BATCH_EMPTY_Y, O.BATCH_ONE_POINT, tuple(O.BATCH_SHARED_Y)):
        assert len(special) >= 2 and min(special) >= 256
    assert all(xs[k, 1] == 0 for k in O.BATCH_EMPTY_X) and all(ys[k, 1] == 0 for k in O.BATCH_EMPTY_Y) and all(xs[k, 1] == 1 for k in O.BATCH_ONE_POINT)
    for k, j in O.BATCH_SHARED_Y.items():                             # the owner of the grid sits in the first round of the plan loop
        assert j < 256 <= k and tuple(ys[k]) == tuple(ys[j]) and tuple(xs[k]) != tuple(xs[j])
    assert len(set(O.BATCH_SHARED_Y.values())) < len(O.BATCH_SHARED_Y)      # one target shared by three problems
    # shuffled, with junk between: the segments do not lie in problem order, do not overlap, and leave rows uncovered
    for seg, rows, shared in ((xs, b["X"], {}), (ys, b["Y"], O.BATCH_SHARED_Y)):
        own = [k for k in range(K) if seg[k, 1] > 0 and k not in shared]
        order = sorted(own, key=lambda k: seg[k, 0])
        assert order != own and sum(a > c for a, c in zip(order, order[1:])) > K // 3
        ends = [(int(seg[k, 0]), int(seg[k, 0] + seg[k, 1])) for k in order]
        assert all(e0 <= s1 for (_, e0), (s1, _) in zip(ends, ends[1:])) and ends[-1][1] <= rows.shape[0]
        assert sum(int(seg[k, 1]) for k in own) < rows.shape[0] - K // 2
    for k, p in enumerate(b["parts"]):
        if p is not None:
            assert np.array_equal(b["X"][xs[k, 0]:xs[k, 0] + xs[k, 1]], p[0]) and np.array_equal(b["Y"][ys[k, 0]:ys[k, 0] + ys[k, 1]], p[1])
    assert sum(p is not None for p in b["parts"]) == K - 6            # every problem is compared but the empty and the one-point ones
    ang = np.degrees(np.arccos(np.clip((np.trace(b["init_R"].astype(np.float64), axis1=1, axis2=2) - 1) / 2, -1, 1)))
    assert 0.15 < ang.max() < 0.21 and len({tuple(r.ravel()) for r in b["init_R"]}) == K


@pytest.mark.parametrize("init", [False, True], ids=["identity", "init_transform"])
def test_batch_of_300_keeps_its_neighbour_margin_and_spreads_its_iteration_counts(init):
    b, ref, f32 = O.batch300(), O.batch300_solved(init), O.batch300_solved(init, f32=True)
    compared = [k for k in range(O.BATCH_K) if ref[k] is not None]
    margin = min(ref[k].nn_margin for k in compared)
    counts = sorted({ref[k].iterations for k in compared})
    print(f"{len(compared)} problems: smallest nearest / second-nearest gap {margin:.2e} (required {O.BATCH_MARGIN:.0e}), iteration counts {counts}")
    assert O.BATCH_MARGIN > 1e-5 and margin >= O.BATCH_MARGIN         # above the 1e-5 of the normals tests
    assert all(ref[k].converged for k in compared)
    assert len(counts) >= 3 and len({ref[k].iterations for k in compared if k >= 256}) >= 3      # neighbours in done[] finish at different iterations
    assert all(f32[k].iterations == ref[k].iterations for k in compared)      # the stop is no rounding decision
    worst = max(max(np.abs(f32[k].R - ref[k].R).max(), np.abs(f32[k].T - ref[k].T).max(), abs(f32[k].rmse - ref[k].rmse)) for k in compared)
    print(f"fp32 statements vs fp64: worst deviation {worst:.2e}")
    assert worst < 5e-7
    if not init:                                                      # the truth of the lattice pairs is known
        dev = [max(np.abs(ref[k].R - R).max(), np.abs(ref[k].T - T).max())
               for k in compared if b["kinds"][k] == "lattice" for R, T in [O.make_lattice_pair(**O.batch_lattice_args(k))[2:]]]
        print(f"{len(dev)} lattice pairs: the yardstick within {max(dev):.2e} of the truth")
        assert max(dev) < 1e-7
        for k, j in O.BATCH_SHARED_Y.items():                          # a subset of an exact fit is an exact fit
            assert np.abs(ref[k].R - ref[j].R).max() < 1e-7
    else:
        assert max(np.abs(ref[k].R - O.batch300_solved(False)[k].R).max() for k in compared if b["kinds"][k] != "surface") < 1e-7


@pytest.mark.parametrize("nx", O.BIG_NX)
def test_big_problem_has_more_than_64_items_and_keeps_its_margin(nx):
    X, Y, xs, ys, parts = O.big_batch(nx)
    ref = O.big_solved(nx)
    items = -(-nx // 256)
    print(f"{nx} x {parts[1][1].shape[0]}: {items} items, gap {ref[1].nn_margin:.2e}, {ref[1].iterations} iterations, rmse {ref[1].rmse:.2e}")
    assert items > (64 if nx < 20_000 else 128) and xs[1, 0] > 0 and 216 <= parts[1][1].shape[0] <= 1000
    assert all(r.converged and r.nn_margin >= O.BATCH_MARGIN for r in ref) and ref[1].rmse > 1e-3
    assert O.icp(*parts[1], dtype=np.float32, margins=False).iterations == ref[1].iterations
