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
