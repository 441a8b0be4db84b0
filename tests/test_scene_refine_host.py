"""CPU: rap_scene_refine refuses bad arguments before anything touches the device, its workspace query is host arithmetic, the Python
wrappers refuse CPU tensors and bad knobs, a host build of the dense solver (rap_amd/csrc/sym_solve.h) agrees with numpy.linalg.pinv,
and the inputs the GPU tests (tests/test_scene_refine_gpu.py) hold the kernels to are fit for it -- the margins of the "exact" cases and
the fp32 bound are measured from the yardstick (tests/scene_refine_oracle.py) alone, not from the code under test."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import scene_refine_oracle as S
from rap_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, ONE = ctypes.c_void_p(0), ctypes.c_void_p(256)      # NULL; a non-NULL sentinel -- every call below fails before a pointer is used


def call(lib, **kw):
    a = dict(P=ONE, Pn=ONE, vs=ONE, V=8, n=4000, ss=ONE, S=2, ed=ONE, E=24, budget=12000, mv=16, fixed=N, iR=N, iT=N, it=10, thr=1e-6, gate=0.0,
             R=ONE, T=ONE, rmse=ONE, iters=ONE, conv=ONE, er=N, ec=N, ws=ONE, wsb=1 << 30)
    a.update(kw)
    return lib.rap_scene_refine(a["P"], a["Pn"], a["vs"], a["V"], a["n"], a["ss"], a["S"], a["ed"], a["E"], a["budget"], a["mv"], a["fixed"],
                                a["iR"], a["iT"], a["it"], a["thr"], a["gate"], a["R"], a["T"], a["rmse"], a["iters"], a["conv"], a["er"], a["ec"],
                                a["ws"], a["wsb"], N)


def test_rap_scene_refine_refuses_bad_arguments_without_a_gpu():
    lib = _lib.load()
    assert lib.rap_version() == 6                                        # the addition is additive
    for name in ("P", "Pn", "vs", "ss", "ed", "R", "T", "rmse", "iters", "conv"):
        assert call(lib, **{name: N}) == -1, name
    for name, bad in (("V", (0, -1, 65536)), ("S", (0, -2)), ("E", (0, -1, 65536)), ("n", (0, -5, 1 << 31)), ("budget", (0, -1, 1 << 40)),
                      ("mv", (1, 0, 17, -3)), ("it", (0, -1)), ("thr", (float("nan"),)), ("gate", (float("nan"),))):
        for v in bad:
            assert call(lib, **{name: v}) == -1, (name, v)
    need = lib.rap_scene_refine_workspace_bytes(4000, 8, 2, 24, 12000, 16)
    assert need > 0 and call(lib, ws=N) == -2 and call(lib, wsb=need - 1) == -2 and call(lib, wsb=0) == -2


def test_scene_refine_workspace_query_is_host_arithmetic():
    lib = _lib.load()
    q = lib.rap_scene_refine_workspace_bytes
    for bad in ((0, 8, 2, 24, 100, 16), (100, 0, 2, 24, 100, 16), (100, 8, 0, 24, 100, 16), (100, 8, 2, 0, 100, 16), (100, 8, 2, 24, 0, 16),
                (100, 8, 2, 24, 100, 1), (100, 8, 2, 24, 100, 17), (100, 65536, 2, 24, 100, 16), (100, 8, 2, 65536, 100, 16)):
        assert q(*bad) == 0, bad
    up = lambda n: -(-n // 256) * 256
    for n, V, Sn, E, budget in ((1, 1, 1, 1, 1), (1000, 3, 1, 6, 2000), (4000, 8, 2, 24, 12000), (200_000, 64, 4, 960, 3_000_000), (513, 16, 1, 240, 255)):
        items = budget // 256 + E + 1
        grid = lib.rap_icp_grid_workspace_bytes(7, n, V) - lib.rap_icp_workspace_bytes(7, V)      # one grid per view over the n rows
        want = (up(items * 32) + up(items * 232)            # work items; one partial of 28 fp64 moments + a count per item
                + up(E * 16) + 3 * up(E * 4)                # per edge: item range and views; scene, place in its scene's list, done flag
                + up(E * 36) + up(E * 12)                   # the fp32 pose of the edge
                + up(E * 232) + up(E * 42 * 8)              # the edge's summed moments; A_w and g_w in the world frame
                + up(V * 16) + up(V * 96)                   # per view: clamped rows, scene, fixed flag; the fp64 pose
                + up(Sn * 16) + up(Sn * 8) + up(Sn * 4)     # per scene: views and edge list; previous rmse; done flag
                + grid)
        assert q(n, V, Sn, E, budget, 16) == want == q(n, V, Sn, E, budget, 2), (n, V, Sn, E, budget)      # the solve's matrices live in LDS


def test_python_entry_points_refuse_cpu_tensors_and_bad_knobs():
    import rap_amd
    P, seg, sc = torch.zeros(20, 3), torch.tensor([[0, 10], [10, 10]]), torch.tensor([[0, 2]])
    for kw in (dict(max_views=1), dict(max_views=17), dict(max_iterations=0), dict(max_correspondence_distance=0.0), dict(row_budget=0)):
        with pytest.raises(ValueError):
            rap_amd.refine_scene_packed(P, seg, sc, **kw)
        with pytest.raises(ValueError):
            rap_amd.refine_registration(P, torch.tensor([[10, 10]]), torch.zeros(1, 2, 3, 3), torch.zeros(1, 2, 3), **kw)
    with pytest.raises(_lib.RapError):
        rap_amd.refine_scene_packed(P, seg, sc)
    with pytest.raises(_lib.RapError):
        rap_amd.refine_registration(P, torch.tensor([[10, 10]]), torch.zeros(1, 2, 3, 3), torch.zeros(1, 2, 3))
    assert rap_amd.SceneRefinement._fields == ("R", "T", "rmse", "iterations", "converged", "edge_rmse", "edge_count")


def test_all_pairs_table_of_the_wrapper_is_the_yardsticks():
    from rap_amd.scene import _all_pairs
    for mv, scenes in ((16, [(0, 3), (3, 16), (19, 1)]), (4, [(2, 4), (6, 2), (8, 0), (8, 7)])):
        got = _all_pairs(torch.tensor(scenes, dtype=torch.int32), 40, mv).numpy()
        want = S.all_pairs([(f, min(c, mv)) for f, c in scenes], mv)
        assert got.shape == (len(scenes) * mv * (mv - 1), 2) and np.array_equal(got, want)


def test_registration_tables_fix_flagged_nonempty_parts_or_the_first_nonempty_one():
    from rap_amd.scene import _registration_tables
    ppp = torch.tensor([[0, 5, 7, 0], [4, 0, 6, 2], [3, 3, 3, 3]])
    anchors = torch.tensor([[True, False, False, False], [False, True, True, True], [False, False, False, False]])
    cloud = torch.zeros(int(ppp.sum()), 3)
    seg, scenes, fixed = _registration_tables(cloud, ppp, anchors, None)
    assert seg.tolist() == [[0, 0], [0, 5], [5, 7], [12, 0], [12, 4], [16, 0], [16, 6], [22, 2], [24, 3], [27, 3], [30, 3], [33, 3]]
    assert scenes.tolist() == [[0, 4], [4, 4], [8, 4]]
    assert fixed.tolist() == [0, 1, 0, 0, 0, 0, 1, 1, 1, 0, 0, 0]        # flagged but empty: the first non-empty one; flagged; none flagged
    assert _registration_tables(cloud, ppp, None, None)[2].tolist() == [0, 1, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]


# ---- the dense solve ----
@pytest.fixture(scope="module")
def solver(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("host") / "libsym_solve_host.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", out, os.path.join(ROOT, "tests", "host", "sym_solve_host.cpp")])
    lib = ctypes.CDLL(out)
    D = np.ctypeslib.ndpointer(np.float64, flags="C")
    lib.sym_solve_step.argtypes = [D, D, ctypes.c_int, ctypes.c_double, D]
    lib.sym_solve_step.restype = ctypes.c_int
    lib.sym_solve_pair_of.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    return lib


def system(n, kind, seed):
    """H = J^T J, g = J^T r for a random 3n x n J: full rank; rank-deficient by 1; by 6 (every 6-block shares six directions: a free
    gauge); by a whole zero 6-block (a view without an edge)"""
    rng = np.random.default_rng(seed)
    J = rng.normal(size=(3 * n, n))
    if kind == "rank-1":
        v = rng.normal(size=n)
        J = J - np.outer(J @ v, v) / (v @ v)
    elif kind == "gauge":
        B = n // 6
        J = J @ (np.eye(n) - np.kron(np.ones((B, B)) / B, np.eye(6)))
    elif kind == "block":
        J[:, 6:12] = 0.0
    return J.T @ J, J.T @ rng.normal(size=3 * n)


SOLVE_BOUND = 1e-12      # relative to |x|.  Measured (printed below): 2e-14 at n = 96, 2e-15 at n = 6; eps * n * cond = 2.2e-16 * 96 * 16 = 3.4e-13


@pytest.mark.parametrize("n", [6, 12, 42, 90, 96])
def test_host_build_of_the_solver_agrees_with_numpy_pinv(solver, n):
    worst, sweeps = 0.0, 0
    for kind, rank in (("spd", n), ("rank-1", n - 1), ("gauge", n - 6), ("block", n - 6)):
        if n < 12 and kind in ("gauge", "block"):
            continue
        for seed in range(3):
            H, g = system(n, kind, 100 * n + seed)
            lam = np.linalg.eigvalsh(H)
            assert int((lam > 1e-12 * lam[-1]).sum()) == rank
            x = np.zeros(n)
            sw = solver.sym_solve_step(np.ascontiguousarray(H), g, n, 1e-12, x)
            ref = -np.linalg.pinv(H, rcond=1e-12, hermitian=True) @ g
            err = np.linalg.norm(x - ref) / np.linalg.norm(ref)
            worst, sweeps = max(worst, err), max(sweeps, sw)
            assert 0 < sw < solver.sym_solve_max_sweeps() and err <= SOLVE_BOUND, (kind, seed, sw, err)
            if kind == "block":
                assert not x[6:12].any()                                 # a view without an edge does not move: exactly
    print(f"n = {n}: worst |x - pinv| / |x| {worst:.2e} (bound {SOLVE_BOUND:.0e}), at most {sweeps} sweeps (cap {solver.sym_solve_max_sweeps()})")


def test_solver_takes_zero_and_refuses_odd_sizes_and_its_tournament_meets_every_pair_once(solver):
    x = np.ones(6)
    assert solver.sym_solve_step(np.zeros((6, 6)), np.ones(6), 6, 1e-12, x) == 1 and not x.any()
    assert solver.sym_solve_step(np.zeros((7, 7)), np.ones(7), 7, 1e-12, np.zeros(7)) == -1
    assert solver.sym_solve_step(np.zeros((98, 98)), np.ones(98), 98, 1e-12, np.zeros(98)) == -1
    p, q = ctypes.c_int(), ctypes.c_int()
    for n in (2, 6, 96):
        seen = set()
        for step in range(n - 1):
            used = set()
            for j in range(n // 2):
                solver.sym_solve_pair_of(n, step, j, ctypes.byref(p), ctypes.byref(q))
                assert 0 <= p.value < q.value < n and not {p.value, q.value} & used
                used |= {p.value, q.value}
                seen.add((p.value, q.value))
        assert len(seen) == n * (n - 1) // 2


# ---- the inputs of the GPU tests ----
EXACT = [c for c in S.PARITY_CASES if c[4]]


@pytest.mark.parametrize("V,seed,gate,variant,exact", EXACT, ids=[f"{c[0]}views-{c[3]}" for c in EXACT])
def test_exact_cases_keep_their_neighbour_gate_and_rel_margins(V, seed, gate, variant, exact):
    r, f = S.parity_solved(V, seed, gate, variant, margins=True), S.parity_solved(V, seed, gate, variant, f32=True)
    print(f"{V} views {variant}: neighbour gap {r.nn_margin:.2e}, gate margin {r.gate_margin:.2e}, rel margin {r.rel_margin:.2e} "
          f"(fp32 run {f.rel_margin:.2e}) over {r.iterations[0]} iterations, {r.edge_count.sum()} pairs")
    assert r.converged.all() and r.nn_margin >= S.MARGIN and r.gate_margin >= S.MARGIN and r.rel_margin >= S.MARGIN and f.rel_margin >= S.MARGIN
    assert np.array_equal(f.iterations, r.iterations) and np.array_equal(f.edge_count, r.edge_count)
    if gate is not None:
        assert 0 < r.edge_count.sum() < sum(S.SMALL_ROWS[:V]) * (V - 1)  # the gate matters


def test_cases_cover_every_size_and_every_variant_with_and_without_a_gate():
    assert {(c[0], c[2] is None) for c in S.PARITY_CASES} == {(v, g) for v in (3, 4, 8, 16) for g in (False, True)}
    assert {(c[3], c[2] is None) for c in S.PARITY_CASES} == {(v, g) for v in S.FIXED_VARIANTS for g in (False, True)}
    for V, seed, gate, variant, exact in S.PARITY_CASES:
        rows = S.parity_scene(V, seed, variant)["seg"][:, 1]
        assert rows.min() >= 200 and rows.max() <= 600


def test_fp32_bound_is_three_times_the_yardsticks_own_fp32_deviation():
    worst = 0.0
    for V, seed, gate, variant, exact in S.PARITY_CASES:
        r, f = S.parity_solved(V, seed, gate, variant), S.parity_solved(V, seed, gate, variant, f32=True)
        d = S.deviation(r, f)
        worst = max(worst, d)
        print(f"{V} views, {variant}, gate {gate}: fp32 moved points vs fp64 {d:.2e}, gate margin of the fp32 run {f.gate_margin:.2e}")
        if gate is not None and not exact:
            assert f.gate_margin >= 5e-8 and np.abs(f.edge_count - r.edge_count).max() <= 1      # 13 x the spacing of fp32 at the gate (3.7e-9)
    for name, r, f in (("ring", S.ring_solved(), S.ring_solved(True)), ("planar", S.planar_solved(), S.planar_solved(True))):
        d = S.deviation(r, f)
        worst = max(worst, d)
        print(f"{name}: fp32 moved points vs fp64 {d:.2e}")
    print(f"largest {worst:.2e}; recorded {S.FP32_MEASURED:.2e}; bound {S.FP32_BOUND:.1e}")
    assert worst <= S.FP32_MEASURED and S.FP32_MEASURED <= 1.5 * worst   # the constant is the measurement, not a guess
    assert S.FP32_BOUND == max(3 * S.FP32_MEASURED, 2e-6)


def test_joint_refinement_of_the_ring_beats_the_chain_of_pairwise_icps():
    sc, joint, (Rc, Tc) = S.ring_scene(), S.ring_solved(), S.ring_chain()
    edges = S.ring_edges()
    start, chain, ours = (S.total_rmse(sc, R, T, edges, S.GATE) for R, T in ((sc["R0"], sc["T0"]), (Rc, Tc), (joint.R, joint.T)))
    print(f"ring of {S.RING_V}: total rmse at the start {start:.3e}, after the chain of five pairwise ICPs {chain:.3e}, after the joint refinement {ours:.3e}")
    assert joint.converged[0] and ours < chain < start
    assert len(edges) == 2 * S.RING_V and S.ring_solved(True).iterations[0] == joint.iterations[0]


def test_yardstick_rules_for_tables_budget_and_left_out_scenes():
    sc = S.parity_scene(3, 9, "first")
    args = (sc["P"], sc["N"], sc["seg"])
    r = S.refine(*args, [(0, 3)], [(0, 1), (1, 1), (0, 3), (-1, 0), (2, 0)], max_iterations=1, margins=False)
    assert r.live.tolist() == [True, False, False, False, True] and r.edge_count[1] == 0 and np.isnan(r.edge_rmse[1])
    assert np.array_equal(r.R[0], np.eye(3)) and r.iterations[0] == 1 and not r.converged[0]
    out = S.refine(*args, [(0, 3)], S.pairs_of(0, 3), max_views=2, margins=False)
    assert np.isnan(out.rmse[0]) and out.iterations[0] == 0 and not out.live.any()
    n0 = int(sc["seg"][0, 1])
    b = S.refine(*args, [(0, 3)], [(0, 1), (0, 2), (1, 0)], row_budget=2 * n0 + 3, max_iterations=1, margins=False)
    assert b.live.tolist() == [True, True, False]
    none = S.refine(*args, [(0, 3)], [(0, 1)], init_T=np.asarray([[0, 0, 0], [0, 0, 9], [0, 0, 0]], np.float32), init_R=np.tile(np.eye(3, dtype=np.float32), (3, 1, 1)),
                    max_correspondence_distance=0.05, margins=False)
    assert np.isinf(none.rmse[0]) and none.iterations[0] == 0 and not none.converged[0]
