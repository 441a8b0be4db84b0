"""CPU: what the GPU tests of the k-best walk (tests/test_knn_gpu.py, tests/test_guards_knn_gpu.py) rely on, measured from the yardstick
(tests/knn_cases.py, tests/icp_plane_oracle.py) and never from the code under test; and the argument checks and the workspace
arithmetic of the three entry points, which return before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import icp_plane_oracle as P
import knn_cases as C
import nn_grid_cases as G
from rap_amd import _lib

N, ONE = ctypes.c_void_p(0), ctypes.c_void_p(256)      # NULL; a non-NULL sentinel -- every call below fails before a pointer is used


def test_exact_inputs_are_exact_in_fp32():
    for name, Y in list(C.exact_inputs().items()) + [("queries", C.exact_queries())]:
        assert Y.dtype == np.float32 and (Y * 4 == np.round(Y * 4)).all() and np.abs(Y).max() <= 64, name
        d = (Y[:, None, :].astype(np.float64) - Y[None].astype(np.float64))
        exact = (d * d).sum(axis=2)
        assert np.array_equal(exact.astype(np.float32).astype(np.float64), exact), name        # every d2 is an fp32 number
    E = C.exact_inputs()
    assert [E[n].shape[0] for n in ("lattice7", "lattice7_dup", "flat19", "line40", "copies33", "single")] == [343, 343, 361, 40, 33, 1]
    assert np.unique(E["lattice7"], axis=0).shape[0] == 343 and np.unique(E["lattice7_dup"], axis=0).shape[0] == 240
    assert np.ptp(E["flat19"][:, 2]) == 0 and np.linalg.matrix_rank(E["line40"] - E["line40"][0]) == 1
    q = C.exact_queries()
    box = np.abs(q).max(axis=1)
    assert (box[:60] <= 2.25).all() and (box[60:120] == 2.25).all() and (box[120:] > 2.25).all() and box.max() >= 2.25 + 45


def test_yardstick_agrees_with_the_older_ones():
    """knn() against the first arg-min of tests/nn_grid_cases.py (k = 1) and against the neighbour counts of icp_plane_oracle"""
    Y, X, _ = G.lattice()
    i, d2, _ = G.first_argmin(X, Y)
    idx, dd, cnt = C.knn(X, Y, 1)
    assert np.array_equal(idx[:, 0], i) and np.array_equal(dd[:, 0], d2) and (cnt == 1).all()
    pts = C.two_cluster()
    for k, r in C.TWO_CLUSTER_SETTINGS:
        assert np.array_equal(C.knn(pts, pts, k, r)[2], P.estimate_normals(pts, k, r)[2])
    idx, dd, cnt = C.knn(np.asarray([[np.nan, 0, 0], [0, 0, 0]], np.float32), np.asarray([[0, 0, 0], [np.inf, 0, 0], [1, 0, 0]], np.float32), 3)
    assert cnt.tolist() == [0, 2] and idx[1].tolist() == [0, 2, -1] and dd[1].tolist() == [0.0, 1.0, np.inf] and (idx[0] == -1).all()


def test_two_cluster_cloud_keeps_its_neighbour_sets_apart():
    pts = C.two_cluster()
    assert pts.shape == (310, 3) and (pts[:, 0] > 20).sum() == 300
    for k, r in C.TWO_CLUSTER_SETTINGS:
        _, _, counts, gap = P.estimate_normals(pts, k, r)
        print(f"two clusters max_nn {k} radius {r}: smallest gap {gap.min():.2e} (required {P.SWEEP_GAP:.0e}), {(counts < 3).sum()} rows below three neighbours")
        assert gap.min() >= P.SWEEP_GAP, (k, r, gap.min())
        if r > 0:
            assert (counts < 3).sum() == 1 and 3 < counts.max() < k      # the radius binds for every row, and leaves one without an estimate
        else:
            assert (counts == k).all()
    # the small cluster finds most of a 32-list forty units away
    idx, _, _ = C.knn(pts, pts, 32)
    small = np.nonzero(pts[:, 0] < 20)[0]
    assert ((pts[idx[small]][:, :, 0] > 20).sum(axis=1) == 22).all()


def test_exact_inputs_hold_ties_whose_winner_lies_in_a_farther_shell():
    E = C.exact_inputs()
    hits = {name: [C.far_shell_ties(E[name], k) for k in C.KS] for name in ("lattice7", "lattice7_dup", "flat19", "line40")}
    print(f"queries with a far-shell winner per list size {C.KS}: {hits}")
    assert sum(hits["flat19"]) > 0 and sum(hits["lattice7"]) > 0 and sum(hits["line40"]) > 0, hits


# ---- the three entry points, without a GPU ------------------------------------------------------------------------------------------------
def knn_call(lib, **kw):
    a = dict(X=ONE, xs=ONE, Y=ONE, ys=ONE, K=2, nx=1000, ny=900, k=20, r=0.0, idx=ONE, d2=ONE, cnt=ONE, ws=ONE, wsb=1 << 30)
    a.update(kw)
    return lib.rap_k_nearest_neighbors(a["X"], a["xs"], a["Y"], a["ys"], a["K"], a["nx"], a["ny"], a["k"], a["r"], a["idx"], a["d2"], a["cnt"],
                                       a["ws"], a["wsb"], N)


def normals_call(lib, **kw):
    a = dict(P=ONE, seg=ONE, K=2, n=1000, max_nn=20, radius=0.5, vp=N, normals=ONE, eig=N, ws=ONE, wsb=1 << 30)
    a.update(kw)
    return lib.rap_estimate_normals_grid(a["P"], a["seg"], a["K"], a["n"], a["max_nn"], a["radius"], a["vp"], a["normals"], a["eig"], a["ws"],
                                         a["wsb"], N)


def outlier_call(lib, **kw):
    a = dict(pts=ONE, n=1000, k=20, ratio=2.5, idx=ONE, cnt=ONE, stats=N, ws=ONE, wsb=1 << 30)
    a.update(kw)
    return lib.rap_statistical_outliers_grid(a["pts"], a["n"], a["k"], a["ratio"], a["idx"], a["cnt"], a["stats"], a["ws"], a["wsb"], N)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    for name in ("X", "xs", "Y", "ys", "idx", "d2", "cnt"):
        assert knn_call(lib, **{name: N}) == -1, name
    for bad in (dict(k=0), dict(k=33), dict(k=-1), dict(K=0), dict(K=65536), dict(nx=0), dict(ny=0), dict(nx=1 << 31), dict(r=float("nan"))):
        assert knn_call(lib, **bad) == -1, bad
    need = lib.rap_knn_workspace_bytes(1000, 900, 2)
    assert knn_call(lib, ws=N) == -2 and knn_call(lib, wsb=need - 1) == -2 and knn_call(lib, wsb=0) == -2
    for name in ("P", "seg", "normals"):
        assert normals_call(lib, **{name: N}) == -1, name
    for bad in (dict(K=0), dict(K=65536), dict(n=0), dict(n=1 << 31), dict(max_nn=2), dict(max_nn=33), dict(radius=float("nan"))):
        assert normals_call(lib, **bad) == -1, bad
    need = lib.rap_normals_grid_workspace_bytes(1000, 2)
    assert normals_call(lib, ws=N) == -2 and normals_call(lib, wsb=need - 1) == -2
    for name in ("pts", "idx", "cnt"):
        assert outlier_call(lib, **{name: N}) == -1, name
    for bad in (dict(k=0), dict(k=33), dict(n=0), dict(ratio=0.0), dict(ratio=float("nan"))):
        assert outlier_call(lib, **bad) == -1, bad
    need = lib.rap_outlier_grid_workspace_bytes(1000)
    assert outlier_call(lib, ws=N) == -2 and outlier_call(lib, wsb=need - 1) == -2


def up(n):
    return -(-n // 256) * 256


def grid_bytes(ny, K):
    """the index: 64 bytes and a box per problem, two cell tables, a cell per row, the sorted rows, a sum per 2048 cells"""
    cells = ny + 8 * K + 1
    return up(K * 64) + up(K * 32) + 2 * up(cells * 4) + up(ny * 4) + up(ny * 16) + up((cells // 2048 + 1) * 4)


def test_workspace_queries_are_host_arithmetic_on_top_of_the_older_ones():
    lib = _lib.load()
    q = lib.rap_knn_workspace_bytes
    assert q(0, 5, 1) == 0 and q(5, 0, 1) == 0 and q(5, 5, 0) == 0
    assert lib.rap_normals_grid_workspace_bytes(0, 1) == 0 and lib.rap_normals_grid_workspace_bytes(9, 0) == 0
    assert lib.rap_outlier_grid_workspace_bytes(0) == 0 and lib.rap_outlier_grid_workspace_bytes(-3) == 0
    for nx, ny, K in ((1, 1, 1), (256, 300, 2), (1000, 20_000, 6), (100_000, 100_000, 1)):
        items = up((nx // 256 + K + 1) * 32)
        assert lib.rap_knn_workspace_bytes(nx, ny, K) == lib.rap_nn_grid_workspace_bytes(nx, ny, K) == items + grid_bytes(ny, K)
        assert lib.rap_normals_grid_workspace_bytes(ny, K) == lib.rap_normals_workspace_bytes(ny, K) + grid_bytes(ny, K)
        assert lib.rap_outlier_grid_workspace_bytes(ny) == lib.rap_outlier_workspace_bytes(ny) + 256 + up((ny // 256 + 2) * 32) + grid_bytes(ny, 1)
    assert lib.rap_outlier_grid_workspace_bytes(1 << 28) > 1 << 32


def test_python_entry_points_refuse_cpu_tensors_and_unknown_searches():
    import rap_amd
    from rap_amd.point_sampling import remove_statistical_outlier
    pts = torch.zeros(8, 3)
    seg = torch.tensor([[0, 8]])
    for search in ("kd", "", None, "Grid"):
        with pytest.raises(ValueError):
            rap_amd.estimate_normals_packed(pts, seg, search=search)
        with pytest.raises(ValueError):
            rap_amd.estimate_point_normals(pts, search=search)
        with pytest.raises(ValueError):
            remove_statistical_outlier(pts, search=search)
    for search in ("brute", "grid"):
        with pytest.raises(_lib.RapError):
            rap_amd.estimate_normals_packed(pts, seg, search=search)
        with pytest.raises(_lib.RapError):
            remove_statistical_outlier(pts, search=search)
    with pytest.raises(_lib.RapError):
        rap_amd.k_nearest_neighbors_packed(pts, seg, pts, seg, 3)
    assert "k_nearest_neighbors_packed" in rap_amd.__all__
