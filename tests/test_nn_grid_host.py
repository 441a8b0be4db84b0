"""CPU: the entry points of the grid neighbour search (rap_icp_grid, rap_nearest_neighbors and their workspace queries) refuse bad
arguments before anything touches the device, the queries are host arithmetic, the Python wrappers refuse CPU tensors and unknown
search names, and the lattice of tests/test_nn_grid_gpu.py really holds the ties it is there for."""
import ctypes

import numpy as np
import pytest
import torch

import nn_grid_cases as C
from rap_amd import _lib

N, ONE = ctypes.c_void_p(0), ctypes.c_void_p(256)      # NULL; a non-NULL sentinel -- every call below fails before a pointer is used


def icp_grid(lib, **kw):
    a = dict(X=ONE, xs=ONE, Y=ONE, ys=ONE, K=2, NX=1000, NY=900, iR=N, iT=N, it=10, thr=1e-6, gate=0.0, R=ONE, T=ONE, rmse=ONE, iters=ONE,
             conv=ONE, Xt=N, ws=ONE, wsb=1 << 30)
    a.update(kw)
    return lib.rap_icp_grid(a["X"], a["xs"], a["Y"], a["ys"], a["K"], a["NX"], a["NY"], a["iR"], a["iT"], a["it"], a["thr"], a["gate"],
                            a["R"], a["T"], a["rmse"], a["iters"], a["conv"], a["Xt"], a["ws"], a["wsb"], N)


def nearest(lib, **kw):
    a = dict(X=ONE, xs=ONE, Y=ONE, ys=ONE, K=2, NX=1000, NY=900, R=N, T=N, gate=0.0, idx=ONE, d2=ONE, ws=ONE, wsb=1 << 30)
    a.update(kw)
    return lib.rap_nearest_neighbors(a["X"], a["xs"], a["Y"], a["ys"], a["K"], a["NX"], a["NY"], a["R"], a["T"], a["gate"], a["idx"], a["d2"],
                                     a["ws"], a["wsb"], N)


def test_rap_icp_grid_refuses_bad_arguments_without_a_gpu():
    lib = _lib.load()
    for name in ("X", "xs", "Y", "ys", "R", "T", "rmse", "iters", "conv"):
        assert icp_grid(lib, **{name: N}) == -1, name
    assert icp_grid(lib, K=0) == -1 and icp_grid(lib, K=-3) == -1 and icp_grid(lib, K=65536) == -1
    assert icp_grid(lib, it=0) == -1 and icp_grid(lib, it=-1) == -1
    assert icp_grid(lib, NX=0) == -1 and icp_grid(lib, NY=0) == -1 and icp_grid(lib, NX=1 << 31) == -1 and icp_grid(lib, NY=1 << 31) == -1
    assert icp_grid(lib, thr=float("nan")) == -1 and icp_grid(lib, gate=float("nan")) == -1
    need = lib.rap_icp_grid_workspace_bytes(1000, 900, 2)
    assert icp_grid(lib, ws=N) == -2 and icp_grid(lib, wsb=need - 1) == -2 and icp_grid(lib, wsb=0) == -2
    assert icp_grid(lib, wsb=lib.rap_icp_workspace_bytes(1000, 2)) == -2      # the brute-force path's workspace is not enough


def test_rap_nearest_neighbors_refuses_bad_arguments_without_a_gpu():
    lib = _lib.load()
    for name in ("X", "xs", "Y", "ys", "idx", "d2"):
        assert nearest(lib, **{name: N}) == -1, name
    assert nearest(lib, R=ONE) == -1 and nearest(lib, T=ONE) == -1                 # R and T come together
    assert nearest(lib, K=0) == -1 and nearest(lib, K=-1) == -1 and nearest(lib, K=65536) == -1
    assert nearest(lib, NX=0) == -1 and nearest(lib, NY=0) == -1 and nearest(lib, NX=1 << 31) == -1 and nearest(lib, NY=1 << 31) == -1
    assert nearest(lib, gate=float("nan")) == -1
    need = lib.rap_nn_grid_workspace_bytes(1000, 900, 2)
    assert nearest(lib, ws=N) == -2 and nearest(lib, wsb=need - 1) == -2 and nearest(lib, wsb=0) == -2


def test_grid_workspace_queries_are_host_arithmetic():
    lib = _lib.load()
    up = lambda n: -(-n // 256) * 256
    for q in (lib.rap_icp_grid_workspace_bytes, lib.rap_nn_grid_workspace_bytes):
        for bad in ((0, 10, 1), (10, 0, 1), (10, 10, 0), (-1, 10, 1), (10, -5, 1), (10, 10, -2)):
            assert q(*bad) == 0, bad
        sizes = [1, 255, 256, 257, 4099, 100_000, 2_000_000]
        for a, b in zip(sizes, sizes[1:]):                              # monotone in each argument
            assert 0 < q(a, 1000, 4) <= q(b, 1000, 4)
            assert 0 < q(1000, a, 4) <= q(1000, b, 4)
        for a, b in zip((1, 2, 6, 32, 640), (2, 6, 32, 640, 65535)):
            assert q(1000, 1000, a) <= q(1000, 1000, b)
        assert q(1 << 40, 1 << 40, 1) > 1 << 42                          # 64-bit arithmetic (the calls themselves refuse such sizes)
    for nx, ny, K in ((1, 1, 1), (256, 257, 1), (1000, 4099, 6), (100_000, 100_000, 1), (131072, 131072, 32)):
        cells = ny + 8 * K + 1
        # per problem a 64-byte grid and its 32-byte box; per cell its first row and its fill level; per row of Y its cell and its
        # 16-byte sorted copy; one partial sum per 2048 cells
        index = up(K * 64) + up(K * 32) + 2 * up(cells * 4) + up(ny * 4) + up(ny * 16) + up((cells // 2048 + 1) * 4)
        assert lib.rap_icp_grid_workspace_bytes(nx, ny, K) == lib.rap_icp_workspace_bytes(nx, K) + index, (nx, ny, K)
        assert lib.rap_nn_grid_workspace_bytes(nx, ny, K) == up((nx // 256 + K + 1) * 32) + index, (nx, ny, K)
        assert lib.rap_icp_grid_workspace_bytes(nx, ny, K) >= lib.rap_icp_workspace_bytes(nx, K)


def test_python_wrappers_refuse_cpu_tensors_and_unknown_searches():
    import rap_amd
    X, Y = torch.zeros(8, 3), torch.zeros(9, 3)
    seg = torch.tensor([[0, 8]], dtype=torch.int32)
    one = (torch.eye(3).reshape(1, 1, 3, 3), torch.zeros(1, 1, 3))
    with pytest.raises(_lib.RapError):
        rap_amd.iterative_closest_point(X, Y, search="grid")
    with pytest.raises(_lib.RapError):
        rap_amd.icp_packed(X, seg, Y, seg, search="grid")
    with pytest.raises(_lib.RapError):
        rap_amd.nearest_neighbors_packed(X, seg, Y, seg)
    with pytest.raises(_lib.RapError):
        rap_amd.align_anchor(X, X, torch.tensor([[8]]), torch.tensor([[True]]), search="grid")
    with pytest.raises(_lib.RapError):
        rap_amd.compute_transform_errors_icp(X, X, *one, *one, torch.tensor([[8]]), torch.tensor([[False]]), search="grid")
    for bad in ("kd", "auto", "", None):                                 # refused before anything else is looked at
        with pytest.raises(ValueError):
            rap_amd.iterative_closest_point(X, Y, search=bad)
        with pytest.raises(ValueError):
            rap_amd.icp_packed(X, seg, Y, seg, search=bad)
        with pytest.raises(ValueError):
            rap_amd.align_anchor(X, X, torch.tensor([[8]]), torch.tensor([[True]]), search=bad)
        with pytest.raises(ValueError):
            rap_amd.compute_transform_errors_icp(X, X, *one, *one, torch.tensor([[8]]), torch.tensor([[False]]), search=bad)
    assert "nearest_neighbors_packed" in rap_amd.__all__


def test_lattice_holds_exact_two_four_and_eight_way_ties_across_cells():
    Y, X, kind = C.lattice()
    assert Y.shape == (512, 3) and (kind == "outside").sum() == 64
    i32, d32, n32 = C.first_argmin(X, Y, np.float32)
    i64, d64, n64 = C.first_argmin(X, Y, np.float64)
    assert np.array_equal(i32, i64) and np.array_equal(d32.astype(np.float64), d64) and np.array_equal(n32, n64)      # exact in fp32
    for name, ways in (("edge", 2), ("face", 4), ("cell", 8), ("point", 1)):
        assert (n64[kind == name] == ways).all(), name
    assert (n64[kind == "outside"] > 1).any() and (n64[kind == "outside"] == 1).any()
    # the tied rows of a query do not all sit in one cell of the grid the device builds (for most queries: the cell edge is not the spacing)
    cell, dims, h = C.grid_cells(Y)
    assert dims.prod() <= 520 and (dims > 1).all() and h != C.SPACING
    d = X[:, None, :].astype(np.float64) - Y[None, :, :]
    D = (d * d).sum(axis=2)
    for name, ways in (("edge", 2), ("face", 4), ("cell", 8)):
        split = 0
        for q in np.flatnonzero(kind == name):
            tied = np.flatnonzero(D[q] == D[q].min())
            split += len({tuple(c) for c in cell[tied]}) > 1
            assert tied[0] == i64[q]
        print(f"{name}: {split} of {(kind == name).sum()} queries have their {ways} tied rows in more than one cell (cells {dims}, h {h:.4f})")
        assert split >= 10, name
    # the first arg-min is not the lowest lattice position: the row order is a permutation, so "first" is a property of the order
    assert (i64[kind == "cell"] != np.sort(i64[kind == "cell"])).any()
    # half a spacing is the distance of the edge midpoints, exactly: the two gates of the GPU test fall either side of it
    assert (np.sqrt(d32[kind == "edge"]) == C.HALF).all()
