"""GPU: the k-best walk over the grid index (rap_amd/csrc/nn_knn.hip) and the three entry points built on it.

rap_k_nearest_neighbors is compared EXACTLY (rows, distance bits, counts) with the numpy yardstick of tests/knn_cases.py on inputs whose
fp32 distances are exact; the grid path of the normal estimation is held to the bound of the brute-force one (2e-6 against the fp64
yardstick of tests/icp_plane_oracle.py, tests/test_normals_gpu.py) on inputs whose neighbour sets the yardstick proves apart
(tests/test_knn_cases_host.py, tests/test_normals_host.py); the grid path of the outlier removal is bit-identical to the brute-force entry
on the exact inputs and held to that entry's rule against the fp64 KD-tree oracle on the others (tests/test_preproc_scale_gpu.py's
check_outliers, restated).  Every comparison prints its figures before it asserts (run with -s)."""
import numpy as np
import pytest
import torch

import icp_plane_oracle as P
import knn_cases as C
import rap_amd
from oracle import preproc_cases as PC
from oracle import rap_oracle as O
from rap_amd import _lib
from rap_amd.point_sampling import remove_statistical_outlier
from test_normals_gpu import TOL, batch, deviation, seg_tensor

pytestmark = pytest.mark.gpu

RAP_OK, RAP_ERR_INVALID, RAP_ERR_WORKSPACE = 0, -1, -2
I32 = torch.int32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def knn_gpu(dev, X, x_rows, Y, y_rows, k, max_distance=None):
    idx, d2, cnt = rap_amd.k_nearest_neighbors_packed(torch.from_numpy(X).to(dev), seg_tensor(dev, x_rows), torch.from_numpy(Y).to(dev),
                                                      seg_tensor(dev, y_rows), k, max_distance)
    return idx.cpu().numpy(), d2.cpu().numpy(), cnt.cpu().numpy()


def assert_same(got, want, tag, y_start=0):
    """idx, d2 bits and count, exactly; `want` indexes the y segment"""
    idx, d2, cnt = want
    idx = np.where(idx >= 0, idx + y_start, -1)
    bad = np.nonzero((got[0] != idx).any(axis=1) | (bits(got[1]) != bits(d2)).any(axis=1) | (got[2] != cnt))[0]
    assert bad.size == 0, (tag, f"{bad.size} rows differ; first {int(bad[0])}: got {got[0][bad[0]].tolist()} {got[1][bad[0]].tolist()} "
                           f"count {int(got[2][bad[0]])}, want {idx[bad[0]].tolist()} {d2[bad[0]].tolist()} count {int(cnt[bad[0]])}")


# ---------------------------------------------------------------------------------------------
# rap_k_nearest_neighbors
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lattice7", "lattice7_dup", "flat19", "line40", "copies33", "single"])
def test_knn_equals_the_yardstick_exactly_on_every_exact_input(dev, name):
    """A self-search of the whole cloud at every list size (k exceeds the short clouds), then with max_distance equal to a distance
    that occurs (the lattice spacing: inclusive) and smaller than a cell (0.25: the row and its copies only)."""
    Y = C.exact_inputs()[name]
    n = Y.shape[0]
    for k in C.KS:
        assert_same(knn_gpu(dev, Y, [[0, n]], Y, [[0, n]], k), C.knn(Y, Y, k), (name, k))
    for k, r in ((12, 0.75), (20, 0.5), (32, 0.75), (3, 0.25)):
        want = C.knn(Y, Y, k, r)
        assert_same(knn_gpu(dev, Y, [[0, n]], Y, [[0, n]], k, r), want, (name, k, r))
        print(f"{name} k {k} max_distance {r}: counts {want[2].min()} .. {want[2].max()}")
    if name == "lattice7":                                                # the six rows at exactly one spacing are in, nothing beyond
        idx, d2, cnt = knn_gpu(dev, Y, [[0, n]], Y, [[0, n]], 12, 0.75)
        assert cnt.max() == 7 and cnt.min() == 4 and d2[cnt == 7][:, 1:7].min() == 0.5625 == d2[cnt == 7][:, 1:7].max()


def test_knn_with_queries_inside_on_and_far_outside_the_box_and_non_finite_rows(dev):
    Y = np.concatenate([C.exact_inputs()["lattice7"], np.asarray([[np.nan, 0, 0], [0.5, np.inf, 0.25]], np.float32)])
    Y = Y[np.random.default_rng(3).permutation(Y.shape[0])]
    X = np.concatenate([C.exact_queries(), np.asarray([[0, np.nan, 0], [-np.inf, 0, 0], [0.25, 0.5, 0.75]], np.float32)])
    nx, ny = X.shape[0], Y.shape[0]
    for k in C.KS:
        for r in (None, 0.75, 46.0):
            want = C.knn(X, Y, k, r)
            assert_same(knn_gpu(dev, X, [[0, nx]], Y, [[0, ny]], k, r), want, (k, r))
    want = C.knn(X, Y, 20)
    bad_rows = np.nonzero(~np.isfinite(Y).all(axis=1))[0]
    assert (want[2][:-3] == 20).all() and want[2][-3:].tolist() == [0, 0, 20] and not np.isin(want[0], bad_rows).any()


def segments_case():
    """-> X, x rows, Y, y rows, per problem (x start, x len, y start, y len): six problems over packed arrays with junk between them --
    two that share one y segment, an empty x segment, an empty y segment, an x segment past the array, a table in no order"""
    E, rng = C.exact_inputs(), np.random.default_rng(21)
    junk = lambda m: (rng.integers(-40, 41, (m, 3)) * 0.25).astype(np.float32)
    Y = np.concatenate([junk(3), E["flat19"], junk(2), E["lattice7"]])
    yf, yl = 3, 3 + 361 + 2
    X = np.concatenate([junk(4), C.exact_queries(), junk(2), E["lattice7_dup"], junk(3), E["flat19"][:50], junk(1), E["line40"][:10]])
    xq, xd = 4, 4 + 160 + 2
    xf = xd + 343 + 3
    xl = xf + 50 + 1
    x_rows = [[xd, 343], [60, 0], [xl, 10], [X.shape[0] + 7, 20], [xq, 160], [xf, 50]]
    y_rows = [[yl, 343], [yf, 361], [yf + 5, 0], [yf, 361], [yl, 343], [yf, 361]]
    live = [(xd, 343, yl, 343), (xl, 10, 0, 0), (xq, 160, yl, 343), (xf, 50, yf, 361)]
    return X, x_rows, Y, y_rows, live


def knn_abi(dev, X, x_rows, Y, y_rows, k, r, ws_short=0):
    """through the C ABI into buffers that hold a pattern -> (rc, idx, d2, count) on the CPU"""
    lib = _lib.load()
    Xd, Yd = torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev)
    K, NX, NY = len(x_rows), X.shape[0], Y.shape[0]
    idx = torch.full((NX, k), -7, dtype=I32, device=dev)
    d2 = torch.full((NX, k), -3.25, dtype=torch.float32, device=dev)
    cnt = torch.full((NX,), -9, dtype=I32, device=dev)
    need = lib.rap_knn_workspace_bytes(NX, NY, K)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    xs, ys = seg_tensor(dev, x_rows), seg_tensor(dev, y_rows)             # named: two temporaries would share one block of the allocator
    rc = lib.rap_k_nearest_neighbors(_lib.ptr(Xd), _lib.ptr(xs), _lib.ptr(Yd), _lib.ptr(ys), K, NX, NY, k,
                                     r, _lib.ptr(idx), _lib.ptr(d2), _lib.ptr(cnt), _lib.ptr(ws), need - ws_short, _lib.current_stream(dev))
    torch.cuda.synchronize()
    return rc, idx.cpu().numpy(), d2.cpu().numpy(), cnt.cpu().numpy()


def test_knn_over_ragged_shared_and_empty_segments_leaves_other_rows_alone(dev):
    X, x_rows, Y, y_rows, live = segments_case()
    for k, r in ((1, 0.0), (12, 0.0), (21, 1.5), (32, 0.0)):
        rc, idx, d2, cnt = knn_abi(dev, X, x_rows, Y, y_rows, k, r)
        assert rc == RAP_OK
        covered = np.zeros(X.shape[0], bool)
        for xs, xn, ys, yn in live:
            want = C.knn(X[xs:xs + xn], Y[ys:ys + yn], k, r)
            assert_same((idx[xs:xs + xn], d2[xs:xs + xn], cnt[xs:xs + xn]), want, (k, r, xs), y_start=ys)
            covered[xs:xs + xn] = True
        assert (idx[~covered] == -7).all() and (d2[~covered] == -3.25).all() and (cnt[~covered] == -9).all()
        assert (cnt[live[1][0]:live[1][0] + 10] == 0).all()               # the empty y segment: written, and empty
    # the wrapper fills what the call leaves alone
    got = knn_gpu(dev, X, x_rows, Y, y_rows, 3)
    assert (got[0][~covered] == -1).all() and np.isinf(got[1][~covered]).all() and (got[2][~covered] == 0).all()


def test_knn_searches_an_overlapping_unequal_segment_row_by_row_and_still_exactly(dev):
    """y segments [0,300) and [1,300) of 300 rows: the second no longer fits the index's budget of n_y_points rows"""
    Y = C.exact_inputs()["lattice7"][:300]
    X = np.concatenate([C.exact_queries(), C.exact_inputs()["lattice7_dup"][:100]])
    for k in (1, 12, 32):
        for r in (None, 0.75):
            got = knn_gpu(dev, X, [[0, 160], [160, 100]], Y, [[0, 300], [1, 300]], k, r)      # the table's (1, 300) clamps to 299 rows
            assert_same([g[:160] for g in got], C.knn(X[:160], Y, k, r), ("indexed", k, r))
            assert_same([g[160:] for g in got], C.knn(X[160:], Y[1:], k, r), ("row by row", k, r), y_start=1)


def test_knn_with_one_slot_is_nearest_neighbors_bit_for_bit(dev):
    X, x_rows, Y, y_rows, _ = segments_case()
    cases = [(X, x_rows, Y, y_rows), (P.normals_input(3, 300), [[0, 300]], P.sweep_lattice(513), [[0, 513]]),
             (C.two_cluster(), [[0, 310]], C.two_cluster(), [[5, 300]])]
    for Xc, xr, Yc, yr in cases:
        for r in (None, 0.6):
            idx, d2, cnt = knn_gpu(dev, Xc, xr, Yc, yr, 1, r)
            i1, d1 = rap_amd.nearest_neighbors_packed(torch.from_numpy(Xc).to(dev), seg_tensor(dev, xr), torch.from_numpy(Yc).to(dev),
                                                      seg_tensor(dev, yr), max_distance=r)
            assert np.array_equal(idx[:, 0], i1.cpu().numpy()) and np.array_equal(bits(d2[:, 0]), bits(d1.cpu().numpy()))
            assert np.array_equal(cnt, (i1.cpu().numpy() >= 0).astype(np.int32))


def test_knn_call_contract(dev):
    Y = C.exact_inputs()["flat19"]
    assert knn_abi(dev, Y, [[0, 361]], Y, [[0, 361]], 0, 0.0)[0] == RAP_ERR_INVALID
    assert knn_abi(dev, Y, [[0, 361]], Y, [[0, 361]], 33, 0.0)[0] == RAP_ERR_INVALID
    rc, idx, d2, cnt = knn_abi(dev, Y, [[0, 361]], Y, [[0, 361]], 20, 0.0, ws_short=1)
    assert rc == RAP_ERR_WORKSPACE and (idx == -7).all() and (d2 == -3.25).all() and (cnt == -9).all()
    a, b = knn_abi(dev, Y, [[0, 361]], Y, [[0, 361]], 20, 0.0), knn_abi(dev, Y, [[0, 361]], Y, [[0, 361]], 20, 0.0)
    assert a[0] == RAP_OK and all(np.array_equal(u, v) for u, v in zip(a[1:], b[1:]))
    Y_d, seg = torch.from_numpy(Y).to(dev), seg_tensor(dev, [[0, 361]])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                               # no host synchronisation in the call
    try:
        got = rap_amd.k_nearest_neighbors_packed(Y_d, seg, Y_d, seg, 20)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert np.array_equal(got[0].cpu().numpy(), a[1])


# ---------------------------------------------------------------------------------------------
# estimate_normals_packed(search="grid")
# ---------------------------------------------------------------------------------------------
def normals(dev, pts, rows, search="grid", **kw):
    n, e = rap_amd.estimate_normals_packed(torch.from_numpy(pts).to(dev), seg_tensor(dev, rows), return_eigenvalues=True, search=search, **kw)
    return n.cpu(), e.cpu()


def check_normals(dev, pts, ref, tag, signed=False, **kw):
    """grid path against the yardstick `ref` = (normals, eigenvalues, counts, gap) within TOL; zero rows exactly where counts < 3"""
    ref_n, ref_e, counts = ref[0], ref[1], ref[2]
    n, e = normals(dev, pts, [[0, pts.shape[0]]], **kw)
    bn, be = normals(dev, pts, [[0, pts.shape[0]]], search="brute", **kw)
    dn, de = deviation(n, e, ref_n, ref_e, signed)
    vs = max(float((n - bn).abs().max()), float(((e - be).abs() / be[:, 2:3].clamp(min=1e-30)).max())) if pts.shape[0] else 0.0
    print(f"{tag}: worst |dn| {dn:.2e}, |d lambda| / lambda_max {de:.2e} (bound {TOL:.0e}); worst deviation from search='brute' {vs:.2e}; "
          f"{int((counts < 3).sum())} rows without an estimate")
    assert dn <= TOL and de <= TOL, tag
    none = counts < 3
    zero = ~(n.numpy().any(axis=1) | e.numpy().any(axis=1))
    assert np.array_equal(zero, none), tag
    return n, e


@pytest.mark.parametrize("length", P.SWEEP_LENGTHS)
def test_grid_normals_edge_sweep_over_segment_lengths_and_list_sizes(dev, length):
    pts = P.sweep_lattice(length)
    for k in P.SWEEP_MAX_NN:
        check_normals(dev, pts, P.estimate_normals(pts, k, 0.0), f"length {length} max_nn {k}", max_nn=k, radius=0.0)
    check_normals(dev, pts, P.estimate_normals(pts, 12, P.SWEEP_RADIUS), f"length {length} radius {P.SWEEP_RADIUS}", max_nn=12, radius=P.SWEEP_RADIUS)


def test_grid_normals_match_the_yardstick_under_both_orientation_rules(dev):
    c = P.NORMALS_CASE
    pts = P.normals_input(c["seed"], c["n"])
    ref = P.normals_solved(c["seed"], c["n"], c["max_nn"], c["radius"])
    n, e = check_normals(dev, pts, ref, "no viewpoint", max_nn=c["max_nn"], radius=c["radius"])
    a = np.sort(np.abs(ref[0]), axis=1)
    clear = a[:, 2] - a[:, 1] > 1e-3                                   # the sign rule, where the largest component is the largest by a margin
    assert clear.sum() > c["n"] // 2 and np.abs(n.double().numpy() - ref[0])[clear].max() <= TOL
    ref_v = P.normals_solved(c["seed"], c["n"], c["max_nn"], c["radius"], P.VIEWPOINT)
    nv, ev = check_normals(dev, pts, ref_v, "viewpoint", signed=True, max_nn=c["max_nn"], radius=c["radius"], viewpoint=torch.tensor(P.VIEWPOINT))
    assert torch.equal(ev, e)
    nd, _ = normals(dev, pts, [[0, c["n"]]], max_nn=c["max_nn"], radius=c["radius"], viewpoint=torch.tensor(tuple(-v for v in P.VIEWPOINT)))
    assert torch.equal(nd, -nv)
    one = rap_amd.estimate_point_normals(torch.from_numpy(pts).to(dev), k_neighbors=c["max_nn"], radius=c["radius"], search="grid")
    assert torch.equal(one.cpu(), n)


def test_grid_normals_on_two_clusters_forty_units_apart(dev):
    pts = C.two_cluster()
    for k, r in C.TWO_CLUSTER_SETTINGS:
        check_normals(dev, pts, P.estimate_normals(pts, k, r), f"two clusters max_nn {k} radius {r}", max_nn=k, radius=r)


def test_grid_normals_ragged_batch_equals_solo_runs_and_any_order_bit_for_bit(dev):
    """what the canonical order of the list is for: call = call, batch = solo, and the batch with its table in another order"""
    pts, rows, parts = batch(dev)
    P_d = torch.from_numpy(pts).to(dev)
    i32 = lambda t: t.cpu().view(torch.int32)
    for kw in (dict(max_nn=12, radius=0.0), dict(max_nn=20, radius=0.5)):
        lib_n, lib_e = rap_amd.estimate_normals_packed(P_d, seg_tensor(dev, rows), return_eigenvalues=True, search="grid", **kw)
        again = rap_amd.estimate_normals_packed(P_d, seg_tensor(dev, rows), return_eigenvalues=True, search="grid", **kw)
        assert torch.equal(i32(lib_n), i32(again[0])) and torch.equal(i32(lib_e), i32(again[1]))
        other = rap_amd.estimate_normals_packed(P_d, seg_tensor(dev, [rows[i] for i in (4, 2, 3, 0, 1)]), return_eigenvalues=True, search="grid", **kw)
        assert torch.equal(i32(lib_n), i32(other[0])) and torch.equal(i32(lib_e), i32(other[1]))
        covered = np.zeros(pts.shape[0], bool)
        for k, cloud, start in parts:
            solo_n, solo_e = normals(dev, cloud, [[0, cloud.shape[0]]], **kw)
            assert torch.equal(i32(lib_n[start:start + cloud.shape[0]]), solo_n.view(torch.int32)), k
            assert torch.equal(i32(lib_e[start:start + cloud.shape[0]]), solo_e.view(torch.int32)), k
            covered[start:start + cloud.shape[0]] = True
        assert not lib_n.cpu().numpy()[~covered].any() and bool(torch.isfinite(lib_n).all())
    k, B, b = parts[1]                                                  # the NaN row: no estimate, and nobody's neighbour
    ref = P.estimate_normals(B, 12, 0.0)
    lib_n, lib_e = rap_amd.estimate_normals_packed(P_d, seg_tensor(dev, rows), max_nn=12, radius=0.0, return_eigenvalues=True, search="grid")
    dn, de = deviation(lib_n[b:b + 255].cpu(), lib_e[b:b + 255].cpu(), ref[0], ref[1], signed=False)
    print(f"segment with a NaN row: worst |dn| {dn:.2e}")
    assert ref[2][17] == 0 and not lib_n[b + 17].cpu().any() and dn <= TOL and de <= TOL
    # rows outside every segment are not written: through the C ABI, into buffers that hold a pattern
    lib = _lib.load()
    N = pts.shape[0]
    out = torch.full((N, 3), 7.5, dtype=torch.float32, device=dev)
    eig = torch.full((N, 3), -3.25, dtype=torch.float32, device=dev)
    ws = torch.empty(lib.rap_normals_grid_workspace_bytes(N, len(rows)), dtype=torch.uint8, device=dev)
    seg = seg_tensor(dev, rows)
    rc = lib.rap_estimate_normals_grid(_lib.ptr(P_d), _lib.ptr(seg), len(rows), N, 12, 0.0, None, _lib.ptr(out), _lib.ptr(eig),
                                       _lib.ptr(ws), ws.numel(), _lib.current_stream(dev))
    torch.cuda.synchronize()
    assert rc == RAP_OK
    out, eig = out.cpu(), eig.cpu()
    assert (out[~covered] == 7.5).all() and (eig[~covered] == -3.25).all()
    assert torch.equal(out[covered].view(torch.int32), lib_n.cpu()[covered].view(torch.int32))


def test_grid_normals_make_no_host_synchronisation_and_replay_from_a_graph(dev):
    pts, rows, _ = batch(dev)
    P_d, seg = torch.from_numpy(pts).to(dev), seg_tensor(dev, rows)
    vp = torch.tensor(P.VIEWPOINT, device=dev)
    call = lambda: rap_amd.estimate_normals_packed(P_d, seg, max_nn=20, radius=0.5, viewpoint=vp, return_eigenvalues=True, search="grid")
    want = [t.cpu().view(torch.int32).clone() for t in call()]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = call()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(torch.equal(g.cpu().view(torch.int32), w) for g, w in zip(got, want))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    for t in out:
        t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(g.cpu().view(torch.int32), w) for g, w in zip(out, want))


# ---------------------------------------------------------------------------------------------
# remove_statistical_outlier(search="grid")
# ---------------------------------------------------------------------------------------------
def outliers_abi(dev, pts, k, ratio, grid=True, ws_short=0):
    """rap_statistical_outliers[_grid] with stats_out -> (rc, inlier indices (CPU), count, stats bits as int64)"""
    lib = _lib.load()
    p = torch.as_tensor(pts).float().to(dev).contiguous()
    N = p.shape[0]
    idx = torch.full((N,), -7, dtype=torch.int64, device=dev)
    count = torch.full((1,), -7, dtype=I32, device=dev)
    stats = torch.full((3,), float("nan"), dtype=torch.float64, device=dev)
    need = (lib.rap_outlier_grid_workspace_bytes if grid else lib.rap_outlier_workspace_bytes)(N)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    entry = lib.rap_statistical_outliers_grid if grid else lib.rap_statistical_outliers
    rc = entry(_lib.ptr(p), N, int(k), float(ratio), _lib.ptr(idx), _lib.ptr(count), _lib.ptr(stats), _lib.ptr(ws), need - ws_short,
               _lib.current_stream(dev))
    torch.cuda.synchronize(dev)
    if rc != RAP_OK:
        return rc, idx.cpu(), int(count.cpu()), None
    return rc, idx[: int(count.cpu())].cpu(), int(count.cpu()), stats.cpu()


@pytest.mark.parametrize("name", ["lattice7", "lattice7_dup", "flat19", "line40", "copies33", "single"])
def test_grid_outlier_removal_equals_the_brute_entry_bit_for_bit_on_exact_inputs(dev, name):
    pts = C.exact_inputs()[name]
    for k in C.OUTLIER_KS:
        for ratio in (0.5, 2.0):
            g, b = outliers_abi(dev, pts, k, ratio), outliers_abi(dev, pts, k, ratio, grid=False)
            assert g[0] == RAP_OK == b[0]
            print(f"{name} k {k} ratio {ratio}: kept {g[2]} of {pts.shape[0]} (brute {b[2]}), stats {g[3].tolist()}")
            assert g[2] == b[2] and torch.equal(g[1], b[1]) and torch.equal(g[3].view(torch.int64), b[3].view(torch.int64)), (name, k, ratio)
    if name == "copies33":
        assert outliers_abi(dev, pts, 20, 2.0)[2] == 0                    # every mean distance is 0: nothing is kept


def check_outliers(dev, pts, k, ratio, tag):
    """tests/test_preproc_scale_gpu.py's rule for the brute-force entry, restated for the grid one: against O.remove_statistical_outlier
    (fp64 KD-tree) only points within 1e-4 (relative) of the threshold may differ, that edge set is at most 0.5 % of N (a condition on
    the inputs, from the oracle alone), and stats_out is within 1e-6 relative of the oracle's fp64 values"""
    n = pts.shape[0]
    ref_idx, avg = O.remove_statistical_outlier(pts.float().numpy(), k, ratio)
    pos = avg > 0
    mean = avg[pos].sum() / n
    std = np.sqrt(((avg[pos] - mean) ** 2).sum() / (n - 1)) if n > 1 else 0.0
    thr = mean + ratio * std
    edge = set(np.nonzero(np.abs(avg - thr) < 1e-4 * thr)[0].tolist())
    assert len(edge) <= 0.005 * n, (tag, len(edge), n)
    rc, idx, count, stats = outliers_abi(dev, pts, k, ratio)
    assert rc == RAP_OK
    got, want = set(idx.tolist()), set(ref_idx.tolist())
    rel = [abs(s - r) / r if r > 0 else abs(s) for s, r in zip(stats.tolist(), (mean, std, thr))]
    print(f"grid outliers {tag}: N={n} k={k} kept {len(got)} (oracle {len(want)}), edge set {len(edge)} ({100 * len(edge) / n:.3f} %), "
          f"stats rel err mean {rel[0]:.1e} std {rel[1]:.1e} thr {rel[2]:.1e}")
    assert (got ^ want) <= edge, (tag, sorted(got ^ want)[:5])
    assert idx.tolist() == sorted(got) and len(got) == idx.numel() == count
    assert max(rel) < 1e-6, (tag, rel)


@pytest.mark.parametrize("n,seed", [(1023, 0), (1025, 2), (2049, 4)])
def test_grid_outlier_removal_against_the_kd_tree_oracle(dev, n, seed):
    pts = PC.outlier_cloud(n, seed)
    for k in (2, 20, 21, 32):
        check_outliers(dev, pts, k, 2.0, f"n={n}")


def test_grid_outlier_removal_with_duplicate_points(dev):
    pts = PC.outlier_cloud(3000, 7)
    pts[2100:] = pts[:900]
    pts = pts[torch.randperm(3000, generator=torch.Generator().manual_seed(1))]
    for k in (2, 20, 21):
        check_outliers(dev, pts, k, 2.0, "30% duplicates")


def test_grid_outlier_removal_with_fewer_points_than_neighbours(dev):
    g = torch.Generator().manual_seed(9)
    pts = torch.rand(5, 3, generator=g)
    pts[4] = torch.tensor([9.0, 9.0, 9.0])
    for ratio in (0.5, 1.0, 2.5):
        ref_idx, _ = O.remove_statistical_outlier(pts.numpy(), 20, ratio)
        check_outliers(dev, pts, 20, ratio, "n=5")
        filt, idx = remove_statistical_outlier(pts.to(dev), nb_neighbors=20, std_ratio=ratio, search="grid")
        assert idx.cpu().tolist() == ref_idx.tolist() and torch.equal(filt.cpu(), pts[idx.cpu()])


def test_grid_outlier_removal_call_contract(dev):
    pts = PC.outlier_cloud(1500, 4)
    assert outliers_abi(dev, pts, 0, 2.5)[0] == RAP_ERR_INVALID
    assert outliers_abi(dev, pts, 33, 2.5)[0] == RAP_ERR_INVALID
    assert outliers_abi(dev, pts, 32, 2.5)[0] == RAP_OK
    rc, idx, count, _ = outliers_abi(dev, pts, 20, 2.5, ws_short=1)
    assert rc == RAP_ERR_WORKSPACE and (idx == -7).all() and count == -7
    a, b = outliers_abi(dev, pts, 20, 2.5), outliers_abi(dev, pts, 20, 2.5)
    assert torch.equal(a[1], b[1]) and torch.equal(a[3].view(torch.int64), b[3].view(torch.int64))
    filt, idx = remove_statistical_outlier(pts.to(dev), search="grid")                   # the wrapper's defaults: 20 neighbours, ratio 2.5
    assert torch.equal(idx.cpu(), a[1]) and torch.equal(filt.cpu(), pts[a[1]])
