"""GPU: the normal estimation (rap_amd/csrc/normals.hip, rap_amd/normals.py) against its fp64 yardstick (tests/icp_plane_oracle.py).

Bound: 2e-6 absolute per component of a normal, and 2e-6 of the largest eigenvalue for the eigenvalues -- the class and the bound of
fit_transformations (tests/test_kernels_gpu.py): the core is fp64 and the result is rounded to fp32 (6e-8).  It holds only where the
device and the yardstick pick the same neighbours, which tests/test_normals_host.py asserts for every input used here (no neighbour
set within 1e-5 of another one; the fp32 distances of the two differ by one rounding, ~1e-8).  Every test prints its worst deviation
before it asserts (run with -s to see them)."""
import numpy as np
import pytest
import torch

import icp_plane_oracle as P
import rap_amd

pytestmark = pytest.mark.gpu

TOL = 2e-6


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def seg_tensor(dev, rows):
    return torch.tensor(rows, dtype=torch.int32, device=dev)


def run(dev, pts, rows, **kw):
    n, e = rap_amd.estimate_normals_packed(torch.from_numpy(pts).to(dev), seg_tensor(dev, rows), return_eigenvalues=True, **kw)
    return n.cpu(), e.cpu()


def deviation(n, e, ref_n, ref_e, signed):
    """-> worst |dn| (up to sign unless `signed`) and worst |de| / lambda_max over the rows"""
    n, e = n.double().numpy(), e.double().numpy()
    dn = np.abs(n - ref_n).max(axis=1)
    if not signed:
        dn = np.minimum(dn, np.abs(n + ref_n).max(axis=1))
    scale = np.maximum(ref_e[:, 2:3], 1e-300)
    return float(dn.max()), float((np.abs(e - ref_e) / scale).max())


def test_normals_match_the_yardstick_and_follow_both_orientation_rules(dev):
    c = P.NORMALS_CASE
    pts = P.normals_input(c["seed"], c["n"])
    ref_n, ref_e, _, _ = P.normals_solved(c["seed"], c["n"], c["max_nn"], c["radius"])
    n, e = run(dev, pts, [[0, c["n"]]], max_nn=c["max_nn"], radius=c["radius"])
    dn, de = deviation(n, e, ref_n, ref_e, signed=False)
    print(f"no viewpoint: worst |dn| up to sign {dn:.2e}, worst |d lambda| / lambda_max {de:.2e}")
    assert dn <= TOL and de <= TOL
    # the sign rule, on rows where the largest component is the largest by a margin
    a = np.sort(np.abs(ref_n), axis=1)
    clear = a[:, 2] - a[:, 1] > 1e-3
    assert clear.sum() > c["n"] // 2
    big = np.abs(ref_n).argmax(axis=1)
    got = n.numpy()[np.arange(c["n"]), big]
    assert (got[clear] > 0).all()
    assert np.abs(n.double().numpy() - ref_n)[clear].max() <= TOL
    # with a viewpoint the orientation is exact
    ref_v = P.normals_solved(c["seed"], c["n"], c["max_nn"], c["radius"], P.VIEWPOINT)[0]
    nv, ev = run(dev, pts, [[0, c["n"]]], max_nn=c["max_nn"], radius=c["radius"], viewpoint=torch.tensor(P.VIEWPOINT))
    dv, _ = deviation(nv, ev, ref_v, ref_e, signed=True)
    print(f"viewpoint: worst |dn| {dv:.2e}")
    assert dv <= TOL and torch.equal(ev, e)
    down = tuple(-v for v in P.VIEWPOINT)
    nd, _ = run(dev, pts, [[0, c["n"]]], max_nn=c["max_nn"], radius=c["radius"], viewpoint=torch.tensor(down))
    assert torch.equal(nd, -nv)
    # the single-cloud wrapper with the reference's signature
    one = rap_amd.estimate_point_normals(torch.from_numpy(pts).to(dev), k_neighbors=c["max_nn"], radius=c["radius"])
    assert torch.equal(one.cpu(), n)


@pytest.mark.parametrize("length", P.SWEEP_LENGTHS)
def test_edge_sweep_over_segment_lengths_and_list_sizes(dev, length):
    pts = P.sweep_lattice(length)
    for k in P.SWEEP_MAX_NN:                                          # max_nn > length for the short segments
        ref_n, ref_e, counts, _ = P.estimate_normals(pts, k, 0.0)
        n, e = run(dev, pts, [[0, length]], max_nn=k, radius=0.0)
        dn, de = deviation(n, e, ref_n, ref_e, signed=False)
        print(f"length {length} max_nn {k}: worst |dn| {dn:.2e}, |d lambda| / lambda_max {de:.2e}")
        assert dn <= TOL and de <= TOL
        if length < 3:
            assert not n.any() and not e.any()
    # a radius that leaves some rows with fewer than three neighbours: those get the zero normal
    ref_n, ref_e, counts, _ = P.estimate_normals(pts, 12, P.SWEEP_RADIUS)
    n, e = run(dev, pts, [[0, length]], max_nn=12, radius=P.SWEEP_RADIUS)
    dn, de = deviation(n, e, ref_n, ref_e, signed=False)
    print(f"length {length} radius {P.SWEEP_RADIUS}: worst |dn| {dn:.2e}; {(counts < 3).sum()} rows without an estimate")
    assert dn <= TOL and de <= TOL
    none = counts < 3
    assert not n.numpy()[none].any() and not e.numpy()[none].any()
    assert (np.abs(np.linalg.norm(n.double().numpy()[~none], axis=1) - 1.0) < 1e-6).all()


def batch(dev):
    """segments that are neither contiguous nor ordered, an empty one, one with a NaN row: [junk 7 | C 257 | junk 3 | A 300 | B 255 | junk 5]"""
    rng = np.random.default_rng(5)
    junk = lambda m: rng.uniform(-1, 1, (m, 3)).astype(np.float32)
    A, B, C = P.normals_input(3, 300), P.sweep_lattice(255).copy(), P.sweep_lattice(257)
    B[17] = (np.nan, 0.5, 0.5)
    pts = np.concatenate([junk(7), C, junk(3), A, B, junk(5)])
    a, b, c = 7 + 257 + 3, 7 + 257 + 3 + 300, 7
    rows = [[a, 300], [pts.shape[0] + 4, 9], [b, 255], [40, 0], [c, 257]]
    return pts, rows, ((0, A, a), (2, B, b), (4, C, c))


def test_ragged_batch_equals_solo_runs_bit_for_bit_and_leaves_other_rows_alone(dev):
    pts, rows, parts = batch(dev)
    P_d = torch.from_numpy(pts).to(dev)
    lib_n, lib_e = rap_amd.estimate_normals_packed(P_d, seg_tensor(dev, rows), max_nn=12, radius=0.0, return_eigenvalues=True)
    again = rap_amd.estimate_normals_packed(P_d, seg_tensor(dev, rows), max_nn=12, radius=0.0, return_eigenvalues=True)
    assert torch.equal(lib_n.cpu().view(torch.int32), again[0].cpu().view(torch.int32)) and torch.equal(lib_e.cpu().view(torch.int32), again[1].cpu().view(torch.int32))
    covered = np.zeros(pts.shape[0], bool)
    for k, cloud, start in parts:
        solo_n, solo_e = run(dev, cloud, [[0, cloud.shape[0]]], max_nn=12, radius=0.0)
        assert torch.equal(lib_n[start:start + cloud.shape[0]].cpu().view(torch.int32), solo_n.view(torch.int32)), k
        assert torch.equal(lib_e[start:start + cloud.shape[0]].cpu().view(torch.int32), solo_e.view(torch.int32)), k
        covered[start:start + cloud.shape[0]] = True
    # the NaN row: no estimate for it, and it is nobody's neighbour (the yardstick leaves it out too)
    k, B, b = parts[1]
    ref_n, ref_e, counts, gap = P.estimate_normals(B, 12, 0.0)
    assert counts[17] == 0 and not lib_n[b + 17].cpu().any() and gap.min() >= P.SWEEP_GAP
    dn, de = deviation(lib_n[b:b + 255].cpu(), lib_e[b:b + 255].cpu(), ref_n, ref_e, signed=False)
    print(f"segment with a NaN row: worst |dn| {dn:.2e}")
    assert dn <= TOL and de <= TOL and bool(torch.isfinite(lib_n).all())
    # rows outside every segment are not written: through the C ABI, into buffers that hold a pattern
    from rap_amd import _lib
    lib = _lib.load()
    N = pts.shape[0]
    out = torch.full((N, 3), 7.5, dtype=torch.float32, device=dev)
    eig = torch.full((N, 3), -3.25, dtype=torch.float32, device=dev)
    ws = torch.empty(lib.rap_normals_workspace_bytes(N, len(rows)), dtype=torch.uint8, device=dev)
    rc = lib.rap_estimate_normals(_lib.ptr(P_d), _lib.ptr(seg_tensor(dev, rows)), len(rows), N, 12, 0.0, None, _lib.ptr(out), _lib.ptr(eig), _lib.ptr(ws),
                                  ws.numel(), _lib.current_stream(dev))
    torch.cuda.synchronize()
    assert rc == 0
    out, eig = out.cpu(), eig.cpu()
    assert (out[~covered] == 7.5).all() and (eig[~covered] == -3.25).all()
    assert torch.equal(out[covered].view(torch.int32), lib_n.cpu()[covered].view(torch.int32))


def test_call_makes_no_host_synchronisation_and_replays_from_a_graph(dev):
    pts, rows, _ = batch(dev)
    P_d, seg = torch.from_numpy(pts).to(dev), seg_tensor(dev, rows)
    vp = torch.tensor(P.VIEWPOINT, device=dev)
    call = lambda: rap_amd.estimate_normals_packed(P_d, seg, max_nn=20, radius=0.5, viewpoint=vp, return_eigenvalues=True)
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
