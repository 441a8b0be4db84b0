"""Guard-band tests of rap_k_nearest_neighbors, rap_estimate_normals_grid and rap_statistical_outliers_grid through the C ABI: outputs
sized exactly between guard bytes, the workspace at exactly the queried bytes and 0xFF-filled, a short workspace refused without a byte
written, results independent of what lies beyond the inputs.  Harness and limits: tests/test_guards_gpu.py and tests/guards.py (an
overrun longer than the pad and a read that reaches no result are not seen)."""
import ctypes

import numpy as np
import pytest
import torch

import icp_plane_oracle as P
import knn_cases as C
from rap_amd import _lib
from test_guards_gpu import F32, I32, I64, refused_call_wrote_nothing, run_both, stream
from test_knn_gpu import assert_same, segments_case
from test_normals_gpu import TOL, batch, deviation

pytestmark = pytest.mark.gpu

P2 = ctypes.c_void_p
F64 = torch.float64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.mark.parametrize("k", [3, 32])
def test_k_nearest_neighbors_writes_only_the_rows_of_its_segments_and_its_exact_workspace(lib, dev, k):
    """the segments of tests/test_knn_gpu.py, whose X and Y both END with a segment: the last query and the last candidate lie against
    the back guard"""
    X, x_rows, Y, y_rows, live = segments_case()
    assert X.shape[0] == live[1][0] + 10                                # X ends with the ten queries of problem 2
    NX, NY, K = X.shape[0], Y.shape[0], len(x_rows)                     # Y ends with the lattice
    Xt, Yt = torch.from_numpy(X), torch.from_numpy(Y)
    xs, ys = torch.tensor(x_rows, dtype=I32), torch.tensor(y_rows, dtype=I32)
    need = lib.rap_knn_workspace_bytes(NX, NY, K)
    want = [(a, n, b, C.knn(X[a:a + n], Y[b:b + m], k)) for a, n, b, m in live]

    def call(c, short=0):
        idx, d2, cnt = c.out_view(I32, (NX, k), "idx_out"), c.out_view(F32, (NX, k), "d2_out"), c.out_view(I32, (NX,), "count_out")
        ws = c.out(need, name="knn workspace")
        rc = lib.rap_k_nearest_neighbors(_lib.ptr(c.inp(Xt)), _lib.ptr(c.inp(xs)), _lib.ptr(c.inp(Yt)), _lib.ptr(c.inp(ys)), K, NX, NY, k, 0.0,
                                         _lib.ptr(idx), _lib.ptr(d2), _lib.ptr(cnt), P2(ws.ptr), need - short, stream(dev))
        torch.cuda.synchronize()
        return rc, idx, d2, cnt

    def run(c):
        rc, idx, d2, cnt = call(c)
        assert rc == 0
        i, d, n = idx.cpu().numpy(), d2.cpu().numpy(), cnt.cpu().numpy()
        covered = np.zeros(NX, bool)
        for a, m, b, w in want:
            assert_same((i[a:a + m], d[a:a + m], n[a:a + m]), w, (k, a), y_start=b)
            covered[a:a + m] = True
        assert (i[~covered] == -1).all() and (d2.view(I32).cpu().numpy()[~covered] == -1).all() and (n[~covered] == -1).all()      # the 0xFF fill
        return [idx, d2, cnt]
    run_both(dev, run)
    refused_call_wrote_nothing(dev, call)


def test_estimate_normals_grid_writes_only_the_rows_of_its_segments_and_its_exact_workspace(lib, dev):
    pts, rows, parts = batch(dev)
    pts = pts[:-5]                                                      # the last segment ends the array
    N, K = pts.shape[0], len(rows)
    Pt, seg = torch.from_numpy(pts), torch.tensor(rows, dtype=I32)
    vp = torch.tensor([P.VIEWPOINT] * K, dtype=F32)
    need = lib.rap_normals_grid_workspace_bytes(N, K)
    assert need > lib.rap_normals_workspace_bytes(N, K) > 0
    refs = [(start, cloud.shape[0], P.estimate_normals(cloud, 12, 0.0, P.VIEWPOINT)) for _, cloud, start in parts]

    def call(c, short=0, with_eig=True):
        nrm = c.out_view(F32, (N, 3), "normals")
        eig = c.out_view(F32, (N, 3), "eigenvalues") if with_eig else None
        ws = c.out(need, name="normals grid workspace")
        rc = lib.rap_estimate_normals_grid(_lib.ptr(c.inp(Pt)), _lib.ptr(c.inp(seg)), K, N, 12, 0.0, _lib.ptr(c.inp(vp)), _lib.ptr(nrm),
                                           _lib.ptr(eig), P2(ws.ptr), need - short, stream(dev))
        torch.cuda.synchronize()
        return rc, nrm, eig

    def run_with(with_eig):
        def run(c):
            rc, nrm, eig = call(c, with_eig=with_eig)
            assert rc == 0
            covered = np.zeros(N, bool)
            for start, n, ref in refs:
                e = eig[start:start + n].cpu() if with_eig else torch.from_numpy(ref[1]).float()
                dn, de = deviation(nrm[start:start + n].cpu(), e, ref[0], ref[1], signed=False)
                assert dn <= TOL and de <= TOL, (start, dn, de)
                covered[start:start + n] = True
            assert (nrm.view(I32).cpu().numpy()[~covered] == -1).all()                     # still the 0xFF fill: never written
            return [nrm, eig] if with_eig else [nrm]
        return run
    run_both(dev, run_with(True))
    run_both(dev, run_with(False))
    refused_call_wrote_nothing(dev, call)


@pytest.mark.parametrize("n,k", [(1025, 20), (343, 32)])
def test_statistical_outliers_grid_writes_only_its_outputs_and_its_exact_workspace(lib, dev, n, k):
    """inlier_indices sized exactly N; against the brute-force entry on an exact input (343: the lattice with duplicates, bit for bit)
    and by the kept count on a float one"""
    from oracle import preproc_cases as PC
    pts = torch.from_numpy(C.exact_inputs()["lattice7_dup"]) if n == 343 else PC.outlier_cloud(n, 2).float()
    need = lib.rap_outlier_grid_workspace_bytes(n)
    assert need > lib.rap_outlier_workspace_bytes(n) > 0
    p_d = pts.to(dev).contiguous()
    b_idx, b_cnt, b_stats = torch.empty(n, dtype=I64, device=dev), torch.empty(1, dtype=I32, device=dev), torch.empty(3, dtype=F64, device=dev)
    b_ws = torch.empty(lib.rap_outlier_workspace_bytes(n), dtype=torch.uint8, device=dev)
    assert lib.rap_statistical_outliers(_lib.ptr(p_d), n, k, 2.0, _lib.ptr(b_idx), _lib.ptr(b_cnt), _lib.ptr(b_stats), _lib.ptr(b_ws),
                                        b_ws.numel(), stream(dev)) == 0
    torch.cuda.synchronize()
    kept = int(b_cnt.cpu())

    def call(c, short=0):
        idx, cnt, stats = c.out_view(I64, (n,), "inlier_indices"), c.out_view(I32, (1,), "count_out"), c.out_view(F64, (3,), "stats_out")
        ws = c.out(need, name="outlier grid workspace")
        rc = lib.rap_statistical_outliers_grid(_lib.ptr(c.inp(pts)), n, k, 2.0, _lib.ptr(idx), _lib.ptr(cnt), _lib.ptr(stats), P2(ws.ptr),
                                               need - short, stream(dev))
        torch.cuda.synchronize()
        return rc, idx, cnt, stats

    def run(c):
        rc, idx, cnt, stats = call(c)
        assert rc == 0
        m = int(cnt.cpu())
        assert (idx[m:].cpu() == -1).all() and bool((idx[:m].cpu()[1:] > idx[:m].cpu()[:-1]).all())      # ascending; the rest never written
        if n == 343:
            assert m == kept and torch.equal(idx[:m].cpu(), b_idx[:kept].cpu()) and torch.equal(stats.cpu().view(I64), b_stats.cpu().view(I64))
        else:
            # both entries may differ from the fp64 oracle inside its edge set only (<= 0.5 % of N on this input) and by 1e-6 in the statistics
            assert abs(m - kept) <= 0.005 * n and torch.allclose(stats.cpu(), b_stats.cpu(), rtol=2e-6, atol=0)
        return [idx, cnt, stats]
    run_both(dev, run)
    refused_call_wrote_nothing(dev, call)
