"""Guard-band tests of rap_icp_plane, rap_icp_plane_grid and rap_estimate_normals through the C ABI: outputs sized exactly, the workspace
at exactly the queried bytes, a short workspace refused without a byte written, and results independent of what lies beyond the inputs.
Harness and limits: tests/test_guards_gpu.py and tests/guards.py (an overrun longer than the pad and a read that reaches no result are
not seen).  The same refusals without a GPU: tests/test_icp_plane_host.py and tests/test_normals_host.py."""
import ctypes

import numpy as np
import pytest
import torch

import icp_plane_oracle as P
from rap_amd import _lib
from test_guards_gpu import F32, I32, U8, refused_call_wrote_nothing, run_both, stream

pytestmark = pytest.mark.gpu

P2 = ctypes.c_void_p


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.mark.parametrize("grid", [False, True], ids=["brute", "grid"])
def test_icp_plane_writes_only_its_outputs_and_its_exact_workspace(lib, dev, grid):
    # three problems whose segments end exactly at the ends of X and of Y (a partial second item last in X, a candidate tile of 256 + 44
    # last in Y), a one-point problem, and an empty one whose table row points past the arrays (clamped on the device)
    (sa, na, ma), (sb, nb, mb) = P.PLANE_PAIRS
    Xb, Yb, Nb = P.pair(sb, nb, mb)
    Xa, Ya, Na = P.pair(sa, 300, 300)
    refs = [P.icp_plane(Xa, Ya, Na, margins=False), P.solved(sb, nb, mb)]
    X = torch.from_numpy(np.concatenate([Xb, Xb[:1], Xa]))
    Y = torch.from_numpy(np.concatenate([Yb, Ya]))
    Yn = torch.from_numpy(np.concatenate([Nb, Na]))
    NX, NY, K = X.shape[0], Y.shape[0], 4
    x_seg = torch.tensor([[nb + 1, 300], [0, nb], [nb, 1], [NX + 5, 9]], dtype=I32)
    y_seg = torch.tensor([[mb, 300], [0, mb], [0, mb], [NY - 2, 50]], dtype=I32)
    need = lib.rap_icp_plane_grid_workspace_bytes(NX, NY, K) if grid else lib.rap_icp_plane_workspace_bytes(NX, K)
    fn = lib.rap_icp_plane_grid if grid else lib.rap_icp_plane
    assert need > 0

    def call(c, short=0, with_xt=True):
        R, T = c.out_view(F32, (K, 3, 3), "R"), c.out_view(F32, (K, 3), "T")
        rmse, iters, conv = c.out_view(F32, (K,), "rmse"), c.out_view(I32, (K,), "iterations"), c.out_view(U8, (K,), "converged")
        Xt = c.out_view(F32, (NX, 3), "Xt") if with_xt else None
        ws = c.out(need, name="icp plane workspace")
        rc = fn(_lib.ptr(c.inp(X)), _lib.ptr(c.inp(x_seg)), _lib.ptr(c.inp(Y)), _lib.ptr(c.inp(y_seg)), _lib.ptr(c.inp(Yn)), K, NX, NY, None, None,
                100, 1e-6, 0.0, _lib.ptr(R), _lib.ptr(T), _lib.ptr(rmse), _lib.ptr(iters), _lib.ptr(conv), _lib.ptr(Xt), P2(ws.ptr), need - short,
                stream(dev))
        torch.cuda.synchronize()
        return rc, R, T, rmse, iters, conv, Xt

    def run_with(with_xt):
        def run(c):
            rc, R, T, rmse, iters, conv, Xt = call(c, with_xt=with_xt)
            assert rc == 0
            for k, ref in enumerate(refs):
                dR, dT = np.abs(R[k].double().cpu().numpy() - ref.R).max(), np.abs(T[k].double().cpu().numpy() - ref.T).max()
                print(f"problem {k}: |dR| {dR:.2e} |dT| {dT:.2e} |drmse| {abs(float(rmse[k]) - ref.rmse):.2e}")
                assert int(conv[k]) == 1
            # the margin-checked pair is held to the yardstick; the 300 x 300 one only has to have run (its margins are not checked)
            assert np.abs(R[1].double().cpu().numpy() - refs[1].R).max() <= 2e-6 and abs(float(rmse[1]) - refs[1].rmse) <= 2e-6
            assert int(iters[1]) == refs[1].iterations
            assert bool(torch.isfinite(R[2]).all()) and bool(torch.isfinite(rmse[2]))
            assert int(rmse.view(I32)[3]) != -1                      # a NaN the call wrote, not the 0xFF fill
            assert torch.isnan(rmse[3]) and int(iters[3]) == 0 and int(conv[3]) == 0 and torch.equal(R[3].cpu(), torch.eye(3))
            outs = [R, T, rmse, iters, conv]
            if with_xt:
                assert bool(torch.isfinite(Xt).all())                 # every row of X lies in a segment here: every row was written
                outs.append(Xt)
            return outs
        return run
    run_both(dev, run_with(True))
    run_both(dev, run_with(False))                                    # Xt = NULL: no apply launch
    refused_call_wrote_nothing(dev, call)


def test_icp_plane_refuses_null_arguments_with_nothing_written(lib, dev):
    X, Y, Yn = (torch.from_numpy(a).to(dev) for a in P.pair(*P.PLANE_PAIRS[0]))
    seg = torch.tensor([[0, 256]], dtype=I32, device=dev)
    outs = [torch.full((nbytes,), 0xFF, dtype=U8, device=dev) for nbytes in (36, 12, 4, 4, 4)]      # R, T, rmse, iterations, converged
    need = lib.rap_icp_plane_grid_workspace_bytes(256, 256, 1)
    ws = torch.full((need,), 0xFF, dtype=U8, device=dev)
    for fn in (lib.rap_icp_plane, lib.rap_icp_plane_grid):
        for miss in range(5):
            a = [_lib.ptr(X), _lib.ptr(seg), _lib.ptr(Y), _lib.ptr(seg), _lib.ptr(Yn)]
            a[miss] = None
            rc = fn(*a, 1, 256, 256, None, None, 10, 1e-6, 0.0, *[_lib.ptr(o) for o in outs], None, _lib.ptr(ws), need, stream(dev))
            assert rc == -1, miss
        rc = fn(_lib.ptr(X), _lib.ptr(seg), _lib.ptr(Y), _lib.ptr(seg), _lib.ptr(Yn), 1, 256, 256, None, None, 10, 1e-6, 0.0,
                *[_lib.ptr(o) for o in outs], None, None, need, stream(dev))
        assert rc == -2
    torch.cuda.synchronize()
    assert all(bool((o == 0xFF).all()) for o in outs) and bool((ws == 0xFF).all())


@pytest.mark.parametrize("max_nn,radius", [(32, 0.0), (12, P.SWEEP_RADIUS)])
def test_estimate_normals_writes_only_its_rows_and_its_exact_workspace(lib, dev, max_nn, radius):
    # segments that end exactly at the end of P (a partial third item), a segment of 257 (a candidate tile of one), an empty row past the array
    A, B = P.sweep_lattice(513), P.sweep_lattice(257)
    pts = torch.from_numpy(np.concatenate([B, A]))
    Npts, K = pts.shape[0], 3
    seg = torch.tensor([[257, 513], [Npts + 3, 8], [0, 257]], dtype=I32)
    vp = torch.tensor([[0.0, 0.0, 50.0]] * K)
    refs = [(257, P.estimate_normals(A, max_nn, radius, (0.0, 0.0, 50.0))), (0, P.estimate_normals(B, max_nn, radius, (0.0, 0.0, 50.0)))]
    need = lib.rap_normals_workspace_bytes(Npts, K)
    assert need > 0

    def call(c, short=0):
        n, e = c.out_view(F32, (Npts, 3), "normals"), c.out_view(F32, (Npts, 3), "eigenvalues")
        ws = c.out(need, name="normals workspace")
        rc = lib.rap_estimate_normals(_lib.ptr(c.inp(pts)), _lib.ptr(c.inp(seg)), K, Npts, max_nn, radius, _lib.ptr(c.inp(vp)), _lib.ptr(n), _lib.ptr(e),
                                      P2(ws.ptr), need - short, stream(dev))
        torch.cuda.synchronize()
        return rc, n, e

    def run(c):
        rc, n, e = call(c)
        assert rc == 0
        for start, (ref_n, ref_e, counts, gap) in refs:
            got = n[start:start + ref_n.shape[0]].double().cpu().numpy()
            has = counts >= 3
            # the viewpoint is far away but some normals are nearly orthogonal to its direction: compare up to sign
            dn = np.minimum(np.abs(got - ref_n).max(axis=1), np.abs(got + ref_n).max(axis=1)).max()
            de = (np.abs(e[start:start + ref_n.shape[0]].double().cpu().numpy() - ref_e) / np.maximum(ref_e[:, 2:3], 1e-300)).max()
            print(f"max_nn {max_nn} radius {radius}: worst |dn| {dn:.2e}, |d lambda| / lambda_max {de:.2e}")
            assert dn <= 2e-6 and de <= 2e-6 and not got[~has].any()
        return [n, e]
    run_both(dev, run)
    refused_call_wrote_nothing(dev, call)
    # NULL arguments: refused, nothing written
    out = torch.full((Npts * 12,), 0xFF, dtype=U8, device=dev)
    ws = torch.full((need,), 0xFF, dtype=U8, device=dev)
    d = [pts.to(dev), seg.to(dev)]
    for miss in range(3):
        a = [_lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(out)]
        a[miss] = None
        assert lib.rap_estimate_normals(a[0], a[1], K, Npts, max_nn, radius, None, a[2], None, _lib.ptr(ws), need, stream(dev)) == -1, miss
    assert lib.rap_estimate_normals(_lib.ptr(d[0]), _lib.ptr(d[1]), K, Npts, max_nn, radius, None, _lib.ptr(out), None, None, need, stream(dev)) == -2
    torch.cuda.synchronize()
    assert bool((out == 0xFF).all()) and bool((ws == 0xFF).all())
