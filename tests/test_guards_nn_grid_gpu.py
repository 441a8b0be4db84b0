"""Guard-band tests of rap_icp_grid and rap_nearest_neighbors through the C ABI: outputs sized exactly, the workspace at exactly the
queried bytes, a short workspace refused without a byte written, results independent of what lies beyond X, Y and the segment tables,
and rows of idx_out / d2_out outside every segment left alone.  Harness and limits: tests/test_guards_gpu.py and tests/guards.py (an
overrun longer than the pad and a read that reaches no result are not seen)."""
import ctypes

import numpy as np
import pytest
import torch

import icp_oracle as O
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


def problems():
    """tests/test_guards_icp_gpu.py's three problems and an empty one: segments that end exactly at the ends of X and of Y, a one-point
    problem that shares problem 1's rows of Y (one grid for both), and a table row that points past the arrays (clamped on the device)"""
    Xa, Ya = O.pair(O.SINGLE_SEED, 300, 257)
    Xb, Yb = O.pair(O.EXACT_COUNT[0][0], 256, 256)
    X = torch.from_numpy(np.concatenate([Xb, Xb[:1], Xa]))
    Y = torch.from_numpy(np.concatenate([Yb, Ya]))
    NX, NY = X.shape[0], Y.shape[0]
    x_seg = torch.tensor([[257, 300], [0, 256], [256, 1], [NX + 5, 9]], dtype=I32)
    y_seg = torch.tensor([[256, 257], [0, 256], [0, 256], [NY - 2, 50]], dtype=I32)
    return X, Y, x_seg, y_seg, NX, NY, 4


def test_icp_grid_writes_only_its_outputs_and_its_exact_workspace(lib, dev):
    X, Y, x_seg, y_seg, NX, NY, K = problems()
    refs = [O.solved(O.SINGLE_SEED, 300, 257), O.solved(*O.EXACT_COUNT[0])]
    need = lib.rap_icp_grid_workspace_bytes(NX, NY, K)
    assert need > lib.rap_icp_workspace_bytes(NX, K) > 0

    def call(c, short=0, with_xt=True):
        R, T = c.out_view(F32, (K, 3, 3), "R"), c.out_view(F32, (K, 3), "T")
        rmse, iters, conv = c.out_view(F32, (K,), "rmse"), c.out_view(I32, (K,), "iterations"), c.out_view(U8, (K,), "converged")
        Xt = c.out_view(F32, (NX, 3), "Xt") if with_xt else None
        ws = c.out(need, name="icp grid workspace")
        rc = lib.rap_icp_grid(_lib.ptr(c.inp(X)), _lib.ptr(c.inp(x_seg)), _lib.ptr(c.inp(Y)), _lib.ptr(c.inp(y_seg)), K, NX, NY, None, None,
                              100, 1e-6, 0.0, _lib.ptr(R), _lib.ptr(T), _lib.ptr(rmse), _lib.ptr(iters), _lib.ptr(conv), _lib.ptr(Xt),
                              P2(ws.ptr), need - short, stream(dev))
        torch.cuda.synchronize()
        return rc, R, T, rmse, iters, conv, Xt

    def run_with(with_xt):
        def run(c):
            rc, R, T, rmse, iters, conv, Xt = call(c, with_xt=with_xt)
            assert rc == 0
            for k, ref in enumerate(refs):
                assert np.abs(R[k].double().cpu().numpy() - ref.R).max() <= 2e-6 and np.abs(T[k].double().cpu().numpy() - ref.T).max() <= 2e-6
                assert abs(float(rmse[k]) - ref.rmse) <= 2e-6 and int(conv[k]) == 1
            assert int(iters[1]) == refs[1].iterations
            assert int(conv[2]) == 1 and float(rmse[2]) < 1e-6
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


def test_nearest_neighbors_writes_only_the_rows_of_its_segments_and_its_exact_workspace(lib, dev):
    X, Y, _, y_seg, NX, NY, K = problems()
    # rows 250..255 and the last four rows of X lie in no segment
    x_seg = torch.tensor([[257, 296], [0, 250], [256, 1], [NX + 5, 9]], dtype=I32)
    need = lib.rap_nn_grid_workspace_bytes(NX, NY, K)
    assert need > 0
    D = ((X[:, None, :].double() - Y[None].double()) ** 2).sum(dim=2).numpy()

    def call(c, short=0):
        idx, d2 = c.out_view(I32, (NX,), "idx_out"), c.out_view(F32, (NX,), "d2_out")
        ws = c.out(need, name="nn grid workspace")
        rc = lib.rap_nearest_neighbors(_lib.ptr(c.inp(X)), _lib.ptr(c.inp(x_seg)), _lib.ptr(c.inp(Y)), _lib.ptr(c.inp(y_seg)), K, NX, NY,
                                       None, None, 0.0, _lib.ptr(idx), _lib.ptr(d2), P2(ws.ptr), need - short, stream(dev))
        torch.cuda.synchronize()
        return rc, idx, d2

    def run(c):
        rc, idx, d2 = call(c)
        assert rc == 0
        i, d = idx.cpu().numpy(), d2.cpu().numpy()
        for (xs, xn), (ys, yn) in (((257, 296), (256, 257)), ((0, 250), (0, 256)), ((256, 1), (0, 256))):
            rows = np.arange(xs, xs + xn)
            assert ((i[rows] >= ys) & (i[rows] < ys + yn)).all()      # a row of Y (not of the segment), inside the problem's segment
            best = D[rows, ys:ys + yn].min(axis=1)
            assert np.allclose(D[rows, i[rows]], best, rtol=1e-6, atol=0) and np.allclose(d[rows], best, rtol=1e-6, atol=1e-12)
        outside = np.r_[250:256, 257 + 296:NX]
        assert (i[outside] == -1).all() and (d2.view(I32).cpu().numpy()[outside] == -1).all()      # still the 0xFF fill: never written
        return [idx, d2]
    run_both(dev, run)
    refused_call_wrote_nothing(dev, call)
