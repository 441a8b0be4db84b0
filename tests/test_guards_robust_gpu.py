"""Guard-band tests of rap_icp_plane_robust, rap_icp_plane_grid_robust and rap_scene_refine_robust through the C ABI: every output
(`weights` included) sized exactly and between guard bytes, the workspace at exactly the queried bytes and 0xFF-filled, a short workspace
and bad arguments refused without a byte written, results independent of what lies beyond the inputs.  Harness and limits:
tests/test_guards_gpu.py and tests/guards.py.  The same refusals without a GPU: tests/test_robust_host.py."""
import ctypes

import numpy as np
import pytest
import torch

import guards as G
import robust_cases as C
import scene_refine_oracle as S
from rap_amd import _lib
from test_guards_gpu import F32, I32, U8, Case, refused_call_wrote_nothing, run_both, stream

pytestmark = pytest.mark.gpu

P2 = ctypes.c_void_p
LOSS, SCALE = "tukey", C.SCALE["tukey"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.mark.parametrize("with_weights", [True, False], ids=["weights", "weights-NULL"])
@pytest.mark.parametrize("grid", [False, True], ids=["brute", "grid"])
def test_icp_plane_robust_writes_only_its_outputs_and_its_exact_workspace(lib, dev, grid, with_weights):
    # the exact contaminated pair, whose segments end exactly at the ends of X and of Y (a second item of one query last in X); a one-point
    # problem in front of it; an empty problem whose table row points past the arrays (clamped on the device)
    Xa, Ya, Na = C.contaminated_pair(*C.EXACT_PAIR)
    ref = C.pair_solved(*C.EXACT_PAIR, LOSS)
    nx, ny = Xa.shape[0], Ya.shape[0]
    X = torch.from_numpy(np.concatenate([Xa[1:2], Xa]))
    Y, Yn = torch.from_numpy(Ya), torch.from_numpy(Na)
    NX, NY, K = X.shape[0], ny, 3
    x_seg = torch.tensor([[0, 1], [NX + 5, 9], [1, nx]], dtype=I32)
    y_seg = torch.tensor([[0, ny], [NY - 2, 50], [0, ny]], dtype=I32)
    need = lib.rap_icp_plane_grid_robust_workspace_bytes(NX, NY, K) if grid else lib.rap_icp_plane_robust_workspace_bytes(NX, K)
    fn = lib.rap_icp_plane_grid_robust if grid else lib.rap_icp_plane_robust
    assert need > 0

    def call(c, short=0, loss=C.CODES[LOSS], scale=SCALE):
        R, T = c.out_view(F32, (K, 3, 3), "R"), c.out_view(F32, (K, 3), "T")
        rmse, iters, conv = c.out_view(F32, (K,), "rmse"), c.out_view(I32, (K,), "iterations"), c.out_view(U8, (K,), "converged")
        Xt = c.out_view(F32, (NX, 3), "Xt")
        w = c.out_view(F32, (NX,), "weights") if with_weights else None
        ws = c.out(need, name="robust icp plane workspace")
        rc = fn(_lib.ptr(c.inp(X)), _lib.ptr(c.inp(x_seg)), _lib.ptr(c.inp(Y)), _lib.ptr(c.inp(y_seg)), _lib.ptr(c.inp(Yn)), K, NX, NY, None, None,
                100, C.THR, 0.0, _lib.ptr(R), _lib.ptr(T), _lib.ptr(rmse), _lib.ptr(iters), _lib.ptr(conv), _lib.ptr(Xt), loss, scale, _lib.ptr(w),
                P2(ws.ptr), need - short, stream(dev))
        torch.cuda.synchronize()
        return rc, R, T, rmse, iters, conv, Xt, w

    def run(c):
        rc, R, T, rmse, iters, conv, Xt, w = call(c)
        assert rc == 0
        d = max(np.abs(R[2].double().cpu().numpy() - ref.R).max(), np.abs(T[2].double().cpu().numpy() - ref.T).max(), abs(float(rmse[2]) - ref.rmse))
        print(f"poses/rmse {d:.2e}, iterations {int(iters[2])} / {ref.iterations}")
        assert d <= C.FP32_BOUND and int(iters[2]) == ref.iterations and int(conv[2]) == 1
        assert bool(torch.isfinite(R[0]).all()) and bool(torch.isfinite(rmse[0]))
        assert int(rmse.view(I32)[1]) != -1                          # a NaN the call wrote, not the 0xFF fill
        assert torch.isnan(rmse[1]) and int(iters[1]) == 0 and int(conv[1]) == 0 and torch.equal(R[1].cpu(), torch.eye(3))
        assert bool(torch.isfinite(Xt).all())                         # every row of X lies in a segment here: every row was written
        outs = [R, T, rmse, iters, conv, Xt]
        if with_weights:
            wn = w.double().cpu().numpy()
            assert np.isfinite(wn).all() and np.abs(wn[1:] - ref.weights).max() <= C.WEIGHT_BOUND and not wn[1::5].any()
            outs.append(w)
        return outs
    run_both(dev, run)
    refused_call_wrote_nothing(dev, call)
    # a loss the call does not know, and a scale it cannot use: refused like a short workspace, with nothing written
    for loss, scale in ((4, SCALE), (-1, SCALE), (1, 0.0), (2, float("nan")), (3, float("inf"))):
        refused_invalid(dev, lambda c, short=0: call(c, 0, loss, scale))


def refused_invalid(dev, call):
    """refused_call_wrote_nothing for RAP_ERR_INVALID"""
    c = Case(dev, 0x00)
    assert call(c)[0] == -1
    c.check()
    for g in c.guards:
        if g.guard == G.GUARD:
            assert g.untouched(), f"{g.name}: a refused call wrote into it"


@pytest.mark.parametrize("with_edges_out", [True, False], ids=["edge-outputs", "edge-outputs-NULL"])
def test_scene_refine_robust_writes_only_its_outputs_and_its_exact_workspace(lib, dev, with_edges_out):
    # the contaminated ring, whose last view ends exactly at the end of P; a view table row past the array (clamped on the device)
    # outside every scene; edges that are ignored; the row budget exactly the sum of the live edges' source rows
    sc, ref = C.contaminated_ring(), C.ring_solved(LOSS)
    Pt, Nt = torch.from_numpy(sc["P"]), torch.from_numpy(sc["N"])
    n, V0 = Pt.shape[0], S.RING_V
    seg = torch.tensor([list(int(v) for v in r) for r in sc["seg"]] + [[n + 5, 9]], dtype=I32)
    scenes = torch.tensor([[0, V0]], dtype=I32)
    pairs = [tuple(int(v) for v in e) for e in S.ring_edges()]
    edges = torch.tensor(pairs + [(6, 0), (0, 6), (2, 2), (9, 1)], dtype=I32)
    R0 = torch.from_numpy(np.concatenate([sc["R0"], np.eye(3, dtype=np.float32)[None]]))
    T0 = torch.from_numpy(np.concatenate([sc["T0"], np.zeros((1, 3), np.float32)]))
    V, Sn, E = V0 + 1, 1, edges.shape[0]
    budget = int(2 * sc["seg"][:, 1].sum())
    need = lib.rap_scene_refine_robust_workspace_bytes(n, V, Sn, E, budget, 16)
    assert need > lib.rap_scene_refine_workspace_bytes(n, V, Sn, E, budget, 16) > 0

    def call(c, short=0, loss=C.CODES[LOSS], scale=SCALE):
        R, T = c.out_view(F32, (V, 3, 3), "R"), c.out_view(F32, (V, 3), "T")
        rmse, iters, conv = c.out_view(F32, (Sn,), "rmse"), c.out_view(I32, (Sn,), "iterations"), c.out_view(U8, (Sn,), "converged")
        er = c.out_view(F32, (E,), "edge_rmse") if with_edges_out else None
        ec = c.out_view(I32, (E,), "edge_count") if with_edges_out else None
        ws = c.out(need, name="robust scene refine workspace")
        rc = lib.rap_scene_refine_robust(_lib.ptr(c.inp(Pt)), _lib.ptr(c.inp(Nt)), _lib.ptr(c.inp(seg)), V, n, _lib.ptr(c.inp(scenes)), Sn,
                                         _lib.ptr(c.inp(edges)), E, budget, 16, None, _lib.ptr(c.inp(R0)), _lib.ptr(c.inp(T0)), 30, C.THR, C.GATE,
                                         _lib.ptr(R), _lib.ptr(T), _lib.ptr(rmse), _lib.ptr(iters), _lib.ptr(conv), _lib.ptr(er), _lib.ptr(ec),
                                         loss, scale, P2(ws.ptr), need - short, stream(dev))
        torch.cuda.synchronize()
        return rc, R, T, rmse, iters, conv, er, ec

    def run(c):
        rc, R, T, rmse, iters, conv, er, ec = call(c)
        assert rc == 0
        dR, dT = np.abs(R[:V0].double().cpu().numpy() - ref.R).max(), np.abs(T[:V0].double().cpu().numpy() - ref.T).max()
        print(f"|dR| {dR:.2e} |dT| {dT:.2e} |drmse| {abs(float(rmse[0]) - ref.rmse[0]):.2e}, iterations {int(iters[0])}")
        assert max(dR, dT, abs(float(rmse[0]) - ref.rmse[0])) <= C.FP32_BOUND and int(iters[0]) == ref.iterations[0] and int(conv[0]) == 1
        assert torch.equal(R[V0].cpu(), torch.eye(3)) and not T[V0].any()  # the view outside every scene: its init, written by the call
        outs = [R, T, rmse, iters, conv]
        if with_edges_out:
            assert np.abs(ec[:12].cpu().numpy() - ref.edge_count).max() <= 1 and not ec[12:].any() and bool(torch.isnan(er[12:]).all())
            assert np.abs(er[:12].double().cpu().numpy() - ref.edge_rmse).max() <= C.FP32_BOUND
            outs += [er, ec]
        return outs
    run_both(dev, run)
    refused_call_wrote_nothing(dev, call)
    for loss, scale in ((4, SCALE), (-1, SCALE), (1, -1.0), (2, float("nan")), (3, float("inf"))):
        refused_invalid(dev, lambda c, short=0: call(c, 0, loss, scale))
