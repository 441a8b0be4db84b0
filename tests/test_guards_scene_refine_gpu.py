"""Guard-band test of rap_scene_refine through the C ABI: every output sized exactly and between guard bytes, the workspace at exactly
the queried bytes and 0xFF-filled, a short workspace and NULL arguments refused without a byte written, results equal to the unguarded
call.  Harness and limits: tests/test_guards_gpu.py and tests/guards.py.  The same refusals without a GPU: tests/test_scene_refine_host.py."""
import ctypes

import numpy as np
import pytest
import torch

import scene_refine_oracle as S
import rap_amd
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


@pytest.mark.parametrize("with_edges_out", [True, False], ids=["edge-outputs", "edge-outputs-NULL"])
def test_scene_refine_writes_only_its_outputs_and_its_exact_workspace(lib, dev, with_edges_out):
    # the margin-checked gauge-free 3-view scene, whose last view ends exactly at the end of P; a view table row past the array (clamped on
    # the device) outside every scene; edges that are ignored; the row budget exactly the sum of the live edges' source rows
    V0, seed, gate, variant, _ = S.PARITY_CASES[1]
    sc, ref = S.parity_scene(V0, seed, variant), S.parity_solved(V0, seed, gate, variant)
    Pt, Nt = torch.from_numpy(sc["P"]), torch.from_numpy(sc["N"])
    n = Pt.shape[0]
    seg = torch.tensor([list(r) for r in sc["seg"]] + [[n + 5, 9]], dtype=I32)
    scenes = torch.tensor([[0, 3]], dtype=I32)
    pairs = [tuple(int(v) for v in e) for e in S.pairs_of(0, 3)]
    edges = torch.tensor(pairs + [(3, 0), (0, 3), (2, 2), (7, 1)], dtype=I32)
    fixed = torch.zeros(4, dtype=U8)
    R0 = torch.from_numpy(np.concatenate([sc["R0"], np.eye(3, dtype=np.float32)[None]]))
    T0 = torch.from_numpy(np.concatenate([sc["T0"], np.zeros((1, 3), np.float32)]))
    V, Sn, E = 4, 1, edges.shape[0]
    budget = int(2 * sc["seg"][:, 1].sum())
    need = lib.rap_scene_refine_workspace_bytes(n, V, Sn, E, budget, 16)
    assert need > 0
    plain = rap_amd.refine_scene_packed(Pt.to(dev), seg.to(dev), scenes.to(dev), R0.to(dev), T0.to(dev), edges=edges.to(dev), normals=Nt.to(dev),
                                        fixed=fixed.to(dev), relative_rmse_thr=S.THR, max_correspondence_distance=gate, row_budget=budget)

    def call(c, short=0):
        R, T = c.out_view(F32, (V, 3, 3), "R"), c.out_view(F32, (V, 3), "T")
        rmse, iters, conv = c.out_view(F32, (Sn,), "rmse"), c.out_view(I32, (Sn,), "iterations"), c.out_view(U8, (Sn,), "converged")
        er = c.out_view(F32, (E,), "edge_rmse") if with_edges_out else None
        ec = c.out_view(I32, (E,), "edge_count") if with_edges_out else None
        ws = c.out(need, name="scene refine workspace")
        rc = lib.rap_scene_refine(_lib.ptr(c.inp(Pt)), _lib.ptr(c.inp(Nt)), _lib.ptr(c.inp(seg)), V, n, _lib.ptr(c.inp(scenes)), Sn,
                                  _lib.ptr(c.inp(edges)), E, budget, 16, _lib.ptr(c.inp(fixed)), _lib.ptr(c.inp(R0)), _lib.ptr(c.inp(T0)), 30,
                                  S.THR, gate, _lib.ptr(R), _lib.ptr(T), _lib.ptr(rmse), _lib.ptr(iters), _lib.ptr(conv), _lib.ptr(er),
                                  _lib.ptr(ec), P2(ws.ptr), need - short, stream(dev))
        torch.cuda.synchronize()
        return rc, R, T, rmse, iters, conv, er, ec

    def run(c):
        rc, R, T, rmse, iters, conv, er, ec = call(c)
        assert rc == 0
        dR, dT = np.abs(R[:3].double().cpu().numpy() - ref.R).max(), np.abs(T[:3].double().cpu().numpy() - ref.T).max()
        print(f"|dR| {dR:.2e} |dT| {dT:.2e} |drmse| {abs(float(rmse[0]) - ref.rmse[0]):.2e}, iterations {int(iters[0])}")
        assert max(dR, dT, abs(float(rmse[0]) - ref.rmse[0])) <= S.FP32_BOUND and int(iters[0]) == ref.iterations[0] and int(conv[0]) == 1
        assert torch.equal(R.view(I32), plain.R.view(I32)) and torch.equal(T.view(I32), plain.T.view(I32))
        assert torch.equal(rmse.view(I32), plain.rmse.view(I32)) and torch.equal(iters, plain.iterations)
        assert torch.equal(R[3].cpu(), torch.eye(3)) and not T[3].any()  # the view outside every scene: its init, written by the call
        outs = [R, T, rmse, iters, conv]
        if with_edges_out:
            assert torch.equal(ec, plain.edge_count) and torch.equal(er.view(I32), plain.edge_rmse.view(I32))
            assert ec[:6].cpu().tolist() == ref.edge_count.tolist() and not ec[6:].any() and bool(torch.isnan(er[6:]).all())
            outs += [er, ec]
        return outs
    run_both(dev, run)
    refused_call_wrote_nothing(dev, call)


def test_scene_refine_refuses_null_arguments_with_nothing_written(lib, dev):
    sc = S.parity_scene(3, 9, "first")
    n = sc["P"].shape[0]
    d = [torch.from_numpy(sc["P"]).to(dev), torch.from_numpy(sc["N"]).to(dev), torch.from_numpy(sc["seg"]).to(dev),
         torch.tensor([[0, 3]], dtype=I32, device=dev), torch.from_numpy(S.pairs_of(0, 3)).to(dev)]
    outs = [torch.full((nbytes,), 0xFF, dtype=U8, device=dev) for nbytes in (108, 36, 4, 4, 1, 24, 24)]
    need = lib.rap_scene_refine_workspace_bytes(n, 3, 1, 6, 2 * n, 16)
    ws = torch.full((need,), 0xFF, dtype=U8, device=dev)

    def go(a, o, wsp, it=10):
        return lib.rap_scene_refine(a[0], a[1], a[2], 3, n, a[3], 1, a[4], 6, 2 * n, 16, None, None, None, it, 1e-6, 0.0, *o, wsp, need, stream(dev))
    for miss in range(5):
        a = [_lib.ptr(x) for x in d]
        a[miss] = None
        assert go(a, [_lib.ptr(o) for o in outs], _lib.ptr(ws)) == -1, miss
    for miss in range(5):
        o = [_lib.ptr(x) for x in outs]
        o[miss] = None
        assert go([_lib.ptr(x) for x in d], o, _lib.ptr(ws)) == -1, miss
    assert go([_lib.ptr(x) for x in d], [_lib.ptr(o) for o in outs], _lib.ptr(ws), it=0) == -1
    assert go([_lib.ptr(x) for x in d], [_lib.ptr(o) for o in outs], None) == -2
    torch.cuda.synchronize()
    assert all(bool((o == 0xFF).all()) for o in outs) and bool((ws == 0xFF).all())
