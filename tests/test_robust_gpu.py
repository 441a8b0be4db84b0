"""GPU: the robust point-to-plane calls (rap_icp_plane_robust, rap_icp_plane_grid_robust, rap_scene_refine_robust and the loss keywords
of rap_amd/icp.py and rap_amd/scene.py) against their fp64 yardstick (tests/robust_cases.py).

Bounds: poses, rmse and edge_rmse within robust_cases.FP32_BOUND of the yardstick, weights within robust_cases.WEIGHT_BOUND; both are
the larger of 2e-6 and three times the yardstick's own fp32-mode deviation, measured in tests/test_robust_host.py, which also asserts
that no neighbour, gate or stopping decision of the cases compared exactly comes within 1e-5 of flipping.  Every parity test prints its
worst deviation before it asserts (run with -s to see them)."""
import numpy as np
import pytest
import torch

import icp_oracle as O
import robust_cases as C
import scene_refine_oracle as SO
import rap_amd
from rap_amd import _lib

pytestmark = pytest.mark.gpu

F32, I32, U8 = torch.float32, torch.int32, torch.uint8
PLANE = dict(estimation="point_to_plane")
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def t(dev, a, dtype=None):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(dev)


def bits(x):
    return x.contiguous().cpu().reshape(-1).view(U8).clone()


def sol_bits(sol, weights=None):
    out = [bits(x) for x in (sol.converged.to(U8), sol.rmse, sol.Xt, sol.R, sol.T, sol.iterations)]
    return out + ([bits(weights)] if weights is not None else [])


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def pair_c(lib, dev, grid, X, xs, Y, ys, Yn, loss=None, scale=0.0, iR=None, iT=None, gate=0.0, weights=None, fill=None, it=100):
    """the C entry point itself: loss None -> the sibling (rap_icp_plane / _grid), else the robust twin with that RAP_LOSS_* code.
    fill: a byte the workspace is filled with first.  -> dict of the outputs"""
    K, NX, NY = xs.shape[0], X.shape[0], Y.shape[0]
    o = dict(R=torch.empty((K, 3, 3), dtype=F32, device=dev), T=torch.empty((K, 3), dtype=F32, device=dev),
             rmse=torch.empty((K,), dtype=F32, device=dev), iterations=torch.empty((K,), dtype=I32, device=dev),
             converged=torch.empty((K,), dtype=U8, device=dev), Xt=X.clone())
    name = "rap_icp_plane" + ("_grid" if grid else "") + ("" if loss is None else "_robust")
    q = getattr(lib, name + "_workspace_bytes")
    need = q(NX, NY, K) if grid else q(NX, K)
    ws = torch.empty((need,), dtype=U8, device=dev)
    if fill is not None:
        ws.fill_(fill)
    extra = () if loss is None else (loss, scale, _lib.ptr(weights))
    rc = getattr(lib, name)(_lib.ptr(X), _lib.ptr(xs), _lib.ptr(Y), _lib.ptr(ys), _lib.ptr(Yn), K, NX, NY, _lib.ptr(iR), _lib.ptr(iT), it, C.THR,
                            gate, _lib.ptr(o["R"]), _lib.ptr(o["T"]), _lib.ptr(o["rmse"]), _lib.ptr(o["iterations"]), _lib.ptr(o["converged"]),
                            _lib.ptr(o["Xt"]), *extra, _lib.ptr(ws), need, _lib.current_stream(dev))
    assert rc == 0, (name, rc)
    torch.cuda.synchronize()
    return o


def dict_bits(o):
    return [bits(o[n]) for n in ("R", "T", "rmse", "iterations", "converged", "Xt")]


# ---- 1. parity with the yardstick on the exact contaminated pair ----
@pytest.mark.parametrize("loss,scale", C.ROBUST)
def test_contaminated_pair_matches_the_yardstick_and_grid_equals_brute(dev, loss, scale):
    X, Y, Yn = C.contaminated_pair(*C.EXACT_PAIR)
    ref = C.pair_solved(*C.EXACT_PAIR, loss)
    got = {}
    for search in ("brute", "grid"):
        sol, w = rap_amd.iterative_closest_point(t(dev, X), t(dev, Y), Y_normals=t(dev, Yn), relative_rmse_thr=C.THR, search=search, loss=loss,
                                                 loss_scale=scale, return_weights=True, **PLANE)
        R, T = sol.R[0].double().cpu().numpy(), sol.T[0].double().cpu().numpy()
        dR, dT, dr = np.abs(R - ref.R).max(), np.abs(T - ref.T).max(), abs(float(sol.rmse[0]) - ref.rmse)
        dw = np.abs(w.double().cpu().numpy() - ref.weights).max()
        print(f"{loss} {search}: |dR| {dR:.2e} |dT| {dT:.2e} |drmse| {dr:.2e} (bound {C.FP32_BOUND:.1e}), |dw| {dw:.2e} (bound {C.WEIGHT_BOUND:.1e}), "
              f"iterations {int(sol.iterations[0])} / {ref.iterations}")
        assert max(dR, dT, dr) <= C.FP32_BOUND and dw <= C.WEIGHT_BOUND
        assert int(sol.iterations[0]) == ref.iterations and bool(sol.converged[0]) == ref.converged
        assert w.shape == (C.EXACT_PAIR[1],) and abs(np.linalg.det(R) - 1.0) < 1e-6
        if loss == "tukey":                                              # the lifted rows are several scales off the surface: exactly zero
            assert not w[0::5].any() and bool((w > 0).any())
        got[search] = sol_bits(sol, w)
    assert same(got["brute"], got["grid"])
    # the plain call on the same pair ends elsewhere: the loss is not a no-op
    plain = rap_amd.iterative_closest_point(t(dev, X), t(dev, Y), Y_normals=t(dev, Yn), relative_rmse_thr=C.THR, **PLANE)
    assert np.abs(plain.T[0].double().cpu().numpy() - ref.T).max() > 1e-3


def test_gated_rows_and_rows_beyond_the_scale_both_get_weight_zero(dev):
    X, Y, Yn = C.contaminated_pair(*C.EXACT_PAIR)
    ref = C.gated_solved()
    for search in ("brute", "grid"):
        sol, w = rap_amd.iterative_closest_point(t(dev, X), t(dev, Y), Y_normals=t(dev, Yn), relative_rmse_thr=C.THR, search=search, loss="tukey",
                                                 loss_scale=C.SCALE["tukey"], max_correspondence_distance=C.PAIR_GATE, return_weights=True, **PLANE)
        w = w.double().cpu().numpy()
        d = max(np.abs(sol.R[0].double().cpu().numpy() - ref.R).max(), np.abs(sol.T[0].double().cpu().numpy() - ref.T).max(),
                abs(float(sol.rmse[0]) - ref.rmse))
        print(f"gated {search}: poses/rmse {d:.2e}, |dw| {np.abs(w - ref.weights).max():.2e}, {int((w > 0).sum())} rows with a weight")
        assert d <= C.FP32_BOUND and np.abs(w - ref.weights).max() <= C.WEIGHT_BOUND and int(sol.iterations[0]) == ref.iterations
        assert np.array_equal(w > 0, ref.weights > 0) and 0 < (w > 0).sum() < ref.count < X.shape[0]


# ---- 2. RAP_LOSS_NONE is the sibling, bit for bit ----
def batch_tensors(dev):
    b = C.batch()
    return (t(dev, b["X"]), t(dev, b["x_seg"], I32), t(dev, b["Y"]), t(dev, b["y_seg"], I32), t(dev, b["Yn"])), t(dev, b["init_R"]), t(dev, b["init_T"])


@pytest.mark.parametrize("grid", [False, True], ids=["brute", "grid"])
def test_pairwise_robust_call_with_loss_none_returns_its_siblings_bits(lib, dev, grid):
    clouds, iR, iT = batch_tensors(dev)
    for gate in (0.0, 0.1):
        want = dict_bits(pair_c(lib, dev, grid, *clouds, iR=iR, iT=iT, gate=gate))
        w = torch.full((clouds[0].shape[0],), 7.0, dtype=F32, device=dev)
        assert same(dict_bits(pair_c(lib, dev, grid, *clouds, loss=0, scale=NAN, iR=iR, iT=iT, gate=gate, weights=w)), want)      # the scale is ignored
        assert same(dict_bits(pair_c(lib, dev, grid, *clouds, loss=0, scale=-1.0, iR=iR, iT=iT, gate=gate)), want)      # weights = NULL
        wc = w.cpu().numpy()
        assert set(np.unique(wc[C.batch()["covered"]])) <= {0.0, 1.0} and (wc[~C.batch()["covered"]] == 7.0).all()
    X, Y, Yn = (t(dev, a) for a in C.contaminated_pair(*C.EXACT_PAIR))      # ... and through the wrapper, which takes loss none to the robust call
    search = "grid" if grid else "brute"                                     # only when the weights are asked for
    sol, w = rap_amd.iterative_closest_point(X, Y, Y_normals=Yn, search=search, return_weights=True, **PLANE)
    assert same(sol_bits(sol), sol_bits(rap_amd.iterative_closest_point(X, Y, Y_normals=Yn, search=search, **PLANE))) and bool((w == 1).all())


def scene_c(lib, dev, P, N, seg, scenes, edges, R0, T0, loss=None, scale=0.0, gate=0.0, fill=None, it=30, edge_out=True):
    """rap_scene_refine (loss None) or rap_scene_refine_robust through the C ABI -> dict of the outputs"""
    V, S, E, n = seg.shape[0], scenes.shape[0], edges.shape[0], P.shape[0]
    budget = n * 15
    o = dict(R=torch.empty((V, 3, 3), dtype=F32, device=dev), T=torch.empty((V, 3), dtype=F32, device=dev),
             rmse=torch.empty((S,), dtype=F32, device=dev), iterations=torch.empty((S,), dtype=I32, device=dev),
             converged=torch.empty((S,), dtype=U8, device=dev), edge_rmse=torch.empty((E,), dtype=F32, device=dev) if edge_out else None,
             edge_count=torch.empty((E,), dtype=I32, device=dev) if edge_out else None)
    name = "rap_scene_refine" + ("" if loss is None else "_robust")
    need = getattr(lib, name + "_workspace_bytes")(n, V, S, E, budget, 16)
    ws = torch.empty((need,), dtype=U8, device=dev)
    if fill is not None:
        ws.fill_(fill)
    extra = () if loss is None else (loss, scale)
    rc = getattr(lib, name)(_lib.ptr(P), _lib.ptr(N), _lib.ptr(seg), V, n, _lib.ptr(scenes), S, _lib.ptr(edges), E, budget, 16, None, _lib.ptr(R0),
                            _lib.ptr(T0), it, C.THR, gate, _lib.ptr(o["R"]), _lib.ptr(o["T"]), _lib.ptr(o["rmse"]), _lib.ptr(o["iterations"]),
                            _lib.ptr(o["converged"]), _lib.ptr(o["edge_rmse"]), _lib.ptr(o["edge_count"]), *extra, _lib.ptr(ws), need,
                            _lib.current_stream(dev))
    assert rc == 0, (name, rc)
    torch.cuda.synchronize()
    return o


def scene_bits(o):
    return [bits(o[n]) for n in ("R", "T", "rmse", "iterations", "converged", "edge_rmse", "edge_count") if o[n] is not None]


def ring_tensors(dev, contaminated=True):
    sc = C.contaminated_ring() if contaminated else SO.ring_scene()
    return (t(dev, sc["P"]), t(dev, sc["N"]), t(dev, sc["seg"], I32), torch.tensor([[0, SO.RING_V]], dtype=I32, device=dev),
            t(dev, SO.ring_edges(), I32), t(dev, sc["R0"]), t(dev, sc["T0"]))


def test_scene_robust_call_with_loss_none_returns_its_siblings_bits(lib, dev):
    for contaminated in (True, False):
        args = ring_tensors(dev, contaminated)
        want = scene_bits(scene_c(lib, dev, *args, gate=C.GATE))
        assert same(scene_bits(scene_c(lib, dev, *args, loss=0, scale=NAN, gate=C.GATE, fill=0xFF)), want)
    assert same(scene_bits(scene_c(lib, dev, *args, loss=0, scale=0.0, gate=C.GATE, edge_out=False)), want[:5])


# ---- 3. one packed batch: item and tile edges, an empty problem, a problem whose every weight is zero ----
@pytest.mark.parametrize("search", ["brute", "grid"])
def test_batch_problems_get_the_bits_they_get_alone_whatever_the_workspace_held(lib, dev, search):
    b, ref = C.batch(), C.batch_solved()
    clouds, iR, iT = batch_tensors(dev)
    code, scale, grid = C.CODES[C.BATCH_LOSS], C.BATCH_SCALE, search == "grid"
    NX = b["X"].shape[0]
    runs = []
    for fill in (0x00, 0xFF):                                            # twice, over different workspace contents
        w = torch.full((NX,), 7.0, dtype=F32, device=dev)
        o = pair_c(lib, dev, grid, *clouds, loss=code, scale=scale, iR=iR, iT=iT, weights=w, fill=fill)
        runs.append(dict_bits(o) + [bits(w)])
    assert same(*runs)
    wc = w.cpu().numpy()
    assert (wc[~b["covered"]] == 7.0).all() and (wc[b["covered"]] != 7.0).all()      # rows outside every segment are untouched; every other is written
    assert same(dict_bits(pair_c(lib, dev, grid, *clouds, loss=code, scale=scale, iR=iR, iT=iT)), runs[0][:6])      # weights = NULL
    for k, part in enumerate(b["parts"]):
        xs, xn = (int(v) for v in b["x_seg"][k])
        if part is None:                                                 # the empty problem
            assert torch.isnan(o["rmse"][k]) and int(o["iterations"][k]) == 0 and int(o["converged"][k]) == 0
            assert torch.equal(o["R"][k].cpu(), torch.eye(3)) and not o["T"][k].any()
            continue
        Xs, Ys, Ns = (t(dev, a) for a in part)
        seg = lambda n: torch.tensor([[0, n]], dtype=I32, device=dev)
        ws = torch.full((xn,), 7.0, dtype=F32, device=dev)
        solo = pair_c(lib, dev, grid, Xs, seg(xn), Ys, seg(Ys.shape[0]), Ns, loss=code, scale=scale, iR=iR[k:k + 1], iT=iT[k:k + 1], weights=ws)
        for name in ("R", "T", "rmse", "iterations", "converged"):
            assert torch.equal(bits(o[name][k]), bits(solo[name][0])), (k, name)
        assert torch.equal(bits(o["Xt"][xs:xs + xn]), bits(solo["Xt"])) and torch.equal(bits(w[xs:xs + xn]), bits(ws)), k
        r = ref[k]
        if r.wsum == 0.0:                                                # W == 0: as a problem without pairs, with the pose it had
            assert torch.isinf(o["rmse"][k]) and float(o["rmse"][k]) > 0 and int(o["converged"][k]) == 0 and int(o["iterations"][k]) == 0
            assert torch.equal(bits(o["R"][k]), bits(iR[k])) and torch.equal(bits(o["T"][k]), bits(iT[k])) and not w[xs:xs + xn].any()
            continue
        d = max(np.abs(o["R"][k].double().cpu().numpy() - r.R).max(), np.abs(o["T"][k].double().cpu().numpy() - r.T).max(),
                abs(float(o["rmse"][k]) - r.rmse))
        dw = np.abs(wc[xs:xs + xn] - r.weights).max()
        print(f"{search} problem {k} ({xn} rows): poses/rmse {d:.2e}, |dw| {dw:.2e}, iterations {int(o['iterations'][k])} / {r.iterations}")
        assert d <= C.FP32_BOUND and dw <= C.WEIGHT_BOUND and int(o["iterations"][k]) == r.iterations and int(o["converged"][k]) == 1
    far = b["far"]
    assert ref[far].wsum == 0.0 and ref[far].count == 200 and ref[0].wsum == 0.0


# ---- 4. the scene call ----
@pytest.mark.parametrize("loss,scale", C.ROBUST)
def test_contaminated_ring_matches_the_yardstick(dev, loss, scale):
    sc, ref = C.contaminated_ring(), C.ring_solved(loss)
    sol = rap_amd.refine_scene_packed(t(dev, sc["P"]), t(dev, sc["seg"], I32), torch.tensor([[0, SO.RING_V]], dtype=I32, device=dev), t(dev, sc["R0"]),
                                      t(dev, sc["T0"]), edges=t(dev, SO.ring_edges(), I32), normals=t(dev, sc["N"]), relative_rmse_thr=C.THR,
                                      max_correspondence_distance=C.GATE, loss=loss, loss_scale=scale)
    got = O.Result(R=sol.R.double().cpu().numpy(), T=sol.T.double().cpu().numpy(), rmse=sol.rmse.double().cpu().numpy(),
                   edge_rmse=sol.edge_rmse.double().cpu().numpy())
    d = SO.deviation(got, ref)
    print(f"ring {loss}: deviation {d:.2e} (bound {C.FP32_BOUND:.1e}), iterations {int(sol.iterations[0])} / {int(ref.iterations[0])}, "
          f"errors {C.ring_errors(got)}")
    assert d <= C.FP32_BOUND and int(sol.iterations[0]) == int(ref.iterations[0]) and bool(sol.converged[0])
    assert np.abs(sol.edge_count.cpu().numpy() - ref.edge_count).max() <= 1      # a pair at the gate to within fp32 (the ring's margins are 1e-7)
    assert np.array_equal(got.R[0], sc["R0"][0].astype(np.float64))      # the fixed view


@pytest.mark.parametrize("loss,scale", C.ROBUST)
def test_two_views_one_edge_is_the_robust_pairwise_call_bit_for_bit(lib, dev, loss, scale):
    X, Y, Yn = C.contaminated_pair(*C.EXACT_PAIR)
    nx, ny = X.shape[0], Y.shape[0]
    seg = lambda n: torch.tensor([[0, n]], dtype=I32, device=dev)
    pair = pair_c(lib, dev, True, t(dev, X), seg(nx), t(dev, Y), seg(ny), t(dev, Yn), loss=C.CODES[loss], scale=scale)
    P, N = np.concatenate([Y, X]), np.concatenate([Yn, np.zeros_like(X)])
    eye = torch.eye(3, device=dev).repeat(2, 1, 1)
    o = scene_c(lib, dev, t(dev, P), t(dev, N), torch.tensor([[0, ny], [ny, nx]], dtype=I32, device=dev), torch.tensor([[0, 2]], dtype=I32, device=dev),
                torch.tensor([[1, 0]], dtype=I32, device=dev), eye, torch.zeros((2, 3), device=dev), loss=C.CODES[loss], scale=scale, it=100)
    assert torch.equal(o["R"][0].cpu(), torch.eye(3)) and not o["T"][0].any()      # the first view is fixed at the identity: the pairwise frame
    for name, mine in (("R", o["R"][1]), ("T", o["T"][1]), ("rmse", o["rmse"][0]), ("iterations", o["iterations"][0]), ("converged", o["converged"][0])):
        assert torch.equal(bits(mine), bits(pair[name][0])), (loss, name)
    assert int(o["edge_count"][0]) == nx and abs(float(o["edge_rmse"][0]) - float(o["rmse"][0])) <= 1e-7


def test_a_scene_whose_every_weight_is_zero_stops_and_leaves_the_other_scene_alone(lib, dev):
    ring, far = C.contaminated_ring(), C.far_scene()
    n0, code, scale = ring["P"].shape[0], C.CODES[C.BATCH_LOSS], C.BATCH_SCALE
    rng = np.random.default_rng(8)
    Rf = np.stack([SO.small_rotation(rng, 0.2) for _ in range(2)]).astype(np.float32)      # small: every residual stays several scales
    Tf = rng.uniform(-0.002, 0.002, (2, 3)).astype(np.float32)
    P, N = np.concatenate([ring["P"], far["P"]]), np.concatenate([ring["N"], far["N"]])
    seg = np.concatenate([ring["seg"], far["seg"] + (n0, 0)])
    edges = np.concatenate([SO.ring_edges(), [(6, 7), (7, 6)]])
    R0, T0 = np.concatenate([ring["R0"], Rf]), np.concatenate([ring["T0"], Tf])
    ref = C.refine(far["P"], far["N"], far["seg"], [(0, 2)], [(0, 1), (1, 0)], C.BATCH_LOSS, scale, None, Rf, Tf, relative_rmse_thr=C.THR, margins=False)
    assert ref.wsum[0] == 0.0 and list(ref.edge_count) == [200, 256]
    both = scene_c(lib, dev, t(dev, P), t(dev, N), t(dev, seg, I32), torch.tensor([[0, 6], [6, 2]], dtype=I32, device=dev), t(dev, edges, I32),
                   t(dev, R0), t(dev, T0), loss=code, scale=scale, gate=0.0)
    assert torch.isinf(both["rmse"][1]) and float(both["rmse"][1]) > 0 and int(both["converged"][1]) == 0 and int(both["iterations"][1]) == 0
    assert torch.equal(bits(both["R"][6:]), bits(t(dev, Rf))) and torch.equal(bits(both["T"][6:]), bits(t(dev, Tf)))      # the init, bit for bit
    assert both["edge_count"][12:].cpu().tolist() == [200, 256]          # the pairs are counted; their weights are zero
    alone = scene_c(lib, dev, *ring_tensors(dev), loss=code, scale=scale, gate=0.0)
    for name, sl in (("R", slice(0, 6)), ("T", slice(0, 6)), ("rmse", slice(0, 1)), ("iterations", slice(0, 1)), ("converged", slice(0, 1)),
                     ("edge_rmse", slice(0, 12)), ("edge_count", slice(0, 12))):
        assert torch.equal(bits(both[name][sl]), bits(alone[name])), name
    assert int(both["converged"][0]) == 1 and bool(torch.isfinite(both["rmse"][0]))


# ---- 5. no host synchronisation ----
def test_wrappers_with_a_loss_do_not_synchronise(dev):
    sc = C.contaminated_ring()
    ppp = torch.tensor([[int(n) for n in sc["seg"][:, 1]]], dtype=torch.int64, device=dev)
    rot = t(dev, np.ascontiguousarray(sc["R0"].transpose(0, 2, 1))[None])      # the sampler's convention: registered = cond @ R^T + t
    tr = t(dev, sc["T0"][None])
    Pd, Nd, ed = t(dev, sc["P"]), t(dev, sc["N"]), t(dev, SO.ring_edges(), I32)
    reg = lambda: rap_amd.refine_registration(Pd, ppp, rot, tr, normals=Nd, edges=ed, relative_rmse_thr=C.THR, max_correspondence_distance=C.GATE,
                                              loss="cauchy", loss_scale=C.SCALE["cauchy"])
    clouds, iR, iT = batch_tensors(dev)
    icp = lambda: rap_amd.icp_packed(*clouds[:4], init_R=iR, init_T=iT, relative_rmse_thr=C.THR, y_normals=clouds[4], loss=C.BATCH_LOSS,
                                     loss_scale=C.BATCH_SCALE, return_weights=True, search="grid", **PLANE)
    want_reg, want_icp = reg(), icp()                                    # (also sizes the workspace: growing it is an allocation, not a sync)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got_reg, got_icp = reg(), icp()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(got_reg, want_reg))
    assert same(sol_bits(got_icp[0], got_icp[1]), sol_bits(want_icp[0], want_icp[1]))
    ref = C.ring_solved("cauchy")
    Rg = got_reg[0][0].transpose(1, 2).double().cpu().numpy()
    d = max(np.abs(Rg - ref.R).max(), np.abs(got_reg[1][0].double().cpu().numpy() - ref.T).max(), abs(float(got_reg[2][0]) - ref.rmse[0]))
    print(f"refine_registration(loss='cauchy'): deviation {d:.2e}")
    assert d <= C.FP32_BOUND
    graph = torch.cuda.CUDAGraph()                                       # ... and the pairwise call replays from a graph, as its sibling does
    with torch.cuda.graph(graph):
        cap = icp()
    for _ in range(2):
        for x in (cap[0].R, cap[0].T, cap[0].rmse, cap[1]):
            x.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        assert same(sol_bits(cap[0], cap[1]), sol_bits(want_icp[0], want_icp[1]))
