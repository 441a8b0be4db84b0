"""GPU: the joint multi-view refinement (rap_scene_refine, rap_amd/csrc/scene_refine.hip) against its fp64 yardstick
(tests/scene_refine_oracle.py) and against the pairwise point-to-plane ICP it reduces to.  The bound is scene_refine_oracle.FP32_BOUND:
three times what the yardstick's own fp32 run deviates by, measured in tests/test_scene_refine_host.py, never below 2e-6; the margins
of the "exact" cases are asserted there too, from the yardstick alone.  E = 1 is the reduction test, E = 240 the 16-view parity case."""
import numpy as np
import pytest
import torch

import icp_plane_oracle as PO
import scene_refine_oracle as S
import rap_amd
from rap_amd import _lib
from rap_amd.flow_model import workspace

pytestmark = pytest.mark.gpu
BOUND = S.FP32_BOUND
I32 = torch.int32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def t(a, dev, dtype=None):
    return None if a is None else torch.as_tensor(np.asarray(a), dtype=dtype).to(dev)


def run(dev, P, N, seg, scene_seg, edges, fixed=None, R0=None, T0=None, **kw):
    kw.setdefault("relative_rmse_thr", S.THR)
    sol = rap_amd.refine_scene_packed(t(P, dev), t(seg, dev, I32), t(scene_seg, dev, I32), t(R0, dev), t(T0, dev), edges=t(edges, dev, I32),
                                      normals=t(N, dev), fixed=t(fixed, dev), **kw)
    torch.cuda.synchronize()
    return sol


def num(sol):
    return S.O.Result(R=sol.R.double().cpu().numpy(), T=sol.T.double().cpu().numpy(), rmse=sol.rmse.double().cpu().numpy(),
                      iterations=sol.iterations.cpu().numpy(), converged=sol.converged.cpu().numpy(),
                      edge_rmse=sol.edge_rmse.double().cpu().numpy(), edge_count=sol.edge_count.cpu().numpy())


def bits(sol, views=slice(None), scenes=slice(None)):
    return [sol.R[views].view(I32).cpu(), sol.T[views].view(I32).cpu(), sol.rmse[scenes].view(I32).cpu(), sol.iterations[scenes].cpu(),
            sol.converged[scenes].cpu()]


def same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def held(got, ref, what):
    d = S.deviation(got, ref)
    print(f"{what}: deviation {d:.2e} (bound {BOUND:.1e}), iterations {got.iterations.tolist()} / {ref.iterations.tolist()}")
    assert d <= BOUND, what
    assert np.array_equal(np.isnan(got.edge_rmse), np.isnan(ref.edge_rmse)) and np.array_equal(np.isfinite(got.rmse), np.isfinite(ref.rmse))


# ---- 1. reduction to the pairwise call ----
# identity: the same statements as the pairwise call.  rotated: the target fixed at a rotation about the origin; the world-frame step
# is then the pairwise step conjugated by that rotation, exactly.  posed: a rotated AND translated target.  The update of step 5 applies
# tau directly (p <- p dR^T + tau, not the SE(3) exponential), so with T_b != 0 the world-frame step and the pairwise step differ by
# (dR - I - [omega]x) T_b = O(|omega|^2 |T_b|) -- 3e-3 at the first step of these pairs -- and the two runs agree only where both have
# converged: that case runs both for 12 iterations without the early stop and compares the fixed points.
POSES = {"identity": (0.0, (0, 0, 0), {}), "rotated": (25.0, (0, 0, 0), {}),
         "posed-fixed-point": (25.0, (0.3, -0.2, 0.5), dict(max_iterations=12, relative_rmse_thr=float("-inf")))}


@pytest.mark.parametrize("pose", list(POSES))
@pytest.mark.parametrize("seed,nx,ny", PO.PLANE_PAIRS)
def test_two_views_one_edge_is_the_pairwise_plane_icp(dev, seed, nx, ny, pose):
    degrees, shift, knobs = POSES[pose]
    knobs = dict(dict(max_iterations=100, relative_rmse_thr=1e-6), **knobs)
    X, Y, Yn = PO.pair(seed, nx, ny)
    pair = rap_amd.icp_packed(t(X, dev), torch.tensor([[0, nx]], device=dev), t(Y, dev), torch.tensor([[0, ny]], device=dev),
                              estimation="point_to_plane", search="grid", y_normals=t(Yn, dev), return_Xt=False, **knobs)
    P = np.concatenate([Y, X])
    N = np.concatenate([Yn, np.zeros_like(X)])
    Rb = S.O.rotation((0.2, 0.9, -0.4), degrees).astype(np.float32)
    Tb = np.asarray(shift, np.float32)
    sol = run(dev, P, N, [(0, ny), (ny, nx)], [(0, 2)], [(1, 0)], None, np.stack([Rb, Rb]), np.stack([Tb, Tb]), **knobs)
    R, T = sol.R.double().cpu().numpy(), sol.T.double().cpu().numpy()
    assert np.array_equal(R[0], Rb.astype(np.float64)) and np.array_equal(T[0], Tb.astype(np.float64))
    Rrel, Trel = R[1] @ R[0].T, (T[1] - T[0]) @ R[0].T
    dR, dT = np.abs(Rrel - pair.R[0].double().cpu().numpy()).max(), np.abs(Trel - pair.T[0].double().cpu().numpy()).max()
    dr = abs(float(sol.rmse[0]) - float(pair.rmse[0]))
    print(f"seed {seed} {pose}: |dR| {dR:.2e} |dT| {dT:.2e} |drmse| {dr:.2e}, iterations {int(sol.iterations[0])} / {int(pair.iterations[0])}")
    assert max(dR, dT, dr) <= BOUND
    assert int(sol.iterations[0]) == int(pair.iterations[0]) and bool(sol.converged[0]) == bool(pair.converged[0])
    assert int(sol.edge_count[0]) == nx and abs(float(sol.edge_rmse[0]) - float(sol.rmse[0])) <= 1e-7


# ---- 2. oracle parity ----
@pytest.mark.parametrize("V,seed,gate,variant,exact", S.PARITY_CASES, ids=[f"{c[0]}views-{c[3]}-{'gate' if c[2] else 'nogate'}" for c in S.PARITY_CASES])
def test_scene_matches_the_fp64_yardstick(dev, V, seed, gate, variant, exact):
    sc, ref, f32 = S.parity_scene(V, seed, variant), S.parity_solved(V, seed, gate, variant), S.parity_solved(V, seed, gate, variant, f32=True)
    sol = run(dev, sc["P"], sc["N"], sc["seg"], [(0, V)], S.pairs_of(0, V), S.fixed_of(variant, V)[0], sc["R0"], sc["T0"],
              max_correspondence_distance=gate)
    got = num(sol)
    held(got, ref, f"{V} views, {variant}, gate {gate}")                # the raw output: the minimum-norm step is unique, gauge-free too
    if variant == "none":
        Rg, Tg = S.remove_common_motion(got.R, got.T, ref.R, ref.T, [0])
        d = max(np.abs(Rg - ref.R).max(), np.abs(Tg - ref.T).max())
        print(f"after removing the common rigid motion: {d:.2e}")
        assert d <= BOUND
        moved = max(np.abs(got.R - sc["R0"]).max(), np.abs(got.T - sc["T0"]).max())
        assert moved > 1e-3
    fixed = S.fixed_of(variant, V)[1]
    for v in fixed:
        assert np.array_equal(got.R[v], sc["R0"][v].astype(np.float64)) and np.array_equal(got.T[v], sc["T0"][v].astype(np.float64))
    decided = min(ref.rel_margin, f32.rel_margin) >= S.MARGIN and np.array_equal(ref.iterations, f32.iterations)
    if exact or decided:
        assert np.array_equal(got.iterations, ref.iterations) and np.array_equal(got.converged, ref.converged)
    if exact or gate is None:
        assert np.array_equal(got.edge_count, ref.edge_count)
    else:
        assert np.abs(got.edge_count - ref.edge_count).max() <= 1      # a pair at the gate to within fp32 (margin 5e-8, not 1e-5)
    assert bool(got.converged.all())


# ---- 3. loop closure ----
def test_ring_of_six_views_closes_as_the_yardstick_does(dev):
    sc, ref = S.ring_scene(), S.ring_solved()
    sol = run(dev, sc["P"], sc["N"], sc["seg"], [(0, S.RING_V)], S.ring_edges(), None, sc["R0"], sc["T0"], max_correspondence_distance=S.GATE)
    held(num(sol), ref, "ring")
    assert bool(sol.converged[0]) and int(sol.iterations[0]) == int(ref.iterations[0])


# ---- 4. what does not move ----
def test_fixed_edgeless_gated_out_and_outside_views_keep_every_bit(dev):
    sc = S.parity_scene(3, 9, "first")
    rng = np.random.default_rng(5)
    P, N, seg = sc["P"], sc["N"], sc["seg"]
    # views 0..2: the scene; 3: a copy of view 1 with no edge; 4: outside every scene; 5, 6: a scene whose views are 10 apart
    extra = [P[seg[1, 0]:seg[1, 0] + seg[1, 1]]] * 2 + [P[seg[0, 0]:seg[0, 0] + 200], P[seg[0, 0]:seg[0, 0] + 200]]
    extra_n = [N[seg[1, 0]:seg[1, 0] + seg[1, 1]]] * 2 + [N[seg[0, 0]:seg[0, 0] + 200], N[seg[0, 0]:seg[0, 0] + 200]]
    Pall, Nall = np.concatenate([P] + extra), np.concatenate([N] + extra_n)
    lens = [int(n) for n in seg[:, 1]] + [int(seg[1, 1])] * 2 + [200, 200]
    starts = np.cumsum([0] + lens[:-1])
    vseg = np.stack([starts, lens], axis=1)
    R0 = np.concatenate([sc["R0"], np.stack([S.small_rotation(rng, 20).astype(np.float32) for _ in range(4)])])
    T0 = np.concatenate([sc["T0"], rng.uniform(-1, 1, (4, 3)).astype(np.float32)])
    T0[2] += 10.0                                                        # view 2: every pair with it is outside the gate
    T0[6] = T0[5] + 10.0
    R0[6] = R0[5]
    # scene 0 = views 0..3, view 4 in no scene, scene 1 = views 5, 6
    edges = [(1, 0), (0, 1), (2, 0), (0, 2), (2, 1), (5, 6), (6, 5), (4, 0), (0, 4)]
    sol = run(dev, Pall, Nall, vseg, [(0, 4), (5, 2)], edges, None, R0, T0, max_correspondence_distance=S.GATE)
    R, T = sol.R.cpu().numpy(), sol.T.cpu().numpy()
    for v in (0, 2, 3, 4, 5, 6):
        assert np.array_equal(R[v].view(np.int32), R0[v].view(np.int32)) and np.array_equal(T[v].view(np.int32), T0[v].view(np.int32)), v
    assert np.abs(R[1] - R0[1]).max() > 1e-3 and bool(sol.converged[0]) and int(sol.iterations[0]) >= 2
    assert torch.isinf(sol.rmse[1]) and int(sol.iterations[1]) == 0 and not bool(sol.converged[1])
    cnt = sol.edge_count.cpu().numpy()
    assert cnt[0] > 0 and cnt[1] > 0 and not cnt[2:].any()
    assert bool(torch.isnan(sol.edge_rmse[2:]).all())                   # gated out: 0 pairs; ignored: NaN as well
    ref = S.refine(Pall, Nall, vseg, [(0, 4), (5, 2)], edges, None, R0, T0, relative_rmse_thr=S.THR, max_correspondence_distance=S.GATE, margins=False)
    held(num(sol), ref, "still views")


# ---- 5. tables ----
def _batch():
    """three scenes in one view table -- A: 3 views, B: 4 views plus an empty and a negative-length view, C: 17 views of 5 rows (left out at
    max_views = 16) -- and an edge table with everything that must be ignored in it"""
    a, b = S.parity_scene(3, 9, "first"), S.parity_scene(4, 86, "two")
    nA, nB = a["P"].shape[0], b["P"].shape[0]
    tiny = np.tile(a["P"][:5], (17, 1))
    P = np.concatenate([a["P"], b["P"], tiny])
    N = np.concatenate([a["N"], b["N"], np.tile(a["N"][:5], (17, 1))])
    seg = [tuple(r) for r in a["seg"]] + [(s + nA, n) for s, n in b["seg"]] + [(nA + 7, 0), (nA + 9, -4)] + [(nA + nB + 5 * i, 5) for i in range(17)]
    R0 = np.concatenate([a["R0"], b["R0"], np.tile(np.eye(3, dtype=np.float32), (19, 1, 1))])
    T0 = np.concatenate([a["T0"], b["T0"], np.zeros((19, 3), np.float32)])
    scenes = {"A": (0, 3), "B": (3, 6), "C": (9, 17)}
    eA = [tuple(e) for e in S.pairs_of(0, 3)] + [(1, 1), (0, 1)]         # a == b; a duplicate, which counts twice
    eB = [tuple(e) for e in S.pairs_of(3, 4)] + [(3, 7), (8, 4), (7, 8)]  # to and from the empty and the negative-length view
    eC = [(9, 10), (10, 9)]
    junk = [(0, 4), (5, 2), (-1, 0), (0, 26), (40, 1), (12, 3)]          # across scenes, out of range, into the scene that is left out
    return P, N, np.asarray(seg, np.int32), R0, T0, scenes, eA, eB, eC, junk


def test_tables_scene_order_edge_order_and_everything_that_is_ignored(dev):
    P, N, seg, R0, T0, scenes, eA, eB, eC, junk = _batch()
    fixedB = np.zeros(len(seg), np.uint8)
    fixedB[0] = 1
    fixedB[[4, 6]] = 1                                                  # scene B: its "two" variant (views 1 and 3 of the scene)
    order1 = [scenes["A"], scenes["B"], scenes["C"]]
    edges1 = eA + junk[:3] + eB + eC + junk[3:]
    sol1 = run(dev, P, N, seg, order1, edges1, fixedB, R0, T0)
    ref = S.refine(P, N, seg, order1, edges1, fixedB, R0, T0, relative_rmse_thr=S.THR, margins=False)
    held(num(sol1), ref, "batch")
    assert np.array_equal(sol1.edge_count.cpu().numpy(), ref.edge_count) and ref.edge_count[len(eA) - 1] == ref.edge_count[0] > 0
    live = sol1.edge_count.cpu().numpy() > 0
    assert live.sum() == 6 + 1 + 12 and not live[len(eA) - 2]
    # the scene that is left out: NaN / 0 / 0 and the init; its neighbours are not affected
    assert torch.isnan(sol1.rmse[2]) and int(sol1.iterations[2]) == 0 and not bool(sol1.converged[2])
    assert np.array_equal(sol1.R[9:].cpu().numpy(), R0[9:]) and np.array_equal(sol1.T[7:9].cpu().numpy(), T0[7:9])
    assert bool(sol1.converged[:2].all())
    # another scene order (edges follow their scenes, each scene's own order kept): the same bits, scene by scene
    order2 = [scenes["C"], scenes["B"], scenes["A"]]
    edges2 = junk + eC + eB + eA
    sol2 = run(dev, P, N, seg, order2, edges2, fixedB, R0, T0)
    assert same_bits(bits(sol1, slice(None), [0, 1, 2]), bits(sol2, slice(None), [2, 1, 0]))
    # another edge order inside the scenes: the sums of H take another order, the result stays within the bound
    edges3 = eA[::-1] + eB[::-1] + eC + junk
    sol3 = run(dev, P, N, seg, order1, edges3, fixedB, R0, T0)
    got3 = num(sol3)
    got3.edge_rmse = ref.edge_rmse                                       # the edges sit in other rows: poses and rmse are compared
    held(got3, ref, "edge order")
    # scene A alone (its own view table) and inside the batch: the same bits; and whatever the workspace held before
    a = S.parity_scene(3, 9, "first")
    alone = run(dev, a["P"], a["N"], a["seg"], [(0, 3)], eA, None, a["R0"], a["T0"])
    assert same_bits(bits(alone), bits(sol1, slice(0, 3), slice(0, 1)))
    with torch.inference_mode():                                         # the buffer may have been made under inference mode by another test
        workspace(dev, 1).fill_(0x5A)
    again = run(dev, a["P"], a["N"], a["seg"], [(0, 3)], eA, None, a["R0"], a["T0"])
    with torch.inference_mode():
        workspace(dev, 1).fill_(0xFF)
    third = run(dev, a["P"], a["N"], a["seg"], [(0, 3)], eA, None, a["R0"], a["T0"])
    assert same_bits(bits(alone), bits(again)) and same_bits(bits(alone), bits(third))
    assert torch.equal(alone.edge_count, again.edge_count) and torch.equal(alone.edge_rmse.view(I32), third.edge_rmse.view(I32))


# ---- 6. work-list edges ----
def _worklist_scene():
    rows = (257, 1, 255, 256, 257, 513) + (64,) * 10
    sc = S.make_scene(77, rows, S.windows_overlapping(16, 0.9), start_true=(0,))
    edges = [(0, j) for j in range(1, 16)] + [(j, 0) for j in range(1, 6)]
    return sc, rows, np.asarray(edges, np.int32)


def test_work_list_tile_edges_one_source_of_fifteen_edges_and_the_row_budget(dev):
    sc, rows, edges = _worklist_scene()
    total = 15 * rows[0] + sum(rows[1:6])
    args = (sc["P"], sc["N"], sc["seg"], [(0, 16)], edges, None, sc["R0"], sc["T0"])
    ref = S.refine(*args, relative_rmse_thr=S.THR, margins=False)
    free = run(dev, *args)
    held(num(free), ref, "work list")
    assert np.array_equal(free.edge_count.cpu().numpy(), ref.edge_count) and ref.edge_count[15] == 1 and ref.edge_count[19] == 513
    exact = run(dev, *args, row_budget=total)
    assert same_bits(bits(free), bits(exact)) and torch.equal(free.edge_count, exact.edge_count)
    short = run(dev, *args, row_budget=total - 1)
    ref_short = S.refine(sc["P"], sc["N"], sc["seg"], [(0, 16)], edges[:-1], None, sc["R0"], sc["T0"], relative_rmse_thr=S.THR, margins=False)
    got = num(short)
    assert got.edge_count[-1] == 0 and np.isnan(got.edge_rmse[-1]) and np.array_equal(got.edge_count[:-1], ref_short.edge_count)
    got.edge_rmse, got.edge_count = got.edge_rmse[:-1], got.edge_count[:-1]
    held(got, ref_short, "one row short")
    assert np.array_equal(S.refine(*args, relative_rmse_thr=S.THR, margins=False, row_budget=total - 1).edge_count[:-1], ref_short.edge_count)


# ---- 7. planar scene ----
def test_planar_scene_does_not_slide(dev):
    sc = S.planar_scene()
    args = (sc["P"], sc["N"], sc["seg"], [(0, 3)], S.pairs_of(0, 3), None, sc["R0"], sc["T0"])
    ref = S.planar_solved()
    sol = run(dev, *args)
    got = num(sol)
    held(got, ref, "planar")
    assert np.isfinite(got.R).all() and np.abs(np.linalg.det(got.R) - 1.0).max() < 1e-5
    assert np.abs(got.R @ np.transpose(got.R, (0, 2, 1)) - np.eye(3)).max() < 1e-5 and float(got.rmse[0]) < 1e-3


# ---- 8. the sampler's convention ----
def test_refine_registration_is_refine_scene_packed_on_the_transposed_poses_without_a_sync(dev):
    a, b = S.parity_scene(3, 9, "first"), S.parity_scene(4, 86, "two")
    cloud = t(np.concatenate([a["P"], b["P"]]), dev)
    normals = t(np.concatenate([a["N"], b["N"]]), dev)
    ppp = torch.tensor([[int(a["seg"][0, 1]), int(a["seg"][1, 1]), 0, int(a["seg"][2, 1])], [int(n) for n in b["seg"][:, 1]]], device=dev)
    R0 = np.zeros((2, 4, 3, 3), np.float32)
    T0 = np.zeros((2, 4, 3), np.float32)
    R0[0, [0, 1, 3]], T0[0, [0, 1, 3]] = np.transpose(a["R0"], (0, 2, 1)), a["T0"]
    R0[1], T0[1] = np.transpose(b["R0"], (0, 2, 1)), b["T0"]
    anchors = torch.tensor([[False, True, True, False], [False, False, True, False]], device=dev)      # sample 0 flags its empty part too
    cu = torch.tensor([0, a["P"].shape[0], cloud.shape[0]], dtype=I32, device=dev)
    rot, trans = t(R0, dev), t(T0, dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                              # no host synchronisation in the call
    try:
        R, T, rmse = rap_amd.refine_registration(cloud, ppp, rot, trans, anchors, cu_seqlens_batch=cu, normals=normals, relative_rmse_thr=S.THR)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    n0, n1 = (int(v) for v in a["seg"][:2, 1])
    seg = [(0, n0), (n0, n1), (n0 + n1, 0), (n0 + n1, int(a["seg"][2, 1]))] + [(int(s) + a["P"].shape[0], int(n)) for s, n in b["seg"]]
    fixed = np.asarray([0, 1, 0, 0, 0, 0, 1, 0], np.uint8)
    sol = rap_amd.refine_scene_packed(cloud, t(seg, dev, I32), t([(0, 4), (4, 4)], dev, I32), rot.reshape(8, 3, 3).transpose(1, 2),
                                      trans.reshape(8, 3), normals=normals, fixed=t(fixed, dev), relative_rmse_thr=S.THR)
    assert torch.equal(R.reshape(8, 3, 3), sol.R.transpose(1, 2)) and torch.equal(T.reshape(8, 3), sol.T) and torch.equal(rmse, sol.rmse)
    assert R.shape == (2, 4, 3, 3) and T.shape == (2, 4, 3) and rmse.shape == (2,)
    assert not R[0, 2].any() and not T[0, 2].any()                      # the empty part keeps its zero rows
    assert torch.equal(R[0, 1], rot[0, 1]) and torch.equal(R[1, 2], rot[1, 2]) and bool(sol.converged.all())
    assert (R[0, 0] - rot[0, 0]).abs().max() > 1e-3                      # slot 0 is no anchor here: it moved
    ref = S.refine(cloud.cpu().numpy(), normals.cpu().numpy(), seg, [(0, 4), (4, 4)], S.all_pairs([(0, 4), (4, 4)]), fixed,
                   np.transpose(R0.reshape(8, 3, 3), (0, 2, 1)), T0.reshape(8, 3), relative_rmse_thr=S.THR, margins=False)
    held(num(sol), ref, "registration batch (all ordered pairs formed on the device)")
