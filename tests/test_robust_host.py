"""CPU: the robust losses of the point-to-plane calls.  A host build of rap_amd/csrc/robust_loss.h (the statements the device epilogue
runs) agrees with the table of include/rapflow.h; the three robust entry points and the Python wrappers refuse bad arguments before
anything touches the device, and the workspace twins are host arithmetic; the yardstick (tests/robust_cases.py) with loss none IS the two
existing yardsticks; and the inputs the GPU tests (tests/test_robust_gpu.py) hold the kernels to are fit for it -- the margins of the
cases that are compared exactly, the fp32 bounds and the property that makes the feature worth having are all measured from the
yardstick alone, not from the code under test."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import icp_oracle as O
import icp_plane_oracle as PO
import robust_cases as C
import scene_refine_oracle as SO
from rap_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, ONE = ctypes.c_void_p(0), ctypes.c_void_p(256)      # NULL; a non-NULL sentinel -- every call below fails before a pointer is used
EPS = np.finfo(np.float64).eps


# ---- the header ----
@pytest.fixture(scope="module")
def header(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("host") / "librobust_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", out, os.path.join(ROOT, "tests", "host", "robust_host.cpp")])
    lib = ctypes.CDLL(out)
    D = np.ctypeslib.ndpointer(np.float64, flags="C")
    lib.robust_eval.argtypes = [ctypes.c_int, D, ctypes.c_int, ctypes.c_double, D, D]
    lib.robust_eval.restype = None

    def run(loss, r, k):
        r = np.ascontiguousarray(r, np.float64)
        w, rho = np.empty_like(r), np.empty_like(r)
        lib.robust_eval(C.CODES[loss], r, r.size, float(k), w, rho)
        return w, rho
    run.lib = lib
    return run


def residuals(k):
    """across |r| = k and exactly at it, r = 0, tiny and large |r|, both signs"""
    mags = [0.0, 1e-300, 1e-12 * k, 0.25 * k, 0.5 * k, 0.999 * k, np.nextafter(k, 0.0), k, np.nextafter(k, np.inf), 1.001 * k, 2.0 * k,
            10.0 * k, 1e3 * k, 1e6 * k, 1e12 * k]
    return np.asarray([s * m for m in mags for s in (1.0, -1.0)])


@pytest.mark.parametrize("loss", C.LOSSES)
def test_header_weight_and_cost_are_the_tables(header, loss):
    assert [header.lib.robust_code(i) for i in range(4)] == [0, 1, 2, 3] == [C.CODES[l] for l in C.LOSSES]
    for k in (0.01, float(np.float32(0.03)), 1.0, 37.5):
        r = residuals(k)
        w, rho = header(loss, r, k)
        w_ref, rho_ref = C.weight_cost(loss, r, k)
        # the same few fp64 operations in another order: a few ulp of the value (log1p through the platform's libm on both sides)
        assert np.all(np.abs(w - w_ref) <= 8 * EPS * np.abs(w_ref)), (loss, k, np.abs(w - w_ref).max())
        assert np.all(np.abs(rho - rho_ref) <= 8 * EPS * np.abs(rho_ref) + 1e-300), (loss, k, np.abs(rho - rho_ref).max())
        assert np.all(w >= 0.0) and np.all(w <= 1.0) and np.all(rho >= 0.0) and np.all(np.isfinite(w)) and np.all(np.isfinite(rho))
        at0 = np.flatnonzero(r == 0.0)
        assert np.all(w[at0] == 1.0) and np.all(rho[at0] == 0.0)
        assert np.array_equal(w[0::2], w[1::2]) and np.array_equal(rho[0::2], rho[1::2])      # even in r
        if loss == "none":
            assert np.all(w == 1.0) and np.array_equal(rho, 0.5 * r * r)
        if loss == "tukey":
            assert np.all(w[np.abs(r) > k] == 0.0) and np.all(rho[np.abs(r) > k] == k * k / 6.0) and w[np.abs(r) == k].max() == 0.0
        if loss == "huber":
            assert np.all(w[np.abs(r) <= k] == 1.0)
        # continuous across |r| = k: the neighbours of k on either side give the value at k up to rounding
        lo, at, hi = (header(loss, np.asarray([x]), k) for x in (np.nextafter(k, 0.0), k, np.nextafter(k, np.inf)))
        for j in (0, 1):
            scale = 1.0 if j == 0 else k * k
            assert abs(lo[j][0] - at[j][0]) <= 16 * EPS * scale and abs(hi[j][0] - at[j][0]) <= 16 * EPS * scale, (loss, k, j)


@pytest.mark.parametrize("loss", C.LOSSES[1:])
def test_header_weight_is_the_derivative_of_the_cost_over_r(header, loss):
    k = 0.03
    r = np.concatenate([np.linspace(0.05, 0.95, 19), np.linspace(1.05, 6.0, 23)]) * k      # away from the kink of the second derivative
    h = 1e-6 * k
    w, _ = header(loss, r, k)
    _, up = header(loss, r + h, k)
    _, dn = header(loss, r - h, k)
    assert np.abs((up - dn) / (2 * h) - w * r).max() <= 1e-8 * k      # central difference: O(h^2 rho''') + eps rho / h


# ---- refusals ----
def pair_call(lib, grid, **kw):
    a = dict(X=ONE, xs=ONE, Y=ONE, ys=ONE, Yn=ONE, K=3, NX=1000, NY=900, iR=N, iT=N, it=10, thr=1e-6, gate=0.0, R=ONE, T=ONE, rmse=ONE,
             iters=ONE, conv=ONE, Xt=N, loss=1, scale=0.01, weights=N, ws=ONE, wsb=1 << 30)
    a.update(kw)
    fn = lib.rap_icp_plane_grid_robust if grid else lib.rap_icp_plane_robust
    return fn(a["X"], a["xs"], a["Y"], a["ys"], a["Yn"], a["K"], a["NX"], a["NY"], a["iR"], a["iT"], a["it"], a["thr"], a["gate"], a["R"], a["T"],
              a["rmse"], a["iters"], a["conv"], a["Xt"], a["loss"], a["scale"], a["weights"], a["ws"], a["wsb"], N)


def scene_call(lib, **kw):
    a = dict(P=ONE, Pn=ONE, vs=ONE, V=8, n=4000, ss=ONE, S=2, ed=ONE, E=24, budget=12000, mv=16, fixed=N, iR=N, iT=N, it=10, thr=1e-6, gate=0.0,
             R=ONE, T=ONE, rmse=ONE, iters=ONE, conv=ONE, er=N, ec=N, loss=3, scale=0.03, ws=ONE, wsb=1 << 30)
    a.update(kw)
    return lib.rap_scene_refine_robust(a["P"], a["Pn"], a["vs"], a["V"], a["n"], a["ss"], a["S"], a["ed"], a["E"], a["budget"], a["mv"],
                                       a["fixed"], a["iR"], a["iT"], a["it"], a["thr"], a["gate"], a["R"], a["T"], a["rmse"], a["iters"],
                                       a["conv"], a["er"], a["ec"], a["loss"], a["scale"], a["ws"], a["wsb"], N)


BAD_SCALES = (0.0, -0.01, float("nan"), float("inf"), -float("inf"))


@pytest.mark.parametrize("grid", [False, True])
def test_pairwise_robust_entry_points_refuse_bad_arguments_without_a_gpu(grid):
    lib = _lib.load()
    assert lib.rap_version() == 6                                        # the addition is additive
    call = lambda **kw: pair_call(lib, grid, **kw)
    for loss in (-1, 4, 17, -(1 << 31)):
        assert call(loss=loss) == -1, loss
    for loss in (1, 2, 3):
        for s in BAD_SCALES:
            assert call(loss=loss, scale=s) == -1, (loss, s)
    for s in BAD_SCALES:                                                 # loss none ignores the scale: the call gets as far as its workspace
        assert call(loss=0, scale=s, ws=N) == -2, s
    for name in ("X", "xs", "Y", "ys", "Yn", "R", "T", "rmse", "iters", "conv"):      # whatever the sibling refuses
        assert call(**{name: N}) == -1, name
    for name, bad in (("K", (0, -1) + ((65536,) if grid else ())), ("NX", (0, -3, 1 << 31)), ("NY", (0, -3, 1 << 31)), ("it", (0, -1)),
                      ("thr", (float("nan"),)), ("gate", (float("nan"),))):
        for v in bad:
            assert call(**{name: v}) == -1, (name, v)
    need = lib.rap_icp_plane_grid_robust_workspace_bytes(1000, 900, 3) if grid else lib.rap_icp_plane_robust_workspace_bytes(1000, 3)
    assert need > 0 and call(ws=N) == -2 and call(wsb=need - 1) == -2 and call(wsb=0) == -2
    assert call(weights=ONE, wsb=need - 1) == -2


def test_scene_robust_entry_point_refuses_bad_arguments_without_a_gpu():
    lib = _lib.load()
    for loss in (-1, 4, 99):
        assert scene_call(lib, loss=loss) == -1, loss
    for loss in (1, 2, 3):
        for s in BAD_SCALES:
            assert scene_call(lib, loss=loss, scale=s) == -1, (loss, s)
    for s in BAD_SCALES:
        assert scene_call(lib, loss=0, scale=s, ws=N) == -2, s
    for name in ("P", "Pn", "vs", "ss", "ed", "R", "T", "rmse", "iters", "conv"):
        assert scene_call(lib, **{name: N}) == -1, name
    for name, bad in (("V", (0, -1, 65536)), ("S", (0, -2)), ("E", (0, -1, 65536)), ("n", (0, -5, 1 << 31)), ("budget", (0, -1, 1 << 40)),
                      ("mv", (1, 0, 17, -3)), ("it", (0, -1)), ("thr", (float("nan"),)), ("gate", (float("nan"),))):
        for v in bad:
            assert scene_call(lib, **{name: v}) == -1, (name, v)
    need = lib.rap_scene_refine_robust_workspace_bytes(4000, 8, 2, 24, 12000, 16)
    assert need > 0 and scene_call(lib, ws=N) == -2 and scene_call(lib, wsb=need - 1) == -2 and scene_call(lib, wsb=0) == -2


def test_robust_workspace_twins_are_host_arithmetic():
    lib = _lib.load()
    up = lambda n: -(-n // 256) * 256
    for bad in ((0, 3), (-1, 3), (100, 0), (100, -2)):
        assert lib.rap_icp_plane_robust_workspace_bytes(*bad) == 0 == lib.rap_icp_plane_workspace_bytes(*bad), bad
    for bad in ((0, 50, 3), (100, 0, 3), (100, 50, 0), (-1, 50, 3)):
        assert lib.rap_icp_plane_grid_robust_workspace_bytes(*bad) == 0 == lib.rap_icp_plane_grid_workspace_bytes(*bad), bad
    for n, K in ((1, 1), (255, 1), (256, 2), (1000, 3), (100_000, 300)):
        items = n // 256 + K + 1                                         # a partial grows from 28 to 29 fp64 moments (W) beside its count
        grow = up(items * 240) - up(items * 232)
        assert lib.rap_icp_plane_robust_workspace_bytes(n, K) == lib.rap_icp_plane_workspace_bytes(n, K) + grow, (n, K)
        for ny in (1, 777, 50_000):
            assert lib.rap_icp_plane_grid_robust_workspace_bytes(n, ny, K) == lib.rap_icp_plane_grid_workspace_bytes(n, ny, K) + grow, (n, ny, K)
    q, qr = lib.rap_scene_refine_workspace_bytes, lib.rap_scene_refine_robust_workspace_bytes
    for bad in ((0, 8, 2, 24, 100, 16), (100, 0, 2, 24, 100, 16), (100, 8, 0, 24, 100, 16), (100, 8, 2, 0, 100, 16), (100, 8, 2, 24, 0, 16),
                (100, 8, 2, 24, 100, 1), (100, 8, 2, 24, 100, 17), (100, 65536, 2, 24, 100, 16), (100, 8, 2, 65536, 100, 16)):
        assert qr(*bad) == 0 == q(*bad), bad
    for n, V, Sn, E, budget in ((1, 1, 1, 1, 1), (1000, 3, 1, 6, 2000), (4000, 8, 2, 24, 12000), (200_000, 64, 4, 960, 3_000_000)):
        items = budget // 256 + E + 1                                    # the item partials and the per-edge sums both grow
        grow = up(items * 240) - up(items * 232) + up(E * 240) - up(E * 232)
        assert qr(n, V, Sn, E, budget, 16) == q(n, V, Sn, E, budget, 16) + grow == qr(n, V, Sn, E, budget, 2), (n, V, Sn, E, budget)


def test_python_wrappers_refuse_bad_losses_before_anything_else():
    import rap_amd
    X, Y = torch.zeros(10, 3), torch.zeros(12, 3)
    seg = torch.tensor([[0, 10]])
    plane = dict(estimation="point_to_plane")
    P, vseg, sc = torch.zeros(20, 3), torch.tensor([[0, 10], [10, 10]]), torch.tensor([[0, 2]])
    reg = (P, torch.tensor([[10, 10]]), torch.zeros(1, 2, 3, 3), torch.zeros(1, 2, 3))
    bad = (dict(loss="l2", loss_scale=0.01), dict(loss="Huber", loss_scale=0.01), dict(loss=1, loss_scale=0.01),      # an unknown loss
           dict(loss="huber"), dict(loss_scale=0.01),                                                                 # one without the other
           dict(loss="tukey", loss_scale=0.0), dict(loss="tukey", loss_scale=-1.0), dict(loss="cauchy", loss_scale=float("nan")),
           dict(loss="cauchy", loss_scale=float("inf")))
    for kw in bad:
        with pytest.raises(ValueError):
            rap_amd.icp_packed(X, seg, Y, torch.tensor([[0, 12]]), **plane, **kw)
        with pytest.raises(ValueError):
            rap_amd.iterative_closest_point(X, Y, **plane, **kw)
        with pytest.raises(ValueError):
            rap_amd.refine_scene_packed(P, vseg, sc, **kw)
        with pytest.raises(ValueError):
            rap_amd.refine_registration(*reg, **kw)
    for kw in (dict(loss="huber", loss_scale=0.01), dict(return_weights=True)):      # point-to-point takes neither
        for est in (dict(), dict(estimation="point_to_point")):
            with pytest.raises(ValueError):
                rap_amd.icp_packed(X, seg, Y, torch.tensor([[0, 12]]), **est, **kw)
            with pytest.raises(ValueError):
                rap_amd.iterative_closest_point(X, Y, **est, **kw)
    with pytest.raises(_lib.RapError):                                   # a good loss gets as far as the CPU tensors
        rap_amd.icp_packed(X, seg, Y, torch.tensor([[0, 12]]), **plane, loss="huber", loss_scale=0.01, return_weights=True)
    with pytest.raises(_lib.RapError):
        rap_amd.refine_scene_packed(P, vseg, sc, loss="tukey", loss_scale=0.03)
    assert rap_amd.ICPSolution._fields == ("converged", "rmse", "Xt", "R", "T", "iterations")      # existing code unpacks it


# ---- the yardstick ----
def same_result(a, b, names):
    return all(np.array_equal(np.asarray(getattr(a, n)), np.asarray(getattr(b, n)), equal_nan=True) for n in names)


def test_loss_none_in_the_new_yardstick_is_the_existing_yardsticks():
    names = ("R", "T", "rmse", "iterations", "converged", "Xt", "count")
    for f32 in (False, True):
        X, Y, Yn = C.contaminated_pair(*C.EXACT_PAIR)
        assert same_result(C.icp_plane(X, Y, Yn, relative_rmse_thr=C.THR, f32=f32, margins=False),
                           PO.icp_plane(X, Y, Yn, relative_rmse_thr=C.THR, f32=f32, margins=False), names)
        g = PO.GATE_CASE
        X, Y, Yn = PO.pair(g["seed"], g["nx"], g["ny"], g["x_range"], g["y_range"])
        new = C.icp_plane(X, Y, Yn, "none", 123.0, init=O.INIT, max_correspondence_distance=PO.GATE, f32=f32, margins=False)
        old = PO.icp_plane(X, Y, Yn, init=O.INIT, max_correspondence_distance=PO.GATE, f32=f32, margins=False)
        assert same_result(new, old, names) and new.wsum == new.count and set(np.unique(new.weights)) <= {0.0, 1.0}
        names_s = ("R", "T", "rmse", "iterations", "converged", "edge_rmse", "edge_count", "live")
        assert same_result(C.ring_solved("none", f32=f32, contaminated=False), SO.ring_solved(f32), names_s)
        sc = C.contaminated_ring()
        old = SO.refine(sc["P"], sc["N"], sc["seg"], [(0, SO.RING_V)], SO.ring_edges(), None, sc["R0"], sc["T0"], relative_rmse_thr=C.THR,
                        max_correspondence_distance=C.GATE, f32=f32, margins=False)
        assert same_result(C.ring_solved("none", f32=f32), old, names_s)
    V, seed, gate, variant, _ = SO.PARITY_CASES[1]
    sc = SO.parity_scene(V, seed, variant)
    new = C.refine(sc["P"], sc["N"], sc["seg"], [(0, V)], SO.pairs_of(0, V), "none", None, SO.fixed_of(variant, V)[0], sc["R0"], sc["T0"],
                   relative_rmse_thr=SO.THR, max_correspondence_distance=gate, margins=False)
    assert same_result(new, SO.parity_solved(V, seed, gate, variant), names_s)


@pytest.mark.parametrize("loss", C.LOSSES)
def test_exact_pair_keeps_its_margins_under_every_loss(loss):
    ref = C.pair_solved(*C.EXACT_PAIR, loss, margins=True)
    f32 = C.pair_solved(*C.EXACT_PAIR, loss, f32=True, margins=True)
    print(f"{loss}: neighbour margin {ref.nn_margin:.2e} / {f32.nn_margin:.2e}, rel margin {ref.rel_margin:.2e} / {f32.rel_margin:.2e}, "
          f"iterations {ref.iterations} / {f32.iterations}, rels {ref.rels}")
    assert ref.nn_margin >= C.MARGIN and f32.nn_margin >= C.MARGIN
    assert ref.rel_margin >= C.MARGIN and f32.rel_margin >= C.MARGIN
    assert ref.iterations == f32.iterations >= 3 and ref.converged and f32.converged and ref.count == C.EXACT_PAIR[1]
    if loss != "none":                                                   # the contaminated rows carry next to no weight, the others nearly all
        lifted = np.arange(0, C.EXACT_PAIR[1], 5)
        rest = np.setdiff1d(np.arange(C.EXACT_PAIR[1]), lifted)
        assert ref.weights[lifted].max() < 0.2 and np.median(ref.weights[rest]) > 0.8
        assert (ref.weights[lifted] == 0.0).all() == (loss == "tukey")


def test_gated_pair_keeps_its_margins_and_has_rows_of_every_kind():
    ref, f32 = C.gated_solved(margins=True), C.gated_solved(f32=True, margins=True)
    for r in (ref, f32):
        assert r.nn_margin >= C.MARGIN and r.gate_margin >= C.MARGIN and r.rel_margin >= C.MARGIN
    assert ref.iterations == f32.iterations and ref.converged
    nx = C.EXACT_PAIR[1]
    assert 0 < (ref.weights > 0).sum() < ref.count < nx                  # gated out; counted with weight zero; counted with a weight


def test_batch_problems_are_what_the_gpu_test_takes_them_for():
    b, ref, f32 = C.batch(), C.batch_solved(), C.batch_solved(True)
    assert [int(n) for n in b["x_seg"][:7, 1]] == list(C.BATCH_LENGTHS) and b["parts"][7] is None and b["far"] == 8
    far = ref[b["far"]]
    assert far.count == 200 and far.wsum == 0.0 and np.isinf(far.rmse) and far.iterations == 0 and not far.converged
    assert np.array_equal(far.R, b["init_R"][b["far"]].astype(np.float64)) and not far.weights.any()
    assert ref[0].count == 1 and ref[0].wsum == 0.0                      # its one row is a lifted one: W == 0 from a single pair
    for k in range(1, 7):
        assert ref[k].iterations == f32[k].iterations >= 3 and ref[k].converged and ref[k].wsum > 0.0, k
        assert ref[k].rel_margin >= C.MARGIN and f32[k].rel_margin >= C.MARGIN, k      # the iteration count is decided


def test_ring_iteration_counts_are_decided():
    for loss in C.LOSSES:
        ref, f32 = C.ring_solved(loss), C.ring_solved(loss, f32=True)
        print(f"ring, {loss}: iterations {ref.iterations[0]} / {f32.iterations[0]}, rel margin {ref.rel_margin:.2e} / {f32.rel_margin:.2e}")
        assert ref.rel_margin >= C.MARGIN and f32.rel_margin >= C.MARGIN and ref.iterations[0] == f32.iterations[0] and ref.converged[0]
    fs = C.far_scene()
    r = C.refine(fs["P"], fs["N"], fs["seg"], [(0, 2)], [(0, 1), (1, 0)], C.BATCH_LOSS, C.BATCH_SCALE, relative_rmse_thr=C.THR, margins=False)
    assert r.wsum[0] == 0.0 and np.isinf(r.rmse[0]) and r.iterations[0] == 0 and list(r.edge_count) == [200, 256]


def test_fp32_bounds_are_three_times_the_yardsticks_own_fp32_deviation():
    pose, weight = 0.0, 0.0
    for loss in C.LOSSES:
        p, w = C.pair_deviation(C.pair_solved(*C.EXACT_PAIR, loss), C.pair_solved(*C.EXACT_PAIR, loss, f32=True))
        ring = SO.deviation(C.ring_solved(loss), C.ring_solved(loss, f32=True))
        print(f"{loss}: pair poses/rmse {p:.2e}, weights {w:.2e}; ring {ring:.2e}")
        pose, weight = max(pose, p, ring), max(weight, w)
    for k, (a, f) in enumerate(zip(C.batch_solved(), C.batch_solved(True))):
        if a is not None and np.isfinite(a.rmse):
            p, w = C.pair_deviation(a, f)
            print(f"batch problem {k}: poses/rmse {p:.2e}, weights {w:.2e}")
            pose, weight = max(pose, p), max(weight, w)
    print(f"largest: poses/rmse {pose:.2e} (recorded {C.FP32_MEASURED:.1e}), weights {weight:.2e} (recorded {C.WEIGHT_MEASURED:.1e})")
    assert pose <= C.FP32_MEASURED and C.FP32_BOUND == max(3 * C.FP32_MEASURED, 2e-6)
    assert weight <= C.WEIGHT_MEASURED and C.WEIGHT_BOUND == max(3 * C.WEIGHT_MEASURED, 2e-6)
    assert C.FP32_MEASURED <= 2 * pose and C.WEIGHT_MEASURED <= 2 * weight      # the record is the measurement, not a guess above it


# ---- the property ----
@pytest.mark.parametrize("seed,nx,ny", C.PROPERTY_PAIRS)
def test_every_robust_loss_ends_closer_to_the_truth_on_a_contaminated_pair(seed, nx, ny):
    plain_t, plain_r = C.pair_errors(C.pair_solved(seed, nx, ny, "none"))
    clean_t, _ = C.pair_errors(C.pair_solved(seed, nx, ny, "none", contaminated=False))
    assert plain_t > 5 * clean_t                                         # the contamination does pull the plain estimate
    for loss, _ in C.ROBUST:
        t, r = C.pair_errors(C.pair_solved(seed, nx, ny, loss))
        print(f"({seed}, {nx}, {ny}) {loss}: translation {plain_t / t:.1f} x closer, rotation {plain_r / r:.1f} x closer")
        assert 5 * t <= plain_t and r < plain_r, (loss, t, plain_t, r, plain_r)


def test_every_robust_loss_ends_closer_to_the_truth_on_the_contaminated_ring():
    plain_t, plain_r = C.ring_errors(C.ring_solved("none"))
    for loss, _ in C.ROBUST:
        t, r = C.ring_errors(C.ring_solved(loss))
        print(f"ring {loss}: translation {plain_t / t:.1f} x closer, rotation {plain_r / r:.1f} x closer")
        assert 3 * t <= plain_t and r < plain_r, (loss, t, plain_t, r, plain_r)
