"""Yardstick and inputs of the robust point-to-plane calls (rap_icp_plane_robust, rap_icp_plane_grid_robust, rap_scene_refine_robust):
the comment of include/rapflow.h restated in fp64 numpy -- the weight and the cost of robust_loss.h, the pairwise call on
icp_plane_oracle.icp_plane's statements, the scene call on scene_refine_oracle.refine's -- each with an `f32` mode (moved points formed in
fp32 from the fp32-rounded pose: what the device's search and residuals see).  With loss none both reduce to those two yardsticks
statement by statement (tests/test_robust_host.py asserts equality).

Not a copy of any program: written from the header (iteratively reweighted least squares, Holland and Welsch 1977; Huber 1964; the
Cauchy and Tukey biweight functions as in Zhang 1997, "Parameter estimation techniques: a tutorial").

The contamination recipe, so that anyone can regenerate the inputs:
  pair (seed, nx, ny)   rows 0, 5, 10, ... of X get z += U(0.08, 0.2), drawn from default_rng(1000 + seed)
  scene                 in view order, rows s, s+5, ... of each view (s its first row) move along their own normal by U(0.08, 0.2), all
                        drawn from one default_rng(77)"""
import functools

import numpy as np

import icp_oracle as O
import icp_plane_oracle as PO
import scene_refine_oracle as SO

LOSSES = ("none", "huber", "cauchy", "tukey")
CODES = {"none": 0, "huber": 1, "cauchy": 2, "tukey": 3}      # RAP_LOSS_*
ROBUST = (("huber", 0.01), ("cauchy", 0.01), ("tukey", 0.03))      # the (loss, scale) of every case
SCALE = dict(ROBUST)
THR = PO.BATCH_THR                                 # relative_rmse_thr of the cases (icp_plane_oracle.BATCH_THR, for the reason given there)
MARGIN = 1e-5                                      # neighbour, gate and relative-decrease margins of the cases that are compared exactly
GATE = SO.GATE                                     # of the ring

# THE fp32 BOUNDS of the GPU tests (tests/test_robust_host.py measures them from this yardstick alone and asserts the relations).
# Poses, rmse and edge_rmse: the larger of 2e-6 (the floor of the plane-ICP and scene tests) and 3 x the largest distance between the fp64
# run and the f32=True run over the GPU parity cases.  Measured: see FP32_MEASURED; 3 x that is below the floor, so the floor holds.
# Weights: a weight moves by |dw/dr| |dr| with |dr| the rounding of a residual (about 1e-8 here); |dw/dr| <= 1/k for Huber beyond k,
# 0.65/k for Cauchy and 1.2/k for Tukey, so with k = 0.01 .. 0.03 the same rounding is worth about 1e-6 / 3 in a weight.  The bound is
# derived the same way: the larger of 2e-6 and 3 x the measured largest distance of the weights (the fp32 rounding of a weight on its
# way out, 6e-8, is inside either).  Measured: see WEIGHT_MEASURED; 3 x that is 1.65e-6, so the floor holds here too.
# Not tuned against the kernel.
FP32_MEASURED = 1.1e-7                             # poses / rmse: <= 1.9e-8 on the pairs and the batch, <= 1.1e-7 on the ring
FP32_BOUND = max(3 * FP32_MEASURED, 2e-6)
WEIGHT_MEASURED = 5.5e-7                           # weights: 4.5e-7 on the exact pair (Tukey), 5.5e-7 in the batch (its 513-row problem)
WEIGHT_BOUND = max(3 * WEIGHT_MEASURED, 2e-6)


def weight_cost(loss, r, k):
    """-> (w, rho) of the residuals r (fp64 array) under `loss` at scale k: the table of include/rapflow.h"""
    r = np.asarray(r, np.float64)
    a = np.abs(r)
    if loss == "none":
        return np.ones_like(r), 0.5 * r * r
    k = float(k)
    if loss == "huber":
        inside = a <= k
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.where(inside, 1.0, k / np.where(inside, 1.0, a))
        return w, np.where(inside, 0.5 * r * r, k * (a - 0.5 * k))
    u2 = (r / k) ** 2
    if loss == "cauchy":
        return 1.0 / (1.0 + u2), 0.5 * k * k * np.log1p(u2)
    if loss == "tukey":
        inside = a <= k
        t = np.where(inside, 1.0 - u2, 0.0)
        return t * t, np.where(inside, k * k / 6.0 * (1.0 - t ** 3), k * k / 6.0)
    raise ValueError(loss)


def _scale(loss, k):
    return None if loss == "none" else float(np.float32(k))      # the call takes the scale as a float


def icp_plane(X, Y, Yn, loss="none", loss_scale=None, init=None, max_iterations=100, relative_rmse_thr=1e-6,
              max_correspondence_distance=None, f32=False, margins=True):
    """one problem -> icp_plane_oracle.icp_plane's Result plus weights (nx,) fp64 (of the last iteration that ran; zeros if none did),
    wsum (W of that iteration) and rel_margin (the smallest |rel - relative_rmse_thr| the stopping rule saw): rap_icp_plane_robust"""
    k = _scale(loss, loss_scale)
    X32, Y32 = np.asarray(X, np.float32), np.asarray(Y, np.float32)
    X, Y, Yn = X32.astype(np.float64), Y32.astype(np.float64), np.asarray(Yn, np.float32).astype(np.float64)
    R = np.eye(3) if init is None else np.asarray(init[0], np.float32).astype(np.float64)
    T = np.zeros(3) if init is None else np.asarray(init[1], np.float32).astype(np.float64)

    def moved(R, T):
        if f32:
            return X32 @ R.astype(np.float32) + T.astype(np.float32)
        return X @ R + T
    out = O.Result(R=R, T=T, rmse=np.nan, iterations=0, converged=False, Xt=moved(R, T), nn_margin=np.inf, gate_margin=np.inf, count=0,
                   cond=np.inf, rels=[], weights=np.zeros(X.shape[0]), wsum=0.0, rel_margin=np.inf)
    if X.shape[0] == 0 or Y.shape[0] == 0:
        return out
    ok = PO.usable(Yn)
    prev = None
    for it in range(max_iterations):
        P = moved(out.R, out.T)
        nn, d1, d2 = O.nearest(P, Y32 if f32 else Y, margins)
        dist = np.sqrt(d1)
        out.nn_margin = min(out.nn_margin, float((np.sqrt(d2) - dist).min()))
        S = ok[nn]
        if max_correspondence_distance is not None:
            S = S & (dist <= max_correspondence_distance)
            out.gate_margin = min(out.gate_margin, float(np.abs(dist.astype(np.float64) - max_correspondence_distance).min()))
        out.count = int(S.sum())
        out.weights = np.zeros(X.shape[0])
        if out.count == 0:
            out.rmse, out.converged, out.wsum = np.inf, False, 0.0
            return out
        p, y, n = P[S].astype(np.float64), Y[nn[S]], Yn[nn[S]]
        r = ((p - y) * n).sum(axis=1)
        J = np.concatenate([np.cross(p, n), n], axis=1)
        if loss == "none":
            w = np.ones_like(r)
            A, b, e = J.T @ J, J.T @ r, (r * r).sum()
        else:
            w, rho = weight_cost(loss, r, k)
            Jw = J * w[:, None]
            A, b, e = Jw.T @ J, Jw.T @ r, (2.0 * rho).sum()
        out.weights[S] = w
        out.wsum = float(w.sum())
        if out.wsum == 0.0:
            out.rmse, out.converged = np.inf, False
            return out
        lam = np.linalg.eigvalsh(A)
        out.cond = min(out.cond, float(lam[0] / lam[-1]))
        out.rmse = float(np.sqrt(e / out.count))
        xi = -np.linalg.pinv(A, rcond=PO.RCOND, hermitian=True) @ b
        dR = PO.rodrigues(xi[:3])
        out.R, out.T = out.R @ dR.T, out.T @ dR.T + xi[3:]
        out.Xt = moved(out.R, out.T)
        out.iterations = it + 1
        if prev is not None and prev == 0.0:
            out.converged = True
            return out
        rel = 1.0 if prev is None else (prev - out.rmse) / prev
        out.rels.append(rel)
        out.rel_margin = min(out.rel_margin, abs(rel - relative_rmse_thr))
        if rel <= relative_rmse_thr:
            out.converged = True
            return out
        prev = out.rmse
    return out


def refine(P, N, view_seg, scene_seg, edges, loss="none", loss_scale=None, fixed=None, init_R=None, init_T=None, max_iterations=30,
           relative_rmse_thr=1e-6, max_correspondence_distance=None, max_views=16, row_budget=None, f32=False, margins=True):
    """-> scene_refine_oracle.refine's Result plus wsum (S,) (W of the last iteration the scene ran): rap_scene_refine_robust"""
    k = _scale(loss, loss_scale)
    P32, N32 = np.asarray(P, np.float32).reshape(-1, 3), np.asarray(N, np.float32).reshape(-1, 3)
    P64, N64 = P32.astype(np.float64), N32.astype(np.float64)
    views = SO.clamp_seg(view_seg, P32.shape[0])
    V = views.shape[0]
    scenes = SO.clamp_seg(scene_seg, V)
    S = scenes.shape[0]
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    E = edges.shape[0]
    R = np.tile(np.eye(3), (V, 1, 1)) if init_R is None else np.asarray(init_R, np.float32).astype(np.float64).reshape(V, 3, 3).copy()
    T = np.zeros((V, 3)) if init_T is None else np.asarray(init_T, np.float32).astype(np.float64).reshape(V, 3).copy()
    scene_of = np.full(V, -1)
    fix = np.zeros(V, bool) if fixed is None else np.asarray(fixed).reshape(V) != 0
    left_out = scenes[:, 1] > max_views
    for s, (f, c) in enumerate(scenes):
        if left_out[s]:
            continue
        scene_of[f:f + c] = s
        if fixed is None and c > 0:
            fix[f] = True
    budget = np.inf if row_budget is None else row_budget
    live, rows = np.zeros(E, bool), 0
    for e, (a, b) in enumerate(edges):
        if not (0 <= a < V and 0 <= b < V) or a == b or scene_of[a] < 0 or scene_of[a] != scene_of[b]:
            continue
        if views[a, 1] == 0 or views[b, 1] == 0 or rows + views[a, 1] > budget:
            continue
        live[e] = True
        rows += views[a, 1]
    out = O.Result(R=R, T=T, rmse=np.full(S, np.nan), iterations=np.zeros(S, np.int64), converged=np.zeros(S, bool),
                   edge_rmse=np.full(E, np.nan), edge_count=np.zeros(E, np.int64), live=live, nn_margin=np.inf, gate_margin=np.inf,
                   rel_margin=np.inf, rels=[[] for _ in range(S)], wsum=np.zeros(S))
    ok = PO.usable(N64)
    gate = max_correspondence_distance
    for s, (first, count) in enumerate(scenes):
        if left_out[s]:
            continue
        mine = [e for e in range(E) if live[e] and scene_of[edges[e, 0]] == s]
        free = [v for v in range(first, first + count) if not fix[v]]
        slot = {v: i for i, v in enumerate(free)}
        prev = None
        for it in range(max_iterations):
            H, g = np.zeros((6 * len(free), 6 * len(free))), np.zeros(6 * len(free))
            tot_e, tot_n, tot_w = 0.0, 0, 0.0
            for e in mine:
                a, b = edges[e]
                (xs, xn), (ys, yn) = views[a], views[b]
                Re, Te = R[a] @ R[b].T, (T[a] - T[b]) @ R[b].T
                if f32:
                    q = P32[xs:xs + xn] @ Re.astype(np.float32) + Te.astype(np.float32)
                    Y = P32[ys:ys + yn]
                else:
                    q = P64[xs:xs + xn] @ Re + Te
                    Y = P64[ys:ys + yn]
                nn, d1, d2 = O.nearest(q, Y, margins)
                dist = np.sqrt(d1)
                if margins:
                    out.nn_margin = min(out.nn_margin, float((np.sqrt(d2) - dist).min()))
                sel = ok[ys + nn]
                if gate is not None:
                    sel = sel & (dist <= gate)
                    out.gate_margin = min(out.gate_margin, float(np.abs(dist.astype(np.float64) - gate).min()))
                q64, y, n = q[sel].astype(np.float64), P64[ys + nn[sel]], N64[ys + nn[sel]]
                r = ((q64 - y) * n).sum(axis=1)
                pw, nw = q64 @ R[b] + T[b], n @ R[b]
                J = np.concatenate([np.cross(pw, nw), nw], axis=1)
                if loss == "none":
                    w = np.ones_like(r)
                    Aw, gw, ee = J.T @ J, J.T @ r, (r * r).sum()
                else:
                    w, rho = weight_cost(loss, r, k)
                    Jw = J * w[:, None]
                    Aw, gw, ee = Jw.T @ J, Jw.T @ r, (2.0 * rho).sum()
                out.edge_count[e] = int(sel.sum())
                out.edge_rmse[e] = np.sqrt(ee / sel.sum()) if sel.any() else np.nan
                tot_e += float(ee)
                tot_n += int(sel.sum())
                tot_w += float(w.sum())
                ia, ib = slot.get(a), slot.get(b)
                if ia is not None:
                    H[6 * ia:6 * ia + 6, 6 * ia:6 * ia + 6] += Aw
                    g[6 * ia:6 * ia + 6] += gw
                if ib is not None:
                    H[6 * ib:6 * ib + 6, 6 * ib:6 * ib + 6] += Aw
                    g[6 * ib:6 * ib + 6] -= gw
                if ia is not None and ib is not None:
                    H[6 * ia:6 * ia + 6, 6 * ib:6 * ib + 6] -= Aw
                    H[6 * ib:6 * ib + 6, 6 * ia:6 * ia + 6] -= Aw
            out.wsum[s] = tot_w
            if tot_n == 0 or tot_w == 0.0:
                out.rmse[s], out.converged[s] = np.inf, False
                break
            out.rmse[s] = np.sqrt(tot_e / tot_n)
            if free:
                xi = -np.linalg.pinv(H, rcond=SO.RCOND, hermitian=True) @ g
                for v, i in slot.items():
                    dR = PO.rodrigues(xi[6 * i:6 * i + 3])
                    R[v], T[v] = R[v] @ dR.T, T[v] @ dR.T + xi[6 * i + 3:6 * i + 6]
            out.iterations[s] = it + 1
            if prev is not None and prev == 0.0:
                out.converged[s] = True
                break
            rel = 1.0 if prev is None else (prev - out.rmse[s]) / prev
            out.rels[s].append(rel)
            out.rel_margin = min(out.rel_margin, abs(rel - relative_rmse_thr))
            if rel <= relative_rmse_thr:
                out.converged[s] = True
                break
            prev = out.rmse[s]
    return out


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
EXACT_PAIR = (3, 257, 256)                          # margins >= MARGIN for all four losses (tests/test_robust_host.py asserts it)
PROPERTY_PAIRS = ((3, 257, 256), (1, 300, 513), (3, 1000, 1000))
LIFT = (0.08, 0.2)


@functools.lru_cache(maxsize=None)
def contaminated_pair(seed, nx, ny):
    """icp_plane_oracle.make_pair_with_normals(seed, nx, ny) with every fifth row of X lifted off the surface -> X, Y, Yn fp32"""
    X, Y, Yn = PO.make_pair_with_normals(seed, nx, ny)
    X = X.copy()
    rows = np.arange(0, nx, 5)
    X[rows, 2] += np.random.default_rng(1000 + seed).uniform(LIFT[0], LIFT[1], rows.size).astype(np.float32)
    return X, Y, Yn


@functools.lru_cache(maxsize=None)
def clean_pair(seed, nx, ny):
    return PO.make_pair_with_normals(seed, nx, ny)


@functools.lru_cache(maxsize=None)
def pair_solved(seed, nx, ny, loss, f32=False, margins=False, thr=THR, contaminated=True):
    X, Y, Yn = (contaminated_pair if contaminated else clean_pair)(seed, nx, ny)
    return icp_plane(X, Y, Yn, loss, SCALE.get(loss), relative_rmse_thr=thr, f32=f32, margins=margins)


PAIR_GATE = 0.1                                    # on the exact pair under Tukey: some rows gated out, some inside with weight zero


@functools.lru_cache(maxsize=None)
def gated_solved(f32=False, margins=False):
    X, Y, Yn = contaminated_pair(*EXACT_PAIR)
    return icp_plane(X, Y, Yn, "tukey", SCALE["tukey"], relative_rmse_thr=THR, max_correspondence_distance=PAIR_GATE, f32=f32, margins=margins)


def pair_errors(res):
    """-> (translation error, rotation error) of a pairwise result against the pose the pair was made with (icp_oracle.R0, T0)"""
    return float(np.linalg.norm(res.T - np.asarray(O.T0))), float(np.linalg.norm(res.R - O.R0))


def contaminate_scene(sc):
    """a copy of a scene_refine_oracle scene with every fifth row of every view moved along its own normal"""
    rng = np.random.default_rng(77)
    P = sc["P"].copy()
    for s, n in sc["seg"]:
        rows = np.arange(s, s + n, 5)
        P[rows] += (rng.uniform(LIFT[0], LIFT[1], rows.size)[:, None] * sc["N"][rows].astype(np.float64)).astype(np.float32)
    out = dict(sc)
    out["P"] = P
    return out


@functools.lru_cache(maxsize=None)
def contaminated_ring():
    return contaminate_scene(SO.ring_scene())


@functools.lru_cache(maxsize=None)
def ring_solved(loss, f32=False, contaminated=True):
    sc = contaminated_ring() if contaminated else SO.ring_scene()
    return refine(sc["P"], sc["N"], sc["seg"], [(0, SO.RING_V)], SO.ring_edges(), loss, SCALE.get(loss), None, sc["R0"], sc["T0"],
                  relative_rmse_thr=THR, max_correspondence_distance=GATE, f32=f32, margins=False)


def ring_errors(res):
    """-> (translation error, rotation error) of the ring's poses against the true ones, after removing the common motion"""
    sc = SO.ring_scene()
    R, T = SO.remove_common_motion(res.R, res.T, sc["R_true"], sc["T_true"], range(SO.RING_V))
    return float(np.abs(T - sc["T_true"]).max()), float(np.abs(R - sc["R_true"]).max())


def pair_deviation(a, b):
    """largest distance between two pairwise results on R, T and rmse; and on the weights"""
    return max(np.abs(a.R - b.R).max(), np.abs(a.T - b.T).max(), abs(a.rmse - b.rmse)), float(np.abs(a.weights - b.weights).max())


# ---- the packed batch of the GPU tests: item and tile edges, an empty problem, a problem whose every weight is zero ----
BATCH_LENGTHS = (1, 2, 3, 255, 256, 257, 513)
BATCH_LOSS, BATCH_SCALE = "tukey", 0.03
FAR_LIFT = 0.25                                    # of the all-zero-weight problem: every residual is several Tukey scales


@functools.lru_cache(maxsize=None)
def batch():
    """-> dict(X, Y, Yn fp32 packed, x_seg, y_seg (K,2) int32, parts: per problem (X, Y, Yn) or None for the empty one, far: the
    number of the problem whose every residual exceeds the scale, covered (NX,) bool, init_R (K,3,3), init_T (K,3) fp32).  Problem i < 7
    takes the first BATCH_LENGTHS[i] rows of contaminated_pair(20 + i, 513, 256)'s X against its whole Y; then the empty problem; then
    a clean source lifted by FAR_LIFT along z.  Junk rows lie between the segments, and the segments are out of order."""
    rng = np.random.default_rng(404)
    junk = lambda n: rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    parts = []
    for i, n in enumerate(BATCH_LENGTHS):
        X, Y, Yn = contaminated_pair(20 + i, 513, 256)
        parts.append((X[:n].copy(), Y, Yn))
    parts.append(None)
    Xf, Yf, Nf = clean_pair(31, 200, 256)
    Xf = (Xf.astype(np.float64) @ O.R0 + np.asarray(O.T0)).astype(np.float32)      # at the target's pose ...
    Xf = Xf + (FAR_LIFT * np.asarray([0, 0, 1.0]) @ O.R0).astype(np.float32)      # ... and lifted off the surface along its z
    parts.append((Xf, Yf, Nf))
    far = len(parts) - 1
    K = len(parts)
    order = rng.permutation(K)
    xr, yr, nr, x_seg, y_seg, ax, ay = [], [], [], np.zeros((K, 2), np.int32), np.zeros((K, 2), np.int32), 0, 0
    for k in order:
        jx, jy = junk(int(rng.integers(1, 5))), junk(int(rng.integers(1, 5)))
        xr.append(jx)
        yr.append(jy)
        nr.append(junk(jy.shape[0]))
        ax += jx.shape[0]
        ay += jy.shape[0]
        if parts[k] is None:
            x_seg[k], y_seg[k] = (ax, 0), (ay, 0)
            continue
        X, Y, Yn = parts[k]
        x_seg[k], y_seg[k] = (ax, X.shape[0]), (ay, Y.shape[0])
        xr.append(X)
        yr.append(Y)
        nr.append(Yn)
        ax += X.shape[0]
        ay += Y.shape[0]
    xr.append(junk(3))
    yr.append(junk(2))
    nr.append(junk(2))
    Xp = np.concatenate(xr)
    covered = np.zeros(Xp.shape[0], bool)
    for a, n in x_seg:
        covered[a:a + n] = True
    init_R = np.tile(np.eye(3, dtype=np.float32), (K, 1, 1))
    init_T = np.zeros((K, 3), np.float32)
    init_R[far] = O.rotation((0.3, -0.2, 0.9), 0.5).astype(np.float32)
    init_T[far] = (0.001, -0.002, 0.0015)
    return dict(X=Xp, Y=np.concatenate(yr), Yn=np.concatenate(nr), x_seg=x_seg, y_seg=y_seg, parts=parts, far=far,
                covered=covered, init_R=init_R, init_T=init_T)


@functools.lru_cache(maxsize=None)
def batch_solved(f32=False):
    b = batch()
    return [None if p is None else icp_plane(p[0], p[1], p[2], BATCH_LOSS, BATCH_SCALE, init=(b["init_R"][k], b["init_T"][k]),
                                             relative_rmse_thr=THR, f32=f32, margins=False) for k, p in enumerate(b["parts"])]


# ---- two scenes in one call: the contaminated ring, and a two-view scene whose every weight is zero ----
@functools.lru_cache(maxsize=None)
def far_scene():
    """two views of one surface patch in the same frame, the second lifted by FAR_LIFT along the surface's z: every residual of both
    edges is several Tukey scales"""
    X, Y, Yn = clean_pair(31, 200, 256)
    Yl = Y.astype(np.float64) @ O.R0.T - np.asarray(O.T0) @ O.R0.T             # the target back in the surface's frame
    Nl = Yn.astype(np.float64) @ O.R0.T
    A = X.astype(np.float32)
    B = (Yl + (0, 0, FAR_LIFT)).astype(np.float32)
    return dict(P=np.concatenate([A, B]), N=np.concatenate([PO.surf_normals(X.astype(np.float64)).astype(np.float32), Nl.astype(np.float32)]),
                seg=np.asarray([(0, A.shape[0]), (A.shape[0], B.shape[0])], np.int32))
