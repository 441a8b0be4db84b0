"""Yardstick of the point-to-plane ICP (rap_amd/csrc/icp_plane.hip) and of the normal estimation (rap_amd/csrc/normals.hip): the two
algorithms of include/rapflow.h restated in fp64 numpy, on the inputs of tests/icp_oracle.py.  `f32=True` runs the plane ICP with the
moved points formed in fp32 from the fp32 rounding of the pose -- what the device's search and residuals see -- and everything else in
fp64 as the device does it.

Not a copy of any program: written from the algorithm as the header states it (Gauss-Newton on the point-to-plane residual, Chen and
Medioni 1992; the plane fit of a neighbourhood's covariance, Hoppe et al. 1992)."""
import functools

import numpy as np

import icp_oracle as O

RCOND = 1e-12


def surf_normals(P):
    """unit normals (+z side) of icp_oracle.surf at its points P (n,3), fp64"""
    x, y = P[:, 0], P[:, 1]
    fx = 0.75 * np.cos(5 * x) * np.cos(4 * y) + 0.2 * x
    fy = -0.6 * np.sin(5 * x) * np.sin(4 * y)
    n = np.stack([-fx, -fy, np.ones_like(x)], axis=1)
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def make_pair_with_normals(seed, nx, ny, x_range=None, y_range=None):
    """icp_oracle.make_pair's X, Y (the same draws) and the analytic normals of Y: those of the surface, moved by R0.  All fp32."""
    rng = np.random.default_rng(seed)
    X = O.surf(rng, nx, x_range)
    Yl = O.surf(rng, ny, y_range)
    Y = (Yl @ O.R0 + np.asarray(O.T0)).astype(np.float32)
    return X.astype(np.float32), Y, (surf_normals(Yl) @ O.R0).astype(np.float32)


def rodrigues(w):
    """exp([w]x), column-vector convention"""
    th = float(np.linalg.norm(w))
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)
    if th < 1e-4:
        a, b = 1.0 - th * th / 6.0, 0.5 - th * th / 24.0
    else:
        a, b = np.sin(th) / th, 2.0 * np.sin(0.5 * th) ** 2 / (th * th)
    return np.eye(3) + a * K + b * (K @ K)


def usable(N):
    return np.isfinite(N).all(axis=1) & (N != 0).any(axis=1)


def icp_plane(X, Y, Yn, init=None, max_iterations=100, relative_rmse_thr=1e-6, max_correspondence_distance=None, f32=False, margins=True):
    """one problem -> Result(R, T, rmse, iterations, converged, Xt, nn_margin, gate_margin, count, cond, rels): rap_icp_plane of
    include/rapflow.h.  count: the pairs of the last iteration; cond: the smallest lambda_min / lambda_max of A over the iterations;
    rels: the relative decrease of the rmse that the stopping rule saw at every iteration (1.0 at the first)."""
    X32, Y32 = np.asarray(X, np.float32), np.asarray(Y, np.float32)
    X, Y, Yn = X32.astype(np.float64), Y32.astype(np.float64), np.asarray(Yn, np.float32).astype(np.float64)
    R = np.eye(3) if init is None else np.asarray(init[0], np.float32).astype(np.float64)
    T = np.zeros(3) if init is None else np.asarray(init[1], np.float32).astype(np.float64)

    def moved(R, T):
        if f32:
            return X32 @ R.astype(np.float32) + T.astype(np.float32)
        return X @ R + T
    out = O.Result(R=R, T=T, rmse=np.nan, iterations=0, converged=False, Xt=moved(R, T), nn_margin=np.inf, gate_margin=np.inf, count=0,
                   cond=np.inf, rels=[])
    if X.shape[0] == 0 or Y.shape[0] == 0:
        return out
    ok = usable(Yn)
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
        if out.count == 0:
            out.rmse, out.converged = np.inf, False
            return out
        p, y, n = P[S].astype(np.float64), Y[nn[S]], Yn[nn[S]]
        r = ((p - y) * n).sum(axis=1)
        J = np.concatenate([np.cross(p, n), n], axis=1)
        A, b = J.T @ J, J.T @ r
        lam = np.linalg.eigvalsh(A)
        out.cond = min(out.cond, float(lam[0] / lam[-1]))
        out.rmse = float(np.sqrt((r * r).sum() / out.count))
        xi = -np.linalg.pinv(A, rcond=RCOND, hermitian=True) @ b
        dR = rodrigues(xi[:3])
        out.R, out.T = out.R @ dR.T, out.T @ dR.T + xi[3:]
        out.Xt = moved(out.R, out.T)
        out.iterations = it + 1
        if prev is not None and prev == 0.0:
            out.converged = True
            return out
        rel = 1.0 if prev is None else (prev - out.rmse) / prev
        out.rels.append(rel)
        if rel <= relative_rmse_thr:
            out.converged = True
            return out
        prev = out.rmse
    return out


def estimate_normals(P, max_nn=20, radius=0.5, viewpoint=None):
    """one segment -> (normals (n,3) fp64, eigenvalues (n,3) fp64 ascending, counts (n,), gap (n,)): rap_estimate_normals of
    include/rapflow.h.  gap: how far the row is from another neighbour set -- the distance between the last neighbour taken and the
    first one left out, and with a radius also the smallest | distance - radius | over the max_nn nearest rows; inf where nothing could flip.
    Distances in fp32 direct differences, as the device forms them."""
    P32 = np.asarray(P, np.float32)
    n = P32.shape[0]
    normals, eig = np.zeros((n, 3)), np.zeros((n, 3))
    counts, gap = np.zeros(n, np.int64), np.full(n, np.inf)
    fin = np.isfinite(P32).all(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(n):
            d = P32[i] - P32
            d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
            dist = np.sqrt(d2)
            cand = fin & np.isfinite(d2)
            if radius > 0:
                inside = cand & (dist <= np.float32(radius))
            else:
                inside = cand
            order = np.lexsort((np.arange(n), d2))                     # by (d2, j)
            nearest = order[cand[order]][:max_nn]                      # the radius aside
            order = order[inside[order]]
            take = order[:max_nn]
            counts[i] = take.size
            if order.size > max_nn:
                gap[i] = float(dist[order[max_nn]]) - float(dist[take[-1]])
            if radius > 0 and nearest.size:                            # only a flip among the max_nn nearest changes the set
                gap[i] = min(gap[i], float(np.abs(dist[nearest].astype(np.float64) - radius).min()))
            if take.size < 3:
                continue
            Q = P32[take].astype(np.float64)
            c = Q - Q.mean(axis=0)
            w, v = np.linalg.eigh(c.T @ c / take.size)
            nv = v[:, 0]
            if viewpoint is not None:
                if nv @ (np.asarray(viewpoint, np.float64) - P32[i].astype(np.float64)) < 0:
                    nv = -nv
            elif nv[np.argmax(np.abs(nv))] < 0:                         # argmax: the first among equals
                nv = -nv
            normals[i], eig[i] = nv, w
    return normals, eig, counts, gap


# ---------------------------------------------------------------------------------------------
# the inputs the host and the GPU tests share
# ---------------------------------------------------------------------------------------------
PLANE_PAIRS = O.EXACT_COUNT                         # (seed, nx, ny): margin-checked in tests/test_icp_plane_host.py
# ... and with normals estimated from Y (20 neighbours, no radius), where the neighbour sets of the estimate must keep a margin too: seed 3
# does not (one row of its Y has its 20th and 21st neighbour 1.2e-7 apart), seed 10 does
ESTIMATED_PAIRS = [(1, 256, 256), (10, 256, 256)]
GATE_CASE = dict(seed=3, nx=256, ny=256, x_range=(-0.5, 0.2), y_range=(-0.2, 0.5))
GATE = 0.05
NORMALS_CASE = dict(seed=3, n=256, max_nn=12, radius=0.5)
VIEWPOINT = (0.1, -0.2, 3.0)                        # far above the surface: n . (v - p) is nowhere near 0


@functools.lru_cache(maxsize=None)
def pair(seed, nx, ny, x_range=None, y_range=None):
    return make_pair_with_normals(seed, nx, ny, x_range, y_range)


@functools.lru_cache(maxsize=None)
def solved(seed, nx, ny, x_range=None, y_range=None, gate=None, max_iterations=100, f32=False, margins=False, estimated=False):
    X, Y, Yn = pair(seed, nx, ny, x_range, y_range)
    if estimated:
        Yn = estimate_normals(Y, 20, 0.0)[0].astype(np.float32)
    return icp_plane(X, Y, Yn, max_iterations=max_iterations, max_correspondence_distance=gate, f32=f32, margins=margins)


@functools.lru_cache(maxsize=None)
def normals_input(seed, n):
    return O.surf(np.random.default_rng(seed), n).astype(np.float32)


@functools.lru_cache(maxsize=None)
def normals_solved(seed, n, max_nn, radius, viewpoint=None):
    return estimate_normals(normals_input(seed, n), max_nn, radius, viewpoint)


@functools.lru_cache(maxsize=None)
def coplanar_case(seed=9):
    """-> X (200,3), Y (300,3), Yn: a flat target (z = 0, every normal +z) and a flat source tilted by 2 degrees about an in-plane axis
    and lifted by 0.01.  Only the tilt and the lift are observable: rotation about z and translation in the plane are not."""
    rng = np.random.default_rng(seed)
    Y = np.concatenate([rng.uniform(-0.5, 0.5, (300, 2)), np.zeros((300, 1))], axis=1)
    X = np.concatenate([rng.uniform(-0.4, 0.4, (200, 2)), np.zeros((200, 1))], axis=1) @ O.rotation((1.0, 0.5, 0.0), 2.0) + (0, 0, 0.01)
    return X.astype(np.float32), Y.astype(np.float32), np.tile(np.asarray([[0, 0, 1]], np.float32), (300, 1))


# the edge sweep of the normals kernel: segment lengths around the 256-row tile, on jittered lattices whose seed was chosen so that no
# neighbour set is within SWEEP_GAP (in distance; the points are ~0.5 apart) of another one -- tests/test_normals_host.py asserts it
SWEEP_LENGTHS = (1, 2, 3, 255, 256, 257, 513)
SWEEP_MAX_NN = (3, 12, 32)
SWEEP_GAP = 1e-5
SWEEP_SEED = 0
SWEEP_SPACING = 0.5
SWEEP_RADIUS = 0.475


@functools.lru_cache(maxsize=None)
def sweep_lattice(n):
    return jittered_lattice(SWEEP_SEED, n, spacing=SWEEP_SPACING)


def jittered_lattice(seed, n, spacing=0.1, jitter=0.3):
    """n points of a jittered 3-d lattice in a random order: neighbour distances differ by a fair fraction of the spacing"""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(n ** (1.0 / 3.0)))
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    g = (g + rng.uniform(-jitter, jitter, g.shape)) * spacing
    return g[rng.permutation(g.shape[0])[:n]].astype(np.float32)


# ---------------------------------------------------------------------------------------------
# table scale: the batches of icp_oracle.batch300 / big_batch with normals, and K = 300 segments for the normal estimation
# ---------------------------------------------------------------------------------------------
def unit_normals(seed, n):
    """caller-supplied normals of a cloud without a surface (a lattice): seeded unit vectors, fp32.  With exact correspondences the residual
    (p - y) . n vanishes at the true pose whatever n is, and random directions keep the 6 x 6 system well conditioned."""
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def batch300_normals():
    """-> Yn (NY,3) fp32 aligned with icp_oracle.batch300()["Y"], and per problem the normals of its y segment: the analytic ones for a
    surface pair, unit_normals for a lattice; junk rows keep junk."""
    b = O.batch300(True)
    Yn = np.random.default_rng(301).uniform(-1, 1, b["Y"].shape).astype(np.float32)
    per = [None] * O.BATCH_K
    for k in range(O.BATCH_K):
        a, n = (int(v) for v in b["y_seg"][k])
        if n == 0:
            continue
        per[k] = pair(*O.BATCH_PLANE_SURFACES[k])[2] if b["kinds"][k] == "surface" else unit_normals(7000 + O.BATCH_SHARED_Y.get(k, k), n)
        Yn[a:a + n] = per[k]
    return Yn, per


# THE STOPPING RULE UNDER ROUNDING.  The device forms the moved points in fp32, which moves the point-to-plane rmse of a 50-point problem by
# up to about 1e-6 of itself from one iteration to the next even when the pose has settled (the yardstick's own fp32 run shows the same:
# tests/test_icp_plane_host.py measures it), and the third Gauss-Newton step of these small problems typically still gains 1e-6 .. 1e-5.
# At the default relative_rmse_thr of 1e-6 the last decision of such a problem is therefore a matter of rounding.  The batch (and the big
# problem with its two small neighbours) runs at BATCH_THR = 1e-3, where the sequence of relative decreases has a gap, and its inputs
# (icp_oracle.BATCH_PLANE_STEPS, BATCH_PLANE_SURFACES) are chosen so that a problem's iteration count is DECIDED: every relative decrease
# the yardstick saw, in its fp64 and in its fp32 run, is a factor of 10 away from that threshold, and a residual of more than 1e-6 is left.
BATCH_THR = 1e-3


@functools.lru_cache(maxsize=None)
def batch300_solved(init=False, f32=False):
    b, (_, per) = O.batch300(True), batch300_normals()
    return [None if p is None else icp_plane(p[0], p[1], per[k], init=(b["init_R"][k], b["init_T"][k]) if init else None, f32=f32, margins=not f32,
                                             relative_rmse_thr=BATCH_THR)
            for k, p in enumerate(b["parts"])]


def decided(ref, f32):
    """no rounding decides the iteration count of this problem (see BATCH_THR): ref, f32 its yardstick with fp64 and fp32 moved points"""
    clear = lambda r: all(v >= 10 * BATCH_THR or v <= BATCH_THR / 10 for v in r.rels)
    return ref.rmse > 1e-6 and clear(ref) and clear(f32) and f32.iterations == ref.iterations


def batch300_decided(init=False):
    """the problems of the batch whose point-to-plane iteration count is decided"""
    ref, f32 = batch300_solved(init), batch300_solved(init, f32=True)
    return [k for k in range(O.BATCH_K) if ref[k] is not None and decided(ref[k], f32[k])]


@functools.lru_cache(maxsize=None)
def big_normals(nx):
    X, Y, x_seg, y_seg, parts = O.big_batch(nx, True)
    per = [unit_normals(7100 + i, p[1].shape[0]) for i, p in enumerate(parts)]
    Yn = np.zeros_like(Y)
    for k in range(3):
        Yn[y_seg[k][0]:y_seg[k][0] + y_seg[k][1]] = per[k]
    return Yn, per


@functools.lru_cache(maxsize=None)
def big_solved(nx, f32=False):
    per = big_normals(nx)[1]
    return [icp_plane(x, y, per[k], f32=f32, margins=not f32, relative_rmse_thr=BATCH_THR) for k, (x, y) in enumerate(O.big_batch(nx, True)[4])]


NORMALS_K = 300
NORMALS_LENGTHS = (3, 5, 12, 40, 255, 257)
NORMALS_MAX_NN = (3, 12)
NORMALS_EMPTY, NORMALS_ONE, NORMALS_TWO = (7, 260, 290), (20, 270), (33, 280)
NORMALS_REPEATS = {264: 100, 296: 258}       # segment number -> the earlier segment it repeats exactly (one below 256, one above)


NORMALS_VIEW_CLEAR = 1e-3


@functools.lru_cache(maxsize=None)
def _sweep_normals(n, max_nn):
    return estimate_normals(sweep_lattice(n), max_nn, 0.0)[0]


def _view_clear(normals, cloud, viewpoint):
    toward = np.asarray(viewpoint, np.float64) - cloud.astype(np.float64)
    est = normals.any(axis=1)
    return bool((np.abs((normals * toward).sum(axis=1)) >= NORMALS_VIEW_CLEAR * np.linalg.norm(toward, axis=1))[est].all())


@functools.lru_cache(maxsize=None)
def normals_batch300():
    """-> dict(P (N,3) fp32, seg (K,2) int32, clouds (per segment, None for an empty one), viewpoint (K,3) fp32, covered (N,) bool):
    K = 300 segments in a shuffled order with junk rows between them.  Segment k holds the rows of sweep_lattice(n) in an order of its
    own (the same neighbour sets, so the margin of the lattice is the segment's; a segment read in place of another of its length
    shows as rows in the wrong order), n drawn from NORMALS_LENGTHS with both long lengths also above segment 256; empty segments and
    segments of one and two rows; two exact repeats of earlier segments; a viewpoint per segment, clear of every normal's flip."""
    rng = np.random.default_rng(303)
    K = NORMALS_K
    lengths = rng.choice(NORMALS_LENGTHS, K, p=[0.3, 0.3, 0.2, 0.14, 0.03, 0.03])
    lengths[[1, 258, 299]] = (255, 257, 255)
    lengths[list(NORMALS_EMPTY)], lengths[list(NORMALS_ONE)], lengths[list(NORMALS_TWO)] = 0, 1, 2
    order = [rng.permutation(int(n)) for n in lengths]
    clouds = [None if n == 0 else sweep_lattice(int(n))[order[k]] for k, n in enumerate(lengths)]
    rows, seg, at = [], np.zeros((K, 2), np.int32), 0
    for k in rng.permutation(K):
        j = rng.uniform(-1, 1, (int(rng.integers(0, 4)), 3)).astype(np.float32)
        rows.append(j)
        at += j.shape[0]
        if k in NORMALS_REPEATS or clouds[k] is None:
            continue
        seg[k] = (at, clouds[k].shape[0])
        rows.append(clouds[k])
        at += clouds[k].shape[0]
    rows.append(rng.uniform(-1, 1, (3, 3)).astype(np.float32))
    for k in NORMALS_EMPTY:
        seg[k] = (11 * k, 0)
    # a viewpoint per segment, drawn again until no normal of the segment (at either list size; the yardstick's, which a row order does not
    # change) is within NORMALS_VIEW_CLEAR of perpendicular to its view direction: the orientation of every row is then no rounding decision
    viewpoint = np.zeros((K, 3), np.float32)
    for k in range(K):
        while True:
            viewpoint[k] = rng.uniform(-6, 6, 3)
            if clouds[k] is None or all(_view_clear(_sweep_normals(int(lengths[k]), m)[order[k]], clouds[k], viewpoint[k]) for m in NORMALS_MAX_NN):
                break
    for k, j in NORMALS_REPEATS.items():
        assert j < k and k >= 256 and lengths[j] >= 12
        seg[k], clouds[k], viewpoint[k] = seg[j], clouds[j], viewpoint[j]
    P_ = np.concatenate(rows)
    covered = np.zeros(P_.shape[0], bool)
    for a, n in seg:
        covered[a:a + n] = True
    return dict(P=P_, seg=seg, clouds=clouds, viewpoint=viewpoint, covered=covered)


@functools.lru_cache(maxsize=None)
def normals_batch300_solved(max_nn, with_viewpoint):
    """per segment estimate_normals(cloud, max_nn, no radius, its viewpoint or None) -- None for an empty segment"""
    b = normals_batch300()
    return [None if c is None else estimate_normals(c, max_nn, 0.0, b["viewpoint"][k] if with_viewpoint else None) for k, c in enumerate(b["clouds"])]
