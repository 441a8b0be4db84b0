"""Yardstick of the batched ICP (rap_amd/csrc/icp.hip): the algorithm of include/rapflow.h (pytorch3d's iterative_closest_point, one
problem) restated in numpy with brute-force neighbours, in fp64 by default; `dtype=np.float32` runs the same statements in fp32 (what a
plain fp32 implementation deviates by).  Plus the seeded inputs the ICP tests share, and fp64 restatements of the two reference metrics
that call ICP (eval/metrics.py:50-90 and the use_icp branch of :165-303) with the departures rap_amd/icp.py states.

Not a copy of any program: written from the published algorithm, like the project's chamfer / FPS / ball-query yardsticks."""
import functools

import numpy as np

T0 = (0.03, -0.02, 0.01)


def rotation(axis, degrees):
    """Rodrigues: the rotation matrix about `axis` (column-vector convention), fp64"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    th = np.deg2rad(degrees)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


R0 = rotation((0.3, -0.5, 0.8), 4.0)


def surf(rng, n, x_range=None):
    xy = rng.uniform(-0.5, 0.5, (n, 2))
    if x_range is not None:                                          # the same draws mapped to a narrower strip in x
        xy[:, 0] = x_range[0] + (xy[:, 0] + 0.5) * (x_range[1] - x_range[0])
    x, y = xy[:, 0], xy[:, 1]
    return np.stack([x, y, 0.15 * np.sin(5 * x) * np.cos(4 * y) + 0.1 * x * x], axis=1)


def make_pair(seed, nx, ny, x_range=None, y_range=None):
    """-> X (nx,3), Y (ny,3) fp32: two samplings of one surface, Y moved by R0 (4 degrees) and T0"""
    rng = np.random.default_rng(seed)
    X = surf(rng, nx, x_range)
    Yl = surf(rng, ny, y_range)
    return X.astype(np.float32), (Yl @ R0 + np.asarray(T0)).astype(np.float32)


def make_lattice_pair(seed, side=8, spacing=0.05, degrees=1.0, shift=0.002):
    """-> X, Y fp32, R (row-vector convention), T fp64: Y is a permutation of X R + T exactly as fp32 holds it (the truth is refitted to
    the rounded points by the caller's tolerance: the rounding of Y moves the best fit by less than 1e-8)"""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    X = ((g - (side - 1) / 2) * spacing + rng.uniform(-0.2, 0.2, g.shape) * spacing).astype(np.float32)
    R = rotation((0.5, 0.4, -0.7), degrees)
    T = np.asarray([shift, -shift, shift]) / np.sqrt(3.0)
    Y = (X.astype(np.float64) @ R + T)[rng.permutation(X.shape[0])]
    return X, Y.astype(np.float32), R, T


def nearest(Xt, Y, second=True, chunk=512):
    """-> first arg-min index, nearest distance^2, second-nearest distance^2 (inf without `second`) per row of Xt; direct differences
    in Xt's dtype"""
    idx = np.empty(Xt.shape[0], np.int64)
    d1 = np.empty(Xt.shape[0], Xt.dtype)
    d2 = np.full(Xt.shape[0], np.inf, Xt.dtype)
    Yc = [np.ascontiguousarray(Y[:, c]) for c in range(3)]
    for a in range(0, Xt.shape[0], chunk):
        dx, dy, dz = (Xt[a:a + chunk, c, None] - Yc[c][None, :] for c in range(3))
        D = dx * dx + dy * dy + dz * dz
        i = D.argmin(axis=1)                                           # the first minimum
        idx[a:a + chunk] = i
        d1[a:a + chunk] = D[np.arange(D.shape[0]), i]
        if second and Y.shape[0] > 1:
            D[np.arange(D.shape[0]), i] = np.inf
            d2[a:a + chunk] = D.min(axis=1)
    return idx, d1, d2


def kabsch(Xs, Ys):
    """least-squares proper rotation and translation with Xs R + T ~ Ys (row vectors)"""
    mx, my = Xs.mean(axis=0), Ys.mean(axis=0)
    H = (Xs - mx).T @ (Ys - my)
    U, _, Vt = np.linalg.svd(H)
    D = np.eye(3, dtype=Xs.dtype)
    D[2, 2] = np.sign(np.linalg.det(U @ Vt)) or 1.0
    R = U @ D @ Vt
    return R, my - mx @ R


class Result:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def icp(X, Y, init=None, max_iterations=100, relative_rmse_thr=1e-6, max_correspondence_distance=None, dtype=np.float64, margins=True):
    """one problem -> Result(R, T, rmse, iterations, converged, Xt, nn_margin, gate_margin).  nn_margin: the smallest gap between the
    nearest and the second-nearest DISTANCE over all points and iterations; gate_margin: the smallest | nearest distance - gate |
    (nn_margin stays inf with margins=False, which halves the work)."""
    X, Y = np.asarray(X, dtype), np.asarray(Y, dtype)
    R = np.eye(3, dtype=dtype) if init is None else np.asarray(init[0], dtype)
    T = np.zeros(3, dtype) if init is None else np.asarray(init[1], dtype)
    out = Result(R=R, T=T, rmse=np.nan, iterations=0, converged=False, Xt=X @ R + T, nn_margin=np.inf, gate_margin=np.inf)
    if X.shape[0] == 0 or Y.shape[0] == 0:
        return out
    prev = None
    for it in range(max_iterations):
        nn, d1, d2 = nearest(out.Xt, Y, margins)
        dist = np.sqrt(d1)
        out.nn_margin = min(out.nn_margin, float((np.sqrt(d2) - dist).min()))
        if max_correspondence_distance is not None:
            S = dist <= dtype(max_correspondence_distance)
            out.gate_margin = min(out.gate_margin, float(np.abs(dist.astype(np.float64) - max_correspondence_distance).min()))
        else:
            S = np.ones(X.shape[0], bool)
        if not S.any():
            out.rmse, out.converged = np.inf, False
            return out
        out.R, out.T = kabsch(X[S], Y[nn[S]])
        out.Xt = X @ out.R + out.T
        res = out.Xt[S] - Y[nn[S]]
        out.rmse = float(np.sqrt((res * res).sum(axis=1).mean()))
        out.iterations = it + 1
        if prev is not None and prev == 0.0:
            out.converged = True
            return out
        rel = 1.0 if prev is None else (prev - out.rmse) / prev
        if rel <= relative_rmse_thr:
            out.converged = True
            return out
        prev = out.rmse
    return out


# ---------------------------------------------------------------------------------------------
# the two reference metrics that call ICP, in fp64 on a packed batch (points (TP,3), points_per_part (B,P), anchor (B,P) bool)
# ---------------------------------------------------------------------------------------------
def part_offsets(ppp):
    flat = np.asarray(ppp, np.int64).reshape(-1)
    return (np.cumsum(flat) - flat).reshape(np.asarray(ppp).shape)


def align_anchor(gt, pred, ppp, anchor):
    """eval/metrics.py:50-90 with rap_amd.icp.align_anchor's three stated departures -> aligned cloud (TP,3) fp64"""
    gt, pred = np.asarray(gt, np.float64), np.asarray(pred, np.float64)
    off = part_offsets(ppp)
    out = pred.copy()
    B, P = np.asarray(ppp).shape
    for b in range(B):
        cand = [p for p in range(P) if ppp[b][p] > 0 and anchor[b][p]]
        if not cand:
            continue
        a, n = int(off[b][cand[0]]), int(ppp[b][cand[0]])
        r = icp(pred[a:a + n], gt[a:a + n])
        s, e = int(off[b][0]), int(off[b][P - 1] + ppp[b][P - 1])
        out[s:e] = pred[s:e] @ r.R + r.T
    return out


def transform_errors_icp(cond, gt, R_pred, t_pred, ppp, anchor, scale):
    """the use_icp branch of eval/metrics.py:165-303 -> (rot_mean (B,), trans_mean (B,), rot (B,P), trans (B,P)) fp64, degrees"""
    cond, gt = np.asarray(cond, np.float64), np.asarray(gt, np.float64)
    off = part_offsets(ppp)
    B, P = np.asarray(ppp).shape
    rot, trans = np.zeros((B, P)), np.zeros((B, P))
    for b in range(B):
        for p in range(P):
            n, a = int(ppp[b][p]), int(off[b][p])
            if n == 0 or anchor[b][p]:
                continue
            moved = cond[a:a + n] @ np.asarray(R_pred[b][p], np.float64).T + np.asarray(t_pred[b][p], np.float64)
            r = icp(gt[a:a + n], moved)
            rot[b, p] = np.rad2deg(np.arccos(np.clip(0.5 * (np.trace(r.R) - 1.0), -1.0, 1.0)))
            trans[b, p] = np.linalg.norm(r.T * float(scale[b]))
    cnt = ((np.asarray(ppp) != 0) & ~np.asarray(anchor, bool)).sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return rot.sum(axis=1) / cnt, trans.sum(axis=1) / cnt, rot, trans


# ---------------------------------------------------------------------------------------------
# the inputs the host and the GPU tests share (the yardstick of each is computed once per process)
# ---------------------------------------------------------------------------------------------
SINGLE_SIZES = [(256, 256), (300, 257), (513, 1000), (1000, 4099)]      # one full item; a partial second item, tile of 256 + 1; a last
SINGLE_SEED = 0                                                         # item of one query; sixteen candidate tiles + 3
EXACT_COUNT = [(3, 256, 256), (1, 256, 256)]                            # (seed, nx, ny) whose neighbour margin is >= 1e-5 throughout
GATE_CASE = dict(seed=5, nx=700, ny=900, x_range=(-0.5, 0.2), y_range=(-0.2, 0.5))
GATE = 0.03
INIT = (rotation((0.2, 0.9, -0.1), 2.0).T, np.asarray((0.02, -0.01, 0.005)))      # row-vector convention


@functools.lru_cache(maxsize=None)
def pair(seed, nx, ny, x_range=None, y_range=None):
    return make_pair(seed, nx, ny, x_range, y_range)


@functools.lru_cache(maxsize=None)
def solved(seed, nx, ny, x_range=None, y_range=None, gate=None, init=False, max_iterations=100, f32=False, margins=False):
    X, Y = pair(seed, nx, ny, x_range, y_range)
    return icp(X, Y, init=INIT if init else None, max_iterations=max_iterations, max_correspondence_distance=gate,
               dtype=np.float32 if f32 else np.float64, margins=margins)


def random_rotation(rng, max_degrees=180.0):
    return rotation(rng.normal(size=3), rng.uniform(0.3 * max_degrees, max_degrees))


@functools.lru_cache(maxsize=None)
def metrics_batch(seed=7):
    """A packed batch for align_anchor / compute_transform_errors_icp: B = 3, P = 3, parts of 100-300 points.  Sample 0 has an empty
    part and its anchor in slot 2, sample 1 its anchor in slot 0, sample 2 no anchor.  gt = cond R_gt^T + t_gt; the predicted poses are
    off by 1-3 degrees and up to 0.01, the predicted cloud by a 2 degree motion of the sample, both with 0.002 of noise per point (far
    below the point spacing, so that the last correspondences -- which alone decide R and T -- have a wide margin)."""
    rng = np.random.default_rng(seed)
    ppp = np.array([[150, 0, 260], [200, 120, 100], [300, 180, 110]], np.int64)
    anchor = np.array([[0, 0, 1], [1, 0, 0], [0, 0, 0]], bool)
    B, P = ppp.shape
    cu = np.concatenate([[0], np.cumsum(ppp.sum(axis=1))]).astype(np.int32)
    gt, cond, pred = [], [], []
    R_gt, t_gt, R_pred, t_pred = (np.zeros((B, P, 3, 3)), np.zeros((B, P, 3)), np.zeros((B, P, 3, 3)), np.zeros((B, P, 3)))
    for b in range(B):
        Ra, ta = random_rotation(rng, 2.0), rng.uniform(-0.01, 0.01, 3)
        for p in range(P):
            n = int(ppp[b, p])
            R_gt[b, p], t_gt[b, p] = random_rotation(rng), rng.uniform(-0.3, 0.3, 3)
            R_pred[b, p] = R_gt[b, p] @ rotation(rng.normal(size=3), rng.uniform(1.0, 3.0))
            t_pred[b, p] = t_gt[b, p] + rng.uniform(-0.01, 0.01, 3)
            c = surf(rng, n) @ random_rotation(rng)
            g = c @ R_gt[b, p].T + t_gt[b, p]
            cond.append(c + rng.normal(scale=0.002, size=c.shape))
            gt.append(g)
            pred.append(g @ Ra + ta + rng.normal(scale=0.002, size=g.shape))
    f = lambda parts: np.concatenate(parts).astype(np.float32)
    return dict(gt=f(gt), cond=f(cond), pred=f(pred), ppp=ppp, anchor=anchor, cu=cu, R_gt=R_gt.astype(np.float32),
                t_gt=t_gt.astype(np.float32), R_pred=R_pred.astype(np.float32), t_pred=t_pred.astype(np.float32),
                scale=np.array([0.8, 1.0, 1.3], np.float32))


# ---------------------------------------------------------------------------------------------
# table scale: K = 300 problems in one call, and one problem of more than 64 items (tests/test_table_scale_gpu.py)
# ---------------------------------------------------------------------------------------------
BATCH_K = 300
BATCH_MARGIN = 5e-5            # the smallest nearest / second-nearest gap (a distance) of every compared problem, over all its iterations:
#                                five times the 1e-5 of the normals tests, fifty times what fp32 moves a distance by
# the small surface pairs of the batch: problem number -> (seed, nx, ny), seeds chosen so that both estimators keep BATCH_MARGIN
BATCH_SURFACES = {5: (117, 48, 96), 13: (126, 48, 96), 21: (136, 64, 128), 29: (138, 48, 96), 37: (139, 64, 128), 45: (146, 80, 160),
                  53: (148, 64, 128), 61: (153, 48, 96), 69: (154, 64, 128), 77: (156, 48, 96), 85: (161, 80, 160), 93: (174, 48, 96),
                  101: (178, 64, 128), 109: (187, 64, 128), 117: (201, 48, 96), 125: (210, 48, 96), 133: (216, 48, 96), 141: (231, 48, 96),
                  149: (240, 48, 96), 157: (247, 64, 128), 165: (253, 64, 128), 173: (265, 64, 128), 181: (270, 48, 96), 189: (273, 48, 96),
                  197: (277, 64, 128), 205: (282, 48, 96), 213: (295, 64, 128), 221: (300, 48, 96), 229: (306, 48, 96), 237: (316, 64, 128),
                  245: (336, 48, 96), 253: (339, 48, 96), 261: (343, 64, 128), 269: (349, 64, 128), 277: (357, 48, 96)}
BATCH_EMPTY_X, BATCH_EMPTY_Y, BATCH_ONE_POINT = (259, 281), (263, 285), (267, 289)
# problem number -> the earlier problem (below 256) whose y segment it searches: its grid's owner sits in another round of the plan loop
BATCH_SHARED_Y = {271: 3, 275: 129, 279: 254, 293: 3, 297: 40}


# THE POINT-TO-PLANE VARIANT of the batch.  An exact fit ends at a point-to-plane rmse of 1e-8 that is made of input roundings alone, and
# whether that still decreases by a millionth is no property of the algorithm: the iteration count of such a problem cannot be compared.
# So in this variant every lattice problem carries a residual (residual_lattice_pair: the x points moved by up to a tenth of the spacing,
# as big_pair does), and the seeds -- BATCH_PLANE_STEPS[k] steps of 300 past 1000 + k for a lattice, BATCH_PLANE_SURFACES for a surface
# pair -- are the first of their sequence at which no stopping decision of the yardstick is a matter of rounding
# (icp_plane_oracle.BATCH_THR; tests/test_icp_plane_host.py proves it for every problem).
BATCH_PLANE_SURFACES = {5: (126, 48, 96), 13: (129, 48, 96), 21: (141, 48, 96), 29: (148, 64, 128), 37: (161, 80, 160), 45: (162, 48, 96),
                        53: (168, 48, 96), 61: (184, 64, 128), 69: (187, 64, 128), 77: (195, 48, 96), 85: (201, 48, 96), 93: (209, 80, 160),
                        101: (213, 48, 96), 109: (216, 48, 96), 117: (227, 80, 160), 125: (228, 48, 96), 133: (231, 48, 96), 141: (235, 64, 128),
                        149: (247, 64, 128), 157: (261, 48, 96), 165: (268, 64, 128), 173: (273, 48, 96), 181: (276, 48, 96), 189: (282, 48, 96),
                        197: (288, 48, 96), 205: (295, 64, 128), 213: (297, 48, 96), 221: (300, 48, 96), 229: (313, 64, 128), 237: (316, 64, 128),
                        245: (329, 80, 160), 253: (336, 48, 96), 261: (339, 48, 96), 269: (343, 64, 128), 277: (348, 48, 96)}
BATCH_PLANE_STEPS = "0" * 39 + "1" + "0" * 260      # one digit per problem


def batch_lattice_args(k, plane=False):
    return dict(seed=1000 + k + 300 * (int(BATCH_PLANE_STEPS[k], 36) if plane else 0), side=4 + k % 3, degrees=0.5 + (k % 11) / 10.0)


def residual_lattice_pair(seed, side, degrees, spacing=0.05):
    """make_lattice_pair with every x point moved by up to a tenth of the spacing per axis: the same correspondences, a residual near 3e-3"""
    X, Y, R, T = make_lattice_pair(seed, side, spacing, degrees)
    X = X.astype(np.float64) + np.random.default_rng(seed + 7).uniform(-0.1, 0.1, X.shape) * spacing
    return X.astype(np.float32), Y, R, T


@functools.lru_cache(maxsize=None)
def batch300(plane=False):
    """(plane: the variant for the point-to-plane estimator, see BATCH_PLANE_STEPS)
    -> dict(X, Y, x_seg (K,2), y_seg (K,2), parts, init_R (K,3,3), init_T (K,3), kinds): K = 300 problems whose segments lie in
    a shuffled order with 0 to 3 junk rows between them.  Lattice pairs with a known truth (make_lattice_pair: side 4..6, 0.5..1.5
    degrees), the surface pairs of BATCH_SURFACES (which take different numbers of iterations), empty-X, empty-Y and one-point problems
    at numbers >= 256, and the problems of BATCH_SHARED_Y: the x of an earlier lattice problem without its last 5 points, against that
    problem's own y segment.  parts[k] = (X_k, Y_k) as the yardstick takes them (None for a problem that is not compared); init_R, init_T:
    a start of up to 0.2 degrees and 5e-4 per problem, for the variant with init_transform."""
    rng = np.random.default_rng(300)
    K = BATCH_K
    xs, ys, kinds, y_of = [None] * K, [None] * K, ["lattice"] * K, list(range(K))
    surfaces = BATCH_PLANE_SURFACES if plane else BATCH_SURFACES
    for k in range(K):
        if k in BATCH_SURFACES:
            xs[k], ys[k] = pair(*surfaces[k])
            kinds[k] = "surface"
        else:
            xs[k], ys[k] = (residual_lattice_pair if plane else make_lattice_pair)(**batch_lattice_args(k, plane))[:2]
    for k, j in BATCH_SHARED_Y.items():
        assert kinds[j] == "lattice" and j < 256 <= k
        xs[k], ys[k], y_of[k], kinds[k] = xs[j][:-5], ys[j], j, "shared_y"
    for k in BATCH_EMPTY_X:
        xs[k], kinds[k] = xs[k][:0], "empty_x"
    for k in BATCH_EMPTY_Y:
        ys[k], kinds[k] = ys[k][:0], "empty_y"
    for k in BATCH_ONE_POINT:
        xs[k], kinds[k] = xs[k][:1], "one_point"
    junk = lambda: rng.uniform(-1, 1, (int(rng.integers(0, 4)), 3)).astype(np.float32)

    def pack(clouds, own):
        rows, seg, at = [junk()], np.zeros((K, 2), np.int32), 0
        at = rows[0].shape[0]
        for k in rng.permutation(K):
            if own[k] != k:
                continue
            seg[k] = (at, clouds[k].shape[0])
            rows += [clouds[k], junk()]
            at += clouds[k].shape[0] + rows[-1].shape[0]
        for k in range(K):
            if own[k] != k:
                seg[k] = seg[own[k]]
        return np.concatenate(rows), seg
    X, x_seg = pack(xs, list(range(K)))
    Y, y_seg = pack(ys, y_of)
    for k in BATCH_EMPTY_X:
        x_seg[k] = (17, 0)
    for k in BATCH_EMPTY_Y:
        y_seg[k] = (40, 0)
    init_R = np.stack([rotation(rng.normal(size=3), rng.uniform(0.0, 0.2)).T for _ in range(K)]).astype(np.float32)
    init_T = rng.uniform(-5e-4, 5e-4, (K, 3)).astype(np.float32)
    parts = [(xs[k], ys[k]) if kinds[k] in ("lattice", "surface", "shared_y") else None for k in range(K)]
    return dict(X=X, Y=Y, x_seg=x_seg, y_seg=y_seg, parts=parts, init_R=init_R, init_T=init_T, kinds=kinds)


@functools.lru_cache(maxsize=None)
def batch300_solved(init=False, f32=False):
    """the yardstick of every compared problem of batch300(), None for the others (f32: the same statements in fp32, without margins)"""
    b = batch300()
    return [None if p is None else icp(p[0], p[1], init=(b["init_R"][k].astype(np.float64), b["init_T"][k].astype(np.float64)) if init else None,
                                       dtype=np.float32 if f32 else np.float64, margins=not f32)
            for k, p in enumerate(b["parts"])]


BIG_PLANE_SEEDS = (11, 12)
BIG_NX = (16_700, 33_000)      # 66 and 129 items of 256 queries: a second and a third round of the finish kernels' lane-strided sum


@functools.lru_cache(maxsize=None)
def big_pair(nx, seed=0, side=6, spacing=0.05):
    """-> X (nx,3), Y (side^3,3) fp32: the points of a lattice pair's X drawn nx times with replacement, each moved by up to a tenth of
    the spacing per axis; Y as make_lattice_pair leaves it (moved by one degree, permuted).  Not an exact fit: the rmse stays near 3e-3."""
    X0, Y, _, _ = make_lattice_pair(seed, side, spacing)
    rng = np.random.default_rng(seed + 1)
    X = X0[rng.integers(0, X0.shape[0], nx)].astype(np.float64) + rng.uniform(-0.1, 0.1, (nx, 3)) * spacing
    return X.astype(np.float32), Y


@functools.lru_cache(maxsize=None)
def big_batch(nx, plane=False):
    """the big problem as problem 1 of 3, between two small lattice problems: its first item is not item 0.  plane: the two neighbours
    carry a residual (BIG_PLANE_SEEDS, chosen as BATCH_PLANE_STEPS is).  -> X, Y, x_seg, y_seg, parts"""
    small = (lambda seed, side: residual_lattice_pair(seed, side, 1.0)[:2]) if plane else (lambda seed, side: make_lattice_pair(seed, side)[:2])
    sa, sc = BIG_PLANE_SEEDS if plane else (11, 12)
    a, b, c = small(sa, 4), big_pair(nx), small(sc, 5)
    X, Y = np.concatenate([a[0], b[0], c[0]]), np.concatenate([c[1], a[1], b[1]])
    na, nb, nc = a[0].shape[0], b[0].shape[0], c[0].shape[0]
    x_seg = np.array([[0, na], [na, nb], [na + nb, nc]], np.int32)
    y_seg = np.array([[nc, na], [nc + na, b[1].shape[0]], [0, nc]], np.int32)
    return X, Y, x_seg, y_seg, [a, b, c]


@functools.lru_cache(maxsize=None)
def big_solved(nx):
    return [icp(x, y) for x, y in big_batch(nx)[4]]
