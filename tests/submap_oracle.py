"""float64 numpy restatement of the four reference functions behind rap_amd.submaps, and the inputs its tests share.

  deskew                       dataset_utils.deskewing (dataset_utils.py:682-747).  UNPINNED: the reference evaluates
                               roma.rotmat_slerp(I, R, s) and roma is not installed, so nothing here ran against the reference's own
                               output.  R(s) = exp(s log R) is restated (``slerp_rotation``) and cross-checked against
                               scipy.spatial.transform.Rotation.from_rotvec(s * rotvec), s < 0 and s > 1 included
                               (tests/test_submaps_host.py).  The reference holds ts and the result in fp32; here everything after the
                               fp32 inputs is float64 (``dtype=np.float32`` runs the same formula in fp32: the measured distance between
                               the two is the bound of the GPU test).
  transform_points / transform_normals / create_submap_from_frames
                               dataset_utils.py:361-407, submap_utils.py:26-50.  PINNED by tests/golden/submaps.npz.
  overlap_ratio                calculate_point_cloud_overlap_ratio_fast (dataset_utils.py:603-650) below its subsampling limit.  PINNED.
  groups_connected             the union-find of check_submap_validity (submap_utils.py:102-164).  PINNED.
The fixture holds inputs and the outputs of the reference's unmodified modules (scripts/make_submap_golden.py).

THE MARGIN RULE of the overlap tests: every world coordinate divided by voxel_size is at least 1e-6 * max(1, |q|) away from an integer in
this oracle (``voxel_margin``), so that no rounding of R p + t or of the quotient can move a point into another voxel; then n_voxels and
every ratio are demanded exactly.  The rule guards against ROUNDING; where the quotient has none -- pose = None and voxel_size = 1, so
that q is the fp32 coordinate itself -- it is not needed, and the two cases at the 21-bit limit of the key (|q| about 1e6, where no
coordinate can be 1.0 away from an integer) are of that kind (``exact_quotient``).
"""
import functools

import numpy as np

# worst |fp32 formula - fp64 formula| / max(1, |p|_inf + |T|_inf) over deskew_case() and deskew_short_case(), every ts_mid: measured by
# tests/test_submaps_host.py::test_deskew_bound_is_the_measured_fp32_deviation, which holds this constant to the measurement's three digits
DESKEW_F32_DEVIATION = 4.66e-7
DESKEW_TOL = 4 * DESKEW_F32_DEVIATION        # the GPU tests' bound
DESKEW_LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, 1025)
DESKEW_THETAS = (0.0, 1e-7, 1e-3, 0.3, 3.0)
TS_MIDS = (0.0, 0.5, 1.0)


# ---- rotations ----------------------------------------------------------------------------------------------------------------------
def hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def rotation(axis, theta):
    """exp(theta [axis]x) in float64, axis normalised here"""
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    K = hat(k)
    return np.eye(3) + np.sin(theta) * K + (1.0 - np.cos(theta)) * (K @ K)


def rotvec(R):
    """log of a rotation with angle in [0, pi): theta * axis"""
    R = np.asarray(R, np.float64)
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    sn, cs = np.linalg.norm(v), 0.5 * (np.trace(R) - 1.0)
    th = np.arctan2(sn, cs)
    k = 1.0 + sn * sn / 6.0 + 3.0 * sn ** 4 / 40.0 if (sn < 1e-4 and cs > 0) else th / sn      # theta / sin(theta)
    return v * k


def slerp_rotation(R, s):
    """(n,3,3): exp(s_i log R) -- what roma.rotmat_slerp(I, R, s) evaluates, for any real s"""
    w = rotvec(R)
    th = np.linalg.norm(w)
    s = np.asarray(s, np.float64).reshape(-1)
    if th == 0.0:
        return np.broadcast_to(np.eye(3), (s.shape[0], 3, 3)).copy()
    K = hat(w / th)
    ang = s * th
    return np.eye(3)[None] + np.sin(ang)[:, None, None] * K[None] + (1.0 - np.cos(ang))[:, None, None] * (K @ K)[None]


# ---- deskew ---------------------------------------------------------------------------------------------------------------------------
def deskew(points, ts, rel_pose, ts_mid=0.5, dtype=np.float64):
    """one sweep: p' = R(s) p + s T, s = (ts - min) / (max - min) - ts_mid (0.5 - ts_mid where max - min <= 1e-8).  Axis and angle come from
    float64 whatever ``dtype`` is; everything per point runs in ``dtype``: p + A (u x p) + B (u x (u x p)) + s T with u = s w,
    x = |s| theta, A = sin x / x, B = (1 - cos x) / x^2 in their half-angle forms."""
    f = dtype
    p = np.asarray(points, np.float32).astype(f)
    if p.shape[0] == 0:
        return p
    t = np.asarray(ts, np.float32).reshape(-1).astype(f)
    rel = np.asarray(rel_pose, np.float64)
    w64 = rotvec(rel[:3, :3])
    w, theta, T = w64.astype(f), f(np.linalg.norm(w64)), rel[:3, 3].astype(f)
    lo, hi = t.min(), t.max()
    s = (t - lo) / (hi - lo) - f(ts_mid) if hi - lo > f(1e-8) else np.full_like(t, f(0.5) - f(ts_mid))
    u = s[:, None] * w[None]
    x = np.abs(s) * theta
    small = x < f(1e-3)
    xs = np.where(small, f(1.0), x)
    sh, ch = np.sin(f(0.5) * xs), np.cos(f(0.5) * xs)
    A = np.where(small, f(1.0) - x * x / f(6.0), f(2.0) * sh * ch / xs)
    B = np.where(small, f(0.5) - x * x / f(24.0), f(2.0) * sh * sh / (xs * xs))
    c1 = np.cross(u, p)
    c2 = np.cross(u, c1)
    out = p + A[:, None] * c1 + B[:, None] * c2 + s[:, None] * T[None]
    assert out.dtype == f
    return out


def deskew_packed(points, ts, cu, rel_pose, ts_mid=0.5, dtype=np.float64):
    out = np.zeros((points.shape[0], 3), dtype)
    for k in range(len(cu) - 1):
        a, b = int(cu[k]), int(cu[k + 1])
        out[a:b] = deskew(points[a:b], ts[a:b], rel_pose[k], ts_mid, dtype)
    return out


def deskew_scale(points, cu, rel_pose):
    """per point max(1, |p|_inf + |T|_inf): what the deskew bound is relative to"""
    sc = np.ones(points.shape[0])
    for k in range(len(cu) - 1):
        a, b = int(cu[k]), int(cu[k + 1])
        sc[a:b] = np.maximum(1.0, np.abs(points[a:b].astype(np.float64)).max(axis=1, initial=0.0) + np.abs(rel_pose[k][:3, 3]).max())
    return sc


def make_pose(rng, theta, t_scale=1.5, t_offset=(0.0, 0.0, 0.0)):
    M = np.eye(4)
    if theta != 0.0:
        M[:3, :3] = rotation(rng.normal(size=3), theta)
    M[:3, 3] = rng.uniform(-t_scale, t_scale, size=3) + np.asarray(t_offset)
    return M


def frame_points(rng, n):
    return np.stack([rng.uniform(-40, 40, n), rng.uniform(-40, 40, n), rng.uniform(-3, 5, n)], axis=1).astype(np.float32)


def deskew_case():
    """F = 13 sweeps in one packed call: every length of DESKEW_LENGTHS and every angle of DESKEW_THETAS (theta = 0 with a translation), then a
    frame whose rel_pose is exactly the identity, one whose ts are all equal (the 1e-8 rule; the one-point frame is another) and two more
    so that every angle meets a frame of more than one point.  In every frame of two points or more the largest ts is its FIRST entry and the smallest
    its LAST.  -> points (N,3) fp32, ts (N,) fp32, cu (F+1,) int32, rel_pose (F,4,4) float64, names"""
    rng = np.random.default_rng(20261020)
    lengths = list(DESKEW_LENGTHS) + [130, 130, 70, 70]
    thetas = [0.3, 3.0, 0.0, 1e-7, 1e-3, 0.3, 3.0, 1e-3, 0.3, None, 0.3, 0.0, 1e-7]
    names = [f"len{n}_theta{th}" for n, th in zip(lengths, thetas)]
    names[9], names[10] = "identity", "constant_ts"
    pts, ts, poses = [], [], []
    for k, (n, th) in enumerate(zip(lengths, thetas)):
        pts.append(frame_points(rng, n))
        t = rng.uniform(0.0, 0.1, n).astype(np.float32)
        if n >= 2:
            t[0], t[-1] = np.float32(0.1), np.float32(0.0)
        if k == 10:
            t[:] = np.float32(0.05)
        ts.append(t)
        poses.append(np.eye(4) if th is None else make_pose(rng, th))
    cu = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    return np.concatenate(pts), np.concatenate(ts), cu, np.stack(poses), names


def deskew_short_case():
    """40 sweeps of 5 points: ONE block of rows that lies in more frames (40) than a block keeps axis and angle for at a time (16), every
    angle of DESKEW_THETAS in turn.  -> points, ts, cu, rel_pose"""
    rng = np.random.default_rng(4005)
    F, n = 40, 5
    pts, ts, poses = [], [], []
    for k in range(F):
        pts.append(frame_points(rng, n))
        t = rng.uniform(0.0, 0.1, n).astype(np.float32)
        t[0], t[-1] = np.float32(0.1), np.float32(0.0)
        ts.append(t)
        poses.append(make_pose(rng, DESKEW_THETAS[k % len(DESKEW_THETAS)]))
    return np.concatenate(pts), np.concatenate(ts), (np.arange(F + 1) * n).astype(np.int32), np.stack(poses)


def ulps(got, want64):
    """largest distance in fp32 ulp between an fp32 array and the fp32 rounding of a float64 one (signs must agree)"""
    want = want64.astype(np.float32)
    return np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)).max() if got.size else 0


SCALE_F = (255, 256, 257, 4099)              # frame counts on either side of one round of the 256-thread table walk, and sixteen rounds
SCALE_LONG = 1100                            # rows of the one long frame of scale_frames_case: more than a chunk of 1024


def scale_frames_case(F):
    """F sweeps whose lengths cycle through 0..7 rows (every eighth frame is empty, and a 1024-row chunk lies in about 290 frames), except
    frame F // 2 with SCALE_LONG rows (so that some chunks lie in ONE frame) and an angle of 0.3.  The other angles cycle through DESKEW_THETAS; every 37th frame has
    an exactly-identity rel_pose.  Stamps as in deskew_case: the largest first, the smallest last.  Poses and unit normals for the fuse
    of the same frames.  -> dict(points, ts, cu, rel_pose, pose, normals, identity (frame numbers), long (frame number))"""
    rng = np.random.default_rng(9000 + F)
    lengths = [k % 8 for k in range(F)]
    lengths[F // 2] = SCALE_LONG
    identity = [k for k in range(5, F, 37) if k != F // 2]
    pts, ts, rel, pose = [], [], [], []
    for k, n in enumerate(lengths):
        pts.append(frame_points(rng, n))
        t = rng.uniform(0.0, 0.1, n).astype(np.float32)
        if n >= 2:
            t[0], t[-1] = np.float32(0.1), np.float32(0.0)
        ts.append(t)
        rel.append(np.eye(4) if k in identity else make_pose(rng, 0.3 if k == F // 2 else DESKEW_THETAS[k % len(DESKEW_THETAS)]))
        pose.append(make_pose(rng, rng.uniform(0.1, 3.0), 30.0))
    P = np.concatenate(pts)
    v = rng.normal(size=(P.shape[0], 3))
    cu = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    return dict(points=P, ts=np.concatenate(ts), cu=cu, rel_pose=np.stack(rel), pose=np.stack(pose),
                normals=(v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32), identity=identity, long=F // 2)


def table_per(n):
    """entries of an n-entry table that one thread of the sanitising block walks (rap_amd/csrc/submaps.hip: ceil(n / 256))"""
    return -(-n // 256)


def malformed_tables(cu, at, limit, need_last=True):
    """single-entry edits of a prefix table at entry `at` (which must not be a thread's first): one decreasing entry, one entry past
    `limit`, and (where the last entry has to be `limit`) a last entry one short of it.  -> [(name, table)]"""
    n, per = len(cu), table_per(len(cu))
    assert per >= 2 and at % per != 0 and 10 < at < n - 1 and (not need_last or (n - 1) % per != 0)
    out = []
    dec = cu.copy()
    dec[at] = cu[at - 10]
    assert dec[at] < dec[at - 1]
    out.append(("decreasing", dec))
    past = cu.copy()
    past[at] = limit + 5
    out.append(("past the limit", past))
    if need_last:
        short = cu.copy()
        short[-1] = limit - 1
        assert short[-1] >= short[-2]                        # still non-decreasing: ONLY the end is wrong
        out.append(("short of the end", short))
    return out


def boundary_repeats_case(F=4099):
    """a VALID table of F one-row frames whose only repeated values sit where one thread's entries end and the next one's begin: frame
    per * t - 1 is empty for every t >= 1, so cu[per * t] == cu[per * t - 1].  -> points, ts, cu, rel_pose"""
    rng = np.random.default_rng(17)
    per = table_per(F + 1)
    lengths = np.ones(F, np.int64)
    lengths[np.arange(per, F + 1, per) - 1] = 0
    cu = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    rep = np.flatnonzero(np.diff(cu) == 0) + 1
    assert rep.size >= 200 and (rep % per == 0).all()
    n = int(cu[-1])
    rel = np.stack([make_pose(rng, DESKEW_THETAS[k % len(DESKEW_THETAS)]) for k in range(F)])
    return frame_points(rng, n), rng.uniform(0.0, 0.1, n).astype(np.float32), cu, rel


# ---- fuse -----------------------------------------------------------------------------------------------------------------------------
def transform_points(points, transform):
    homo = np.hstack([points, np.ones((points.shape[0], 1))])
    return (transform @ homo.T).T[:, :3]


def transform_normals(normals, transform):
    if len(normals) == 0:
        return normals
    out = (transform[:3, :3] @ normals.T).T
    norms = np.linalg.norm(out, axis=1, keepdims=True)
    return out / np.where(norms < 1e-8, 1.0, norms)


def create_submap_from_frames(points_list, poses_list, start_idx, num_frames, normals_list=None):
    all_points, all_normals = [], []
    for i in range(start_idx, min(start_idx + num_frames, len(points_list))):
        all_points.append(transform_points(points_list[i], poses_list[i]) if i < len(poses_list) else points_list[i])
        if normals_list and i < len(normals_list) and normals_list[i] is not None:
            all_normals.append(transform_normals(normals_list[i], poses_list[i]) if i < len(poses_list) else normals_list[i])
    if not all_points:
        return np.array([]), None
    return np.vstack(all_points), (np.vstack(all_normals) if all_normals else None)


def fuse_packed(points, cu, pose, normals=None, origin=None):
    """float64 world points (minus origin) and normals of a packed call"""
    world = np.zeros((points.shape[0], 3))
    wn = np.zeros((points.shape[0], 3)) if normals is not None else None
    for k in range(len(cu) - 1):
        a, b = int(cu[k]), int(cu[k + 1])
        if b > a:
            world[a:b] = transform_points(points[a:b].astype(np.float64), pose[k])
            if normals is not None:
                wn[a:b] = transform_normals(normals[a:b].astype(np.float64), pose[k])
    if origin is not None:
        world = world - np.asarray(origin, np.float64)[None]
    return world, wn


FUSE_FAR = (10_000.0, -7_000.0, 120.0)       # a 10 km translation


def fuse_case():
    """the frame lengths of DESKEW_LENGTHS, poses 10 km from the origin, unit normals with a zero normal in every frame of two or more"""
    rng = np.random.default_rng(77)
    lengths = list(DESKEW_LENGTHS)
    pts = [frame_points(rng, n) for n in lengths]
    nrm = []
    for n in lengths:
        v = rng.normal(size=(n, 3))
        v = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
        if n >= 2:
            v[n // 2] = 0.0
        nrm.append(v)
    pose = np.stack([make_pose(rng, rng.uniform(0.1, 3.0), 30.0, FUSE_FAR) for _ in lengths])
    cu = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    return np.concatenate(pts), np.concatenate(nrm), cu, pose


# ---- overlap --------------------------------------------------------------------------------------------------------------------------
def voxel_sets(world_list, voxel_size):
    sets = []
    for w in world_list:
        w = np.asarray(w, np.float64).reshape(-1, 3)
        w = w[np.isfinite(w).all(axis=1)]
        sets.append(set(map(tuple, np.floor(w / voxel_size).astype(np.int64))))
    return sets


def overlap_ratio(points1, points2, voxel_size=2.0):
    if len(points1) == 0 or len(points2) == 0:
        return 0.0
    a, b = voxel_sets([points1, points2], voxel_size)
    union = len(a | b)
    return len(a & b) / union if union else 0.0


def overlap_matrix(world_list, voxel_size):
    """-> ratio (S,S) float64, n_voxels (S,) int64 for S clouds of float64 world points (non-finite rows dropped)"""
    sets = voxel_sets(world_list, voxel_size)
    S = len(sets)
    ratio = np.zeros((S, S))
    for i in range(S):
        for j in range(S):
            if sets[i] and sets[j]:
                ratio[i, j] = len(sets[i] & sets[j]) / len(sets[i] | sets[j])
    return ratio, np.array([len(s) for s in sets], np.int64)


def voxel_margin(world, voxel_size):
    """smallest distance of a coordinate / voxel_size from an integer, relative to max(1, |q|) (finite rows only)"""
    w = np.asarray(world, np.float64).reshape(-1, 3)
    q = w[np.isfinite(w).all(axis=1)] / voxel_size
    return float((np.abs(q - np.round(q)) / np.maximum(1.0, np.abs(q))).min()) if q.size else 1.0


def case_world(c):
    """the float64 world clouds of the S submaps of an overlap case, from its fp32 points"""
    world, _ = fuse_packed(c["points"], c["cu"], c["pose"]) if c["pose"] is not None else (c["points"].astype(np.float64), None)
    cu, sf = c["cu"], c["submap_frames"]
    return [world[int(cu[sf[s]]):int(cu[sf[s + 1]])] for s in range(len(sf) - 1)]


def exact_quotient(c):
    """pose None and voxel_size 1: q is the fp32 coordinate, no operation rounds (the margin rule guards nothing here)"""
    return c["pose"] is None and c["voxel_size"] == 1.0


def _build(rng, voxel_sets_, voxel_size, posed, dup=2, frames_per_submap=2, extra_rows=None):
    """submaps given as integer voxel arrays -> a packed case.  Every voxel gets `dup` points (an int, or one per submap) at offsets in [0.25, 0.75]^3; a submap is
    split into `frames_per_submap` frames; with `posed` every frame gets its own pose and the points go to that frame's coordinates."""
    pts, lengths, poses, sf = [], [], [], [0]
    for s, vox in enumerate(voxel_sets_):
        vox = np.asarray(vox, np.float64).reshape(-1, 3)
        m = dup if isinstance(dup, int) else dup[s]
        w = (np.repeat(vox, m, axis=0) + rng.uniform(0.25, 0.75, (vox.shape[0] * m, 3))) * voxel_size
        w = w[rng.permutation(w.shape[0])]
        if extra_rows and s in extra_rows:
            w = np.concatenate([w[:1], extra_rows[s], w[1:]]) if w.shape[0] else extra_rows[s]
        for part in np.array_split(w, frames_per_submap if isinstance(frames_per_submap, int) else frames_per_submap[s]):
            M = make_pose(rng, rng.uniform(0.1, 3.0), 20.0) if posed else None
            local = (part - M[:3, 3]) @ M[:3, :3] if posed else part            # R^T (w - t), rows
            pts.append(local.astype(np.float32))
            lengths.append(part.shape[0])
            poses.append(M)
        sf.append(len(lengths))
    return dict(points=np.concatenate(pts).reshape(-1, 3), cu=np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32),
                submap_frames=np.asarray(sf, np.int32), pose=np.stack(poses) if posed else None, voxel_size=voxel_size)


def _lattice(rng, n, lo=(-12, -9, -3), hi=(12, 9, 4)):
    """n distinct integer voxels of a box that straddles zero on every axis"""
    g = np.stack(np.meshgrid(*[np.arange(a, b) for a, b in zip(lo, hi)], indexing="ij"), axis=-1).reshape(-1, 3)
    return g[rng.permutation(g.shape[0])[:n]]


OVERLAP_CASES = ("one", "two", "three", "edge", "counts", "counts_posed", "edge_posed", "extent_max", "rows_100k")


def overlap_case(name):
    """the inputs of tests/test_submaps_gpu.py's overlap tests (the host test asserts the margin rule for every one of them):
      one            S = 1: 300 voxels, negative coordinates
      two            S = 2: two random halves of a pool (a ratio strictly between 0 and 1)
      three          S = 3: a set, the same set moved far away (disjoint: 0), 200 points in ONE voxel; an inf and a NaN row in the first
      edge           S = 5: no points, ONE point (one row, an empty second frame), a set of 257, the same voxels from other points
                     (ratio 1), a strict subset of 100
      counts         S = 5: 255, 256, 257, 5 and 3000 unique voxels drawn from one pool of 3600: every chunk boundary against 5 and 3000
      *_posed        the same through per-frame poses (points in sensor coordinates); the others are pose = None
      extent_max     S = 2, voxel_size 1, pose None: voxel offsets 0 and 2^21 - 1 on x -- the widest grid the key takes
      rows_100k      S = 3, 99 000 rows (three draws of 11 000 voxels from a pool of 32 000, three points each): a size between one sort
                     block and a whole drive, where the device-wide sorts take another path than at a few thousand rows"""
    rng = np.random.default_rng(sum(map(ord, name)))
    posed = name.endswith("_posed")
    base = name[:-6] if posed else name
    vs = 0.5 if posed else 2.0
    if base == "one":
        return _build(rng, [_lattice(rng, 300)], vs, posed)
    if base == "two":
        pool = _lattice(rng, 700)
        return _build(rng, [pool[:450], pool[250:]], vs, posed)
    if base == "three":
        a = _lattice(rng, 320)
        bad = {0: np.array([[np.inf, 1.0, 1.0], [1.0, np.nan, 1.0]])}
        return _build(rng, [a, a + np.array([500, 0, -40]), np.repeat([[-3, 2, -1]], 100, axis=0)], vs, posed, extra_rows=bad)
    if base == "edge":
        a = _lattice(rng, 257)
        return _build(rng, [np.zeros((0, 3)), a[:1] + 50, a, a, a[:100]], vs, posed, dup=[2, 1, 2, 2, 2])
    if base == "counts":
        pool = _lattice(rng, 3600, (-10, -10, -8), (10, 10, 10))
        pick = lambda n: pool[rng.permutation(pool.shape[0])[:n]]
        return _build(rng, [pick(255), pick(256), pick(257), pick(5), pick(3000)], vs, posed, dup=1, frames_per_submap=3)
    if base == "rows_100k":
        pool = _lattice(rng, 32000, (-20, -20, -10), (20, 20, 10))
        pick = lambda n: pool[rng.permutation(pool.shape[0])[:n]]
        return _build(rng, [pick(11000), pick(11000), pick(11000)], vs, posed, dup=3, frames_per_submap=3)
    if base == "extent_max":
        return extent_case((1 << 21) - 1)
    raise KeyError(name)


def extent_case(span):
    """two one-point submaps `span` voxels apart on x at voxel_size 1, pose None: coordinates k + 0.5, exact in fp32 up to 2^22"""
    lo = -(span // 2)
    pts = np.array([[lo + 0.5, 0.5, -0.5], [lo + span + 0.5, 0.5, -0.5]], np.float32)
    assert (pts.astype(np.float64)[:, 0] == np.array([lo + 0.5, lo + span + 0.5])).all()
    return dict(points=pts, cu=np.array([0, 1, 2], np.int32), submap_frames=np.array([0, 1, 2], np.int32), pose=None, voxel_size=1.0)


# ---- overlap at table scale -------------------------------------------------------------------------------------------------------------
def overlap_matrix_incidence(world_list, voxel_size):
    """overlap_matrix by an incidence matrix: M (S,V) says which of the V distinct voxels of the call each submap holds, M M^T in float64
    holds every |A n B| (sums of at most V ones: exact), and the ratio is the same division of the same two integers -- the same doubles
    as the set form (tests/test_submaps_host.py holds the two together), at a cost that allows S = 4096"""
    vox, sid = [], []
    for s, w in enumerate(world_list):
        w = np.asarray(w, np.float64).reshape(-1, 3)
        w = w[np.isfinite(w).all(axis=1)]
        vox.append(np.floor(w / voxel_size).astype(np.int64))
        sid.append(np.full(w.shape[0], s, np.int64))
    S = len(world_list)
    vox, sid = np.concatenate(vox).reshape(-1, 3), np.concatenate(sid)
    if vox.shape[0] == 0:
        return np.zeros((S, S)), np.zeros(S, np.int64)
    _, col = np.unique(vox, axis=0, return_inverse=True)
    col = col.reshape(-1)
    M = np.zeros((S, int(col.max()) + 1))
    M[sid, col] = 1.0
    inter = M @ M.T
    n = np.diag(inter).copy()
    union = n[:, None] + n[None, :] - inter
    both = (n[:, None] > 0) & (n[None, :] > 0)
    ratio = np.where(both, inter / np.where(both, union, 1.0), 0.0)
    assert (inter == np.round(inter)).all()
    return ratio, n.astype(np.int64)


SCALE_S = (255, 256, 257, 1025, 4096)       # submap counts on either side of one round of 256, five rounds, and SUB_MAX_S itself
SCALE_POOL = 1500                            # distinct voxels that every submap of a scale case draws from
SCALE_COUNTS = (40, 64, 100)                 # the sizes that most submaps tie in ...
SCALE_RARE = (0, 1, 256, 257)                # ... and the ones a few have: empty, one voxel, a full chunk of keys, a chunk and one


@functools.lru_cache(maxsize=None)
def overlap_scale_case(S):
    """S submaps of 1 to 4 frames whose unique-voxel counts are SCALE_COUNTS (thirds of the submaps tie in size: the intersect kernel's
    "smaller side, lower index on a tie" rule decides most pairs) with SCALE_RARE at about every 25th submap, all drawn from one pool of
    SCALE_POOL voxels, one point per voxel.  Posed except at S = 4096, where instead an uncovered frame lies before and after the submaps
    (rows of no submap on both sides of the sort by submap number, S + 1 = 4097 among them), each with a row far outside the grid."""
    rng = np.random.default_rng(5000 + S)
    posed = S != 4096
    pool = _lattice(rng, SCALE_POOL)
    counts = rng.choice(SCALE_COUNTS, S)
    rare = rng.permutation(S)[:max(8, S // 25)]
    counts[rare] = np.resize(SCALE_RARE, rare.shape[0])
    sets = [pool[rng.permutation(SCALE_POOL)[:n]] for n in counts]
    c = _build(rng, sets, 0.5 if posed else 2.0, posed, dup=1, frames_per_submap=[int(v) for v in rng.integers(1, 5, S)])
    if not posed:
        far = np.array([[1e7, -1e7, 1e7]], np.float32)
        lead, tail = [np.concatenate([far, ((pool[:n] + 0.5) * 2.0).astype(np.float32)]) for n in (300, 200)]
        c["points"] = np.concatenate([lead, c["points"], tail])
        c["cu"] = np.concatenate([[0], c["cu"] + lead.shape[0], [c["cu"][-1] + lead.shape[0] + tail.shape[0]]]).astype(np.int32)
        c["submap_frames"] = (c["submap_frames"] + 1).astype(np.int32)
    c["counts"] = counts
    return c


@functools.lru_cache(maxsize=None)
def overlap_scale_oracle(S):
    c = overlap_scale_case(S)
    return overlap_matrix_incidence(case_world(c), c["voxel_size"])


CONN_S, CONN_G = 1025, 1027                  # the real matrix of overlap_scale_case(1025); a group count that is no multiple of 4
CONN_LO, CONN_HI = 0.02, 1.0
CONN_BAD = (5, 514, 1026)                    # malformed groups: lengths 0, a member equal to S, length 0 -- the last group among them


def connectivity_scale_case():
    """-> ratio (the oracle's matrix of overlap_scale_case(CONN_S)), groups (CONN_G lists of 1 to 64 members drawn from all of [0, S), the
    lengths cycling), lo, hi, bad (the malformed groups' numbers).  The thresholds are such that both verdicts occur in at least a
    quarter of the well-formed groups (tests/test_submaps_host.py)."""
    ratio, _ = overlap_scale_oracle(CONN_S)
    rng = np.random.default_rng(31)
    groups = [[int(v) for v in rng.integers(0, CONN_S, 1 + (7 * g) % 64)] for g in range(CONN_G)]
    groups[CONN_BAD[0]] = []
    groups[CONN_BAD[1]] = groups[CONN_BAD[1]][:3] + [CONN_S]
    groups[CONN_BAD[2]] = []
    return ratio, groups, CONN_LO, CONN_HI, CONN_BAD


# ---- connectivity -----------------------------------------------------------------------------------------------------------------------
def groups_connected(ratio, group, lo, hi):
    n = len(group)
    parent = list(range(n))

    def find(x):
        if parent[x] != x:
            parent[x] = find(parent[x])
        return parent[x]
    for i in range(n):
        for j in range(i + 1, n):
            if lo <= ratio[group[i], group[j]] <= hi:
                pi, pj = find(i), find(j)
                if pi != pj:
                    parent[pi] = pj
    root = find(0)
    return all(find(i) == root for i in range(n))


def connectivity_case():
    """-> ratio (S,S), groups (list of lists), lo, hi.  S = 80 submaps; the ratios are multiples of 1/16 (exact in both arithmetics),
    lo = 1/4 and hi = 3/4, and the edges are: a chain 0-1-2-...-63 whose links alternate between ratio == lo and ratio == hi exactly,
    a second component 64-65-66 (ratio 1/2), 67 isolated; pairs 0-2 and 1-3 carry 1/8 and 7/8 (just outside)."""
    S = 80
    ratio = np.zeros((S, S))
    def edge(a, b, v):
        ratio[a, b] = ratio[b, a] = v
    for k in range(63):
        edge(k, k + 1, 0.25 if k % 2 == 0 else 0.75)
    edge(64, 65, 0.5); edge(65, 66, 0.5)
    edge(0, 2, 0.125); edge(1, 3, 0.875)
    np.fill_diagonal(ratio, 1.0)
    rng = np.random.default_rng(5)
    groups = [[5], [67], [0, 1], [1, 2], [0, 2], [1, 3], [0, 67], [0, 1, 2], [0, 2, 1], [2, 0, 1], [0, 1, 3], [64, 66, 65], [64, 66], [0, 1, 64, 65],
              list(range(64)), [int(v) for v in rng.permutation(64)], list(range(1, 64)) + [64], [int(v) for v in rng.permutation(63)] + [66],
              [3, 3, 4], [10, 12, 11, 13]]
    return ratio, groups, 0.25, 0.75


# ---- the end-to-end scene -----------------------------------------------------------------------------------------------------------------
E2E_VOXEL, E2E_PLANE_Z = 2.0, -1.75


def e2e_case():
    """A horizontal plane z = E2E_PLANE_Z (world) seen by a sensor that moves at constant velocity and is rolled and pitched: 6 sweeps of 2000
    points.  World x, y sit at voxel offsets in [0.1, 0.9] (so that the voxel of every point survives the fp32 chain).  Frame f > 0 is
    SKEWED in float64 by the inverse of the model: a point stamped s (s' = s - 0.5) is seen from pose_f D(s') with D(s') = [R(s'), s' T],
    i.e. p = R(s')^T (pose_f^-1 X - s' T).  Frame 0 has an identity rel_pose and is not skewed.
    -> points fp32, ts fp32, cu, rel_pose, pose, world (float64, the truth), submap_frames"""
    rng = np.random.default_rng(606)
    F, n = 6, 2000
    rel = np.eye(4)
    rel[:3, :3] = rotation([0.1, -0.05, 1.0], 0.05)
    rel[:3, 3] = [1.2, 0.05, 0.0]
    pose0 = np.eye(4)
    pose0[:3, :3] = rotation([1.0, 0.4, 0.0], 0.07)
    pose0[:3, 3] = [3.0, -2.0, 0.0]
    poses, rels, pts, tss, worlds = [pose0], [np.eye(4)], [], [], []
    for f in range(1, F):
        poses.append(poses[-1] @ rel)
        rels.append(rel.copy())
    for f in range(F):
        c = poses[f][:3, 3]
        vox = np.floor(c[:2] / E2E_VOXEL)[None] + rng.integers(-12, 13, size=(n, 2))
        xy = (vox + rng.uniform(0.1, 0.9, (n, 2))) * E2E_VOXEL
        X = np.concatenate([xy, np.full((n, 1), E2E_PLANE_Z)], axis=1)
        s = rng.uniform(0.0, 1.0, n).astype(np.float32)
        s[0], s[-1] = np.float32(1.0), np.float32(0.0)
        Xf = (X - poses[f][:3, 3]) @ poses[f][:3, :3]                        # pose_f^-1 X, rows
        if f == 0:
            p = Xf
        else:
            sp = s.astype(np.float64) - 0.5
            Rs = slerp_rotation(rel[:3, :3], sp)
            p = np.einsum("nji,nj->ni", Rs, Xf - sp[:, None] * rel[:3, 3][None])      # R(s')^T (.)
        pts.append(p.astype(np.float32)); tss.append(s); worlds.append(X)
    cu = (np.arange(F + 1) * n).astype(np.int32)
    return (np.concatenate(pts), np.concatenate(tss), cu, np.stack(rels), np.stack(poses), np.concatenate(worlds),
            np.array([0, 2, 4, 6], np.int32))
