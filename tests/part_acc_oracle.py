"""Yardsticks of the part-accuracy tests (no GPU, no SciPy, no reference): a float64 numpy chamfer matrix, the Python transcription of the
assignment SciPy makes, the fp32 error bound of the device's chamfer matrix, and the generated cases the GPU tests run (so that the host
tests can check their margins without a GPU).

``lsap`` restates scipy.optimize.linear_sum_assignment for square matrices (rectangular_lsap: the shortest augmenting path of Crouse
2016) line by line; tests/test_part_acc_host.py holds it to SciPy itself on the build machine, the GPU tests hold the device to it.
"""
from __future__ import annotations

import math

import numpy as np

THRESHOLD = 0.01
REL_MARGIN = 1e-3          # every |cd - threshold| >= REL_MARGIN * threshold: no fp32 rounding can flip a cost entry
U32 = 2.0 ** -24


# ---------------------------------------------------------------------------------------------
# chamfer matrix
# ---------------------------------------------------------------------------------------------
def _d2(x, y, dtype):
    d = x[:, None, :].astype(dtype) - y[None, :, :].astype(dtype)
    if dtype == np.float32:                      # the device's chain up to contraction: every operation rounded to fp32
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return (d * d).sum(-1)


def chamfer(x, y, dtype=np.float64) -> float:
    """pytorch3d's chamfer_distance(x, y, norm=2, point_reduction="mean", bidirectional): distances in `dtype`, means in float64"""
    d = _d2(x, y, dtype).astype(np.float64)
    return float(d.min(axis=1).mean() + d.min(axis=0).mean())


def part_slices(ppp_row, start):
    out, pos = [], int(start)
    for n in ppp_row:
        out.append((pos, pos + int(n)))
        pos += int(n)
    return out


def chamfer_matrix(gt, pred, ppp, cu, dtype=np.float64) -> np.ndarray:
    """(B,P,P) float64 indexed by part slot, NaN where either part is empty.  gt, pred (TP,3); ppp (B,P); cu (B+1,)"""
    B, P = ppp.shape
    cd = np.full((B, P, P), np.nan)
    for b in range(B):
        sl = part_slices(ppp[b], cu[b])
        for i, (a, e) in enumerate(sl):
            for j, (c, f) in enumerate(sl):
                if e > a and f > c:
                    cd[b, i, j] = chamfer(gt[a:e], pred[c:f], dtype)
    return cd


# fp32 bound of the device's cd against chamfer_matrix(..., float64) on the same fp32 inputs, as an error bound:
#   a difference of two fp32 numbers is rounded once (1 + u), u = 2^-24; its square once more: (1 + u)^3 per term at the most (a fused
#   term has one rounding less); the three non-negative terms are added with two roundings: |d2_fp32 / d2 - 1| <= (1 + u)^5 - 1;
#   min is monotone, so the minimum of values that are each within that factor is within that factor of the true minimum;
#   the means are formed in double (n * 2^-53: nothing at this scale) of non-negative numbers, and so is their sum: still (1 + u)^5;
#   the result is rounded to fp32 once: (1 + u)^6 - 1 < 6.000002 u.  CD_REL_BOUND = 7 u leaves the second-order terms and the
#   double-precision dust a whole unit.  A cd of exactly 0 (coincident points) stays exactly 0.
# Worst observed (not what the bound comes from): this module's fp32 evaluation against its float64 one over the generated cases 1.95 u
# (tests/test_part_acc_host.py prints it), the device against float64 over the same cases 3.74 u (tests/test_part_acc_gpu.py prints it).
CD_REL_BOUND = 7 * U32
assert (1 + U32) ** 6 - 1 < CD_REL_BOUND


def cd_within_bound(cd_dev, cd64) -> tuple[bool, float]:
    """-> (every entry within CD_REL_BOUND * cd64 and NaN exactly where cd64 is NaN, worst ratio |dev - cd64| / (u * cd64))"""
    cd_dev = np.asarray(cd_dev, dtype=np.float64)
    nan = np.isnan(cd64)
    if not np.array_equal(np.isnan(cd_dev), nan):
        return False, math.inf
    a, r = cd_dev[~nan], cd64[~nan]
    if a.size == 0:
        return True, 0.0
    err = np.abs(a - r)
    pos = r > 0
    worst = float((err[pos] / (U32 * r[pos])).max()) if pos.any() else 0.0
    return bool((err <= CD_REL_BOUND * r).all()), worst


# ---------------------------------------------------------------------------------------------
# assignment
# ---------------------------------------------------------------------------------------------
def lsap(cost) -> np.ndarray:
    """col4row of scipy.optimize.linear_sum_assignment(cost) for a square matrix (row_ind is arange(n))"""
    cost = np.asarray(cost, dtype=np.float64)
    n = cost.shape[0]
    assert cost.shape == (n, n)
    c = cost.tolist()
    inf = math.inf
    u, v = [0.0] * n, [0.0] * n
    path, col4row, row4col = [-1] * n, [-1] * n, [-1] * n
    for cur in range(n):
        min_val = 0.0
        remaining = [n - it - 1 for it in range(n)]
        num_remaining = n
        SR, SC, spc = [False] * n, [False] * n, [inf] * n
        sink, i = -1, cur
        while sink == -1:
            index, lowest = -1, inf
            SR[i] = True
            ci, ui = c[i], u[i]
            for it in range(num_remaining):
                j = remaining[it]
                r = min_val + ci[j] - ui - v[j]
                if r < spc[j]:
                    path[j] = i
                    spc[j] = r
                if spc[j] < lowest or (spc[j] == lowest and row4col[j] == -1):
                    lowest = spc[j]
                    index = it
            min_val = lowest
            if min_val == inf:
                raise ValueError("cost matrix is infeasible")
            j = remaining[index]
            if row4col[j] == -1:
                sink = j
            else:
                i = row4col[j]
            SC[j] = True
            num_remaining -= 1
            remaining[index] = remaining[num_remaining]
        u[cur] += min_val
        for k in range(n):
            if SR[k] and k != cur:
                u[k] += min_val - spc[col4row[k]]
        for k in range(n):
            if SC[k]:
                v[k] -= min_val - spc[k]
        j = sink
        while True:
            i = path[j]
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    return np.asarray(col4row, dtype=np.int64)


def part_acc_from_cd(cd, ppp, threshold=THRESHOLD):
    """the reference's steps after the chamfer matrix (metrics.py:126-158) with `lsap` in SciPy's place -> part_acc (B,) float32 (NaN for
    a sample without parts: the reference raises there), matched_part_ids (B,P) int64 in the reference's compacted indexing"""
    B, P = ppp.shape
    acc = np.zeros(B, dtype=np.float32)
    matched = np.zeros((B, P), dtype=np.int64)
    for b in range(B):
        idx = np.nonzero(ppp[b] > 0)[0]
        n = idx.size
        if n == 0:
            acc[b] = np.nan
            continue
        m = cd[b][np.ix_(idx, idx)]
        col = lsap((m >= threshold).astype(np.float64))
        acc[b] = np.float32(int((m[np.arange(n), col] < threshold).sum()) / n)
        matched[b, :n] = col
    return acc, matched


def margins_ok(cd, threshold=THRESHOLD) -> bool:
    v = cd[~np.isnan(cd)]
    return bool((np.abs(v - threshold) >= REL_MARGIN * threshold).all())


# ---------------------------------------------------------------------------------------------
# generated cases of the GPU tests: dict(gt, pred (TP,3) float32, ppp (B,P) int64, cu (B+1,) int32, threshold)
# ---------------------------------------------------------------------------------------------
TILE = 256


def _pack(samples, P, threshold=THRESHOLD):
    """samples: list of (sizes, gt parts, pred parts)"""
    gt = [p for s in samples for p in s[1]]
    pred = [p for s in samples for p in s[2]]
    ppp = np.asarray([list(s[0]) + [0] * (P - len(s[0])) for s in samples], dtype=np.int64)
    cu = np.zeros(len(samples) + 1, dtype=np.int32)
    cu[1:] = np.cumsum(ppp.sum(axis=1))
    z = np.zeros((0, 3), dtype=np.float32)
    return dict(gt=np.concatenate(gt + [z]).astype(np.float32), pred=np.concatenate(pred + [z]).astype(np.float32), ppp=ppp, cu=cu,
                threshold=threshold)


def blob_sample(sizes, rng, perm=None, spread=0.2, noise=1e-3, displaced=()):
    """parts are blobs of `spread` around centres 2 apart; pred part perm[k] lies where gt part k does (plus noise); a displaced pred part
    sits 0.5 away from its pose"""
    live = [k for k, n in enumerate(sizes) if n > 0]
    perm = dict(zip(live, live)) if perm is None else perm
    centre = {k: np.array([2.0 * k, 0.0, 0.0]) + rng.uniform(-0.1, 0.1, 3) for k in live}
    gt, pred = [None] * len(sizes), [None] * len(sizes)
    for k, n in enumerate(sizes):
        gt[k] = (centre[k] + rng.uniform(-spread, spread, (n, 3))) if n else np.zeros((0, 3))
    for k, n in enumerate(sizes):
        if not n:
            continue
        j = perm[k]                             # pred part j takes gt part k's place; equal sizes are not required for a chamfer
        m = sizes[j]
        src = gt[k][rng.integers(0, n, m)] if m != n else gt[k][rng.permutation(n)]
        pred[j] = src + rng.normal(0, noise, (m, 3)) + (np.array([0.0, 0.5, 0.0]) if j in displaced else 0.0)
    for k, n in enumerate(sizes):
        if not n:
            pred[k] = np.zeros((0, 3))
    return sizes, [g.astype(np.float32) for g in gt], [p.astype(np.float32) for p in pred]


# part lengths from {1, 2, 63, 64, 65, 255, 256, 257, 513}; positions are relative to the sample's start, the LDS tile is 256 candidates
EDGE_CASES = {
    # boundaries at 256 (on a tile edge), 255 (just before), 257 (just after); queries: one full tile, partial tiles
    "boundary-on-edge": [[256, 1, 255, 2]],                    # ends at 256 | 257 | 512 | 514
    "boundary-before-edge": [[255, 2, 255, 1]],                # ends at 255 | 257 | 512 | 513
    "boundary-after-edge": [[257, 255, 1, 64]],                # ends at 257 | 512 | 513 | 577
    "three-tiles": [[63, 513, 65, 1]],                         # the second part covers 63 .. 576: tiles 0, 1 and 2; query tiles 256 + 256 + 1
    "empties": [[0, 64, 0, 65, 0], [0, 0, 2, 0, 0], [1, 0, 0, 0, 63]],      # empty first, middle, last
    "mixed-batch": [[65, 63, 64], [257], [2, 1, 1, 2, 1]],     # B = 3 with 3, 1 and 5 parts
    "all-empty-sample": [[64, 2, 0], [0, 0, 0], [1, 255, 1]],
}
MANY_ITEMS_B = 360                                              # 360 samples x 3 parts of 1-2 points: 1080 work items > one round of 1024 blocks


def edge_case(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "many-items":
        rows = [[int(rng.integers(1, 3)) for _ in range(3)] for _ in range(MANY_ITEMS_B)]
    else:
        rows = EDGE_CASES[name]
    P = max(len(r) for r in rows)
    samples = []
    for r in rows:
        live = [k for k, n in enumerate(r) if n > 0]
        perm = dict(zip(live, live[1:] + live[:1])) if len(live) > 1 else None          # a rotation of the live parts
        samples.append(blob_sample(r, rng, perm=perm, displaced=(live[0],) if len(live) > 2 else ()))
    return _pack(samples, P)


EDGE_NAMES = list(EDGE_CASES) + ["many-items"]


def lattice_case(n, seed):
    """n parts of 1-2 points on the integer lattice (all coordinates exact in fp32), pred = gt parts permuted; about a third of the parts
    come in identical pairs (interchangeable: ties for the solver), a few pred parts are moved by one lattice step.  Every cd is exactly
    0 or >= 1; threshold 0.5."""
    rng = np.random.default_rng(seed)
    sizes = [int(rng.integers(1, 3)) for _ in range(n)]
    gt = []
    for k, m in enumerate(sizes):
        twin = k > 0 and rng.random() < 0.35 and sizes[k - 1] == m
        base = gt[k - 1] if twin else np.array([[3.0 * k, 3.0 * (k % 7), 0.0]] * m) + np.arange(m)[:, None] * np.array([0.0, 0.0, 1.0])
        gt.append(np.array(base, dtype=np.float32))
    # pred slot j gets gt part src[j]; slot sizes are fixed by points_per_part, so the permutation stays within equal sizes
    by_size = {}
    for k, m in enumerate(sizes):
        by_size.setdefault(m, []).append(k)
    src = np.arange(n)
    for m, ks in by_size.items():
        src[ks] = np.asarray(ks)[rng.permutation(len(ks))]
    pred = [gt[src[j]].copy() for j in range(n)]
    for j in rng.choice(n, size=max(1, n // 10), replace=False) if n > 2 else []:
        pred[j] = pred[j] + np.array([0.0, 0.0, 5.0], dtype=np.float32)          # fails against everything: cd >= 1
    return _pack([(sizes, gt, pred)], n, threshold=0.5)


LATTICE_SIZES = (1, 2, 63, 64, 65, 256)


def interchangeable_case(seed=5):
    """Producer -> consumer: B = 2 samples of P = 4 parts with equal point counts and no empty slot; the parts are the same shape at
    different poses, and the prediction places part k at the ground-truth pose of part perm[k].  -> the case plus the gt / pred poses."""
    rng = np.random.default_rng(seed)
    n, P = 40, 4
    shape = rng.uniform(-0.2, 0.2, (n, 3))
    samples, Rg, tg, Rp, tp, perms = [], [], [], [], [], []

    def rot(axis, deg):
        a = np.asarray(axis, dtype=np.float64); a /= np.linalg.norm(a)
        th = math.radians(deg)
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)
    for b in range(2):
        R = [rot(rng.normal(size=3), 40.0 + 50.0 * k) for k in range(P)]
        t = [np.array([1.5 * k, 0.5 * b, 0.0]) for k in range(P)]
        perm = [[1, 2, 3, 0], [2, 3, 0, 1]][b]
        gt = [shape @ R[k].T + t[k] for k in range(P)]
        pred = [shape @ R[perm[k]].T + t[perm[k]] for k in range(P)]
        samples.append(([n] * P, [g.astype(np.float32) for g in gt], [p.astype(np.float32) for p in pred]))
        Rg.append(R); tg.append(t); Rp.append([R[perm[k]] for k in range(P)]); tp.append([t[perm[k]] for k in range(P)]); perms.append(perm)
    case = _pack(samples, P)
    f = lambda x: np.asarray(x, dtype=np.float32)
    return case, f(Rg), f(tg), f(Rp), f(tp), np.asarray(perms, dtype=np.int64)
