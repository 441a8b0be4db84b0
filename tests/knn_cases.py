"""Inputs that the host and the GPU tests of the k-best walk over the grid index (rap_amd/csrc/nn_knn.hip) share, and its numpy yardstick.

Two kinds of input.  EXACT ones: every coordinate is a multiple of 0.25 with |value| <= 64, so every difference is a multiple of 0.25
below 128, every square a multiple of 1/16 below 2^14 and every three-term sum below 2^20 sixteenths -- exact in fp32 whatever the
contraction.  On these the k nearest rows are a matter of the (d2, row) tie rule alone, and ties are everywhere.  FLOAT ones (jittered
lattices, a surface patch) are used only where the yardstick itself proves that no neighbour set lies within SWEEP_GAP of another one
(the `gap` of icp_plane_oracle.estimate_normals; tests/test_knn_cases_host.py asserts it), because the device's fp32 distance and
numpy's differ by a rounding."""
import functools

import numpy as np

import icp_plane_oracle as P

KS = (1, 3, 12, 20, 21, 32)                        # list sizes: one slot, below / at / above a multiple of four, the 20 / 21 switch of outlier.hip, the most
OUTLIER_KS = (1, 2, 20, 21, 32)
TWO_CLUSTER_SETTINGS = ((12, 0.0), (32, 0.0), (20, 0.75))      # (max_nn, radius)


def knn(X, Y, k, radius=None):
    """The yardstick: for every row of X the k admissible rows of Y with the smallest (d2, row), ascending.  d2 in fp32 from direct
    differences; admissible: the row of Y and d2 finite, and sqrt(d2) <= radius in fp32 where a radius is given; a non-finite row of X
    admits nothing.  -> (idx (n,k) int32, -1 in unused slots; d2 (n,k) fp32, inf there; count (n,) int32)"""
    X, Y = np.asarray(X, np.float32), np.asarray(Y, np.float32)
    n, m = X.shape[0], Y.shape[0]
    idx = np.full((n, k), -1, np.int32)
    out = np.full((n, k), np.inf, np.float32)
    count = np.zeros(n, np.int32)
    fin = np.isfinite(Y).all(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(n):
            d = X[i] - Y
            d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
            ok = fin & np.isfinite(d2)
            if radius is not None and radius > 0:
                ok &= np.sqrt(d2) <= np.float32(radius)
            order = np.lexsort((np.arange(m), d2))
            take = order[ok[order]][:k]
            idx[i, :take.size], out[i, :take.size], count[i] = take, d2[take], take.size
    return idx, out, count


def _shuffled(rows, seed):
    rows = np.asarray(rows, np.float32)
    return rows[np.random.default_rng(seed).permutation(rows.shape[0])]


@functools.lru_cache(maxsize=None)
def exact_inputs():
    """name -> (n,3) fp32, every coordinate a multiple of 0.25 with |value| <= 64"""
    g = np.stack(np.meshgrid(*[np.arange(7)] * 3, indexing="ij"), -1).reshape(-1, 3)
    lattice = _shuffled(g * 0.75 - 2.25, 11)
    dup = lattice.copy()
    rng = np.random.default_rng(12)
    where = rng.permutation(343)[:103]                                   # 30 %: each becomes a copy of a row that stays
    dup[where] = dup[rng.choice(np.setdiff1d(np.arange(343), where), 103)]
    f = np.stack(np.meshgrid(np.arange(19), np.arange(19), indexing="ij"), -1).reshape(-1, 2)
    flat = _shuffled(np.concatenate([f * 0.5 - 4.0, np.full((361, 1), 1.25)], axis=1), 13)
    line = _shuffled(np.outer(np.arange(40), (0.25, 0.5, -0.25)) + (1.0, -3.0, 2.0), 14)
    return {"lattice7": lattice, "lattice7_dup": dup, "flat19": flat, "line40": line,
            "copies33": np.tile(np.asarray([[0.5, -1.25, 3.0]], np.float32), (33, 1)), "single": np.asarray([[2.0, 0.25, -0.75]], np.float32)}


@functools.lru_cache(maxsize=None)
def exact_queries():
    """Queries for X != Y against exact_inputs()['lattice7'] (the box [-2.25, 2.25]^3): 60 inside the box, 60 on its faces, 40 up to ten
    box lengths (45) outside it; multiples of 0.25 throughout"""
    rng = np.random.default_rng(15)
    inside = rng.integers(-9, 10, (60, 3)) * 0.25
    face = rng.integers(-9, 10, (60, 3)) * 0.25
    face[np.arange(60), np.arange(60) % 3] = np.where(np.arange(60) % 2, 2.25, -2.25)
    out = rng.integers(-9, 10, (40, 3)) * 0.25
    far = rng.integers(1, 181, 40) * 0.25                                # 0.25 .. 45 beyond the face
    out[np.arange(40), np.arange(40) % 3] = np.where(np.arange(40) % 2, 2.25 + far, -2.25 - far)
    out[:6] = [(47.25, 0, 0), (-47.25, 0.5, 0), (0, 47.25, -1), (47.25, 47.25, 47.25), (-47.25, 47.25, 2.25), (2.25, -47.25, -47.25)]
    X = np.concatenate([inside, face, out]).astype(np.float32)
    assert np.abs(X).max() <= 64 and (X * 4 == np.round(X * 4)).all()
    return X


@functools.lru_cache(maxsize=None)
def two_cluster():
    """Ten points and three hundred, forty units apart: most cells of the grid are empty, and the small cluster finds most of its
    neighbours in the far one"""
    a = P.jittered_lattice(2, 10, spacing=0.5)
    b = P.jittered_lattice(102, 300, spacing=0.5) + np.asarray((40, 0, 0), np.float32)
    pts = np.concatenate([a, b]).astype(np.float32)
    return pts[np.random.default_rng(2).permutation(310)]


def grid_cells(Y):
    """The cell of every finite row of Y under nn_grid.hip's sizing rule, restated for any number of axes with an
    extent: h = (volume / n)^(1 / axes), grown by a quarter at a time until no dimension exceeds 1024 and the cell count
    is at most n + 8; an axis without extent has one cell.  (The last bits of the device's h do not matter to what this is used for.)
    -> (cell (n,3) int, dims (3,), h)"""
    Y = np.asarray(Y, np.float32)
    Y = Y[np.isfinite(Y).all(axis=1)]
    n = Y.shape[0]
    lo, hi = Y.min(axis=0), Y.max(axis=0)
    e = (hi - lo).astype(np.float64)
    axes = int((e > 0).sum())
    if axes == 0:
        return np.zeros((n, 3), np.int64), np.ones(3, np.int64), 1.0
    h = (np.prod(np.where(e > 0, e, 1.0)) / n) ** (1.0 / axes)
    h = max(h, e.max() / 1023.5)
    while True:
        dims = np.where(e > 0, np.floor(e / h) + 1, 1).astype(np.int64)
        if dims.max() <= 1024 and dims.prod() <= n + 8:
            break
        h *= 1.25
    cell = np.minimum(np.floor((Y - lo).astype(np.float64) / h).astype(np.int64), dims - 1)
    return cell, dims, float(h)


def far_shell_ties(Y, k):
    """How many self-queries of the exact cloud Y have, at list size k, a tie across the end of the list whose WINNER lies in a farther
    Chebyshev shell of cells than the loser: rows a < b at the same d2 from the query, a the k-th neighbour, b the first one left out,
    shell(a) > shell(b).  A walk that stops as soon as its list is full and the bound reaches the worst distance (>= in place of >), or
    that breaks ties by arrival, returns b there."""
    cell, _, _ = grid_cells(Y)
    n = Y.shape[0]
    if n <= k:
        return 0
    hits = 0
    for i in range(n):
        d = Y[i] - Y
        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        order = np.lexsort((np.arange(n), d2))
        a, b = order[k - 1], order[k]
        if d2[a] == d2[b]:
            shell = np.abs(cell - cell[i]).max(axis=1)
            hits += bool(shell[a] > shell[b])
    return hits
