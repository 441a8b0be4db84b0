"""Inputs that the host and the GPU tests of the grid neighbour search (rap_amd/csrc/nn_grid.hip) share, and its brute-force yardstick.

The lattice case: Y is an 8 x 8 x 8 lattice of spacing 0.25 in a fixed random row order; X holds the midpoints of its edges (two
nearest rows at the same distance), the centres of its faces (four), the centres of its cells (eight), the lattice points themselves and
64 points up to three spacings outside the box on every side.  Every coordinate is a multiple of 1/8 below 4, so every squared distance
is exact in fp32 in any summation order: the first arg-min is a matter of the tie rule alone."""
import functools

import numpy as np

SIDE, SPACING = 8, 0.25
HALF = np.float32(SPACING / 2)


@functools.lru_cache(maxsize=None)
def lattice():
    """-> Y (512,3), X (n,3) fp32, kind (n,) of 'edge' / 'face' / 'cell' / 'point' / 'outside'"""
    rng = np.random.default_rng(2024)
    g = np.stack(np.meshgrid(*[np.arange(SIDE)] * 3, indexing="ij"), -1).reshape(-1, 3)
    Y = ((g - SIDE // 2) * SPACING).astype(np.float32)[rng.permutation(SIDE ** 3)]
    lo, hi = -SIDE // 2 * SPACING, (SIDE - 1 - SIDE // 2) * SPACING
    parts, kinds = [], []
    for name, offs in (("edge", [(1, 0, 0), (0, 1, 0), (0, 0, 1)]), ("face", [(1, 1, 0), (1, 0, 1), (0, 1, 1)]), ("cell", [(1, 1, 1)])):
        for o in offs:
            o = np.asarray(o)
            keep = ((g + o) < SIDE).all(axis=1)                         # the cell / face / edge that starts at g exists
            parts.append(((g[keep] - SIDE // 2) * SPACING + o * SPACING / 2).astype(np.float32))
            kinds += [name] * int(keep.sum())
    parts.append(((g - SIDE // 2) * SPACING).astype(np.float32))
    kinds += ["point"] * g.shape[0]
    out = rng.integers(round((lo - 3 * SPACING) * 8), round((hi + 3 * SPACING) * 8) + 1, (64, 3)).astype(np.float64) / 8
    for i in range(64):                                                 # every side of the box gets its share: axis i % 3, below or above
        a, up = i % 3, (i // 3) % 2
        step = rng.integers(1, 7) / 8                                   # 1/8 .. 3 spacings
        out[i, a] = hi + step if up else lo - step
    parts.append(out.astype(np.float32))
    kinds += ["outside"] * 64
    return Y, np.concatenate(parts), np.asarray(kinds)


def first_argmin(X, Y, dtype=np.float32):
    """-> (first arg-min over the rows of Y, its squared distance, how many rows share it) per row of X, direct differences in `dtype`"""
    X, Y = X.astype(dtype), Y.astype(dtype)
    d = X[:, None, :] - Y[None, :, :]
    D = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    i = D.argmin(axis=1)
    best = D[np.arange(D.shape[0]), i]
    return i, best, (D == best[:, None]).sum(axis=1)


def gated(idx, d2, gate):
    """the entry point's rule for max_distance: sqrtf(d2) <= gate in fp32, else -1 / inf"""
    keep = np.sqrt(d2.astype(np.float32)) <= np.float32(gate)
    return np.where(keep, idx, -1), np.where(keep, d2, np.float32(np.inf)).astype(np.float32)


def grid_cells(Y):
    """The cell of every row of Y under nn_grid.hip's sizing rule, restated: cubic cells of edge h = cbrt(volume / n), grown by a quarter
    at a time until the cell count is at most n + 8.  (The device takes the cube root in fp32 through exp2 / log2; the last bits of h do
    not matter to what this is used for.)  -> (cell (n,3) int, dims (3,), h)"""
    lo, hi = Y.min(axis=0), Y.max(axis=0)
    e = (hi - lo).astype(np.float32)
    h = np.float32(np.cbrt(np.prod(e.astype(np.float64)) / Y.shape[0]))
    while True:
        dims = np.floor(e / h).astype(np.int64) + 1
        if dims.prod() <= Y.shape[0] + 8:
            break
        h = np.float32(h * np.float32(1.25))
    cell = np.minimum(np.floor((Y - lo).astype(np.float32) / h).astype(np.int64), dims - 1)
    return cell, dims, float(h)
