"""Fixture of the part-accuracy metric: tests/golden/part_acc.npz.

The yardstick is the reference's UNMODIFIED ``compute_part_acc`` (rectified_point_flow/eval/metrics.py:92-163), imported through
``oracle.ref_loader.load_reference()`` and called with SciPy's own ``linear_sum_assignment``.  Needs the reference mounted and SciPy;
writes arrays only.

pytorch3d is absent, so ``chamfer_distance`` in the reference metrics module's globals is bound to a float64 brute-force restatement of
its published result for the call the reference makes (x_lengths / y_lengths honoured, norm 2, point_reduction "mean",
batch_reduction None, both directions): chamfer PARITY IS UNPINNED for that one call, as for compute_cd and ICP; the padding, the pair
expansion, the thresholding, the assignment and the bookkeeping of matched_part_ids are the reference's own code.  The stand-in also
records the matrices it returns, which is how the fixture comes by ``cd``.

B = 4 samples of P = 6 part slots and 70 points each (the reference's (B,N,3) form needs equal totals), 1 to 70 points per part:
  0  three interchangeable parts of one shape, predicted at one another's poses, and a displaced part that fails the threshold;
  1  a trailing empty part, two parts of one shape at the SAME pose (a 2 x 2 block of zero costs: a tie the solver breaks) and one
     more copy elsewhere;
  2  interior empty parts, two swapped parts;
  3  one part.
Before writing, the script asserts that every |cd - threshold| >= 1e-3 * threshold, so that no fp32 rounding can flip a cost entry.

usage: python scripts/make_part_acc_golden.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

THRESHOLD = 0.01
REL_MARGIN = 1e-3
N = 70
SIZES = [[10, 10, 10, 20, 19, 1], [15, 15, 25, 15, 0, 0], [20, 0, 20, 0, 30, 0], [70, 0, 0, 0, 0, 0]]

RECORDED = []


def chamfer_stand_in(x, y, x_lengths=None, y_lengths=None, single_directional=False, norm=2, point_reduction="mean", batch_reduction="mean",
                     **kw):
    """pytorch3d.loss.chamfer.chamfer_distance as compute_part_acc calls it (metrics.py:140-148), float64 brute force; parity unpinned."""
    assert not single_directional and norm == 2 and point_reduction == "mean" and batch_reduction is None and not kw
    out = []
    for k in range(x.shape[0]):
        a, b = x[k, :int(x_lengths[k])].double(), y[k, :int(y_lengths[k])].double()
        d = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
        out.append(d.min(dim=1).values.mean() + d.min(dim=0).values.mean())
    cd = torch.stack(out)
    RECORDED.append(cd.clone())
    return cd, None


def build():
    rng = np.random.default_rng(20240611)
    gt, pred = np.zeros((len(SIZES), N, 3)), np.zeros((len(SIZES), N, 3))

    def put(b, sizes, gparts, pparts):
        assert sum(sizes) == N
        gt[b] = np.concatenate([g for g in gparts if len(g)])
        pred[b] = np.concatenate([p for p in pparts if len(p)])

    noise = lambda n: rng.normal(0, 1e-3, (n, 3))
    E = np.zeros((0, 3))
    # sample 0
    s = SIZES[0]
    shape = rng.uniform(-0.15, 0.15, (10, 3))
    off = [np.array([0.0, 0, 0]), np.array([1.0, 0, 0]), np.array([0.0, 1.0, 0])]
    g = [shape + off[0], shape + off[1], shape + off[2], rng.uniform(-0.15, 0.15, (20, 3)) + [2.0, 0, 0],
         rng.uniform(-0.15, 0.15, (19, 3)) + [0, 2.0, 0], np.array([[3.0, 3.0, 0.0]])]
    p = [shape[rng.permutation(10)] + off[1] + noise(10), shape[rng.permutation(10)] + off[2] + noise(10),
         shape[rng.permutation(10)] + off[0] + noise(10), g[3] + noise(20), g[4] + [0.0, 0.0, 0.4] + noise(19), g[5] + noise(1)]
    put(0, s, g, p)
    # sample 1
    s = SIZES[1]
    shape = rng.uniform(-0.15, 0.15, (15, 3))
    g = [shape, shape + 1e-3, rng.uniform(-0.15, 0.15, (25, 3)) + [0, 0, 2.0], shape + [1.5, 0, 0], E, E]
    p = [shape + [1.5, 0, 0] + noise(15), shape + noise(15), g[2] + noise(25), shape[rng.permutation(15)] + noise(15), E, E]
    put(1, s, g, p)
    # sample 2
    s = SIZES[2]
    shape = rng.uniform(-0.15, 0.15, (20, 3))
    g = [shape, E, shape + [0, 1.0, 0], E, rng.uniform(-0.15, 0.15, (30, 3)) + [1.0, 1.0, 1.0], E]
    p = [g[2] + noise(20), E, g[0] + noise(20), E, g[4] + noise(30), E]
    put(2, s, g, p)
    # sample 3
    g = [rng.uniform(-0.3, 0.3, (70, 3))] + [E] * 5
    p = [g[0] + noise(70)] + [E] * 5
    put(3, SIZES[3], g, p)
    return gt.astype(np.float32), pred.astype(np.float32), np.asarray(SIZES, dtype=np.int64)


def main():
    from oracle import ref_loader
    ref = ref_loader.load_reference()
    mod = ref.metrics
    import scipy
    import scipy.optimize
    assert mod.linear_sum_assignment is scipy.optimize.linear_sum_assignment
    mod.chamfer_distance = chamfer_stand_in
    gt, pred, ppp = build()
    B, P = ppp.shape
    acc, matched = mod.compute_part_acc(torch.from_numpy(gt), torch.from_numpy(pred), torch.from_numpy(ppp), threshold=THRESHOLD)
    assert len(RECORDED) == B
    cd = np.full((B, P, P), np.nan)
    for b in range(B):
        idx = np.nonzero(ppp[b] > 0)[0]
        cd[b][np.ix_(idx, idx)] = RECORDED[b].numpy().reshape(idx.size, idx.size)
    v = cd[~np.isnan(cd)]
    assert (np.abs(v - THRESHOLD) >= REL_MARGIN * THRESHOLD).all(), "a chamfer distance lies within the margin of the threshold"
    arrays = dict(pointclouds_gt=gt, pointclouds_pred=pred, points_per_part=ppp, threshold=np.float64(THRESHOLD),
                  part_acc=acc.numpy().astype(np.float32), matched_part_ids=matched.numpy().astype(np.int64), cd=cd,
                  scipy_version=np.asarray(scipy.__version__))
    path = os.path.join(ROOT, "tests", "golden", "part_acc.npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size < 100_000, f"{path}: {size} bytes"
    print(f"{path}: {size} bytes; SciPy {scipy.__version__}")
    print("part_acc", arrays["part_acc"])
    print("matched_part_ids\n", arrays["matched_part_ids"])
    below = np.where(np.isnan(cd), -1, (cd < THRESHOLD).astype(int))
    print("cd < threshold (-1: empty)\n", below)


if __name__ == "__main__":
    main()
