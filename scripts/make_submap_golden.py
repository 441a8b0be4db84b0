"""Record tests/golden/submaps.npz: small inputs and what the reference's UNMODIFIED dataset_process/utils/{dataset_utils,submap_utils}.py
return for them -- create_submap_from_frames (fused clouds and normals), calculate_point_cloud_overlap_ratio_fast (pair ratios, below
its random-subsampling limit) and check_submap_validity (verdicts).  Needs the reference checkout (oracle.ref_loader.REFERENCE_ROOT);
only data is written, nothing of the reference's text.  deskewing is not recorded: it needs roma, which is not installed
(tests/submap_oracle.py says what stands in for it).

    python scripts/make_submap_golden.py
"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import submap_oracle as O                      # noqa: E402
from oracle import ref_loader                  # noqa: E402

VOXEL = 1.0
BOUNDARIES = [(0, 1), (2, 3), (4, 5), (6, 7), (1, 2), (3, 3)]           # (first, last) frame ids, the end inclusive
PAIRS = [(0, 1), (0, 4), (1, 4), (2, 3), (0, 3), (4, 4), (1, 5), (2, 5)]
# (selected submaps, min_overlap_ratio, max_overlap_ratio)
VERDICTS = [([0, 4, 1], 0.05, 1.0), ([0, 1], 0.05, 1.0), ([0, 1, 2, 3], 0.01, 1.0), ([0, 3], 0.01, 1.0), ([3, 2, 5, 1, 4, 0], 0.02, 0.9),
            ([0, 4], 0.0, 0.2), ([2], 0.5, 0.6), ([0, 4, 1], 0.3, 1.0), ([1, 5], 0.05, 0.5)]


def main():
    du = ref_loader.load_reference_dataset_utils()
    su = importlib.import_module("dataset_process.utils.submap_utils")      # by path, through the package stubs the loader registered
    rng = np.random.default_rng(2026)
    F, n = 8, 40
    points, normals, poses = [], [], []
    for f in range(F):
        M = np.eye(4)
        M[:3, :3] = O.rotation([0.05, -0.02, 1.0], 0.04 * f)
        M[:3, 3] = [1.5 * f, 0.1 * f, 0.02 * f]
        while True:                                                          # fp32 points whose voxels keep the margin rule
            p = np.stack([rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), rng.uniform(-1, 1, n)], axis=1).astype(np.float32)
            if O.voxel_margin(O.transform_points(p.astype(np.float64), M), VOXEL) >= 1e-4:
                break
        v = rng.normal(size=(n, 3))
        v = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
        v[f % n] = 0.0                                                       # a zero normal in every frame
        points.append(p); normals.append(v); poses.append(M)
    p64, n64 = [p.astype(np.float64) for p in points], [v.astype(np.float64) for v in normals]
    frame_ids = list(range(F))
    out = dict(points=np.stack(points), normals=np.stack(normals), poses=np.stack(poses), voxel_size=np.float64(VOXEL),
               boundaries=np.asarray(BOUNDARIES, np.int64), pairs=np.asarray(PAIRS, np.int64))
    for k, (a, b) in enumerate(BOUNDARIES):
        fp, fn = su.create_submap_from_frames(p64, poses, a, b - a + 1, n64)
        out[f"fused_points_{k}"], out[f"fused_normals_{k}"] = fp, fn
    subs = [su.create_submap_from_frames(p64, poses, a, b - a + 1)[0] for a, b in BOUNDARIES]
    out["pair_ratio"] = np.array([du.calculate_point_cloud_overlap_ratio_fast(subs[i], subs[j], voxel_size=VOXEL) for i, j in PAIRS])
    out["empty_ratio"] = np.float64(du.calculate_point_cloud_overlap_ratio_fast(np.zeros((0, 3)), subs[0], voxel_size=VOXEL))
    centers = [s.mean(axis=0) for s in subs]
    verdicts = []
    for sel, lo, hi in VERDICTS:
        verdicts.append(su.check_submap_validity(sel, BOUNDARIES, centers, p64, poses, frame_ids, 0.0, 1e9, lo, hi, "voxel", 0, VOXEL))
    out["verdict_groups"] = np.array([sel + [-1] * (8 - len(sel)) for sel, _, _ in VERDICTS], np.int64)
    out["verdict_lo_hi"] = np.array([[lo, hi] for _, lo, hi in VERDICTS])
    out["verdicts"] = np.array(verdicts, np.bool_)
    path = os.path.join(ROOT, "tests", "golden", "submaps.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; ratios", out["pair_ratio"], "verdicts", out["verdicts"].astype(int))


if __name__ == "__main__":
    main()
