"""TEST INFRASTRUCTURE ONLY -- seeded inputs for the preprocessing-stage tests (MiniSpinNet, farthest point sampling, statistical
outlier removal) at realistic sizes and at constructed edges.  Shared by tests/test_oracle.py (CPU: the oracle is checked against
hand-built expectations on these inputs) and tests/test_preproc_scale_gpu.py (GPU: the kernels are checked against the oracle).
Nothing here reads the reference tree."""
from __future__ import annotations

import numpy as np
import torch

from . import spinnet_oracle as SO

SCALE_DES_R = 0.25
SCALE_K = 2 * 2048 + 404          # two full chunks of the default 2 048 keypoints and a partial one; 404 * 140 is not a multiple of 256


def spinnet_scale_case(seed: int = 0):
    """One surface-like cloud of 50 000 points below the sensor (z about -3: the patch normals have a definite side), with 4 500
    keypoints -> (pts (N,3) fp32, kpts (K,3) fp32, des_r, perm (N,) int64).
    44 000 points on a 12 x 12 sheet (about 60 per ball of radius 0.25) and 6 000 on a dense 0.9 x 0.9 tile of the same sheet (more than
    512 per ball away from its rim: the cap and the centre-on-the-512th-hit rule at scale).  3 900 keypoints are members of the sheet,
    150 members of the tile, 450 are NOT members of the cloud (sheet positions moved off the surface).  The share of the dense patches is
    kept small on purpose: every patch point is one more chance of a (voxel, point) pair within rounding of the voxel radius, and such
    keypoints are excluded from the comparison (spinnet_oracle ambiguity flag)."""
    g = torch.Generator().manual_seed(1000 + seed)
    height = lambda xy: -3.0 + 0.5 * torch.sin(0.8 * xy[:, 0]) + 0.3 * torch.cos(0.6 * xy[:, 1])
    xy_a = torch.rand(44000, 2, generator=g) * 12.0
    xy_b = torch.rand(6000, 2, generator=g) * 0.9 + torch.tensor([5.0, 6.0])
    xy = torch.cat([xy_a, xy_b])
    pts = torch.cat([xy, (height(xy) + 0.004 * torch.randn(50000, generator=g))[:, None]], dim=1).float()
    ia = torch.randperm(44000, generator=g)[:3900 + 450]
    ib = 44000 + torch.randperm(6000, generator=g)[:150]
    members = pts[torch.cat([ia[:3900], ib])]
    off = pts[ia[3900:]] + torch.cat([0.03 * torch.randn(450, 2, generator=g), 0.05 * (torch.rand(450, 1, generator=g) - 0.5)], dim=1)
    kpts = torch.cat([members, off.float()])[torch.randperm(SCALE_K, generator=g)].contiguous()
    perm = torch.randperm(50000, generator=g)
    return pts[torch.randperm(50000, generator=g)].contiguous(), kpts, SCALE_DES_R, perm


# ---------------------------------------------------------------------------------------------
# constructed patch edges: the number of in-radius points of every keypoint is known exactly
# ---------------------------------------------------------------------------------------------
EDGE_DES_R = 0.5
EDGE_COUNTS_FULL = (0, 1, 9, 10, 11, 511, 512, 513, 2200, 40)      # the last station holds 20 distinct points, each twice
EDGE_SIZES = {1: (1, 0), 3: (1, 0, 2), 1023: (511, 0, 10, 9), 1024: (512, 11, 1), 1025: (513, 10, 0), 4099: EDGE_COUNTS_FULL}


def _clear_of_voxel_shells(q64, vox64, margin=8.0):
    """True where no voxel centre has | |v - q|^2 - (0.8/3)^2 | <= margin * eps * (|v|^2 + |q|^2)"""
    d2 = ((vox64[None] - q64[:, None]) ** 2).sum(-1)
    scale = (vox64 ** 2).sum(-1)[None] + (q64 ** 2).sum(-1)[:, None]
    return ~((d2 - (0.8 / 3) ** 2).abs() <= margin * SO.AMBIGUITY_EPS * scale).any(dim=1)


def spinnet_edge_case(n_total: int, seed: int = 0):
    """Stations 10 units apart, one keypoint each; station s holds exactly EDGE_SIZES[n_total][s] points within des_r of its keypoint,
    all CLEARLY inside (|p - kpt| <= 0.75 r, in a ball flattened along z), and the rest of the cloud (up to n_total points) is clearly outside every ball
    (2 r ... 3 r from a keypoint).  For a station with >= 512 hits the 512th hit in scan order -- the patch centre -- sits 0.6 r away
    from the keypoint.  Inside points are drawn by rejection so that in the global-z mode no (voxel centre, patch point) pair is near
    the voxel radius either: the oracle flags nothing on these clouds.  The keypoint of the 513-station is a member of the cloud and
    the first point of its own ball in scan order (patch point 0).
    -> dict(pts, perm, kpts, des_r, counts, patches): `pts[perm]` is the scan order; `patches` (K, 512, 3) float64 is the expected
    UN-centred patch (the first 512 hits in scan order, then the keypoint), built here point by point."""
    counts = EDGE_SIZES[n_total]
    r = EDGE_DES_R
    g = torch.Generator().manual_seed(7000 + 13 * n_total + seed)
    vox64 = SO.voxel_centres().double()
    S = len(counts)
    kpts = (torch.arange(S, dtype=torch.float32)[:, None] * torch.tensor([10.0, 0.0, 0.0]) +
            torch.rand(S, 3, generator=g) * torch.tensor([1.0, 3.0, 1.0]) + torch.tensor([0.0, 0.0, -4.0])).float()

    def unit(n):
        v = torch.randn(n, 3, generator=g)
        return v / v.norm(dim=1, keepdim=True)

    flat = torch.tensor([1.0, 1.0, 0.3])        # surface-like balls: the patch normal of the local-reference-frame mode is well defined
    station_pts = []
    for s, c in enumerate(counts):
        k = kpts[s]
        if c == 0:
            station_pts.append(torch.zeros(0, 3))
            continue
        centre = k
        while c >= 512:                                                         # the 512th hit, when there is one
            centre = (k + 0.6 * r * unit(1)[0]).float()
            if bool(_clear_of_voxel_shells((k - centre).double()[None] / r, vox64)):
                break
        n_distinct = 20 if (c == 40 and n_total == 4099) else c
        got = []
        if c == 513:
            got.append(k[None].clone())                                         # the keypoint itself: patch point 0 of its own ball
        while sum(t.shape[0] for t in got) < n_distinct:
            cand = (k + unit(256) * (0.75 * r) * torch.rand(256, 1, generator=g) ** (1 / 3) * flat).float()
            cand = cand[((cand - k).double().norm(dim=1) <= 0.75 * r) & _clear_of_voxel_shells((cand - centre).double() / r, vox64)]
            got.append(cand)
        p = torch.cat(got)[:n_distinct]
        if n_distinct != c:
            p = torch.cat([p, p])[torch.randperm(c, generator=g)]               # exact duplicates, anywhere in the order
        if c >= 512:
            p[511] = centre
        station_pts.append(p)
    n_in = sum(counts)
    assert n_in <= n_total
    n_out = n_total - n_in
    out_station = torch.randint(0, S, (n_out,), generator=g)
    outside = (kpts[out_station] + unit(n_out) * r * (2.0 + torch.rand(n_out, 1, generator=g))).float()
    # random merge of the stations (and the outside points) that keeps every station's own order
    labels = torch.cat([torch.full((c,), s, dtype=torch.long) for s, c in enumerate(counts)] + [torch.full((n_out,), S, dtype=torch.long)])
    labels = labels[torch.randperm(n_total, generator=g)]
    scan = torch.zeros(n_total, 3)
    for s in range(S):
        scan[labels == s] = station_pts[s]
    scan[labels == S] = outside
    perm = torch.randperm(n_total, generator=g)
    pts = torch.zeros(n_total, 3)
    pts[perm] = scan                                                            # pts[perm] == scan
    patches = torch.zeros(S, 512, 3, dtype=torch.float64)
    for s, c in enumerate(counts):
        patches[s] = kpts[s].double()
        m = min(c, 512)
        patches[s, :m] = station_pts[s][:m].double()
    return {"pts": pts.float().contiguous(), "perm": perm, "kpts": kpts.contiguous(), "des_r": r, "counts": torch.tensor(counts),
            "patches": patches}


def stage1_by_loops(sd, patch_un, des_r):
    """Independent, loop-written stage 1 of MiniSpinNet (global-z mode) for ONE un-centred patch (512,3) float64: centre on the last slot,
    divide by des_r, per voxel the first 10 patch points within 0.8 / 3 (common.py:396-440 with its index-0 mask), de-rotation by the
    azimuth bin, the 3 -> 16 point MLP with eval BatchNorm + ReLU, max over the 10 slots -> x0 (16, 3, 7, 20) float64."""
    q = ((patch_un - patch_un[-1]) / des_r).numpy()
    vox = SO.voxel_centres().double().numpy()
    W = sd["pnt_layer.0.weight"].double().reshape(16, 3).numpy(); b = sd["pnt_layer.0.bias"].double().numpy()
    gam, bet = sd["pnt_layer.1.weight"].double().numpy(), sd["pnt_layer.1.bias"].double().numpy()
    rm, rv = sd["pnt_layer.1.running_mean"].double().numpy(), sd["pnt_layer.1.running_var"].double().numpy()
    out = np.zeros((420, 16))
    for v in range(420):
        hits = np.nonzero(((vox[v] - q) ** 2).sum(-1) < (0.8 / 3) ** 2)[0][:10]
        samples = np.zeros((10, 3))
        for s, j in enumerate(hits):
            samples[s] = q[j]
        if len(hits) and hits[0] == 0:
            samples[0] = 0.0
        ang = -(v % 20) * (2 * np.pi / 20)
        ca, sa = np.float64(np.float32(np.cos(ang))), np.float64(np.float32(np.sin(ang)))       # the reference rounds its table to fp32
        rot = np.stack([samples[:, 0] * ca - samples[:, 1] * sa, samples[:, 0] * sa + samples[:, 1] * ca, samples[:, 2]], axis=1)
        y = rot @ W.T + b
        y = (y - rm) / np.sqrt(rv + 1e-5) * gam + bet
        out[v] = np.maximum(y, 0.0).max(axis=0)
    return torch.from_numpy(out.T.reshape(16, 3, 7, 20).copy())


# ---------------------------------------------------------------------------------------------
# farthest point sampling: integer lattices (exact fp32 arithmetic, real ties)
# ---------------------------------------------------------------------------------------------
def lattice_cloud(n: int, seed: int, side: int = 1024):
    """n DISTINCT integer lattice points with coordinates in [0, side - 1], as fp32: every difference, square and three-term sum is
    below 2^22 and exact in fp32, with or without FMA contraction, so the index list of FPS is unique whatever the summation order."""
    rs = np.random.RandomState(seed)
    if side ** 3 <= 8 * n:
        keys = rs.permutation(side ** 3)[:n].astype(np.int64)                   # a small lattice: most of it is taken
    else:
        keys = rs.permutation(np.unique(rs.randint(0, side ** 3, size=int(n * 1.2) + 16, dtype=np.int64)))[:n]
    assert len(keys) == n
    return torch.from_numpy(np.stack([keys % side, (keys // side) % side, keys // (side * side)], axis=1).astype(np.float32))


def grid_cloud(nx: int, ny: int, nz: int, seed: int | None = None):
    """the full nx x ny x nz integer grid (most FPS picks are exact ties), optionally in a seeded random order"""
    gx, gy, gz = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    p = np.stack([gx.ravel(), gy.ravel(), gz.ravel()], axis=1).astype(np.float32)
    if seed is not None:
        p = p[np.random.RandomState(seed).permutation(len(p))]
    return torch.from_numpy(p)


# ---------------------------------------------------------------------------------------------
# statistical outlier removal
# ---------------------------------------------------------------------------------------------
def outlier_cloud(n: int, seed: int, noise_share: float = 0.03):
    """a wavy slab with floating noise above it, shuffled (the raw-scan shape of extract_sample_features.py's input)"""
    g = torch.Generator().manual_seed(500 + seed)
    n_noise = int(round(n * noise_share))
    n_surf = n - n_noise
    side = (n_surf / 55.0) ** 0.5                                               # about 55 points per unit area at every size
    surf = torch.rand(n_surf, 3, generator=g) * torch.tensor([side, side, 0.05])
    surf[:, 2] += 0.4 * torch.sin(surf[:, 0])
    noise = torch.rand(n_noise, 3, generator=g) * torch.tensor([side, side, 6.0]) + torch.tensor([0.0, 0.0, 1.0])
    return torch.cat([surf, noise])[torch.randperm(n, generator=g)].contiguous()
