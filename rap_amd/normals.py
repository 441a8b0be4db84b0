"""Surface normals on the device (``normals.hip``): the plane fit of every point's neighbourhood.

The reference estimates normals with Open3D on the host (``dataset_process/utils/dataset_utils.py:325-358``: hybrid search,
``radius=0.5``, ``max_nn=20``).  ``estimate_normals_packed`` is the batched form on packed clouds plus a segment table;
``estimate_point_normals`` has the reference's signature for one cloud.  The point-to-plane ICP of ``rap_amd.icp`` takes its target
normals from here when the caller has none.
"""
from __future__ import annotations

import torch

from . import _lib
from .flow_model import _f32c, _require_cuda, workspace


SEARCHES = ("brute", "grid")


def estimate_normals_packed(P, seg, max_nn: int = 20, radius: float = 0.5, viewpoint=None, return_eigenvalues: bool = False,
                            search: str = "brute"):
    """Normals of K clouds packed into ``P (N,3)`` fp32: cloud k is ``P[s:s+n]`` with ``(s, n) = seg[k]`` (``seg`` (K,2) int32 on the
    device; rows need not be contiguous or ordered and must not overlap).  For every row the neighbours are the ``max_nn`` (3 .. 32)
    nearest rows of its own cloud within ``radius`` (``radius <= 0`` or None: no limit), itself included, ties by row index; the normal is
    the unit eigenvector of the smallest eigenvalue of their covariance (fp64 on the device, rounded to fp32).  ``viewpoint`` (K,3) or
    (3,): normals point towards it; None: the component of largest magnitude is positive.  Rows with fewer than three neighbours (or a
    non-finite coordinate) get the zero vector; rows outside every segment are zero too.  -> normals (N,3), and with
    ``return_eigenvalues`` also the eigenvalues (N,3), ascending.  Semantics: ``rap_estimate_normals`` in include/rapflow.h.
    ``search="brute"`` looks at every row of the cloud for every row, which suits voxel-downsampled clouds; ``search="grid"``
    (``rap_estimate_normals_grid``) finds the same neighbours through a uniform-grid index built on the device, for
    clouds at full resolution -- the same normals to the last bits of the fp64 sums (both within 2e-6 of an fp64 plane fit).  No host
    synchronisation."""
    if search not in SEARCHES:
        raise ValueError(f"search must be one of {SEARCHES}, got {search!r}")
    _require_cuda(P, "P")
    device = P.device
    P = _f32c(P.reshape(-1, 3))
    sg = seg.to(device=device, dtype=torch.int32).reshape(-1, 2).contiguous()
    K, N = sg.shape[0], P.shape[0]
    if K == 0:
        raise ValueError("seg must hold at least one (start, len) row")
    if not 3 <= int(max_nn) <= 32:
        raise ValueError(f"max_nn must lie in [3, 32], got {max_nn}")
    r = 0.0 if radius is None else float(radius)
    if r != r:
        raise ValueError("radius must not be NaN")
    vp = None
    if viewpoint is not None:
        vp = _f32c(viewpoint.to(device).reshape(-1, 3).expand(K, 3))
    normals = torch.zeros((N, 3), dtype=torch.float32, device=device)
    eig = torch.zeros((N, 3), dtype=torch.float32, device=device) if return_eigenvalues else None
    if N > 0:
        lib = _lib.load()
        grid = search == "grid"
        ws = workspace(device, (lib.rap_normals_grid_workspace_bytes if grid else lib.rap_normals_workspace_bytes)(N, K))
        entry = lib.rap_estimate_normals_grid if grid else lib.rap_estimate_normals
        with torch.cuda.device(device):
            rc = entry(_lib.ptr(P), _lib.ptr(sg), K, N, int(max_nn), r, _lib.ptr(vp), _lib.ptr(normals), _lib.ptr(eig),
                       _lib.ptr(ws), ws.numel(), _lib.current_stream(device))
        _lib.check(rc, "rap_estimate_normals_grid" if grid else "rap_estimate_normals")
    return (normals, eig) if return_eigenvalues else normals


def estimate_point_normals(points, k_neighbors: int = 20, radius: float = 0.5, viewpoint=None, search: str = "brute"):
    """Reference signature (``estimate_point_normals``, dataset_process/utils/dataset_utils.py:325-358) for one ``(N,3)`` cloud on the
    device -> normals (N,3) fp32.  The neighbourhood is Open3D's hybrid search (the ``k_neighbors`` nearest within ``radius``, the point
    itself included) and the normal the same plane fit.  Two departures from the reference:
      * orientation: the reference propagates a consistent orientation over the tangent planes; here every normal is oriented on its own,
        towards ``viewpoint`` (3,) if given, else with its largest component positive.  A residual that uses ``n`` only as a direction
        (point-to-plane ICP) does not see the difference;
      * a point with fewer than three neighbours gets the zero vector, not Open3D's (0, 0, 1): ``rap_icp_plane`` skips a zero normal.
    ``search``: as ``estimate_normals_packed`` ("grid" for a cloud at full resolution)."""
    if search not in SEARCHES:
        raise ValueError(f"search must be one of {SEARCHES}, got {search!r}")
    if points.dim() != 2 or points.shape[-1] != 3:
        raise ValueError(f"points must be (N,3), got {tuple(points.shape)}")
    _require_cuda(points, "points")
    seg = torch.full((1, 2), points.shape[0], dtype=torch.int32, device=points.device)      # filled on the device: capturable
    seg[:, 0] = 0
    return estimate_normals_packed(points, seg, max_nn=k_neighbors, radius=radius, viewpoint=viewpoint, search=search)
