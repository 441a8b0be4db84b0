"""Surface normals on the device (``normals.hip``): the plane fit of every point's neighbourhood.

The reference estimates normals with Open3D on the host (``dataset_process/utils/dataset_utils.py:325-358``: hybrid search,
``radius=0.5``, ``max_nn=20``).  ``estimate_normals_packed`` is the batched form on packed clouds plus a segment table;
``estimate_point_normals`` has the reference's signature for one cloud.  The point-to-plane ICP of ``rap_amd.icp`` takes its target
normals from here when the caller has none.  ``orient_normals_packed`` (``orient.hip``) gives existing normals one consistent orientation
per connected component of the k-NN graph, the reference's ``orient_normals_consistent_tangent_plane`` step.
"""
from __future__ import annotations

import torch

from . import _lib
from .flow_model import _f32c, _require_cuda, workspace


SEARCHES = ("brute", "grid")
ORIENTATIONS = ("independent", "consistent")


def orient_normals_packed(P, normals, seg, k: int = 15, viewpoint=None, return_components: bool = False):
    """A consistent orientation for the ``normals (N,3)`` of K clouds packed into ``P (N,3)`` with the segment table ``seg`` (K,2) of
    ``estimate_normals_packed``: the signs that the minimum spanning forest of the Riemannian graph propagates (``rap_orient_normals`` in
    include/rapflow.h).  The graph joins every row to its ``k`` (2 .. 32) nearest rows of the same cloud, itself
    counted; an edge weighs ``1 - |n_i . n_j|``; along a tree edge the sign follows ``n_i . n_j >= 0``.  Every connected component is
    oriented from its own seed, its highest point (largest z, the lowest row among equals), whose normal points up, or towards
    ``viewpoint`` (K,3) or (3,) if given.  -> a new (N,3) tensor: every row is the input row or its exact negation (rows with a non-finite
    coordinate or a non-finite or zero normal, and rows outside every segment, are returned as they came); with ``return_components`` also
    ``components`` (N,) int32, the row of the seed of each row's component (-1 for the rows just named).  No host synchronisation."""
    _require_cuda(P, "P")
    device = P.device
    P = _f32c(P.reshape(-1, 3))
    out = normals.to(device=device, dtype=torch.float32).reshape(-1, 3).clone(memory_format=torch.contiguous_format)
    sg = seg.to(device=device, dtype=torch.int32).reshape(-1, 2).contiguous()
    K, N = sg.shape[0], P.shape[0]
    if K == 0:
        raise ValueError("seg must hold at least one (start, len) row")
    if out.shape[0] != N:
        raise ValueError(f"normals must have the {N} rows of P, got {out.shape[0]}")
    if not 2 <= int(k) <= 32:
        raise ValueError(f"k must lie in [2, 32], got {k}")
    vp = None
    if viewpoint is not None:
        vp = _f32c(viewpoint.to(device).reshape(-1, 3).expand(K, 3))
    comp = torch.full((N,), -1, dtype=torch.int32, device=device) if return_components else None
    if N > 0:
        lib = _lib.load()
        ws = workspace(device, lib.rap_orient_normals_workspace_bytes(N, K))
        with torch.cuda.device(device):
            rc = lib.rap_orient_normals(_lib.ptr(P), _lib.ptr(sg), K, N, int(k), _lib.ptr(vp), _lib.ptr(out), _lib.ptr(comp), _lib.ptr(ws),
                                        ws.numel(), _lib.current_stream(device))
        _lib.check(rc, "rap_orient_normals")
    return (out, comp) if return_components else out


def estimate_normals_packed(P, seg, max_nn: int = 20, radius: float = 0.5, viewpoint=None, return_eigenvalues: bool = False,
                            search: str = "brute", orientation: str = "independent", orient_k=None):
    """Normals of K clouds packed into ``P (N,3)`` fp32: cloud k is ``P[s:s+n]`` with ``(s, n) = seg[k]`` (``seg`` (K,2) int32 on the
    device; rows need not be contiguous or ordered and must not overlap).  For every row the neighbours are the ``max_nn`` (3 .. 32)
    nearest rows of its own cloud within ``radius`` (``radius <= 0`` or None: no limit), itself included, ties by row index; the normal is
    the unit eigenvector of the smallest eigenvalue of their covariance (fp64 on the device, rounded to fp32).  ``viewpoint`` (K,3) or
    (3,): normals point towards it; None: the component of largest magnitude is positive.  Rows with fewer than three neighbours (or a
    non-finite coordinate) get the zero vector; rows outside every segment are zero too.  -> normals (N,3), and with
    ``return_eigenvalues`` also the eigenvalues (N,3), ascending.  Semantics: ``rap_estimate_normals`` in include/rapflow.h.
    ``search="brute"`` looks at every row of the cloud for every row, which suits voxel-downsampled clouds; ``search="grid"``
    (``rap_estimate_normals_grid``) finds the same neighbours through a uniform-grid index built on the device, for
    clouds at full resolution -- the same normals to the last bits of the fp64 sums (both within 2e-6 of an fp64 plane fit).
    ``orientation="independent"`` (the default) leaves every normal with the sign rule above; ``"consistent"`` then runs
    ``orient_normals_packed`` over the result with ``k = orient_k or max_nn`` (the reference passes its ``k_neighbors`` to both steps) and
    the same ``viewpoint``, which then decides the sign of each component's seed only.  No host synchronisation."""
    if search not in SEARCHES:
        raise ValueError(f"search must be one of {SEARCHES}, got {search!r}")
    if orientation not in ORIENTATIONS:
        raise ValueError(f"orientation must be one of {ORIENTATIONS}, got {orientation!r}")
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
    if orientation == "consistent":
        normals = orient_normals_packed(P, normals, sg, k=int(orient_k or max_nn), viewpoint=vp)
    return (normals, eig) if return_eigenvalues else normals


def estimate_point_normals(points, k_neighbors: int = 20, radius: float = 0.5, viewpoint=None, search: str = "brute",
                           orientation: str = "independent", orient_k=None):
    """Reference signature (``estimate_point_normals``, dataset_process/utils/dataset_utils.py:325-358) for one ``(N,3)`` cloud on the
    device -> normals (N,3) fp32.  The neighbourhood is Open3D's hybrid search (the ``k_neighbors`` nearest within ``radius``, the point
    itself included) and the normal the same plane fit.  Orientation: the reference propagates a consistent orientation over the
    tangent planes (Open3D's ``orient_normals_consistent_tangent_plane(k=k_neighbors)``); ``orientation="consistent"`` is that step on the
    device (``orient_normals_packed`` with ``k = orient_k or k_neighbors``, at most 32).  The default, ``"independent"``, orients every
    normal on its own, towards ``viewpoint`` (3,) if given, else with its largest component positive: enough for a residual that uses
    ``n`` only as a direction (point-to-plane ICP), and half of a closed surface inside out for anything that reads the sign.  Two
    departures from the reference remain:
      * the consistent orientation spans the k-NN graph alone: Open3D adds the edges of a Euclidean minimum spanning tree, which joins
        everything; here each connected component of the k-NN graph is oriented from its own highest point (``orient_normals_packed``
        returns the components);
      * a point with fewer than three neighbours gets the zero vector, not Open3D's (0, 0, 1): ``rap_icp_plane`` skips a zero normal, and
        the orientation leaves such a row out of the graph.
    ``search``: as ``estimate_normals_packed`` ("grid" for a cloud at full resolution)."""
    if search not in SEARCHES:
        raise ValueError(f"search must be one of {SEARCHES}, got {search!r}")
    if orientation not in ORIENTATIONS:
        raise ValueError(f"orientation must be one of {ORIENTATIONS}, got {orientation!r}")
    if points.dim() != 2 or points.shape[-1] != 3:
        raise ValueError(f"points must be (N,3), got {tuple(points.shape)}")
    _require_cuda(points, "points")
    seg = torch.full((1, 2), points.shape[0], dtype=torch.int32, device=points.device)      # filled on the device: capturable
    seg[:, 0] = 0
    return estimate_normals_packed(points, seg, max_nn=k_neighbors, radius=radius, viewpoint=viewpoint, search=search, orientation=orientation,
                                   orient_k=orient_k)
