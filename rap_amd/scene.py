"""Joint multi-view refinement of registered scenes on the device (``scene_refine.hip``, ``rap_scene_refine`` in include/rapflow.h).

Every other refinement tool of the package is pairwise (``icp_packed`` aligns one segment to one segment).  A scene of several views
polished pair by pair accumulates drift round a loop; refined view by view against the anchor it ignores every other overlap.  Here all
poses of a scene are the unknowns of ONE point-to-plane Gauss-Newton problem, with every overlapping ordered pair of views contributing.
The reference has no counterpart (it runs pytorch3d's pairwise ICP only, in its metrics): this is unpinned, and its yardstick is the fp64
restatement of the header in tests/scene_refine_oracle.py.

``refine_scene_packed`` is the packed form (ICP's row-vector convention, world = x @ R + T); ``refine_registration`` takes what
``fit_transformations`` returns (the sampler's convention, registered = cond @ R^T + t) and returns poses in that convention.
"""
from __future__ import annotations

import collections

import torch

from . import _lib
from .flow_model import _f32c, _require_cuda, workspace
from .icp import _check_loss, _part_offsets

SceneRefinement = collections.namedtuple("SceneRefinement", ["R", "T", "rmse", "iterations", "converged", "edge_rmse", "edge_count"])
SceneRefinement.__doc__ = """Result of a scene refinement, every field a device tensor: R (V,3,3) and T (V,3) with world = x @ R + T (row
vectors), rmse (S,) fp32, iterations (S,) int32, converged (S,) bool, and per edge of the last iteration its scene ran edge_rmse (E,)
fp32 (NaN for an ignored edge) and edge_count (E,) int32 (0 for an ignored edge)."""

MAX_VIEWS = 16
MAX_TABLE = 65535


def _check_knobs(max_iterations, max_correspondence_distance, max_views, row_budget):
    if int(max_iterations) <= 0:
        raise ValueError("max_iterations must be positive")
    if not 2 <= int(max_views) <= MAX_VIEWS:
        raise ValueError(f"max_views must lie in [2, {MAX_VIEWS}], got {max_views}")
    if max_correspondence_distance is not None and not float(max_correspondence_distance) > 0.0:
        raise ValueError("max_correspondence_distance must be positive (None: no gate)")
    if row_budget is not None and int(row_budget) <= 0:
        raise ValueError("row_budget must be positive (None: n_points * (max_views - 1))")


def _all_pairs(scene_seg, V, max_views):
    """every ordered pair of the first max_views views of every scene, (S * max_views * (max_views - 1), 2) int32, formed on the device;
    a pair that reaches past its scene's views is (-1, -1), which the call ignores"""
    device = scene_seg.device
    k = torch.arange(max_views * (max_views - 1), dtype=torch.int32, device=device)       # pair (i, j), j != i, in ascending (i, j)
    i, r = k // (max_views - 1), k % (max_views - 1)
    j = r + (r >= i).to(torch.int32)
    first, count = scene_seg[:, 0:1], scene_seg[:, 1:2].clamp(max=V)
    inside = (i[None, :] < count) & (j[None, :] < count)
    minus = torch.full_like(inside, -1, dtype=torch.int32)
    a = torch.where(inside, first + i[None, :], minus)
    b = torch.where(inside, first + j[None, :], minus)
    return torch.stack([a, b], dim=2).reshape(-1, 2).contiguous()


def refine_scene_packed(points, view_seg, scene_seg, R=None, T=None, edges=None, normals=None, fixed=None, max_iterations: int = 30,
                        relative_rmse_thr: float = 1e-6, max_correspondence_distance: float | None = None, max_views: int = MAX_VIEWS,
                        row_budget: int | None = None, loss: str | None = None, loss_scale: float | None = None) -> SceneRefinement:
    """Joint point-to-plane refinement of S scenes on packed clouds (``rap_scene_refine``: the algorithm, the rules for tables and the
    limits are in include/rapflow.h).  ``points`` (N,3) fp32, every view in its own frame; ``view_seg`` (V,2) int32 (start, len) rows,
    views must not overlap; ``scene_seg`` (S,2) int32 (first view, number of views); ``R`` (V,3,3) / ``T`` (V,3) the starting poses in
    ICP's convention world = x @ R + T (None: the identity); ``edges`` (E,2) int32 directed (source view, target view) pairs, None: all
    ordered pairs inside each scene, formed on the device (``S * max_views * (max_views - 1)`` rows); ``normals`` (N,3) per view in its
    own frame, None: ``estimate_normals_packed(points, view_seg, max_nn=20, radius=0.0, search="grid")``; ``fixed`` (V,) marks the views
    whose pose is not a variable, None: the first view of every scene (a scene without a fixed view is legal: the minimum-norm step
    resolves the gauge).  A scene with more than ``max_views`` (2 .. 16) views is left out (rmse NaN).  ``row_budget``: upper bound on
    the rows of the source views summed over the edges, None: ``N * (max_views - 1)``, which all ordered pairs cannot exceed.
    ``loss`` (``"huber"``, ``"cauchy"`` or ``"tukey"``) with ``loss_scale`` (its scale k > 0, in the units of the clouds) weights every
    residual by that robust loss (``rap_scene_refine_robust``: rmse and edge_rmse become sqrt(sum 2 rho / n), and a scene whose every
    weight is zero stops as one without pairs does).  No host synchronisation.  -> ``SceneRefinement``."""
    _check_knobs(max_iterations, max_correspondence_distance, max_views, row_budget)
    robust = _check_loss(loss, loss_scale)
    _require_cuda(points, "points")
    device = points.device
    P = _f32c(points.reshape(-1, 3))
    vs = view_seg.to(device=device, dtype=torch.int32).reshape(-1, 2).contiguous()
    ss = scene_seg.to(device=device, dtype=torch.int32).reshape(-1, 2).contiguous()
    V, S, mv = vs.shape[0], ss.shape[0], int(max_views)
    if V == 0 or S == 0 or V > MAX_TABLE:
        raise ValueError(f"view_seg and scene_seg must hold between 1 and {MAX_TABLE} views and at least one scene, got {V} and {S}")
    if edges is None:
        if S * mv * (mv - 1) > MAX_TABLE:
            raise ValueError(f"all ordered pairs of {S} scenes of up to {mv} views are more than {MAX_TABLE} edges: pass edges, or a smaller max_views")
        ed = _all_pairs(ss, V, mv)
    else:
        ed = edges.to(device=device, dtype=torch.int32).reshape(-1, 2).contiguous()
    E = ed.shape[0]
    if E == 0 or E > MAX_TABLE:
        raise ValueError(f"edges must hold between 1 and {MAX_TABLE} rows, got {E}")
    if P.shape[0] == 0:                                                  # the C ABI wants a non-empty array; every view clamps to nothing
        P = torch.zeros((1, 3), dtype=torch.float32, device=device)
        vs = torch.zeros_like(vs)
        normals = None
    N = P.shape[0]
    if normals is None:
        from .normals import estimate_normals_packed
        Pn = estimate_normals_packed(P, vs, max_nn=20, radius=0.0, search="grid")
    else:
        Pn = _f32c(normals.to(device).reshape(-1, 3))
        if Pn.shape[0] != N:
            raise ValueError(f"normals must have one row per row of points, got {Pn.shape[0]} for {N}")
    if (R is None) != (T is None):
        raise ValueError("R and T must be given together")
    iR = None if R is None else _f32c(R.to(device).reshape(V, 3, 3))
    iT = None if T is None else _f32c(T.to(device).reshape(V, 3))
    fx = None if fixed is None else fixed.to(device=device).reshape(V).ne(0).to(torch.uint8).contiguous()
    budget = N * (mv - 1) if row_budget is None else int(row_budget)
    gate = 0.0 if max_correspondence_distance is None else float(max_correspondence_distance)
    Ro = torch.empty((V, 3, 3), dtype=torch.float32, device=device)
    To = torch.empty((V, 3), dtype=torch.float32, device=device)
    rmse = torch.empty((S,), dtype=torch.float32, device=device)
    iters = torch.empty((S,), dtype=torch.int32, device=device)
    conv = torch.empty((S,), dtype=torch.uint8, device=device)
    ermse = torch.empty((E,), dtype=torch.float32, device=device)
    ecount = torch.empty((E,), dtype=torch.int32, device=device)
    lib = _lib.load()
    name = "rap_scene_refine" if robust is None else "rap_scene_refine_robust"      # the plain call stays on the entry point it always used
    nbytes = getattr(lib, name + "_workspace_bytes")(N, V, S, E, budget, mv)
    if nbytes == 0:
        raise ValueError(f"rap_scene_refine does not take these sizes: {N} points, {V} views, {S} scenes, {E} edges, row budget {budget}")
    ws = workspace(device, nbytes)
    with torch.cuda.device(device):
        rc = getattr(lib, name)(_lib.ptr(P), _lib.ptr(Pn), _lib.ptr(vs), V, N, _lib.ptr(ss), S, _lib.ptr(ed), E, budget, mv, _lib.ptr(fx),
                                  _lib.ptr(iR), _lib.ptr(iT), int(max_iterations), float(relative_rmse_thr), gate, _lib.ptr(Ro), _lib.ptr(To),
                                  _lib.ptr(rmse), _lib.ptr(iters), _lib.ptr(conv), _lib.ptr(ermse), _lib.ptr(ecount), *(robust or ()),
                                  _lib.ptr(ws), ws.numel(), _lib.current_stream(device))
    _lib.check(rc, name)
    return SceneRefinement(Ro, To, rmse, iters, conv.bool(), ermse, ecount)


def _registration_tables(pointclouds, points_per_part, anchor_parts, cu_seqlens_batch):
    """-> view_seg (B*P,2), scene_seg (B,2), fixed (B*P,) uint8 of a sampler batch: a view per part, a scene per sample; fixed = the
    flagged non-empty anchor parts, the first non-empty part where none is flagged.  Device arithmetic only."""
    device = pointclouds.device
    ppp = points_per_part.to(device=device, dtype=torch.int64)
    B, P = ppp.shape
    off, _ = _part_offsets(pointclouds, ppp, cu_seqlens_batch)
    view_seg = torch.stack([off, ppp], dim=2).reshape(B * P, 2).to(torch.int32)
    scene_seg = torch.stack([torch.arange(B, device=device) * P, torch.full((B,), P, device=device)], dim=1).to(torch.int32)
    nonempty = ppp > 0
    cand = torch.zeros_like(nonempty) if anchor_parts is None else anchor_parts.to(device=device).bool().reshape(B, P) & nonempty
    first = torch.zeros_like(nonempty)
    first.scatter_(1, nonempty.to(torch.int64).argmax(dim=1, keepdim=True), True)
    fixed = torch.where(cand.any(dim=1, keepdim=True), cand, first & nonempty)
    return view_seg, scene_seg, fixed.reshape(B * P).to(torch.uint8)


def refine_registration(pointclouds, points_per_part, rotations, translations, anchor_parts=None, cu_seqlens_batch=None, normals=None,
                        edges=None, max_iterations: int = 30, relative_rmse_thr: float = 1e-6,
                        max_correspondence_distance: float | None = None, max_views: int = MAX_VIEWS, row_budget: int | None = None,
                        loss: str | None = None, loss_scale: float | None = None):
    """Polish the poses of a registered batch on its own clouds: ``pointclouds`` (TP,3) packed (with ``cu_seqlens_batch``) or (B,N,3),
    the condition clouds, every part in its own frame; ``points_per_part`` (B,P); ``rotations`` (B,P,3,3) and ``translations`` (B,P,3)
    in the sampler's convention registered = cond @ R^T + t -- what ``fit_transformations`` returns and ``save_transformation_files``
    takes.  Every sample is one scene, every part one view (P <= ``max_views``, else the sample is left out: its poses come back
    unchanged and its rmse is NaN); the flagged non-empty parts of ``anchor_parts`` (B,P) stay fixed, the first non-empty part where
    none is flagged.  ``edges`` (E,2): directed pairs of view numbers ``b * P + p``, None: all ordered pairs of a sample.  The other
    knobs, ``loss`` and ``loss_scale`` included, are ``refine_scene_packed``'s.  -> (rotations (B,P,3,3), translations (B,P,3), rmse (B,)) in the same convention; empty parts
    keep their (zero) rows.  One ``rap_scene_refine`` (with a loss: ``rap_scene_refine_robust``) call, no host synchronisation."""
    _check_knobs(max_iterations, max_correspondence_distance, max_views, row_budget)
    _check_loss(loss, loss_scale)
    _require_cuda(pointclouds, "pointclouds")
    device = pointclouds.device
    B, P = points_per_part.shape
    view_seg, scene_seg, fixed = _registration_tables(pointclouds, points_per_part, anchor_parts, cu_seqlens_batch)
    R = _f32c(rotations.to(device).reshape(B * P, 3, 3)).transpose(1, 2)
    T = _f32c(translations.to(device).reshape(B * P, 3))
    sol = refine_scene_packed(pointclouds.reshape(-1, 3), view_seg, scene_seg, R, T, edges=edges, normals=normals, fixed=fixed,
                              max_iterations=max_iterations, relative_rmse_thr=relative_rmse_thr,
                              max_correspondence_distance=max_correspondence_distance, max_views=max_views, row_budget=row_budget,
                              loss=loss, loss_scale=loss_scale)
    return sol.R.transpose(1, 2).reshape(B, P, 3, 3).contiguous(), sol.T.reshape(B, P, 3), sol.rmse
