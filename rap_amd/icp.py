"""Batched ICP on the device (point-to-point: ``icp.hip``; point-to-plane: ``icp_plane.hip``) and the two reference metrics that rest
on it.

The reference takes ICP from pytorch3d (``iterative_closest_point``; ``rectified_point_flow/eval/metrics.py:79`` and ``:261``) and runs
it one problem at a time, with a KNN launch, an SVD launch and a host read of the convergence test per iteration.  Here one ``rap_icp``
call takes a ragged batch of independent problems: every problem stops on its own, on the device, and the call never synchronises.

``iterative_closest_point`` is the fine-registration step a user applies to their own clouds; ``icp_packed`` is the form under it
(packed clouds plus segment tables); ``align_anchor`` (``metrics.py:50-90``) and ``compute_transform_errors_icp`` (the ``use_icp``
branch of ``metrics.py:165-303``) each make one such call for all samples.
"""
from __future__ import annotations

import collections

import torch

from . import _lib
from .flow_model import _f32c, _require_cuda, workspace

ICPSolution = collections.namedtuple("ICPSolution", ["converged", "rmse", "Xt", "R", "T", "iterations"])
ICPSolution.__doc__ = """Result of an ICP call, every field a device tensor: converged (K,) bool, rmse (K,), Xt (the moved X, in the
layout X was given in), R (K,3,3) and T (K,3) with ``Xt = X @ R + T`` (row vectors, det R = +1), iterations (K,) int32."""


SEARCHES = ("brute", "grid")
ESTIMATIONS = ("point_to_point", "point_to_plane")


def _check_search(search):
    if search not in SEARCHES:
        raise ValueError(f"search must be one of {SEARCHES}, got {search!r}")


def _check_estimation(estimation):
    if estimation not in ESTIMATIONS:
        raise ValueError(f"estimation must be one of {ESTIMATIONS}, got {estimation!r}")


LOSSES = {"huber": 1, "cauchy": 2, "tukey": 3}      # the RAP_LOSS_* codes of include/rapflow.h (0: none)


def _check_loss(loss, loss_scale):
    """-> (RAP_LOSS_* code, scale) of a robust call, or None for the plain one"""
    if loss is None:
        if loss_scale is not None:
            raise ValueError("loss_scale is only used with a loss")
        return None
    if loss not in LOSSES:
        raise ValueError(f"loss must be None or one of {tuple(LOSSES)}, got {loss!r}")
    if loss_scale is None:
        raise ValueError(f"loss={loss!r} needs a loss_scale, in the units of the clouds")
    k = float(loss_scale)
    if not (k > 0.0 and k < float("inf")):
        raise ValueError(f"loss_scale must be a positive finite number, got {loss_scale!r}")
    return LOSSES[loss], k


def icp_packed(X, x_seg, Y, y_seg, init_R=None, init_T=None, max_iterations: int = 100, relative_rmse_thr: float = 1e-6,
               max_correspondence_distance: float | None = None, return_Xt: bool = True, search: str = "brute",
               estimation: str = "point_to_point", y_normals=None, loss: str | None = None, loss_scale: float | None = None,
               return_weights: bool = False):
    """K problems on packed clouds: problem k aligns ``X[xs:xs+xn]`` to ``Y[ys:ys+yn]`` with ``(xs, xn) = x_seg[k]``,
    ``(ys, yn) = y_seg[k]``.  X (NX,3), Y (NY,3) fp32; x_seg, y_seg (K,2) int32 device tensors whose rows need not be contiguous or
    ordered (the x segments must not overlap); init_R (K,3,3) / init_T (K,3) or None.  Semantics, stopping rules and the treatment of
    empty problems: ``rap_icp`` in include/rapflow.h.  No host synchronisation; ``Xt`` (NX,3) starts as a copy of X, so rows outside
    every segment pass through unchanged.  ``search``: ``"brute"`` (every x against every y, ``rap_icp``) or ``"grid"`` (a uniform-grid
    index over Y built once per call, ``rap_icp_grid``); both give the same bits.

    ``estimation="point_to_plane"`` minimises the distance to the tangent plane of the neighbour instead (``rap_icp_plane`` /
    ``rap_icp_plane_grid``: a Gauss-Newton step per iteration; on scan surfaces a few iterations instead of dozens, because points may
    slide along the surface).  ``y_normals`` (NY,3): the normals of Y, rows with a zero or non-finite normal are left out of the fit;
    None: estimated in the same call from Y's own segments (``estimate_normals_packed`` with 20 neighbours, no radius, no viewpoint --
    the sign of a normal does not enter the residual; y segments may repeat, but segments that overlap without being equal can leave
    rows without a normal: pass ``y_normals`` then).  The reported rmse is then the point-to-plane residual of the transform that
    ENTERED the last iteration, one update behind the returned R, T.

    ``loss`` (``"huber"``, ``"cauchy"`` or ``"tukey"``) with ``loss_scale`` (its scale k > 0, in the units of the clouds) weights every
    point-to-plane residual by that robust loss in each Gauss-Newton step (``rap_icp_plane_robust`` / ``rap_icp_plane_grid_robust``:
    which pairs count is unchanged, the rmse becomes sqrt(sum 2 rho / n), and a problem whose every weight is zero stops as one without
    pairs does).  ``return_weights=True`` returns ``(ICPSolution, weights)``, weights (NX,) fp32: the weight every row of X had in the
    last iteration its problem ran -- 0 for a row that was gated out or matched a row without a usable normal, 1 for every counted
    row without a loss; rows outside every segment hold 0.  Both are point-to-plane only: weighting the Kabsch solve of
    ``estimation="point_to_point"`` is not built, and asking for it raises ValueError."""
    _check_search(search)
    _check_estimation(estimation)
    plane = estimation == "point_to_plane"
    robust = _check_loss(loss, loss_scale)
    if (robust is not None or return_weights) and not plane:
        raise ValueError("loss and return_weights need estimation='point_to_plane' (a weighted point-to-point solve is not built)")
    if y_normals is not None and not plane:
        raise ValueError("y_normals is only used by estimation='point_to_plane'")
    _require_cuda(X, "X")
    _require_cuda(Y, "Y")
    device = X.device
    X, Y = _f32c(X.reshape(-1, 3)), _f32c(Y.to(device).reshape(-1, 3))
    xs = x_seg.to(device=device, dtype=torch.int32).reshape(-1, 2).contiguous()
    ys = y_seg.to(device=device, dtype=torch.int32).reshape(-1, 2).contiguous()
    K = xs.shape[0]
    if K == 0 or ys.shape[0] != K:
        raise ValueError(f"x_seg and y_seg must hold the same positive number of (start, len) rows, got {xs.shape[0]} and {ys.shape[0]}")
    if int(max_iterations) <= 0:
        raise ValueError("max_iterations must be positive")
    empty_X = X if X.shape[0] == 0 and return_Xt else None
    n_x_rows = X.shape[0]
    if X.shape[0] == 0:                                                  # the C ABI wants non-empty arrays; every segment clamps to nothing
        X = torch.zeros((1, 3), dtype=torch.float32, device=device)
        xs = torch.zeros_like(xs)
        return_Xt = False
    Yn = None
    if plane and y_normals is not None:
        Yn = _f32c(y_normals.to(device).reshape(-1, 3))
        if Yn.shape[0] != Y.shape[0]:
            raise ValueError(f"y_normals must have one row per row of Y, got {Yn.shape[0]} for {Y.shape[0]}")
    if Y.shape[0] == 0:
        Y = torch.zeros((1, 3), dtype=torch.float32, device=device)
        ys = torch.zeros_like(ys)
        Yn = None
    if plane and Yn is None:
        from .normals import estimate_normals_packed
        Yn = estimate_normals_packed(Y, ys, max_nn=20, radius=0.0)
    NX, NY = X.shape[0], Y.shape[0]
    iR = None if init_R is None else _f32c(init_R.to(device).reshape(K, 3, 3))
    iT = None if init_T is None else _f32c(init_T.to(device).reshape(K, 3))
    R = torch.empty((K, 3, 3), dtype=torch.float32, device=device)
    T = torch.empty((K, 3), dtype=torch.float32, device=device)
    rmse = torch.empty((K,), dtype=torch.float32, device=device)
    iters = torch.empty((K,), dtype=torch.int32, device=device)
    conv = torch.empty((K,), dtype=torch.uint8, device=device)
    Xt = X.clone() if return_Xt else None
    gate = 0.0 if max_correspondence_distance is None else float(max_correspondence_distance)
    if max_correspondence_distance is not None and not gate > 0.0:
        raise ValueError("max_correspondence_distance must be positive (None: no gate)")
    lib = _lib.load()
    grid = search == "grid"
    weighted = robust is not None or return_weights                     # the plain call stays on the entry points it always used
    name = ("rap_icp_plane" if plane else "rap_icp") + ("_grid" if grid else "") + ("_robust" if weighted else "")
    fn, query = getattr(lib, name), getattr(lib, name + "_workspace_bytes")
    ws = workspace(device, query(NX, NY, K) if grid else query(NX, K))
    clouds = (_lib.ptr(X), _lib.ptr(xs), _lib.ptr(Y), _lib.ptr(ys)) + ((_lib.ptr(Yn),) if plane else ())
    weights = torch.zeros((NX,), dtype=torch.float32, device=device) if return_weights else None
    extra = (robust[0] if robust else 0, robust[1] if robust else 0.0, _lib.ptr(weights)) if weighted else ()
    with torch.cuda.device(device):
        rc = fn(*clouds, K, NX, NY, _lib.ptr(iR), _lib.ptr(iT), int(max_iterations),
                float(relative_rmse_thr), gate, _lib.ptr(R), _lib.ptr(T), _lib.ptr(rmse), _lib.ptr(iters), _lib.ptr(conv),
                _lib.ptr(Xt), *extra, _lib.ptr(ws), ws.numel(), _lib.current_stream(device))
    _lib.check(rc, name)
    sol = ICPSolution(conv.bool(), rmse, empty_X if Xt is None else Xt, R, T, iters)
    if return_weights:
        return sol, (weights[:0] if empty_X is not None or n_x_rows == 0 else weights)
    return sol


def nearest_neighbors_packed(X, x_seg, Y, y_seg, R=None, T=None, max_distance: float | None = None):
    """Exact nearest neighbours of K problems on packed clouds, through the uniform-grid index of ``rap_nearest_neighbors``: for every
    row i of ``X[xs:xs+xn]`` (moved by ``x @ R[k] + T[k]`` where R (K,3,3) and T (K,3) are given) the row of Y, within
    ``Y[ys:ys+yn]``, that is nearest to it -- the first one among equals, as a brute-force arg-min.  -> (idx (NX,) int32: the row in Y,
    d2 (NX,) fp32: the squared distance); -1 and inf where there is no neighbour within ``max_distance`` (None: no limit), where the
    y segment is empty, and for rows of X outside every segment.  No host synchronisation."""
    _require_cuda(X, "X")
    _require_cuda(Y, "Y")
    device = X.device
    X, Y = _f32c(X.reshape(-1, 3)), _f32c(Y.to(device).reshape(-1, 3))
    xs = x_seg.to(device=device, dtype=torch.int32).reshape(-1, 2).contiguous()
    ys = y_seg.to(device=device, dtype=torch.int32).reshape(-1, 2).contiguous()
    K = xs.shape[0]
    if K == 0 or ys.shape[0] != K:
        raise ValueError(f"x_seg and y_seg must hold the same positive number of (start, len) rows, got {xs.shape[0]} and {ys.shape[0]}")
    if (R is None) != (T is None):
        raise ValueError("R and T must be given together")
    gate = 0.0 if max_distance is None else float(max_distance)
    if max_distance is not None and not gate > 0.0:
        raise ValueError("max_distance must be positive (None: no limit)")
    NX = X.shape[0]
    idx = torch.full((NX,), -1, dtype=torch.int32, device=device)
    d2 = torch.full((NX,), float("inf"), dtype=torch.float32, device=device)
    if NX == 0:
        return idx, d2
    if Y.shape[0] == 0:                                                  # the C ABI wants non-empty arrays; every segment clamps to nothing
        Y = torch.zeros((1, 3), dtype=torch.float32, device=device)
        ys = torch.zeros_like(ys)
    NY = Y.shape[0]
    Rk = None if R is None else _f32c(R.to(device).reshape(K, 3, 3))
    Tk = None if T is None else _f32c(T.to(device).reshape(K, 3))
    lib = _lib.load()
    ws = workspace(device, lib.rap_nn_grid_workspace_bytes(NX, NY, K))
    with torch.cuda.device(device):
        rc = lib.rap_nearest_neighbors(_lib.ptr(X), _lib.ptr(xs), _lib.ptr(Y), _lib.ptr(ys), K, NX, NY, _lib.ptr(Rk), _lib.ptr(Tk), gate,
                                       _lib.ptr(idx), _lib.ptr(d2), _lib.ptr(ws), ws.numel(), _lib.current_stream(device))
    _lib.check(rc, "rap_nearest_neighbors")
    return idx, d2


def k_nearest_neighbors_packed(X, x_seg, Y, y_seg, k: int, max_distance: float | None = None):
    """The exact ``k`` (1 .. 32) nearest neighbours of K problems on packed clouds, through the uniform-grid index
    (``rap_k_nearest_neighbors``): for every row i of ``X[xs:xs+xn]`` the ``count[i] <= k`` rows of Y within ``Y[ys:ys+yn]`` (and within
    ``max_distance``; None: no limit) with the smallest (squared distance, row), in ascending order.  -> (idx (NX,k) int32: rows of
    Y, d2 (NX,k) fp32: squared distances, count (NX,) int32); unused slots hold -1 and inf, and rows of X outside every segment
    count 0.  Segments as ``nearest_neighbors_packed``, whose result ``k = 1`` reproduces bit for bit.  No host synchronisation."""
    _require_cuda(X, "X")
    _require_cuda(Y, "Y")
    device = X.device
    X, Y = _f32c(X.reshape(-1, 3)), _f32c(Y.to(device).reshape(-1, 3))
    xs = x_seg.to(device=device, dtype=torch.int32).reshape(-1, 2).contiguous()
    ys = y_seg.to(device=device, dtype=torch.int32).reshape(-1, 2).contiguous()
    K = xs.shape[0]
    if K == 0 or ys.shape[0] != K:
        raise ValueError(f"x_seg and y_seg must hold the same positive number of (start, len) rows, got {xs.shape[0]} and {ys.shape[0]}")
    if not 1 <= int(k) <= 32:
        raise ValueError(f"k must lie in [1, 32], got {k}")
    gate = 0.0 if max_distance is None else float(max_distance)
    if max_distance is not None and not gate > 0.0:
        raise ValueError("max_distance must be positive (None: no limit)")
    NX = X.shape[0]
    idx = torch.full((NX, int(k)), -1, dtype=torch.int32, device=device)
    d2 = torch.full((NX, int(k)), float("inf"), dtype=torch.float32, device=device)
    count = torch.zeros((NX,), dtype=torch.int32, device=device)
    if NX == 0:
        return idx, d2, count
    if Y.shape[0] == 0:                                                  # the C ABI wants non-empty arrays; every segment clamps to nothing
        Y = torch.zeros((1, 3), dtype=torch.float32, device=device)
        ys = torch.zeros_like(ys)
    NY = Y.shape[0]
    lib = _lib.load()
    ws = workspace(device, lib.rap_knn_workspace_bytes(NX, NY, K))
    with torch.cuda.device(device):
        rc = lib.rap_k_nearest_neighbors(_lib.ptr(X), _lib.ptr(xs), _lib.ptr(Y), _lib.ptr(ys), K, NX, NY, int(k), gate, _lib.ptr(idx),
                                         _lib.ptr(d2), _lib.ptr(count), _lib.ptr(ws), ws.numel(), _lib.current_stream(device))
    _lib.check(rc, "rap_k_nearest_neighbors")
    return idx, d2, count


def _lengths(lengths, K, N, device):
    if lengths is None:
        return torch.full((K,), N, dtype=torch.int32, device=device)
    return lengths.to(device=device, dtype=torch.int32).reshape(K).clamp(min=0, max=N)


def iterative_closest_point(X, Y, init_transform=None, max_iterations: int = 100, relative_rmse_thr: float = 1e-6,
                            max_correspondence_distance: float | None = None, x_lengths=None, y_lengths=None,
                            search: str = "brute", estimation: str = "point_to_point", Y_normals=None, loss: str | None = None,
                            loss_scale: float | None = None, return_weights: bool = False):
    """ICP of X onto Y (point-to-point by default): padded batches ``X (K,N,3)``, ``Y (K,M,3)`` with optional ``x_lengths`` /
    ``y_lengths`` (K,), or
    ``(N,3)`` / ``(M,3)`` for one problem.  ``init_transform = (R, T)`` with R (K,3,3) or (3,3), T (K,3) or (3,) in the row-vector
    convention ``Xt = X @ R + T``.  pytorch3d's algorithm and defaults (rigid, no scale estimate), except that every problem of the batch
    stops on its own and that a problem whose rmse reaches exactly 0 counts as converged.  ``max_correspondence_distance`` keeps only
    the points whose neighbour lies within that distance in each fit.  Returns an ``ICPSolution``; ``Xt`` has X's shape (padding rows
    unchanged).  One ``rap_icp`` call, no host synchronisation.  ``search="grid"`` finds the same neighbours through a uniform-grid
    index over Y (``rap_icp_grid``): the same bits, and far less work on large clouds.  ``estimation="point_to_plane"``: the
    point-to-plane estimator of ``icp_packed`` with ``Y_normals`` (K,M,3) or (M,3), estimated from Y where None.  ``loss`` /
    ``loss_scale`` / ``return_weights``: the robust losses of ``icp_packed`` (point-to-plane only; a weighted point-to-point solve is
    not built); with ``return_weights`` the result is ``(ICPSolution, weights)``, weights of X's shape without its last axis."""
    _check_search(search)
    _check_estimation(estimation)
    if (_check_loss(loss, loss_scale) is not None or return_weights) and estimation != "point_to_plane":
        raise ValueError("loss and return_weights need estimation='point_to_plane' (a weighted point-to-point solve is not built)")
    if Y_normals is not None and estimation != "point_to_plane":
        raise ValueError("Y_normals is only used by estimation='point_to_plane'")
    _require_cuda(X, "X")
    single = X.dim() == 2
    Xb = X.unsqueeze(0) if single else X
    Yb = Y.unsqueeze(0) if Y.dim() == 2 else Y
    if Xb.dim() != 3 or Yb.dim() != 3 or Xb.shape[-1] != 3 or Yb.shape[-1] != 3 or Xb.shape[0] != Yb.shape[0]:
        raise ValueError(f"X and Y must be (K,N,3) and (K,M,3) or (N,3) and (M,3), got {tuple(X.shape)} and {tuple(Y.shape)}")
    device = X.device
    K, N, M = Xb.shape[0], Xb.shape[1], Yb.shape[1]
    ar = torch.arange(K, dtype=torch.int32, device=device)
    x_seg = torch.stack([ar * N, _lengths(x_lengths, K, N, device)], dim=1)
    y_seg = torch.stack([ar * M, _lengths(y_lengths, K, M, device)], dim=1)
    iR = iT = None
    if init_transform is not None:
        iR, iT = init_transform[0], init_transform[1]
        iR = iR.to(device).reshape(-1, 3, 3).expand(K, 3, 3)
        iT = iT.to(device).reshape(-1, 3).expand(K, 3)
    if Y_normals is not None and tuple(Y_normals.shape) != tuple(Y.shape):
        raise ValueError(f"Y_normals must have Y's shape {tuple(Y.shape)}, got {tuple(Y_normals.shape)}")
    sol = icp_packed(Xb, x_seg, Yb, y_seg, iR, iT, max_iterations, relative_rmse_thr, max_correspondence_distance, search=search,
                     estimation=estimation, y_normals=Y_normals, loss=loss, loss_scale=loss_scale, return_weights=return_weights)
    if return_weights:
        sol, weights = sol
        return sol._replace(Xt=sol.Xt.reshape(X.shape)), weights.reshape(X.shape[:-1])
    return sol._replace(Xt=sol.Xt.reshape(X.shape))


def _apply_rows(P, R, T):
    """P[i] @ R[i] + T[i] for (n,3), (n,3,3), (n,3): elementwise fp32, so a row's result does not depend on how many rows there are"""
    return ((P[:, 0:1] * R[:, 0, :] + P[:, 1:2] * R[:, 1, :]) + P[:, 2:3] * R[:, 2, :]) + T


def _part_offsets(pointclouds, points_per_part, cu_seqlens_batch):
    """-> (B,P) int64 first row of every part in pointclouds.reshape(-1, 3), (B,) first row of every sample; device cumulative sums"""
    ppp = points_per_part.to(device=pointclouds.device, dtype=torch.int64)
    B = ppp.shape[0]
    if cu_seqlens_batch is not None:
        base = cu_seqlens_batch.to(device=ppp.device, dtype=torch.int64)[:B]
    elif pointclouds.dim() == 3:
        base = torch.arange(B, dtype=torch.int64, device=ppp.device) * pointclouds.shape[1]
    else:
        per = ppp.sum(dim=1)
        base = per.cumsum(0) - per
    return base[:, None] + ppp.cumsum(dim=1) - ppp, base


def align_anchor(pointclouds_gt, pointclouds_pred, points_per_part, anchor_parts, cu_seqlens_batch=None, search: str = "brute") -> torch.Tensor:
    """Reference signature (eval/metrics.py:50-90) plus ``cu_seqlens_batch`` for packed ``(TP,3)`` clouds -> the predicted cloud, every
    sample moved by the ICP alignment of its predicted anchor part (the first non-empty part flagged in ``anchor_parts``) onto the same
    part of the ground truth.  One ``rap_icp`` call for all samples, segment tables from cumulative sums on the device, no host sync.

    Three deliberate departures from the reference text:
      * metrics.py:73-80 -- the reference never advances ``pts_count`` in its first loop, so it runs ICP on the rows of the FIRST part
        whatever part is the anchor: right only when the anchor is the first non-empty part.  Here the anchor part's own offset is used.
      * metrics.py:87 -- the reference moves the cloud by ``pred @ R.T + T`` although pytorch3d's solution means ``Xt = X @ R + T``.
        Here the cloud is moved by ICP's own convention, ``pred @ R + T``.
      * metrics.py:72-87 -- a sample without an anchor keeps ``anchor_align_icp`` of the previous sample (a NameError for the first).
        Here such a sample is returned unchanged.

    ``search``: the neighbour search of the ICP call, ``"brute"`` or ``"grid"`` (``icp_packed``)."""
    _check_search(search)
    _require_cuda(pointclouds_pred, "pointclouds_pred")
    device = pointclouds_pred.device
    shape = pointclouds_pred.shape
    B, P = anchor_parts.shape
    ppp = points_per_part.to(device=device, dtype=torch.int64)
    off, base = _part_offsets(pointclouds_pred, ppp, cu_seqlens_batch)
    cand = anchor_parts.to(device=device).bool() & (ppp > 0)
    has = cand.any(dim=1)
    first = cand.to(torch.int64).argmax(dim=1, keepdim=True)               # the first flagged non-empty part (0 when there is none)
    start = off.gather(1, first).squeeze(1)
    length = torch.where(has, ppp.gather(1, first).squeeze(1), torch.zeros_like(start))
    seg = torch.stack([start, length], dim=1).to(torch.int32)
    pred = _f32c(pointclouds_pred.reshape(-1, 3))
    gt = _f32c(pointclouds_gt.to(device).reshape(-1, 3))
    sol = icp_packed(pred, seg, gt, seg, return_Xt=False, search=search)                  # an empty problem returns the identity: "unchanged"
    # every point of sample b moves by (R_b, T_b); rows outside every sample (padding of a (B,N,3) batch) stay
    TPn = pred.shape[0]
    n_b = ppp.sum(dim=1)
    rows = torch.arange(TPn, dtype=torch.int64, device=device)
    b_of = (torch.searchsorted(base.contiguous(), rows, right=True) - 1).clamp(min=0)
    inside = (rows >= base[b_of]) & (rows < base[b_of] + n_b[b_of]) & has[b_of]
    moved = _apply_rows(pred, sol.R[b_of], sol.T[b_of])
    return torch.where(inside[:, None], moved, pred).reshape(shape)


def compute_transform_errors_icp(pointclouds, pointclouds_gt, rotations_gt, translations_gt, rotations_pred, translations_pred,
                                 points_per_part, anchor_part, matched_part_ids=None, scale=None, cu_seqlens_batch=None,
                                 return_per_part: bool = False, search: str = "brute"):
    """``compute_transform_errors(..., use_icp=True)`` of the reference (eval/metrics.py:165-303, the branch at :257-265), with that
    function's argument list minus ``use_icp`` -> (rot_errors_mean (B,) in degrees, trans_errors_mean (B,)).  For every non-empty
    non-anchor part ICP aligns the ground-truth part onto ``cond @ R_pred^T + t_pred``; the rotation error is the angle of the ICP
    rotation (from its trace), the translation error ``|T| * scale``; means over those parts (NaN for a sample without one, as the
    reference's division).  ``rotations_gt`` / ``translations_gt`` are accepted for signature parity: this branch does not read them.
    ``matched_part_ids`` re-orders the predicted poses (:215-218).  One ``rap_icp`` call plus elementwise torch on the device, no host
    synchronisation.  ``return_per_part`` (an extension) also returns the (B,P) per-part errors.  ``search``: the neighbour search of
    the ICP call, ``"brute"`` or ``"grid"`` (``icp_packed``)."""
    _check_search(search)
    _require_cuda(pointclouds, "pointclouds")
    device = pointclouds.device
    B, P = points_per_part.shape
    ppp = points_per_part.to(device=device, dtype=torch.int64)
    Rp = _f32c(rotations_pred.to(device).reshape(B, P, 3, 3))
    tp = _f32c(translations_pred.to(device).reshape(B, P, 3))
    if matched_part_ids is not None:
        mid = matched_part_ids.to(device=device, dtype=torch.int64).clamp(min=0, max=P - 1)
        Rp = torch.gather(Rp, 1, mid[:, :, None, None].expand(B, P, 3, 3))
        tp = torch.gather(tp, 1, mid[:, :, None].expand(B, P, 3))
    sc = torch.ones((B,), dtype=torch.float32, device=device) if scale is None else _f32c(scale.to(device).reshape(B))
    off, _ = _part_offsets(pointclouds, ppp, cu_seqlens_batch)
    cond = _f32c(pointclouds.reshape(-1, 3))
    gt = _f32c(pointclouds_gt.to(device).reshape(-1, 3))
    TPn = cond.shape[0]
    # cond @ R_pred^T + t_pred per part (:260), in fp32 as the reference forms it: the part of every row from the part offsets
    rows = torch.arange(TPn, dtype=torch.int64, device=device)
    flat_off = off.reshape(-1)
    flat_len = ppp.reshape(-1)
    order = torch.argsort(flat_off, stable=True)                            # offsets ascend except over empty parts and padding
    pos = (torch.searchsorted(flat_off[order].contiguous(), rows, right=True) - 1).clamp(min=0)
    # among parts that share an offset (empty ones in front of a non-empty one) the stable sort puts the non-empty one last
    part = order[pos]
    inside = (rows >= flat_off[part]) & (rows < flat_off[part] + flat_len[part])
    Rrow, trow = Rp.reshape(B * P, 3, 3)[part], tp.reshape(B * P, 3)[part]
    moved = _apply_rows(cond, Rrow.transpose(1, 2), trow)
    moved = torch.where(inside[:, None], moved, cond)
    valid = (ppp != 0) & ~anchor_part.to(device=device).bool()
    seg = torch.stack([off, torch.where(valid, ppp, torch.zeros_like(ppp))], dim=2).reshape(B * P, 2).to(torch.int32)
    sol = icp_packed(gt, seg, moved, seg, return_Xt=False, search=search)
    R64 = sol.R.to(torch.float64)
    cos = (0.5 * (R64[:, 0, 0] + R64[:, 1, 1] + R64[:, 2, 2] - 1.0)).clamp(-1.0, 1.0)
    rot = torch.rad2deg(torch.acos(cos)).to(torch.float32).reshape(B, P)
    trans = (sol.T.to(torch.float64).norm(dim=1).reshape(B, P) * sc[:, None].to(torch.float64)).to(torch.float32)
    zero = torch.zeros_like(rot)
    rot, trans = torch.where(valid, rot, zero), torch.where(valid, trans, zero)
    n_parts = valid.sum(dim=1)
    rot_m, trans_m = rot.sum(dim=1) / n_parts, trans.sum(dim=1) / n_parts
    if return_per_part:
        return rot_m, trans_m, rot, trans
    return rot_m, trans_m
