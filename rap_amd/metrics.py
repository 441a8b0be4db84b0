"""Host-side mirror of the reference's nearest-neighbour registration metrics.

``compute_cd`` and ``compute_correspondence_rmse`` keep the reference signatures and return structures
(``rectified_point_flow/eval/metrics.py:14-48`` and ``:386-469``); the N x M distance work runs in one LDS-tiled kernel
(``nn_metrics.hip``) instead of pytorch3d's chamfer op per object / a dense ``torch.cdist`` matrix.

``compute_pair_metrics`` is the batched form the evaluator needs (every scan pair of a packed batch in one sync-free call,
``pair_metrics.hip``); ``compute_transform_errors_direct`` (``:305-383``) and ``compute_approximate_transform_error``
(``:487-508``) complete the set ``Evaluator._compute_metrics`` imports.
"""
from __future__ import annotations

import torch

from . import _lib
from .flow_model import _f32c, _require_cuda, workspace


def compute_cd(pointclouds_gt, pointclouds_pred, cu_seqlens_batch, anchor_indices=None) -> torch.Tensor:
    """-> (B,) whole-object chamfer RMSE: sqrt(0.5 * (mean_i min_j |gt_i - pred_j|^2 + mean_j min_i |pred_j - gt_i|^2))."""
    gt = pointclouds_gt.reshape(-1, 3)
    pred = pointclouds_pred.reshape(-1, 3)
    _require_cuda(pred, "pointclouds_pred")
    device = pred.device
    gt, pred = _f32c(gt.to(device)), _f32c(pred)
    cu = cu_seqlens_batch.to(device=device, dtype=torch.int32).contiguous()
    B, TP = cu.shape[0] - 1, pred.shape[0]
    out = torch.empty((B,), dtype=torch.float32, device=device)
    lib = _lib.load()
    ws = workspace(device, lib.rap_nn_metrics_workspace_bytes(TP, B))
    with torch.cuda.device(device):
        rc = lib.rap_chamfer_rmse(_lib.ptr(gt), _lib.ptr(pred), _lib.ptr(cu), B, TP, _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                                  _lib.current_stream(device))
    _lib.check(rc, "rap_chamfer_rmse")
    return out


def compute_part_acc(pointclouds_gt, pointclouds_pred, points_per_part, threshold: float = 0.01, return_matched_part_ids: bool = True,
                     cu_seqlens_batch=None, return_cd_matrix: bool = False):
    """Reference signature and return structure (eval/metrics.py:92-163) -> ``part_acc (B,)`` fp32, or ``(part_acc, matched_part_ids
    (B,P) int64)``: the share of parts whose chamfer distance to the ground-truth part they are matched with is below ``threshold``,
    under the assignment ``scipy.optimize.linear_sum_assignment`` makes of the 0/1 matrix ``cd >= threshold`` -- the same permutation,
    computed on the device (``part_acc.hip``, ``assign.h``).  ``cd[b,i,j]`` is pytorch3d's bidirectional squared chamfer distance with
    mean reduction between ground-truth part i and predicted part j (no root, no factor 1/2).

    ``matched_part_ids`` keeps the reference's OWN indexing: row ``i`` and value ``j`` count the NON-EMPTY parts of the sample in order,
    not the part slots, and entries from ``n_parts`` on are 0.  ``compute_transform_errors*`` index slots with it, as the reference's do:
    the two agree only when no empty slot precedes a used one.  A sample without any non-empty part gets ``part_acc = NaN`` and zeros
    (the reference raises there).

    Clouds are ``(B,N,3)`` as in the reference, or packed ``(TP,3)`` with ``cu_seqlens_batch`` (B+1,) (an extension);
    ``return_cd_matrix`` (an extension) appends the ``(B,P,P)`` matrix, indexed by part slot, NaN where either part is empty.  One call
    for the whole batch, no host synchronisation (the reference copies every sample's matrix to the host).  P <= 256."""
    _require_cuda(pointclouds_pred, "pointclouds_pred")
    device = pointclouds_pred.device
    B, P = points_per_part.shape
    if cu_seqlens_batch is None:
        if pointclouds_pred.dim() != 3:
            raise ValueError("cu_seqlens_batch is required when the point clouds are packed (TP, 3)")
        if pointclouds_pred.shape[0] != B:
            raise ValueError(f"point clouds have batch size {pointclouds_pred.shape[0]}, points_per_part has {B}")
        N = pointclouds_pred.shape[1]
        cu = torch.arange(B + 1, dtype=torch.int32, device=device) * N
    else:
        cu = cu_seqlens_batch.to(device=device, dtype=torch.int32).contiguous()
        if cu.shape[0] != B + 1:
            raise ValueError(f"cu_seqlens_batch must have B + 1 = {B + 1} entries, got {cu.shape[0]}")
    gt, pred = _f32c(pointclouds_gt.to(device).reshape(-1, 3)), _f32c(pointclouds_pred.reshape(-1, 3))
    TP = pred.shape[0]
    if gt.shape[0] != TP:
        raise ValueError(f"pointclouds_gt has {gt.shape[0]} points, pointclouds_pred has {TP}")
    ppp = points_per_part.to(device=device, dtype=torch.int64).contiguous()
    acc = torch.empty((B,), dtype=torch.float32, device=device)
    matched = torch.empty((B, P), dtype=torch.int64, device=device)
    cd = torch.empty((B, P, P), dtype=torch.float32, device=device) if return_cd_matrix else None
    lib = _lib.load()
    ws = workspace(device, lib.rap_part_acc_workspace_bytes(TP, B, P))
    with torch.cuda.device(device):
        rc = lib.rap_part_acc(_lib.ptr(gt), _lib.ptr(pred), _lib.ptr(ppp), _lib.ptr(cu), B, P, TP, float(threshold), _lib.ptr(acc),
                              _lib.ptr(matched), _lib.ptr(cd), _lib.ptr(ws), ws.numel(), _lib.current_stream(device))
    _lib.check(rc, "rap_part_acc")
    out = (acc, matched) if return_matched_part_ids else (acc,)
    if return_cd_matrix:
        out = out + (cd,)
    return out if len(out) > 1 else out[0]


def compute_correspondence_rmse(source_gt, target_gt, source_pred, target_pred, distance_threshold: float = 0.1):
    """-> (rmse tensor, num_correspondences int, correspondence_ratio float), as the reference (one scan pair).  The two Python
    numbers of the return value are the reference's API and cost the one host read-back this function makes."""
    def _2d(pc, name):                                                  # metrics.py:414-423
        if pc.dim() == 1:
            pc = pc.unsqueeze(0)
        if pc.dim() == 3:
            if pc.shape[0] != 1:
                raise ValueError(f"This function only works for a single pair of point clouds. {name} has shape (B, N, 3) with B > 1.")
            pc = pc.squeeze(0)
        return pc
    sg, tg, sp, tp = (_2d(x, n) for x, n in ((source_gt, "source_gt"), (target_gt, "target_gt"), (source_pred, "source_pred"),
                                              (target_pred, "target_pred")))
    _require_cuda(sg, "source_gt")
    device = sg.device
    Ns, Nt = sg.shape[0], tg.shape[0]
    if Ns == 0 or Nt == 0:
        return torch.tensor(float("inf"), device=device), 0, 0.0          # :433-434
    if sp.shape[0] != Ns:
        raise ValueError(f"source_pred must have the same number of points as source_gt. Got {sp.shape[0]} vs {Ns}.")
    if tp.shape[0] != Nt:
        raise ValueError(f"target_pred must have the same number of points as target_gt. Got {tp.shape[0]} vs {Nt}.")
    sg, tg, sp, tp = _f32c(sg), _f32c(tg.to(device)), _f32c(sp.to(device)), _f32c(tp.to(device))
    out = torch.empty((3,), dtype=torch.float32, device=device)
    lib = _lib.load()
    ws = workspace(device, lib.rap_nn_metrics_workspace_bytes(Ns, 1))
    with torch.cuda.device(device):
        rc = lib.rap_correspondence_rmse(_lib.ptr(sg), _lib.ptr(tg), _lib.ptr(sp), _lib.ptr(tp), Ns, Nt, float(distance_threshold),
                                         _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.current_stream(device))
    _lib.check(rc, "rap_correspondence_rmse")
    host = out.cpu()
    n = int(host[1].item())
    if n == 0:
        return torch.tensor(float("inf"), device=device), 0, 0.0          # :453-454
    return out[0], n, n / Ns


def compute_transform_errors(pointclouds, pointclouds_gt, rotations_gt, translations_gt, rotations_pred, translations_pred, points_per_part,
                             anchor_part, matched_part_ids=None, scale=None, cu_seqlens_batch=None, use_icp: bool = False,
                             return_per_part: bool = False):
    """Reference signature (eval/metrics.py:165-303) -> (rot_errors_mean (B,) in degrees, trans_errors_mean (B,)); the RRE / RTE of the
    registration task.  ``use_icp=False`` only: the ICP refinement is pytorch3d's and, in the reference's own words, "for the interchangable
    case, which does not apply for point cloud registration tasks" (:264).  ``pointclouds`` / ``pointclouds_gt`` / ``cu_seqlens_batch`` are
    accepted for signature parity -- the no-ICP branch reads only the poses.  One kernel, no host synchronisation (the reference loops
    B x P with a ``.nonzero()`` per sample).  ``return_per_part`` (an extension) also returns the (B,P) per-part errors."""
    if use_icp:
        raise NotImplementedError("use_icp=True (pytorch3d iterative_closest_point) is not part of the registration path (metrics.py:264)")
    _require_cuda(rotations_pred, "rotations_pred")
    device = rotations_pred.device
    B, P = points_per_part.shape
    Rg, tg = _f32c(rotations_gt.to(device).reshape(B, P, 3, 3)), _f32c(translations_gt.to(device).reshape(B, P, 3))
    Rp, tp = _f32c(rotations_pred.reshape(B, P, 3, 3)), _f32c(translations_pred.to(device).reshape(B, P, 3))
    ppp = points_per_part.to(device=device, dtype=torch.int64).contiguous()
    anc = anchor_part.to(device=device, dtype=torch.uint8).contiguous()
    mid = None if matched_part_ids is None else matched_part_ids.to(device=device, dtype=torch.int64).contiguous()
    sc = None if scale is None else _f32c(scale.to(device).reshape(B))
    rot_pp = torch.empty((B, P), dtype=torch.float32, device=device); trans_pp = torch.empty_like(rot_pp)
    rot_m = torch.empty((B,), dtype=torch.float32, device=device); trans_m = torch.empty_like(rot_m)
    lib = _lib.load()
    with torch.cuda.device(device):
        rc = lib.rap_transform_errors(_lib.ptr(Rg), _lib.ptr(tg), _lib.ptr(Rp), _lib.ptr(tp), _lib.ptr(ppp), _lib.ptr(anc), _lib.ptr(mid),
                                      _lib.ptr(sc), B, P, _lib.ptr(rot_pp), _lib.ptr(trans_pp), _lib.ptr(rot_m), _lib.ptr(trans_m),
                                      _lib.current_stream(device))
    _lib.check(rc, "rap_transform_errors")
    if return_per_part:
        return rot_m, trans_m, rot_pp, trans_pp
    return rot_m, trans_m


def compute_transform_errors_direct(rotations_gt, translations_gt, rotations_pred, translations_pred, points_per_part,
                                    matched_part_ids=None, scale=None, return_per_part: bool = False):
    """Reference signature (eval/metrics.py:305-383) -> (rot_errors_mean (B,) in degrees, trans_errors_mean (B,)): the pose errors WITHOUT
    an anchor frame -- ``delta_R = R_gt^T R_pred``, ``delta_t = (t_pred - t_gt) * scale``, mean over every non-empty part (NaN for a
    sample without one).  One kernel, no host synchronisation.  ``return_per_part`` (an extension) also returns the (B,P) errors."""
    _require_cuda(rotations_pred, "rotations_pred")
    device = rotations_pred.device
    B, P = points_per_part.shape
    Rg, tg = _f32c(rotations_gt.to(device).reshape(B, P, 3, 3)), _f32c(translations_gt.to(device).reshape(B, P, 3))
    Rp, tp = _f32c(rotations_pred.reshape(B, P, 3, 3)), _f32c(translations_pred.to(device).reshape(B, P, 3))
    ppp = points_per_part.to(device=device, dtype=torch.int64).contiguous()
    mid = None if matched_part_ids is None else matched_part_ids.to(device=device, dtype=torch.int64).contiguous()
    sc = None if scale is None else _f32c(scale.to(device).reshape(B))
    rot_pp = torch.empty((B, P), dtype=torch.float32, device=device); trans_pp = torch.empty_like(rot_pp)
    rot_m = torch.empty((B,), dtype=torch.float32, device=device); trans_m = torch.empty_like(rot_m)
    lib = _lib.load()
    with torch.cuda.device(device):
        rc = lib.rap_transform_errors_direct(_lib.ptr(Rg), _lib.ptr(tg), _lib.ptr(Rp), _lib.ptr(tp), _lib.ptr(ppp), _lib.ptr(mid),
                                             _lib.ptr(sc), B, P, _lib.ptr(rot_pp), _lib.ptr(trans_pp), _lib.ptr(rot_m), _lib.ptr(trans_m),
                                             _lib.current_stream(device))
    _lib.check(rc, "rap_transform_errors_direct")
    if return_per_part:
        return rot_m, trans_m, rot_pp, trans_pp
    return rot_m, trans_m


def compute_pair_metrics(data: dict, cloud, rotations_pred=None, translations_pred=None, distance_threshold: float = 0.05) -> torch.Tensor:
    """The scan-pair block of ``Evaluator._compute_metrics`` (eval/evaluator.py:124-248) for ALL pairs of a packed batch with P = 2
    -> (B,4) fp32 on the device: ``{correspondence rmse (m), correspondence ratio, transform error rmse (m), number of correspondences}``.

    With predicted poses ("transformed", the evaluator's default) ``cloud`` is ``data["pointclouds"]`` and the compared clouds are the
    inputs moved by the predicted poses; without them ("direct") ``cloud`` is the predicted cloud and the transform error is ``inf``.
    ``data`` needs "pointclouds_gt", "points_per_part", "cu_seqlens_batch", "scales", "rotations", "translations".  Three launches, no
    host synchronisation when the inputs are on the device in their final dtypes (int64 / int32 / fp32)."""
    ppp = data["points_per_part"]
    if ppp.dim() != 2 or ppp.shape[1] != 2:
        raise ValueError(f"compute_pair_metrics needs scan pairs, points_per_part of shape (B, 2); got {tuple(ppp.shape)}")
    if (rotations_pred is None) != (translations_pred is None):
        raise ValueError("rotations_pred and translations_pred must be given together")
    cloud = cloud.reshape(-1, 3)
    _require_cuda(cloud, "cloud")
    device = cloud.device
    gt = data["pointclouds_gt"].reshape(-1, 3)
    _require_cuda(gt, "pointclouds_gt")
    B, TP = ppp.shape[0], cloud.shape[0]
    if gt.shape[0] != TP:
        raise ValueError(f"pointclouds_gt has {gt.shape[0]} points, cloud has {TP}")
    gt, cloud = _f32c(gt), _f32c(cloud)
    ppp = ppp.to(device=device, dtype=torch.int64).contiguous()
    cu = data["cu_seqlens_batch"].to(device=device, dtype=torch.int32).contiguous()
    if cu.shape[0] != B + 1:
        raise ValueError(f"cu_seqlens_batch must have B + 1 = {B + 1} entries, got {cu.shape[0]}")
    sc = _f32c(data["scales"].to(device).reshape(B))
    Rg, tg = _f32c(data["rotations"].to(device).reshape(B, 2, 3, 3)), _f32c(data["translations"].to(device).reshape(B, 2, 3))
    Rp = None if rotations_pred is None else _f32c(rotations_pred.to(device).reshape(B, 2, 3, 3))
    tp = None if translations_pred is None else _f32c(translations_pred.to(device).reshape(B, 2, 3))
    out = torch.empty((B, 4), dtype=torch.float32, device=device)
    lib = _lib.load()
    ws = workspace(device, lib.rap_pair_metrics_workspace_bytes(TP, B))
    with torch.cuda.device(device):
        rc = lib.rap_pair_metrics(_lib.ptr(gt), _lib.ptr(cloud), _lib.ptr(ppp), _lib.ptr(cu), _lib.ptr(sc), _lib.ptr(Rg), _lib.ptr(tg),
                                  _lib.ptr(Rp), _lib.ptr(tp), B, TP, float(distance_threshold), _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                                  _lib.current_stream(device))
    _lib.check(rc, "rap_pair_metrics")
    return out


def compute_approximate_transform_error(rotation_error, translation_error, covariance=None) -> torch.Tensor:
    """Reference eval/metrics.py:487-508 for device tensors ``(...,3,3)`` / ``(...,3)`` -> ``(...)``: ``er^T er`` with
    ``er = [t, q_x, q_y, q_z]``, q the unit quaternion of the rotation error -- like the reference a SQUARED error, the evaluator takes
    the root.  Only the identity covariance (or ``None``), the one the evaluator passes, is supported.  ``|q_xyz|^2 = (3 - tr R) / 4``
    for a rotation matrix; evaluated in float64 (in fp32 the trace form loses small angles).  Elementwise torch on the device, no sync;
    ``compute_pair_metrics`` computes the same quantity inside its finish kernel."""
    if covariance is not None:
        import numpy as np
        cov = np.asarray(covariance.detach().cpu() if isinstance(covariance, torch.Tensor) else covariance, dtype=np.float64)
        if cov.shape != (6, 6) or not np.array_equal(cov, np.eye(6)):
            raise NotImplementedError("compute_approximate_transform_error supports the identity covariance only (the one the "
                                      "evaluator passes, evaluator.py:151)")
    _require_cuda(rotation_error, "rotation_error")
    R = rotation_error.to(torch.float64)
    t = translation_error.to(device=R.device, dtype=torch.float64)
    tr = R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2]
    q2 = ((3.0 - tr) * 0.25).clamp(min=0.0, max=1.0)
    return ((t * t).sum(dim=-1) + q2).to(torch.float32)
