"""Host-side mirror of the reference's evaluator: the metrics table and the transform writer.

``Evaluator.compute_metrics`` is ``Evaluator._compute_metrics`` (``rectified_point_flow/eval/evaluator.py:30-250``): the same keys in
the same order, every value a (B,) fp32 device tensor, and no host synchronisation -- the reference loops over the B pairs with
``.cpu()`` / ``.item()`` in the loop, here the pair block is one call (``metrics.compute_pair_metrics``).

``save_transformation_files`` writes the same ``*_transform.txt`` files, names and number format as
``Evaluator._save_transformation_files`` (``rectified_point_flow/eval/evaluator.py:383-490``; consumed by
``demo.py:1332-1342``); the 4x4 matrices of a whole batch come from one kernel (``rap_relative_transforms``) instead of a
per-part numpy loop, and one device-to-host copy.
"""
from __future__ import annotations

from pathlib import Path

import torch

from . import _lib
from .flow_model import _f32c, _require_cuda
from .metrics import compute_cd, compute_pair_metrics, compute_transform_errors
from .selection import compute_rigidity_rmse


def compute_relative_transforms(rotations_pred, translations_pred, rotations_gt, translations_gt, scales, points_per_part,
                                global_rotation=None, global_translation=None) -> torch.Tensor:
    """-> (B,P,4,4) fp32: predicted pose relative to the GT pose in metres (x inv(global frame) if given); zero blocks for
    parts without points."""
    _require_cuda(rotations_pred, "rotations_pred")
    device = rotations_pred.device
    B, P = points_per_part.shape
    Rp, tp = _f32c(rotations_pred), _f32c(translations_pred.to(device))
    Rg, tg = _f32c(rotations_gt.to(device)), _f32c(translations_gt.to(device))
    sc = _f32c(scales.to(device))
    ppp = points_per_part.to(device=device, dtype=torch.int64).contiguous()
    if (global_rotation is None) != (global_translation is None):
        raise ValueError("global_rotation and global_translation must be given together")
    Gr = None if global_rotation is None else _f32c(global_rotation.to(device)).reshape(B, 3, 3)
    Gt = None if global_translation is None else _f32c(global_translation.to(device)).reshape(B, 3)
    out = torch.empty((B, P, 4, 4), dtype=torch.float32, device=device)
    lib = _lib.load()
    with torch.cuda.device(device):
        rc = lib.rap_relative_transforms(_lib.ptr(Rp), _lib.ptr(tp), _lib.ptr(Rg), _lib.ptr(tg), _lib.ptr(sc), _lib.ptr(ppp), B, P,
                                         _lib.ptr(Gr), _lib.ptr(Gt), _lib.ptr(out), _lib.current_stream(device))
    _lib.check(rc, "rap_relative_transforms")
    return out


def _suffix(generation_idx) -> str:
    if isinstance(generation_idx, str):                                     # evaluator.py:427-432
        return generation_idx if generation_idx.startswith("generation") else f"generation_{generation_idx}"
    return f"generation{generation_idx:02d}"                                # :434


def save_transformation_files(data: dict, sample_dir, dataset_name: str, sample_indices, generation_idx, rotations_pred,
                              translations_pred, global_rotation=None, global_translation=None) -> list[Path]:
    """Write ``{dataset}_sample{idx:05d}_{suffix}_part{pid:02d}_transform.txt`` for every non-empty part of every sample of
    the batch (4 rows of ``%12.8f``, evaluator.py:476-483).  ``data`` needs "rotations", "translations", "scales",
    "points_per_part" (the reference's batch schema); ``sample_indices[b]`` is the dataset index of batch element b.
    Returns the paths written."""
    ppp = data["points_per_part"]
    M = compute_relative_transforms(rotations_pred, translations_pred, data["rotations"], data["translations"], data["scales"], ppp,
                                    global_rotation, global_translation).cpu()
    ppp = ppp.cpu()
    sample_dir = Path(sample_dir)
    sample_dir.mkdir(parents=True, exist_ok=True)
    suffix = _suffix(generation_idx)
    written = []
    for b in range(ppp.shape[0]):
        for pid in torch.where(ppp[b] > 0)[0].tolist():
            path = sample_dir / f"{dataset_name}_sample{int(sample_indices[b]):05d}_{suffix}_part{pid:02d}_transform.txt"
            with open(path, "w") as f:
                for row in M[b, pid].tolist():
                    f.write(" ".join(f"{val:12.8f}" for val in row) + "\n")
            written.append(path)
    return written


class Evaluator:
    """Drop-in for the metric side of ``rectified_point_flow.eval.evaluator.Evaluator``.  ``model`` and the saving options of the
    reference constructor are accepted and kept; the PLY / JSON writers are host I/O and not part of this package
    (``save_transformation_files`` above writes the transform files)."""

    PAIR_DISTANCE_THRESHOLD = 0.05          # evaluator.py:189, 210: 5 cm, hard-coded there

    def __init__(self, model=None, save_pointcloud_parts: bool = False, save_merged_pointcloud_steps: bool = False,
                 max_samples_per_batch: int | None = None, rmse_eval_on: bool = False, rmse_eval_on_transformed: bool = True,
                 folder_suffix: str | None = None, save_json: bool = True):
        self.model = model
        self.save_pointcloud_parts = save_pointcloud_parts
        self.save_merged_pointcloud_steps = save_merged_pointcloud_steps
        self.max_samples_per_batch = max_samples_per_batch
        self.rmse_eval_on = rmse_eval_on
        self.rmse_eval_on_transformed = rmse_eval_on_transformed
        self.folder_suffix = folder_suffix
        self.save_json = save_json

    @staticmethod
    def _recall_at_thresholds(metrics: torch.Tensor, thresholds):            # evaluator.py:252-255; NaN / inf -> 0
        return [(metrics <= threshold).float() for threshold in thresholds]

    @staticmethod
    def _combined_recall_at_specific_pairs(rot_errors, trans_errors, threshold_pairs):      # :257-280
        return [((rot_errors <= r) & (trans_errors <= t)).float() for r, t in threshold_pairs]

    def compute_metrics(self, data: dict, pointclouds_pred, rotations_pred=None, translations_pred=None) -> dict:
        """-> {reference key: (B,) fp32 device tensor}.  ``data``: the reference's batch schema ("pointclouds", "pointclouds_gt",
        "points_per_part", "anchor_parts", "scales", "rotations", "translations", "cu_seqlens_batch").  ``translations_pred`` is in
        the scaled space, as there."""
        pts, pts_gt = data["pointclouds"], data["pointclouds_gt"]
        points_per_part, scales = data["points_per_part"], data["scales"]
        cu = data["cu_seqlens_batch"]
        _require_cuda(pointclouds_pred, "pointclouds_pred")
        device = pointclouds_pred.device
        scales = _f32c(scales.to(device))
        object_cd = compute_cd(pts_gt, pointclouds_pred, cu)                                              # :49
        object_cd_m = object_cd * scales
        metrics = {"chamfer_l2 (m)": object_cd_m, "object_chamfer": object_cd}
        have_poses = rotations_pred is not None and translations_pred is not None
        if have_poses:
            rot_errors, trans_errors = compute_transform_errors(pts, pts_gt, data["rotations"], data["translations"], rotations_pred,
                                                                translations_pred, points_per_part, data["anchor_parts"], None, scales,
                                                                cu)                                        # :60-62
            # the direct errors of :65-67 enter no column of the reference's table (only its commented-out ECDF block read them);
            # metrics.compute_transform_errors_direct is public on its own
            combined = self._combined_recall_at_specific_pairs(rot_errors, trans_errors,
                                                               [(10, 0.2), (15, 0.3), (1, 0.3), (2, 0.3), (5, 2.0), (10, 5.0)])
            rigidity = compute_rigidity_rmse(pts, pointclouds_pred, rotations_pred, translations_pred, points_per_part, cu, scales)
            metrics.update({
                "average_rotation_error (deg)": rot_errors,
                "average_translation_error (m)": trans_errors,
                "recall_at_10deg_0.2m (nss)": combined[0],
                "recall_at_15deg_0.3m (indoor_bufferx)": combined[1],
                "recall_at_5deg_2m (outdoor_bufferx)": combined[4],
                "recall_at_10deg_5m (map)": combined[5],
                "recall_at_chamfer_0.2m": self._recall_at_thresholds(object_cd_m, [0.2])[0],
                "rigidity_rmse (m)": rigidity,
            })
        if self.rmse_eval_on and points_per_part.shape[1] == 2:                                           # :125
            if self.rmse_eval_on_transformed and not have_poses:
                return metrics                                                                            # :127-128
            if self.rmse_eval_on_transformed:
                pm = compute_pair_metrics(data, pts, rotations_pred, translations_pred, self.PAIR_DISTANCE_THRESHOLD)
            else:
                pm = compute_pair_metrics(data, pointclouds_pred, None, None, self.PAIR_DISTANCE_THRESHOLD)
            rmse, ratio, terr, _ = pm.t().contiguous().unbind(0)
            metrics.update({
                "correspondence_rmse (m)": rmse,
                "correspondence_ratio": ratio,
                "recall_at_rmse_0.2m": self._recall_at_thresholds(rmse, [0.2])[0],
                "transform_error_rmse (m)": terr,
                "recall_at_transform_error_rmse_0.2m": self._recall_at_thresholds(terr, [0.2])[0],
            })
        return metrics

    _compute_metrics = compute_metrics          # the reference's name

    def run(self, data: dict, pointclouds_pred, rotations_pred=None, translations_pred=None, save_results: bool = False,
            generation_idx=0, trajectory=None, original_trajectory=None) -> dict:
        """Reference signature (evaluator.py:827-837) -> the metrics table.  ``save_results=True`` is not supported: the PLY / JSON
        writers are host I/O; write the transform files with ``save_transformation_files``."""
        if save_results:
            raise NotImplementedError("Evaluator.run(save_results=True): the PLY / JSON writers are not part of rap_amd; use "
                                      "rap_amd.evaluator.save_transformation_files for the *_transform.txt files")
        return self.compute_metrics(data, pointclouds_pred, rotations_pred, translations_pred)
