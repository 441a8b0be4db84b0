"""rap_amd -- MI355X-native (gfx950) rectified-flow registration sampler.

One hot path of PRBonn/RAP, rebuilt as hand-written HIP kernels behind the reference's own Python API:
``rectified_point_flow/{sampler.py, flow_model/, procrustes.py}`` behind
``RectifiedPointFlow.sample_rectified_flow``.  See DESIGN.md / INTEGRATION.md.
"""
from .data import transform_and_collate
from .evaluator import Evaluator
from .flow_model import PointCloudDiT
from .normals import estimate_normals_packed, estimate_point_normals, orient_normals_packed
from .icp import (ICPSolution, align_anchor, compute_transform_errors_icp, icp_packed, iterative_closest_point, k_nearest_neighbors_packed,
                  nearest_neighbors_packed)
from .metrics import compute_part_acc
from .modeling import RectifiedPointFlow
from .procrustes import fit_transformations, rigidify_prediction_with_procrustes, solve_procrustes
from .sampler import euler_step, flow_sampler, get_sampler
from .scene import SceneRefinement, refine_registration, refine_scene_packed
from .submaps import (calculate_point_cloud_overlap_ratio_fast, check_submap_validity, create_submap_from_frames, deskew_packed, deskewing,
                      fuse_frames_packed, groups_connected, submap_overlap_matrix)
from .selection import (average_trajectory_rigidity_rmse, compute_overlap_ratio, compute_rigidity_rmse,
                        select_generations_by_overlap, select_generations_by_rigidity)

__all__ = ["PointCloudDiT", "RectifiedPointFlow", "fit_transformations", "rigidify_prediction_with_procrustes",
           "solve_procrustes", "euler_step", "flow_sampler", "get_sampler", "compute_rigidity_rmse",
           "average_trajectory_rigidity_rmse", "select_generations_by_rigidity", "compute_overlap_ratio",
           "select_generations_by_overlap", "transform_and_collate", "Evaluator", "iterative_closest_point", "icp_packed", "ICPSolution",
           "align_anchor", "compute_transform_errors_icp", "compute_part_acc", "nearest_neighbors_packed", "k_nearest_neighbors_packed",
           "estimate_normals_packed", "estimate_point_normals", "orient_normals_packed", "deskew_packed", "fuse_frames_packed", "submap_overlap_matrix",
           "groups_connected", "deskewing", "create_submap_from_frames", "calculate_point_cloud_overlap_ratio_fast",
           "check_submap_validity", "refine_scene_packed", "refine_registration", "SceneRefinement"]
