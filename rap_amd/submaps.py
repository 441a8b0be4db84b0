"""Submaps on the device (``submaps.hip``): sweeps and poses -> deskewed, fused submaps, their voxel-overlap matrix, and the connectivity
of candidate groups -- the stage of the reference's data preparation that comes before the "views" exist
(``dataset_process/utils/processing_utils.py:1927-2090``).

Packed forms (no host synchronisation; F frames are one ``(N,3)`` array plus the int32 prefix table ``cu_frames`` (F+1,), S submaps are
contiguous runs of frames, ``submap_frames`` (S+1,) a prefix table over frames):
``deskew_packed``, ``fuse_frames_packed``, ``submap_overlap_matrix``, ``groups_connected``.

Mirrors with the reference's signatures (tensors or numpy arrays in; they may synchronise to return Python values):
``deskewing`` (dataset_utils.py:682-747), ``create_submap_from_frames`` (submap_utils.py:26-50),
``calculate_point_cloud_overlap_ratio_fast`` (dataset_utils.py:603-650), ``check_submap_validity`` (submap_utils.py:102-164).

Malformed input (a table that is not a prefix table of its array, a voxel grid wider than 2^21 voxels, a group member out of range) is
not known to the host when a packed call returns: the call writes NaN results and sets bits of a status word on the device
(include/rapflow.h).  Without a ``status=`` tensor of the caller's, the word is followed here: ``check_pending()`` raises ``ValueError``
for verdicts that have arrived, ``synchronize()`` waits for all of them; every packed call looks at the arrived ones first.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .flow_model import _f32c, _require_cuda, workspace

STATUS_BITS = {1: "a prefix table is not one (cu_frames must run from 0 to the number of points, submap_frames within [0, F], neither may decrease)",
               2: "the voxel grid spans 2^21 voxels or more on an axis",
               4: "a group has a length outside [1, n_max] or a member outside [0, S)"}
_pending: list = []          # (event, pinned host int32, what)
_pin = None
_pin_next = 0


def _describe(bits: int) -> str:
    return "; ".join(text for bit, text in STATUS_BITS.items() if bits & bit) or f"status {bits:#x}"


def check_pending(block: bool = True) -> None:
    """Raise ValueError if earlier packed calls found their input malformed (their results are NaN); the message names every such call
    whose verdict was read.  ``block=False`` looks only at the verdicts that have already arrived and never waits for the GPU.  Nothing is
    polled while the current stream is being captured into a graph (an event query is not allowed there)."""
    global _pending
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        return
    keep, bad = [], []
    for ev, host, what in _pending:
        if not block and not ev.query():
            keep.append((ev, host, what))
            continue
        if block:
            ev.synchronize()
        bits = int(host.item())
        if bits:
            bad.append(f"{what}: {_describe(bits)}")
    _pending = keep
    if bad:
        raise ValueError(" | ".join(bad) + " -- the results of " + ("that call" if len(bad) == 1 else f"these {len(bad)} calls") + " are NaN")


def synchronize() -> None:
    """Wait for the device and raise the deferred errors of the packed calls (for a caller that is about to read results)."""
    torch.cuda.synchronize()
    check_pending(block=True)


class _Status:
    """the status word of one call: the caller's tensor, or a fresh one that ``done()`` hands to the pending list"""

    def __init__(self, status, device, what):
        check_pending(block=False)
        self.own = status is None
        self.what, self.device = what, device
        if self.own:
            self.t = torch.zeros(1, dtype=torch.int32, device=device)
        else:
            _require_cuda(status, "status")
            if status.dtype != torch.int32 or status.numel() != 1:
                raise ValueError("status must be one int32 on the device")
            self.t = status

    def done(self):
        global _pin, _pin_next
        if not self.own or torch.cuda.is_current_stream_capturing():
            return
        if len(_pending) >= 64:
            check_pending(block=True)
        if _pin is None:
            _pin = torch.zeros(128, dtype=torch.int32).pin_memory()
        host = _pin[_pin_next:_pin_next + 1]
        _pin_next = (_pin_next + 1) % _pin.numel()
        host.copy_(self.t, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        _pending.append((ev, host, self.what))


def _table(t, device, name):
    t = torch.as_tensor(t) if not isinstance(t, torch.Tensor) else t
    if t.dim() != 1 or t.numel() < 1:
        raise ValueError(f"{name} must be a 1-D prefix table with at least one entry")
    return t.to(device=device, dtype=torch.int32).contiguous()


def _poses(p, device, F, name):
    p = torch.as_tensor(p) if not isinstance(p, torch.Tensor) else p
    if tuple(p.shape) != (F, 4, 4):
        raise ValueError(f"{name} must be ({F},4,4), got {tuple(p.shape)}")
    return p.to(device=device, dtype=torch.float64).contiguous()


def _points(points, name="points"):
    if points.dim() != 2 or points.shape[-1] != 3:
        raise ValueError(f"{name} must be (N,3), got {tuple(points.shape)}")
    _require_cuda(points, name)
    return _f32c(points)


def deskew_packed(points, ts, cu_frames, rel_pose, ts_mid: float = 0.5, status=None):
    """Motion compensation of F packed sweeps: ``points`` (N,3) fp32, ``ts`` (N,) time stamps, ``cu_frames`` (F+1,),
    ``rel_pose`` (F,4,4) float64 = ``inv(pose[f-1]) @ pose[f]`` -> (N,3) fp32.  Per frame ``s = (ts - min) / (max - min) - ts_mid``
    (``0.5 - ts_mid`` where ``max - min <= 1e-8``, the reference's rule) and ``p' = R(s) p + s T`` with ``R(s) = exp(s log R)``.  A frame
    whose ``rel_pose`` is the identity comes back bit for bit.  Semantics: ``rap_deskew`` in include/rapflow.h.  No host synchronisation."""
    P = _points(points)
    device = P.device
    t = _f32c(ts.reshape(-1))
    _require_cuda(ts, "ts")
    N = P.shape[0]
    if t.shape[0] != N:
        raise ValueError(f"ts must have one entry per point ({N}), got {t.shape[0]}")
    cu = _table(cu_frames, device, "cu_frames")
    F = cu.shape[0] - 1
    rp = _poses(rel_pose, device, F, "rel_pose")
    out = torch.empty_like(P)
    if F == 0:
        if N:
            raise ValueError("points without a frame")
        return out
    st = _Status(status, device, f"deskew_packed of {F} frame(s), {N} points")
    lib = _lib.load()
    ws = workspace(device, lib.rap_deskew_workspace_bytes(N, F))
    with torch.cuda.device(device):
        rc = lib.rap_deskew(_lib.ptr(P), _lib.ptr(t), _lib.ptr(cu), F, N, _lib.ptr(rp), float(ts_mid), _lib.ptr(out), _lib.ptr(st.t), _lib.ptr(ws),
                            ws.numel(), _lib.current_stream(device))
    _lib.check(rc, "rap_deskew")
    st.done()
    return out


def fuse_frames_packed(points, cu_frames, pose, normals=None, origin=None, status=None):
    """Frames -> world: ``world = fp32(R p + t - origin)`` with the arithmetic in double (``origin`` (3,) float64 or None), rows in their
    order, so submap s is ``world[cu_frames[submap_frames[s]]:cu_frames[submap_frames[s+1]]]`` -- ``create_submap_from_frames`` for every
    submap at once.  With ``normals`` (N,3) -> ``(world, world_normals)``, ``R n`` divided by its norm (by 1 below 1e-8).
    Semantics: ``rap_fuse_frames``.  No host synchronisation."""
    P = _points(points)
    device = P.device
    N = P.shape[0]
    cu = _table(cu_frames, device, "cu_frames")
    F = cu.shape[0] - 1
    po = _poses(pose, device, F, "pose")
    nrm = None
    if normals is not None:
        nrm = _points(normals, "normals")
        if nrm.shape[0] != N:
            raise ValueError(f"normals must have one row per point ({N}), got {nrm.shape[0]}")
    org = None
    if origin is not None:
        org = (torch.as_tensor(origin) if not isinstance(origin, torch.Tensor) else origin).to(device=device, dtype=torch.float64).reshape(3).contiguous()
    world = torch.empty_like(P)
    wn = torch.empty_like(P) if nrm is not None else None
    if F == 0:
        if N:
            raise ValueError("points without a frame")
    else:
        st = _Status(status, device, f"fuse_frames_packed of {F} frame(s), {N} points")
        lib = _lib.load()
        ws = workspace(device, lib.rap_fuse_frames_workspace_bytes(N, F))
        with torch.cuda.device(device):
            rc = lib.rap_fuse_frames(_lib.ptr(P), _lib.ptr(nrm), _lib.ptr(cu), F, N, _lib.ptr(po), _lib.ptr(org), _lib.ptr(world), _lib.ptr(wn),
                                     _lib.ptr(st.t), _lib.ptr(ws), ws.numel(), _lib.current_stream(device))
        _lib.check(rc, "rap_fuse_frames")
        st.done()
    return world if nrm is None else (world, wn)


def submap_overlap_matrix(points, cu_frames, submap_frames, voxel_size: float = 2.0, pose=None, status=None):
    """The voxel-set Jaccard matrix of S submaps -> ``(ratio (S,S) float64, n_voxels (S,) int64)``: ``ratio[i,j] = |Vi n Vj| / |Vi u Vj|``
    with ``V`` the set of ``floor((R p + t) / voxel_size)`` (double) of a submap's rows, 0.0 where a set is empty.  ``pose`` (F,4,4) float64,
    or None for points that are already in a common frame.  S <= 4096.  Semantics: ``rap_submap_overlap``.  No host synchronisation."""
    P = _points(points)
    device = P.device
    N = P.shape[0]
    cu = _table(cu_frames, device, "cu_frames")
    sf = _table(submap_frames, device, "submap_frames")
    F, S = cu.shape[0] - 1, sf.shape[0] - 1
    if F < 1 or not 1 <= S <= 4096:
        raise ValueError(f"need at least one frame and 1 .. 4096 submaps, got F = {F}, S = {S}")
    vs = float(voxel_size)
    if not (vs > 0.0 and vs < float("inf")):
        raise ValueError(f"voxel_size must be positive and finite, got {voxel_size}")
    po = _poses(pose, device, F, "pose") if pose is not None else None
    ratio = torch.empty((S, S), dtype=torch.float64, device=device)
    nv = torch.empty((S,), dtype=torch.int64, device=device)
    st = _Status(status, device, f"submap_overlap_matrix of {S} submap(s), {N} points")
    lib = _lib.load()
    ws = workspace(device, lib.rap_submap_overlap_workspace_bytes(N, F, S))
    with torch.cuda.device(device):
        rc = lib.rap_submap_overlap(_lib.ptr(P), _lib.ptr(cu), F, N, _lib.ptr(po), _lib.ptr(sf), S, vs, _lib.ptr(ratio), _lib.ptr(nv), _lib.ptr(st.t),
                                    _lib.ptr(ws), ws.numel(), _lib.current_stream(device))
    _lib.check(rc, "rap_submap_overlap")
    st.done()
    return ratio, nv


def groups_connected(ratio, groups, group_len, lo: float, hi: float, status=None):
    """For G candidate groups of submaps (``groups`` (G,n_max <= 64) int32, the first ``group_len[g]`` entries of row g): is the group
    connected through pairs with ``lo <= ratio <= hi`` (both inclusive)?  -> (G,) uint8.  The union-find of ``check_submap_validity``.
    Semantics: ``rap_submap_groups_connected``.  No host synchronisation."""
    _require_cuda(ratio, "ratio")
    device = ratio.device
    if ratio.dim() != 2 or ratio.shape[0] != ratio.shape[1] or not 1 <= ratio.shape[0] <= 4096:
        raise ValueError(f"ratio must be (S,S) with 1 <= S <= 4096, got {tuple(ratio.shape)}")
    r = ratio.to(torch.float64).contiguous()
    g = (torch.as_tensor(groups) if not isinstance(groups, torch.Tensor) else groups).to(device=device, dtype=torch.int32).contiguous()
    if g.dim() != 2 or not 1 <= g.shape[1] <= 64:
        raise ValueError(f"groups must be (G, n_max) with 1 <= n_max <= 64, got {tuple(g.shape)}")
    gl = _table(group_len, device, "group_len") if g.shape[0] else torch.zeros(0, dtype=torch.int32, device=device)
    if gl.shape[0] != g.shape[0]:
        raise ValueError(f"group_len must have one entry per group ({g.shape[0]}), got {gl.shape[0]}")
    if lo != lo or hi != hi:
        raise ValueError("lo and hi must not be NaN")
    out = torch.zeros((g.shape[0],), dtype=torch.uint8, device=device)
    if g.shape[0]:
        st = _Status(status, device, f"groups_connected of {g.shape[0]} group(s)")
        lib = _lib.load()
        with torch.cuda.device(device):
            rc = lib.rap_submap_groups_connected(_lib.ptr(r), r.shape[0], _lib.ptr(g), _lib.ptr(gl), g.shape[0], g.shape[1], float(lo), float(hi),
                                                 _lib.ptr(out), _lib.ptr(st.t), _lib.current_stream(device))
        _lib.check(rc, "rap_submap_groups_connected")
        st.done()
    return out


# ---- the reference's signatures -----------------------------------------------------------------------------------------------------
def _dev(x, name, dtype=None):
    """numpy array -> tensor on the current GPU; a tensor must already live on a GPU (no CPU path)"""
    if isinstance(x, torch.Tensor):
        _require_cuda(x, name)
        return x if dtype is None else x.to(dtype)
    if not torch.cuda.is_available():
        raise _lib.RapError(f"{name}: rap_amd has no CPU path and no GPU is available")
    return torch.as_tensor(np.asarray(x), device="cuda", dtype=dtype)


def deskewing(points, ts, pose, ts_mid_pose: float = 0.5):
    """Reference signature (``deskewing``, dataset_utils.py:682-747): one sweep ``points`` (N,3) or (N,4) (columns past xyz are kept),
    ``ts`` (N,) or (N,1), ``pose`` (4,4) the transformation from the current to the last frame.  ``ts is None`` returns the input.
    A numpy array in gives a numpy array back (fp32, as the reference's); a tensor gives a tensor."""
    if ts is None:
        return points
    as_numpy = not isinstance(points, torch.Tensor)
    p = _dev(points, "points", torch.float32)
    if p.dim() != 2 or p.shape[-1] < 3:
        raise ValueError(f"points must be (N,3) or (N,4), got {tuple(p.shape)}")
    t = _dev(ts, "ts", torch.float32).reshape(-1)
    rel = _dev(pose, "pose", torch.float64).reshape(1, 4, 4)
    cu = torch.tensor([0, p.shape[0]], dtype=torch.int32, device=p.device)
    out = p.clone()
    out[:, :3] = deskew_packed(p[:, :3], t, cu, rel, ts_mid_pose)
    synchronize()
    return out.cpu().numpy() if as_numpy else out


def create_submap_from_frames(points_list, poses_list, start_idx: int, num_frames: int, normals_list=None):
    """Reference signature (``create_submap_from_frames``, submap_utils.py:26-50): the frames ``start_idx .. start_idx + num_frames - 1``
    (cut at the end of ``points_list``) in world coordinates, stacked -> ``(points, normals or None)``, fp32 on the device (numpy lists
    give numpy arrays back).  A frame without a pose is taken as it is, as in the reference.  Normals are all or nothing over the range
    (the reference stacks whatever frames have them, which no longer lines up with the points)."""
    stop = min(start_idx + num_frames, len(points_list))
    idx = list(range(start_idx, stop))
    as_numpy = not any(isinstance(points_list[i], torch.Tensor) for i in idx)
    if not idx:
        return (np.array([]), None) if as_numpy else (torch.empty((0, 3)), None)
    pts = [_dev(points_list[i], "points_list", torch.float32).reshape(-1, 3) for i in idx]
    device = pts[0].device
    have = [bool(normals_list) and i < len(normals_list) and normals_list[i] is not None for i in idx]
    if any(have) and not all(have):
        raise ValueError("normals_list must hold normals for every frame of the range or for none")
    nrm = torch.cat([_dev(normals_list[i], "normals_list", torch.float32).reshape(-1, 3).to(device) for i in idx]) if all(have) else None
    eye = torch.eye(4, dtype=torch.float64, device=device)
    pose = torch.stack([_dev(poses_list[i], "poses_list", torch.float64).to(device) if i < len(poses_list) else eye for i in idx])
    cu = torch.tensor(np.concatenate([[0], np.cumsum([p.shape[0] for p in pts])]), dtype=torch.int32, device=device)
    res = fuse_frames_packed(torch.cat(pts), cu, pose, normals=nrm)
    world, wn = res if nrm is not None else (res, None)
    synchronize()
    if as_numpy:
        return world.cpu().numpy(), (wn.cpu().numpy() if wn is not None else None)
    return world, wn


def calculate_point_cloud_overlap_ratio_fast(points1, points2, voxel_size: float = 2.0, max_points_per_cloud: int = 20000, generator=None):
    """Reference signature (``calculate_point_cloud_overlap_ratio_fast``, dataset_utils.py:603-650) -> float: the Jaccard ratio of the two
    clouds' voxel sets.  A cloud with more than ``max_points_per_cloud`` points is cut to a random subset of that size, drawn on the
    device with ``generator`` (a ``torch.Generator`` of that device; the reference draws an unseeded ``np.random.choice``).  Below the
    limit the result is deterministic and equals the reference's."""
    a, b = _dev(points1, "points1", torch.float32).reshape(-1, 3), _dev(points2, "points2", torch.float32).reshape(-1, 3)
    if a.shape[0] == 0 or b.shape[0] == 0:
        return 0.0
    b = b.to(a.device)
    clouds = []
    for c in (a, b):
        if c.shape[0] > max_points_per_cloud:
            c = c[torch.randperm(c.shape[0], generator=generator, device=c.device)[:max_points_per_cloud]]
        clouds.append(c)
    cu = torch.tensor([0, clouds[0].shape[0], clouds[0].shape[0] + clouds[1].shape[0]], dtype=torch.int32, device=a.device)
    sf = torch.tensor([0, 1, 2], dtype=torch.int32, device=a.device)
    ratio, _ = submap_overlap_matrix(torch.cat(clouds), cu, sf, voxel_size)
    synchronize()
    return float(ratio[0, 1])


def check_submap_validity(selected_indices, submap_boundaries, submap_centers, points_list, poses, frame_ids, min_spatial_threshold,
                          max_spatial_threshold, min_overlap_ratio, max_overlap_ratio, overlap_method=None, min_frame_interval: int = 0,
                          overlap_voxel_size: float = 2.0, attempt: int = -1) -> bool:
    """Reference signature (``check_submap_validity``, submap_utils.py:102-164) -> bool: are the selected submaps connected through pairs
    whose voxel overlap lies in ``[min_overlap_ratio, max_overlap_ratio]``?  As in the reference only the overlap decides here
    (``submap_centers``, the spatial thresholds, ``overlap_method`` and ``min_frame_interval`` are not looked at: that is
    ``check_submap_validity_fast``, a few host integers).  One overlap matrix and one connectivity call for the whole group; every point
    is used (the reference cuts clouds above 20 000 points to a random subset, pair by pair).  At most 64 submaps."""
    n = len(selected_indices)
    if not 1 <= n <= 64:
        raise ValueError(f"need 1 .. 64 selected submaps, got {n}")
    frames, sf = [], [0]
    for idx in selected_indices:
        first, last = submap_boundaries[idx]
        i0, i1 = frame_ids.index(first), frame_ids.index(last) + 1         # the end of a boundary is inclusive
        frames += list(range(i0, min(i1, len(points_list))))
        sf.append(len(frames))
    if not frames:
        return n == 1
    pts = [_dev(points_list[i], "points_list", torch.float32).reshape(-1, 3) for i in frames]
    device = pts[0].device
    eye = torch.eye(4, dtype=torch.float64, device=device)
    pose = torch.stack([_dev(poses[i], "poses", torch.float64).to(device) if i < len(poses) else eye for i in frames])
    cu = torch.tensor(np.concatenate([[0], np.cumsum([p.shape[0] for p in pts])]), dtype=torch.int32, device=device)
    ratio, _ = submap_overlap_matrix(torch.cat(pts), cu, torch.tensor(sf, dtype=torch.int32, device=device), overlap_voxel_size, pose=pose)
    group = torch.arange(n, dtype=torch.int32, device=device).reshape(1, n)
    ok = groups_connected(ratio, group, torch.tensor([n], dtype=torch.int32, device=device), min_overlap_ratio, max_overlap_ratio)
    synchronize()
    return bool(ok[0])
