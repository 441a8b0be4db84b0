"""Time the evaluator's metrics table at the 32 x 2 x 4096 geometry (rmse_eval_on, transformed clouds).

  --mode batched   one rap_amd.Evaluator.compute_metrics call (three launches for all pairs, no host read)
  --mode loop      the same table from the functions that existed before the batched kernel: compute_cd, compute_transform_errors,
                   compute_rigidity_rmse and a Python loop of compute_correspondence_rmse over the pairs on torch-scaled,
                   torch-transformed parts (one host read-back per pair), the transform error by torch ops on the device.
                   Uses nothing newer, so it runs against an older checkout: --package-root DIR puts DIR first on sys.path.

Per call: wall time (perf_counter around the call and a stream synchronisation) and GPU time (HIP events around the call); after
--warmup calls, the median and the 10th / 90th percentile over --calls (>= 20).  Prints one JSON line; --out FILE also writes it.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time


def make_batch(torch, B, n, seed=2024):
    """B scan pairs of n + n points: two views of one random cloud, the second view jittered by up to 3 cm (in metres) so that about
    half of the source points have a correspondence within 5 cm; predicted poses = GT poses off by 1 degree / 1 cm."""
    g = torch.Generator().manual_seed(seed)
    scales = torch.rand(B, generator=g) * 45 + 5
    src = torch.rand(B, n, 3, generator=g) - 0.5
    jit = torch.randn(B, n, 3, generator=g) * (0.03 / scales)[:, None, None]
    gt = torch.stack([src, src + jit], dim=1)                                       # (B,2,n,3)
    q = torch.randn(B, 2, 4, generator=g); q = q / q.norm(dim=-1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                     2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], dim=-1).view(B, 2, 3, 3)
    t = torch.rand(B, 2, 3, generator=g) - 0.5
    cond = torch.einsum("bpni,bpij->bpnj", gt - t[:, :, None, :], R)                # gt = cond @ R^T + t
    th = torch.tensor(3.14159265 / 180.0)
    Rz = torch.tensor([[torch.cos(th), -torch.sin(th), 0.0], [torch.sin(th), torch.cos(th), 0.0], [0.0, 0.0, 1.0]])
    R_pred, t_pred = R @ Rz, t + 0.01 / scales[:, None, None]
    pred = torch.einsum("bpni,bpji->bpnj", cond, R_pred) + t_pred[:, :, None, :]
    dev = torch.device("cuda")
    anchor = torch.zeros(B, 2, dtype=torch.uint8); anchor[:, 0] = 1
    data = {"pointclouds": cond.reshape(-1, 3).contiguous().to(dev), "pointclouds_gt": gt.reshape(-1, 3).contiguous().to(dev),
            "points_per_part": torch.full((B, 2), n, dtype=torch.int64, device=dev), "anchor_parts": anchor.to(dev),
            "scales": scales.to(dev), "rotations": R.contiguous().to(dev), "translations": t.contiguous().to(dev),
            "cu_seqlens_batch": (torch.arange(B + 1, dtype=torch.int32) * 2 * n).to(dev)}
    return data, pred.reshape(-1, 3).contiguous().to(dev), R_pred.contiguous().to(dev), t_pred.contiguous().to(dev)


def table_by_loop(torch, data, pred, R_pred, t_pred):
    from rap_amd.metrics import compute_cd, compute_correspondence_rmse, compute_transform_errors
    from rap_amd.selection import compute_rigidity_rmse
    pts, gt, ppp, cu, sc = data["pointclouds"], data["pointclouds_gt"], data["points_per_part"], data["cu_seqlens_batch"], data["scales"]
    B, n = ppp.shape[0], gt.shape[0] // (2 * ppp.shape[0])
    cd = compute_cd(gt, pred, cu)
    out = {"chamfer_l2 (m)": cd * sc, "object_chamfer": cd}
    rot, trans = compute_transform_errors(pts, gt, data["rotations"], data["translations"], R_pred, t_pred, ppp, data["anchor_parts"], None, sc, cu)
    out["average_rotation_error (deg)"], out["average_translation_error (m)"] = rot, trans
    out["rigidity_rmse (m)"] = compute_rigidity_rmse(pts, pred, R_pred, t_pred, ppp, cu, sc)
    s3 = sc[:, None, None, None]
    gt_s = gt.view(B, 2, n, 3) * s3
    moved = (pts.view(B, 2, n, 3) * s3) @ R_pred.transpose(-1, -2) + (t_pred * sc[:, None, None])[:, :, None, :]
    rmse, ratio = torch.zeros(B, device=gt.device), torch.zeros(B, device=gt.device)
    for b in range(B):                                                             # evaluator.py:153-236, one read-back per pair
        r, _, c = compute_correspondence_rmse(gt_s[b, 0], gt_s[b, 1], moved[b, 0], moved[b, 1], distance_threshold=0.05)
        rmse[b], ratio[b] = r, c
    def rel(R, t):
        Rr = R[:, 1] @ R[:, 0].transpose(-1, -2)
        return Rr, t[:, 1] * sc[:, None] - (Rr @ (t[:, 0] * sc[:, None])[:, :, None])[:, :, 0]
    Rg, tg = rel(data["rotations"], data["translations"]); Re, te = rel(R_pred, t_pred)
    dR, dt = Rg.transpose(-1, -2) @ Re, te - tg
    q2 = ((3.0 - dR.diagonal(dim1=-2, dim2=-1).sum(-1)) * 0.25).clamp(min=0.0)
    out["correspondence_rmse (m)"], out["correspondence_ratio"] = rmse, ratio
    out["transform_error_rmse (m)"] = torch.sqrt((dt * dt).sum(-1) + q2)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mode", choices=("batched", "loop"), default="batched")
    ap.add_argument("--package-root", default=None)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    root = a.package_root or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import torch
    import rap_amd
    data, pred, R_pred, t_pred = make_batch(torch, a.batch, a.points)
    if a.mode == "batched":
        ev = rap_amd.Evaluator(rmse_eval_on=True, rmse_eval_on_transformed=True)
        call = lambda: ev.compute_metrics(data, pred, R_pred, t_pred)
    else:
        call = lambda: table_by_loop(torch, data, pred, R_pred, t_pred)
    for _ in range(a.warmup):
        out = call()
    torch.cuda.synchronize()
    wall, gpu = [], []
    for _ in range(max(a.calls, 20)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        out = call()
        e1.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        gpu.append(e0.elapsed_time(e1))
    pct = lambda v, p: sorted(v)[min(len(v) - 1, int(round(p * (len(v) - 1))))]
    res = {"mode": a.mode, "package": os.path.dirname(os.path.abspath(rap_amd.__file__)), "batch": a.batch, "points_per_part": a.points,
           "calls": len(wall), "warmup": a.warmup,
           "wall_ms": {"median": statistics.median(wall), "p10": pct(wall, 0.1), "p90": pct(wall, 0.9)},
           "gpu_ms": {"median": statistics.median(gpu), "p10": pct(gpu, 0.1), "p90": pct(gpu, 0.9)},
           "mean_correspondence_ratio": float(out["correspondence_ratio"].mean()),
           "mean_correspondence_rmse_m": float(out["correspondence_rmse (m)"].mean()),
           "mean_transform_error_m": float(out["transform_error_rmse (m)"].mean())}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
