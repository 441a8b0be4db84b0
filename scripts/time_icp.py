"""Time the batched ICP (rap_icp) at a fixed 30 iterations: relative_rmse_thr = -inf, so no problem stops early and every call does the
same work.  Two workloads: 32 problems of 4096 x 4096 points, and one problem of 100 000 x 100 000.

Per call: GPU time (HIP events around the call) after --warmup calls, the median and the 10th / 90th percentile over --calls; and the pair
distances per second = iterations x sum(nx * ny) / time.  The search kernel this one is built from does 2.1 G pairs in 0.69 ms (DESIGN.md
section 7, row 4).  Prints one JSON line per workload; --out FILE also writes them.

--search grid times the same calls on the uniform-grid neighbour index (rap_icp_grid: the same results, bit for bit); its
"pair_distances_per_s" is then the rate a brute-force search would need to keep up, not work that was done.

--estimation point_to_plane times rap_icp_plane / rap_icp_plane_grid on the same clouds with the analytic normals of the surface (the
iterations after the fourth or so run at the fixed point: the same work, which is what a per-iteration time needs).  --normals-points N
adds a line for the normal estimation (rap_estimate_normals, 20 neighbours within 0.5) of one cloud of N points of the same surface.

--loss {huber,cauchy,tukey,all} (point-to-plane only) times the robust entry points (rap_icp_plane_robust / rap_icp_plane_grid_robust) at
--loss-scale.  Every workload is then timed with loss none through the plain entry point first, in the same process, and each robust
line carries "ratio_to_none": its median over that one.  There is no threshold: the number to read is the ratio.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

WORKLOADS = {"32x4096": (32, 4096), "1x100000": (1, 100_000)}


def make_problems(torch, K, n, seed=2024):
    """K pairs of n + n points: two samplings of one bumpy surface, the second moved by 4 degrees and a few centimetres"""
    g = torch.Generator().manual_seed(seed)

    def surf():
        xy = torch.rand(K, n, 2, generator=g) - 0.5
        x, y = xy[..., 0], xy[..., 1]
        return torch.stack([x, y, 0.15 * torch.sin(5 * x) * torch.cos(4 * y) + 0.1 * x * x], dim=-1)
    th = torch.tensor(4.0 * 3.14159265 / 180.0)
    Rz = torch.tensor([[torch.cos(th), -torch.sin(th), 0.0], [torch.sin(th), torch.cos(th), 0.0], [0.0, 0.0, 1.0]])
    X, Yl = surf(), surf()
    x, y = Yl[..., 0], Yl[..., 1]                                     # the surface's normal (-f_x, -f_y, 1), moved with the cloud
    nrm = torch.stack([-(0.75 * torch.cos(5 * x) * torch.cos(4 * y) + 0.2 * x), 0.6 * torch.sin(5 * x) * torch.sin(4 * y), torch.ones_like(x)], dim=-1)
    nrm = nrm / nrm.norm(dim=-1, keepdim=True)
    return X.cuda(), (Yl @ Rz + torch.tensor([0.03, -0.02, 0.01])).cuda(), (nrm @ Rz).cuda()


def time_calls(torch, call, warmup, calls):
    for _ in range(warmup):
        out = call()
    torch.cuda.synchronize()
    gpu = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = call()
        e1.record()
        torch.cuda.synchronize()
        gpu.append(e0.elapsed_time(e1))
    return out, gpu


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", choices=sorted(WORKLOADS) + ["all"], default="all")
    ap.add_argument("--iterations", type=int, default=30)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--search", choices=["brute", "grid"], default="brute")
    ap.add_argument("--estimation", choices=["point_to_point", "point_to_plane"], default="point_to_point")
    ap.add_argument("--normals-points", type=int, default=0, help="also time the normal estimation of one cloud of this many points")
    ap.add_argument("--loss", choices=["none", "huber", "cauchy", "tukey", "all"], default="none")
    ap.add_argument("--loss-scale", type=float, default=0.01)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.loss != "none" and a.estimation != "point_to_plane":
        ap.error("--loss needs --estimation point_to_plane")
    losses = [None] + (["huber", "cauchy", "tukey"] if a.loss == "all" else [] if a.loss == "none" else [a.loss])
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import rap_amd
    lines = []
    pct = lambda v, p: sorted(v)[min(len(v) - 1, int(round(p * (len(v) - 1))))]
    for name in (sorted(WORKLOADS) if a.workload == "all" else [a.workload]):
        K, n = WORKLOADS[name]
        X, Y, Yn = make_problems(torch, K, n)
        extra = dict(estimation=a.estimation, Y_normals=Yn) if a.estimation == "point_to_plane" else {}
        base = None
        for loss in losses:
            robust = dict(loss=loss, loss_scale=a.loss_scale) if loss else {}
            call = lambda: rap_amd.iterative_closest_point(X, Y, max_iterations=a.iterations, relative_rmse_thr=float("-inf"), search=a.search,
                                                           **extra, **robust)
            sol, gpu = time_calls(torch, call, a.warmup, a.calls)
            assert int(sol.iterations.min()) == a.iterations and not bool(sol.converged.any()), "a problem stopped early"
            med = statistics.median(gpu)
            pairs = a.iterations * K * n * n
            row = {"workload": name, "search": a.search, "estimation": a.estimation, "problems": K, "points": n, "iterations": a.iterations, "calls": len(gpu), "warmup": a.warmup,
                   "gpu_ms": {"median": med, "p10": pct(gpu, 0.1), "p90": pct(gpu, 0.9)}, "ms_per_iteration": med / a.iterations,
                   "pair_distances_per_s": pairs / (med * 1e-3), "mean_rmse": float(sol.rmse.mean())}
            if len(losses) > 1:
                base = med if loss is None else base
                row.update({"loss": loss or "none", "loss_scale": a.loss_scale if loss else None,
                            "entry_point": "rap_icp_plane" + ("_grid" if a.search == "grid" else "") + ("_robust" if loss else ""),
                            "ratio_to_none": med / base})
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
    if a.normals_points > 0:
        P = make_problems(torch, 1, a.normals_points)[1][0]
        nrm, gpu = time_calls(torch, lambda: rap_amd.estimate_point_normals(P, k_neighbors=20, radius=0.5), a.warmup, a.calls)
        assert bool(torch.isfinite(nrm).all()) and bool((nrm.norm(dim=1) > 0.5).all()), "a point without a normal"
        lines.append(json.dumps({"workload": "normals", "points": a.normals_points, "max_nn": 20, "radius": 0.5, "calls": len(gpu), "warmup": a.warmup,
                                 "gpu_ms": {"median": statistics.median(gpu), "p10": pct(gpu, 0.1), "p90": pct(gpu, 0.9)},
                                 "pair_distances_per_s": a.normals_points ** 2 / (statistics.median(gpu) * 1e-3)}))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
