"""Time the batched ICP (rap_icp) at a fixed 30 iterations: relative_rmse_thr = -inf, so no problem stops early and every call does the
same work.  Two workloads: 32 problems of 4096 x 4096 points, and one problem of 100 000 x 100 000.

Per call: GPU time (HIP events around the call) after --warmup calls, the median and the 10th / 90th percentile over --calls; and the pair
distances per second = iterations x sum(nx * ny) / time.  The search kernel this one is built from does 2.1 G pairs in 0.69 ms (DESIGN.md
section 7, row 4).  Prints one JSON line per workload; --out FILE also writes them.

--search grid times the same calls on the uniform-grid neighbour index (rap_icp_grid: the same results, bit for bit); its
"pair_distances_per_s" is then the rate a brute-force search would need to keep up, not work that was done.
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
    return surf().cuda(), (surf() @ Rz + torch.tensor([0.03, -0.02, 0.01])).cuda()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", choices=sorted(WORKLOADS) + ["all"], default="all")
    ap.add_argument("--iterations", type=int, default=30)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--search", choices=["brute", "grid"], default="brute")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import rap_amd
    lines = []
    for name in (sorted(WORKLOADS) if a.workload == "all" else [a.workload]):
        K, n = WORKLOADS[name]
        X, Y = make_problems(torch, K, n)
        call = lambda: rap_amd.iterative_closest_point(X, Y, max_iterations=a.iterations, relative_rmse_thr=float("-inf"), search=a.search)
        for _ in range(a.warmup):
            sol = call()
        torch.cuda.synchronize()
        gpu = []
        for _ in range(a.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            sol = call()
            e1.record()
            torch.cuda.synchronize()
            gpu.append(e0.elapsed_time(e1))
        assert int(sol.iterations.min()) == a.iterations and not bool(sol.converged.any()), "a problem stopped early"
        pct = lambda v, p: sorted(v)[min(len(v) - 1, int(round(p * (len(v) - 1))))]
        med = statistics.median(gpu)
        pairs = a.iterations * K * n * n
        lines.append(json.dumps({"workload": name, "search": a.search, "problems": K, "points": n, "iterations": a.iterations, "calls": len(gpu), "warmup": a.warmup,
                                 "gpu_ms": {"median": med, "p10": pct(gpu, 0.1), "p90": pct(gpu, 0.9)}, "ms_per_iteration": med / a.iterations,
                                 "pair_distances_per_s": pairs / (med * 1e-3), "mean_rmse": float(sol.rmse.mean())}))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
