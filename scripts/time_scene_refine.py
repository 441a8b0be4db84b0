"""Time the joint multi-view refinement (rap_scene_refine) at a fixed number of iterations: relative_rmse_thr = -inf, so no scene stops
early and every call does the same work.  Workloads: one scene of 4 and of 8 views, 20 000 and 200 000 points per view, all ordered pairs
(12 / 56 edges), on the bumpy surface of scripts/time_icp.py -- every view samples an overlapping window of it, lives in a frame of its
own and starts a degree and a centimetre off; the analytic normals of the surface.

Per call: GPU time (HIP events around the call) after --warmup calls, the median and the 10th / 90th percentile over --calls, clocks as
found.  As context, in the same session, the P - 1 pairwise point-to-plane ICPs of every other view against the first on the grid index
(one icp_packed call of P - 1 problems, the same number of iterations): what a user could do before, which ignores every overlap but
the anchor's.  There is no threshold: the call is new.  Prints one JSON line per workload; --out FILE also writes them.

--loss {huber,cauchy,tukey,all} also times rap_scene_refine_robust at --loss-scale on every workload, after the plain call and in the same
process: one more line per loss, with "ratio_to_none" = its median over the plain call's.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

WORKLOADS = [(4, 20_000), (8, 20_000), (4, 200_000), (8, 200_000)]


def make_scene(torch, V, n, seed=2024):
    """-> P (V*n,3), N (V*n,3), seg (V,2), R0 (V,3,3), T0 (V,3): view v samples the window [lo_v, lo_v + 0.7] x [-0.5, 0.5] of the surface,
    is moved into its own frame (world = x R_v + T_v) and starts a degree and a centimetre off that pose (view 0 at it)"""
    g = torch.Generator().manual_seed(seed)

    def rot(axis, deg):
        a = torch.tensor(axis, dtype=torch.float64)
        a = a / a.norm()
        K = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=torch.float64)
        th = math.radians(deg)
        return torch.eye(3, dtype=torch.float64) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)
    Ps, Ns, R0, T0 = [], [], [], []
    for v in range(V):
        lo = -0.5 + 0.3 * v / max(V - 1, 1)
        xy = torch.rand(n, 2, generator=g, dtype=torch.float64)
        x, y = lo + 0.7 * xy[:, 0], xy[:, 1] - 0.5
        W = torch.stack([x, y, 0.15 * torch.sin(5 * x) * torch.cos(4 * y) + 0.1 * x * x], dim=-1)
        nw = torch.stack([-(0.75 * torch.cos(5 * x) * torch.cos(4 * y) + 0.2 * x), 0.6 * torch.sin(5 * x) * torch.sin(4 * y), torch.ones_like(x)], dim=-1)
        nw = nw / nw.norm(dim=-1, keepdim=True)
        R = rot((0.3 + v, -0.5, 0.8), 5.0 + v)
        T = torch.tensor([0.05 * v, -0.03, 0.02 * v], dtype=torch.float64)
        Ps.append(((W - T) @ R.T).float())
        Ns.append((nw @ R.T).float())
        off = rot((1.0, v, -0.5), 1.0 if v else 0.0)
        R0.append((R @ off).float())
        T0.append((T + (0.01 if v else 0.0) * torch.tensor([0.6, -0.5, 0.6], dtype=torch.float64)).float())
    seg = torch.tensor([[v * n, n] for v in range(V)], dtype=torch.int32)
    return torch.cat(Ps).cuda(), torch.cat(Ns).cuda(), seg.cuda(), torch.stack(R0).cuda(), torch.stack(T0).cuda()


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
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gate", type=float, default=0.05)
    ap.add_argument("--loss", choices=["none", "huber", "cauchy", "tukey", "all"], default="none")
    ap.add_argument("--loss-scale", type=float, default=0.01)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    losses = ["huber", "cauchy", "tukey"] if a.loss == "all" else [] if a.loss == "none" else [a.loss]
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import rap_amd
    lines = []
    pct = lambda v, p: sorted(v)[min(len(v) - 1, int(round(p * (len(v) - 1))))]
    stats = lambda gpu: {"median": statistics.median(gpu), "p10": pct(gpu, 0.1), "p90": pct(gpu, 0.9)}
    ninf = float("-inf")
    for V, n in WORKLOADS:
        P, N, seg, R0, T0 = make_scene(torch, V, n)
        scenes = torch.tensor([[0, V]], dtype=torch.int32, device="cuda")
        sol, gpu = time_calls(torch, lambda: rap_amd.refine_scene_packed(P, seg, scenes, R0, T0, normals=N, max_iterations=a.iterations,
                                                                         relative_rmse_thr=ninf, max_correspondence_distance=a.gate, max_views=V), a.warmup, a.calls)
        assert int(sol.iterations[0]) == a.iterations and not bool(sol.converged[0]), "the scene stopped early"
        # context: every other view against the first, pairwise, from the same start (R_e = R_v R_0^T, T_e = (T_v - T_0) R_0^T)
        iR = R0[1:] @ R0[0].T
        iT = (T0[1:] - T0[0]) @ R0[0].T
        pair, gpu_pair = time_calls(torch, lambda: rap_amd.icp_packed(P, seg[1:], P, seg[:1].expand(V - 1, 2), iR, iT, max_iterations=a.iterations,
                                                                     relative_rmse_thr=ninf, max_correspondence_distance=a.gate, return_Xt=False,
                                                                     search="grid", estimation="point_to_plane", y_normals=N), a.warmup, a.calls)
        med = statistics.median(gpu)
        lines.append(json.dumps({"workload": f"{V}x{n}", "views": V, "points_per_view": n, "edges": V * (V - 1), "iterations": a.iterations, "gate": a.gate,
                                 "calls": len(gpu), "warmup": a.warmup, "gpu_ms": stats(gpu), "ms_per_iteration": med / a.iterations,
                                 "queries_per_s": a.iterations * V * (V - 1) * n / (med * 1e-3), "rmse": float(sol.rmse[0]),
                                 "pairs_last_iteration": int(sol.edge_count.sum()),
                                 "pairwise_against_anchor": {"problems": V - 1, "gpu_ms": stats(gpu_pair), "mean_rmse": float(pair.rmse.mean())},
                                 "threshold": None}))
        print(lines[-1], flush=True)
        for loss in losses:
            rob, gpu_r = time_calls(torch, lambda: rap_amd.refine_scene_packed(P, seg, scenes, R0, T0, normals=N, max_iterations=a.iterations,
                                                                              relative_rmse_thr=ninf, max_correspondence_distance=a.gate, max_views=V,
                                                                              loss=loss, loss_scale=a.loss_scale), a.warmup, a.calls)
            assert int(rob.iterations[0]) == a.iterations and not bool(rob.converged[0]), "the scene stopped early"
            med_r = statistics.median(gpu_r)
            lines.append(json.dumps({"workload": f"{V}x{n}", "views": V, "points_per_view": n, "edges": V * (V - 1), "iterations": a.iterations,
                                     "gate": a.gate, "loss": loss, "loss_scale": a.loss_scale, "entry_point": "rap_scene_refine_robust",
                                     "calls": len(gpu_r), "warmup": a.warmup, "gpu_ms": stats(gpu_r), "ms_per_iteration": med_r / a.iterations,
                                     "rmse": float(rob.rmse[0]), "pairs_last_iteration": int(rob.edge_count.sum()), "ratio_to_none": med_r / med,
                                     "threshold": None}))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
