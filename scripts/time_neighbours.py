"""Time the brute-force and the grid-index paths of the neighbourhood calls side by side, in one session:

  normals          estimate_point_normals, 20 neighbours within 0.5, on 20 000 and 200 000 points of the bumpy surface of
                   scripts/time_icp.py (the 20 000-point brute-force row is the one of DESIGN.md section 7.3)
  outliers         remove_statistical_outlier, 20 neighbours, ratio 2.5, on 100 000 and 1 000 000 points of oracle/preproc_cases.py's
                   outlier_cloud (a slab with floating noise: the cloud of tests/test_preproc_scale_gpu.py's raw-scan case)
  knn              k_nearest_neighbors_packed, k = 20, 100 000 queries against 100 000 rows of the surface (grid only: there is no
                   brute-force entry with this result)

Per row: GPU time (HIP events around the call) after --warmup calls, the median and the 10th / 90th percentile over --calls; a call
that takes longer than --slow-ms is timed over 3 calls after 1 instead.  The brute-force kernels are the yardstick.  For the grid rows
"index_ms" is the time of rap_nearest_neighbors for ONE query against the same cloud -- the work-list launch, the nine launches of the
index build and a one-block query, i.e. what the index costs -- and "walk_ms" the rest of the call.  --skip-brute-above N leaves out
the brute-force rows above N points (a million-point outlier call is 10^12 pair distances).  One JSON line per row; --out FILE also
writes them.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

NORMALS_POINTS = (20_000, 200_000)
OUTLIER_POINTS = (100_000, 1_000_000)
KNN_POINTS = 100_000


def time_calls(torch, call, warmup, calls, slow_ms):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = call()
    e1.record()
    torch.cuda.synchronize()
    if e0.elapsed_time(e1) > slow_ms:
        warmup, calls = 1, 3
    for _ in range(max(0, warmup - 1)):
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
    return out, gpu, warmup


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", default="normals,outliers,knn")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--slow-ms", type=float, default=200.0)
    ap.add_argument("--skip-brute-above", type=int, default=1 << 62)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import torch
    import rap_amd
    from rap_amd.point_sampling import remove_statistical_outlier
    from time_icp import make_problems
    lines = []
    pct = lambda v, p: sorted(v)[min(len(v) - 1, int(round(p * (len(v) - 1))))]
    dev = torch.device("cuda:0")
    one = torch.tensor([[0, 1]], dtype=torch.int32, device=dev)

    def index_ms(cloud):
        seg = torch.tensor([[0, cloud.shape[0]]], dtype=torch.int32, device=dev)
        _, gpu, _ = time_calls(torch, lambda: rap_amd.nearest_neighbors_packed(cloud[:1], one, cloud, seg), a.warmup, a.calls, a.slow_ms)
        return statistics.median(gpu)

    def row(workload, points, search, call, cloud, check):
        out, gpu, warm = time_calls(torch, call, a.warmup, a.calls, a.slow_ms)
        med = statistics.median(gpu)
        rec = {"workload": workload, "points": points, "search": search, "calls": len(gpu), "warmup": warm,
               "gpu_ms": {"median": med, "p10": pct(gpu, 0.1), "p90": pct(gpu, 0.9)}, "brute_pair_distances_per_s": float(points) ** 2 / (med * 1e-3)}
        if search == "grid":
            rec["index_ms"] = index_ms(cloud)
            rec["walk_ms"] = med - rec["index_ms"]
        rec.update(check(out))
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        return out

    rows = a.rows.split(",")
    if "normals" in rows:
        for n in NORMALS_POINTS:
            P = make_problems(torch, 1, n)[1][0].contiguous()
            outs = {}
            for search in ("brute", "grid"):
                if search == "brute" and n > a.skip_brute_above:
                    continue
                outs[search] = row("normals", n, search, lambda: rap_amd.estimate_point_normals(P, k_neighbors=20, radius=0.5, search=search), P,
                                   lambda nrm: {"rows_without_a_normal": int((nrm.norm(dim=1) < 0.5).sum())})
            if len(outs) == 2:
                print(json.dumps({"workload": "normals", "points": n, "worst_abs_difference_grid_vs_brute": float((outs["grid"] - outs["brute"]).abs().max())}), flush=True)
    if "outliers" in rows:
        from oracle import preproc_cases as PC
        for n in OUTLIER_POINTS:
            pts = PC.outlier_cloud(n, 3).float().to(dev).contiguous()
            outs = {}
            for search in ("brute", "grid"):
                if search == "brute" and n > a.skip_brute_above:
                    continue
                outs[search] = row("outliers", n, search, lambda: remove_statistical_outlier(pts, 20, 2.5, search=search), pts,
                                   lambda r: {"kept": int(r[1].numel())})
            if len(outs) == 2:
                print(json.dumps({"workload": "outliers", "points": n, "same_index_list": bool(torch.equal(outs["grid"][1], outs["brute"][1]))}), flush=True)
    if "knn" in rows:
        X, Y, _ = make_problems(torch, 1, KNN_POINTS)
        X, Y = X[0].contiguous(), Y[0].contiguous()
        seg = torch.tensor([[0, KNN_POINTS]], dtype=torch.int32, device=dev)
        row("knn", KNN_POINTS, "grid", lambda: rap_amd.k_nearest_neighbors_packed(X, seg, Y, seg, 20), Y,
            lambda r: {"k": 20, "full_lists": int((r[2] == 20).sum())})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
