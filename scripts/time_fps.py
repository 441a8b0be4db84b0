"""Time the two paths of farthest point sampling side by side, in one session: search="brute"
(rap_farthest_point_sampling: every pick re-reads the cloud; the yardstick) and search="grid" (rap_farthest_point_sampling_grid: the
same index lists over a bucket index), on the bumpy surface of scripts/time_icp.py:

  K =  4 096 of  20 000 points
  K = 20 000 of 100 000 points                     the reference's largest request (demo.py:568-571)
  K =  2 048 of each of 64 clouds x 16 384 points  the row of scripts/kernel_bench.py: do many small clouds lose?
  K = 20 000 of 400 000 points

Per shape the two paths ALTERNATE call by call after --warmup calls of each; GPU time from HIP events around the call; the median and
the 10th / 90th percentile over --calls.  "gpu_ms" is sample_farthest_points as a caller sees it (table uploads, the launch, the gather
of the sampled points); "entry_ms" the C entry point alone on buffers allocated once.  For the grid rows "build_ms" is the entry point
with K = 2 -- bounding box, sort, bucket boxes and the first pick, which opens every bucket -- i.e. what the index costs, and
"build_share" its share of entry_ms.  Every shape also records whether the two paths returned the same index lists.
--sweep times the grid entry point over points per bucket {16, 32, 48, 64, 128} x block size {256, 512, 1024} (rap_set_tuning keys
22 and 23) at the first two shapes.  One JSON line per row; --out FILE also writes them.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

SHAPES = ((1, 20_000, 4_096), (1, 100_000, 20_000), (64, 16_384, 2_048), (1, 400_000, 20_000))      # clouds, points per cloud, K
SWEEP_PER = (16, 32, 48, 64, 128)
SWEEP_BLOCK = (256, 512, 1024)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="0,1,2,3", help="indices into the shape list")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--sweep-calls", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "scripts"))
    import torch
    from rap_amd import _lib
    from rap_amd.point_sampling import sample_farthest_points
    from time_icp import make_problems
    lib = _lib.load()
    dev = torch.device("cuda:0")
    lines = []
    pct = lambda v, p: sorted(v)[min(len(v) - 1, int(round(p * (len(v) - 1))))]
    stats = lambda v: {"median": statistics.median(v), "p10": pct(v, 0.1), "p90": pct(v, 0.9)}

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = call()
        e1.record()
        torch.cuda.synchronize()
        return out, e0.elapsed_time(e1)

    def alternate(calls_by_name, warmup, calls):
        """-> ({name: last output}, {name: [ms]}): warm each, then one call of each in turn, `calls` times"""
        outs, ms = {}, {k: [] for k in calls_by_name}
        for name, call in calls_by_name.items():
            for _ in range(warmup):
                outs[name] = call()
        torch.cuda.synchronize()
        for _ in range(calls):
            for name, call in calls_by_name.items():
                outs[name], t = timed(call)
                ms[name].append(t)
        return outs, ms

    def entries(pts, C, n, K):
        """the two C entry points on buffers allocated once -> {name: call}, each returning its (C, K) int32 indices"""
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
        cs, cl, ks, st = i32([i * n for i in range(C)]), i32([n] * C), i32([K] * C), i32([0] * C)
        flat = pts.reshape(C * n, 3)
        dist = torch.empty(C * n, dtype=torch.float32, device=dev)
        ws = torch.empty(lib.rap_fps_grid_workspace_bytes(C * n, C), dtype=torch.uint8, device=dev)
        out_b, out_g = (torch.empty((C, K), dtype=torch.int32, device=dev) for _ in range(2))
        stream = _lib.current_stream(dev)

        def brute():
            _lib.check(lib.rap_farthest_point_sampling(_lib.ptr(flat), _lib.ptr(cs), _lib.ptr(cl), _lib.ptr(ks), _lib.ptr(st), C, K, _lib.ptr(out_b),
                                                       _lib.ptr(dist), stream), "rap_farthest_point_sampling")
            return out_b

        def grid(k_d=ks):
            _lib.check(lib.rap_farthest_point_sampling_grid(_lib.ptr(flat), C * n, _lib.ptr(cs), _lib.ptr(cl), _lib.ptr(k_d), _lib.ptr(st), C, K,
                                                            _lib.ptr(out_g), _lib.ptr(ws), ws.numel(), stream), "rap_farthest_point_sampling_grid")
            return out_g
        two = i32([2] * C)
        return {"brute": brute, "grid": grid}, lambda: grid(two)

    def params():
        per, cap = ctypes.c_int32(), ctypes.c_int32()
        lib.rap_fps_grid_params(ctypes.byref(per), ctypes.byref(cap))
        return per.value, cap.value

    shapes = [SHAPES[int(i)] for i in a.shapes.split(",") if i != ""]
    for C, n, K in shapes:
        pts = make_problems(torch, C, n)[0].contiguous()
        zeros = torch.zeros(C, dtype=torch.int64)
        api = {s: (lambda s=s: sample_farthest_points(pts, K=K, start_idx=zeros, search=s)) for s in ("brute", "grid")}
        outs, ms = alternate(api, a.warmup, a.calls)
        same = bool(torch.equal(outs["brute"][1], outs["grid"][1]))
        abi, build = entries(pts, C, n, K)
        outs_e, ms_e = alternate(abi, a.warmup, a.calls)
        same = same and bool(torch.equal(outs_e["brute"], outs_e["grid"])) and bool(torch.equal(outs_e["grid"].long(), outs["grid"][1]))
        _, ms_b = alternate({"build": build}, a.warmup, a.calls)
        per, cap = params()
        for s in ("brute", "grid"):
            rec = {"workload": "fps", "clouds": C, "points": n, "K": K, "search": s, "calls": a.calls, "warmup": a.warmup, "gpu_ms": stats(ms[s]),
                   "entry_ms": stats(ms_e[s]), "us_per_pick": statistics.median(ms_e[s]) * 1e3 / K}
            if s == "grid":
                rec.update({"points_per_bucket": per, "max_buckets": cap, "build_ms": stats(ms_b["build"]),
                            "build_share": statistics.median(ms_b["build"]) / statistics.median(ms_e[s])})
            emit(rec)
        emit({"workload": "fps", "clouds": C, "points": n, "K": K, "same_index_lists": same,
              "grid_p90_below_brute_p10": bool(pct(ms_e["grid"], 0.9) < pct(ms_e["brute"], 0.1)),
              "speedup_entry_median": statistics.median(ms_e["brute"]) / statistics.median(ms_e["grid"])})
    if a.sweep:
        per0, _ = params()
        try:
            for C, n, K in SHAPES[:2]:
                pts = make_problems(torch, C, n)[0].contiguous()
                abi, build = entries(pts, C, n, K)
                want = abi["brute"]().clone()
                for block in SWEEP_BLOCK:
                    for per in SWEEP_PER:
                        assert lib.rap_set_tuning(22, per) == 0 and lib.rap_set_tuning(23, block) == 0
                        outs, ms = alternate({"grid": abi["grid"], "build": build}, 2, a.sweep_calls)
                        emit({"workload": "fps sweep", "clouds": C, "points": n, "K": K, "points_per_bucket": per, "block": block, "calls": a.sweep_calls,
                              "entry_ms": stats(ms["grid"]), "build_ms": stats(ms["build"]), "same_index_lists": bool(torch.equal(abi["grid"](), want))})
        finally:
            lib.rap_set_tuning(22, per0)
            lib.rap_set_tuning(23, 512)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
