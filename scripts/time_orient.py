"""Time the consistent normal orientation next to the normal estimation it follows, in one session:

  normals_grid     rap_estimate_normals_grid, 20 neighbours within 0.5 (the row of DESIGN.md section 7.6)
  orient           rap_orient_normals, k = 15, on the normals of that call

both on 20 000 and 200 000 points of the bumpy surface of scripts/time_icp.py, one segment, through the C ABI with the workspace
allocated once.  rap_orient_normals works in place; a second call on its own output builds the same lists, the same weights (|d| does not see
a sign) and the same forest, so the timed calls repeat the first one's work.  Per row: GPU time (HIP events around the call) after
--warmup calls, the median and the 10th / 90th percentile over --calls.  "launches" is the call's launch count, host arithmetic in the
number of points (rounds after the last merge leave at their first instruction, but are launched).  One JSON line per row; --out FILE
also writes them.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

POINTS = (20_000, 200_000)
K = 15


def launches(n):
    rounds = n.bit_length() - 1 if n >= 2 else 0
    jumps = sum(max(1, ((n >> t) - 1).bit_length()) for t in range(rounds))
    return {"rounds": rounds, "launches": 16 + 3 * rounds + jumps}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--slow-ms", type=float, default=200.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import torch
    import rap_amd
    from rap_amd import _lib
    from time_icp import make_problems
    from time_neighbours import time_calls
    lib = _lib.load()
    lines = []
    pct = lambda v, p: sorted(v)[min(len(v) - 1, int(round(p * (len(v) - 1))))]
    dev = torch.device("cuda:0")
    stream = _lib.current_stream(dev)

    def row(workload, points, call, extra):
        _, gpu, warm = time_calls(torch, call, a.warmup, a.calls, a.slow_ms)
        rec = {"workload": workload, "points": points, "calls": len(gpu), "warmup": warm,
               "gpu_ms": {"median": statistics.median(gpu), "p10": pct(gpu, 0.1), "p90": pct(gpu, 0.9)}}
        rec.update(extra())
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for n in POINTS:
        P = make_problems(torch, 1, n)[1][0].contiguous()
        seg = torch.tensor([[0, n]], dtype=torch.int32, device=dev)
        normals = torch.zeros((n, 3), dtype=torch.float32, device=dev)
        comp = torch.empty(n, dtype=torch.int32, device=dev)
        ws = torch.empty(max(lib.rap_normals_grid_workspace_bytes(n, 1), lib.rap_orient_normals_workspace_bytes(n, 1)), dtype=torch.uint8, device=dev)

        def estimate():
            _lib.check(lib.rap_estimate_normals_grid(_lib.ptr(P), _lib.ptr(seg), 1, n, 20, 0.5, None, _lib.ptr(normals), None, _lib.ptr(ws), ws.numel(),
                                                     stream), "rap_estimate_normals_grid")

        def orient():
            _lib.check(lib.rap_orient_normals(_lib.ptr(P), _lib.ptr(seg), 1, n, K, None, _lib.ptr(normals), _lib.ptr(comp), _lib.ptr(ws), ws.numel(),
                                              stream), "rap_orient_normals")

        row("normals_grid", n, estimate, lambda: {"rows_without_a_normal": int((normals.norm(dim=1) < 0.5).sum())})
        independent = normals.clone()
        first = rap_amd.orient_normals_packed(P, independent, seg, k=K)
        row("orient", n, orient, lambda: {"k": K, **launches(n), "components": int(comp[comp >= 0].unique().numel()),
                                          "rows_flipped": int(((normals * independent).sum(dim=1) < 0).sum()),
                                          "same_bits_as_the_first_call": bool(torch.equal(normals.view(torch.int32), first.view(torch.int32))),
                                          "workspace_mib": lib.rap_orient_normals_workspace_bytes(n, 1) / 2 ** 20})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
