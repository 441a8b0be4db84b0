"""Time the submap stage on one synthetic drive: --sweeps sweeps of --points points, --submaps submaps of equal length, --groups candidate
groups of four submaps.  GPU: rap_amd.deskew_packed, fuse_frames_packed, submap_overlap_matrix and groups_connected, each timed with HIP
events after --warmup calls (median, 10th and 90th percentile over --calls).  Host: the numpy yardstick (tests/submap_oracle.py) doing
the reference's loop -- one sweep at a time for deskew and fuse, one PAIR at a time for the overlap with each submap cut to 20 000
random points first, as calculate_point_cloud_overlap_ratio_fast does, and a union-find per group.  The host loop is timed on
--host-sweeps sweeps and --host-pairs pairs and scaled to the drive ("host_s_scaled"; "host_s_measured" is what the clock saw).
Prints one JSON line per stage; --out FILE also writes them.  Run it once, under a timeout.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sweeps", type=int, default=200)
    ap.add_argument("--points", type=int, default=60_000)
    ap.add_argument("--submaps", type=int, default=20)
    ap.add_argument("--groups", type=int, default=200)
    ap.add_argument("--voxel", type=float, default=2.0)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-sweeps", type=int, default=8)
    ap.add_argument("--host-pairs", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import rap_amd
    import submap_oracle as O

    F, n, S = a.sweeps, a.points, a.submaps
    rng = np.random.default_rng(11)
    # a drive: 1.2 m and 0.03 rad per sweep; every sweep a disc of 60 m around the sensor, 3 m high
    rel = np.eye(4)
    rel[:3, :3] = O.rotation([0.02, -0.01, 1.0], 0.03)
    rel[:3, 3] = [1.2, 0.04, 0.0]
    poses = [np.eye(4)]
    for _ in range(F - 1):
        poses.append(poses[-1] @ rel)
    pose = np.stack(poses)
    rels = np.stack([np.eye(4)] + [rel] * (F - 1))
    r, ang = 60.0 * np.sqrt(rng.uniform(0, 1, (F, n))), rng.uniform(0, 2 * np.pi, (F, n))
    P = np.stack([r * np.cos(ang), r * np.sin(ang), rng.uniform(-2, 1, (F, n))], axis=-1).astype(np.float32).reshape(-1, 3)
    ts = rng.uniform(0, 0.1, F * n).astype(np.float32)
    cu = (np.arange(F + 1) * n).astype(np.int32)
    sf = np.linspace(0, F, S + 1).round().astype(np.int32)
    groups = np.stack([rng.choice(S, size=4, replace=False) for _ in range(a.groups)]).astype(np.int32)
    lo, hi = 0.05, 0.9

    dev = torch.device("cuda:0")
    tP, tts, tcu, tsf = (torch.from_numpy(x).to(dev) for x in (P, ts, cu, sf))
    trel, tpose, tg = torch.from_numpy(rels).to(dev), torch.from_numpy(pose).to(dev), torch.from_numpy(groups).to(dev)
    tgl = torch.full((a.groups,), 4, dtype=torch.int32, device=dev)
    pct = lambda v, p: sorted(v)[min(len(v) - 1, int(round(p * (len(v) - 1))))]

    def timed(call):
        for _ in range(a.warmup):
            out = call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = call()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return out, {"median": statistics.median(ms), "p10": pct(ms, 0.1), "p90": pct(ms, 0.9)}

    desk, t_desk = timed(lambda: rap_amd.deskew_packed(tP, tts, tcu, trel))
    world, t_fuse = timed(lambda: rap_amd.fuse_frames_packed(desk, tcu, tpose))
    (ratio, nv), t_over = timed(lambda: rap_amd.submap_overlap_matrix(desk, tcu, tsf, a.voxel, pose=tpose))
    ok, t_conn = timed(lambda: rap_amd.groups_connected(ratio, tg, tgl, lo, hi))
    rap_amd.submaps.synchronize()

    # the host loop, on a part of the drive
    hs, hp = min(a.host_sweeps, F), a.host_pairs
    t0 = time.perf_counter()
    hd = [O.deskew(P[cu[k]:cu[k + 1]], ts[cu[k]:cu[k + 1]], rels[k], 0.5) for k in range(F - hs, F)]
    t1 = time.perf_counter()
    hw = [O.transform_points(x, pose[k]) for x, k in zip(hd, range(F - hs, F))]
    t2 = time.perf_counter()
    dw = world.cpu().numpy().astype(np.float64)
    subs = [dw[cu[sf[s]]:cu[sf[s + 1]]] for s in range(S)]
    pairs = [(i, j) for i in range(S) for j in range(i + 1, S)]
    chosen = [pairs[k] for k in rng.choice(len(pairs), size=min(hp, len(pairs)), replace=False)]
    t3 = time.perf_counter()
    for i, j in chosen:
        x, y = (c[rng.choice(len(c), 20000, replace=False)] if len(c) > 20000 else c for c in (subs[i], subs[j]))
        O.overlap_ratio(x, y, a.voxel)
    t4 = time.perf_counter()
    rm = ratio.cpu().numpy()
    verdicts = [O.groups_connected(rm, list(g), lo, hi) for g in groups]
    t5 = time.perf_counter()
    assert verdicts == [bool(v) for v in ok.cpu().numpy()], "connectivity differs from the host's"
    err = np.abs(desk[cu[F - hs]:].cpu().numpy() - np.concatenate(hd)).max()
    assert err < 1e-3, err

    base = {"sweeps": F, "points_per_sweep": n, "submaps": S, "groups": a.groups, "voxel_size": a.voxel, "calls": a.calls, "warmup": a.warmup}
    lines = [
        {"stage": "deskew", **base, "gpu_ms": t_desk, "host_s_measured": t1 - t0, "host_sweeps": hs, "host_s_scaled": (t1 - t0) * F / hs},
        {"stage": "fuse", **base, "gpu_ms": t_fuse, "host_s_measured": t2 - t1, "host_sweeps": hs, "host_s_scaled": (t2 - t1) * F / hs},
        {"stage": "overlap_matrix", **base, "gpu_ms": t_over, "unique_voxels": int(nv.sum()), "host_s_measured": t4 - t3, "host_pairs": len(chosen),
         "host_points_per_cloud": 20000, "host_s_scaled": (t4 - t3) * len(pairs) / len(chosen)},
        {"stage": "groups_connected", **base, "gpu_ms": t_conn, "host_s_measured": t5 - t4, "host_s_scaled": t5 - t4,
         "connected_groups": int(sum(verdicts))},
    ]
    gpu_total = sum(x["gpu_ms"]["median"] for x in lines)
    host_total = sum(x["host_s_scaled"] for x in lines)
    lines.append({"stage": "total", **base, "gpu_ms_median_sum": gpu_total, "host_s_scaled_sum": host_total, "ratio": host_total / (gpu_total * 1e-3)})
    for x in lines:
        print(json.dumps(x), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(json.dumps(x) for x in lines) + "\n")


if __name__ == "__main__":
    main()
