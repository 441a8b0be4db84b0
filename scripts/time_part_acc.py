"""Time compute_part_acc (rap_part_acc: one sync-free call for the batch) against the reference's formulation of the same metric run by
torch on the same device: per sample pad the parts, expand to n_parts^2 padded pairs, torch.cdist, masked minima and means, copy the
matrix to the host, scipy.optimize.linear_sum_assignment there (reference eval/metrics.py:125-158 with torch.cdist in pytorch3d's place).

Workloads "BxPxN": B samples of P parts with N/2 .. N points each (lengths drawn per part), predictions = ground truth + 1 mm noise, one
part in five displaced so that it fails the threshold.  Both sides are checked to give the same part_acc and matched_part_ids before
anything is timed: the torch side is tried with torch.cdist, with torch.cdist(compute_mode="donot_use_mm_for_euclid_dist") and with explicit
coordinate differences, in that order, and the first form that agrees with the device call is the one timed ("torch_distance"; the verdict
of every form tried is in "torch_forms_tried").  Per side: wall-clock milliseconds per call between two device synchronisations (the reference's formulation
synchronises inside, so device events alone would not cover it), median and 10th / 90th percentile over --calls after --warmup calls; for
the device call also the HIP-event time.  pair distances = 2 * sum_b N_b^2 for the device call (every point against the other cloud of
its sample, both directions).  Prints one JSON line per workload; --out FILE also writes them.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

WORKLOADS = {"32x20x250": (32, 20, 250), "8x64x128": (8, 64, 128), "4x6x4096": (4, 6, 4096)}


def make_batch(torch, B, P, N, seed=2025):
    g = torch.Generator().manual_seed(seed)
    ppp = torch.randint(N // 2, N + 1, (B, P), generator=g)
    gt, pred = [], []
    for b in range(B):
        for p in range(P):
            n = int(ppp[b, p])
            x = torch.tensor([1.0 * p, 0.0, 0.0]) + (torch.rand(n, 3, generator=g) - 0.5) * 0.4
            y = x + torch.randn(n, 3, generator=g) * 1e-3 + (torch.tensor([0.0, 0.5, 0.0]) if (b + p) % 5 == 0 else 0.0)
            gt.append(x); pred.append(y)
    cu = torch.zeros(B + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(ppp.sum(dim=1), 0).to(torch.int32)
    return torch.cat(gt).cuda(), torch.cat(pred).cuda(), ppp.cuda(), cu.cuda()


def reference_formulation(torch, gt, pred, ppp, cu, threshold, distance="cdist"):
    from scipy.optimize import linear_sum_assignment
    from torch.nn.utils.rnn import pad_sequence
    B, P = ppp.shape
    counts, cu_h = ppp.tolist(), cu.tolist()
    part_acc = torch.zeros(B, device=gt.device)
    matched = torch.zeros(B, P, device=gt.device, dtype=torch.long)
    for b in range(B):
        lens = torch.tensor([c for c in counts[b] if c > 0], device=gt.device)
        xs = [s for s in torch.split(gt[cu_h[b]:cu_h[b + 1]], counts[b]) if s.shape[0] > 0]
        ys = [s for s in torch.split(pred[cu_h[b]:cu_h[b + 1]], counts[b]) if s.shape[0] > 0]
        x, y = pad_sequence(xs, batch_first=True), pad_sequence(ys, batch_first=True)
        n, L, _ = x.shape
        x = x.unsqueeze(1).expand(n, n, L, 3).reshape(-1, L, 3)
        y = y.unsqueeze(0).expand(n, n, L, 3).reshape(-1, L, 3)
        lx, ly = lens.unsqueeze(1).expand(n, n).reshape(-1), lens.unsqueeze(0).expand(n, n).reshape(-1)
        if distance == "cdist":
            d = torch.cdist(x, y) ** 2
        elif distance == "cdist_no_mm":
            d = torch.cdist(x, y, compute_mode="donot_use_mm_for_euclid_dist") ** 2
        else:
            d = ((x[:, :, None, :] - y[:, None, :, :]) ** 2).sum(dim=-1)
        ar = torch.arange(L, device=gt.device)
        mx, my = ar[None, :] < lx[:, None], ar[None, :] < ly[:, None]
        inf = torch.tensor(float("inf"), device=gt.device)
        cx = torch.where(mx, torch.where(my[:, None, :], d, inf).min(dim=2).values, 0.0).sum(dim=1) / lx
        cy = torch.where(my, torch.where(mx[:, :, None], d, inf).min(dim=1).values, 0.0).sum(dim=1) / ly
        cd = (cx + cy).view(n, n)
        rows, cols = linear_sum_assignment((cd >= threshold).float().cpu().numpy())
        part_acc[b] = (cd[rows, cols] < threshold).sum().item() / n
        matched[b, torch.as_tensor(rows, device=gt.device)] = torch.as_tensor(cols, device=gt.device)
    return part_acc, matched


def wall_ms(torch, call, warmup, calls):
    for _ in range(warmup):
        call()
    out = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def event_ms(torch, call, calls):
    out = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", choices=sorted(WORKLOADS) + ["all"], default="all")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--threshold", type=float, default=0.01)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import rap_amd
    assert torch.cuda.is_available(), "time_part_acc.py needs a GPU"
    pct = lambda v, p: sorted(v)[min(len(v) - 1, int(round(p * (len(v) - 1))))]
    stats = lambda v: {"median": statistics.median(v), "p10": pct(v, 0.1), "p90": pct(v, 0.9)}
    lines = []
    for name in (sorted(WORKLOADS) if a.workload == "all" else [a.workload]):
        B, P, N = WORKLOADS[name]
        gt, pred, ppp, cu = make_batch(torch, B, P, N)
        ours = lambda: rap_amd.compute_part_acc(gt, pred, ppp, a.threshold, cu_seqlens_batch=cu)
        acc_o, m_o = ours()
        agrees = {}
        for distance in ("cdist", "cdist_no_mm", "differences"):      # the first form of the torch side that gives the device's answer is timed
            acc_t, m_t = reference_formulation(torch, gt, pred, ppp, cu, a.threshold, distance)
            agrees[distance] = bool(torch.equal(m_o, m_t) and torch.equal(acc_o, acc_t))
            if agrees[distance]:
                break
        assert agrees[distance], f"{name}: the two sides disagree in every form of the torch side: {agrees}"
        theirs = lambda: reference_formulation(torch, gt, pred, ppp, cu, a.threshold, distance)
        w_o, w_t = wall_ms(torch, ours, a.warmup, a.calls), wall_ms(torch, theirs, a.warmup, max(3, a.calls // 4))
        ev = event_ms(torch, ours, a.calls)
        sizes = (cu[1:] - cu[:-1]).double()
        pairs = 2.0 * float((sizes * sizes).sum())
        lines.append(json.dumps({"workload": name, "samples": B, "parts": P, "points": int(cu[-1]), "calls": a.calls, "warmup": a.warmup,
                                 "part_acc_mean": float(acc_o.mean()), "device_call_wall_ms": stats(w_o), "device_call_event_ms": stats(ev),
                                 "torch_scipy_wall_ms": stats(w_t), "torch_distance": distance, "torch_forms_tried": agrees,
                                 "pair_distances": pairs,
                                 "pair_distances_per_s": pairs / (statistics.median(ev) * 1e-3)}))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
