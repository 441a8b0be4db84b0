"""Fixtures of the evaluator's metrics table: tests/golden/evaluator_pairs.npz, tests/golden/evaluator_parts3.npz.

The yardstick is the reference's UNMODIFIED ``Evaluator._compute_metrics`` (rectified_point_flow/eval/evaluator.py:30-250), imported
through ``oracle.ref_loader.load_reference_evaluator()`` and called on an instance made with ``object.__new__`` (it reads only
``rmse_eval_on`` and ``rmse_eval_on_transformed``).  Needs the reference mounted; writes arrays only.

pytorch3d is absent, so ``chamfer_distance`` in the reference metrics module's globals is bound to a float64 brute-force restatement of its
documented result (mean_i min_j |x_i - y_j|^2 + mean_j min_i |y_j - x_i|^2) -- the same stand-in status ``oracle.rap_oracle.compute_cd``
has: chamfer PARITY IS UNPINNED for that one call, everything else is the reference's own code.

Every case is recorded twice: with float32 inputs ("f32", the reference as shipped) and with all floating inputs cast to float64 ("f64").
The f64 record is what the device is held to; the f32 record shows how far the reference is from itself.  The reference's
``compute_transform_errors_direct`` (plain, with scale, with matched_part_ids) is recorded the same two ways on the fixture's poses.

Before writing, the script asserts the margins that keep exact checks honest (``check_margins``; tests/test_evaluator_host.py re-checks
them on the stored arrays) and re-draws a sample with another seed until they hold:
  * every thresholded value is at least 1e-3 (relative) away from every threshold it is compared with, or is NaN / inf;
  * no source point's fp64 nearest distance lies within 2e-5 m of the 0.05 m threshold, and for every source point within the threshold
    the nearest and second-nearest target differ by more than 2e-5 m (coordinates reach 50 m, one fp32 ulp there is 3.8e-6 m, a
    direct-difference distance of rounded coordinates is off by at most about 7e-6 m).

usage: python scripts/make_evaluator_golden.py
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAIR_THRESHOLD = 0.05
NN_MARGIN = 2e-5
REL_MARGIN = 1e-3
THRESHOLDS = {"average_rotation_error (deg)": (5.0, 10.0, 15.0), "average_translation_error (m)": (0.2, 0.3, 2.0, 5.0),
              "chamfer_l2 (m)": (0.2,), "correspondence_rmse (m)": (0.2,), "transform_error_rmse (m)": (0.2,)}
FLOAT_KEYS = ("pointclouds", "pointclouds_gt", "scales", "rotations", "translations")
RUNS = {"off": (False, True, True), "transformed": (True, True, True), "direct": (True, False, True), "noposes": (True, True, False)}


def axis_angle(axis, deg):
    a = torch.as_tensor(axis, dtype=torch.float64)
    a = a / a.norm()
    th = math.radians(deg)
    K = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=torch.float64)
    return torch.eye(3, dtype=torch.float64) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


def random_rotation(g):
    q = torch.randn(4, generator=g, dtype=torch.float64)
    w, x, y, z = (q / q.norm()).tolist()
    return torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], dtype=torch.float64)


def surface(xy):
    x, y = xy[:, 0], xy[:, 1]
    return torch.stack([x, y, 0.1 * torch.sin(5 * x) * torch.cos(4 * y) + 0.05 * x], dim=1)


def make_views(sizes, scale, g, far=False):
    """Views of one smooth surface inside [-0.5, 0.5]^3 (normalised units).  View 0 is a random sample; every later view holds, for
    about 60 % of view 0's points, a neighbour on the surface 2 mm ... 9 cm (in metres, i.e. / scale) away, the rest fresh samples --
    so that about half of the source points have a correspondence within 5 cm whatever the scale."""
    views = []
    base = None
    for p, n in enumerate(sizes):
        if n == 0:
            views.append(torch.zeros(0, 3, dtype=torch.float64)); continue
        xy = torch.rand(n, 2, generator=g, dtype=torch.float64) * 0.9 - 0.45
        if base is None:
            base = xy
        else:
            m = min(n, int(round(0.6 * base.shape[0])) or 1)
            pick = torch.randperm(base.shape[0], generator=g)[:m]
            r = (torch.rand(m, generator=g, dtype=torch.float64) * 0.088 + 0.002) / scale
            phi = torch.rand(m, generator=g, dtype=torch.float64) * 2 * math.pi
            xy[:m] = base[pick] + torch.stack([r * torch.cos(phi), r * torch.sin(phi)], dim=1)
            xy = xy[torch.randperm(n, generator=g)]
        v = surface(xy)
        if far and p > 0:
            v = v + torch.tensor([2.0, 0.0, 0.0], dtype=torch.float64)
        views.append(v)
    return views


def make_sample(spec, g):
    """-> cond, gt, pred (n,3), R_gt, t_gt, R_pred, t_pred (P,...) float64, anchor (P,) bool;  gt = cond @ R_gt^T + t_gt."""
    sizes, scale, anchor = spec["sizes"], spec["scale"], spec.get("anchor", 0)
    P = len(sizes)
    views = make_views(sizes, scale, g, spec.get("far", False))
    cond, gt, pred = [], [], []
    Rg, tg, Rp, tp = (torch.zeros(P, 3, 3, dtype=torch.float64), torch.zeros(P, 3, dtype=torch.float64),
                      torch.zeros(P, 3, 3, dtype=torch.float64), torch.zeros(P, 3, dtype=torch.float64))
    for p, v in enumerate(views):
        axis = torch.randn(3, generator=g, dtype=torch.float64)
        tdir = torch.randn(3, generator=g, dtype=torch.float64); tdir = tdir / tdir.norm()
        if p == anchor:                                     # the anchor keeps its pose and is predicted almost exactly
            R, t = torch.eye(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64)
            Rerr, terr = axis_angle(axis, 0.05), tdir * 1e-4 / scale
        else:
            R, t = random_rotation(g), (v.mean(0) if v.shape[0] else torch.zeros(3, dtype=torch.float64))
            Rerr, terr = axis_angle(axis, spec["rot_deg"]), tdir * spec["trans_m"] / scale
        Rg[p], tg[p] = R, t
        Rp[p], tp[p] = R @ Rerr, t + terr                   # predicted rotation = GT x a rotation of rot_deg
        c = (v - t) @ R                                     # gt = c @ R^T + t
        cond.append(c); gt.append(v)
        # residual of the predicted cloud against its own pose: 3e-3 normalised units per coordinate whatever the scale.  The rigidity
        # kernels (and the reference's float32 run) round coordinates of size 0.5 to 3e-8; a residual d sees that as e / d per
        # coordinate and e / (d sqrt(3 n)) in the RMSE over n points -- 2e-7 for d = 5e-3 and n = 150, a tenth of the 2e-6 the
        # rigidity column is held to.  A residual of millimetres at scale 50 (4e-5 units) would put the float32 floor itself at 2e-5.
        pred.append(c @ Rp[p].T + tp[p] + torch.randn(v.shape, generator=g, dtype=torch.float64) * 3e-3)
    anc = torch.zeros(P, dtype=torch.bool); anc[anchor] = True
    return torch.cat(cond), torch.cat(gt), torch.cat(pred), Rg, tg, Rp, tp, anc


def nn_margin_ok(gt32, sizes, scale32):
    """The NN margin conditions of one pair, on the fp64 distances of the fp32 inputs scaled in fp64 (what the f64 record sees)."""
    n0, n1 = sizes[0], sizes[1]
    if n0 == 0 or n1 == 0:
        return True
    s = gt32[:n0].double() * float(scale32)
    t = gt32[n0:n0 + n1].double() * float(scale32)
    d = torch.cdist(s, t, p=2, compute_mode="donot_use_mm_for_euclid_dist")
    k = d.topk(min(2, n1), dim=1, largest=False).values
    if bool(((k[:, 0] - PAIR_THRESHOLD).abs() <= NN_MARGIN).any()):
        return False
    if n1 > 1:
        inside = k[:, 0] <= PAIR_THRESHOLD
        if bool((inside & ((k[:, 1] - k[:, 0]) <= NN_MARGIN)).any()):
            return False
    return True


def build_batch(specs, seed):
    P = max(len(s["sizes"]) for s in specs)
    rows = []
    for b, spec in enumerate(specs):
        for attempt in range(200):
            g = torch.Generator().manual_seed(seed * 100003 + b * 1009 + attempt)
            smp = make_sample(spec, g)
            if P != 2 or nn_margin_ok(smp[1].float(), spec["sizes"], torch.tensor(spec["scale"], dtype=torch.float32)):
                break
        else:
            raise RuntimeError(f"sample {b}: no draw met the nearest-neighbour margins")
        rows.append(smp)
    lens = [r[0].shape[0] for r in rows]
    cu = torch.zeros(len(specs) + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(torch.tensor(lens), 0).to(torch.int32)
    ppp = torch.tensor([s["sizes"] for s in specs], dtype=torch.int64)
    anchor_parts = torch.stack([r[7] for r in rows])
    anchor_indices = torch.cat([torch.repeat_interleave(r[7], ppp[b]) for b, r in enumerate(rows)])
    cu_part = torch.zeros(ppp.numel() + 1, dtype=torch.int32)
    cu_part[1:] = torch.cumsum(ppp.reshape(-1), 0).to(torch.int32)
    data = {"pointclouds": torch.cat([r[0] for r in rows]).float(), "pointclouds_gt": torch.cat([r[1] for r in rows]).float(),
            "points_per_part": ppp, "anchor_parts": anchor_parts, "anchor_indices": anchor_indices,
            "scales": torch.tensor([s["scale"] for s in specs], dtype=torch.float32),
            "rotations": torch.stack([r[3] for r in rows]).float(), "translations": torch.stack([r[4] for r in rows]).float(),
            "cu_seqlens_batch": cu, "cu_seqlens_part": cu_part}
    pred = {"pointclouds_pred": torch.cat([r[2] for r in rows]).float(), "rotations_pred": torch.stack([r[5] for r in rows]).float(),
            "translations_pred": torch.stack([r[6] for r in rows]).float()}
    return data, pred


def chamfer_stand_in(x, y, single_directional=False, norm=2, point_reduction="mean", **kw):
    """pytorch3d.loss.chamfer.chamfer_distance as compute_cd calls it (metrics.py:37-43), float64 brute force; parity unpinned."""
    assert not single_directional and norm == 2 and point_reduction == "mean" and x.shape[0] == 1 and y.shape[0] == 1
    d = torch.cdist(x[0].double(), y[0].double(), p=2, compute_mode="donot_use_mm_for_euclid_dist") ** 2
    return (d.min(dim=1).values.mean() + d.min(dim=0).values.mean()).to(x.dtype), None


def load_reference():
    from oracle import ref_loader
    ev = ref_loader.load_reference_evaluator()
    mod = sys.modules["rectified_point_flow.eval.metrics"]
    mod.chamfer_distance = chamfer_stand_in
    return ev, mod


def cast(d, dtype):
    return {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in d.items()}


def run_reference(ev, data, pred, rmse_eval_on, transformed, with_poses, dtype):
    inst = object.__new__(ev.Evaluator)
    inst.rmse_eval_on, inst.rmse_eval_on_transformed = rmse_eval_on, transformed
    d, p = cast(data, dtype), cast(pred, dtype)
    with torch.no_grad():
        out = inst._compute_metrics(d, p["pointclouds_pred"], p["rotations_pred"] if with_poses else None,
                                    p["translations_pred"] if with_poses else None)
    return {k: v.detach().double().numpy() for k, v in out.items()}


def matched_ids(ppp):
    B, P = ppp.shape
    return torch.stack([torch.roll(torch.arange(P), b + 1) for b in range(B)]).to(torch.int64)


def run_direct(mod, data, pred, dtype):
    d, p = cast(data, dtype), cast(pred, dtype)
    mid = matched_ids(data["points_per_part"])
    out = {}
    for tag, m, sc in (("plain", None, None), ("scaled", None, d["scales"]), ("matched", mid, d["scales"])):
        r, t = mod.compute_transform_errors_direct(d["rotations"], d["translations"], p["rotations_pred"], p["translations_pred"],
                                                   data["points_per_part"], m, sc)
        out[f"{tag}_rot"], out[f"{tag}_trans"] = r.double().numpy(), t.double().numpy()
    return out, mid


def check_margins(records):
    """records: {run: {key: (B,) float64}} of the f64 pass."""
    for run, rec in records.items():
        for key, thresholds in THRESHOLDS.items():
            if key not in rec:
                continue
            v = rec[key]
            for thr in thresholds:
                ok = ~np.isfinite(v) | (np.abs(v - thr) >= REL_MARGIN * thr)
                assert ok.all(), f"{run} / {key}: {v} too close to {thr}"


def pair_counts(data):
    """fp64 number of correspondences per pair (the yardstick of the exact count check)."""
    ppp, cu, gt, sc = data["points_per_part"], data["cu_seqlens_batch"], data["pointclouds_gt"], data["scales"]
    out = []
    for b in range(ppp.shape[0]):
        n0, n1, a = int(ppp[b, 0]), int(ppp[b, 1]), int(cu[b])
        if n0 == 0 or n1 == 0:
            out.append(0); continue
        s, t = gt[a:a + n0].double() * float(sc[b]), gt[a + n0:a + n0 + n1].double() * float(sc[b])
        d = torch.cdist(s, t, p=2, compute_mode="donot_use_mm_for_euclid_dist").min(dim=1).values
        out.append(int((d <= PAIR_THRESHOLD).sum()))
    return np.asarray(out, dtype=np.int64)


def write_case(name, specs, seed, ev, mod):
    data, pred = build_batch(specs, seed)
    arrays = {k: v.numpy() for k, v in {**data, **pred}.items()}
    rec64 = {}
    for run, (on, transformed, poses) in RUNS.items():
        for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            rec = run_reference(ev, data, pred, on, transformed, poses, dtype)
            arrays[f"{run}/keys"] = np.asarray(list(rec.keys()))
            for k, v in rec.items():
                arrays[f"{run}/{tag}/{k}"] = v
            if tag == "f64":
                rec64[run] = rec
    check_margins(rec64)
    for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        out, mid = run_direct(mod, data, pred, dtype)
        for k, v in out.items():
            arrays[f"direct_errors/{tag}/{k}"] = v
    arrays["matched_part_ids"] = mid.numpy()
    if data["points_per_part"].shape[1] == 2:
        arrays["pair_count64"] = pair_counts(data)
    path = os.path.join(ROOT, "tests", "golden", f"{name}.npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size < 1_000_000, f"{path}: {size} bytes"
    print(f"{path}: {size} bytes, {len(arrays)} arrays")
    for run, rec in rec64.items():
        print(f"  [{run}]")
        for k, v in rec.items():
            print(f"    {k:45s} {np.array2string(v, precision=4, max_line_width=200)}")
    return arrays


PAIRS = [
    dict(sizes=[4096, 4096], scale=10.0, rot_deg=0.3, trans_m=0.001),
    dict(sizes=[900, 1100], scale=1.0, rot_deg=2.0, trans_m=0.01),
    dict(sizes=[257, 255], scale=50.0, rot_deg=4.0, trans_m=1.0),
    dict(sizes=[1, 300], scale=5.0, rot_deg=8.0, trans_m=0.25),
    dict(sizes=[700, 0], scale=20.0, rot_deg=12.0, trans_m=0.5),                 # empty target
    dict(sizes=[600, 500], scale=30.0, rot_deg=20.0, trans_m=1.5, anchor=1),    # the anchor is part 1
    dict(sizes=[800, 800], scale=7.5, rot_deg=90.0, trans_m=3.0, far=True),     # views far apart: no correspondence
    dict(sizes=[1500, 1300], scale=2.5, rot_deg=170.0, trans_m=6.0),
]
PARTS3 = [
    dict(sizes=[400, 300, 0], scale=5.0, rot_deg=1.0, trans_m=0.02),
    dict(sizes=[256, 256, 256], scale=12.0, rot_deg=6.0, trans_m=0.25),
    dict(sizes=[100, 50, 0], scale=40.0, rot_deg=30.0, trans_m=4.0),
]


def main():
    ev, mod = load_reference()
    write_case("evaluator_pairs", PAIRS, 7, ev, mod)
    write_case("evaluator_parts3", PARTS3, 11, ev, mod)


if __name__ == "__main__":
    main()
