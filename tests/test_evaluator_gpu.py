"""GPU: rap_amd.Evaluator -- the reference's metrics table (eval/evaluator.py:30-250) computed on the device without a host synchronisation --
against the records of the reference's unmodified Evaluator._compute_metrics (tests/golden/evaluator_*.npz, scripts/make_evaluator_golden.py).

The device is held to the FLOAT64 record of the reference; the float32 record ("as shipped") only enters the tolerance:
    max(project tolerance, 4 x |float32 record - float64 record|)
A float32 implementation that orders its sums differently should land within a few times the reference's own float32-to-float64 distance;
a wrong formula does not.  Recall columns and correspondence counts are demanded exactly (the fixture's margins make that fair,
tests/test_evaluator_host.py::test_fixture_margins_hold_on_the_stored_arrays).  Chamfer parity rests on a restated pytorch3d (see the
generator's docstring) and all parity is on synthetic poses."""
import os

import numpy as np
import pytest
import torch

import rap_amd
from conftest import ROOT
from rap_amd import metrics
from rap_amd import synthetic as S

pytestmark = pytest.mark.gpu

DATA_KEYS = ("pointclouds", "pointclouds_gt", "points_per_part", "anchor_parts", "anchor_indices", "scales", "rotations", "translations",
             "cu_seqlens_batch", "cu_seqlens_part")
RUNS = {"off": (False, True, True), "transformed": (True, True, True), "direct": (True, False, True), "noposes": (True, True, False)}


def _fixture(name):
    z = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    z = {k: z[k] for k in z.files}
    dev = torch.device("cuda")
    data = {k: torch.from_numpy(z[k]).to(dev) for k in DATA_KEYS}
    pred = {k: torch.from_numpy(z[k]).to(dev) for k in ("pointclouds_pred", "rotations_pred", "translations_pred")}
    return z, data, pred


def _project_tolerance(key, ref64, scales):
    """Taken from the existing tests of the same quantities."""
    if key == "chamfer_l2 (m)":
        return 2e-6 * scales
    if key == "object_chamfer":
        return np.full_like(scales, 2e-6)
    if key == "average_rotation_error (deg)":
        return np.full_like(scales, 5e-3)
    if key in ("average_translation_error (m)", "transform_error_rmse (m)"):
        return 1e-5 * np.maximum(1.0, scales)
    if key == "rigidity_rmse (m)":
        return 2e-6 * np.abs(ref64)
    if key == "correspondence_rmse (m)":
        return 2e-6 * np.abs(ref64) + 1e-7
    raise KeyError(key)


def _check_table(z, data, pred, run, worst):
    on, transformed, poses = RUNS[run]
    ev = rap_amd.Evaluator(rmse_eval_on=on, rmse_eval_on_transformed=transformed)
    out = ev.compute_metrics(data, pred["pointclouds_pred"], pred["rotations_pred"] if poses else None,
                             pred["translations_pred"] if poses else None)
    assert list(out) == list(z[f"{run}/keys"]), run                           # the reference's keys in the reference's order
    B = data["points_per_part"].shape[0]
    scales = z["scales"].astype(np.float64)
    for key, val in out.items():
        assert val.is_cuda and val.dtype == torch.float32 and tuple(val.shape) == (B,), key
        got = val.double().cpu().numpy()
        r64, r32 = z[f"{run}/f64/{key}"], z[f"{run}/f32/{key}"]
        assert np.array_equal(np.isnan(got), np.isnan(r64)), (run, key, got, r64)
        assert np.array_equal(np.isinf(got), np.isinf(r64)), (run, key, got, r64)
        fin = np.isfinite(r64)
        if key.startswith("recall"):
            assert np.array_equal(got, r64), (run, key, got, r64)
            continue
        if key == "correspondence_ratio":
            n_source = z["points_per_part"][:, 0].astype(np.float64)
            count = np.rint(got * n_source)
            assert np.abs(got * n_source - count).max() < 1e-3
            assert np.array_equal(count.astype(np.int64), z["pair_count64"]), (run, count, z["pair_count64"])
            continue
        with np.errstate(invalid="ignore"):
            own = np.where(np.isfinite(r32) & fin, np.abs(r32 - r64), 0.0)
        tol = np.maximum(_project_tolerance(key, r64, scales), 4.0 * own)
        if not fin.any():                                   # a column of inf only (the transform error in direct mode): placement was checked above
            continue
        with np.errstate(invalid="ignore"):
            dev = np.abs(got - r64)
        print(f"[{run}] {key:32s} worst |device - f64| = {dev[fin].max():.3e}  (tolerance there {tol[fin][dev[fin].argmax()]:.3e}, "
              f"reference's own |f32 - f64| max {own[fin].max():.3e})")
        worst[key] = max(worst.get(key, 0.0), float(dev[fin].max()))
        assert (dev[fin] <= tol[fin]).all(), (run, key, got, r64, tol)
    return out


def test_metrics_table_matches_the_reference_record_pairs():
    """evaluator_pairs, all four runs.  The test prints the worst |device - float64 record| of every column and run
    before it asserts (run with -s)."""
    z, data, pred = _fixture("evaluator_pairs")
    worst = {}
    for run in RUNS:
        out = _check_table(z, data, pred, run, worst)
        if run == "noposes":
            assert list(out) == ["chamfer_l2 (m)", "object_chamfer"]          # the early return of evaluator.py:127-128
    print("worst per column:", {k: f"{v:.2e}" for k, v in worst.items()})
    # the count column of the (B,4) tensor itself
    pm = metrics.compute_pair_metrics(data, data["pointclouds"], pred["rotations_pred"], pred["translations_pred"])
    assert np.array_equal(pm[:, 3].cpu().numpy().astype(np.int64), z["pair_count64"])


def test_metrics_table_matches_the_reference_record_three_parts():
    """evaluator_parts3 (P = 3, empty trailing parts): no pair keys even with rmse_eval_on=True; the other columns as above."""
    z, data, pred = _fixture("evaluator_parts3")
    worst = {}
    for run in RUNS:
        out = _check_table(z, data, pred, run, worst)
        assert not any(k.startswith("correspondence") or "transform_error" in k or "rmse_0.2m" in k for k in out)
    print("worst per column:", {k: f"{v:.2e}" for k, v in worst.items()})


@pytest.mark.parametrize("name", ["evaluator_pairs", "evaluator_parts3"])
def test_transform_errors_direct_matches_the_reference_record(name):
    z, data, pred = _fixture(name)
    mid = torch.from_numpy(z["matched_part_ids"]).cuda()
    for tag, m, sc in (("plain", None, None), ("scaled", None, data["scales"]), ("matched", mid, data["scales"])):
        r, t = metrics.compute_transform_errors_direct(data["rotations"], data["translations"], pred["rotations_pred"],
                                                       pred["translations_pred"], data["points_per_part"], m, sc)
        s = z["scales"].astype(np.float64) if sc is not None else np.ones(len(z["scales"]))
        for got, key, proj in ((r, f"{tag}_rot", np.full_like(s, 5e-3)), (t, f"{tag}_trans", 1e-5 * np.maximum(1.0, s))):
            g = got.double().cpu().numpy()
            r64, r32 = z[f"direct_errors/f64/{key}"], z[f"direct_errors/f32/{key}"]
            assert np.array_equal(np.isnan(g), np.isnan(r64))
            fin = np.isfinite(r64)
            tol = np.maximum(proj, 4.0 * np.where(fin, np.abs(r32 - r64), 0.0))
            print(f"{name} {key}: worst |device - f64| = {np.abs(g - r64)[fin].max():.3e}")
            assert (np.abs(g - r64)[fin] <= tol[fin]).all(), (key, g, r64)


def test_batched_pairs_agree_with_the_single_pair_function():
    """Direct mode against the shipped compute_correspondence_rmse on torch-scaled parts: same count exactly, rmse to 2e-6 relative --
    a contracted x * s - y in the batched kernel would show here."""
    z, data, pred = _fixture("evaluator_pairs")
    pm = metrics.compute_pair_metrics(data, pred["pointclouds_pred"]).cpu().numpy()
    ppp, cu = z["points_per_part"], z["cu_seqlens_batch"]
    sp = torch.repeat_interleave(data["scales"], torch.from_numpy(np.diff(cu)).cuda().long()).view(-1, 1)
    gt_s, pr_s = data["pointclouds_gt"] * sp, pred["pointclouds_pred"] * sp
    for b in range(ppp.shape[0]):
        a, n0, n1 = int(cu[b]), int(ppp[b, 0]), int(ppp[b, 1])
        rmse, n, ratio = metrics.compute_correspondence_rmse(gt_s[a:a + n0], gt_s[a + n0:a + n0 + n1], pr_s[a:a + n0], pr_s[a + n0:a + n0 + n1],
                                                             0.05)
        assert int(pm[b, 3]) == n, (b, pm[b], n)
        assert pm[b, 1] == np.float32(ratio)
        if n == 0:
            assert np.isinf(pm[b, 0]) and np.isinf(float(rmse))
        else:
            assert abs(float(pm[b, 0]) - float(rmse)) <= 2e-6 * float(rmse), (b, pm[b, 0], float(rmse))
        assert np.isinf(pm[b, 2])                                         # no transform error without predicted poses


def _full_geometry(B=32, n=4096, seed=99):
    """32 pairs x 2 x 4096: the second view IS the first view (same points, its own frame), poses exact."""
    g = torch.Generator().manual_seed(seed)
    pts = torch.rand(B, n, 3, generator=g) - 0.5
    R = torch.stack([torch.stack([torch.eye(3, dtype=torch.float64), S._random_rotation(g)]) for _ in range(B)]).float()      # (B,2,3,3)
    t = torch.stack([torch.stack([torch.zeros(3), torch.rand(3, generator=g) - 0.5]) for _ in range(B)]).float()
    gt = torch.stack([pts, pts], dim=1)                                                                # (B,2,n,3)
    cond = torch.einsum("bpni,bpij->bpnj", gt - t[:, :, None, :], R)                                   # gt = cond @ R^T + t
    scales = torch.rand(B, generator=g) * 45 + 5
    dev = torch.device("cuda")
    anchor = torch.zeros(B, 2, dtype=torch.bool); anchor[:, 0] = True
    data = {"pointclouds": cond.reshape(-1, 3).to(dev), "pointclouds_gt": gt.reshape(-1, 3).contiguous().to(dev),
            "points_per_part": torch.full((B, 2), n, dtype=torch.int64, device=dev), "anchor_parts": anchor.to(dev),
            "scales": scales.to(dev), "rotations": R.to(dev), "translations": t.to(dev),
            "cu_seqlens_batch": (torch.arange(B + 1, dtype=torch.int32) * 2 * n).to(dev)}
    return data


def test_full_geometry_properties():
    data = _full_geometry()
    s = data["scales"].double().cpu().numpy()
    R, t = data["rotations"], data["translations"]
    pm = metrics.compute_pair_metrics(data, data["pointclouds"], R, t).double().cpu().numpy()
    print("identical views: worst rmse / scale", (pm[:, 0] / s).max(), "worst transform error / scale", (pm[:, 2] / s).max())
    assert (pm[:, 1] == 1.0).all() and (pm[:, 3] == 4096).all()
    assert (pm[:, 0] < 1e-5 * s).all() and (pm[:, 2] < 1e-5 * s).all()
    # a pure translation error d on the target pose, d * s >= 0.1 m
    d = torch.tensor([0.03, -0.02, 0.01], device="cuda")
    t_off = t.clone(); t_off[:, 1] += d
    ds = float(d.double().norm()) * s
    assert ds.min() >= 0.1
    pm = metrics.compute_pair_metrics(data, data["pointclouds"], R, t_off).double().cpu().numpy()
    print("translation error: worst relative rmse", (np.abs(pm[:, 0] - ds) / ds).max(), "transform error", (np.abs(pm[:, 2] - ds) / ds).max())
    assert (pm[:, 1] == 1.0).all()
    assert (np.abs(pm[:, 0] - ds) <= 1e-5 * ds).all() and (np.abs(pm[:, 2] - ds) <= 1e-4 * ds).all()
    # views 10 units apart: no correspondence
    far = dict(data)
    gt = data["pointclouds_gt"].view(32, 2, 4096, 3).clone(); gt[:, 1, :, 0] += 10.0
    far["pointclouds_gt"] = gt.view(-1, 3)
    pm = metrics.compute_pair_metrics(far, data["pointclouds"], R, t).cpu().numpy()
    assert np.isinf(pm[:, 0]).all() and (pm[:, 1] == 0).all() and (pm[:, 3] == 0).all() and np.isfinite(pm[:, 2]).all()


def test_metrics_are_deterministic():
    z, data, pred = _fixture("evaluator_pairs")
    ev = rap_amd.Evaluator(rmse_eval_on=True)
    a = ev.compute_metrics(data, pred["pointclouds_pred"], pred["rotations_pred"], pred["translations_pred"])
    b = ev.compute_metrics(data, pred["pointclouds_pred"], pred["rotations_pred"], pred["translations_pred"])
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k       # bitwise, NaN included
    full = _full_geometry()
    p = metrics.compute_pair_metrics(full, full["pointclouds"], full["rotations"], full["translations"])
    q = metrics.compute_pair_metrics(full, full["pointclouds"], full["rotations"], full["translations"])
    assert torch.equal(p.view(torch.int32), q.view(torch.int32))


def test_compute_metrics_makes_no_host_synchronisation():
    z, data, pred = _fixture("evaluator_pairs")
    data = dict(data)
    data["anchor_parts"] = data["anchor_parts"].to(torch.uint8)              # every input on the device in its final dtype
    ev = rap_amd.Evaluator(rmse_eval_on=True)
    warm = ev.compute_metrics(data, pred["pointclouds_pred"], pred["rotations_pred"], pred["translations_pred"])      # workspace cached
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            warm["chamfer_l2 (m)"][0].item()                                 # the mode does catch a synchronisation on this build
        out = ev.compute_metrics(data, pred["pointclouds_pred"], pred["rotations_pred"], pred["translations_pred"])
        direct = rap_amd.Evaluator(rmse_eval_on=True, rmse_eval_on_transformed=False).compute_metrics(
            data, pred["pointclouds_pred"], pred["rotations_pred"], pred["translations_pred"])
        metrics.compute_transform_errors_direct(data["rotations"], data["translations"], pred["rotations_pred"], pred["translations_pred"],
                                                data["points_per_part"], None, data["scales"])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for k in warm:
        assert torch.equal(out[k].view(torch.int32), warm[k].view(torch.int32)), k
    assert len(direct) == len(out)


def test_refusals():
    from rap_amd._lib import RapError
    z, data, pred = _fixture("evaluator_parts3")
    with pytest.raises(ValueError):
        metrics.compute_pair_metrics(data, data["pointclouds"], pred["rotations_pred"], pred["translations_pred"])      # P = 3
    z, data, pred = _fixture("evaluator_pairs")
    cpu = {k: v.cpu() for k, v in data.items()}
    with pytest.raises(RapError):
        metrics.compute_pair_metrics(cpu, cpu["pointclouds"])
    with pytest.raises(RapError):
        rap_amd.Evaluator().compute_metrics(cpu, pred["pointclouds_pred"].cpu())
    eye = torch.eye(3, device="cuda")
    with pytest.raises(NotImplementedError):
        metrics.compute_approximate_transform_error(eye, torch.zeros(3, device="cuda"), 2.0 * torch.eye(6))
    with pytest.raises(NotImplementedError, match="save_transformation_files"):
        rap_amd.Evaluator().run(data, pred["pointclouds_pred"], save_results=True)
    # the identity covariance is the supported one; a rotation by 90 degrees about z has |q_xyz|^2 = 1 / 2
    Rz = torch.tensor([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]], device="cuda")
    v = metrics.compute_approximate_transform_error(torch.stack([eye, Rz]), torch.tensor([[0.0, 0.0, 0.0], [3.0, 0.0, 4.0]], device="cuda"),
                                                    np.eye(6, dtype=np.float32))
    assert torch.allclose(v.cpu(), torch.tensor([0.0, 25.5]), atol=1e-6)
    # run() without saving is the table
    out = rap_amd.Evaluator(rmse_eval_on=True).run(data, pred["pointclouds_pred"], pred["rotations_pred"], pred["translations_pred"])
    assert "transform_error_rmse (m)" in out
