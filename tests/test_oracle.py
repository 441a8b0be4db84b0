"""CPU: the oracle (oracle/rap_oracle.py) against the golden vectors produced by the reference's own
modules (the `*_live_reference*` tests: fixtures of small direct calls into them) and against analytic known-answer tests."""
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_CASES, LATENT_CASES, MODEL_SIZE_CASES, SWITCH_CASES, load_golden
from oracle import rap_oracle as O
from rap_amd import synthetic as S


def _cfg(g, name=None):
    cfg = dict(S.RAP_12)
    cfg["num_layers"] = int(g["num_layers"])
    cfg.update(SWITCH_CASES.get(name, {}))
    cfg.update(LATENT_CASES.get(name, {}))
    return cfg


@pytest.mark.parametrize("name", GOLDEN_CASES + MODEL_SIZE_CASES + list(SWITCH_CASES) + list(LATENT_CASES))
def test_oracle_matches_reference_golden(name):
    g, inp = load_golden(name)
    cfg = _cfg(g, name)
    sd = S.make_weights(cfg, int(g["weight_seed"]))
    chk = float(sum(v.double().sum().item() for v in sd.values()))
    assert abs(chk - float(g["weights_checksum"])) < 1e-6, "seeded weights differ from the ones the golden was made with"
    # inputs regenerate bit-identically from the seed-independent generator? (the fixture stores them anyway)
    out = O.sample(sd, cfg, inp, int(g["num_steps"]), bool(g["rigidity"]))
    for k in ("end_point_trajectory", "trajectory", "R", "t"):
        ref = torch.from_numpy(g[k])
        err = float((out[k] - ref).abs().max())
        assert err < 5e-6, (k, err)
    if "sample_features" in g:         # transformer_features out of the sampling call (round 3; modeling.py:678-695)
        f_ref = torch.from_numpy(g["sample_features"])
        assert float(g["sample_features_timestep"]) == pytest.approx(1.0 / int(g["num_steps"]))
        assert float((out["transformer_features"] - f_ref).abs().max()) < 2e-5 * max(1.0, float(f_ref.abs().max()))
    cu_b, cu_p = O.prepare_cu_seqlens(inp)
    fw = O.dit_forward(sd, cfg, inp["x_1"], torch.from_numpy(g["fwd_timesteps"]), inp["pointclouds"], inp["features"],
                       inp["scales"], inp["anchor_indices"], cu_b, cu_p, return_transformer_features=True, latent=inp.get("latent_features"))
    assert float((fw["velocity"] - torch.from_numpy(g["fwd_velocity"])).abs().max()) < 2e-6
    assert float((fw["transformer_features"] - torch.from_numpy(g["fwd_features"])).abs().max()) < 2e-5


def test_oracle_matches_reference_at_configs0_in_full():
    """BASELINE configs[0] -- the reference's own CPU-runnable case -- in full: demo pair (2 views x 1024 points), rap_12, all 10 Euler
    steps with rigidity forcing.  tests/golden/headline_c0_rigid.npz is the UNMODIFIED reference's output (make_golden.py
    --headline-only --c0: final clouds, poses, per-step maxima and every 8th point of every step); the oracle must reproduce it."""
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "headline_c0_rigid.npz"))
    g = {k: z[k] for k in z.files}
    cfg = dict(S.RAP_12)
    sd = S.make_weights(cfg, int(g["weight_seed"]))
    assert abs(float(sum(v.double().sum().item() for v in sd.values())) - float(g["weights_checksum"])) < 1e-6
    inp = S.make_uniform_inputs(1, int(g["views"]), int(g["points"]), seed=int(g["input_seed"]))
    out = O.sample(sd, cfg, inp, int(g["num_steps"]), bool(g["rigidity"]))
    st = int(g["stride"])
    errs = {"final_end_point": float((out["end_point_trajectory"][-1] - torch.from_numpy(g["final_end_point"])).abs().max()),
            "final_x_t": float((out["trajectory"][-1] - torch.from_numpy(g["final_x_t"])).abs().max()),
            "end_point_steps": float((out["end_point_trajectory"][:, ::st] - torch.from_numpy(g["end_point_strided"])).abs().max()),
            "x_t_steps": float((out["trajectory"][:, ::st] - torch.from_numpy(g["x_t_strided"])).abs().max()),
            "R": float((out["R"] - torch.from_numpy(g["R"])).abs().max()), "t": float((out["t"] - torch.from_numpy(g["t"])).abs().max())}
    print("oracle vs reference, configs[0] in full:", errs)
    assert max(errs.values()) < 1e-5, errs


def _live_checks():
    """What the reference's own modules returned for the small cases below (oracle/make_golden.py --live-checks-only: the inputs
    are regenerated from the seeds of its *_check_inputs helpers)."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "live_reference_checks.npz"))
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("switch", [{}] + list(SWITCH_CASES.values()) + list(LATENT_CASES.values()),
                         ids=["shipped-config"] + list(SWITCH_CASES) + list(LATENT_CASES))
def test_oracle_matches_live_reference_modules(switch, request):
    from oracle.make_golden import FEATURE_ROW_STRIDE, live_check_inputs
    name = request.node.callspec.id
    z = _live_checks()
    cfg, sd, inp = live_check_inputs(switch)
    assert abs(float(sum(v.double().sum().item() for v in sd.values())) - float(z[f"model_{name}_weights_checksum"])) < 1e-6
    assert abs(sum(float(v.double().sum()) for v in inp.values()) - float(z[f"model_{name}_inputs_checksum"])) < 1e-6
    for rigid in ((False, True) if not switch else (True,)):
        tag = f"model_{name}_{'rigid' if rigid else 'free'}"
        ref = {k: torch.from_numpy(z[f"{tag}_{k}"]) for k in ("end_point_trajectory", "trajectory", "R", "t")}
        mine = O.sample(sd, cfg, inp, 3, rigid)
        for k in ("end_point_trajectory", "trajectory", "R", "t"):
            assert float((ref[k] - mine[k]).abs().max()) < 5e-6, (rigid, k)
        # the features the sampling call captures on its last model call (modeling.py:678-695): same call index, same values --
        # every FEATURE_ROW_STRIDE-th token row element by element, every row through its norm (the bound the element-wise one implies)
        assert float(z[f"{tag}_features_timestep"]) == pytest.approx(1.0 / 3.0)
        f = mine["transformer_features"]
        tol = 2e-5 * max(1.0, float(z[f"{tag}_features_absmax"]))
        assert abs(float(f.abs().max()) - float(z[f"{tag}_features_absmax"])) < tol, rigid
        assert float((torch.from_numpy(z[f"{tag}_features_rows"]) - f[::FEATURE_ROW_STRIDE]).abs().max()) < tol, rigid
        norms = torch.linalg.vector_norm(f.double(), dim=1)
        assert norms.shape[0] == z[f"{tag}_features_row_norms"].shape[0]
        assert float((torch.from_numpy(z[f"{tag}_features_row_norms"]) - norms).abs().max()) < tol * f.shape[1] ** 0.5, rigid


def test_fp32_oracle_vs_fp64_ground_truth_sets_the_tolerance_scale():
    cfg = dict(S.RAP_12); cfg["num_layers"] = 2
    sd = S.make_weights(cfg, 0)
    inp = S.make_inputs([[37, 64, 100], [50, 129]], seed=7)
    a = O.sample(sd, cfg, inp, 4, True)
    b = O.sample(sd, cfg, inp, 4, True, dtype=torch.float64)
    assert float((a["end_point_trajectory"].double() - b["end_point_trajectory"]).abs().max()) < 1e-5
    assert float((a["R"].double() - b["R"]).abs().max()) < 1e-5


# ---------------- analytic known-answer tests ----------------
def test_kat_posenc_against_math_sin():
    x = torch.tensor([[0.3, -1.7, 2.9]], dtype=torch.float64)
    pe = O.posenc(x)
    assert pe.shape == (1, 63)
    assert torch.equal(pe[0, :3], x[0])
    for k in range(10):
        for c in range(3):
            assert abs(pe[0, 3 + 6 * k + c].item() - math.sin(2.0 ** k * x[0, c].item())) < 1e-12
            assert abs(pe[0, 3 + 6 * k + 3 + c].item() - math.cos(2.0 ** k * x[0, c].item())) < 1e-12


def test_kat_procrustes_exact_recovery_and_reflection_case():
    g = torch.Generator().manual_seed(5)
    src = torch.randn(50, 3, generator=g, dtype=torch.float64)
    q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
    if torch.det(q) < 0:
        q[:, 0] *= -1
    t0 = torch.tensor([0.3, -0.2, 1.0], dtype=torch.float64)
    R, t = O.solve_procrustes(src, src @ q.T + t0)
    assert float((R - q).abs().max()) < 1e-12 and float((t - t0).abs().max()) < 1e-12
    # planar source + mirrored target: the det fix must return a proper rotation
    src[:, 2] = 0
    mirror = torch.diag(torch.tensor([1.0, 1.0, -1.0], dtype=torch.float64))
    R, _ = O.solve_procrustes(src, src @ (q @ mirror).T)
    assert abs(float(torch.det(R)) - 1.0) < 1e-12


def test_kat_euler_is_exact_in_one_step_for_straight_flow():
    x1 = torch.randn(10, 3, dtype=torch.float64)
    x0 = torch.randn(10, 3, dtype=torch.float64)
    x_t, x0_hat = O.euler_step(x1, 1.0, 1.0, lambda x, t: x1 - x0)
    assert float((x_t - x0).abs().max()) < 1e-14 and float((x0_hat - x0).abs().max()) < 1e-14


def test_kat_attention_single_token_segment_returns_v():
    qkv = torch.randn(5, 3, 8, 64, dtype=torch.float64)
    cu = torch.tensor([0, 1, 5], dtype=torch.int32)
    out = O.varlen_attention(qkv, cu)
    assert float((out[0] - qkv[0, 2]).abs().max()) < 1e-14


def test_kat_timestep_sinusoid_layout():
    ts = O.timestep_sinusoid(torch.tensor([0.5]))
    assert ts.shape == (1, 256)
    assert abs(ts[0, 0].item() - math.cos(0.5)) < 1e-6          # cos first (flip_sin_to_cos=True), w_0 = 1
    assert abs(ts[0, 128].item() - math.sin(0.5)) < 1e-6
    assert abs(ts[0, 127].item() - math.cos(0.5 * math.exp(-math.log(10000) * 127 / 128))) < 1e-6


# ---------------------------------------------------------------------------------------------
# generation selection by rigidity
# ---------------------------------------------------------------------------------------------
def _selection_golden():
    g, inp = load_golden("selection_g3")
    cu_b, _ = O.prepare_cu_seqlens(inp)
    return g, inp, cu_b.long(), torch.from_numpy(g["trajectories"])


def test_oracle_selection_matches_reference_golden():
    """oracle restatement of compute_rigidity_rmse / trajectory average / argmin-select vs the fixture produced by the
    reference's own fit_transformations + compute_rigidity_rmse (oracle/make_golden.py::make_selection_golden)."""
    g, inp, cu, trajs = _selection_golden()
    cond, ppp, scales = inp["pointclouds"], inp["points_per_part"], inp["scales"]
    G = trajs.shape[0]
    for tag in ("avg", "final"):
        rig, Rs, ts = [], [], []
        for k in range(G):
            R, t = O.fit_transformations(cond, trajs[k][-1], ppp, cu)
            Rs.append(R); ts.append(t)
            if tag == "avg":
                rig.append(O.average_trajectory_rigidity_rmse(cond, trajs[k], ppp, cu, scales)[0])
            else:
                rig.append(O.compute_rigidity_rmse(cond, trajs[k][-1], R, t, ppp, cu, scales))
        stacked = torch.stack(rig)
        ref = torch.from_numpy(g[f"{tag}_rigidity_rmse"])
        assert (stacked - ref).abs().max().item() <= 2e-6 * ref.abs().max().item()
        best, cloud, R, t = O.select_generations_by_rigidity(stacked, trajs[:, -1], torch.stack(Rs), torch.stack(ts), cu)
        assert torch.equal(best, torch.from_numpy(g[f"{tag}_best_gen_indices"]))
        assert (cloud - torch.from_numpy(g[f"{tag}_pointclouds_selected"])).abs().max().item() == 0.0
        assert (R - torch.from_numpy(g[f"{tag}_rotations_selected"])).abs().max().item() < 1e-5
    R0, t0 = O.fit_transformations(cond, trajs[0][-1], ppp, cu)
    pp = O.compute_rigidity_rmse(cond, trajs[0][-1], R0, t0, ppp, cu, None, average_per_part=True)
    assert (pp - torch.from_numpy(g["per_part_rmse"])).abs().max().item() < 2e-6


def test_oracle_rigidity_matches_live_reference_function():
    """the reference's fit_transformations + compute_rigidity_rmse (values in the live-checks fixture) vs the restatement, with the
    reference's poses as input to both"""
    from oracle.make_golden import rigidity_check_inputs
    z = _live_checks()
    inp, cu, pred = rigidity_check_inputs()     # empty parts only as trailing padding: the reference's split_parts drops empty splits and mis-indexes otherwise
    R, t = torch.from_numpy(z["rigidity_R"]), torch.from_numpy(z["rigidity_t"])
    for per_part in (False, True):
        for scaled in (False, True):
            a = torch.from_numpy(z[f"rigidity_rmse_{int(per_part)}{int(scaled)}"])
            b = O.compute_rigidity_rmse(inp["pointclouds"], pred, R, t, inp["points_per_part"], cu, inp["scales"] if scaled else None, per_part)
            assert a.shape == b.shape and (a - b).abs().max().item() < 1e-6


# ---------------------------------------------------------------------------------------------
# output transform files
# ---------------------------------------------------------------------------------------------
def _transform_golden():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transform_files.npz"))
    g = {k: z[k] for k in z.files}
    T = lambda k: torch.from_numpy(g[k])
    data = {"rotations": T("in_rotations"), "translations": T("in_translations"), "scales": T("in_scales"),
            "points_per_part": T("in_points_per_part")}
    return g, data, T


def test_oracle_relative_transforms_match_reference_written_files():
    """oracle restatement vs the matrices parsed back from the text files the reference's own
    Evaluator._save_transformation_files wrote (oracle/make_golden.py::make_transform_golden); %12.8f => 1e-8 quantum."""
    g, data, T = _transform_golden()
    ppp = data["points_per_part"]
    valid = [(b, p) for b in range(ppp.shape[0]) for p in range(ppp.shape[1]) if ppp[b, p] > 0]
    for tag, gr, gt in (("plain", None, None), ("global", T("global_rotation"), T("global_translation"))):
        M = O.relative_transforms(T("R_pred"), T("t_pred"), data["rotations"], data["translations"], data["scales"], ppp, gr, gt)
        got = torch.stack([M[b, p] for b, p in valid]).double()
        ref = torch.from_numpy(g[f"{tag}_matrices"])
        assert got.shape == ref.shape
        assert (got - ref).abs().max().item() < 1e-5 * max(1.0, ref.abs().max().item())


# ---------------------------------------------------------------------------------------------
# cross-part overlap ratio
# ---------------------------------------------------------------------------------------------
def _overlap_golden():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "overlap_ratio.npz"))
    return {k: z[k] for k in z.files}


def test_oracle_transform_errors_match_reference_golden():
    """compute_transform_errors, no-ICP branch (eval/metrics.py:165-303): the restatement vs the reference's own function (fixture from
    oracle/make_golden.py --transform-errors-only): plain, scaled, and with matched_part_ids; NaN where a sample has no movable part."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transform_errors.npz"))
    T = lambda k: torch.from_numpy(z[k])
    for tag, mid, sc in (("plain", None, None), ("scaled", None, T("scale")), ("matched", T("matched_part_ids"), T("scale"))):
        re, te, _, _ = O.compute_transform_errors(T("R_gt"), T("t_gt"), T("R_pred"), T("t_pred"), T("points_per_part"), T("anchor_part"), mid, sc)
        ref_r, ref_t = T(f"{tag}_rot"), T(f"{tag}_trans")
        assert torch.equal(torch.isnan(re), torch.isnan(ref_r)) and bool(torch.isnan(ref_r).any())
        ok = ~torch.isnan(ref_r)
        assert float((re[ok] - ref_r[ok]).abs().max()) < 2e-3 and float((te[ok] - ref_t[ok]).abs().max()) < 1e-5, tag
    # fp64 evaluation of the same formula: what the fp32 values are a rounding of (acos near 1 is ill-conditioned: 0.3 degrees in the fixture)
    re64, te64, _, _ = O.compute_transform_errors(T("R_gt").double(), T("t_gt").double(), T("R_pred").double(), T("t_pred").double(),
                                                  T("points_per_part"), T("anchor_part"))
    ok = ~torch.isnan(re64)
    assert float((re64[ok].float() - T("plain_rot")[ok]).abs().max()) < 2e-2


def test_oracle_overlap_ratio_matches_reference_golden():
    """The oracle uses exact fp64 distances; the reference's fp32 cdist can flip a point whose nearest other-part neighbour
    sits within ~1e-5 of a threshold, so the comparison allows 2 points per object (the fixture has 301-700 per object)."""
    g = _overlap_golden()
    pred, ppp, cu = torch.from_numpy(g["pred"]), torch.from_numpy(g["points_per_part"]), torch.from_numpy(g["cu_seqlens"])
    ratios, min_d = O.compute_overlap_ratio(pred, ppp, cu, g["taus"].tolist())
    n = (cu[1:] - cu[:-1]).double()
    assert ((ratios - torch.from_numpy(g["ratios"]).double()).abs() * n[None, :]).max().item() <= 2.0 + 1e-6
    assert ratios[:, 1].abs().max().item() == 0.0            # single-part object
    assert torch.isinf(min_d[int(cu[1]):int(cu[2])]).all()


# ---------------------------------------------------------------------------------------------
# MiniSpinNet local feature extractor
# ---------------------------------------------------------------------------------------------
def _spinnet_golden():
    from rap_amd.spinnet import make_spinnet_weights
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spinnet_k16.npz"))
    return z, make_spinnet_weights(int(z["weight_seed"]))


def test_spinnet_oracle_matches_reference_golden():
    from oracle import spinnet_oracle as SO
    z, sd = _spinnet_golden()
    out = SO.forward(sd, torch.from_numpy(z["pts"]), torch.from_numpy(z["kpts"]), float(z["des_r"]), torch.from_numpy(z["perm"]))
    assert (out["patches"][:, :4] - torch.from_numpy(z["patches_first"])).abs().max().item() == 0.0
    assert (out["patches"][:, -1] - torch.from_numpy(z["patches_last"])).abs().max().item() == 0.0
    assert (out["desc"] - torch.from_numpy(z["desc"])).abs().max().item() < 2e-6
    counts = z["ball_counts"]
    assert counts.min() == 0 and (counts < 512).any() and (counts > 512).any()      # the fixture exercises fill and cap


def test_spinnet_oracle_matches_live_reference():
    from oracle import spinnet_oracle as SO
    from oracle.make_golden import spinnet_check_inputs
    from rap_amd.spinnet import make_spinnet_weights
    z = _live_checks()
    sd = make_spinnet_weights(3)
    pts, kpts, des_r, _ = spinnet_check_inputs()
    out = SO.forward(sd, pts, kpts, des_r, torch.as_tensor(z["spinnet_perm"]))
    assert out["patches"].shape == z["spinnet_patches"].shape
    assert (out["patches"] - torch.from_numpy(z["spinnet_patches"])).abs().max().item() == 0.0
    assert (out["desc"] - torch.from_numpy(z["spinnet_desc"])).abs().max().item() < 2e-6


def test_spinnet_fp64_chunked_oracle_reproduces_both_reference_fixtures():
    """The scaled form of the oracle (fp64, chunked ball queries, convolutions as slices + matmul, local reference frame) against the two
    fixtures written by the reference's own module, within the bounds the GPU tests use for them (5e-5 global-z, 2e-4 LRF).  A chunk of 5
    keypoints leaves a partial last chunk."""
    from oracle import spinnet_oracle as SO
    from rap_amd.spinnet import make_spinnet_weights
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    for name, lrf, bound in (("spinnet_k16.npz", False, 5e-5), ("spinnet_k16_lrf.npz", True, 2e-4)):
        z = np.load(os.path.join(golden, name))
        sd = make_spinnet_weights(int(z["weight_seed"]))
        args = (sd, torch.from_numpy(z["pts"]), torch.from_numpy(z["kpts"]), float(z["des_r"]), torch.from_numpy(z["perm"]))
        out = SO.forward(*args, dtype=torch.float64, lrf=lrf, chunk=5)
        err = (out["desc"] - torch.from_numpy(z["desc"]).double()).abs().max().item()
        print(f"{name}: fp64 chunked oracle vs the reference's fp32 descriptors {err:.2e}")
        assert out["desc"].dtype == torch.float64 and err < bound, (name, err)
        assert (out["patches"][:, :4] - torch.from_numpy(z["patches_first"]).double()).abs().max().item() < (1e-4 if lrf else 1e-6)
        assert out["ambiguous"].dtype == torch.bool and out["ambiguous"].shape == (16,)
        if lrf:
            # the fp32 form of the same mode (torch's own layers) agrees too, and the empty ball keeps the identity frame
            out32 = SO.forward(*args, lrf=True)
            assert (out32["desc"] - torch.from_numpy(z["desc"])).abs().max().item() < bound
        else:
            assert torch.equal(out["ball_counts"], torch.from_numpy(np.minimum(z["ball_counts"], 512)).long())
            # slices + matmul are the same convolutions as torch's: fp64 with torch's own layers is not reachable through forward(), so
            # compare the two forms through the fp32 path, which uses them
            out32 = SO.forward(*args)
            assert (out32["desc"].double() - out["desc"]).abs().max().item() < 2e-6
            assert (out32["x0"].double() - out["x0"]).abs().max().item() < 1e-5


def test_spinnet_chunked_ball_query_equals_the_dense_one():
    from oracle import spinnet_oracle as SO
    g = torch.Generator().manual_seed(3)
    p2 = torch.randn(700, 3, generator=g)
    p1 = torch.cat([p2[:40], torch.randn(31, 3, generator=g), torch.full((1, 3), 50.0)])      # members, strangers, one empty ball
    for K, r in ((512, 1.2), (10, 0.5), (3, 0.05)):
        idx, nn = SO.ball_query_first_k(p1, p2, K, r)
        for chunk in (1, 7, 72, 1000):
            idx_c, nn_c = SO.ball_query_first_k_chunked(p1, p2, K, r, chunk=chunk)
            assert torch.equal(idx, idx_c) and torch.equal(nn, nn_c), (K, r, chunk)
        # and the batched form used by the voxel query: every batch entry equals its own unbatched call
        bi, bn = SO.ball_query_first_k(p1[:8, None, :].expand(8, 5, 3).contiguous(), p2[None].expand(8, -1, -1), K, r)
        for b in range(8):
            ui, un = SO.ball_query_first_k(p1[b:b + 1].expand(5, 3), p2, K, r)
            assert torch.equal(bi[b], ui) and torch.equal(bn[b], un)
    assert (idx[-1] == -1).all() and (nn[-1] == 0).all()


def test_spinnet_oracle_on_constructed_patch_edges_matches_hand_built_expectations():
    """The edge clouds of oracle/preproc_cases.py (known in-radius counts 0, 1, 9, 10, 11, 511, 512, 513, 2 200, duplicates; a keypoint
    that is patch point 0 of its own ball): the oracle's ball counts, its patches (first 512 hits in scan order, keypoint fill, centred on
    slot 511) and its stage-1 output x0 equal expectations built point by point / voxel by voxel in loops, and nothing is flagged --
    what the GPU test then compares the kernel with."""
    from oracle import preproc_cases as PC, spinnet_oracle as SO
    from rap_amd.spinnet import make_spinnet_weights
    sd = make_spinnet_weights(6)
    for n_total in (1, 3, 1023, 1024, 1025, 4099):
        c = PC.spinnet_edge_case(n_total)
        assert c["pts"].shape == (n_total, 3) and c["pts"].dtype == torch.float32
        out = SO.forward(sd, c["pts"], c["kpts"], c["des_r"], c["perm"], dtype=torch.float64)
        assert torch.equal(out["ball_counts"], c["counts"].clamp(max=512)), n_total
        assert not out["ambiguous"].any(), n_total
        want = (c["patches"] - c["patches"][:, -1:, :]) / c["des_r"]
        assert (out["patches"] - want).abs().max().item() < 1e-13, n_total
        for s, cnt in enumerate(c["counts"].tolist()):
            centre = c["patches"][s, -1]
            if cnt >= 512:                      # the 512th hit, 0.6 r from the keypoint -- not the keypoint
                assert abs((centre - c["kpts"][s].double()).norm().item() / c["des_r"] - 0.6) < 1e-5
            else:
                assert torch.equal(centre, c["kpts"][s].double())
            x0 = PC.stage1_by_loops(sd, c["patches"][s], c["des_r"])
            assert (out["x0"][s] - x0).abs().max().item() < 1e-12, (n_total, s)
        out32 = SO.forward(sd, c["pts"], c["kpts"], c["des_r"], c["perm"])
        assert (out32["patches"].double() - want).abs().max().item() < 1e-6
        assert (out32["desc"].double() - out["desc"]).abs().max().item() < 5e-6
    full = PC.spinnet_edge_case(4099)
    assert sorted(full["counts"].tolist()) == sorted(PC.EDGE_COUNTS_FULL)
    s513 = full["counts"].tolist().index(513)
    assert torch.equal(full["patches"][s513, 0], full["kpts"][s513].double())          # the keypoint is patch point 0 of its own ball
    dup = full["patches"][full["counts"].tolist().index(40), :40]
    assert torch.unique(dup, dim=0).shape[0] == 20                                     # exact duplicates in the cloud
    # the index-0 mask is visible on these inputs: without it stage 1 differs
    q = (full["patches"][s513] - full["patches"][s513, -1]) / full["des_r"]
    vox = SO.voxel_centres().double()
    assert (((vox - q[0]) ** 2).sum(-1) < (0.8 / 3) ** 2).any()


def test_spinnet_ambiguity_flag_fires_on_a_point_at_the_radius_and_only_there():
    from oracle import spinnet_oracle as SO
    from rap_amd.spinnet import make_spinnet_weights
    sd = make_spinnet_weights(0)
    kpts = torch.tensor([[0.0, 0.0, 0.0], [20.0, 0.0, 0.0], [40.0, 0.0, 0.0]])
    r = 0.5
    # keypoint 0: a point at distance r (1 + 1e-7); keypoint 1: two clearly inside points chosen off every voxel shell; keypoint 2: a
    # patch point whose distance to a voxel centre is within rounding of 0.8 / 3
    vox = SO.voxel_centres().double()
    q = vox[200] + torch.tensor([0.0, 0.0, 0.8 / 3 * (1 + 1e-8)], dtype=torch.float64)
    pts = torch.cat([torch.tensor([[r * (1 + 1e-7), 0.0, 0.0], [20.05, 0.01, 0.02], [20.0, -0.11, 0.03]], dtype=torch.float64),
                     kpts[2].double()[None] + q[None] * r])
    out = SO.forward(sd, pts.float(), kpts, r, torch.arange(4), dtype=torch.float64)
    assert out["ambiguous"].tolist() == [True, False, True]
    assert torch.isfinite(out["desc"]).all()


def test_fps_oracle_device_argument_keeps_the_index_list():
    from oracle import preproc_cases as PC
    p = PC.grid_cloud(6, 6, 6, seed=1)
    a = O.farthest_point_sampling(p, 216, 216, 215)
    b = O.farthest_point_sampling(p, 216, 216, 215, device="cpu")
    assert torch.equal(a, b) and a.dtype == torch.long and sorted(a.tolist()) == list(range(216))
    # first maximum on ties: from a corner of a 2 x 2 square the two adjacent corners tie after the far one -- the lower index is picked
    sq = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 1.0, 0.0]])
    assert O.farthest_point_sampling(sq, 4, 4, 0).tolist() == [0, 3, 1, 2]
    lat = PC.lattice_cloud(5000, 3)
    assert torch.unique(lat, dim=0).shape[0] == 5000 and lat.max() <= 1023 and lat.min() >= 0 and torch.equal(lat, lat.round())


# ---------------------------------------------------------------------------------------------
# nearest-neighbour metrics
# ---------------------------------------------------------------------------------------------
def test_oracle_correspondence_rmse_matches_reference_golden():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nn_metrics.npz"))
    T = lambda k: torch.from_numpy(z[k])
    for thr in (0.02, 0.05):
        rmse, n, ratio, _ = O.compute_correspondence_rmse(T("source_gt"), T("target_gt"), T("source_pred"), T("target_pred"), thr)
        ref = z[f"corr_{thr}"]
        assert abs(n - ref[1]) <= 1 and abs(float(rmse) - ref[0]) < 1e-4 * ref[0] + 1e-6       # fp32 cdist vs fp64 at the threshold
    rmse, n, ratio, _ = O.compute_correspondence_rmse(T("source_gt"), T("target_gt") + 10.0, T("source_pred"), T("target_pred"), 0.05)
    assert n == 0 and np.isinf(float(rmse)) and np.isinf(z["corr_none"][0])


# ---------------------------------------------------------------------------------------------
# voxel down-sampling (preprocessing)
# ---------------------------------------------------------------------------------------------
def _voxel_golden():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "voxel_downsample.npz"))
    g = torch.Generator().manual_seed(int(z["seed"]))
    p = (torch.rand(int(z["n"]), 3, generator=g) - 0.4) * torch.from_numpy(z["scale"])
    return z, p


def test_oracle_voxel_downsample_matches_reference_golden():
    z, p = _voxel_golden()
    for vs in (0.25, 1.0):
        assert np.array_equal(O.voxel_down_sample(p.numpy(), vs), z[f"idx_{vs}"])


def test_oracle_voxel_downsample_matches_live_reference():
    from oracle.make_golden import VOXEL_CHECK_CASES, voxel_check_points, voxel_index_digest
    z = _live_checks()
    for seed, (n, vs, scale) in enumerate(VOXEL_CHECK_CASES):
        idx = O.voxel_down_sample(voxel_check_points(seed, n, scale).numpy(), vs)
        assert len(idx) == int(z[f"voxel_idx_{seed}_len"]), (n, vs, len(idx))
        assert voxel_index_digest(idx) == str(z[f"voxel_idx_{seed}_sha256"]), (n, vs)


# ---------------------------------------------------------------------------------------------
# input side of the boundary: _transform (evaluation split) + variable_collate_fn
# ---------------------------------------------------------------------------------------------
COLLATE_KEYS = ("cu_seqlens", "pointclouds", "pointclouds_gt", "part_indices", "anchor_indices", "features", "rotations", "translations",
                "points_per_part", "anchor_parts", "init_rotation", "scales", "global_rotation", "global_translation")


def load_collate_golden():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "collate_transform.npz"))
    samples = []
    for b in range(int(z["num_samples"])):
        counts = z[f"raw_counts_{b}"]; off = np.concatenate([[0], np.cumsum(counts)])
        pts, fe = z[f"raw_points_{b}"], z[f"raw_features_{b}"]
        samples.append({"parts": [pts[off[i]:off[i + 1]] for i in range(len(counts))],
                        "features": [fe[off[i]:off[i + 1]] for i in range(len(counts))]})
    return z, samples


def test_oracle_transform_and_collate_matches_reference_golden():
    z, samples = load_collate_golden()
    got = O.transform_and_collate(samples, int(z["max_parts"]), int(z["numpy_seed"]))
    for k in COLLATE_KEYS:
        ref = z["ref_" + k]
        g = got[k].numpy()
        assert g.shape == ref.shape and g.dtype == ref.dtype, (k, g.shape, ref.shape, g.dtype, ref.dtype)
        if ref.dtype.kind == "f":
            assert np.abs(g - ref).max() <= 1e-6 * max(1.0, np.abs(ref).max()), (k, np.abs(g - ref).max())
        else:
            assert np.array_equal(g, ref), k
    # the invariant the reference asserts in its own __main__ (dataset.py:927-932): cond @ R^T + t recovers gt for non-anchor parts
    ppp = got["points_per_part"][0]; st = 0
    for i in range(int((ppp > 0).sum())):
        ed = st + int(ppp[i])
        if not bool(got["anchor_parts"][0, i]):
            rec = got["pointclouds"][st:ed] @ got["rotations"][0, i].T + got["translations"][0, i]
            assert (rec - got["pointclouds_gt"][st:ed]).abs().max() < 1e-6
        st = ed


def test_oracle_transform_and_collate_matches_live_reference():
    from oracle.make_golden import collate_samples
    z = _live_checks()
    samples = collate_samples(seed=9)
    got = O.transform_and_collate(samples, 6, 4)
    # the reference's collated features are a row permutation of the raw ones: the fixture stores that permutation
    raw = np.concatenate([np.concatenate(s["features"]) for s in samples])
    ref = {k: torch.from_numpy(z["collate_" + k]) for k in COLLATE_KEYS if k != "features"}
    ref["features"] = torch.from_numpy(raw[z["collate_features_row_of_raw"]])
    for k in COLLATE_KEYS:
        r, g = ref[k], got[k]
        assert r.shape == g.shape and r.dtype == g.dtype, k
        if r.dtype.is_floating_point:
            assert (r - g).abs().max().item() <= 1e-6 * max(1.0, r.abs().max().item()), k
        else:
            assert torch.equal(r, g), k


# ---------------------------------------------------------------------------------------------
# preprocessing in front of FPS / MiniSpinNet: voxel-adaptive sample counts (pinned), statistical outlier removal (unpinned)
# ---------------------------------------------------------------------------------------------
def adaptive_parts():
    g = np.random.RandomState(5)
    return [g.rand(4000, 3) * np.array([20, 15, 3.0]), g.rand(37, 3), np.zeros((0, 3)), g.rand(900, 3) * np.array([4, 4, 1.0]) - 2.0]


ADAPTIVE_EXPECTED = ([1500, 37, 0, 309], [3856, 30, 0, 618])     # counts / occupied voxels printed by the reference's own functions


def test_oracle_adaptive_sample_count_matches_reference_values():
    parts = adaptive_parts()
    assert O.calculate_adaptive_sample_count_per_part(parts, 0.25, 0.5, 50, 1500) == ADAPTIVE_EXPECTED[0]
    assert [O.calculate_voxel_coverage(p, 0.25) for p in parts] == ADAPTIVE_EXPECTED[1]


def test_oracle_adaptive_sample_count_matches_live_reference():
    from oracle.make_golden import ADAPTIVE_CHECK_ARGS
    z = _live_checks()
    parts = adaptive_parts()
    for i, (vs, ratio, mn, mx) in enumerate(ADAPTIVE_CHECK_ARGS):
        assert O.calculate_adaptive_sample_count_per_part(parts, vs, ratio, mn, mx) == z[f"adaptive_counts_{i}"].tolist()


def test_oracle_statistical_outlier_rule_on_a_known_case():
    """Analytic check of the restated Open3D rule: a regular 10 x 10 x 1 grid (spacing 1) plus one far point -- only the far point
    has a mean neighbour distance beyond mean + 2.5 std, and duplicated points (d = 0 with k = 2) are dropped by the d > 0 test."""
    xs, ys = np.meshgrid(np.arange(10.0), np.arange(10.0))
    grid = np.stack([xs.ravel(), ys.ravel(), np.zeros(100)], axis=1)
    pts = np.concatenate([grid, [[50.0, 50.0, 0.0]]])
    idx, avg = O.remove_statistical_outlier(pts, nb_neighbors=5, std_ratio=2.5)
    assert list(idx) == list(range(100)) and avg[100] > 40
    dup = np.concatenate([grid, grid[:1]])                       # point 0 twice: with k = 2 both copies see only each other -> d = 0
    idx2, avg2 = O.remove_statistical_outlier(dup, nb_neighbors=2, std_ratio=10.0)
    assert avg2[0] == 0 and avg2[100] == 0 and 0 not in idx2 and 100 not in idx2


def test_device_checker_attention_math_equals_sdpa_on_cpu():
    """The explicit matmul + softmax attention the DEVICE-side checker uses (`_softmax_attention_chunked`, query rows in chunks) is the
    function F.scaled_dot_product_attention evaluates on the CPU path -- checked here on CPU, with a chunk size that forces several
    ragged chunks, in fp32 and fp64."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(5)
    for dtype, tol in ((torch.float32, 2e-6), (torch.float64, 1e-14)):
        q, k, v = (torch.randn(8, 301, 64, generator=g, dtype=dtype) for _ in range(3))
        ref = F.scaled_dot_product_attention(q, k, v)
        got = O._softmax_attention_chunked(q, k, v, max_score_elems=8 * 301 * 37)
        assert float((got - ref).abs().max()) <= tol
        one = O._softmax_attention_chunked(q[:, :1], k[:, :1], v[:, :1])       # single-token segment: out = v
        assert torch.equal(one, v[:, :1])


def test_sample_device_argument_is_a_noop_on_cpu():
    """`O.sample(..., device="cpu")` is the same evaluation as the default (the device argument only moves tensors)."""
    g, inp = load_golden("l2_ragged_rigid")
    cfg = dict(S.RAP_12); cfg["num_layers"] = int(g["num_layers"])
    sd = S.make_weights(cfg, int(g["weight_seed"]))
    a = O.sample(sd, cfg, inp, int(g["num_steps"]), bool(g["rigidity"]))
    b = O.sample(sd, cfg, inp, int(g["num_steps"]), bool(g["rigidity"]), device="cpu")
    for k in ("end_point_trajectory", "trajectory", "R", "t"):
        assert torch.equal(a[k], b[k])
