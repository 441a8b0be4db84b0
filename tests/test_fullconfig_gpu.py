"""Parity at FULL configuration depth: the numbers the driver actually times, checked sample by sample.

The CPU reference cannot produce these cases in test time (one 2 x 4096 pair costs 854 s of CPU, two steps of configs[4] 4 185 s), so
the checker here is the SAME restatement the CPU tests pin to the unmodified reference (`oracle/rap_oracle.py`), evaluated on the
MI355X through PyTorch-ROCm in fp32 (`O.sample(..., device="cuda")`: plain torch ops, attention by torch's fp32 memory-efficient
SDPA kernel -- or explicit matmul + softmax in query chunks where a build lacks it -- the 3 x 3 SVDs on the host LAPACK).  The chain is closed by `test_device_oracle_equals_cpu_oracle`:

    unmodified reference (CPU)  ==  oracle on CPU  (tests/test_oracle.py, <= 5e-6, run in the build container + golden fixtures)
    oracle on CPU               ==  oracle on the GPU   (here, <= 5e-6, same seeded inputs as the golden l2_ragged_rigid)
    oracle on the GPU           ==  librapflow          (here, stated fp32 tolerances of SURVEY.md section 8d)

The device oracle is test infrastructure: it is imported only here and in bench.py's parity legs, never by rap_amd/.

  (a) configs[1]: ALL 32 pairs x 2 x 4096, rap_12, 20 steps, rigidity on = the batch bench.py times
  (b) configs[4]: 2 x 32 768, rap_12, ALL 50 steps (attention at L = 65 536 in every layer and step), B = 1   [slow]
  (c) configs[3]: B = 16 samples x 8 x 2048, rap_12, all 30 steps, rigidity on
  (d) one 400 000-token sample (16 parts of 25 000 points, the reference's max_points_per_batch, RAP_inference.yaml:35-36;
      layer.py:106-128 takes max_seqlen up to that), 2 layers, one flow step
"""
import json
import os
import time

import pytest
import torch

import rap_amd
from conftest import ROOT, load_golden
from oracle import rap_oracle as O
from rap_amd import synthetic as S

pytestmark = pytest.mark.gpu

# stated fp32 tolerances
TOL_CLOUD, TOL_R, TOL_T = 5e-4, 1e-3, 1e-3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _record(row, name="fullconfig_parity.jsonl"):
    out = os.path.join(ROOT, "gpurun_out")
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, name), "a") as f:
            f.write(json.dumps(row) + "\n")
    except OSError:
        pass
    print(row)


def _weights(layers):
    cfg = dict(S.RAP_12); cfg["num_layers"] = layers
    return cfg, S.make_weights(cfg, 0)


def _hip(cfg, sd, inp, steps, rigid, dev, dtype="float32", residual_dtype=None):
    m = rap_amd.PointCloudDiT(in_dim=0, out_dim=3, embed_dim=512, num_layers=cfg["num_layers"], num_heads=8, local_feat_dim=32,
                              attn_dtype=dtype, compute_dtype=dtype, residual_dtype=residual_dtype)
    m.load_state_dict(sd)
    m.to(dev)
    flow = rap_amd.RectifiedPointFlow(flow_model=m, inference_sampling_steps=steps, rigidity_forcing=rigid)
    d = {k: v.to(dev) for k, v in inp.items()}
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = flow.sample_and_register(d, x_1=d["x_1"])
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def _checker(cfg, sd, inp, steps, rigid, dev):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    ref = O.sample(sd, cfg, inp, steps, rigid, device=dev)
    torch.cuda.synchronize()
    return ref, time.perf_counter() - t0


def _errors(out, ref, cu, ppp):
    """max-abs deviations over the whole batch, per flow step, and per SAMPLE (so that a single bad pair cannot hide)."""
    ep = (out["end_point_trajectory"] - ref["end_point_trajectory"]).abs()
    xt = (out["trajectory"] - ref["trajectory"]).abs()
    per_step = ep.amax(dim=(1, 2))
    B = ppp.shape[0]
    final = ep[-1].amax(dim=1)
    per_sample = torch.stack([final[int(cu[b]):int(cu[b + 1])].max() if cu[b + 1] > cu[b] else final.new_zeros(()) for b in range(B)])
    Rf = torch.linalg.matrix_norm(out["R"] - ref["R"])
    tf = (out["t"] - ref["t"]).abs().amax(dim=-1)
    return {"final_cloud": float(ep[-1].max()), "final_x_t": float(xt[-1].max()), "worst_step_cloud": float(per_step.max()),
            "worst_step_x_t": float(xt.amax(dim=(1, 2)).max()), "first_step_cloud": float(per_step[0]), "last_step_cloud": float(per_step[-1]),
            "R_frob": float(Rf.max()), "t": float(tf.max()), "worst_sample": int(per_sample.argmax()),
            "per_sample_final_cloud_max": float(per_sample.max()), "per_sample_final_cloud_median": float(per_sample.median()),
            "last_sample_final_cloud": float(per_sample[-1]), "last_sample_R_frob": float(Rf[-1].max()), "samples": B}


def _assert_fp32(e):
    assert e["worst_step_cloud"] <= TOL_CLOUD and e["worst_step_x_t"] <= TOL_CLOUD, e
    assert e["final_cloud"] <= TOL_CLOUD and e["R_frob"] <= TOL_R and e["t"] <= TOL_T, e
    # what an exact-fp32 path achieves (an order of magnitude inside the stated bounds) -- on EVERY sample of the batch
    assert e["per_sample_final_cloud_max"] < 5e-5 and e["R_frob"] < 1e-4, e


def test_device_oracle_equals_cpu_oracle(dev):
    """Closes the chain reference -> CPU oracle -> device oracle on the seeded inputs of the golden case l2_ragged_rigid (ragged
    parts, rigidity forcing, every flow step) and on a full-size pair forward."""
    g, inp = load_golden("l2_ragged_rigid")
    cfg, sd = _weights(int(g["num_layers"]))
    steps, rigid = int(g["num_steps"]), bool(g["rigidity"])
    cpu = O.sample(sd, cfg, inp, steps, rigid)
    gpu = O.sample(sd, cfg, inp, steps, rigid, device=dev)
    worst = 0.0
    for k in ("end_point_trajectory", "trajectory", "R", "t", "transformer_features"):
        scale = 1.0 if k != "transformer_features" else max(1.0, float(cpu[k].abs().max()))
        err = float((gpu[k].cpu() - cpu[k]).abs().max()) / scale
        worst = max(worst, err)
        assert err <= 5e-6, (k, err)
        # ... and against the fixture the UNMODIFIED reference produced for these inputs
        gk = "sample_features" if k == "transformer_features" else k
        assert float((gpu[k].cpu() - torch.from_numpy(g[gk])).abs().max()) / scale <= 5e-6, k
    _record({"case": "device_oracle_vs_cpu_oracle:l2_ragged_rigid", "max_abs": worst})


def test_c1_all_32_pairs_match_the_checker(dev):
    """(a) the batch bench.py times: every one of the 32 pairs, every flow step."""
    cfg, sd = _weights(12)
    inp = S.make_inputs([[4096, 4096] for _ in range(32)], seed=1234)
    out, t_hip = _hip(cfg, sd, inp, 20, True, dev)
    ref, t_ref = _checker(cfg, sd, inp, 20, True, dev)
    e = _errors(out, ref, inp["cu_seqlens"], inp["points_per_part"])
    _record({"case": "c1_all_32_pairs", "dtype": "f32", **e, "hip_s": t_hip, "checker_s": t_ref})
    _assert_fp32(e)
    del out
    outh, t_h = _hip(cfg, sd, inp, 20, True, dev, dtype="bfloat16")
    eh = _errors(outh, ref, inp["cu_seqlens"], inp["points_per_part"])
    _record({"case": "c1_all_32_pairs", "dtype": "bf16", **eh, "hip_s": t_h})
    # ~3 x the WORST pair of the 32 measured on MI355X (r04: cloud 4.9e-3, |dR|_F 9.7e-3, t 2.3e-3 -- pair 11, five times pair 0's): a 10 x
    # regression of the bf16 path fails (the class bounds 5e-2 / 1e-1 of rounds 1-4 would have passed it)
    assert eh["final_cloud"] <= 1.5e-2 and eh["R_frob"] <= 3e-2 and eh["t"] <= 7e-3, eh
    del outh
    # split precision (round 5): fp32-ACCURATE arithmetic on the fp16 matrix pipe -- held to the fp32 asserts, on every pair
    outx, t_x = _hip(cfg, sd, inp, 20, True, dev, dtype="float32x2")
    ex = _errors(outx, ref, inp["cu_seqlens"], inp["points_per_part"])
    _record({"case": "c1_all_32_pairs", "dtype": "f32x2", **ex, "hip_s": t_x})
    _assert_fp32(ex)


def test_c3_16_samples_all_30_steps_match_the_checker(dev):
    """(c) configs[3] at the batch size the bench uses for it (16 samples = 262 144 tokens), all 30 steps, rigidity on."""
    cfg, sd = _weights(12)
    inp = S.make_inputs([[2048] * 8 for _ in range(16)], seed=1234)
    out, t_hip = _hip(cfg, sd, inp, 30, True, dev)
    ref, t_ref = _checker(cfg, sd, inp, 30, True, dev)
    e = _errors(out, ref, inp["cu_seqlens"], inp["points_per_part"])
    _record({"case": "c3_16_samples_30_steps", "dtype": "f32", **e, "hip_s": t_hip, "checker_s": t_ref})
    _assert_fp32(e)


@pytest.mark.slow
def test_c4_all_50_steps_match_the_checker(dev):
    """(b) configs[4]: 2 x 32 768 points, rap_12, ALL 50 flow steps; fp32 at the stated tolerances, bf16 deviation recorded."""
    cfg, sd = _weights(12)
    inp = S.make_inputs([[32768, 32768]], seed=1234)
    out, t_hip = _hip(cfg, sd, inp, 50, True, dev)
    ref, t_ref = _checker(cfg, sd, inp, 50, True, dev)
    e = _errors(out, ref, inp["cu_seqlens"], inp["points_per_part"])
    _record({"case": "c4_all_50_steps", "dtype": "f32", **e, "hip_s": t_hip, "checker_s": t_ref})
    _assert_fp32(e)
    del out
    # bf16: ~3 x the measured deviation (r04: 5.4e-4 / 1.5e-3 / 3.1e-4); split precision: the fp32 asserts
    for dtype, cloud_tol, R_tol, t_tol in (("bfloat16", 1.7e-3, 4.5e-3, 1e-3), ("float32x2", None, None, None)):
        outh, t_h = _hip(cfg, sd, inp, 50, True, dev, dtype=dtype)
        eh = _errors(outh, ref, inp["cu_seqlens"], inp["points_per_part"])
        _record({"case": "c4_all_50_steps", "dtype": dtype, **eh, "hip_s": t_h})
        if dtype == "float32x2":
            _assert_fp32(eh)
        else:
            assert eh["final_cloud"] <= cloud_tol and eh["R_frob"] <= R_tol and eh["t"] <= t_tol, eh
        det = torch.linalg.det(outh["R"].double())
        assert (det - 1).abs().max().item() < 1e-4


def test_400k_token_sample_matches_the_checker(dev):
    """(d) one sample at the reference's max_points_per_batch: 16 parts of 25 000 points = 400 000 tokens in ONE attention segment
    (32-bit offsets, work lists and the V^T image at their largest), 2 layers, one flow step with rigidity projection and pose fit;
    velocity recovered from the end point (t = 1: x0_hat = x_1 - v) on every 16th point, everything else on all points."""
    cfg, sd = _weights(2)
    inp = S.make_inputs([[25000] * 16], seed=77)
    # bf16: ~3 x the measured deviation (r04: velocity 5.4e-4, cloud 6.2e-4, last x_t 2.9e-3); split precision: the fp32 bounds
    for dtype, vtol, ctol in (("float32", 1e-4, TOL_CLOUD), ("float32x2", 1e-4, TOL_CLOUD), ("bfloat16", 1.7e-3, 9e-3)):
        out, t_hip = _hip(cfg, sd, inp, 1, True, dev, dtype=dtype)
        if dtype == "float32":
            ref, t_ref = _checker(cfg, sd, inp, 1, True, dev)
            v_ref = (inp["x_1"].to(dev) - ref["end_point_trajectory"][0])[::16]
        v = (inp["x_1"].to(dev) - out["end_point_trajectory"][0])[::16]
        vmax = float(v_ref.abs().max())
        e = _errors(out, ref, inp["cu_seqlens"], inp["points_per_part"])
        ev = float((v - v_ref).abs().max())
        _record({"case": "400k_tokens_1_sample", "dtype": dtype, "velocity_max_abs_err": ev, "max_abs_v": vmax, **e, "hip_s": t_hip,
                 "checker_s": t_ref})
        assert ev <= vtol * max(1.0, vmax), (dtype, ev, vmax)
        assert e["final_cloud"] <= ctol and e["final_x_t"] <= ctol, (dtype, e)
        if dtype in ("float32", "float32x2"):
            assert e["R_frob"] <= TOL_R and e["t"] <= TOL_T, e


def test_ragged_regime_batch_on_the_padded_fast_path(dev):
    """Round 4: every token-row buffer of the workspace is carved at align_up(TP, 256) rows and the layer kernels run over the padded
    row count, so a RAGGED batch (the reference's real regime, RAP_inference.yaml:30-36) takes the same persistent GEMMs as the
    uniform one.  A ragged reference-regime batch (~70 k points in samples of 2 / 8 / 64 parts, not a multiple of 256):
    (1) fp32 equals the device-side checker at the stated tolerances; (2) the filler rows never leak: with the WHOLE workspace
    pre-filled with NaN bit patterns the results are bit-identical, in fp32 and in both 16-bit modes (the 16-bit attention multiplies
    masked keys by p = 0, so a non-finite filler V column would poison real rows); (3) the attention work lists are emitted
    longest-segment-first (tests/test_kernels_gpu.py checks the order itself): switching that off changes no bit of the results."""
    from rap_amd import flow_model as FM
    cfg, sd = _weights(2)
    parts = S.ragged_regime_parts(70000, seed=11)
    inp = S.make_inputs(parts, seed=501)
    TP = int(inp["pointclouds"].shape[0])
    assert TP % 256 != 0
    ref = None
    for dtype in ("float32", "bfloat16", "float16", "float32x2"):
        out, _ = _hip(cfg, sd, inp, 2, True, dev, dtype=dtype)
        with torch.inference_mode():                          # (the workspace tensors were allocated under inference_mode)
            for buf in FM._WORKSPACES.values():
                buf.fill_(0xFF)                               # NaN in fp32, bf16 and fp16
        torch.cuda.synchronize()
        again, _ = _hip(cfg, sd, inp, 2, True, dev, dtype=dtype)
        for k in ("end_point_trajectory", "trajectory", "R", "t"):
            assert torch.isfinite(again[k]).all(), (dtype, k)
            assert torch.equal(out[k], again[k]), (dtype, k)
        # (3) the ORDER of the attention work lists (tuning key 15) is not observable in the results
        from rap_amd import _lib
        lib = _lib.load()
        try:
            assert lib.rap_set_tuning(15, 0) == 0
            unsorted, _ = _hip(cfg, sd, inp, 2, True, dev, dtype=dtype)
        finally:
            assert lib.rap_set_tuning(15, 1) == 0
        for k in ("end_point_trajectory", "trajectory", "R", "t"):
            assert torch.equal(out[k], unsorted[k]), (dtype, k)
        if dtype == "float32":
            ref, _ = _checker(cfg, sd, inp, 2, True, dev)
            e = _errors(out, ref, inp["cu_seqlens"], inp["points_per_part"])
            _record({"case": "ragged_regime_70k", "dtype": "f32", **e})
            _assert_fp32(e)
        elif dtype == "float32x2":
            e = _errors(out, ref, inp["cu_seqlens"], inp["points_per_part"])
            _record({"case": "ragged_regime_70k", "dtype": dtype, **e})
            _assert_fp32(e)
        else:
            e = _errors(out, ref, inp["cu_seqlens"], inp["points_per_part"])
            _record({"case": "ragged_regime_70k", "dtype": dtype, **e})
            # ~3 x the measured deviation (r04: bf16 8.5e-4 / 1.5e-3, fp16 1.4e-4 / 2.6e-4)
            ctol, rtol = (2.6e-3, 4.5e-3) if dtype == "bfloat16" else (4.2e-4, 7.8e-4)
            assert e["final_cloud"] <= ctol and e["R_frob"] <= rtol, (dtype, e)
