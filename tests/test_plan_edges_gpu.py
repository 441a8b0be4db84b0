"""GPU: one whole model call on each side of every boundary of the call plan (tests/plan_cases.py), against a float64 evaluation of the
oracle on the device, inside a workspace of exactly rap_workspace_bytes between guard bands and filled with 0xFF (any stale or unwritten
value a kernel reads is a NaN).  One model per mode and one float64 oracle run per geometry for the whole module.

  * every (pair member, mode): rap_sample through sample_and_register -- guards intact, outputs finite, the library's plan for the call is
    the listed one, all four attention launches bounded; fp32 and split precision at test_fullconfig_gpu._assert_fp32 (per-sample bound
    included), the 16-bit modes at the bounds of test_h16_gpu.py / test_small_call_gpu.py;
  * the row pairs 2048 | 2049 and 4096 | 4097 through model(...) too (rap_dit_forward: per-sample timesteps, the caller's part table, a
    feature output -- in the fp16 stream the head GEMMs at ragged M = TP on planes sized for TQ) at the bounds of test_widths_gpu.py;
  * at 2 049 and 3 841 tokens (two planes, fusion on) the ring / fused / small-item launch sequence against the round-5 one, bit for bit.

Every call is a valid call at a valid size; errors, yardsticks (the plain fp32 device oracle's distance from float64 on the same inputs)
and the file's wall time go to plan_edges.jsonl in the suite's record directory (test_fullconfig_gpu._record).
"""
import time

import pytest
import torch

import guards
import plan_cases as PC
import rap_amd
from oracle import rap_oracle as O
from rap_amd import _lib
from rap_amd import synthetic as S
from test_fullconfig_gpu import _assert_fp32, _errors, _record as _record_to
from test_h16_gpu import FWD_REL_BOUND

pytestmark = pytest.mark.gpu

KEYS = ("end_point_trajectory", "trajectory", "R", "t")
_MODELS, _REF64, _YARD, _FWD64, _SD64 = {}, {}, {}, {}, {}


def _record(row):
    """one line per case in plan_edges.jsonl, next to the suite's other parity records"""
    _record_to(row, "plan_edges.jsonl")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    t0 = time.perf_counter()
    yield torch.device("cuda:0")
    torch.cuda.synchronize()
    _record({"case": "file", "wall_s": round(time.perf_counter() - t0, 2)})


def _cfg():
    cfg = dict(S.RAP_12); cfg["num_layers"] = PC.LAYERS
    return cfg


def _weights():
    if "sd" not in _SD64:
        _SD64["sd"] = S.make_weights(_cfg(), 0)
    return _SD64["sd"]


def _model(dev, mode):
    if mode not in _MODELS:
        cdt, rdt = PC.MODES[mode]
        m = rap_amd.PointCloudDiT(in_dim=0, out_dim=3, embed_dim=PC.D, num_layers=PC.LAYERS, num_heads=PC.HEADS, local_feat_dim=32, compute_dtype=cdt,
                                  residual_dtype=rdt)
        m.load_state_dict(_weights()); m.to(dev)
        m._activate(dev)
        _MODELS[mode] = m
    return _MODELS[mode]


def _ref64(dev, m):
    """the float64 device oracle of a geometry, once"""
    if m.name not in _REF64:
        r = O.sample(_weights(), _cfg(), PC.inputs(m), PC.STEPS, True, dtype=torch.float64, device=dev)
        _REF64[m.name] = {k: r[k] for k in KEYS}
    return _REF64[m.name]


def _yardstick(dev, m):
    """how far the plain fp32 device oracle sits from float64 on the same inputs"""
    if m.name not in _YARD:
        r = O.sample(_weights(), _cfg(), PC.inputs(m), PC.STEPS, True, device=dev)
        inp = PC.inputs(m)
        _YARD[m.name] = _errors({k: r[k] for k in KEYS}, _ref64(dev, m), inp["cu_seqlens"], inp["points_per_part"])
    return _YARD[m.name]


def _sample(dev, mode, m):
    flow = rap_amd.RectifiedPointFlow(flow_model=_model(dev, mode), inference_sampling_steps=PC.STEPS, rigidity_forcing=True, num_streams=1,
                                      graph_replay=False)
    inp = PC.inputs(m)
    out = flow.sample_and_register({k: v.to(dev) for k, v in inp.items()}, x_1=inp["x_1"].to(dev))
    torch.cuda.synchronize()
    return {k: out[k] for k in KEYS}


def _check_plan(lib, model, mode, TP, B, nseg, rows, ex):
    """the library's plan for this call (live tuning keys) is the listed one, its size is rap_workspace_bytes, and that is what the call got"""
    p = PC.lib_plan(lib, mode, TP, B, nseg, rows=rows)
    assert p == PC.plan(mode, TP, B, nseg, rows=rows), p
    assert p.ws_bytes == lib.rap_workspace_bytes(model._handle, TP, B, nseg, rows)
    assert p.ws_bytes in [g.nbytes for g in ex.handed], (p.ws_bytes, [g.nbytes for g in ex.handed])
    assert lib.rap_model_bounded_attention_launches(model._handle) == 2 * PC.LAYERS
    return p


CASES = PC.cases()


@pytest.mark.parametrize("pair,side,m,mode", CASES, ids=[PC.case_id(p, s, mode) for p, s, _, mode in CASES])
def test_sampling_call_on_each_side_of_every_plan_boundary(dev, monkeypatch, pair, side, m, mode):
    lib = _lib.load()
    ref = _ref64(dev, m)
    model = _model(dev, mode)
    t0 = time.perf_counter()
    ex = guards.exact_workspaces(monkeypatch)
    out = _sample(dev, mode, m)
    ex.check_all()
    wall = time.perf_counter() - t0
    for k in KEYS:
        assert torch.isfinite(out[k]).all(), k
    p = _check_plan(lib, model, mode, m.TP, m.B, m.nseg, PC.STEPS, ex)
    if pair.name == "rows-768" and mode == "x2":
        # tuning key 17 at its default: 768 rows take the fp32 layout, 1 024 the split layout, both inside the size that covers either
        assert p.dtype == (0 if side == "low" else 3)
        assert p.ws_bytes == max(PC.plan("x2", m.TP, m.B, m.nseg, force_dtype=fd).ws_bytes for fd in (0, 3))
    inp = PC.inputs(m)
    e = _errors(out, ref, inp["cu_seqlens"], inp["points_per_part"])
    row = {"case": PC.case_id(pair, side, mode), "TP": m.TP, "B": m.B, "nseg": m.nseg, "wall_s": round(wall, 3),
           **{k: e[k] for k in ("final_cloud", "worst_step_cloud", "worst_step_x_t", "R_frob", "t", "per_sample_final_cloud_max", "worst_sample")}}
    cdt = PC.MODES[mode][0]
    if cdt in ("float32", "float32x2"):
        y = _yardstick(dev, m)
        row["yardstick"] = {k: y[k] for k in ("worst_step_cloud", "worst_step_x_t", "R_frob", "t", "per_sample_final_cloud_max")}
        _record(row)
        _assert_fp32(e)
    else:
        _record(row)
        assert e["final_cloud"] < PC.H16_SAMPLE_BOUND[cdt] and e["R_frob"] < PC.H16_SAMPLE_BOUND[cdt], e
        assert e["worst_step_cloud"] < PC.H16_STEP_BOUND, e


FWD_CASES = [c for c in CASES if c[0].name in PC.FWD_PAIRS]


def _fwd64(dev, m):
    """the oracle's forward in float64 on the device: per-sample timesteps, velocity and transformer features"""
    if m.name not in _FWD64:
        inp = PC.inputs(m)
        if "dev" not in _SD64:
            _SD64["dev"] = {k: v.to(device=dev, dtype=torch.float64) for k, v in _weights().items()}
        cu_b, cu_p = O.prepare_cu_seqlens(inp)
        ts = torch.linspace(0.15, 0.9, m.B)
        f64 = lambda t: t.to(device=dev, dtype=torch.float64)
        with torch.inference_mode():
            r = O.dit_forward(_SD64["dev"], _cfg(), f64(inp["x_1"]), f64(ts), f64(inp["pointclouds"]), f64(inp["features"]), f64(inp["scales"]),
                              inp["anchor_indices"].to(dev), cu_b, cu_p, return_transformer_features=True)
        _FWD64[m.name] = (ts, r["velocity"], r["transformer_features"])
    return _FWD64[m.name]


@pytest.mark.parametrize("pair,side,m,mode", FWD_CASES, ids=[PC.case_id(p, s, mode) for p, s, _, mode in FWD_CASES])
def test_forward_call_on_each_side_of_the_few_token_boundaries(dev, monkeypatch, pair, side, m, mode):
    lib = _lib.load()
    ts, v_ref, f_ref = _fwd64(dev, m)
    model = _model(dev, mode)
    inp = PC.inputs(m)
    cu_b, cu_p = O.prepare_cu_seqlens(inp)
    d = {k: v.to(dev) for k, v in inp.items()}
    ex = guards.exact_workspaces(monkeypatch)
    out = model(x=d["x_1"], timesteps=ts.to(dev), cond_coord=d["pointclouds"], local_features=d["features"], latent_features=None, scales=d["scales"],
                anchor_indices=d["anchor_indices"], cu_seqlens_batch=cu_b.to(dev), cu_seqlens_part=cu_p.to(dev), return_transformer_features=True)
    torch.cuda.synchronize()
    ex.check_all()
    v, f = out["velocity"], out["transformer_features"]
    assert torch.isfinite(v).all() and torch.isfinite(f).all()
    VP = cu_p.shape[0] - 1
    assert VP < m.nseg                                       # (the caller's part table holds the non-empty parts only)
    _check_plan(lib, model, mode, m.TP, m.B, VP, m.B, ex)
    vmax, fmax = float(v_ref.abs().max()), float(f_ref.abs().max())
    ev, ef = float((v - v_ref).abs().max()), float((f - f_ref).abs().max())
    _record({"case": "forward-" + PC.case_id(pair, side, mode), "velocity": ev, "features": ef, "max_v": vmax, "max_f": fmax})
    cdt, rdt = PC.MODES[mode]
    if cdt in ("float32", "float32x2"):
        assert ev <= PC.FWD_FP32_V_REL * vmax and ev < PC.FWD_FP32_V_ABS and ef < PC.FWD_FP32_F_ABS, (ev, ef)
    else:
        assert FWD_REL_BOUND == PC.FWD_REL_BOUND
        bound = FWD_REL_BOUND[cdt] * (2.0 if (cdt, rdt) == ("float16", "float16") else 1.0)
        assert ev / vmax < bound and ef / fmax < 4 * bound, (ev / vmax, ef / fmax)


BITID = [(m, mode) for m in PC.members() if m.name in PC.BITID_MEMBERS for mode in PC.BITID_MODES]


@pytest.mark.parametrize("m,mode", BITID, ids=[f"{m.name}-{mode}" for m, mode in BITID])
def test_ring_and_fused_sequence_is_bit_identical_to_the_round5_sequence_on_two_planes(dev, m, mode):
    """tests/test_small_call_gpu.py's check at the sizes where the split-K buffer holds TWO planes and the fusion is still on (tuning keys
    18 / 19 / 20 = 256 / 1 / 2 against 0 / 0 / 0): bit-identical in the 16-bit mode; split precision also splits the out-projection's K in the
    fused sequence, so fp32-class agreement there"""
    lib = _lib.load()
    p = PC.lib_plan(lib, mode, m.TP, m.B, m.nseg)
    assert p.planes == 2 and p.fused == 1
    outs = {}
    for tag, pairs in (("r6", [(18, 256), (19, 1), (20, 2)]), ("r5", [(18, 0), (19, 0), (20, 0)])):
        with PC.tuned(lib, pairs):
            outs[tag] = _sample(dev, mode, m)
    for k in KEYS:
        assert torch.isfinite(outs["r5"][k]).all()
        if mode == "x2":
            assert float((outs["r6"][k] - outs["r5"][k]).abs().max()) < PC.BITID_X2_TOL, k
        else:
            assert torch.equal(outs["r6"][k], outs["r5"][k]), (k, float((outs["r6"][k] - outs["r5"][k]).abs().max()))
