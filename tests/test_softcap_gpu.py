"""GPU: softcap and final_mlp_act, from the kernels to the constructor.

  a. the soft-capped attention kernels (rap_attention_f32_softcap, rap_x2_attention_softcap, rap_attention_h16_softcap for bf16 and
     fp16) over the segment-edge sweep of tests/attention_cases.py against the float64 oracle of tests/softcap_cases.py, a saturated
     case (raw logits +-1e3 under a cap of 5), single-token segments, rows outside the table, the argument checks;
  b. the bias + GELU epilogue of the fp32 GEMM at the head's shapes and on both 256 x 256 kernels (persistent, one tile per block);
  c. the model: every fixture of the unmodified reference (scripts/make_softcap_golden.py) in float32, float32x2 and bfloat16, the
     getters, the workspace query against the capped plan, graph replay.

Bounds.  fp32 and split precision: max(the family's bound of the uncapped kernel, FP32_SHARP_FACTOR x the error of a plain torch-CPU fp32
evaluation of the same capped attention against float64) -- the project's rule for fp32 attention cases (attention_cases.py:18-26).
16-bit: ATTN_ULPS x ULP[dt], the expression of the uncapped test_attention_h16_ragged_segments.  Every output is handed over full of NaN,
every workspace full of 0xFF."""
import ctypes
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import attention_cases as A
import rap_amd
import softcap_cases as SC
import test_h16_gpu as TH
import test_kernels_gpu as TK
import test_x2_gpu as TX
from oracle import rap_oracle as O
from rap_amd import _lib, synthetic as S

pytestmark = pytest.mark.gpu

SWEEP_STARTS = [0, 33, 63]
CAPS = [10.0, 50.0]                 # the sweep's logits reach ~18: 10 bends them hard, 50 barely does
FAMILIES = ["fp32", "x2", "bf16", "f16"]
DT = {"bf16": 1, "f16": 2}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def stream(dev):
    return _lib.current_stream(dev)


def fresh_ws(dev, nbytes):
    return torch.full((max(int(nbytes), 1),), 0xFF, dtype=torch.uint8, device=dev)


def raw_bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def run_capped(lib, dev, family, q, k, v, cu, cap, ws_short=0, expect=0):
    """q, k, v (H, TP, 64) fp32 on the CPU -> (the values (TP, H * 64) on the CPU, the raw output tensor); NaN wherever the call wrote nothing"""
    Hh, TP, _ = q.shape
    cu_d = torch.tensor([int(c) for c in cu], dtype=torch.int32, device=dev)
    nseg = cu_d.numel() - 1
    need = lib.rap_attention_workspace_bytes(TP, nseg)
    ws = fresh_ws(dev, need)
    if family == "fp32":
        hm = torch.stack([q, k, v]).contiguous().to(dev)                     # [3][H][TP][64]
        out = torch.full((TP, Hh * 64), float("nan"), device=dev)
        rc = lib.rap_attention_f32_softcap(_lib.ptr(hm), _lib.ptr(cu_d), nseg, _lib.ptr(out), TP, Hh, cap, _lib.ptr(ws), need - ws_short, stream(dev))
    elif family == "x2":
        qk, vt, nblk = TX.make_x2_attention_operands(q, k, v)
        qk, vt = qk.to(dev), vt.to(dev)
        out = torch.full((TP, 2 * Hh * 64), float("nan"), dtype=torch.float16, device=dev)
        rc = lib.rap_x2_attention_softcap(_lib.ptr(qk), _lib.ptr(vt), nblk, _lib.ptr(cu_d), nseg, _lib.ptr(out), TP, Hh, cap, _lib.ptr(ws), need - ws_short,
                                          stream(dev))
    else:
        dt = DT[family]
        qk, vt, nblk = TH.pack_qkv(q, k, v, dt, dev)
        out = torch.full((TP, Hh * 64), float("nan"), dtype=TH.TORCH_DT[dt], device=dev)
        rc = lib.rap_attention_h16_softcap(dt, _lib.ptr(qk), _lib.ptr(vt), nblk, _lib.ptr(cu_d), nseg, _lib.ptr(out), TP, Hh, cap, _lib.ptr(ws),
                                           need - ws_short, stream(dev))
    torch.cuda.synchronize()
    assert rc == expect, (family, rc)
    raw = out.cpu()
    return (TX.unpack_ref(raw, Hh * 64) if family == "x2" else raw.double()), raw


def rounded(family, q, k, v):
    """the operands the kernel sees: the 16-bit families round them, the fp32-accurate ones do not"""
    if family in DT:
        return tuple(TH.to_h(x, DT[family]).float() for x in (q, k, v))
    return q, k, v


def bound_for(family, q, k, v, cu, cap, ref):
    """-> (bound, the yardstick's error or None)"""
    if family in DT:
        return TH.ATTN_ULPS * TH.ULP[DT[family]], None
    yard = float((SC.attention_f32_plain(q, k, v, cu, cap).double() - ref).abs().max())
    return max(TK.ATTN_BOUND if family == "fp32" else TX.X2_ATTN_BOUND, A.FP32_SHARP_FACTOR * yard), yard


@functools.lru_cache(maxsize=None)
def _sweep_ref(start, cap, rounding):
    q, k, v = rounded(rounding, *A.sweep_operands(start))
    return SC.attention_ref64(q, k, v, A.sweep_table(start), cap)


def sweep_ref(start, cap, family):
    """one float64 reference per (table, cap, rounding of the operands), shared by the parametrisations"""
    return _sweep_ref(start, cap, family if family in DT else "fp32")


# ---------------------------------------------------------------------------------------------
# a. the soft-capped attention kernels
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("start", SWEEP_STARTS)
@pytest.mark.parametrize("family", FAMILIES)
def test_capped_attention_over_the_segment_edge_sweep(lib, dev, family, start, cap):
    """16-bit, measured on an MI355X (max abs error against float64 on the rounded operands, worst over the three tables; bound 8 ulp =
    3.1e-2 bf16, 3.9e-3 fp16) -- capped and, on the same operands through rap_attention_h16, uncapped (the same operands): bf16 4.8e-3 .. 7.3e-3 capped against 5.9e-3 .. 6.8e-3, fp16 7.1e-4 .. 1.2e-3 against 7.1e-4 .. 9.5e-4 -- the
    uncapped test's bound holds as it is."""
    q, k, v = A.sweep_operands(start)
    cu = A.sweep_table(start)
    ref = sweep_ref(start, cap, family)
    qr, kr, vr = rounded(family, q, k, v)
    bound, yard = bound_for(family, qr, kr, vr, cu, cap, ref)
    out, _ = run_capped(lib, dev, family, q, k, v, cu, cap)
    assert not torch.isnan(out).any(), "NaN left in covered rows"
    err = float((out - ref).abs().max())
    line = f"SOFTCAP sweep {family:<5} start {start:<3} cap {cap:<5} max abs err vs fp64 {err:.3e}  (bound {bound:.3e}"
    if family in DT:      # the uncapped kernel on the same operands, for the record
        plain = TH.run_attention_h(lib, dev, DT[family], q, k, v, torch.tensor(cu))
        line += f", uncapped kernel {float((plain.double() - sweep_ref(start, 0.0, family)).abs().max()):.3e}"
    else:
        line += f", yardstick {yard:.3e}"
    print(line + ")")
    bent = float((ref - sweep_ref(start, 0.0, family)).abs().max())
    assert bent > (1e-2 if cap == 10.0 else 1e-7), bent        # (an ignored cap cannot pass: the capped oracle differs from the plain one)
    assert err < bound, (family, start, cap, err, bound)


@pytest.mark.parametrize("family", FAMILIES)
def test_capped_attention_saturates_cleanly(lib, dev, family):
    """One 129-row segment from row 63 (behind a 63-token filler), q and k scaled so that the raw logits reach +-1e3, softcap = 5:
    |s / c| up to 200 -- tanh is +-1 for almost every pair, e^(2 s / c) overflows and underflows inside the kernel's tanh."""
    cu = A.SHARP_TABLES["129-from-63"]
    q, k, v = A.operands(cu[-1], 77)
    lo, hi = A.logits_range(q, k, cu)
    f = (1.0e3 / max(-lo, hi)) ** 0.5
    q, k = q * f, k * f
    lo, hi = A.logits_range(q, k, cu)
    assert max(-lo, hi) > 990.0 and min(-lo, hi) > 500.0, (lo, hi)
    qr, kr, vr = rounded(family, q, k, v)
    ref = SC.attention_ref64(qr, kr, vr, cu, 5.0)
    bound, yard = bound_for(family, qr, kr, vr, cu, 5.0, ref)
    out, _ = run_capped(lib, dev, family, q, k, v, cu, 5.0)
    assert torch.isfinite(out).all(), family
    err = float((out - ref).abs().max())
    print(f"SOFTCAP saturated {family:<5} logits [{lo:.0f}, {hi:.0f}] cap 5: max abs err vs fp64 {err:.3e}  (bound {bound:.3e}, yardstick {yard})")
    assert err < bound, (family, err, bound)


@pytest.mark.parametrize("family", FAMILIES)
def test_capped_single_token_segments_return_v(lib, dev, family):
    g = torch.Generator().manual_seed(3)
    TP, Hh = 130, 2
    q, k, v = (torch.randn(Hh, TP, 64, generator=g) for _ in range(3))
    out, raw = run_capped(lib, dev, family, q, k, v, list(range(TP + 1)), 5.0)
    if family == "x2":
        # split precision: the one probability is exp2 of an FMA's rounding residual (s c - round(s c), not 0) and the fp32 quotient is
        # re-split into a head and a tail, so the UNCAPPED kernel returns split(v) to 2^-20 of max|v|, not its bits
        # (test_x2_attention_single_token_segments_return_v); the capped kernel is held to the same statement
        hi, lo = TX.split_ref(v)
        want = (hi.double() + lo.double()).permute(1, 0, 2).reshape(TP, Hh * 64)
        assert float((out - want).abs().max()) <= 2.0 ** -20 * float(want.abs().max())
    elif family == "fp32":
        assert torch.equal(raw_bits(raw), raw_bits(v.permute(1, 0, 2).reshape(TP, Hh * 64)))
    else:
        assert torch.equal(raw_bits(raw), raw_bits(TH.to_h(v, DT[family]).permute(1, 0, 2).reshape(TP, Hh * 64)))      # softmax over one key is exactly 1


@pytest.mark.parametrize("family", FAMILIES)
def test_capped_attention_leaves_rows_outside_the_table_alone(lib, dev, family):
    cu, TP = [5, 100, 100, 170], 200
    q, k, v = A.operands(TP, 41)
    qr, kr, vr = rounded(family, q, k, v)
    ref = SC.attention_ref64(qr, kr, vr, cu, 10.0)
    out, raw = run_capped(lib, dev, family, q, k, v, cu, 10.0)
    prefill = torch.full_like(raw, float("nan"))
    assert torch.equal(raw_bits(raw[:5]), raw_bits(prefill[:5])) and torch.equal(raw_bits(raw[170:]), raw_bits(prefill[170:]))
    bound, _ = bound_for(family, qr, kr, vr, cu, 10.0, ref)
    err = float((out[5:170] - ref[5:170]).abs().max())
    assert err < bound, (family, err, bound)


@pytest.mark.parametrize("family", FAMILIES)
def test_capped_attention_argument_checks(lib, dev, family):
    cu, TP = [0, 70, 200], 200
    q, k, v = A.operands(TP, 43)
    for cap in (0.0, -1.0, float("nan")):
        _, raw = run_capped(lib, dev, family, q, k, v, cu, cap, expect=-1)
        assert torch.isnan(raw.float()).all(), (family, cap)
    _, raw = run_capped(lib, dev, family, q, k, v, cu, 5.0, ws_short=1, expect=-2)           # one byte short: refused, out unchanged
    assert torch.equal(raw_bits(raw), raw_bits(torch.full_like(raw, float("nan")))), family


# ---------------------------------------------------------------------------------------------
# b. bias + GELU
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 127, 128, 129, 256, 300])
@pytest.mark.parametrize("N", [512, 256])
def test_gemm_bias_gelu_at_the_head_shapes(lib, dev, N, M):
    K = 512
    g = torch.Generator().manual_seed(M + N)
    Am = torch.randn(M, K, generator=g); W = torch.randn(N, K, generator=g) / K ** 0.5; b = torch.randn(N, generator=g)
    ref = F.gelu(Am.double() @ W.double().T + b.double())                  # erf form, nn.GELU()'s default
    C = torch.full((M, N), float("nan"), device=dev)
    TK.gemm(lib, dev, 8, Am.to(dev), W.to(dev), C, M, N, K, bias=b.to(dev))
    err = float((C.cpu().double() - ref).abs().max())
    assert err < TH.F32_OUT_BOUND, (M, N, err)                              # (NaN -- an element never written -- fails this too)
    assert float((ref - F.silu(Am.double() @ W.double().T + b.double())).abs().max()) > 1e-2      # not SiLU's values


@pytest.mark.parametrize("extra,kernel", [(0, 3), (37, 2)], ids=["persistent", "one-tile-256"])
def test_gemm_bias_gelu_on_the_256_tile_kernels(lib, dev, extra, kernel):
    """The smallest M at which N = 512, K = 512 takes the persistent 256 x 256 kernel (read from rap_gemm_f32_form: 65 536 rows, 512 tiles),
    and 37 rows more -- a ragged last row tile, which takes the one-tile-per-block 256 x 256 kernel.  The float64 reference covers the
    first and the last 256 rows and 1024 rows drawn from the rest; every element is checked to be written."""
    N = K = 512
    M = next(m for m in range(256, (1 << 18) + 1, 256) if lib.rap_gemm_f32_form(8, m, N, K, K, K, N, 0, 0, 0) // 100 == 3) + extra
    assert M == 256 * 256 + extra and lib.rap_gemm_f32_form(8, M, N, K, K, K, N, 0, 0, 0) // 100 == kernel
    assert lib.rap_gemm_f32_form(8, 256 * 256 - 256, N, K, K, K, N, 0, 0, 0) // 100 == 1                    # below 512 tiles: 128 x 128
    g = torch.Generator(device=dev).manual_seed(9)
    Ad = torch.randn(M, K, generator=g, device=dev); Wd = torch.randn(N, K, generator=g, device=dev) / K ** 0.5
    bd = torch.randn(N, generator=g, device=dev)
    C = torch.full((M, N), float("nan"), device=dev)
    TK.gemm(lib, dev, 8, Ad, Wd, C, M, N, K, bias=bd)
    assert bool(torch.isfinite(C).all())
    rows = torch.cat([torch.arange(256), torch.arange(M - 256, M), torch.randint(256, M - 256, (1024,), generator=torch.Generator().manual_seed(1))])
    ref = F.gelu(Ad[rows.to(dev)].cpu().double() @ Wd.cpu().double().T + bd.cpu().double())
    err = float((C[rows.to(dev)].cpu().double() - ref).abs().max())
    assert err < TH.F32_OUT_BOUND, err


# ---------------------------------------------------------------------------------------------
# c. the model
# ---------------------------------------------------------------------------------------------
def to_dev(inp, dev):
    return {k: v.to(dev) for k, v in inp.items()}


def build(name, mode, dev, **override):
    g, inp = SC.load_fixture(name)
    kw = dict(SC.FIXTURES[name])
    cfg = dict(S.RAP_12); cfg["num_layers"] = int(g["num_layers"]); cfg["qk_norm"] = kw["qk_norm"]
    sd = S.make_weights(cfg, int(g["weight_seed"]))
    assert abs(sum(t.double().sum().item() for t in sd.values()) - float(g["weights_checksum"])) < 1e-6
    args = dict(qk_norm=kw["qk_norm"], softcap=kw["softcap"], final_mlp_act=SC.act_class(kw["final_mlp_act"]))
    args.update(override)
    model = rap_amd.PointCloudDiT(in_dim=0, out_dim=3, embed_dim=512, num_layers=cfg["num_layers"], num_heads=8, local_feat_dim=32,
                                  attn_dtype="float32", compute_dtype=mode, **args)
    model.load_state_dict(sd)
    return g, inp, kw, model.to(dev)


def forward(model, inp, g, dev):
    cu_b, cu_p = O.prepare_cu_seqlens(inp)
    d = to_dev(inp, dev)
    return model(x=d["x_1"], timesteps=torch.from_numpy(g["fwd_timesteps"]).to(dev), cond_coord=d["pointclouds"], local_features=d["features"],
                 latent_features=None, scales=d["scales"], anchor_indices=d["anchor_indices"], cu_seqlens_batch=cu_b.to(dev),
                 cu_seqlens_part=cu_p.to(dev))


@pytest.mark.parametrize("mode", ["float32", "float32x2", "bfloat16"])
@pytest.mark.parametrize("name", list(SC.FIXTURES))
def test_switched_models_match_reference_golden(lib, dev, name, mode):
    """One forward and the whole sampling call against the fixture the unmodified reference wrote with the same switches, held to
    test_constructor_switches_match_reference_golden's asserts.  float32x2 runs with tuning key 17 = 0, so that the split-precision kernels
    take this 328-token call (by default such a model runs it on the fp32 kernels).  The bfloat16 class bound cannot tell an ignored cap from
    an honoured one (the cap moves the velocity by 5e-3, the bound is 3e-2): the kernel-level tests above carry the 16-bit proof."""
    g, inp, kw, model = build(name, mode, dev)
    try:
        if mode == "float32x2":
            assert lib.rap_set_tuning(17, 0) == 0
        v = forward(model, inp, g, dev)
        v_ref = torch.from_numpy(g["fwd_velocity"])
        ev = float((v.cpu() - v_ref).abs().max())
        d = to_dev(inp, dev)
        flow = rap_amd.RectifiedPointFlow(flow_model=model, inference_sampling_steps=int(g["num_steps"]), rigidity_forcing=bool(g["rigidity"]))
        res = flow.sample_rectified_flow(d, None, x_1=d["x_1"])
        e0 = float((res["end_point_trajectory"].cpu() - torch.from_numpy(g["end_point_trajectory"])).abs().max())
        e1 = float((res["trajectory"].cpu() - torch.from_numpy(g["trajectory"])).abs().max())
        R, t = flow.last_poses
    finally:
        assert lib.rap_set_tuning(17, 1024) == 0
    print(f"SOFTCAP model {name} [{mode}]: velocity {ev:.2e} (1e-4 max|v| = {1e-4 * float(v_ref.abs().max()):.2e})  x0 {e0:.2e}  xt {e1:.2e}")
    assert lib.rap_model_compute_dtype(model._handle) == _lib.DTYPES[mode]
    assert lib.rap_model_softcap(model._handle) == ctypes.c_float(kw["softcap"]).value
    assert lib.rap_model_final_act(model._handle) == SC.ACT_CODE[kw["final_mlp_act"]]
    assert lib.rap_model_qk_norm(model._handle) == int(kw["qk_norm"])
    if kw["softcap"] > 0:
        assert lib.rap_model_bounded_attention_launches(model._handle) == 0
    else:
        assert lib.rap_model_bounded_attention_launches(model._handle) == 2 * int(g["num_layers"])
    if mode == "bfloat16":
        assert ev <= 3e-2 * max(1.0, float(v_ref.abs().max())) and e0 <= 5e-2 and e1 <= 5e-2, (ev, e0, e1)
        return
    assert ev <= 1e-4 * float(v_ref.abs().max()) and ev < 2e-5, ev
    assert e0 < 5e-5 and e1 < 5e-5, (e0, e1)
    assert float(torch.linalg.matrix_norm(R.cpu() - torch.from_numpy(g["R"])).max()) < 1e-4
    assert float((t.cpu() - torch.from_numpy(g["t"])).abs().max()) < 1e-4


@pytest.mark.parametrize("mode", ["float32", "float32x2", "bfloat16"])
def test_softcap_zero_and_silu_are_the_default_model_bit_for_bit(lib, dev, mode):
    name = "l2_softcap1_rigid"
    g, inp, _, default = build(name, mode, dev, softcap=0.0, final_mlp_act=None)
    _, _, _, explicit = build(name, mode, dev, softcap=0.0, final_mlp_act=nn.SiLU)
    _, _, _, capped = build(name, mode, dev)
    try:
        if mode == "float32x2":
            assert lib.rap_set_tuning(17, 0) == 0
        a, b, c = (forward(m, inp, g, dev) for m in (default, explicit, capped))
    finally:
        assert lib.rap_set_tuning(17, 1024) == 0
    assert lib.rap_model_softcap(explicit._handle) == 0.0 and lib.rap_model_final_act(explicit._handle) == 0
    assert torch.equal(raw_bits(a), raw_bits(b))
    plain = torch.from_numpy(g["fwd_velocity_plain"])
    if mode != "bfloat16":
        assert float((a.cpu() - plain).abs().max()) <= 1e-4 * float(plain.abs().max())            # ... and that is the reference's plain model
    assert float((c - a).abs().max()) > 1e-3                                                       # the cap is not ignored (the reference: 5e-3)


def test_setters_on_a_live_handle(lib, dev):
    g, inp, kw, model = build("l2_gelu_rigid", "float32", dev)
    h = model._handle
    try:
        for bad in (-1.0, float("nan"), float("inf")):
            assert lib.rap_model_set_softcap(h, bad) == -1
        assert lib.rap_model_softcap(h) == 0.0
        assert lib.rap_model_set_softcap(h, 2.5) == 0 and lib.rap_model_softcap(h) == 2.5
        assert lib.rap_model_bounded_attention_launches(h) == 0
        assert lib.rap_model_set_softcap(h, 0.0) == 0 and lib.rap_model_bounded_attention_launches(h) == 2 * int(g["num_layers"])
        for bad in (-1, 3, 100):
            assert lib.rap_model_set_final_act(h, bad) == -1
        assert lib.rap_model_final_act(h) == 1
        for act in (0, 2, 1):
            assert lib.rap_model_set_final_act(h, act) == 0 and lib.rap_model_final_act(h) == act
    finally:
        assert lib.rap_model_set_softcap(h, 0.0) == 0 and lib.rap_model_set_final_act(h, 1) == 0
    # ... and both switches are set again on a re-created native handle
    g, inp, kw, capped = build("l2_softcap1_relu_rigid", "float32", dev)
    before = forward(capped, inp, g, dev)
    capped._release()
    assert not capped._handle
    after = forward(capped, inp, g, dev)
    assert lib.rap_model_softcap(capped._handle) == 1.0 and lib.rap_model_final_act(capped._handle) == 2
    assert torch.equal(raw_bits(before), raw_bits(after))


@pytest.mark.parametrize("mode", ["float32", "float32x2"])
def test_capped_call_stays_inside_exactly_rap_workspace_bytes(monkeypatch, lib, dev, mode):
    """rap_workspace_bytes against the capped plan: a forward and a sampling call of a capped model with the ReLU head inside an exactly
    sized, 0xFF-filled workspace between guard bands (tests/guards.py), same bits as on the ordinary shared buffer"""
    import test_guards_workspace_gpu as TGW
    g, inp, kw, model = build("l2_softcap1_relu_rigid", mode, dev)
    d = to_dev(inp, dev)
    flow = rap_amd.RectifiedPointFlow(flow_model=model, inference_sampling_steps=2, rigidity_forcing=True, num_streams=1)

    def sample():
        out = flow.sample_rectified_flow(d, None, x_1=d["x_1"], return_tarjectory=True)
        flow.synchronize()
        return {"trajectory": out["trajectory"], "R": flow.last_poses[0], "t": flow.last_poses[1]}
    try:
        if mode == "float32x2":
            assert lib.rap_set_tuning(17, 0) == 0
        fwd = TGW.exact_against_shared(monkeypatch, lambda: forward(model, inp, g, dev), f"capped forward {mode}", 1)
        smp = TGW.exact_against_shared(monkeypatch, sample, f"capped sample_rectified_flow {mode}")
    finally:
        assert lib.rap_set_tuning(17, 1024) == 0
    assert torch.isfinite(fwd).all() and torch.isfinite(smp["R"]).all()
    assert float((fwd.cpu() - torch.from_numpy(g["fwd_velocity"])).abs().max()) < 2e-5


def test_capped_sampling_call_replays_from_a_graph_bit_for_bit(lib, dev):
    g, inp, kw, model = build("l2_softcap1_relu_rigid", "float32", dev)
    flow = rap_amd.RectifiedPointFlow(flow_model=model, inference_sampling_steps=3, rigidity_forcing=True)
    a = to_dev(inp, dev)
    b = to_dev(S.make_inputs([[60, 41], [130, 20, 77]], seed=52), dev)          # same geometry, other clouds / features / noise
    static = {k: v.clone() for k, v in a.items()}
    flow.sample_and_register(static, x_1=static["x_1"])                          # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = flow.sample_and_register(static, x_1=static["x_1"])
    for src in (b, a):
        for k in static:
            static[k].copy_(src[k])
        graph.replay()
        torch.cuda.synchronize()
        eager = flow.sample_and_register(src, x_1=src["x_1"])
        for k in ("end_point_trajectory", "trajectory", "R", "t"):
            assert torch.equal(out[k], eager[k]), k
    e0 = float((out["end_point_trajectory"].cpu() - torch.from_numpy(g["end_point_trajectory"])).abs().max())
    assert e0 < 5e-5, e0                                                          # (the last replay ran the fixture's inputs)
