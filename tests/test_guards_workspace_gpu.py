"""Guard-band tests of the Python surface: every wrapper and the model path run with EXACTLY the scratch their ``rap_*_workspace_bytes``
query returned.

``rap_amd``'s wrappers take their scratch from one grow-only buffer, so in the rest of the suite every call after the first large one
runs with more scratch than it asked for and an under-reporting query (or a kernel that runs past the carved total) is invisible.  Here
``guards.exact_workspaces`` hands every request a fresh buffer of exactly the requested bytes between guard bands; after the call every
guard must be intact and the result must be BITWISE equal to the same call on the ordinary shared buffer (a result that changes with
the amount of scratch is a finding too).  What the guards see and do not see: tests/guards.py.
"""
import os

import numpy as np
import pytest
import torch

import guards as G
import rap_amd
from conftest import ROOT
from oracle import rap_oracle as O
from rap_amd import _lib, flow_model, metrics, procrustes, selection, synthetic as S
from width_cases import width_cfg

pytestmark = pytest.mark.gpu

TABLE = [[37, 0, 100], [2049, 1]]        # an empty part in the middle, a part one past the 2048-point chunk, a one-point part


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    d = torch.device("cuda:0")
    flow_model.workspace(d, 64 << 20)                     # the ordinary shared buffer: far more scratch than any call here asks for
    return d


def same_bits(a, b, what):
    if isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and a.shape == b.shape, what
        assert torch.equal(a.reshape(-1).contiguous().view(torch.uint8), b.reshape(-1).contiguous().view(torch.uint8)), f"{what}: the result changes with the amount of scratch"
    elif isinstance(a, dict):
        assert list(a) == list(b), what
        for k in a:
            same_bits(a[k], b[k], f"{what}[{k!r}]")
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            same_bits(x, y, f"{what}[{i}]")
    else:
        assert a == b, what


def exact_against_shared(monkeypatch, call, what, n_workspaces=None):
    """call() on the shared buffer, then under exact workspaces: guards intact, same bits"""
    shared = call()
    torch.cuda.synchronize()
    ex = G.exact_workspaces(monkeypatch)
    try:
        exact = call()
        torch.cuda.synchronize()
        ex.check_all()
    finally:
        monkeypatch.undo()
    if n_workspaces is not None:
        assert len(ex.handed) == n_workspaces, (what, len(ex.handed))
    same_bits(shared, exact, what)
    return exact


@pytest.fixture(scope="module")
def batch(dev):
    inp = S.make_inputs(TABLE, seed=5)
    g = torch.Generator().manual_seed(10)
    pred = inp["pointclouds_gt"] + 0.05 * torch.randn(inp["pointclouds_gt"].shape, generator=g)
    d = {k: v.to(dev) for k, v in inp.items()}
    d["pred"] = pred.to(dev)
    d["cpu"] = inp
    d["pred_cpu"] = pred
    return d


def test_procrustes_wrappers_with_exact_workspaces(monkeypatch, dev, batch):
    cond, pred, ppp, cu = batch["pointclouds"], batch["pred"], batch["points_per_part"], batch["cu_seqlens"]
    R, t = exact_against_shared(monkeypatch, lambda: procrustes.fit_transformations(cond, pred, ppp, cu), "fit_transformations", 1)
    from test_guards_callers_gpu import procrustes_per_part
    Rr, tr, _ = procrustes_per_part(batch["cpu"]["pointclouds"], batch["pred_cpu"], batch["cpu"]["points_per_part"])
    well = batch["cpu"]["points_per_part"] >= 3                                 # (a one-point part fixes no rotation)
    assert (R.cpu().double() - Rr)[well].abs().max().item() < 2e-6 and (t.cpu().double() - tr)[well].abs().max().item() < 2e-6      # (tests/test_kernels_gpu.py)
    assert torch.equal(R.cpu()[0, 1], torch.zeros(3, 3)) and torch.equal(R.cpu()[1, 2], torch.zeros(3, 3))               # the empty parts
    exact_against_shared(monkeypatch, lambda: procrustes.rigidify_prediction_with_procrustes(pred, cond, ppp, cu), "rigidify", 1)
    exact_against_shared(monkeypatch, lambda: procrustes.rigidify_blend(pred, cond, ppp, batch["x_1"], 0.35, 0.65), "rigidify_blend", 1)


def test_rigidity_rmse_wrappers_with_exact_workspaces(monkeypatch, dev, batch):
    cond, pred, ppp, cu, sc = batch["pointclouds"], batch["pred"], batch["points_per_part"], batch["cu_seqlens"], batch["scales"]
    R, t = procrustes.fit_transformations(cond, pred, ppp, cu)
    for per_part in (False, True):
        out = exact_against_shared(monkeypatch, lambda: selection.compute_rigidity_rmse(cond, pred, R, t, ppp, cu, sc, per_part), "rigidity_rmse", 1)
        assert torch.isfinite(out).all()
    traj = torch.stack([pred, batch["pointclouds_gt"], pred * 0.9])
    exact_against_shared(monkeypatch, lambda: selection.average_trajectory_rigidity_rmse(cond, traj, ppp, cu, sc, return_per_step=True),
                         "trajectory rigidity_rmse", 1)
    exact_against_shared(monkeypatch, lambda: selection.average_trajectory_rigidity_rmse(cond, traj, ppp, cu, sc), "trajectory rigidity_rmse (own per-step)", 1)


def test_nearest_neighbour_wrappers_with_exact_workspaces(monkeypatch, dev, batch):
    pred, gt, ppp, cu = batch["pred"], batch["pointclouds_gt"], batch["points_per_part"], batch["cu_seqlens"]
    exact_against_shared(monkeypatch, lambda: selection.compute_overlap_ratio(pred, ppp, cu, return_min_distances=True), "overlap_ratio", 1)
    exact_against_shared(monkeypatch, lambda: selection.compute_overlap_ratio(pred, ppp, cu), "overlap_ratio (own min-dist)", 1)
    cd = exact_against_shared(monkeypatch, lambda: metrics.compute_cd(gt, pred, cu), "compute_cd", 1)
    assert torch.isfinite(cd).all()
    for ns, nt in ((1, 257), (255, 1), (257, 255)):
        sg, tg = gt[:ns], gt[300:300 + nt]
        sp, tp = pred[:ns], pred[300:300 + nt]
        exact_against_shared(monkeypatch, lambda: metrics.compute_correspondence_rmse(sg, tg, sp, tp, 0.5), f"correspondence_rmse {ns} x {nt}", 1)


def pair_fixture(dev):
    z = np.load(os.path.join(ROOT, "tests", "golden", "evaluator_pairs.npz"))
    keys = ("pointclouds", "pointclouds_gt", "points_per_part", "anchor_parts", "anchor_indices", "scales", "rotations", "translations",
            "cu_seqlens_batch", "cu_seqlens_part")
    data = {k: torch.from_numpy(z[k]).to(dev) for k in keys}
    pred = {k: torch.from_numpy(z[k]).to(dev) for k in ("pointclouds_pred", "rotations_pred", "translations_pred")}
    return z, data, pred


def test_pair_metrics_and_evaluator_with_exact_workspaces(monkeypatch, dev):
    z, data, pred = pair_fixture(dev)
    pm = exact_against_shared(monkeypatch, lambda: metrics.compute_pair_metrics(data, data["pointclouds"], pred["rotations_pred"],
                                                                                  pred["translations_pred"]), "pair_metrics (transformed)", 1)
    assert np.array_equal(pm[:, 3].cpu().numpy().astype(np.int64), z["pair_count64"])      # (tests/test_evaluator_gpu.py)
    exact_against_shared(monkeypatch, lambda: metrics.compute_pair_metrics(data, pred["pointclouds_pred"]), "pair_metrics (direct)", 1)
    for on, transformed in ((True, True), (True, False), (False, True)):
        ev = rap_amd.Evaluator(rmse_eval_on=on, rmse_eval_on_transformed=transformed)
        out = exact_against_shared(monkeypatch, lambda: ev.compute_metrics(data, pred["pointclouds_pred"], pred["rotations_pred"],
                                                                            pred["translations_pred"]), f"Evaluator.compute_metrics on={on}")
        assert list(out) == list(z[f"{'off' if not on else ('transformed' if transformed else 'direct')}/keys"])


def test_transform_and_collate_with_exact_workspaces(monkeypatch, dev):
    g = torch.Generator().manual_seed(3)
    samples = []
    for sizes in TABLE:
        parts = [torch.randn(n, 3, generator=g, dtype=torch.float64) * 4 + 100 for n in sizes if n]
        samples.append({"parts": parts, "features": [torch.randn(p.shape[0], 8, generator=g) for p in parts]})

    def call():
        np.random.seed(7)
        out = rap_amd.transform_and_collate(samples, 3, device=dev)
        return {k: v for k, v in out.items() if isinstance(v, torch.Tensor)}
    out = exact_against_shared(monkeypatch, call, "transform_and_collate", 1)
    assert out["cu_seqlens"].tolist() == [0, 137, 137 + 2050] and out["points_per_part"].tolist() == [[37, 100, 0], [2049, 1, 0]]
    assert all(torch.isfinite(v).all() for v in out.values() if v.is_floating_point())


def test_minispinnet_describe_with_exact_workspaces(monkeypatch, dev):
    """5 keypoints in chunks of 4: the second chunk holds one keypoint, the workspace is the one of a 4-keypoint chunk"""
    from rap_amd.spinnet import MiniSpinNet, make_spinnet_weights
    net = MiniSpinNet(des_r=0.25, keypoints_per_chunk=4)
    net.load_state_dict(make_spinnet_weights(1))
    net.to(dev)
    g = torch.Generator().manual_seed(2)
    pts = torch.rand(3000, 3, generator=g)
    kpts = pts[torch.randperm(3000, generator=g)[:5]]
    perm = torch.randperm(3000, generator=g).numpy()
    desc = exact_against_shared(monkeypatch, lambda: net(pts[None].to(dev), kpts[None].to(dev), 0.25, True, perm=perm)["desc"], "MiniSpinNet", 1)
    assert torch.isfinite(desc).all() and (desc.norm(dim=1) - 1).abs().max().item() < 1e-5            # unit-norm descriptors


# ---------------------------------------------------------------------------------------------
# PointCloudDiT.forward and sample_rectified_flow at exactly rap_workspace_bytes
# ---------------------------------------------------------------------------------------------
BATCHES = {"380-tokens-padded-empty-part": [[37, 64, 100], [50, 129]], "8-tokens": [[5, 3]]}
MODES = [("float32", None, False), ("bfloat16", "float32", False), ("bfloat16", "float16", False), ("float16", "float32", False),
         ("float16", "float16", False), ("float32x2", None, False), ("float32x2", None, True)]
_MODELS = {}


def model_for(dev, cdt, rdt):
    if (cdt, rdt) not in _MODELS:
        cfg = width_cfg(256, 4)
        cfg["num_layers"] = 2
        m = rap_amd.PointCloudDiT(in_dim=0, out_dim=3, embed_dim=256, num_layers=2, num_heads=4, local_feat_dim=cfg["local_feat_dim"],
                                  compute_dtype=cdt, residual_dtype=rdt)
        m.load_state_dict(S.make_weights(cfg, 0))
        _MODELS[(cdt, rdt)] = (cfg, m.to(dev))
    return _MODELS[(cdt, rdt)]


@pytest.mark.parametrize("geom", list(BATCHES))
@pytest.mark.parametrize("cdt,rdt,force_split", MODES, ids=[f"{c}-{r or 'f32'}-stream{'-forced' if f else ''}" for c, r, f in MODES])
def test_model_forward_and_sampling_with_exact_workspaces(monkeypatch, dev, cdt, rdt, force_split, geom):
    """2 layers, d = 256, 2 flow steps with rigidity forcing.  TP = 380 is no multiple of 256 (the token-row buffers are carved at 512
    rows) and its second sample has a padded empty part; 8 tokens take every few-token form.  `forced`: tuning key 17 = 0, so that the
    split-precision kernels run at these sizes (by default a float32x2 model runs calls this small on the fp32 kernels, inside the
    same carve)."""
    lib = _lib.load()
    cfg, model = model_for(dev, cdt, rdt)
    inp = S.make_inputs(BATCHES[geom], seed=11, feat_dim=cfg["local_feat_dim"])
    cu_b, cu_p = O.prepare_cu_seqlens(inp)
    d = {k: v.to(dev) for k, v in inp.items()}
    B = len(BATCHES[geom])
    ts = torch.linspace(1.0, 0.4, B).to(dev)
    flow = rap_amd.RectifiedPointFlow(flow_model=model, inference_sampling_steps=2, rigidity_forcing=True, num_streams=1)

    def forward():
        return model(x=d["x_1"], timesteps=ts, cond_coord=d["pointclouds"], local_features=d["features"], latent_features=None, scales=d["scales"],
                     anchor_indices=d["anchor_indices"], cu_seqlens_batch=cu_b.to(dev), cu_seqlens_part=cu_p.to(dev), return_transformer_features=True)

    def sample():
        out = flow.sample_rectified_flow(d, None, x_1=d["x_1"], return_tarjectory=True, return_transformer_features=True)
        flow.synchronize()
        return {"trajectory": out["trajectory"], "transformer_features": out["transformer_features"], "R": flow.last_poses[0], "t": flow.last_poses[1]}
    try:
        if force_split:
            assert lib.rap_set_tuning(17, 0) == 0
        fwd = exact_against_shared(monkeypatch, forward, f"forward {cdt}", 1)
        smp = exact_against_shared(monkeypatch, sample, f"sample_rectified_flow {cdt}")
    finally:
        assert lib.rap_set_tuning(17, 1024) == 0
    assert torch.isfinite(fwd["velocity"]).all() and torch.isfinite(fwd["transformer_features"]).all()
    assert all(torch.isfinite(v).all() for v in smp["trajectory"].values()) and torch.isfinite(smp["R"]).all()


def test_model_entry_points_refuse_a_short_workspace_without_writing(dev):
    """rap_dit_forward / rap_sample with ws_bytes = rap_workspace_bytes - 1: RAP_ERR_WORKSPACE, every output and the workspace still
    0xFF, every guard intact"""
    import ctypes
    lib = _lib.load()
    cfg, model = model_for(dev, "bfloat16", "float16")
    handle = model._activate(dev)
    inp = S.make_inputs(BATCHES["380-tokens-padded-empty-part"], seed=11, feat_dim=cfg["local_feat_dim"])
    cu_b, cu_p = O.prepare_cu_seqlens(inp)
    d = {k: v.to(dev) for k, v in inp.items()}
    TP, (B, P), S_ = inp["x_1"].shape[0], inp["points_per_part"].shape, 2
    VP = cu_p.numel() - 1
    ts = torch.linspace(1.0, 0.4, B).to(dev)
    anchor = d["anchor_indices"].to(torch.uint8)
    cu_b32, cu_p32 = cu_b.to(device=dev, dtype=torch.int32), cu_p.to(device=dev, dtype=torch.int32)
    stream = _lib.current_stream(dev)
    out = lambda shape, name: G.Guarded(int(np.prod(shape)) * 4, dev, 0xFF, pitch=shape[-1] * 4, name=name)

    need = lib.rap_workspace_bytes(handle, TP, B, VP, B)
    guards = [out((TP, 3), "v_out"), out((TP, 256), "feats_out"), G.Guarded(need, dev, 0xFF, pitch=8192, name="workspace")]
    rc = lib.rap_dit_forward_latent(handle, _lib.ptr(d["x_1"]), _lib.ptr(ts), _lib.ptr(d["pointclouds"]), _lib.ptr(d["features"]), None,
                                    _lib.ptr(d["scales"]), _lib.ptr(anchor), _lib.ptr(cu_b32), _lib.ptr(cu_p32), B, VP, TP,
                                    ctypes.c_void_p(guards[0].ptr), ctypes.c_void_p(guards[1].ptr), ctypes.c_void_p(guards[2].ptr), need - 1, stream)
    assert rc == -2
    need_s = lib.rap_workspace_bytes(handle, TP, B, B * P, S_)
    guards += [out((S_, TP, 3), "traj_x0"), out((S_, TP, 3), "traj_xt"), out((B, P, 3, 3), "R_out"), out((B, P, 3), "t_out"),
               out((TP, 256), "feats_out"), G.Guarded(need_s, dev, 0xFF, pitch=8192, name="workspace")]
    s = guards[3:]
    rc = lib.rap_sample_latent(handle, _lib.ptr(d["pointclouds"]), _lib.ptr(d["features"]), None, _lib.ptr(d["scales"]), _lib.ptr(anchor),
                               _lib.ptr(d["points_per_part"]), _lib.ptr(cu_b32), _lib.ptr(d["x_1"]), B, P, TP, S_, 1, ctypes.c_void_p(s[0].ptr),
                               ctypes.c_void_p(s[1].ptr), ctypes.c_void_p(s[2].ptr), ctypes.c_void_p(s[3].ptr), ctypes.c_void_p(s[4].ptr),
                               ctypes.c_void_p(s[5].ptr), need_s - 1, stream)
    assert rc == -2
    torch.cuda.synchronize()
    for g in guards:
        g.check()
        assert g.untouched(), g.name


# ---------------------------------------------------------------------------------------------
# rap_gemm_f32_splitk at exactly rap_gemm_f32_splitk_workspace_bytes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epi,planes", [(1, 0), (2, 2), (2, 4)], ids=["resid", "silu-2-planes", "silu-4-planes"])
def test_gemm_f32_splitk_stays_inside_its_exact_workspace(dev, epi, planes):
    """The fp32 split-K entry point (kernel-level, like tests/test_guards_gpu.py: every output and the workspace between guard bytes, every
    input between 0x00 and then 0xFF neighbours) over the row counts of that file: the partial planes fill the reported workspace exactly
    -- 17 k-tiles over 4 blocks for the residual form, so the last share is the long one -- and one byte less is refused with nothing
    written."""
    import ctypes
    import torch.nn.functional as F
    import test_guards_gpu as TG
    import test_kernels_gpu as TK
    lib = _lib.load()
    N, K = (512, 544) if epi == 1 else (384, 512)
    for M in TG.MS:
        need = lib.rap_gemm_f32_splitk_workspace_bytes(epi, M, N, K, planes)
        assert need == (4 if epi == 1 else planes) * M * N * 4
        g = torch.Generator().manual_seed(47 + M)
        A = torch.randn(M, K, generator=g); W = torch.randn(N, K, generator=g) / K ** 0.5
        bias = torch.randn(N, generator=g); h = torch.randn(M, N, generator=g)
        u = A.double() @ W.double().T + bias.double()
        ref = h.double() + u if epi == 1 else F.silu(u)

        def call(c, ws_bytes):
            C = c.out_view(torch.float32, (M, N), "C")
            ws = c.out(need, pitch=N * 4, name="split-K workspace")
            Ad, Wd, bd = c.inp(A, "A"), c.inp(W, "W"), c.inp(bias, "bias")
            hd = c.inp(h, "resid") if epi == 1 else None
            rc = lib.rap_gemm_f32_splitk(epi, _lib.ptr(Ad), K, _lib.ptr(Wd), K, _lib.ptr(C), N, M, N, K, _lib.ptr(bd), _lib.ptr(hd), N if epi == 1 else 0,
                                         planes, ctypes.c_void_p(ws.ptr), ws_bytes, _lib.current_stream(dev))
            torch.cuda.synchronize()
            return rc, C

        def run(c):
            rc, C = call(c, need)
            assert rc == 0
            assert (C.cpu().double() - ref).abs().max().item() < TK.GEMM_BOUND, M          # NaN (an element never written) fails this too
            return [C]
        TG.run_both(dev, run)
        c = TG.Case(dev, 0x00)                                                      # one byte short: refused, nothing written
        rc, C = call(c, need - 1)
        assert rc == TG.RAP_ERR_WORKSPACE
        c.check()
        assert bool(torch.isnan(C).all())
