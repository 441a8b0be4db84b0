"""Guard-band tests of the entry points either side of the sampling path (Procrustes, collate, outlier removal, voxel down-sampling,
farthest point sampling, MiniSpinNet, generation selection, nearest-neighbour metrics), through the C ABI: per-point outputs sized
exactly, workspaces at exactly the queried bytes, a short workspace refused without a byte written, and -- for the four
nearest-neighbour entry points -- results independent of what lies beyond the inputs.  Harness and limits: tests/test_guards_gpu.py and
tests/guards.py (an overrun longer than the pad and a read that reaches no result are not seen)."""
import ctypes

import numpy as np
import pytest
import torch

import guards as G
import rap_amd
import test_preproc_scale_gpu as TPS
from oracle import preproc_cases as PC
from oracle import rap_oracle as O
from rap_amd import _lib, metrics, synthetic as S
from test_guards_gpu import F32, I32, I64, U8, RAP_ERR_WORKSPACE, Case, refused_call_wrote_nothing, run_both, stream

pytestmark = pytest.mark.gpu

TABLE = [[37, 0, 100], [2049, 1]]        # an empty part in the middle, a part one past the 2048-point chunk, a one-point part
P2 = ctypes.c_void_p


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def table_batch():
    inp = S.make_inputs(TABLE, seed=5)
    g = torch.Generator().manual_seed(10)
    inp["pred"] = inp["pointclouds_gt"] + 0.05 * torch.randn(inp["pointclouds_gt"].shape, generator=g)
    return inp


# ---------------------------------------------------------------------------------------------
# Procrustes: rap_fit_transformations, rap_rigidify, rap_rigidify_blend
# ---------------------------------------------------------------------------------------------
def procrustes_per_part(cond, pred, ppp):
    """fp64 O.solve_procrustes part by part, from offsets -> (R (B,P,3,3), t (B,P,3), rigidified cloud (TP,3)).  (The oracle's own
    fit_transformations keeps the reference's indexing, which cannot take an empty part in front of a non-empty one:
    tests/test_kernels_gpu.py::test_procrustes_empty_part_in_the_middle.)"""
    B, P = ppp.shape
    R, t = torch.zeros(B, P, 3, 3, dtype=torch.float64), torch.zeros(B, P, 3, dtype=torch.float64)
    rig = torch.zeros(cond.shape, dtype=torch.float64)
    off = 0
    for b in range(B):
        for p in range(P):
            n = int(ppp[b, p])
            if n:
                src = cond[off:off + n].double()
                R[b, p], t[b, p] = O.solve_procrustes(src, pred[off:off + n].double())
                rig[off:off + n] = src @ R[b, p].T + t[b, p]
            off += n
    return R, t, rig


def test_procrustes_entry_points_write_only_their_poses_and_points(lib, dev, table_batch):
    b = table_batch
    cond, pred, ppp, cu, x1 = b["pointclouds"], b["pred"], b["points_per_part"], b["cu_seqlens"], b["x_1"]
    B, P = ppp.shape
    TP = cond.shape[0]
    need = lib.rap_procrustes_workspace_bytes(B * P)
    Rr, tr, rig_ref = procrustes_per_part(cond, pred, ppp)
    w0, w1 = 0.35, 0.65

    def fit(c, short=0):
        R, t = c.out_view(F32, (B, P, 3, 3), "R_out"), c.out_view(F32, (B, P, 3), "t_out")
        ws = c.out(need, name="procrustes workspace")
        rc = lib.rap_fit_transformations(_lib.ptr(c.inp(cond)), _lib.ptr(c.inp(pred)), _lib.ptr(c.inp(ppp)), B, P, _lib.ptr(R), _lib.ptr(t),
                                         P2(ws.ptr), need - short, stream(dev))
        torch.cuda.synchronize()
        return rc, R, t

    def rigidify(c, short=0):
        out = c.out_view(F32, (TP, 3), "out")
        ws = c.out(need, name="procrustes workspace")
        rc = lib.rap_rigidify(_lib.ptr(c.inp(pred)), _lib.ptr(c.inp(cond)), _lib.ptr(c.inp(ppp)), B, P, _lib.ptr(out), P2(ws.ptr), need - short,
                              stream(dev))
        torch.cuda.synchronize()
        return rc, out

    def blend(c, short=0):
        out = c.out_view(F32, (TP, 3), "x_t_out")
        ws = c.out(need, name="procrustes workspace")
        rc = lib.rap_rigidify_blend(_lib.ptr(c.inp(pred)), _lib.ptr(c.inp(cond)), _lib.ptr(c.inp(ppp)), B, P, _lib.ptr(c.inp(x1)), w0, w1,
                                    _lib.ptr(out), P2(ws.ptr), need - short, stream(dev))
        torch.cuda.synchronize()
        return rc, out

    def run_fit(c):
        rc, R, t = fit(c)
        assert rc == 0
        well = ppp >= 3                                         # (a one-point part fixes no rotation: its pose is held to what it must do, below)
        assert (R.cpu().double() - Rr)[well].abs().max().item() < 2e-6 and (t.cpu().double() - tr)[well].abs().max().item() < 2e-6   # (tests/test_kernels_gpu.py)
        moved = cond[-1].double() @ R.cpu()[1, 1].double().T + t.cpu()[1, 1].double()
        assert (moved - pred[-1].double()).abs().max().item() < 2e-6 and abs(float(torch.det(R.cpu()[1, 1].double())) - 1) < 1e-5
        assert torch.equal(R.cpu()[0, 1], torch.zeros(3, 3)) and torch.equal(t.cpu()[1, 2], torch.zeros(3))               # empty parts: zero rows
        return [R, t]

    def run_rigidify(c):
        rc, out = rigidify(c)
        assert rc == 0 and (out.cpu().double() - rig_ref).abs().max().item() < 2e-6
        return [out]

    def run_blend(c):
        rc, out = blend(c)
        # rigidify's 2e-6 times w0, plus three fp32 roundings (two products, one sum) of values below 8: 3 * 8 * 2^-24 < 1.5e-6
        ref = rig_ref * float(np.float32(w0)) + x1.double() * float(np.float32(w1))
        assert rc == 0 and (out.cpu().double() - ref).abs().max().item() < 2e-6 * w0 + 1.5e-6
        return [out]
    for run, call in ((run_fit, fit), (run_rigidify, rigidify), (run_blend, blend)):
        run_both(dev, run)
        refused_call_wrote_nothing(dev, call)


def test_rigidity_rmse_entry_points_write_only_their_rows(lib, dev, table_batch):
    b = table_batch
    cond, pred, ppp, cu, sc = b["pointclouds"], b["pred"], b["points_per_part"], b["cu_seqlens"], b["scales"]
    B, P = ppp.shape
    TP, steps = cond.shape[0], 3
    d = lambda t: t.to(dev)
    R, t = rap_amd.fit_transformations(d(cond), d(pred), ppp, cu)
    traj = torch.stack([pred, b["pointclouds_gt"], pred * 0.9])
    want = {pp: rap_amd.compute_rigidity_rmse(d(cond), d(pred), R, t, ppp, cu, d(sc), pp).cpu() for pp in (False, True)}     # (tests/test_sample_gpu.py)
    want_mean, want_steps = (x.cpu() for x in rap_amd.selection.average_trajectory_rigidity_rmse(d(cond), d(traj), ppp, cu, d(sc), return_per_step=True))
    assert all(torch.isfinite(w).all() for w in want.values()) and torch.isfinite(want_steps).all()
    Rc, tc = R.cpu(), t.cpu()
    need = {0: lib.rap_rigidity_workspace_bytes(B * P, 0, B), steps: lib.rap_rigidity_workspace_bytes(B * P, steps, B)}

    def rmse(per_part):
        def call(c, short=0):
            out = c.out_view(F32, (B,), "out")
            ws = c.out(need[0], name="rigidity workspace")
            rc = lib.rap_rigidity_rmse(_lib.ptr(c.inp(cond)), _lib.ptr(c.inp(pred)), _lib.ptr(c.inp(Rc)), _lib.ptr(c.inp(tc)), _lib.ptr(c.inp(ppp)), B, P,
                                       _lib.ptr(c.inp(sc)), 1 if per_part else 0, _lib.ptr(out), P2(ws.ptr), need[0] - short, stream(dev))
            torch.cuda.synchronize()
            return rc, out

        def run(c):
            rc, out = call(c)
            assert rc == 0 and torch.equal(out.cpu(), want[per_part])
            return [out]
        return call, run

    def trajectory(own_per_step):
        def call(c, short=0):
            mean = c.out_view(F32, (B,), "mean_out")
            per_step = None if own_per_step else c.out_view(F32, (steps, B), "per_step_out")
            ws = c.out(need[steps], name="rigidity workspace")
            rc = lib.rap_trajectory_rigidity_rmse(_lib.ptr(c.inp(cond)), _lib.ptr(c.inp(traj)), _lib.ptr(c.inp(ppp)), B, P, TP, steps, _lib.ptr(c.inp(sc)),
                                                  _lib.ptr(mean), _lib.ptr(per_step), P2(ws.ptr), need[steps] - short, stream(dev))
            torch.cuda.synchronize()
            return rc, mean, per_step

        def run(c):
            rc, mean, per_step = call(c)
            assert rc == 0 and torch.equal(mean.cpu(), want_mean) and (own_per_step or torch.equal(per_step.cpu(), want_steps))
            return [mean] + ([] if own_per_step else [per_step])
        return call, run
    for call, run in (rmse(False), rmse(True), trajectory(False), trajectory(True)):
        run_both(dev, run)
        refused_call_wrote_nothing(dev, call)


# ---------------------------------------------------------------------------------------------
# rap_collate_transform
# ---------------------------------------------------------------------------------------------
def test_collate_transform_writes_only_its_outputs(lib, dev):
    g = torch.Generator().manual_seed(3)
    Fd = 8
    parts = [[torch.randn(n, 3, generator=g, dtype=torch.float64) * 4 + 100 for n in sizes if n] for sizes in TABLE]
    feats = [[torch.randn(p.shape[0], Fd, generator=g) for p in ps] for ps in parts]
    samples = [{"parts": ps, "features": fs} for ps, fs in zip(parts, feats)]
    np.random.seed(7)
    want = rap_amd.transform_and_collate(samples, 3, device=dev)                  # (held to the reference's golden in tests/test_kernels_gpu.py)
    np.random.seed(7)
    counts = np.array([[37, 100, 0], [2049, 1, 0]], dtype=np.int64)
    order = torch.from_numpy(rap_amd.data.draw_part_permutations(counts.reshape(-1))).to(I64)
    points = torch.cat([p for ps in parts for p in ps])
    feat_in = torch.cat([f for fs in feats for f in fs])
    B, P, TP = 2, 3, points.shape[0]
    need = lib.rap_collate_workspace_bytes(B, P)
    spec = [("pointclouds", F32, (TP, 3)), ("pointclouds_gt", F32, (TP, 3)), ("features", F32, (TP, Fd)), ("anchor_indices", U8, (TP,)),
            ("part_indices", I64, (TP,)), ("rotations", F32, (B, P, 3, 3)), ("translations", F32, (B, P, 3)), ("scales", F32, (B,)),
            ("anchor_parts", U8, (B, P)), ("global_translation", F32, (B, 3)), ("cu_seqlens", I64, (B + 1,))]

    def call(c, short=0):
        o = {name: c.out_view(dt, shape, name) for name, dt, shape in spec}
        flag = c.inp(torch.zeros(1, dtype=I32), "order_flag")
        ws = c.out(need, name="collate workspace")
        rc = lib.rap_collate_transform(_lib.ptr(c.inp(points)), 1, _lib.ptr(c.inp(torch.from_numpy(counts))), B, P, TP, _lib.ptr(c.inp(order)),
                                       _lib.ptr(c.inp(feat_in)), Fd, _lib.ptr(o["pointclouds"]), _lib.ptr(o["pointclouds_gt"]), _lib.ptr(o["features"]),
                                       _lib.ptr(o["anchor_indices"]), _lib.ptr(o["part_indices"]), _lib.ptr(o["rotations"]),
                                       _lib.ptr(o["translations"]), _lib.ptr(o["scales"]), _lib.ptr(o["anchor_parts"]),
                                       _lib.ptr(o["global_translation"]), _lib.ptr(o["cu_seqlens"]), _lib.ptr(flag), P2(ws.ptr), need - short,
                                       stream(dev))
        torch.cuda.synchronize()
        return rc, o, flag

    def run(c):
        rc, o, flag = call(c)
        assert rc == 0 and int(flag.cpu()) == 0
        for name, dt, _ in spec:
            w = want[name].to(dt) if want[name].dtype == torch.bool else want[name]
            assert torch.equal(o[name].cpu(), w.cpu()), name
        return list(o.values())
    run_both(dev, run)
    refused_call_wrote_nothing(dev, call)


# ---------------------------------------------------------------------------------------------
# preprocessing: outlier removal, voxel down-sampling and coverage, farthest point sampling, MiniSpinNet
# ---------------------------------------------------------------------------------------------
def test_statistical_outliers_with_inlier_indices_sized_exactly_n(lib, dev):
    N = 1025                                                    # one past the 1 024-point LDS tile
    pts = PC.outlier_cloud(N, 2).float()
    rc_ref, idx_ref, stats_ref = TPS.outliers_abi(dev, pts, 20, 2.0)      # (held to the fp64 oracle in tests/test_preproc_scale_gpu.py)
    assert rc_ref == 0 and 0 < idx_ref.numel() < N
    need = lib.rap_outlier_workspace_bytes(N)

    def call(c, short=0):
        idx, count, stats = c.out_view(I64, (N,), "inlier_indices"), c.out_view(I32, (1,), "count_out"), c.out_view(torch.float64, (3,), "stats_out")
        ws = c.out(need, name="outlier workspace")
        rc = lib.rap_statistical_outliers(_lib.ptr(c.inp(pts)), N, 20, 2.0, _lib.ptr(idx), _lib.ptr(count), _lib.ptr(stats), P2(ws.ptr), need - short,
                                          stream(dev))
        torch.cuda.synchronize()
        return rc, idx, count, stats

    def run(c):
        rc, idx, count, stats = call(c)
        n = int(count.cpu())
        assert rc == 0 and torch.equal(idx.cpu()[:n], idx_ref) and stats.cpu().tolist() == stats_ref
        assert bool((idx.cpu()[n:] == -1).all())                # nothing after the kept indices
        return [idx[:n], count, stats]
    run_both(dev, run)
    refused_call_wrote_nothing(dev, call)


def test_voxel_downsample_and_coverage_with_exact_outputs_and_workspaces(lib, dev):
    g = torch.Generator().manual_seed(6)
    N, vs = 3001, 0.1
    pts = (torch.rand(N, 3, generator=g) * torch.tensor([3.0, 2.0, 1.0]) - 0.7).float()
    want = torch.from_numpy(O.voxel_down_sample(pts.numpy(), vs))               # (tests/test_spinnet_gpu.py: bit-exact index lists)
    n_vox = int(np.unique(np.floor(pts.numpy() / np.float32(vs)), axis=0).shape[0])
    pd = pts.to(dev)
    bounds = torch.empty(6, dtype=I64, device=dev); dmax = torch.empty(1, dtype=F32, device=dev)
    _lib.check(lib.rap_voxel_bounds(_lib.ptr(pd), N, vs, _lib.ptr(bounds), _lib.ptr(dmax), stream(dev)), "rap_voxel_bounds")
    hb = bounds.cpu(); h_dmax = float(dmax.cpu())
    slots = lib.rap_voxel_table_slots(hb.data_ptr())
    assert slots > 0
    needs = {"dense": lib.rap_voxel_workspace_bytes(hb.data_ptr()), "sorted": lib.rap_voxel_sorted_workspace_bytes(N),
             "coverage": lib.rap_voxel_coverage_workspace_bytes(hb.data_ptr())}
    assert all(v > 0 for v in needs.values())

    def downsample(path):
        n_idx = min(N, slots) if path == "dense" else N
        fn = lib.rap_voxel_downsample if path == "dense" else lib.rap_voxel_downsample_sorted

        def call(c, short=0):
            idx, count = c.out_view(I64, (n_idx,), "indices_out"), c.out_view(I32, (1,), "count_out")
            ws = c.out(needs[path], name=f"voxel workspace ({path})")
            rc = fn(_lib.ptr(c.inp(pts)), N, vs, hb.data_ptr(), h_dmax, _lib.ptr(idx), _lib.ptr(count), P2(ws.ptr), needs[path] - short, stream(dev))
            torch.cuda.synchronize()
            return rc, idx, count

        def run(c):
            rc, idx, count = call(c)
            n = int(count.cpu())
            assert rc == 0 and n == want.numel() and torch.equal(idx.cpu()[:n], want), path
            assert bool((idx.cpu()[n:] == -1).all()), path
            return [idx[:n], count]
        return call, run

    def coverage(path):
        fn = lib.rap_voxel_coverage if path == "coverage" else lib.rap_voxel_coverage_sorted

        def call(c, short=0):
            count = c.out_view(I64, (1,), "count_out")
            ws = c.out(needs[path], name=f"voxel coverage workspace ({path})")
            rc = fn(_lib.ptr(c.inp(pts)), N, vs, hb.data_ptr(), _lib.ptr(count), P2(ws.ptr), needs[path] - short, stream(dev))
            torch.cuda.synchronize()
            return rc, count

        def run(c):
            rc, count = call(c)
            assert rc == 0 and int(count.cpu()) == n_vox, path
            return [count]
        return call, run
    for call, run in (downsample("dense"), downsample("sorted"), coverage("coverage"), coverage("sorted")):
        run_both(dev, run)
        refused_call_wrote_nothing(dev, call)


def test_farthest_point_sampling_with_exact_indices_and_distance_scratch(lib, dev):
    lengths = [0, 1, 63, 65, 1025]
    clouds = [PC.lattice_cloud(n, 20 + i, side=16).float() if n else torch.zeros(0, 3) for i, n in enumerate(lengths)]
    Ks, starts = [3, 4, 63, 70, 40], [0, 0, 5, 64, 1000]
    k_max, T = max(Ks), sum(lengths)
    pts = torch.cat(clouds)
    cloud_start = torch.tensor(np.concatenate([[0], np.cumsum(lengths)[:-1]]), dtype=I32)
    refs = [O.farthest_point_sampling(cl, n, K, st, device=dev) if n else torch.zeros(0, dtype=I64) for cl, n, K, st in zip(clouds, lengths, Ks, starts)]

    def run(c):
        idx = c.out_view(I32, (len(lengths), k_max), "indices_out")
        dist = c.out_view(F32, (T,), "dist_ws")                 # exactly T floats, as include/rapflow.h documents
        rc = lib.rap_farthest_point_sampling(_lib.ptr(c.inp(pts)), _lib.ptr(c.inp(cloud_start)), _lib.ptr(c.inp(torch.tensor(lengths, dtype=I32))),
                                             _lib.ptr(c.inp(torch.tensor(Ks, dtype=I32))), _lib.ptr(c.inp(torch.tensor(starts, dtype=I32))),
                                             len(lengths), k_max, _lib.ptr(idx), _lib.ptr(dist), stream(dev))
        torch.cuda.synchronize()
        assert rc == 0
        got = idx.cpu().long()
        for i, ref in enumerate(refs):                          # (tests/test_preproc_scale_gpu.py: equal to the sequential oracle, -1 padded)
            assert torch.equal(got[i, :ref.numel()], ref) and bool((got[i, ref.numel():] == -1).all()), i
        return [idx]
    run_both(dev, run)


def test_spinnet_describe_5_keypoints_in_chunks_of_4_with_the_exact_workspace(lib, dev):
    sd, net = TPS.make_net(1, dev, chunk=4)
    g = torch.Generator().manual_seed(2)
    pts = torch.rand(3000, 3, generator=g)
    kpts = pts[torch.randperm(3000, generator=g)[:5]].contiguous()
    need = lib.rap_spinnet_workspace_bytes(4)
    rc, want = TPS.describe(net, pts.to(dev), None, kpts.to(dev), 0.25, 0, 4)
    assert rc == 0 and torch.isfinite(want).all() and (want.norm(dim=1) - 1).abs().max().item() < 1e-5

    def call(c, short=0):
        desc = c.out_view(F32, (5, 32), "desc_out")
        ws = c.out(need, pitch=1152 * 4, name="spinnet workspace")
        rc = TPS.describe(net, c.inp(pts), None, c.inp(kpts), 0.25, 0, 4, ws=ws.view(U8, (need,)), ws_bytes=need - short, desc=desc)[0]
        return rc, desc

    def run(c):
        rc, desc = call(c)
        assert rc == 0 and torch.equal(desc.cpu(), want.cpu())
        return [desc]
    run_both(dev, run)
    refused_call_wrote_nothing(dev, call)


# ---------------------------------------------------------------------------------------------
# rap_select_generation
# ---------------------------------------------------------------------------------------------
def test_select_generation_gathers_write_only_their_outputs(lib, dev):
    g = torch.Generator().manual_seed(12)
    G_, B, P = 3, 3, 2
    cu = torch.tensor([0, 1, 256, 513], dtype=I32)              # sample lengths 1, 255, 257
    TP = 513
    rmse = torch.rand(G_, B, generator=g)
    clouds, R, t = torch.randn(G_, TP, 3, generator=g), torch.randn(G_, B, P, 3, 3, generator=g), torch.randn(G_, B, P, 3, generator=g)
    best_ref = rmse.argmin(0)
    tok = torch.repeat_interleave(torch.arange(B), (cu[1:] - cu[:-1]).long())

    def run(c):
        best, cloud = c.out_view(I32, (B,), "best_out"), c.out_view(F32, (TP, 3), "cloud_out")
        Ro, to = c.out_view(F32, (B, P, 3, 3), "R_out"), c.out_view(F32, (B, P, 3), "t_out")
        rc = lib.rap_select_generation(_lib.ptr(c.inp(rmse)), G_, B, P, TP, _lib.ptr(c.inp(cu)), _lib.ptr(c.inp(clouds)), _lib.ptr(c.inp(R)),
                                       _lib.ptr(c.inp(t)), 0, _lib.ptr(best), _lib.ptr(cloud), _lib.ptr(Ro), _lib.ptr(to), stream(dev))
        torch.cuda.synchronize()
        assert rc == 0 and torch.equal(best.cpu().long(), best_ref)
        assert torch.equal(cloud.cpu(), clouds[best_ref[tok], torch.arange(TP)])
        assert torch.equal(Ro.cpu(), R[best_ref, torch.arange(B)]) and torch.equal(to.cpu(), t[best_ref, torch.arange(B)])
        return [best, cloud, Ro, to]
    run_both(dev, run)


# ---------------------------------------------------------------------------------------------
# nearest-neighbour metrics at segment lengths {1, 255, 257}
# ---------------------------------------------------------------------------------------------
def nn_clouds(n, seed):
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(n, 3, generator=g)
    return gt, gt + 0.02 * torch.randn(n, 3, generator=g)


def test_chamfer_rmse_stays_inside_its_exact_workspace(lib, dev):
    cu = torch.tensor([0, 1, 256, 513], dtype=I32)
    B, TP = 3, 513
    gt, pred = nn_clouds(TP, 21)
    ref = O.compute_cd(gt, pred, cu.long())
    need = lib.rap_nn_metrics_workspace_bytes(TP, B)

    def call(c, short=0):
        out = c.out_view(F32, (B,), "out")
        ws = c.out(need, name="nn workspace")
        rc = lib.rap_chamfer_rmse(_lib.ptr(c.inp(gt)), _lib.ptr(c.inp(pred)), _lib.ptr(c.inp(cu)), B, TP, _lib.ptr(out), P2(ws.ptr), need - short,
                                  stream(dev))
        torch.cuda.synchronize()
        return rc, out

    def run(c):
        rc, out = call(c)
        assert rc == 0 and (out.cpu().double() - ref.double()).abs().max().item() < 2e-6          # (tests/test_sample_gpu.py)
        return [out]
    run_both(dev, run)
    refused_call_wrote_nothing(dev, call)


@pytest.mark.parametrize("ns,nt", [(1, 257), (255, 1), (257, 255)])
def test_correspondence_rmse_stays_inside_its_exact_workspace(lib, dev, ns, nt):
    sg, sp = nn_clouds(ns, 31)
    tg = torch.cat([sg[: min(ns, nt)] + 0.01, torch.rand(max(0, nt - ns), 3, generator=torch.Generator().manual_seed(5))])[:nt].contiguous()
    tp = tg + 0.02 * torch.randn(nt, 3, generator=torch.Generator().manual_seed(6))
    thr = 0.05
    o_rmse, o_n, o_ratio, _ = O.compute_correspondence_rmse(sg, tg, sp, tp, thr)
    assert o_n > 0
    need = lib.rap_nn_metrics_workspace_bytes(ns, 1)

    def call(c, short=0):
        out = c.out_view(F32, (3,), "out3")
        ws = c.out(need, name="nn workspace")
        rc = lib.rap_correspondence_rmse(_lib.ptr(c.inp(sg)), _lib.ptr(c.inp(tg)), _lib.ptr(c.inp(sp)), _lib.ptr(c.inp(tp)), ns, nt, thr,
                                         _lib.ptr(out), P2(ws.ptr), need - short, stream(dev))
        torch.cuda.synchronize()
        return rc, out

    def run(c):
        rc, out = call(c)
        rmse, n, ratio = out.cpu().tolist()
        assert rc == 0 and int(n) == o_n and abs(rmse - float(o_rmse)) < 2e-6 * float(o_rmse) + 1e-7           # (tests/test_sample_gpu.py)
        assert abs(ratio - o_n / ns) < 1e-6
        return [out]
    run_both(dev, run)
    refused_call_wrote_nothing(dev, call)


def test_overlap_ratio_stays_inside_its_exact_workspace(lib, dev):
    ppp = torch.tensor([[1, 255], [255, 257], [257, 1]], dtype=I64)
    cu = torch.tensor([0, 256, 768, 1026], dtype=I32)
    B, P, TP = 3, 2, 1026
    pred = nn_clouds(TP, 41)[0] * 0.5
    taus = [0.02, 0.05]
    ref_ratios, ref_min = O.compute_overlap_ratio(pred, ppp, cu.long(), taus)
    h_taus = (ctypes.c_float * 2)(*taus)
    need = lib.rap_overlap_workspace_bytes(TP, B, P)
    n = (cu[1:] - cu[:-1]).double()

    def call(c, short=0, with_min=True):
        ratios = c.out_view(F32, (2, B), "ratios_out")
        min_d = c.out_view(F32, (TP,), "min_dist_out") if with_min else None
        ws = c.out(need, name="overlap workspace")
        rc = lib.rap_overlap_ratio(_lib.ptr(c.inp(pred)), _lib.ptr(c.inp(ppp)), _lib.ptr(c.inp(cu)), B, P, TP, ctypes.cast(h_taus, P2), 2,
                                   _lib.ptr(ratios), _lib.ptr(min_d), P2(ws.ptr), need - short, stream(dev))
        torch.cuda.synchronize()
        return rc, ratios, min_d

    def run_with(with_min):
        def run(c):
            rc, ratios, min_d = call(c, with_min=with_min)
            assert rc == 0
            assert ((ratios.cpu().double() - ref_ratios).abs() * n[None, :]).max().item() <= 1.0 + 1e-6        # (tests/test_sample_gpu.py)
            if with_min:
                assert (min_d.cpu().double() - ref_min).abs().max().item() < 1e-6
            return [ratios] + ([min_d] if with_min else [])
        return run
    run_both(dev, run_with(True))
    run_both(dev, run_with(False))                              # min_dist_out = NULL: the distances go to the workspace
    refused_call_wrote_nothing(dev, call)


def test_pair_metrics_stays_inside_its_exact_workspace(lib, dev):
    ppp = torch.tensor([[1, 255], [255, 257], [257, 1]], dtype=I64)
    cu = torch.tensor([0, 256, 768, 1026], dtype=I32)
    B, TP, thr = 3, 1026, 0.05
    gt, cloud = nn_clouds(TP, 51)
    for b in range(B):                                         # target = source shifted a little, so that every pair has correspondences
        a, n0, n1 = int(cu[b]), int(ppp[b, 0]), int(ppp[b, 1])
        m = min(n0, n1)
        gt[a + n0:a + n0 + m] = gt[a:a + m] + 0.01
    scales = torch.tensor([0.8, 1.0, 1.2])
    g = torch.Generator().manual_seed(8)
    Rg = torch.stack([S._random_rotation(g).float() for _ in range(B * 2)]).reshape(B, 2, 3, 3).contiguous()
    tg = torch.randn(B, 2, 3, generator=g) * 0.1
    Rp = torch.stack([S._random_rotation(g).float() for _ in range(B * 2)]).reshape(B, 2, 3, 3).contiguous()
    tp = torch.randn(B, 2, 3, generator=g) * 0.1
    need = lib.rap_pair_metrics_workspace_bytes(TP, B)
    d = {"pointclouds_gt": gt.to(dev), "points_per_part": ppp.to(dev), "cu_seqlens_batch": cu.to(dev), "scales": scales.to(dev),
         "rotations": Rg.to(dev), "translations": tg.to(dev)}
    want_t = metrics.compute_pair_metrics(d, cloud.to(dev), Rp.to(dev), tp.to(dev), thr).cpu()       # (held to the reference's record in tests/test_evaluator_gpu.py)

    def call(c, short=0, transformed=False):
        out = c.out_view(F32, (B, 4), "out4")
        ws = c.out(need, name="pair-metrics workspace")
        rc = lib.rap_pair_metrics(_lib.ptr(c.inp(gt)), _lib.ptr(c.inp(cloud)), _lib.ptr(c.inp(ppp)), _lib.ptr(c.inp(cu)), _lib.ptr(c.inp(scales)),
                                  _lib.ptr(c.inp(Rg)), _lib.ptr(c.inp(tg)), _lib.ptr(c.inp(Rp) if transformed else None),
                                  _lib.ptr(c.inp(tp) if transformed else None), B, TP, thr, _lib.ptr(out), P2(ws.ptr), need - short, stream(dev))
        torch.cuda.synchronize()
        return rc, out

    def run_direct(c):
        rc, out = call(c)
        assert rc == 0
        got = out.cpu()
        for b in range(B):                                     # the fp64 oracle on the scaled parts (tests/test_evaluator_gpu.py, tests/test_sample_gpu.py)
            a, n0, n1 = int(cu[b]), int(ppp[b, 0]), int(ppp[b, 1])
            s = float(scales[b])
            sl0, sl1 = slice(a, a + n0), slice(a + n0, a + n0 + n1)
            o_rmse, o_n, _, _ = O.compute_correspondence_rmse(gt[sl0] * s, gt[sl1] * s, cloud[sl0] * s, cloud[sl1] * s, thr)
            assert o_n > 0 and int(got[b, 3]) == o_n and abs(float(got[b, 0]) - float(o_rmse)) < 2e-6 * float(o_rmse) + 1e-7, b
            assert torch.isinf(got[b, 2])
        return [out]

    def run_transformed(c):
        rc, out = call(c, transformed=True)
        assert rc == 0 and torch.equal(out.cpu(), want_t)
        return [out]
    run_both(dev, run_direct)
    run_both(dev, run_transformed)
    refused_call_wrote_nothing(dev, call)
