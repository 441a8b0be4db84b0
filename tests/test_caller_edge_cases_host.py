"""CPU: the inputs of tests/caller_edge_cases.py are what the GPU edge tests take them for -- the part sizes reach every chunk count and
batch count of the Procrustes moments kernel, every threshold keeps its margin from every distance of the float64 oracle, the lattice
distances are exact in fp32, the voxel tables have the slot counts the cases are named for -- and the oracles those tests compare with
agree with a direct numpy / torch restatement on two small cases each."""
import ctypes

import numpy as np
import pytest
import torch

import caller_edge_cases as C
from oracle import rap_oracle as O


# ---------------------------------------------------------------------------------------------
# Procrustes / rigidity inputs
# ---------------------------------------------------------------------------------------------
def test_sweep_sizes_reach_every_chunk_count_and_batch_count():
    sizes = C.SWEEP_SIZES
    assert sizes[:len(C.SIZES_NAMED)] == [1, 2, 3, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 32767, 32768, 32769, 40000,
                                          65537, 70001]
    assert C.proc_chunks_of(0) == 1 and C.proc_chunks_of(2048) == 1 and C.proc_chunks_of(2049) == 2 and C.proc_chunks_of(10 ** 6) == 16
    by_count = {}
    for n in sizes:
        by_count.setdefault(C.proc_chunks_of(n), []).append(n)
    assert sorted(by_count) == list(range(1, 17))
    for nc, ns in by_count.items():
        assert any(n % nc == 0 for n in ns), nc                           # an exact split: every chunk the same length
        if nc > 1:                                                         # (one chunk always is the whole part)
            assert any(n % nc != 0 for n in ns), nc                        # an inexact one: chunk lengths differ by one
    for n in sizes:
        L = C.chunk_lengths(n)
        assert sum(L) == n and min(L) >= 1 and max(L) - min(L) <= 1
    # batches of 2048 a chunk is walked in, and whether the last one has a weighted tail
    seen = {(-(-l // C.PROC_BATCH), l % C.PROC_BATCH != 0) for n in sizes for l in C.chunk_lengths(n)}
    assert {(1, True), (1, False), (2, True), (2, False), (3, True)} <= seen, seen
    assert max(b for b, _ in seen) == 3
    assert max(sizes) > 16 * 2048                                          # past what the suite has run so far


def test_sweep_layout_interleaves_empty_parts():
    s = C.procrustes_sweep()
    ppp = s["ppp"]
    assert ppp.shape[1] == 8 and sorted(int(n) for n in ppp.reshape(-1) if n > 0) == sorted(C.SWEEP_SIZES)
    assert ppp[0, 0] == 0 and (ppp[0, 1:] > 0).all()                       # leading
    assert ppp[1, 3] == 0 and (ppp[1, :3] > 0).all() and (ppp[1, 4:] > 0).all()      # in the middle
    assert (ppp[2] == 0).all()                                             # a sample without points
    assert ppp[3, 7] == 0 and (ppp[3, :7] > 0).all()                       # trailing
    assert int(s["off"][-1]) == s["src"].shape[0] == sum(C.SWEEP_SIZES) and s["traj"].shape == (3, s["src"].shape[0], 3)
    assert torch.equal(s["cu"], s["off"][::8]) and s["cu"][2] == s["cu"][3]
    # the compaction helpers: the same points in the same order, columns mapped back
    cp, where = C.compacted(ppp)
    assert torch.equal(cp.sum(1), ppp.sum(1)) and cp[0].tolist() == ppp[0, 1:].tolist() + [0] and where[0].tolist() == [1, 2, 3, 4, 5, 6, 7, -1]
    assert where[1].tolist() == [0, 1, 2, 4, 5, 6, 7, -1] and (where[2] == -1).all()
    x = torch.arange(ppp.numel(), dtype=torch.float64).reshape(ppp.shape) * (ppp > 0)
    assert torch.equal(C.uncompact(C.compact_like(x, where), where), x)
    # every part is a noisy rigid image: residual of the best fit ~ noise 0.05 per coordinate
    a, e = int(s["off"][8 * 3 + 6]), int(s["off"][8 * 3 + 7])                  # the 70001-point part
    R, t = O.solve_procrustes(s["src"][a:e].double(), s["tgt"][a:e].double())
    res = (s["src"][a:e].double() @ R.T + t - s["tgt"][a:e].double()).pow(2).mean().sqrt()
    assert abs(float(torch.det(R)) - 1) < 1e-12 and 0.045 < float(res) < 0.055


def test_degenerate_and_far_parts_are_what_they_are_named():
    d = C.degenerate_parts()
    kinds = {k for k, _ in d["cases"]}
    assert kinds == set(C.DEGENERATE_UNIQUE) | set(C.DEGENERATE_FREE)
    assert {n for k, n in d["cases"] if k in C.DEGENERATE_UNIQUE} == {3, 300, 2049}
    for k, (kind, n) in enumerate(d["cases"]):
        a, e = int(d["off"][k]), int(d["off"][k + 1])
        assert e - a == n
        s, t = d["src"][a:e].double(), d["tgt"][a:e].double()
        sv = torch.linalg.svdvals(s - s.mean(0))
        H = (s - s.mean(0)).T @ (t - t.mean(0))
        if kind == "planar":
            assert sv[2] < 1e-6 * sv[0] and sv[1] > 1e-2 * sv[0]
        if kind in ("collinear", "two_points"):
            assert sv[1] < 1e-6 * sv[0] and sv[0] > 0
        if kind == "coincident":
            assert sv[0] == 0 and float(H.abs().max()) < 1e-12
        if kind == "reflection" and n > 3:                               # the unconstrained optimum is improper: the determinant rule decides
            U, _, Vt = torch.linalg.svd(H)
            assert torch.det(Vt.T @ U.T) < 0
    f = C.far_parts()
    assert f["ppp"].shape == (2, 4) and C.FAR_FRAMES == ("origin", "centre")
    for j, frame in enumerate(C.FAR_FRAMES):
        for k, (offset, spread, n) in enumerate(C.FAR_CASES):
            a, e = int(f["off"][4 * j + k]), int(f["off"][4 * j + k + 1])
            s = f["src"][a:e].double()
            assert e - a == n and abs(float(s.mean(0)[0]) - offset) < 0.5 and float((s.std(0) - spread).abs().max()) < 0.2
            _, t = O.solve_procrustes(s, f["tgt"][a:e].double())
            print(f"far part, rotated about the {frame}: offset {offset:g} n {n}: largest |t| of the oracle {float(t.abs().max()):.1f}")
            assert float(t.abs().max()) < 0.01 * offset if frame == "origin" else float(t.abs().max()) > 0.3 * offset
    assert {(o, s) for o, s, _ in C.FAR_CASES} == {(300.0, 5.0), (1000.0, 5.0)} and {n for _, _, n in C.FAR_CASES} == {4097, 70001}


# ---------------------------------------------------------------------------------------------
# nearest-neighbour inputs
# ---------------------------------------------------------------------------------------------
def test_overlap_batch_margins_and_tail_slots():
    o = C.overlap_batch()
    ppp, cu, pts = o["ppp"], o["cu"], o["pts"]
    assert ppp.shape[1] == 3
    totals = ppp.sum(1).tolist()
    for N in C.NN_SIZES:
        for sp in C.overlap_splits(N):
            assert list(sp) in ppp.tolist(), sp
    assert [300, 0, 0] in ppp.tolist() and totals.count(1) >= 4          # one non-empty part; single points
    ratios, min_d = O.compute_overlap_ratio(pts, ppp, cu, o["taus"])
    fin = torch.isfinite(min_d)
    for tau in o["taus"]:
        m = float((min_d[fin] - tau).abs().min())
        print(f"tau {tau:.6f}: nearest distance of the oracle is {m:.2e} away, {int((min_d[fin] <= tau).sum())} of {int(fin.sum())} inside")
        assert m > C.MARGIN, (tau, m)
    assert 0.01 < float((min_d[fin] <= o["taus"][0]).double().mean()) and float((min_d[fin] <= o["taus"][2]).double().mean()) < 0.97
    # the tail-slot samples: N = 257 / 513 (one candidate in the last tile), the query's nearest other-part point is the sample's last /
    # first point at 0.02, and every other point of another part is far
    assert sorted((totals[b], w) for b, _, w in o["tail"]) == [(257, "first"), (257, "last"), (513, "first"), (513, "last")]
    for b, q, which in o["tail"]:
        a, e = int(cu[b]), int(cu[b + 1])
        assert (e - a) % C.NN_TILE == 1
        other = e - 1 if which == "last" else a
        pid = torch.repeat_interleave(torch.arange(3), ppp[b])
        d = (pts[a:e].double() - pts[q].double()).norm(dim=1)
        d[pid == pid[q - a]] = float("inf")
        assert int(d.argmin()) == other - a and abs(float(d.min()) - 0.02) < 1e-5 and float(min_d[q]) == float(d.min())
        d[other - a] = float("inf")
        assert float(d.min()) > 10.0


def test_lattices_are_exact_in_fp32():
    assert np.float32(C.F32_BELOW_QUARTER) == np.nextafter(np.float32(0.25), np.float32(0)) and C.F32_BELOW_QUARTER < 0.25
    assert float(np.float32(C.F32_BELOW_QUARTER)) == C.F32_BELOW_QUARTER
    L = C.overlap_lattice()
    p = L["pts"].numpy()
    n0 = int(L["ppp"][0, 0])
    assert p.shape[0] == 280 and p.shape[0] % C.NN_TILE != 0 and L["ppp"].tolist() == [[140, 140]]
    assert ((p[:n0, 0] / 0.25) % 2 == 0).all() and ((p[n0:, 0] / 0.25) % 2 == 1).all()
    for dt in (np.float32, np.float64):
        q = p.astype(dt)
        d = q[:, None, :] - q[None, :, :]
        D = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        other = np.arange(280)[:, None] < n0
        D[other == other.T] = np.inf
        assert (np.sqrt(D.min(axis=1)) == dt(0.25)).all() and D.dtype == dt
    _, min_d = O.compute_overlap_ratio(L["pts"], L["ppp"], L["cu"], L["taus"])
    assert (min_d == 0.25).all()
    K = C.correspondence_lattice()
    for dt in (np.float32, np.float64):
        s, t = K["sg"].numpy().astype(dt), K["tg"].numpy().astype(dt)
        d = s[:, None, :] - t[None, :, :]
        D = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        assert (np.sqrt(D.min(axis=1)) == dt(0.25)).all()
    rmse, n, ratio, _ = O.compute_correspondence_rmse(K["sg"], K["tg"], K["sp"], K["tp"], 0.25)
    assert n == K["sg"].shape[0] == 294 and ratio == 1.0
    assert O.compute_correspondence_rmse(K["sg"], K["tg"], K["sp"], K["tp"], C.F32_BELOW_QUARTER)[1] == 0


def test_correspondence_margins_and_ties():
    pairs = C.correspondence_pairs()
    assert [(p["sg"].shape[0], p["tg"].shape[0]) for p in pairs] == [(1, 1), (1, 300), (300, 1), (255, 257), (256, 256), (257, 255), (513, 1000)]
    for p in pairs:
        d = torch.cdist(p["sg"].double(), p["tg"].double()).min(dim=1).values
        m = float((d - p["thr"]).abs().min())
        n = O.compute_correspondence_rmse(p["sg"], p["tg"], p["sp"], p["tp"], p["thr"])[1]
        print(f"{tuple(p['sg'].shape)} x {tuple(p['tg'].shape)}: thr {p['thr']:.6f}, margin {m:.2e}, {n} correspondences")
        assert m > C.MARGIN and n >= 1 and (p["sg"].shape[0] == 1 or 0.2 < n / p["sg"].shape[0] < 0.8)
        assert p["sp"].shape == p["sg"].shape and p["tp"].shape == p["tg"].shape
    T = C.correspondence_ties()
    s, t = T["sg"].numpy().astype(np.float64), T["tg"].numpy().astype(np.float64)
    D = np.sqrt(((s[:, None, :] - t[None, :, :]) ** 2).sum(-1))
    rows = np.arange(len(s))
    assert (T["first"] < 300).all() and (T["last"] >= 300).all()
    assert (D.argmin(axis=1) == T["first"]).all()                         # numpy's argmin: the first minimum
    assert (D[rows, T["first"]] == D[rows, T["last"]]).all() and (t[T["first"]] == t[T["last"]]).all()
    rest = D.copy(); rest[rows, T["first"]] = np.inf; rest[rows, T["last"]] = np.inf
    assert (rest.min(axis=1) - D.min(axis=1) > 1e-3).all()               # no third candidate near: fp32 cannot change the nearest POINT
    assert (np.abs(D.min(axis=1) - T["thr"]) > 0.03).all() and (D.min(axis=1) < T["thr"]).all()
    assert len({j // C.NN_TILE for j in T["first"]}) == 2 and len({j // C.NN_TILE for j in T["last"]}) == 2      # both copies span tiles
    tp = T["tp"].numpy().astype(np.float64)
    sp = T["sp"].numpy().astype(np.float64)
    r_first = np.sqrt(((sp - tp[T["first"]]) ** 2).sum(1).mean())
    r_last = np.sqrt(((sp - tp[T["last"]]) ** 2).sum(1).mean())
    assert abs(r_first - r_last) > 1e-3 * r_first                         # the rule is visible in the result
    data, cloud, thr = C.pair_batch()
    assert data["points_per_part"].tolist() == [list(x) for x in C.CORR_PAIRS] and cloud.shape == data["pointclouds_gt"].shape
    assert int(data["cu_seqlens_batch"][-1]) == cloud.shape[0] and thr == 0.25


def test_large_pair_has_more_than_64_items_and_keeps_the_threshold_margin():
    data, cloud, thr, pairs = C.large_pair_batch()
    assert data["points_per_part"].tolist() == [list(x) for x in C.LARGE_PAIRS] and cloud.shape == data["pointclouds_gt"].shape
    assert -(-C.LARGE_PAIRS[0][0] // C.NN_TILE) > 64 and int(data["cu_seqlens_batch"][-1]) == cloud.shape[0] and thr == 0.25
    for p in pairs:
        d = torch.cdist(p["sg"].double(), p["tg"].double()).min(dim=1).values
        m = float((d - p["thr"]).abs().min())
        n = O.compute_correspondence_rmse(p["sg"], p["tg"], p["sp"], p["tp"], p["thr"])[1]
        print(f"{tuple(p['sg'].shape)} x {tuple(p['tg'].shape)}: thr {p['thr']:.6f}, margin {m:.2e}, {n} correspondences")
        assert m > C.MARGIN and 0.2 < n / p["sg"].shape[0] < 0.8
        counted = (d <= p["thr"]).numpy()                                  # sources of both kinds in the first AND in the last item
        assert 0 < counted[:C.NN_TILE].sum() < C.NN_TILE and 0 < counted[-(len(d) % C.NN_TILE or C.NN_TILE):].sum()


def test_chamfer_batch_is_the_size_sweep():
    c = C.chamfer_batch()
    assert (c["cu"][1:] - c["cu"][:-1]).tolist() == C.NN_SIZES == [1, 2, 255, 256, 257, 511, 512, 513, 769]
    assert c["gt"].shape == c["pred"].shape == (sum(C.NN_SIZES), 3) and not torch.equal(c["gt"], c["pred"])


# ---------------------------------------------------------------------------------------------
# voxel inputs
# ---------------------------------------------------------------------------------------------
def test_voxel_cases_have_the_grids_they_are_named_for():
    from rap_amd import _lib
    lib = _lib.load()
    cases = C.voxel_cases()

    def slots(p, vs):                                                     # the entry point's own table size (host arithmetic)
        g = np.floor(p / np.float32(vs)).astype(np.int64)
        b = np.ascontiguousarray(np.concatenate([g.min(axis=0), g.max(axis=0)]), dtype=np.int64)
        return lib.rap_voxel_table_slots(ctypes.c_void_p(b.ctypes.data))

    for name, (p, vs) in cases.items():
        assert p.dtype == np.float32 and p.flags.c_contiguous and p.shape[1] == 3, name
        assert slots(p, vs) == C.voxel_slots(C.grid_extent(p, vs)), name
    assert [C.grid_extent(*cases[k]) for k in ("one_voxel_n1", "one_voxel_n50", "v1_block")] == [0, 0, 1]
    assert cases["one_voxel_n1"][0].shape[0] == 1 and cases["one_voxel_n50"][0].shape[0] == 50 and cases["v1_block"][0].shape[0] == 200
    assert O.calculate_voxel_coverage(cases["v1_block"][0], 0.25) == 8    # all eight cells, which the cubic key folds onto four
    assert len(O.voxel_down_sample(cases["v1_block"][0], 0.25)) == 4
    # table edge: one compaction block, and a second, partial one; the first and the last slot are occupied
    for v, want, blocks in ((15, 3616, 1), (16, 4369, 2)):
        p, vs = cases[f"table_v{v}"]
        assert C.grid_extent(p, vs) == v and slots(p, vs) == want == C.voxel_slots(v) and -(-want // C.VX_CHUNK) == blocks
        g = np.floor(p / np.float32(vs)).astype(np.int64)
        assert (g.min(axis=0) == 0).all() and (g == 0).all(axis=1).any() and (g == v).all(axis=1).any()
        key = g[:, 0] + g[:, 1] * v + g[:, 2] * v * v
        assert key.min() == 0 and key.max() == want - 1
    # all centres: every distance is 0 in the oracle's fp32 arithmetic; every voxel holds two points or more
    p, vs = cases["all_centres_twice"]
    grid = np.floor(p / np.float32(vs))
    assert (p - (grid + np.float32(0.5)) * np.float32(vs) == 0).all() and p.shape[0] == 150 and (p[:75] == p[75:][::-1]).all()
    with np.errstate(invalid="ignore"):
        idx = O.voxel_down_sample(p, vs)
    assert (idx < 75).all()                                               # the lowest index of every voxel is in the first copy
    # faces and signs: every multiple of 0.25 in [-2, 2], -0.0, and one fp32 step either side of seven faces
    p, vs = cases["faces_and_signs"]
    vals = np.unique(p)
    ks = (np.arange(-8, 9) * 0.25).astype(np.float32)
    assert np.isin(ks, vals).all() and (np.signbit(p) & (p == 0)).any() and (~np.signbit(p) & (p == 0)).any()
    off_face = vals[~np.isin(vals, ks)]
    assert len(off_face) == 14
    for x in off_face:
        k = ks[np.abs(ks - x).argmin()]
        assert x in (np.nextafter(k, np.float32(np.inf)), np.nextafter(k, np.float32(-np.inf)))
        assert np.floor(x / np.float32(vs)) == (k / 0.25 if x > k else k / 0.25 - 1)      # either side of the face
    for a in range(3):
        assert np.isin(vals, p[:, a]).all()
    for n in (255, 256, 257):
        assert cases[f"n{n}"][0].shape[0] == n
    p, vs = cases["crowded"]
    same = (p == p[250]).all(axis=1)
    assert same.sum() == 10000 and same[250:10250].all() and p.shape[0] == 10500
    assert 250 in O.voxel_down_sample(p, vs)                              # the run's lowest index wins its voxel


# ---------------------------------------------------------------------------------------------
# the oracles the GPU edge tests compare with, against direct restatements (two small cases each)
# ---------------------------------------------------------------------------------------------
def _kabsch_np(s, t):
    s, t = np.asarray(s, dtype=np.float64), np.asarray(t, dtype=np.float64)
    ms, mt = s.mean(0), t.mean(0)
    U, _, Vt = np.linalg.svd((s - ms).T @ (t - mt))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    return R, mt - R @ ms


def _small_batches():
    g = torch.Generator().manual_seed(55)
    out = []
    for rows in ([[5, 9, 0], [12, 4, 7]], [[40, 0, 0], [0, 0, 0], [3, 30, 11]]):
        ppp = torch.tensor(rows, dtype=torch.int64)
        off, cu = C.offsets_of(ppp)
        src = torch.randn(int(off[-1]), 3, generator=g, dtype=torch.float64)
        tgt = torch.cat([C.noisy_rigid_image(src[int(a):int(e)].float(), g, 0.05).double() for a, e in zip(off[:-1], off[1:])])
        out.append((src, tgt, ppp, cu, off))
    return out


def test_procrustes_and_rigidity_oracles_agree_with_a_direct_restatement():
    for src, tgt, ppp, cu, off in _small_batches():
        B, P = ppp.shape
        R, t = O.fit_transformations(src, tgt, ppp, cu)
        rig = O.rigidify_prediction_with_procrustes(tgt, src, ppp, cu)
        sc = torch.linspace(0.5, 2.0, B, dtype=torch.float64)
        traj = torch.stack([tgt, tgt * 1.01, tgt + 0.1])
        want_rig = np.zeros(src.shape)
        per_step = np.zeros((3, B))
        for b in range(B):
            sq_all, rm = [], []
            for p in range(P):
                a, e = int(off[b * P + p]), int(off[b * P + p + 1])
                if e == a:
                    assert float(R[b, p].abs().max()) == 0 and float(t[b, p].abs().max()) == 0
                    continue
                Rn, tn = _kabsch_np(src[a:e], tgt[a:e])
                assert np.abs(R[b, p].numpy() - Rn).max() < 1e-12 and np.abs(t[b, p].numpy() - tn).max() < 1e-12
                Rs, ts = O.solve_procrustes(src[a:e], tgt[a:e])
                assert torch.equal(Rs, R[b, p]) and torch.equal(ts, t[b, p])
                want_rig[a:e] = src[a:e].numpy() @ Rn.T + tn
                sq = ((want_rig[a:e] - tgt[a:e].numpy()) ** 2).sum(1)
                sq_all.append(sq); rm.append(np.sqrt(sq.mean()))
            want = (np.inf, np.inf) if not rm else (np.sqrt(np.concatenate(sq_all).mean()), np.mean(rm))
            for per_part in (False, True):
                for scales in (None, sc):
                    got = float(O.compute_rigidity_rmse(src, tgt, R, t, ppp, cu, scales, per_part)[b])
                    w = want[per_part] * (1.0 if scales is None else float(sc[b]))
                    assert got == w or abs(got - w) < 1e-12 * w, (b, per_part, got, w)
            for s in range(3):
                sq = []
                for p in range(P):
                    a, e = int(off[b * P + p]), int(off[b * P + p + 1])
                    if e > a:
                        Rn, tn = _kabsch_np(src[a:e], traj[s, a:e])
                        sq.append(((src[a:e].numpy() @ Rn.T + tn - traj[s, a:e].numpy()) ** 2).sum(1))
                per_step[s, b] = np.sqrt(np.concatenate(sq).mean()) * float(sc[b]) if sq else np.inf
        assert np.abs(rig.numpy() - want_rig).max() < 1e-12
        mean, steps = O.average_trajectory_rigidity_rmse(src, traj, ppp, cu, sc)
        fin = np.isfinite(per_step)
        assert np.array_equal(np.isinf(steps.numpy()), ~fin) and np.abs(steps.numpy()[fin] - per_step[fin]).max() < 1e-12
        assert np.abs(mean.numpy()[fin[0]] - per_step.mean(0)[fin[0]]).max() < 1e-12


def test_nn_oracles_agree_with_a_direct_restatement():
    g = torch.Generator().manual_seed(56)
    # overlap ratio: per point, a loop over the sample's points of the other parts
    for rows in ([[4, 6, 0], [1, 0, 0], [3, 3, 3]], [[0, 7, 9], [5, 0, 0]]):
        ppp = torch.tensor(rows, dtype=torch.int64)
        off, cu = C.offsets_of(ppp)
        pts = torch.rand(int(off[-1]), 3, generator=g)
        taus = (0.2, 0.4)
        ratios, min_d = O.compute_overlap_ratio(pts, ppp, cu, taus)
        p64 = pts.numpy().astype(np.float64)
        pid = np.concatenate([np.repeat(np.arange(3), r) for r in rows])
        smp = np.concatenate([np.full(sum(r), b) for b, r in enumerate(rows)])
        want = np.full(len(p64), np.inf)
        for i in range(len(p64)):
            for j in range(len(p64)):
                if smp[i] == smp[j] and pid[i] != pid[j]:
                    want[i] = min(want[i], np.sqrt(((p64[i] - p64[j]) ** 2).sum()))
        assert np.array_equal(np.isinf(want), np.isinf(min_d.numpy())) and np.abs(want[np.isfinite(want)] - min_d.numpy()[np.isfinite(want)]).max() < 1e-12
        for ti, tau in enumerate(taus):
            for b, r in enumerate(rows):
                w = (want[smp == b] <= tau).mean() if sum(x > 0 for x in r) > 1 else 0.0
                assert abs(float(ratios[ti, b]) - w) < 1e-12
    # chamfer and correspondence RMSE
    for ns, nt in ((7, 11), (1, 5)):
        a, b = torch.rand(ns, 3, generator=g), torch.rand(nt, 3, generator=g)
        D = ((a.numpy().astype(np.float64)[:, None] - b.numpy().astype(np.float64)[None]) ** 2).sum(-1)
        x, y = (torch.rand(7, 3, generator=g), torch.rand(7, 3, generator=g)) if ns == 7 else (a, a + 0.5)
        Dxy = ((x.numpy().astype(np.float64)[:, None] - y.numpy().astype(np.float64)[None]) ** 2).sum(-1)
        cd = O.compute_cd(torch.cat([x, x[:1]]), torch.cat([y, y[:1]]), torch.tensor([0, ns, ns + 1]))
        assert abs(float(cd[0]) - np.sqrt(0.5 * (Dxy.min(1).mean() + Dxy.min(0).mean()))) < 1e-12
        assert abs(float(cd[1]) - np.sqrt(Dxy[0, 0])) < 1e-12
        sp, tp = torch.rand(ns, 3, generator=g), torch.rand(nt, 3, generator=g)
        thr = float(np.sqrt(np.sort(D.min(1))[ns // 2])) + 1e-3
        rmse, n, ratio, nn = O.compute_correspondence_rmse(a, b, sp, tp, thr)
        j = D.argmin(1)
        ok = np.sqrt(D.min(1)) <= thr
        se = ((sp.numpy().astype(np.float64)[ok] - tp.numpy().astype(np.float64)[j[ok]]) ** 2).sum(1)
        assert n == ok.sum() >= 1 and ratio == n / ns and np.array_equal(nn.numpy(), j) and abs(float(rmse) - np.sqrt(se.mean())) < 1e-12


def test_voxel_oracles_agree_with_a_direct_restatement():
    rng = np.random.default_rng(57)
    for n, vs, shift in ((400, 0.2, 0.0), (90, 0.31, -3.0)):
        p = (rng.random((n, 3)) * 1.5 + shift).astype(np.float32)
        w = np.float32(vs)
        grid = np.floor(p / w)
        d = p - (grid + np.float32(0.5)) * w
        sq = d * d
        dist = np.sqrt((sq[:, 0] + sq[:, 1]) + sq[:, 2])
        level = (dist / dist.max() * np.float32(999)).astype(np.int64)
        g = grid.astype(np.int64); g -= g.min(axis=0)
        v = int(g.max())
        key = g[:, 0] + g[:, 1] * v + g[:, 2] * v * v
        order = np.lexsort((np.arange(n), level, key))                    # by key, then level, then index
        heads = np.concatenate([[True], key[order][1:] != key[order][:-1]])
        assert np.array_equal(O.voxel_down_sample(p, vs), order[heads])
        assert O.calculate_voxel_coverage(p, vs) == len({tuple(r) for r in grid.astype(np.int64)})
    assert O.calculate_voxel_coverage(np.zeros((0, 3), dtype=np.float32), 0.1) == 0
