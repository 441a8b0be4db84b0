"""GPU: edge sweep of the three brute-force nearest-neighbour kernels -- overlap_min_dist_kernel (overlap.hip), nn_query_kernel
(nn_metrics.hip) and pair_query_kernel (pair_metrics.hip) -- against the float64 oracle (inputs: tests/caller_edge_cases.py, checked by
tests/test_caller_edge_cases_host.py).  All three stream candidates through a 256-slot tile: sizes 1, 2 and either side of one, two and
three tiles; the true neighbour in the only occupied slot of a partial last tile, and in the first slot; inclusive thresholds met with
equality on lattices whose distances are exact in fp32; the first-arg-min rule on duplicated target points.  Counts are exact because
every threshold keeps a margin of 1e-5 from every distance of the oracle (asserted there); tolerances are the suite's existing ones."""
import numpy as np
import pytest
import torch

import caller_edge_cases as C
import rap_amd
from oracle import rap_oracle as O
from rap_amd import metrics

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def test_overlap_ratio_at_tile_edges_and_tail_slots(dev):
    o = C.overlap_batch()
    pts, ppp, cu, taus = o["pts"], o["ppp"], o["cu"], o["taus"]
    ratios, min_d = rap_amd.compute_overlap_ratio(pts.to(dev), ppp, cu, taus, return_min_distances=True)
    ref_ratios, ref_min = O.compute_overlap_ratio(pts, ppp, cu, taus)
    ratios, min_d = ratios.cpu().double(), min_d.cpu().double()
    fin = torch.isfinite(ref_min)
    assert torch.equal(torch.isfinite(min_d), fin)                        # inf exactly where a point has no point of another part
    assert float((min_d[fin] - ref_min[fin]).abs().max()) < 1e-6
    n = (cu[1:] - cu[:-1]).double()
    got, want = ratios * n[None, :], ref_ratios * n[None, :]
    assert float((got - got.round()).abs().max()) < 1e-3 and float((want - want.round()).abs().max()) < 1e-9
    assert torch.equal(got.round().long(), want.round().long())           # the ratios as counts: exact
    for b, q, which in o["tail"]:                                         # the query whose only near neighbour is the last / first point
        assert abs(float(min_d[q]) - 0.02) < 1e-5 and abs(float(min_d[q]) - float(ref_min[q])) < 1e-6, (b, which, float(min_d[q]))
    # the same without the caller's min-distance buffer
    assert torch.equal(rap_amd.compute_overlap_ratio(pts.to(dev), ppp, cu, taus).cpu().double(), ratios)


def test_overlap_threshold_is_inclusive_at_equality(dev):
    L = C.overlap_lattice()
    ratios, min_d = rap_amd.compute_overlap_ratio(L["pts"].to(dev), L["ppp"], L["cu"], L["taus"], return_min_distances=True)
    assert bool((min_d.cpu() == 0.25).all())                              # exact in fp32
    assert ratios.cpu().tolist() == [[1.0], [0.0]]                        # d <= 0.25 counts every point, d <= the number below it none


def test_chamfer_at_tile_edges_and_symmetry(dev):
    c = C.chamfer_batch()
    gt, pred = c["gt"].to(dev), c["pred"].to(dev)
    cd = metrics.compute_cd(gt, pred, c["cu"])
    ref = O.compute_cd(c["gt"], c["pred"], c["cu"])
    assert float((cd.cpu().double() - ref).abs().max()) < 2e-6
    assert torch.equal(metrics.compute_cd(pred, gt, c["cu"]), cd)         # bit-identical with the arguments exchanged


def test_correspondence_rmse_at_tile_edges(dev):
    for p in C.correspondence_pairs():
        rmse, n, ratio = metrics.compute_correspondence_rmse(p["sg"].to(dev), p["tg"].to(dev), p["sp"].to(dev), p["tp"].to(dev), p["thr"])
        o_rmse, o_n, o_ratio, _ = O.compute_correspondence_rmse(p["sg"], p["tg"], p["sp"], p["tp"], p["thr"])
        shape = (p["sg"].shape[0], p["tg"].shape[0])
        assert n == o_n and ratio == o_ratio, (shape, n, o_n)
        assert abs(float(rmse) - float(o_rmse)) < 2e-6 * float(o_rmse) + 1e-7, (shape, float(rmse), float(o_rmse))


def test_correspondence_takes_the_first_of_equal_minima(dev):
    """Every nearest target point occurs twice, at j < j', with different target_pred rows: the RMSE is the one of the LOWER index (the
    first minimum, numpy's argmin on the float64 distances), not of the higher."""
    T = C.correspondence_ties()
    s, t = T["sg"].numpy().astype(np.float64), T["tg"].numpy().astype(np.float64)
    D = ((s[:, None, :] - t[None, :, :]) ** 2).sum(-1)
    j = D.argmin(axis=1)                                                  # first minimum
    assert np.array_equal(j, T["first"])
    sp, tp = T["sp"].numpy().astype(np.float64), T["tp"].numpy().astype(np.float64)
    want = np.sqrt(((sp - tp[j]) ** 2).sum(1).mean())
    wrong = np.sqrt(((sp - tp[T["last"]]) ** 2).sum(1).mean())
    rmse, n, ratio = metrics.compute_correspondence_rmse(T["sg"].to(dev), T["tg"].to(dev), T["sp"].to(dev), T["tp"].to(dev), T["thr"])
    assert n == len(s) and ratio == 1.0
    assert abs(float(rmse) - want) < 2e-6 * want + 1e-7, (float(rmse), want, wrong)


def test_correspondence_threshold_is_inclusive_at_equality(dev):
    K = C.correspondence_lattice()
    args = [K[k].to(dev) for k in ("sg", "tg", "sp", "tp")]
    rmse, n, ratio = metrics.compute_correspondence_rmse(*args, distance_threshold=0.25)
    o_rmse, o_n, _, _ = O.compute_correspondence_rmse(K["sg"], K["tg"], K["sp"], K["tp"], 0.25)
    assert n == o_n == K["sg"].shape[0] and ratio == 1.0                  # sqrt(d2) <= 0.25 with sqrt(d2) == 0.25
    assert abs(float(rmse) - float(o_rmse)) < 2e-6 * float(o_rmse) + 1e-7   # (two targets tie for every inner source: the first one)
    rmse, n, ratio = metrics.compute_correspondence_rmse(*args, distance_threshold=C.F32_BELOW_QUARTER)
    assert n == 0 and ratio == 0.0 and bool(torch.isinf(rmse))


def test_batched_pairs_agree_with_the_single_pair_function_at_tile_edges(dev):
    """The (Ns, Nt) list as the samples of one compute_pair_metrics call (direct mode), per pair against compute_correspondence_rmse on
    the parts scaled by torch, under the tolerances of tests/test_evaluator_gpu.py::test_batched_pairs_agree_with_the_single_pair_function."""
    data, cloud, thr = C.pair_batch()
    data = {k: v.to(dev) for k, v in data.items()}
    cloud = cloud.to(dev)
    pm = metrics.compute_pair_metrics(data, cloud, distance_threshold=thr).cpu().numpy()
    cu = data["cu_seqlens_batch"].cpu().numpy()
    sp = torch.repeat_interleave(data["scales"], torch.from_numpy(np.diff(cu)).to(dev).long()).view(-1, 1)
    gt_s, pr_s = data["pointclouds_gt"] * sp, cloud * sp
    for b, (n0, n1) in enumerate(C.CORR_PAIRS):
        a = int(cu[b])
        rmse, n, ratio = metrics.compute_correspondence_rmse(gt_s[a:a + n0], gt_s[a + n0:a + n0 + n1], pr_s[a:a + n0], pr_s[a + n0:a + n0 + n1], thr)
        assert int(pm[b, 3]) == n and n >= 1, (b, pm[b], n)
        assert pm[b, 1] == np.float32(ratio)
        assert abs(float(pm[b, 0]) - float(rmse)) <= 2e-6 * float(rmse), (b, pm[b, 0], float(rmse))
        assert np.isinf(pm[b, 2])                                         # no transform error without predicted poses


def test_a_pair_of_more_than_64_items_matches_the_float64_oracle(dev):
    """16 700 sources are 66 items of 256: pair_finish_kernel's lane-strided sum of item partials takes a second round, which no other
    pair of the suite reaches (the largest has 4096 sources).  The ordinary pair after it starts at item 66.  Against the float64
    oracle on the scaled parts, under test_correspondence_rmse_at_tile_edges' bounds: the count exactly, the rmse to 2e-6 relative + 1e-7."""
    data, cloud, thr, pairs = C.large_pair_batch()
    pm = metrics.compute_pair_metrics({k: v.to(dev) for k, v in data.items()}, cloud.to(dev), distance_threshold=thr).double().cpu().numpy()
    again = metrics.compute_pair_metrics({k: v.to(dev) for k, v in data.items()}, cloud.to(dev), distance_threshold=thr).double().cpu().numpy()
    assert np.array_equal(pm, again)
    for b, p in enumerate(pairs):
        s = data["scales"][b].double()
        o_rmse, o_n, o_ratio, _ = O.compute_correspondence_rmse(p["sg"].double() * s, p["tg"].double() * s, p["sp"].double() * s, p["tp"].double() * s, thr)
        print(f"{tuple(p['sg'].shape)} x {tuple(p['tg'].shape)}: count {int(pm[b, 3])} (oracle {o_n}), rmse {pm[b, 0]:.6f} (oracle {float(o_rmse):.6f}, "
              f"relative deviation {abs(pm[b, 0] - float(o_rmse)) / float(o_rmse):.2e})")
        assert int(pm[b, 3]) == o_n and o_n >= 1
        assert pm[b, 1] == np.float32(o_n / p["sg"].shape[0])
        assert abs(pm[b, 0] - float(o_rmse)) < 2e-6 * float(o_rmse) + 1e-7
        assert np.isinf(pm[b, 2])                                         # no transform error without predicted poses
