"""GPU: edge sweep of the per-part Procrustes fit, the rigid apply (procrustes.hip) and the rigidity RMSE (rigidity.hip) against the
float64 oracle on the same fp32 inputs (inputs: tests/caller_edge_cases.py, checked by tests/test_caller_edge_cases_host.py).

Part sizes from 1 to 70001 points: every chunk count of the moments kernel with an even and an uneven split, chunks walked in one, two
and three batches of 2048 with a weighted tail, parts past 16 x 2048 points; empty parts leading, inside and trailing a sample; the
degenerate geometries of the host Kabsch test through the device path (fp64 moments, the reduce-scatter butterfly, H from raw moments);
parts far from the origin.  Tolerances are the suite's existing ones (2e-6 on R and t, 5e-6 relative on the RMSE).

The oracle, like the reference, indexes a sample's non-empty parts by position (it assumes that empty parts trail); it is called on the
table with the empty parts moved behind -- the same points in the same order -- and its rows are mapped back."""
import pytest
import torch

import caller_edge_cases as C
import rap_amd
from oracle import rap_oracle as O
from rap_amd.procrustes import rigidify_blend

pytestmark = pytest.mark.gpu

RT_BOUND = 2e-6          # tests/test_kernels_gpu.py::test_procrustes_fit_and_rigidify_match_oracle
RMSE_REL = 5e-6          # tests/test_sample_gpu.py::test_rigidity_rmse_edge_cases_match_oracle


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def sweep(dev):
    """the sweep batch, the device fit and the oracle fit (float64, rows at the original part columns), computed once"""
    s = dict(C.procrustes_sweep())
    s["cp"], s["where"] = C.compacted(s["ppp"])
    Rr, tr = O.fit_transformations(s["src"].double(), s["tgt"].double(), s["cp"], s["cu"])
    s["R_ref"], s["t_ref"] = C.uncompact(Rr, s["where"]), C.uncompact(tr, s["where"])
    R, t = rap_amd.fit_transformations(s["src"].to(dev), s["tgt"].to(dev), s["ppp"], s["cu"])
    s["R"], s["t"] = R, t
    return s


def _residual(src, tgt, R, t):
    return float(((src.double() @ R.double().T + t.double()) - tgt.double()).pow(2).sum())


def test_fit_matches_the_oracle_at_every_part_size(sweep):
    s = sweep
    R, t = s["R"].cpu(), s["t"].cpu()
    assert bool(torch.isfinite(R).all()) and bool(torch.isfinite(t).all())
    B, P = s["ppp"].shape
    for b in range(B):
        for p in range(P):
            n = int(s["ppp"][b, p])
            a = int(s["off"][b * P + p])
            if n == 0:
                assert torch.equal(R[b, p], torch.zeros(3, 3)) and torch.equal(t[b, p], torch.zeros(3)), (b, p)      # exact zeros
            elif n >= 3:
                eR = float((R[b, p].double() - s["R_ref"][b, p]).abs().max())
                et = float((t[b, p].double() - s["t_ref"][b, p]).abs().max())
                assert eR < RT_BOUND and et < RT_BOUND, (n, eR, et)
            else:                                                          # the rotation is not unique: a proper rotation with the optimal residual
                Rd = R[b, p].double()
                assert abs(float(torch.det(Rd)) - 1.0) < 1e-5 and float((Rd @ Rd.T - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-5, n
                src, tgt = s["src"][a:a + n], s["tgt"][a:a + n]
                res, res_ref = _residual(src, tgt, R[b, p], t[b, p]), _residual(src, tgt, s["R_ref"][b, p], s["t_ref"][b, p])
                assert res <= res_ref + 1e-6 * (1 + res_ref), (n, res, res_ref)


def test_every_part_of_the_batch_equals_its_solitary_fit(sweep, dev):
    """Chunking depends on the part's size alone and the partials are combined in a fixed order: a part's (R, t) does not depend on
    where it sits in a batch -- bit for bit."""
    s = sweep
    R, t = s["R"].cpu(), s["t"].cpu()
    src, tgt = s["src"].to(dev), s["tgt"].to(dev)
    B, P = s["ppp"].shape
    for k in range(B * P):
        a, e = int(s["off"][k]), int(s["off"][k + 1])
        if e > a:
            Rs, ts = rap_amd.solve_procrustes(src[a:e], tgt[a:e])
            assert torch.equal(Rs.cpu(), R[k // P, k % P]) and torch.equal(ts.cpu(), t[k // P, k % P]), e - a


def test_rigidify_and_blend_match_the_oracle(sweep, dev):
    s = sweep
    # rigidify(prediction, condition): every part of the condition moved onto the prediction
    ref = O.rigidify_prediction_with_procrustes(s["tgt"].double(), s["src"].double(), s["cp"], s["cu"])
    out = rap_amd.rigidify_prediction_with_procrustes(s["tgt"].to(dev), s["src"].to(dev), s["ppp"], s["cu"])
    assert float((out.cpu().double() - ref).abs().max()) < RT_BOUND
    g = torch.Generator().manual_seed(3)
    x1 = torch.randn(s["src"].shape, generator=g)
    w0, w1 = 0.35, 0.65
    blend = rigidify_blend(s["tgt"].to(dev), s["src"].to(dev), s["ppp"], x1.to(dev), w0, w1)
    want = ref * float(torch.tensor(w0)) + x1.double() * float(torch.tensor(w1))          # x0_rigid * w0 + x_1 * w1, the fp32 weights
    assert float((blend.cpu().double() - want).abs().max()) < RT_BOUND


def _rel(got, ref):
    """worst relative deviation over the finite entries; the infinite ones must coincide"""
    got, ref = got.cpu().double(), ref.double()
    assert torch.equal(torch.isinf(got), torch.isinf(ref)), (got, ref)
    fin = torch.isfinite(ref)
    return float(((got[fin] - ref[fin]).abs() / ref[fin].abs()).max())


def test_rigidity_rmse_matches_the_oracle(sweep, dev):
    s = sweep
    src, tgt, sc = s["src"].to(dev), s["tgt"].to(dev), s["scales"]
    Rc, tc = C.compact_like(s["R"].cpu().double(), s["where"]), C.compact_like(s["t"].cpu().double(), s["where"])
    for per_part in (False, True):
        for scales in (None, sc):
            got = rap_amd.compute_rigidity_rmse(src, tgt, s["R"], s["t"], s["ppp"], s["cu"], None if scales is None else scales.to(dev), per_part)
            ref = O.compute_rigidity_rmse(s["src"].double(), s["tgt"].double(), Rc, tc, s["cp"], s["cu"],
                                          None if scales is None else scales.double(), per_part)
            assert bool(torch.isinf(got[2])) and bool(torch.isinf(ref[2]))                # the sample without points
            rel = _rel(got, ref)
            print(f"rigidity rmse per_part={per_part} scales={scales is not None}: worst relative deviation {rel:.2e}")
            assert rel < RMSE_REL, (per_part, scales is not None, rel)


def test_trajectory_rigidity_matches_the_oracle(sweep, dev):
    s = sweep
    mean_ref, per_ref = O.average_trajectory_rigidity_rmse(s["src"].double(), s["traj"].double(), s["cp"], s["cu"], s["scales"].double())
    mean, per = rap_amd.average_trajectory_rigidity_rmse(s["src"].to(dev), s["traj"].to(dev), s["ppp"], s["cu"], s["scales"].to(dev),
                                                         return_per_step=True)
    assert per.shape == (3, s["ppp"].shape[0]) and bool(torch.isinf(per[:, 2]).all()) and bool(torch.isinf(mean[2]))
    assert _rel(per, per_ref) < RMSE_REL and _rel(mean, mean_ref) < RMSE_REL


def test_degenerate_geometry_on_the_device(dev):
    """The kinds of tests/test_host_logic.py::test_device_kabsch_code_matches_oracle_svd, `coincident` (H = 0) and `two_points` through
    the device path, with that test's criteria per kind."""
    d = C.degenerate_parts()
    R, t = rap_amd.fit_transformations(d["src"].to(dev), d["tgt"].to(dev), d["ppp"], d["cu"])
    R, t = R.cpu().reshape(-1, 3, 3), t.cpu().reshape(-1, 3)
    assert bool(torch.isfinite(R).all()) and bool(torch.isfinite(t).all())
    for k, (kind, n) in enumerate(d["cases"]):
        a, e = int(d["off"][k]), int(d["off"][k + 1])
        src, tgt = d["src"][a:e], d["tgt"][a:e]
        Rd = R[k].double()
        assert abs(float(torch.det(Rd)) - 1.0) < 1e-5, (kind, n)
        assert float((Rd @ Rd.T - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-5, (kind, n)
        Rr, tr = O.solve_procrustes(src.double(), tgt.double())
        if kind in C.DEGENERATE_FREE:
            res, res_ref = _residual(src, tgt, R[k], t[k]), _residual(src, tgt, Rr, tr)
            assert res <= res_ref + 1e-6 * (1 + res_ref), (kind, n, res, res_ref)
        else:
            eR, et = float((Rd - Rr).abs().max()), float((t[k].double() - tr).abs().max())
            assert eR < RT_BOUND and et < RT_BOUND, (kind, n, eR, et)


def test_parts_far_from_the_origin(dev):
    """H = sum s t^T - n mu_s mu_t^T from raw fp64 moments, at 300 and 1000 units from the origin with a spread of 5: R within 2e-6, t
    within 2e-6 plus one fp32 rounding of the stored t, and no worse than the reference's own arithmetic in fp32 on the same input.
    Each case twice: the target rotated about the origin (the fitted t is small) and about the part's own centre (|t| up to 1450, where
    one fp32 rounding of the stored t is up to 6e-5).  Measured on an MI355X, worst component, kernel / the reference's fp32 arithmetic:
        about the origin   300, n  4097: dR 2.5e-08 / 1.7e-07   dt 5.7e-09 / 3.5e-05
                           300, n 70001: dR 2.5e-08 / 2.6e-06   dt 2.7e-09 / 6.8e-04
                          1000, n  4097: dR 2.8e-08 / 5.3e-07   dt 5.2e-08 / 5.6e-04
                          1000, n 70001: dR 2.8e-08 / 1.4e-06   dt 1.1e-08 / 1.6e-03
        about the centre   300, n  4097: dR 2.5e-08 / 3.8e-07   dt 9.0e-06 / 8.0e-05
                           300, n 70001: dR 1.7e-08 / 7.4e-07   dt 2.7e-06 / 3.3e-05
                          1000, n  4097: dR 2.7e-08 / 3.9e-07   dt 5.2e-05 / 4.4e-04
                          1000, n 70001: dR 2.8e-08 / 7.1e-07   dt 3.8e-05 / 9.8e-04"""
    f = C.far_parts()
    R, t = rap_amd.fit_transformations(f["src"].to(dev), f["tgt"].to(dev), f["ppp"], f["cu"])
    R, t = R.cpu().reshape(-1, 3, 3), t.cpu().reshape(-1, 3)
    for j, frame in enumerate(C.FAR_FRAMES):
        for i, (offset, spread, n) in enumerate(C.FAR_CASES):
            k = 4 * j + i
            a, e = int(f["off"][k]), int(f["off"][k + 1])
            src, tgt = f["src"][a:e], f["tgt"][a:e]
            Rr, tr = O.solve_procrustes(src.double(), tgt.double())
            R32, t32 = O.solve_procrustes(src, tgt)                       # the reference's arithmetic: float32 throughout
            eR, et = float((R[k].double() - Rr).abs().max()), float((t[k].double() - tr).abs().max())
            eR32, et32 = float((R32.double() - Rr).abs().max()), float((t32.double() - tr).abs().max())
            t_bound = RT_BOUND + 2.0 ** -23 * float(tr.abs().max())
            print(f"far from the origin, rotated about the {frame}: offset {offset:g} spread {spread:g} n {n}: kernel dR {eR:.2e} dt {et:.2e} "
                  f"(bound {t_bound:.2e}, largest |t| {float(tr.abs().max()):.1f}); fp32 reference dR {eR32:.2e} dt {et32:.2e}")
            assert eR < RT_BOUND and et <= t_bound, (frame, offset, n, eR, et, t_bound)
            assert eR <= eR32 + RT_BOUND and et <= et32 + t_bound, (frame, offset, n, eR, eR32, et, et32)
