"""CPU: the symmetric eigen-solvers the normals and the point-to-plane kernels run (rap_amd/csrc/kabsch.h, built for the host with g++)
against LAPACK; the argument checks and the workspace arithmetic of rap_estimate_normals; and the margins the GPU test
(tests/test_normals_gpu.py) relies on, measured from the yardstick (tests/icp_plane_oracle.py), not from the code under test."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import icp_plane_oracle as P
from conftest import ROOT
from rap_amd import _lib

N, ONE = ctypes.c_void_p(0), ctypes.c_void_p(256)      # NULL; a non-NULL sentinel -- every call below fails before a pointer is used
DP = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def eig_lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("host") / "libeig_host.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", out, os.path.join(ROOT, "tests", "host", "eig_host.cpp")])
    lib = ctypes.CDLL(out)
    lib.pinv6_step.argtypes = [DP, DP, ctypes.c_double, DP]
    return lib


def dp(a):
    return a.ctypes.data_as(DP)


def eig3(lib, C):
    C = np.ascontiguousarray(C, np.float64)
    lam, n = np.zeros(3), np.zeros(3)
    lib.eig3_smallest(dp(C), dp(lam), dp(n))
    return lam, n


@pytest.mark.parametrize("kind", ["covariance", "flat", "collinear", "two_equal", "scaled", "zero"])
def test_device_3x3_eigen_solver_matches_lapack(eig_lib, kind):
    rng = np.random.default_rng(sum(map(ord, kind)))
    worst_l = worst_n = 0.0
    for trial in range(200):
        Q = rng.normal(size=(int(rng.integers(3, 33)), 3))
        if kind == "flat":
            Q[:, 2] = 0.0
            Q = Q @ np.linalg.qr(rng.normal(size=(3, 3)))[0]
        elif kind == "collinear":
            Q = np.outer(rng.normal(size=Q.shape[0]), rng.normal(size=3))
        elif kind == "scaled":
            Q *= 10.0 ** rng.uniform(-6, 6)
        c = Q - Q.mean(axis=0)
        C = c.T @ c / Q.shape[0]
        if kind == "two_equal":
            U = np.linalg.qr(rng.normal(size=(3, 3)))[0]
            C = U @ np.diag([0.3, 1.0, 1.0]) @ U.T
        if kind == "zero":
            C = np.zeros((3, 3))
        lam, n = eig3(eig_lib, C)
        w, v = np.linalg.eigh(C)
        scale = max(w[-1], 1e-300)
        worst_l = max(worst_l, np.abs(lam - w).max() / scale)
        assert np.abs(lam - w).max() <= 1e-14 * scale and lam[0] <= lam[1] <= lam[2]
        assert abs(np.linalg.norm(n) - 1.0) < 1e-14
        assert np.abs(C @ n - lam[0] * n).max() <= 1e-14 * scale       # an eigenvector of the smallest eigenvalue, whatever the multiplicity
        if kind in ("covariance", "flat", "scaled", "two_equal"):       # ... and LAPACK's where it is unique
            assert (w[1] - w[0]) / scale > 1e-6
            dn = min(np.abs(n - v[:, 0]).max(), np.abs(n + v[:, 0]).max())
            worst_n = max(worst_n, dn * (w[1] - w[0]) / scale)
            assert dn <= 1e-14 * scale / (w[1] - w[0])
    print(f"{kind}: eigenvalues within {worst_l:.1e} of lambda_max, eigenvector error x relative gap {worst_n:.1e}")


@pytest.mark.parametrize("kind", ["full", "planar_target", "rank1", "scaled"])
def test_device_6x6_pseudo_inverse_step_matches_numpy_pinv(eig_lib, kind):
    rng = np.random.default_rng(sum(map(ord, kind)))
    worst = 0.0
    for trial in range(100):
        m = int(rng.integers(6, 200))
        p, n = rng.normal(size=(m, 3)), rng.normal(size=(m, 3))
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        if kind == "planar_target":
            n[:] = n[0]                                              # all normals parallel: rank 3
        elif kind == "rank1":
            p, n = p[:1], n[:1]
        J = np.concatenate([np.cross(p, n), n], axis=1)
        if kind == "scaled":
            J *= 10.0 ** rng.uniform(-4, 4)
        A, b = J.T @ J, J.T @ rng.normal(size=J.shape[0])
        x = np.zeros(6)
        eig_lib.pinv6_step(dp(np.ascontiguousarray(A)), dp(b), 1e-12, dp(x))
        want = -np.linalg.pinv(A, rcond=1e-12, hermitian=True) @ b
        lam = np.linalg.eigvalsh(A)
        kept = lam[lam > 1e-12 * lam[-1]]
        assert kept.min() / lam[-1] > 1e-9 or kind == "scaled"          # the cut is not close to an eigenvalue
        err = np.abs(x - want).max() / max(np.abs(want).max(), 1e-300)
        worst = max(worst, err * kept.min() / lam[-1])
        assert err <= 1e-12 * lam[-1] / kept.min(), (kind, trial, err)
        lam6, V = np.zeros(6), np.zeros((6, 6))
        eig_lib.eig6(dp(np.ascontiguousarray(A)), dp(lam6), dp(V))
        assert np.abs(np.sort(lam6) - lam).max() <= 1e-13 * lam[-1] and np.abs(V.T @ V - np.eye(6)).max() < 1e-13
    print(f"{kind}: worst relative step error x (lambda_min kept / lambda_max) {worst:.1e}")


def test_device_rodrigues_is_the_matrix_exponential(eig_lib):
    rng = np.random.default_rng(0)
    for th in (0.0, 1e-12, 1e-6, 9.9e-5, 1.01e-4, 1e-2, 1.0, 3.0):
        w = rng.normal(size=3)
        w = np.ascontiguousarray(w / np.linalg.norm(w) * th)
        R = np.zeros((3, 3))
        eig_lib.rodrigues(dp(w), dp(R))
        K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        want, term = np.eye(3), np.eye(3)
        for i in range(1, 40):                                           # the exponential series: |K| <= 3, terms below 1e-30 at i = 40
            term = term @ K / i
            want = want + term
        assert np.abs(R - want).max() < 1e-14 and np.abs(R - P.rodrigues(w)).max() < 1e-15, th


def call(lib, **kw):
    a = dict(P=ONE, seg=ONE, K=2, n=1000, max_nn=20, radius=0.5, vp=N, normals=ONE, eig=N, ws=ONE, wsb=1 << 30)
    a.update(kw)
    return lib.rap_estimate_normals(a["P"], a["seg"], a["K"], a["n"], a["max_nn"], a["radius"], a["vp"], a["normals"], a["eig"], a["ws"], a["wsb"], N)


def test_rap_estimate_normals_refuses_bad_arguments_without_a_gpu():
    lib = _lib.load()
    for name in ("P", "seg", "normals"):
        assert call(lib, **{name: N}) == -1, name
    assert call(lib, K=0) == -1 and call(lib, K=-1) == -1 and call(lib, n=0) == -1 and call(lib, n=1 << 31) == -1
    assert call(lib, max_nn=2) == -1 and call(lib, max_nn=33) == -1 and call(lib, radius=float("nan")) == -1
    need = lib.rap_normals_workspace_bytes(1000, 2)
    assert call(lib, ws=N) == -2 and call(lib, wsb=need - 1) == -2 and call(lib, wsb=0) == -2


def test_normals_workspace_query_is_host_arithmetic():
    q = _lib.load().rap_normals_workspace_bytes
    assert q(0, 1) == 0 and q(-4, 1) == 0 and q(100, 0) == 0
    up = lambda n: -(-n // 256) * 256
    for n, K in ((1, 1), (256, 1), (1000, 6), (20_000, 1)):
        assert q(n, K) == up((n // 256 + K + 1) * 32) + up(K * 4), (n, K)      # the work items, 32 bytes each, and a flag per segment
    assert q(1 << 40, 1) > 1 << 36


def test_python_entry_points_refuse_cpu_tensors_and_bad_arguments():
    import rap_amd
    pts = torch.zeros(8, 3)
    with pytest.raises(_lib.RapError):
        rap_amd.estimate_point_normals(pts)
    with pytest.raises(_lib.RapError):
        rap_amd.estimate_normals_packed(pts, torch.tensor([[0, 8]]))
    with pytest.raises(ValueError):
        rap_amd.estimate_point_normals(torch.zeros(8, 2))
    doc = rap_amd.estimate_point_normals.__doc__
    assert "viewpoint" in doc and "tangent planes" in doc and "zero vector" in doc      # the two stated departures from the reference


def test_gpu_test_input_keeps_a_neighbour_gap_and_an_eigenvalue_gap():
    c = P.NORMALS_CASE
    n, eig, counts, gap = P.normals_solved(c["seed"], c["n"], c["max_nn"], c["radius"])
    sep = ((eig[:, 1] - eig[:, 0]) / eig[:, 2]).min()
    print(f"smallest k-th / (k+1)-th neighbour gap {gap.min():.2e}, smallest (l1 - l0) / l2 {sep:.3f}")
    assert (counts == c["max_nn"]).all()
    assert gap.min() >= 1e-5 and sep >= 0.05
    an = P.surf_normals(P.normals_input(c["seed"], c["n"]).astype(np.float64))
    assert np.abs(np.abs((n * an).sum(axis=1)) - 1.0).max() < 0.05     # the plane fit is the surface normal to a few degrees
    assert (n[np.arange(n.shape[0]), np.abs(n).argmax(axis=1)] > 0).all()
    up = P.normals_solved(c["seed"], c["n"], c["max_nn"], c["radius"], P.VIEWPOINT)[0]
    toward = (up * (np.asarray(P.VIEWPOINT) - P.normals_input(c["seed"], c["n"]))).sum(axis=1)
    assert toward.min() > 1.0                                           # n . (v - p) is far from the flip


@pytest.mark.parametrize("n", P.SWEEP_LENGTHS)
def test_edge_sweep_lattices_keep_their_neighbour_sets_apart(n):
    L = P.sweep_lattice(n)
    for k in P.SWEEP_MAX_NN:
        _, _, counts, gap = P.estimate_normals(L, k, 0.0)
        assert (counts == min(k, n)).all() and gap.min() >= P.SWEEP_GAP, (n, k, gap.min())
    _, _, counts, gap = P.estimate_normals(L, 12, P.SWEEP_RADIUS)
    assert gap.min() >= P.SWEEP_GAP, (n, gap.min())
    if n >= 255:
        assert counts.min() < 3 <= counts.max() and counts.max() <= 12      # the radius leaves some rows without an estimate, and binds


# ---- the 300-segment batch (tests/test_table_scale_gpu.py) ---------------------------------------------------------------------------------
@pytest.mark.parametrize("max_nn", P.NORMALS_MAX_NN)
def test_batch_of_300_segments_keeps_its_neighbour_sets_apart(max_nn):
    b = P.normals_batch300()
    seg, K = b["seg"], P.NORMALS_K
    lengths = seg[:, 1]
    assert K == 300 and set(lengths) == set(P.NORMALS_LENGTHS) | {0, 1, 2}
    assert {int(n) for n in lengths[256:]} >= {0, 1, 2, 255, 257}                     # every kind also past the first round of the item kernel
    for k, j in P.NORMALS_REPEATS.items():
        assert k >= 256 > 0 <= j < k and tuple(seg[k]) == tuple(seg[j]) and lengths[k] >= 12
    assert min(P.NORMALS_REPEATS.values()) < 256 <= max(P.NORMALS_REPEATS.values())
    own = [k for k in range(K) if lengths[k] > 0 and k not in P.NORMALS_REPEATS]
    order = sorted(own, key=lambda k: seg[k, 0])
    ends = [(int(seg[k, 0]), int(seg[k, 0] + seg[k, 1])) for k in order]
    assert order != own and all(e0 <= s1 for (_, e0), (s1, _) in zip(ends, ends[1:])) and ends[-1][1] <= b["P"].shape[0]
    assert 300 < (~b["covered"]).sum() and b["covered"].sum() == sum(int(lengths[k]) for k in own)
    for k in own:
        assert np.array_equal(b["P"][seg[k, 0]:seg[k, 0] + seg[k, 1]], b["clouds"][k])
        assert np.array_equal(np.sort(b["clouds"][k], axis=0), np.sort(P.sweep_lattice(int(lengths[k])), axis=0))
    same = [k for k in own if lengths[k] == 40]
    assert len(same) > 10 and not np.array_equal(b["clouds"][same[0]], b["clouds"][same[1]])      # the same rows in another order
    ref = P.normals_batch300_solved(max_nn, True)
    gap = min(r[3].min() for r in ref if r is not None)
    clear, rows = 0, 0
    for k in own:
        n, eig, counts, _ = ref[k]
        assert (counts == min(max_nn, lengths[k])).all()
        toward = b["viewpoint"][k].astype(np.float64) - b["clouds"][k].astype(np.float64)
        clear += (np.abs((n * toward).sum(axis=1)) >= P.NORMALS_VIEW_CLEAR * np.linalg.norm(toward, axis=1))[counts >= 3].sum()
        rows += (counts >= 3).sum()
    print(f"max_nn {max_nn}: smallest neighbour gap {gap:.2e} (required {P.SWEEP_GAP:.0e}); {clear} of {rows} normals clear of the viewpoint's flip")
    assert gap >= P.SWEEP_GAP and clear == rows > 7000                 # every row: the GPU test compares every sign
    assert len({tuple(v) for v in b["viewpoint"]}) == K - len(P.NORMALS_REPEATS)
