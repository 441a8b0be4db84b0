"""CPU: the assignment of rap_amd/csrc/assign.h (the lines the device kernel compiles, built with g++) and its Python transcription
against SciPy itself; the combine rule of the column scan against the sequential scan; the fixture, the margins of the generated GPU
cases and the fp32 bound of the chamfer matrix.  SciPy is needed here and only here (the GPU tests compare with the transcription)."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import part_acc_oracle as O
from conftest import ROOT

RANDOM_SIZES = (5, 17, 64, 65, 130, 256)
DENSITIES = (0.05, 0.5, 0.95)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("host") / "libassign_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", out,
                           os.path.join(ROOT, "tests", "host", "assign_host.cpp")])
    lib = ctypes.CDLL(out)
    lib.lsap_solve01.restype = ctypes.c_int
    lib.lsap_solve01.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    lib.lsap_picks.restype = None
    lib.lsap_picks.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 5
    return lib


def solve_host(host, cost):
    c = np.ascontiguousarray(cost, dtype=np.uint8)
    n = c.shape[0]
    out = np.full(n, -7, dtype=np.int32)
    assert host.lsap_solve01(c.ctypes.data, n, out.ctypes.data) == 0
    return out.astype(np.int64)


def scipy_cols(cost):
    from scipy.optimize import linear_sum_assignment
    rows, cols = linear_sum_assignment(np.asarray(cost, dtype=np.float32))      # float32 0/1, as metrics.py:152 passes it
    assert np.array_equal(rows, np.arange(len(rows)))
    return cols.astype(np.int64)


def all_binary(n):
    for bits in itertools.product((0, 1), repeat=n * n):
        yield np.asarray(bits, dtype=np.uint8).reshape(n, n)


def random_binary(n, density, seed):
    return (np.random.default_rng(seed * 1000 + n).random((n, n)) < density).astype(np.uint8)


def test_header_solver_equals_scipy_on_every_small_binary_matrix(host):
    count = 0
    for n in (1, 2, 3, 4):
        for c in all_binary(n):
            assert np.array_equal(solve_host(host, c), scipy_cols(c)), c
            count += 1
    assert count == 2 + 16 + 512 + 65536


@pytest.mark.parametrize("n", RANDOM_SIZES)
def test_header_solver_equals_scipy_on_random_binary_matrices(host, n):
    for density in DENSITIES:
        for seed in range(6):
            c = random_binary(n, density, seed)
            assert np.array_equal(solve_host(host, c), scipy_cols(c)), (n, density, seed)
    # structured: the identity's complement (one zero per row), all zeros, all ones, a permutation's complement
    perm = np.random.default_rng(n).permutation(n)
    for c in (1 - np.eye(n, dtype=np.uint8), np.zeros((n, n), np.uint8), np.ones((n, n), np.uint8), 1 - np.eye(n, dtype=np.uint8)[perm]):
        assert np.array_equal(solve_host(host, c), scipy_cols(c))


def test_transcription_equals_scipy_on_every_small_binary_matrix():
    for n in (1, 2, 3, 4):
        for c in all_binary(n):
            assert np.array_equal(O.lsap(c), scipy_cols(c)), c


@pytest.mark.parametrize("n", RANDOM_SIZES)
def test_transcription_equals_scipy_on_random_binary_matrices(n):
    for density in DENSITIES:
        for seed in range(6 if n <= 65 else 2):
            c = random_binary(n, density, seed)
            assert np.array_equal(O.lsap(c), scipy_cols(c)), (n, density, seed)


def test_pick_combine_rule_equals_the_sequential_scan(host):
    """random scan states: a permutation prefix as the remaining list, few distinct values (so that ties are the rule, INFINITY among
    them), assigned and unassigned columns -- the fold of SciPy's loop, the left-to-right reduction and a balanced tree with swapped operands
    end on the same position and the same lowest value"""
    rng = np.random.default_rng(11)
    for trial in range(4000):
        n = int(rng.integers(1, 257))
        num = int(rng.integers(0, n + 1))
        remaining = rng.permutation(n).astype(np.int32)
        levels = int(rng.integers(1, 4))
        spc = rng.integers(0, levels, n).astype(np.float64)
        spc[rng.random(n) < rng.choice([0.0, 0.3, 1.0])] = np.inf
        row4col = np.where(rng.random(n) < rng.choice([0.0, 0.5, 1.0]), -1, rng.integers(0, n, n)).astype(np.int32)
        out, low = np.full(3, -9, np.int32), np.full(3, -9.0)
        host.lsap_picks(num, remaining.ctypes.data, spc.ctypes.data, row4col.ctypes.data, out.ctypes.data, low.ctypes.data)
        assert out[0] == out[1] == out[2], (trial, out)
        assert low[0] == low[1] == low[2], (trial, low)
        if num and np.isfinite(spc[remaining[:num]]).any():
            assert out[0] >= 0 and spc[remaining[out[0]]] == spc[remaining[:num]].min()


def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "part_acc.npz"))
    return {k: z[k] for k in z.files}


def test_fixture_reproduces_from_the_oracle():
    g = golden()
    ppp = g["points_per_part"]
    B, P = ppp.shape
    assert (B, P) == (4, 6) and ppp[ppp > 0].min() == 1 and ppp.max() == 70
    N = g["pointclouds_gt"].shape[1]
    cu = np.arange(B + 1) * N
    thr = float(g["threshold"])
    cd = O.chamfer_matrix(g["pointclouds_gt"].reshape(-1, 3), g["pointclouds_pred"].reshape(-1, 3), ppp, cu)
    assert np.array_equal(np.isnan(cd), np.isnan(g["cd"]))
    ok = ~np.isnan(cd)
    assert np.abs(cd[ok] - g["cd"][ok]).max() <= 1e-12 * g["cd"][ok].max()
    assert O.margins_ok(g["cd"], thr)
    acc, matched = O.part_acc_from_cd(g["cd"], ppp, thr)
    assert np.array_equal(acc, g["part_acc"]) and np.array_equal(matched, g["matched_part_ids"])
    # what the fixture is there to cover
    assert (ppp[1, 4:] == 0).all() and ppp[2, 1] == 0 and ppp[2, 2] > 0 and (ppp[3] > 0).sum() == 1
    assert g["part_acc"][0] < 1.0 and not np.array_equal(g["matched_part_ids"][0], np.arange(P))
    assert g["matched_part_ids"][2, 1] == 0 and g["matched_part_ids"][2, 0] == 1      # compacted indices: gt slot 0 <-> pred slot 2


def generated_cases():
    for name in O.EDGE_NAMES:
        yield name, O.edge_case(name)
    for n in O.LATTICE_SIZES:
        yield f"lattice-{n}", O.lattice_case(n, seed=n)
    yield "interchangeable", O.interchangeable_case()[0]


def test_generated_gpu_cases_keep_the_margin_and_the_fp32_bound():
    """every case the GPU tests run: no cd within 1e-3 * threshold of the threshold, and the oracle evaluated with fp32 distances (every
    operation rounded, the device's chain without its fused step) stays within CD_REL_BOUND of the float64 oracle.  The bound itself is
    derived next to O.CD_REL_BOUND: (1 + u)^6 - 1 with u = 2^-24, taken as 7 u."""
    u = 2.0 ** -24
    assert (1 + u) ** 6 - 1 < O.CD_REL_BOUND == 7 * u
    worst = 0.0
    for name, c in generated_cases():
        cd64 = O.chamfer_matrix(c["gt"], c["pred"], c["ppp"], c["cu"])
        assert O.margins_ok(cd64, c["threshold"]), name
        if name == "many-items" or name.startswith("lattice"):
            cd32 = cd64 if name.startswith("lattice") else None      # the lattice is exact in fp32
            if name.startswith("lattice"):
                v = cd64[~np.isnan(cd64)]
                assert ((v == 0) | (v >= 1)).all() and np.array_equal(v, np.round(v * 4) / 4)
            if cd32 is None:
                continue
        else:
            cd32 = O.chamfer_matrix(c["gt"], c["pred"], c["ppp"], c["cu"], np.float32)
        ok, ratio = O.cd_within_bound(cd32, cd64)
        assert ok, (name, ratio)
        worst = max(worst, ratio)
    print(f"worst |cd_fp32 - cd_fp64| / (2^-24 cd_fp64) over the generated cases: {worst:.3f} (bound {O.CD_REL_BOUND / u:.0f})")
    assert worst <= 7.0


def test_edge_cases_place_the_boundaries_where_the_sweep_says():
    ends = lambda name: np.cumsum(O.EDGE_CASES[name][0]).tolist()
    assert 256 in ends("boundary-on-edge") and 255 in ends("boundary-before-edge") and 257 in ends("boundary-after-edge")
    a, b = ends("three-tiles")[0], ends("three-tiles")[1]
    assert a // O.TILE == 0 and (a + 256) // O.TILE == 1 and (b - 1) // O.TILE == 2
    lens = {n for rows in O.EDGE_CASES.values() for r in rows for n in r if n}
    assert lens <= {1, 2, 63, 64, 65, 255, 256, 257, 513} and max(len(r) for rows in O.EDGE_CASES.values() for r in rows) <= 5
    c = O.edge_case("many-items")
    assert int((c["ppp"] > 0).sum()) > 1024 and c["ppp"].shape[1] <= 5
    big = O.lattice_case(256, seed=256)
    assert big["ppp"].shape == (1, 256) and (big["ppp"] > 0).all() and 350 <= big["gt"].shape[0] <= 450
