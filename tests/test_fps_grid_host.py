"""CPU: the bucket method of farthest point sampling (rap_amd/csrc/fps_grid.hip) restated sequentially on the functions of
rap_amd/csrc/fps_grid.h -- the lines the kernel compiles, built here with g++ (tests/host/fps_grid_host.cpp) -- against the sequential
oracle of oracle/rap_oracle.py: tie-heavy grids, lattices, duplicates, identical rows and a random real-valued cloud, at several bucket
sizes and bucket caps and with the rows inside every bucket in a scrambled order.  Also the workspace arithmetic, the grid rule, the
lower bound itself, and the exactness of the lattice inputs the GPU tests use."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle import preproc_cases as PC
from oracle import rap_oracle as O

PERS = (1, 8, 64)
CAPS = (4096, 50)
SRC = os.path.join(ROOT, "tests", "host", "fps_grid_host.cpp")
FLAGS = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("host") / "libfps_grid_host.so")
    subprocess.check_call(FLAGS + ["-shared", "-fPIC", "-o", out, SRC])
    lib = ctypes.CDLL(out)
    P = ctypes.c_void_p
    lib.fps_host_workspace_bytes.restype, lib.fps_host_workspace_bytes.argtypes = ctypes.c_size_t, [ctypes.c_int64]
    lib.fps_host_target.restype, lib.fps_host_target.argtypes = ctypes.c_int, [ctypes.c_int] * 3
    lib.fps_host_dims.restype, lib.fps_host_dims.argtypes = ctypes.c_float, [P, P, ctypes.c_int, ctypes.c_int, ctypes.c_int, P]
    lib.fps_host_sample.restype = ctypes.c_int
    lib.fps_host_sample.argtypes = [P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint, P, P]
    lib.fps_host_plain.restype, lib.fps_host_plain.argtypes = ctypes.c_int, [P, ctypes.c_int, ctypes.c_int, ctypes.c_int, P]
    return lib


def sample(host, cloud, K, start, per, cap, order_seed=0):
    p = np.ascontiguousarray(cloud.numpy(), dtype=np.float32)
    out = np.full(min(K, len(p)), -7, dtype=np.int32)
    stats = np.zeros(4, dtype=np.int64)
    k = host.fps_host_sample(p.ctypes.data, len(p), K, start, per, cap, order_seed, out.ctypes.data, stats.ctypes.data)
    assert k == len(out), k
    return torch.from_numpy(out.astype(np.int64)), stats


def check(host, cloud, K, start, pers=PERS, caps=CAPS):
    ref = O.farthest_point_sampling(cloud, cloud.shape[0], K, start)
    for per in pers:
        for cap in caps:
            for seed in (0, 12345):
                got, stats = sample(host, cloud, K, start, per, cap, seed)
                mism = torch.nonzero(got != ref)
                assert mism.numel() == 0, (per, cap, seed, f"first difference at pick {int(mism[0])}: {int(got[int(mism[0])])} vs {int(ref[int(mism[0])])}")
                assert 1 <= stats[0] <= cap and stats[1] <= stats[0]
    return ref


def test_tie_heavy_grids_equal_the_oracle(host):
    """16^3, 64 x 64 x 1 and 1 x 1 x 1100 integer grids (two, one and no axis with an extent missing), in order and shuffled, K = n:
    most picks are exact ties that cross buckets."""
    for cloud in (PC.grid_cloud(16, 16, 16), PC.grid_cloud(64, 64, 1), PC.grid_cloud(16, 16, 16, seed=4), PC.grid_cloud(64, 64, 1, seed=5),
                  PC.grid_cloud(1, 1, 1100)):
        n = cloud.shape[0]
        for start in (0, n // 2, n - 1):
            ref = check(host, cloud, n, start, caps=(4096,))
            assert sorted(ref.tolist()) == list(range(n))
    check(host, PC.grid_cloud(16, 16, 16, seed=4), 4096, 1, caps=(50, 1))


def test_lattices_duplicates_and_identical_rows_equal_the_oracle(host):
    check(host, PC.lattice_cloud(3000, 1, side=16), 3000, 5)
    check(host, PC.lattice_cloud(6000, 2), 700, 5999)
    base = PC.lattice_cloud(125, 3, side=5)
    dup = base.repeat(9, 1)[torch.from_numpy(np.random.RandomState(7).permutation(1125))]
    ref = check(host, dup, 1125, 17)
    assert ref[125:].eq(ref[125]).all()                    # once every distance is 0 the first arg-max stays where it is
    same = torch.full((200, 3), 1.5)
    ref = check(host, same, 200, 9)
    assert ref.tolist() == [9] + [0] * 199


def test_a_random_real_valued_cloud_equals_the_oracle(host):
    """No exact arithmetic here: the restatement and the oracle share one unfused fp32 expression, so the skip rule alone is on trial."""
    g = torch.Generator().manual_seed(31)
    cloud = (torch.randn(8000, 3, generator=g) * torch.tensor([20.0, 12.0, 1.5])).float()
    check(host, cloud, 1500, 4242)
    far = torch.cat([cloud[:2000] * 0.01, torch.tensor([[1e6, 1e6, 1e6]])])      # one far outlier: nearly everything in one bucket
    check(host, far, 300, 3, caps=(4096,))


def test_pruning_does_prune(host):
    """Counts of work, not times: on a surface-like cloud a pick opens a few buckets and touches a small share of the rows."""
    cloud = PC.outlier_cloud(20000, 1).float()
    got, stats = sample(host, cloud, 2000, 0, 32, 4096)
    plain = np.full(2000, -7, dtype=np.int32)
    p = np.ascontiguousarray(cloud.numpy())
    assert host.fps_host_plain(p.ctypes.data, 20000, 2000, 0, plain.ctypes.data) == 2000
    assert np.array_equal(got.numpy(), plain)
    rows_per_pick, opened_per_pick = stats[2] / 1998, stats[3] / 1998
    print(f"buckets {stats[0]} ({stats[1]} non-empty), rows touched per pick {rows_per_pick:.0f} of 20000, buckets opened per pick {opened_per_pick:.1f}")
    assert rows_per_pick < 2000 and opened_per_pick < 40      # a tenth of the cloud, generously: the plain loop touches 20 000 rows


def test_grid_rule_and_workspace_arithmetic(host):
    al = lambda v: (v + 255) // 256 * 256
    for T in (1, 15, 16, 17, 1000, 100000, 2 ** 31 - 1):
        assert host.fps_host_workspace_bytes(T) == al(16 * T) + al(4 * T)
    assert host.fps_host_workspace_bytes(0) == 0 and host.fps_host_workspace_bytes(-3) == 0
    from rap_amd import _lib
    lib = _lib.load()
    for T in (1, 17, 100000):
        assert lib.rap_fps_grid_workspace_bytes(T, 3) == host.fps_host_workspace_bytes(T)
    assert lib.rap_fps_grid_workspace_bytes(0, 3) == 0 and lib.rap_fps_grid_workspace_bytes(10, 0) == 0
    per, cap = ctypes.c_int32(-1), ctypes.c_int32(-1)
    lib.rap_fps_grid_params(ctypes.byref(per), ctypes.byref(cap))
    assert per.value in (16, 32, 48, 64, 128) and cap.value in (2048, 4096)
    N = ctypes.c_void_p(0)
    one = ctypes.c_void_p(256)
    assert lib.rap_farthest_point_sampling_grid(N, 10, one, one, one, one, 1, 4, one, one, 1 << 20, N) == -1
    assert lib.rap_farthest_point_sampling_grid(one, 10, one, one, one, one, 0, 4, one, one, 1 << 20, N) == -1
    assert lib.rap_farthest_point_sampling_grid(one, 10, one, one, one, one, 1, 0, one, one, 1 << 20, N) == -1
    assert lib.rap_farthest_point_sampling_grid(one, -1, one, one, one, one, 1, 4, one, one, 1 << 20, N) == -1
    assert lib.rap_farthest_point_sampling_grid(one, 10, one, one, one, one, 1, 4, one, N, 1 << 20, N) == -2
    assert lib.rap_farthest_point_sampling_grid(one, 10, one, one, one, one, 1, 4, one, one, 511, N) == -2
    # the target: ceil(n / per), capped
    assert [host.fps_host_target(n, 32, 4096) for n in (1, 32, 33, 64, 65, 32 * 4096 - 1, 32 * 4096 + 1, 10 ** 9)] == [1, 1, 2, 2, 3, 4096, 4096, 4096]
    dims = np.zeros(4, dtype=np.int32)
    f3 = lambda *v: np.asarray(v, dtype=np.float32)

    def rule(lo, hi, n, per=32, cap=4096):
        lo, hi = f3(*lo), f3(*hi)
        h = host.fps_host_dims(lo.ctypes.data, hi.ctypes.data, n, per, cap, dims.ctypes.data)
        return h, dims.tolist()
    assert rule((1, 2, 3), (1, 2, 3), 200)[1] == [1, 1, 1, 1]                      # identical rows: one bucket
    h, d = rule((0, 0, 0), (15, 15, 15), 4096)
    assert d[3] == d[0] * d[1] * d[2] and 64 <= d[3] <= 4096 and d[0] == d[1] == d[2]
    h, d = rule((0, 0, 0), (63, 63, 0), 4096)
    assert d[2] == 1 and d[0] == d[1] and 64 <= d[3] <= 4096                       # an axis without extent gets one cell
    h, d = rule((0, 0, 0), (0, 0, 1099), 1100)
    assert d[:2] == [1, 1] and 20 <= d[2] <= 4096
    for n in (32 * 4096 - 1, 32 * 4096 + 1, 10 ** 7):
        h, d = rule((-3, 0, 5), (40, 37, 8), n)
        assert 1024 <= d[3] <= 4096, d                                             # capped
    assert rule((0, 0, 0), (np.inf, 1, 1), 100)[1][3] == 0 and rule((0, 0, 0), (np.nan, 1, 1), 100)[1][3] == 0
    assert rule((-3e38, 0, 0), (3e38, 1, 1), 100)[1][3] == 0                       # an extent that overflows: the plain loop
    assert rule((0, 0, 0), (1e-30, 1e-30, 1e-30), 100)[1][3] >= 1                  # a tiny volume still gets a grid


def test_gpu_test_lattices_are_exact_in_fp32():
    """The lattice clouds of tests/test_fps_grid_gpu.py: distinct rows, and every sum of three squared differences below 2^22, so the
    distance is exact in fp32 whatever the compiler fuses and the index list is unique."""
    for n, seed, side in ((20000, 11, 1024), (100000, 12, 1024), (32 * 4096 + 1, 13, 1024), (3000, 1, 16)):
        c = PC.lattice_cloud(n, seed, side=side).numpy().astype(np.int64)
        assert len(np.unique(c, axis=0)) == n
        assert 3 * int(c.max() - c.min()) ** 2 < 2 ** 22
