"""Farthest point sampling over the bucket index (rap_amd/csrc/fps_grid.hip, rap_farthest_point_sampling_grid): for every input the index
lists of rap_farthest_point_sampling, element for element.  Two yardsticks, neither of them the code under test: the sequential
oracle of oracle/rap_oracle.py on exact-arithmetic inputs (integer lattices and grids of oracle/preproc_cases.py, where the fp32
distance is exact whatever the compiler fuses), and the brute-force kernel (held to that oracle by tests/test_preproc_scale_gpu.py)
on everything else."""
import ctypes

import numpy as np
import pytest
import torch

import test_preproc_scale_gpu as TPS
from oracle import preproc_cases as PC
from oracle import rap_oracle as O
from rap_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def grid_params():
    per, cap = ctypes.c_int32(-1), ctypes.c_int32(-1)
    _lib.load().rap_fps_grid_params(ctypes.byref(per), ctypes.byref(cap))
    return per.value, cap.value


def fps_grid_abi(dev, clouds, Ks, starts, tail_rows=1):
    """rap_farthest_point_sampling_grid on a packed batch of clouds (as TPS.fps_abi) -> idx (C, Kmax) int64 on the CPU.  The workspace is
    exactly the queried size; `out` starts as -7 so that the -1 padding is the kernel's."""
    lib = _lib.load()
    lens = [int(p.shape[0]) for p in clouds]
    pts = torch.cat([p.float() for p in clouds] + [torch.zeros(tail_rows, 3)]).to(dev).contiguous()
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    cloud_start = i32(np.concatenate([[0], np.cumsum(lens)[:-1]]).tolist()); cloud_len = i32(lens); k_d = i32(list(Ks)); st_d = i32(list(starts))
    Kmax = max(1, max(Ks))
    out = torch.full((len(clouds), Kmax), -7, dtype=torch.int32, device=dev)
    T = pts.shape[0]
    need = lib.rap_fps_grid_workspace_bytes(T, len(clouds))
    assert need >= 20 * T
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = lib.rap_farthest_point_sampling_grid(_lib.ptr(pts), T, _lib.ptr(cloud_start), _lib.ptr(cloud_len), _lib.ptr(k_d), _lib.ptr(st_d),
                                                  len(clouds), Kmax, _lib.ptr(out), _lib.ptr(ws), need, _lib.current_stream(dev))
    assert rc == TPS.RAP_OK
    torch.cuda.synchronize(dev)
    return out.cpu().long()


def assert_same(got, want, what=""):
    mism = torch.nonzero(got != want)
    assert mism.numel() == 0, f"{what}: first difference at {mism[0].tolist()}: grid {int(got[tuple(mism[0])])}, reference {int(want[tuple(mism[0])])}"


def check_oracle(dev, cloud, K, start):
    got = fps_grid_abi(dev, [cloud], [K], [start])[0]
    ref = O.farthest_point_sampling(cloud, cloud.shape[0], K, start, device=dev)
    assert_same(got[:ref.numel()], ref, f"n={cloud.shape[0]} K={K} start={start}")
    assert (got[ref.numel():] == -1).all()
    return ref


def check_brute(dev, clouds, Ks, starts):
    got, want = fps_grid_abi(dev, clouds, Ks, starts), TPS.fps_abi(dev, clouds, Ks, starts)
    assert_same(got, want, f"lengths {[int(c.shape[0]) for c in clouds]}")
    return got


# ---------------------------------------------------------------------------------------------
# lattices and tie-heavy grids
# ---------------------------------------------------------------------------------------------
def test_lattice_4096_of_20000_equals_the_oracle(dev):
    ref = check_oracle(dev, PC.lattice_cloud(20000, 11), 4096, 12345)
    assert ref.unique().numel() == 4096


def test_lattice_20000_of_100000_equals_the_brute_force_kernel(dev):
    got = check_brute(dev, [PC.lattice_cloud(100000, 12)], [20000], [99999])
    assert got[0].unique().numel() == 20000


GRIDS = {"16^3": lambda: PC.grid_cloud(16, 16, 16), "64x64x1": lambda: PC.grid_cloud(64, 64, 1), "16^3 shuffled": lambda: PC.grid_cloud(16, 16, 16, seed=4),
         "64x64x1 shuffled": lambda: PC.grid_cloud(64, 64, 1, seed=5), "1x1x1100": lambda: PC.grid_cloud(1, 1, 1100)}


@pytest.mark.parametrize("name", list(GRIDS))
def test_tie_heavy_grids_from_several_starts_equal_the_oracle(dev, name):
    """Two, one and no degenerate axis; K = n, so most picks are exact ties, and ties that cross buckets: the winner is the lowest
    ORIGINAL index, whichever bucket holds it and wherever the sort put it.  The five starts run as five clouds of one launch."""
    cloud = GRIDS[name]()
    n = cloud.shape[0]
    starts = [0, 1, n // 2, n - 65, n - 1]
    got = fps_grid_abi(dev, [cloud] * 5, [n] * 5, starts)
    for row, start in enumerate(starts):
        ref = O.farthest_point_sampling(cloud, n, n, start, device=dev)
        assert_same(got[row], ref, f"{name} start {start}")
        assert sorted(ref.tolist()) == list(range(n))


# ---------------------------------------------------------------------------------------------
# ragged launches, clamped starts, K > length, -1 padding, zero-length clouds
# ---------------------------------------------------------------------------------------------
LENGTHS = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 2049]


@pytest.fixture(scope="module")
def ragged_clouds():
    return [PC.lattice_cloud(n, 20 + i, side=16) if n else torch.zeros(0, 3) for i, n in enumerate(LENGTHS)]


@pytest.mark.parametrize("rot", range(4))
def test_ragged_launch_equals_the_oracle(dev, ragged_clouds, rot):
    Ks = [max(1, (1, n, n + 7, 5)[(i + rot) % 4]) for i, n in enumerate(LENGTHS)]
    starts = [0 if n == 0 else (i * 37 + rot) % n for i, n in enumerate(LENGTHS)]
    idx = fps_grid_abi(dev, ragged_clouds, Ks, starts)
    assert idx.shape == (10, max(Ks))
    for i, n in enumerate(LENGTHS):
        if n == 0:
            assert (idx[i] == -1).all()
            continue
        ref = O.farthest_point_sampling(ragged_clouds[i], n, Ks[i], starts[i], device=dev)
        k = ref.numel()
        assert k == min(Ks[i], n) and torch.equal(idx[i, :k], ref) and (idx[i, k:] == -1).all(), (rot, i)
        if Ks[i] >= n:
            assert sorted(idx[i, :n].tolist()) == list(range(n))
    assert_same(idx, TPS.fps_abi(dev, ragged_clouds, Ks, starts), "against the brute-force kernel")


def test_out_of_range_starts_clamp_and_64_clouds_in_one_launch(dev, ragged_clouds):
    sub = [ragged_clouds[3], ragged_clouds[5], ragged_clouds[7], ragged_clouds[0]]
    idx = fps_grid_abi(dev, sub, [63, 10, 40, 3], [-5, 65, 1 << 20, 9])
    for row, (cl, K, st) in enumerate(((sub[0], 63, 0), (sub[1], 10, 64), (sub[2], 40, 1023))):      # negative -> 0, >= length -> length - 1
        ref = O.farthest_point_sampling(cl, cl.shape[0], K, st, device=dev)
        assert torch.equal(idx[row, :K], ref) and (idx[row, K:] == -1).all(), row
    assert (idx[3] == -1).all()
    many = [PC.lattice_cloud(50 + 31 * i, 100 + i, side=13 + i % 5) for i in range(64)]
    Ks = [1 + (i * 13) % 90 for i in range(64)]
    starts = [(i * 7) % many[i].shape[0] for i in range(64)]
    idx = fps_grid_abi(dev, many, Ks, starts)
    for i in range(64):
        ref = O.farthest_point_sampling(many[i], many[i].shape[0], Ks[i], starts[i], device=dev)
        assert torch.equal(idx[i, :ref.numel()], ref) and (idx[i, ref.numel():] == -1).all(), i


# ---------------------------------------------------------------------------------------------
# bucket edges: sizes from the library, not from a copy of its constants
# ---------------------------------------------------------------------------------------------
def test_bucket_edges_around_one_and_two_buckets(dev):
    per, _ = grid_params()
    for n in (per - 1, per, per + 1, 2 * per, 2 * per + 1):
        for start in (0, n - 1):
            ref = check_oracle(dev, PC.lattice_cloud(n, 40 + n, side=16), n, start)
            assert sorted(ref.tolist()) == list(range(n))


@pytest.mark.parametrize("delta", [-1, 1])
def test_bucket_edges_at_the_cap(dev, delta):
    """n = points per bucket x bucket cap -+ 1: the last size at which the grid may aim at its points per bucket and the first at which
    the cap makes the buckets grow."""
    per, cap = grid_params()
    n = per * cap + delta
    check_oracle(dev, PC.lattice_cloud(n, 13), 64, n - 3)


# ---------------------------------------------------------------------------------------------
# inputs on which the index cannot help, or cannot be built
# ---------------------------------------------------------------------------------------------
def test_one_far_outlier_leaves_nearly_everything_in_one_bucket(dev):
    g = torch.Generator().manual_seed(5)
    v = torch.randn(5000, 3, generator=g)
    ball = v / v.norm(dim=1, keepdim=True) * torch.rand(5000, 1, generator=g) ** (1 / 3)
    cloud = torch.cat([ball[:2500], torch.tensor([[1e6, 1e6, 1e6]]), ball[2500:]]).float()
    got = check_brute(dev, [cloud], [300], [7])
    assert got[0, 1] == 2500 and got[0].unique().numel() == 300


def test_duplicates_and_identical_rows(dev):
    """125 lattice points x 9 copies, shuffled, K = n: after 125 picks every distance is 0 and the picks go on (the first arg-max of an
    all-zero array).  Then 200 identical rows."""
    base = PC.lattice_cloud(125, 3, side=5)
    dup = base.repeat(9, 1)[torch.from_numpy(np.random.RandomState(7).permutation(1125))]
    ref = check_oracle(dev, dup, 1125, 17)
    assert ref[:125].unique().numel() == 125 and ref[125:].eq(ref[125]).all()
    same = torch.full((200, 3), 1.5)
    ref = check_oracle(dev, same, 200, 9)
    assert ref.tolist() == [9] + [0] * 199
    check_brute(dev, [dup, same], [1125, 200], [17, 9])


@pytest.mark.parametrize("bad", [float("inf"), float("-inf")], ids=["+inf", "-inf"])
def test_non_finite_rows_take_the_plain_loop_and_equal_the_brute_force_kernel(dev, bad):
    g = torch.Generator().manual_seed(9)
    cloud = (torch.randn(3000, 3, generator=g) * torch.tensor([5.0, 3.0, 1.0])).float()
    cloud[1234] = torch.tensor([float("nan"), 0.5, 0.5])
    cloud[77, 1] = bad
    clean = (torch.randn(2000, 3, generator=g)).float()
    for start in (0, 1234, 77):
        check_brute(dev, [cloud, clean], [300, 300], [start, 5])      # the finite cloud beside it keeps its index


# ---------------------------------------------------------------------------------------------
# a real-valued cloud
# ---------------------------------------------------------------------------------------------
def test_real_valued_cloud_equals_the_brute_force_kernel_and_picks_a_farthest_point(dev):
    """The cloud of TPS.test_fps_picks_a_farthest_point_on_a_real_valued_cloud: here near-ties are decided by the last bit of the fp32
    distance, so the two kernels agree only if they compute the same bits.  Also that test's fp64 property: every pick's distance is
    >= (1 - 2^-20) x the maximum."""
    g = torch.Generator().manual_seed(31)
    cloud = (torch.randn(100000, 3, generator=g) * torch.tensor([20.0, 12.0, 1.5])).float()
    K = 2000
    idx = check_brute(dev, [cloud], [K], [4242])[0]
    assert idx[0] == 4242 and idx.min() >= 0 and idx.unique().numel() == K
    p = cloud.double().to(dev)
    d = torch.full((100000,), float("inf"), dtype=torch.float64, device=dev)
    picked = torch.empty(K - 1, dtype=torch.float64, device=dev); best = torch.empty(K - 1, dtype=torch.float64, device=dev)
    idx_d = idx.to(dev)
    for k in range(1, K):
        d = torch.minimum(d, ((p - p[idx_d[k - 1]]) ** 2).sum(-1))
        picked[k - 1] = d[idx_d[k]]; best[k - 1] = d.max()
    ratio = (picked / best).min().item()
    print(f"fps grid property: min over picks of d(pick) / max d = 1 - {1 - ratio:.2e}")
    assert ratio >= 1 - 2.0 ** -20


# ---------------------------------------------------------------------------------------------
# determinism; every block size and bucket size
# ---------------------------------------------------------------------------------------------
def test_two_calls_agree_and_a_cloud_does_not_see_its_neighbours(dev):
    cloud = PC.outlier_cloud(6000, 4).float()
    other = [PC.lattice_cloud(700, 8, side=16), torch.zeros(0, 3), PC.outlier_cloud(3000, 5).float()]
    alone = fps_grid_abi(dev, [cloud], [900], [11])
    assert torch.equal(alone, fps_grid_abi(dev, [cloud], [900], [11]))
    among = fps_grid_abi(dev, [other[0], other[1], cloud, other[2]], [700, 3, 900, 50], [1, 0, 11, 2])
    assert torch.equal(among[2], alone[0])
    assert_same(alone, TPS.fps_abi(dev, [cloud], [900], [11]), "against the brute-force kernel")


def test_every_block_size_and_bucket_size_gives_the_same_indices(dev):
    """rap_set_tuning keys 22 (points per bucket) and 23 (threads per block) select among three kernels and seven grids: all of them
    write the brute-force kernel's indices, on a surface-like cloud and on a shuffled grid full of ties."""
    lib = _lib.load()
    per0, _ = grid_params()
    clouds = [PC.outlier_cloud(5000, 6).float(), PC.grid_cloud(16, 16, 16, seed=4), PC.lattice_cloud(65, 9, side=16)]
    Ks, starts = [600, 4096, 65], [3, 2048, 64]
    want = TPS.fps_abi(dev, clouds, Ks, starts)
    try:
        for block in (256, 512, 1024):
            assert lib.rap_set_tuning(23, block) == 0
            for per in (1, 8, 16, 32, 48, 64, 128):
                assert lib.rap_set_tuning(22, per) == 0 and grid_params()[0] == per
                assert_same(fps_grid_abi(dev, clouds, Ks, starts), want, f"block {block}, {per} points per bucket")
        assert lib.rap_set_tuning(22, 33) == -1 and lib.rap_set_tuning(23, 128) == -1
    finally:
        assert lib.rap_set_tuning(22, per0) == 0 and lib.rap_set_tuning(23, 512) == 0


# ---------------------------------------------------------------------------------------------
# the Python layer
# ---------------------------------------------------------------------------------------------
def test_python_layer_search_grid_equals_search_brute(dev):
    from rap_amd.point_sampling import apply_batched_fps, sample_farthest_points
    lengths = [0, 65, 2, 1500]
    batch = torch.zeros(4, 1500, 3)
    batch[1, :65] = PC.lattice_cloud(65, 25, side=16); batch[2, :2] = PC.lattice_cloud(2, 22, side=16); batch[3] = PC.outlier_cloud(1500, 7).float()
    kw = dict(lengths=torch.tensor(lengths), K=torch.tensor([4, 70, 2, 300]), start_idx=torch.tensor([0, 64, 1, 1499]))
    s_b, i_b = sample_farthest_points(batch.to(dev), **kw)
    s_g, i_g = sample_farthest_points(batch.to(dev), search="grid", **kw)
    assert i_g.dtype == torch.int64 and i_g.shape == (4, 300) and torch.equal(i_g, i_b) and torch.equal(s_g, s_b)
    assert (i_g[0] == -1).all() and (i_g[1, 65:] == -1).all() and i_g[3].unique().numel() == 300
    ks = torch.tensor([1, 40, 2, 200])
    parts_b, idx_b = apply_batched_fps(batch, torch.tensor([1, 65, 2, 1500]), ks, 1234, dev)
    parts_g, idx_g = apply_batched_fps(batch, torch.tensor([1, 65, 2, 1500]), ks, 1234, dev, search="grid")
    assert torch.equal(idx_g, idx_b) and all(torch.equal(a, b) for a, b in zip(parts_g, parts_b))
    for fn in (lambda: sample_farthest_points(batch.to(dev), search="tree", **kw),
               lambda: apply_batched_fps(batch, torch.tensor([1, 65, 2, 1500]), ks, 1234, dev, search="kd")):
        with pytest.raises(ValueError, match="search must be one of"):
            fn()
