"""GPU: edge cases of voxel down-sampling and the coverage count, on both device paths -- the dense key table (voxel.hip) and the radix
sort (voxel_sort.hip) -- against the oracle: a bit-exact index list, and the number of distinct rows of floor(p / voxel_size).
Inputs: tests/caller_edge_cases.py::voxel_cases (checked by tests/test_caller_edge_cases_host.py): a grid of one voxel (every key 0), the
2 x 2 x 2 grid whose cubic key folds eight cells onto four, a cloud of voxel centres only (largest distance 0: every level equal, the
lowest index wins), points on voxel faces with both signs and one fp32 step either side, tables of 3616 and 4369 slots (one compaction
block of 4096, and a second, partial one) with the first and the last slot occupied, 255 / 256 / 257 points, a voxel holding a run of
10 000 identical points (equal composite keys: the sorted path rests on the sort being stable), and the empty cloud."""
import numpy as np
import pytest
import torch

import caller_edge_cases as C
from oracle import rap_oracle as O
from rap_amd.point_sampling import calculate_voxel_coverage, remove_statistical_outlier, voxel_down_sample_torch

pytestmark = pytest.mark.gpu

CASES = sorted(C.voxel_cases())


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", CASES)
def test_voxel_downsample_and_coverage_edges(dev, name):
    p, vs = C.voxel_cases()[name]
    with np.errstate(invalid="ignore"):                                   # all centres: the reference's level is 0 / 0 for every point
        want = O.voxel_down_sample(p, vs)
    distinct = len(np.unique(np.floor(p / np.float32(vs)).astype(np.int64), axis=0))
    assert distinct == O.calculate_voxel_coverage(p, vs)
    pts = torch.from_numpy(p).to(dev)
    for path in ("dense", "sorted"):
        idx = voxel_down_sample_torch(pts, vs, path=path)
        assert idx.dtype == torch.int64 and idx.device == pts.device
        assert np.array_equal(idx.cpu().numpy(), want), (name, path)
        assert calculate_voxel_coverage(pts, vs, path=path) == distinct, (name, path)
    assert np.array_equal(voxel_down_sample_torch(pts, vs).cpu().numpy(), want)          # the wrapper's own choice of path


def test_empty_cloud(dev):
    """An empty cloud gives an empty index list (the entry points refuse N = 0; the wrapper used to pass it on and raise), coverage 0 and
    an empty outlier result."""
    empty = torch.zeros(0, 3, device=dev)
    for path in (None, "dense", "sorted"):
        idx = voxel_down_sample_torch(empty, 0.25, path=path)
        assert idx.shape == (0,) and idx.dtype == torch.int64 and idx.device == empty.device
        assert calculate_voxel_coverage(empty, 0.25, path=path) == 0
    kept, kidx = remove_statistical_outlier(empty)
    assert kept.shape == (0, 3) and kidx.shape == (0,) and kidx.dtype == torch.int64 and kidx.device == empty.device
