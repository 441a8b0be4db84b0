"""CPU: the workspace queries of the nearest-neighbour, ICP and attention entry points are host arithmetic, and their values are pinned.

A caller sizes one allocation from these numbers, so a refactor of the carve code must not move them.  The expected values were recorded
from the library before the search and ICP code was folded (nn_tile.h, one carve function for the four ICP forms); the attention sizes
are written out as the formulas of their layout, which held before the attention carve was moved onto Carver."""
import pytest

from rap_amd import _lib

# argument sets: (points, problems / samples, parts); NY = NX where a query takes both
SETS = [(1, 1, 1), (257, 3, 3), (4099, 300, 6)]
# query -> (its arguments: n = points, k = problems, p = parts; the recorded bytes for SETS; the lowest value that is NOT refused)
QUERIES = {
    "rap_icp_workspace_bytes": ("nk", [1536, 1792, 64768], 1),
    "rap_icp_grid_workspace_bytes": ("nnk", [3328, 10752, 228608], 1),
    "rap_icp_plane_workspace_bytes": ("nk", [1792, 2816, 121600], 1),
    "rap_icp_plane_grid_workspace_bytes": ("nnk", [3584, 11776, 285440], 1),
    "rap_nn_grid_workspace_bytes": ("nnk", [2048, 9216, 174080], 1),
    "rap_normals_workspace_bytes": ("nk", [512, 512, 11520], 1),
    "rap_nn_metrics_workspace_bytes": ("nk", [1024, 4096, 60160], 0),
    "rap_pair_metrics_workspace_bytes": ("nk", [768, 768, 20224], 0),
    "rap_part_acc_workspace_bytes": ("nkp", [1792, 8192, 285184], 0),
}


def _args(sig, n, k, p):
    return {"nk": (n, k), "nnk": (n, n, k), "nkp": (n, k, p)}[sig]


@pytest.mark.parametrize("name", sorted(QUERIES))
def test_workspace_bytes_are_what_they_were(name):
    sig, expected, _ = QUERIES[name]
    q = getattr(_lib.load(), name)
    assert [q(*_args(sig, *s)) for s in SETS] == expected


@pytest.mark.parametrize("name", sorted(QUERIES))
def test_refused_arguments_give_zero(name):
    """every argument, one at a time: below the query's lowest accepted value (1, or 0 for the entries that take an empty batch) -> 0"""
    sig, _, lowest = QUERIES[name]
    q = getattr(_lib.load(), name)
    for pos in range(len(sig)):
        for bad in range(-2, lowest):
            a = list(_args(sig, 257, 3, 3))
            a[pos] = bad
            assert q(*a) == 0, (name, a)
        a = list(_args(sig, 257, 3, 3))
        a[pos] = lowest
        assert q(*a) > 0, (name, a)


# ---- the kernel-level attention workspaces: [work items | sanitised cu_seqlens | partial O planes | (m, l) plane], every piece 256-aligned
ATTN_TP = [0, 1, 63, 64, 65, 255, 256, 4097, 262144]
ATTN_NSEG = [0, 1, 63, 64, 65535]


def _up256(n):
    return (n + 255) // 256 * 256


def _attn_tables(TP, nseg):
    return _up256((TP // 64 + nseg + 1) * 16) + _up256((nseg + 1) * 4)


def test_attention_workspace_bytes():
    q = _lib.load().rap_attention_workspace_bytes
    for TP in ATTN_TP:
        for nseg in ATTN_NSEG:
            assert q(TP, nseg) == _attn_tables(TP, nseg), (TP, nseg)


@pytest.mark.parametrize("splits", [1, 2, 4])
def test_attention_split_workspace_bytes(splits):
    q = _lib.load().rap_attention_split_workspace_bytes
    for TP in ATTN_TP:
        for nseg in ATTN_NSEG:
            for heads in (1, 8, 16):
                planes = splits * TP * heads * 256 + _up256(splits * TP * heads * 8) if splits > 1 else 0
                assert q(TP, nseg, heads, splits) == _attn_tables(TP, nseg) + planes, (TP, nseg, heads, splits)


def test_attention_split_workspace_refusals_give_zero():
    q = _lib.load().rap_attention_split_workspace_bytes
    assert q(4097, 63, 8, 2) > 0
    for heads in (0, -1):
        assert q(4097, 63, heads, 2) == 0
    for splits in (0, 3, 5):
        assert q(4097, 63, 8, splits) == 0
    assert q(-1, 63, 8, 2) == 0 and q(4097, -1, 8, 2) == 0 and q(-1, 63, 8, 1) == 0 and q(4097, -1, 8, 1) == 0
