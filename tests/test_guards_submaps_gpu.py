"""Guard-band tests of rap_deskew, rap_fuse_frames, rap_submap_overlap and rap_submap_groups_connected through the C ABI: outputs sized
exactly, the workspace at exactly the queried bytes, a short workspace refused without a byte written, and results independent of what
lies beyond the inputs.  Harness and limits: tests/test_guards_gpu.py and tests/guards.py (an overrun longer than the pad and a read that
reaches no result are not seen).  The same refusals without a GPU: tests/test_submaps_host.py."""
import ctypes

import numpy as np
import pytest
import torch

import submap_oracle as O
from submap_oracle import DESKEW_TOL, ulps
from rap_amd import _lib
from test_guards_gpu import F32, I32, I64, U8, refused_call_wrote_nothing, run_both, stream

pytestmark = pytest.mark.gpu

P2 = ctypes.c_void_p
F64 = torch.float64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype)


def test_deskew_writes_only_its_rows_and_its_exact_workspace(lib, dev):
    P, ts, cu, rel, _ = O.deskew_case()                      # the last frame ends exactly at the end of the arrays
    deskew_guard(lib, dev, P, ts, cu, rel)


def test_deskew_with_thousands_of_frames_writes_only_its_rows_and_its_exact_workspace(lib, dev):
    c = O.scale_frames_case(4099)                            # table copies of 16 KiB and 32 KiB: far larger than the carver's alignment
    deskew_guard(lib, dev, c["points"], c["ts"], c["cu"], c["rel_pose"])


def deskew_guard(lib, dev, P, ts, cu, rel):
    N, F = P.shape[0], len(cu) - 1
    want = O.deskew_packed(P, ts, cu, rel, 0.0)
    scale = O.deskew_scale(P, cu, rel)
    need = lib.rap_deskew_workspace_bytes(N, F)
    assert need > 0

    def call(c, short=0):
        out = c.out_view(F32, (N, 3), "out")
        ws = c.out(need, name="deskew workspace")
        rc = lib.rap_deskew(_lib.ptr(c.inp(t(P))), _lib.ptr(c.inp(t(ts))), _lib.ptr(c.inp(t(cu, I32))), F, N, _lib.ptr(c.inp(t(rel, F64))), 0.0,
                            _lib.ptr(out), None, P2(ws.ptr), need - short, stream(dev))
        torch.cuda.synchronize()
        return rc, out

    def run(c):
        rc, out = call(c)
        assert rc == 0
        assert (np.abs(out.double().cpu().numpy() - want).max(axis=1) / scale).max() <= DESKEW_TOL
        return [out]
    run_both(dev, run)
    refused_call_wrote_nothing(dev, call)


@pytest.mark.parametrize("with_normals", [True, False], ids=["normals", "points_only"])
def test_fuse_frames_writes_only_its_rows_and_its_exact_workspace(lib, dev, with_normals):
    P, nrm, cu, pose = O.fuse_case()
    N, F = P.shape[0], len(cu) - 1
    origin = np.array(O.FUSE_FAR)
    want, want_n = O.fuse_packed(P, cu, pose, nrm, origin)
    need = lib.rap_fuse_frames_workspace_bytes(N, F)
    assert need > 0

    def call(c, short=0):
        world = c.out_view(F32, (N, 3), "world")
        wn = c.out_view(F32, (N, 3), "world_normals") if with_normals else None
        ws = c.out(need, name="fuse workspace")
        rc = lib.rap_fuse_frames(_lib.ptr(c.inp(t(P))), _lib.ptr(c.inp(t(nrm)) if with_normals else None), _lib.ptr(c.inp(t(cu, I32))), F, N,
                                 _lib.ptr(c.inp(t(pose, F64))), _lib.ptr(c.inp(t(origin, F64))), _lib.ptr(world), _lib.ptr(wn), None, P2(ws.ptr),
                                 need - short, stream(dev))
        torch.cuda.synchronize()
        return rc, world, wn

    def run(c):
        rc, world, wn = call(c)
        assert rc == 0 and ulps(world.cpu().numpy(), want) <= 1
        if with_normals:
            assert np.abs(wn.double().cpu().numpy() - want_n).max() <= 2e-6
        return [world, wn] if with_normals else [world]
    run_both(dev, run)
    refused_call_wrote_nothing(dev, call)


@pytest.mark.parametrize("name", ["counts_posed", "edge", "three", "scale_257"])
def test_submap_overlap_writes_only_its_matrix_and_its_exact_workspace(lib, dev, name):
    c0 = O.overlap_scale_case(257) if name == "scale_257" else O.overlap_case(name)      # S = 257: tables of more than 256 entries
    N, F, S = c0["points"].shape[0], len(c0["cu"]) - 1, len(c0["submap_frames"]) - 1
    want, want_n = O.overlap_matrix(O.case_world(c0), c0["voxel_size"])
    need = lib.rap_submap_overlap_workspace_bytes(N, F, S)
    assert need > 0

    def call(c, short=0):
        ratio, nv = c.out_view(F64, (S, S), "ratio"), c.out_view(I64, (S,), "n_voxels")
        ws = c.out(need, name="overlap workspace")
        pose = c.inp(t(c0["pose"], F64)) if c0["pose"] is not None else None
        rc = lib.rap_submap_overlap(_lib.ptr(c.inp(t(c0["points"]))), _lib.ptr(c.inp(t(c0["cu"], I32))), F, N, _lib.ptr(pose),
                                    _lib.ptr(c.inp(t(c0["submap_frames"], I32))), S, float(c0["voxel_size"]), _lib.ptr(ratio), _lib.ptr(nv), None,
                                    P2(ws.ptr), need - short, stream(dev))
        torch.cuda.synchronize()
        return rc, ratio, nv

    def run(c):
        rc, ratio, nv = call(c)
        assert rc == 0 and np.array_equal(ratio.cpu().numpy(), want) and np.array_equal(nv.cpu().numpy(), want_n)
        return [ratio, nv]
    run_both(dev, run)
    refused_call_wrote_nothing(dev, call)


def test_groups_connected_writes_only_its_verdicts(lib, dev):
    ratio, groups, lo, hi = O.connectivity_case()
    G, S, n_max = len(groups), ratio.shape[0], 64
    table = np.zeros((G, n_max), np.int32)
    for k, m in enumerate(groups):
        table[k, :len(m)] = m
    glen = np.array([len(m) for m in groups], np.int32)
    want = [int(O.groups_connected(ratio, g, lo, hi)) for g in groups]

    def run(c):
        out = c.out_view(U8, (G,), "connected")
        rc = lib.rap_submap_groups_connected(_lib.ptr(c.inp(t(ratio, F64))), S, _lib.ptr(c.inp(t(table))), _lib.ptr(c.inp(t(glen))), G, n_max, lo, hi,
                                             _lib.ptr(out), None, stream(dev))
        torch.cuda.synchronize()
        assert rc == 0 and list(out.cpu().numpy()) == want
        return [out]
    run_both(dev, run)
    # the last group full to the row's end (64 members end exactly at the end of the table): the permuted chain moved last
    order = [k for k in range(G) if len(groups[k]) < 64] + [k for k in range(G) if len(groups[k]) == 64]
    table2, glen2, want2 = table[order], glen[order], [want[k] for k in order]

    def run2(c):
        out = c.out_view(U8, (G,), "connected")
        rc = lib.rap_submap_groups_connected(_lib.ptr(c.inp(t(ratio, F64))), S, _lib.ptr(c.inp(t(table2))), _lib.ptr(c.inp(t(glen2))), G, n_max, lo, hi,
                                             _lib.ptr(out), None, stream(dev))
        torch.cuda.synchronize()
        assert rc == 0 and list(out.cpu().numpy()) == want2
        return [out]
    run_both(dev, run2)
