"""Guard-band test of rap_orient_normals through the C ABI: normals and component_out sized exactly between guard bytes, the workspace at
exactly rap_orient_normals_workspace_bytes and 0xFF-filled, a short workspace refused without a byte written, the result independent of
what lies beyond the inputs and of the workspace's prior contents.  Harness and limits: tests/test_guards_gpu.py and tests/guards.py (an
overrun longer than the pad and a read that reaches no result are not seen)."""
import ctypes

import numpy as np
import pytest
import torch

import orient_cases as O
from rap_amd import _lib
from test_guards_gpu import F32, I32, refused_call_wrote_nothing, run_both, stream
from test_orient_gpu import assert_same, bits, cloud

pytestmark = pytest.mark.gpu

P2 = ctypes.c_void_p
ORDER = ("cloud257", "single", "line40", "two_clusters", "poisoned", "lattice7_dup")      # the array begins and ends with a segment


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.mark.parametrize("k", [2, 15, 32])
def test_orient_normals_writes_only_the_rows_of_its_segments_and_its_exact_workspace(lib, dev, k):
    starts, at = {}, 0
    for name in ORDER:
        starts[name] = at
        at += cloud(name)[0].shape[0] + (3 if name != ORDER[-1] else 0)
    N, K = at, len(ORDER)
    Pn = np.full((N, 3), np.nan, np.float32)
    covered = np.zeros(N, bool)
    for name in ORDER:
        s, n = starts[name], cloud(name)[0].shape[0]
        Pn[s:s + n] = cloud(name)[0]
        covered[s:s + n] = True
    Pt, seg = torch.from_numpy(Pn), torch.tensor([(starts[name], cloud(name)[0].shape[0]) for name in ORDER], dtype=I32)
    vp = torch.tensor([O.VIEWPOINT] * K, dtype=F32)
    need = lib.rap_orient_normals_workspace_bytes(N, K)
    assert need > lib.rap_normals_grid_workspace_bytes(N, K) > 0

    def call(c, short=0, ws_fill=None):
        nrm, comp = c.out_view(F32, (N, 3), "normals"), c.out_view(I32, (N,), "component_out")
        ws = c.out(need, name="orient workspace")
        if not short:                                                    # normals are in and out: the rows of the segments hold the input
            for name in ORDER:
                nrm[starts[name]:starts[name] + cloud(name)[0].shape[0]] = torch.from_numpy(cloud(name)[1]).to(dev)
        if ws_fill is not None:
            ws.interior.fill_(ws_fill)
        rc = lib.rap_orient_normals(_lib.ptr(c.inp(Pt)), _lib.ptr(c.inp(seg)), K, N, k, _lib.ptr(c.inp(vp)), _lib.ptr(nrm), _lib.ptr(comp),
                                    P2(ws.ptr), need - short, stream(dev))
        torch.cuda.synchronize()
        return rc, nrm, comp

    def run_with(ws_fill):
        def run(c):
            rc, nrm, comp = call(c, ws_fill=ws_fill)
            assert rc == 0
            n_, c_ = nrm.cpu().numpy(), comp.cpu().numpy()
            for name in ORDER:
                s, n = starts[name], cloud(name)[0].shape[0]
                assert_same(n_[s:s + n], c_[s:s + n], O.expected(name, k, True), (name, k), start=s)
            assert (bits(n_)[~covered] == 0xFFFFFFFF).all() and (c_[~covered] == -1).all()      # the 0xFF fill: never written
            in_segment_no_vertex = covered & (c_ == -1)
            assert in_segment_no_vertex.sum() == len(O.poisoned()[2])
            return [nrm, comp]
        return run
    run_both(dev, run_with(None))
    run_both(dev, run_with(0x00))                                        # the workspace's prior contents do not matter
    refused_call_wrote_nothing(dev, call)
