"""Guard-band test of rap_farthest_point_sampling_grid through the C ABI: indices_out between guard bytes, the workspace at exactly the
queried bytes and 0xFF-filled, a workspace one byte short refused with nothing written, null arguments refused, and a result that does
not depend on what follows the inputs.  Harness and limits: tests/test_guards_gpu.py and tests/guards.py."""
import ctypes

import numpy as np
import pytest
import torch

import test_preproc_scale_gpu as TPS
from oracle import preproc_cases as PC
from oracle import rap_oracle as O
from rap_amd import _lib
from test_guards_gpu import I32, I64, RAP_ERR_INVALID, Case, refused_call_wrote_nothing, run_both, stream

pytestmark = pytest.mark.gpu
P2 = ctypes.c_void_p


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_fps_grid_with_exact_indices_and_its_exact_workspace(lib, dev):
    lengths = [0, 1, 63, 65, 1025, 3000]
    clouds = [PC.lattice_cloud(n, 20 + i, side=16).float() if n else torch.zeros(0, 3) for i, n in enumerate(lengths)]
    clouds[5][1500, 2] = float("nan")                            # the last cloud takes the plain loop: its distances live in the same workspace
    Ks, starts = [3, 4, 63, 70, 40, 30], [0, 0, 5, 64, 1000, 2999]
    k_max, T, C = max(Ks), sum(lengths), len(lengths)
    pts = torch.cat(clouds)
    cloud_start = torch.tensor(np.concatenate([[0], np.cumsum(lengths)[:-1]]), dtype=I32)
    refs = [O.farthest_point_sampling(cl, n, K, st, device=dev) if n else torch.zeros(0, dtype=I64) for cl, n, K, st in zip(clouds[:5], lengths, Ks, starts)]
    brute = TPS.fps_abi(dev, clouds, Ks, starts)
    need = lib.rap_fps_grid_workspace_bytes(T, C)
    assert need >= 20 * T

    def call(c, short=0, null=None):
        idx = c.out_view(I32, (C, k_max), "indices_out")
        ws = c.out(need, name="fps grid workspace")
        args = dict(points=_lib.ptr(c.inp(pts)), cloud_start=_lib.ptr(c.inp(cloud_start)), cloud_len=_lib.ptr(c.inp(torch.tensor(lengths, dtype=I32))),
                    k_per_cloud=_lib.ptr(c.inp(torch.tensor(Ks, dtype=I32))), start_idx=_lib.ptr(c.inp(torch.tensor(starts, dtype=I32))),
                    indices_out=_lib.ptr(idx))
        if null:
            args[null] = P2(0)
        rc = lib.rap_farthest_point_sampling_grid(args["points"], T, args["cloud_start"], args["cloud_len"], args["k_per_cloud"], args["start_idx"], C,
                                                  k_max, args["indices_out"], P2(ws.ptr), need - short, stream(dev))
        torch.cuda.synchronize()
        return rc, idx

    def run(c):
        rc, idx = call(c)
        assert rc == 0
        got = idx.cpu().long()
        for i, ref in enumerate(refs):
            assert torch.equal(got[i, :ref.numel()], ref) and bool((got[i, ref.numel():] == -1).all()), i
        assert torch.equal(got, brute)
        return [idx]
    run_both(dev, run)
    refused_call_wrote_nothing(dev, call)
    for null in ("points", "cloud_start", "cloud_len", "k_per_cloud", "start_idx", "indices_out"):
        c = Case(dev, 0x00)
        rc, idx = call(c, null=null)
        assert rc == RAP_ERR_INVALID, null
        c.check()
        assert all(g.untouched() for g in c.guards if g.fill == 0xFF), null
    # no workspace at all, and bad counts
    c = Case(dev, 0x00)
    idx = c.out_view(I32, (C, k_max), "indices_out")
    one = _lib.ptr(c.inp(torch.zeros(8, dtype=I32)))
    assert lib.rap_farthest_point_sampling_grid(_lib.ptr(c.inp(pts)), T, one, one, one, one, C, k_max, _lib.ptr(idx), P2(0), need, stream(dev)) == -2
    assert lib.rap_farthest_point_sampling_grid(_lib.ptr(c.inp(pts)), T, one, one, one, one, 0, k_max, _lib.ptr(idx), P2(0), need, stream(dev)) == -1
    assert lib.rap_farthest_point_sampling_grid(_lib.ptr(c.inp(pts)), T, one, one, one, one, C, 0, _lib.ptr(idx), P2(0), need, stream(dev)) == -1
    assert lib.rap_farthest_point_sampling_grid(_lib.ptr(c.inp(pts)), -1, one, one, one, one, C, k_max, _lib.ptr(idx), P2(0), need, stream(dev)) == -1
    c.check()
    assert all(g.untouched() for g in c.guards if g.fill == 0xFF)
