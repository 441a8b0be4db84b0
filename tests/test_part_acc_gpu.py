"""GPU: rap_amd.metrics.compute_part_acc / rap_part_acc against the reference's fixture, a float64 oracle and the Python transcription of
SciPy's assignment (tests/part_acc_oracle.py; tests/test_part_acc_host.py holds that transcription to SciPy on the build machine).

  test_fixture ........................ tests/golden/part_acc.npz (the reference's own compute_part_acc with SciPy): (B,N,3) and packed input
  test_chamfer_edges .................. part_nn_kernel / part_cd_kernel: part boundaries on, before and after an LDS tile edge, partial
                                        query tiles, a part over three tiles, empty parts first / inside / last, B = 3 with different
                                        n_parts, a sample of empty parts only, more work items than one round of the grid
  test_assignment_at_full_width ....... part_assign_kernel: n = 1, 2, 63, 64, 65, 256 on an exact lattice
  test_matching_feeds_transform_errors  the matched_part_ids of the new call make compute_transform_errors_direct right
  test_two_runs_are_bitwise_equal
  test_guard_bands .................... through the C ABI: outputs and an exact 0xFF workspace between guard bytes, inputs between 0x00 / 0xFF
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import guards as G
import part_acc_oracle as O
from conftest import ROOT
from rap_amd import _lib, metrics

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def expected(kind, key):
    """-> (case, cd64, part_acc, matched): computed once, shared, never modified"""
    c = O.edge_case(key) if kind == "edge" else O.lattice_case(key, seed=key) if kind == "lattice" else O.interchangeable_case()[0]
    cd = O.chamfer_matrix(c["gt"], c["pred"], c["ppp"], c["cu"])
    acc, matched = O.part_acc_from_cd(cd, c["ppp"], c["threshold"])
    return c, cd, acc, matched


def run_packed(dev, c, **kw):
    t = lambda a: torch.from_numpy(a).to(dev)
    out = metrics.compute_part_acc(t(c["gt"]), t(c["pred"]), t(c["ppp"]), threshold=c["threshold"], cu_seqlens_batch=t(c["cu"]),
                                   return_cd_matrix=True, **kw)
    return tuple(o.cpu().numpy() for o in out)


def same_float_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32)) or \
        (np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.nan_to_num(a), np.nan_to_num(b)))


def check_against(c, got, cd64, acc_ref, matched_ref, tag):
    acc, matched, cd = got
    ok, worst = O.cd_within_bound(cd, cd64)
    print(f"{tag}: worst |cd - cd64| / (2^-24 cd64) = {worst:.3f} (bound {O.CD_REL_BOUND / O.U32:.0f})")
    assert ok, (tag, worst)
    assert cd.dtype == np.float32 and acc.dtype == np.float32 and matched.dtype == np.int64
    assert np.array_equal(matched, matched_ref), tag
    assert same_float_bits(acc, acc_ref), (tag, acc, acc_ref)


def test_fixture(dev):
    z = np.load(os.path.join(ROOT, "tests", "golden", "part_acc.npz"))
    gt, pred, ppp, thr = z["pointclouds_gt"], z["pointclouds_pred"], z["points_per_part"], float(z["threshold"])
    B, N = gt.shape[:2]
    t = lambda a: torch.from_numpy(a).to(dev)
    # (B,N,3), the reference's signature and return structure
    acc, matched = metrics.compute_part_acc(t(gt), t(pred), t(ppp), thr)
    assert acc.shape == (B,) and matched.shape == ppp.shape and acc.is_cuda and matched.dtype == torch.int64
    only = metrics.compute_part_acc(t(gt), t(pred), t(ppp), thr, return_matched_part_ids=False)
    assert torch.is_tensor(only) and torch.equal(only, acc)
    acc3, matched3, cd3 = metrics.compute_part_acc(t(gt), t(pred), t(ppp), thr, True, return_cd_matrix=True)
    c = dict(gt=gt.reshape(-1, 3), pred=pred.reshape(-1, 3), ppp=ppp, cu=(np.arange(B + 1) * N).astype(np.int32), threshold=thr)
    packed = run_packed(dev, c)
    for tag, got in (("(B,N,3)", (acc3.cpu().numpy(), matched3.cpu().numpy(), cd3.cpu().numpy())), ("packed", packed)):
        check_against(c, got, z["cd"], z["part_acc"], z["matched_part_ids"], f"fixture {tag}")
    assert np.array_equal(acc.cpu().numpy(), z["part_acc"]) and np.array_equal(matched.cpu().numpy(), z["matched_part_ids"])
    assert same_float_bits(packed[2], cd3.cpu().numpy())


@pytest.mark.parametrize("name", O.EDGE_NAMES)
def test_chamfer_edges(dev, name):
    c, cd64, acc_ref, matched_ref = expected("edge", name)
    got = run_packed(dev, c)
    check_against(c, got, cd64, acc_ref, matched_ref, name)
    empty_samples = (c["ppp"] > 0).sum(axis=1) == 0
    assert np.isnan(got[0][empty_samples]).all() and not np.isnan(got[0][~empty_samples]).any()
    assert (got[1][empty_samples] == 0).all()
    if name == "all-empty-sample":
        assert empty_samples.tolist() == [False, True, False]


@pytest.mark.parametrize("n", O.LATTICE_SIZES)
def test_assignment_at_full_width(dev, n):
    c, cd64, acc_ref, matched_ref = expected("lattice", n)
    acc, matched, cd = run_packed(dev, c)
    assert np.array_equal(cd.astype(np.float64), cd64)                   # lattice coordinates: every distance is exact in fp32
    assert np.array_equal(matched, matched_ref), n
    assert same_float_bits(acc, acc_ref)
    assert sorted(matched[0].tolist()) == list(range(n))                 # a permutation
    if n == 256:
        assert 0.5 < float(acc[0]) < 1.0 and not np.array_equal(matched[0], np.arange(n))


def direct_errors_f64(Rg, tg, Rp, tp, matched):
    """compute_transform_errors_direct (eval/metrics.py:305-383) in float64, every part non-empty"""
    if matched is not None:
        bi = np.arange(Rg.shape[0])[:, None]
        Rp, tp = Rp[bi, matched], tp[bi, matched]
    tr = np.einsum("bpij,bpij->bp", Rg.astype(np.float64), Rp.astype(np.float64))
    rot = np.degrees(np.arccos(np.clip(0.5 * (tr - 1), -1, 1)))
    trans = np.linalg.norm(tp.astype(np.float64) - tg.astype(np.float64), axis=-1)
    return rot.mean(axis=1), trans.mean(axis=1), rot, trans


def ulp32(x):
    return np.spacing(np.maximum(np.abs(np.asarray(x, dtype=np.float64)), 2.0 ** -126).astype(np.float32)).astype(np.float64)


def test_matching_feeds_transform_errors(dev):
    """interchangeable parts placed at one another's ground-truth poses: without a matching compute_transform_errors_direct reports the
    permutation as error; with the matched_part_ids of compute_part_acc it reports what the float64 restatement reports, within the
    2 fp32 ulp tests/test_boundary_edges_gpu.py holds that function to (boundary_cases.TE_DIRECT_ULPS)"""
    c, Rg, tg, Rp, tp, perms = O.interchangeable_case()
    _, cd64, acc_ref, matched_ref = expected("inter", 0)
    t = lambda a: torch.from_numpy(a).to(dev)
    acc, matched = metrics.compute_part_acc(t(c["gt"]), t(c["pred"]), t(c["ppp"]), c["threshold"], cu_seqlens_batch=t(c["cu"]))
    assert np.array_equal(matched.cpu().numpy(), matched_ref) and (acc.cpu().numpy() == 1.0).all()
    for b in range(perms.shape[0]):                                      # gt part perm[k] is matched to pred part k
        assert np.array_equal(matched_ref[b][perms[b]], np.arange(perms.shape[1]))
    plain = metrics.compute_transform_errors_direct(t(Rg), t(tg), t(Rp), t(tp), t(c["ppp"]))
    assert float(plain[0].min()) > 30.0 and float(plain[1].min()) > 1.0
    got = metrics.compute_transform_errors_direct(t(Rg), t(tg), t(Rp), t(tp), t(c["ppp"]), matched_part_ids=matched, return_per_part=True)
    ref = direct_errors_f64(Rg, tg, Rp, tp, matched_ref)
    for g, r in zip(got, ref):
        g = g.cpu().double().numpy()
        assert (np.abs(g - r) <= 2.0 * ulp32(r)).all(), (g, r)
    assert float(got[0].max()) < 0.1 and float(got[1].max()) < 1e-6


def test_two_runs_are_bitwise_equal(dev):
    for kind, key in (("edge", "three-tiles"), ("edge", "mixed-batch"), ("lattice", 256)):
        c = expected(kind, key)[0]
        a = run_packed(dev, c)
        with torch.inference_mode():                                     # (the shared scratch may have been allocated under inference mode)
            metrics.workspace(dev, 1).fill_(0x5A)                        # the scratch of the first run does not reach the second
        b = run_packed(dev, c)
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (kind, key)


def test_guard_bands(dev):
    """One C-ABI call per input-pad content: every output inside a Guarded (0xFF interior, 0xA5 pads), the workspace a Guarded of exactly
    rap_part_acc_workspace_bytes filled with 0xFF, the inputs between 0x00 and then 0xFF.  Results equal the wrapper's; cd = NULL works;
    a workspace one byte short is refused and nothing is written."""
    lib = _lib.load()
    c, cd64, acc_ref, matched_ref = expected("edge", "empties")
    B, P = c["ppp"].shape
    TP = c["gt"].shape[0]
    need = lib.rap_part_acc_workspace_bytes(TP, B, P)
    assert need > 0
    want = run_packed(dev, c)

    def call(pad, with_cd=True, short=0):
        ins = [G.guarded_like(torch.from_numpy(c[k]), dev, guard=pad, name=k) for k in ("gt", "pred", "ppp", "cu")]
        acc, matched = G.Guarded(B * 4, dev, name="part_acc"), G.Guarded(B * P * 8, dev, name="matched")
        cd, ws = G.Guarded(B * P * P * 4, dev, pitch=P * 4, name="cd"), G.Guarded(need, dev, name="workspace")
        rc = lib.rap_part_acc(*(_lib.ptr(v) for _, v in ins), B, P, TP, c["threshold"], ctypes.c_void_p(acc.ptr), ctypes.c_void_p(matched.ptr),
                              ctypes.c_void_p(cd.ptr) if with_cd else None, ctypes.c_void_p(ws.ptr), need - short, _lib.current_stream(dev))
        torch.cuda.synchronize()
        for g in [g for g, _ in ins] + [acc, matched, cd, ws]:
            g.check()
        return rc, acc, matched, cd, ws

    for pad in (0x00, 0xFF):
        rc, acc, matched, cd, ws = call(pad)
        assert rc == 0
        got = (acc.view(torch.float32, (B,)).cpu().numpy(), matched.view(torch.int64, (B, P)).cpu().numpy(),
               cd.view(torch.float32, (B, P, P)).cpu().numpy())
        for x, y in zip(got, want):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
        check_against(c, got, cd64, acc_ref, matched_ref, f"guarded, pads {pad:#04x}")
    rc, acc, matched, cd, ws = call(0x00, with_cd=False)
    assert rc == 0 and cd.untouched()
    assert np.array_equal(matched.view(torch.int64, (B, P)).cpu().numpy(), want[1])
    rc, acc, matched, cd, ws = call(0x00, short=1)
    assert rc == -2 and acc.untouched() and matched.untouched() and cd.untouched() and ws.untouched()
