"""The consistent normal orientation on the device (rap_amd/csrc/orient.hip) against the yardstick of tests/orient_cases.py.

rap_orient_normals is compared EXACTLY (sign pattern, untouched magnitude bits, component_out) on inputs whose distances, dot products
and weights are exact in fp32, so that the result is a matter of the (w, lo, hi) order, the parity and the seed rule alone
(tests/test_orient_cases_host.py proves from the yardstick that these inputs hold ties, zero dot products, several components and
segments shorter than k).  On a sphere, a torus and two spheres the property itself is tested: after
estimate_normals_packed(..., orientation="consistent") every normal points outwards, which the independent rule does not give."""

import numpy as np
import pytest
import torch

import orient_cases as O
from rap_amd import _lib, estimate_normals_packed, estimate_point_normals, orient_normals_packed

pytestmark = pytest.mark.gpu

I32, F32, U8 = torch.int32, torch.float32, torch.uint8
NAMES = tuple(O.exact_clouds()) + ("poisoned",)
COMP_FILL = 0x5A5A5A5A                                                   # component_out before a call: not -1, not a row


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def cloud(name):
    return O.poisoned()[:2] if name == "poisoned" else O.exact_clouds()[name]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def call(lib, dev, P, normals, rows, k, viewpoint=None, ws_fill=0xFF, over=()):
    """one call through the C ABI -> (rc, normals (N,3) fp32 numpy, component_out (N,) int32 numpy, the tensors of the call)"""
    N, K = P.shape[0], len(rows)
    a = dict(P=torch.from_numpy(P).to(dev), seg=torch.tensor(rows, dtype=I32, device=dev), normals=torch.from_numpy(normals).to(dev).clone(),
             comp=torch.full((N,), COMP_FILL, dtype=I32, device=dev), k=k,
             vp=None if viewpoint is None else torch.tensor([viewpoint] * K, dtype=F32, device=dev))
    need = lib.rap_orient_normals_workspace_bytes(N, K)
    a["ws"] = torch.full((need,), ws_fill, dtype=U8, device=dev)
    a["ws_bytes"] = need
    a.update(dict(over))                                               # arguments replaced for this call (None: NULL)
    rc = lib.rap_orient_normals(_lib.ptr(a["P"]), _lib.ptr(a["seg"]), K, N, a["k"], _lib.ptr(a["vp"]), _lib.ptr(a["normals"]), _lib.ptr(a["comp"]),
                                _lib.ptr(a["ws"]), a["ws_bytes"], _lib.current_stream(dev))
    torch.cuda.synchronize()
    return rc, None if a["normals"] is None else a["normals"].cpu().numpy(), None if a["comp"] is None else a["comp"].cpu().numpy(), a


def assert_same(got_normals, got_comp, want, what, start=0):
    want_normals, want_comp, _ = want
    flipped = bits(got_normals) ^ bits(want_normals)
    assert not flipped.any(), f"{what}: {int(flipped.any(axis=1).sum())} rows differ from the yardstick (first {int(flipped.any(axis=1).argmax())})"
    want_comp = np.where(want_comp >= 0, want_comp + start, -1)
    assert np.array_equal(got_comp, want_comp), f"{what}: component_out differs in {int((got_comp != want_comp).sum())} rows"


@pytest.mark.parametrize("k", O.KS)
@pytest.mark.parametrize("name", NAMES)
def test_orient_normals_equals_the_yardstick_exactly(lib, dev, name, k):
    P, normals = cloud(name)
    for vp in (None, O.VIEWPOINT):
        want = O.expected(name, k, vp is not None)
        rc, out, comp, _ = call(lib, dev, P, normals, [(0, P.shape[0])], k, vp)
        assert rc == 0
        assert np.array_equal(bits(out) & 0x7fffffff, bits(normals) & 0x7fffffff), "a magnitude bit changed"
        assert_same(out, comp, want, (name, k, vp))
        rc, again, comp2, _ = call(lib, dev, P, normals, [(0, P.shape[0])], k, vp, ws_fill=0x00)
        assert rc == 0 and np.array_equal(bits(again), bits(out)) and np.array_equal(comp2, comp), "a second call gave other bits"


def packed(order):
    """the exact clouds as segments of one array, five rows of 0xFF between them, in the given table order plus an empty segment, one
    that starts beyond the array and one with a negative length"""
    starts, at = {}, 3
    for name in NAMES:
        starts[name] = at
        at += cloud(name)[0].shape[0] + 5
    P = np.full((at, 3), np.nan, np.float32).view(np.uint32)
    P[:] = 0xFFFFFFFF
    P = P.view(np.float32)
    normals = P.copy()
    for name in NAMES:
        p, n = cloud(name)
        P[starts[name]:starts[name] + p.shape[0]], normals[starts[name]:starts[name] + p.shape[0]] = p, n
    rows = [(starts[name], cloud(name)[0].shape[0]) for name in order]
    rows[2:2] = [(starts[NAMES[0]], 0), (at + 7, 10)]
    rows.append((1, -4))
    return P, normals, rows, starts


@pytest.mark.parametrize("vp", [None, O.VIEWPOINT], ids=["up", "viewpoint"])
def test_a_segment_gives_the_same_bits_alone_and_in_a_batch(lib, dev, vp):
    results = []
    for order in (NAMES, NAMES[::-1]):
        P, normals, rows, starts = packed(order)
        rc, out, comp, _ = call(lib, dev, P, normals, rows, 15, vp)
        assert rc == 0
        covered = np.zeros(P.shape[0], bool)
        for name in NAMES:
            s, n = starts[name], cloud(name)[0].shape[0]
            assert_same(out[s:s + n], comp[s:s + n], O.expected(name, 15, vp is not None), (name, "in a batch"), start=s)
            covered[s:s + n] = True
        # rows outside every segment: never written, neither the normals (still 0xFF) nor the components (still the fill)
        assert (bits(out)[~covered] == 0xFFFFFFFF).all() and (comp[~covered] == COMP_FILL).all()
        results.append((out, comp))
    assert np.array_equal(bits(results[0][0]), bits(results[1][0])) and np.array_equal(results[0][1], results[1][1])


def test_rows_that_are_no_vertices_keep_their_bits(lib, dev):
    P, normals, rows = O.poisoned()
    rc, out, comp, _ = call(lib, dev, P, normals, [(0, P.shape[0])], 15)
    assert rc == 0
    assert np.array_equal(bits(out)[rows], bits(normals)[rows]) and (comp[rows] == -1).all()
    rest = np.setdiff1d(np.arange(P.shape[0]), rows)
    assert (comp[rest] >= 0).all() and O.vertices(P, normals)[comp[rest]].all()
    rc, out2, _, _ = call(lib, dev, P, normals, [(0, P.shape[0])], 15, over=dict(comp=None))        # component_out = NULL
    assert rc == 0 and np.array_equal(bits(out2), bits(out))


def test_python_wrapper_returns_a_new_tensor_and_the_components(dev):
    P, normals = cloud("two_clusters")
    want = O.expected("two_clusters", 15, True)
    Pd, nd = torch.from_numpy(P).to(dev), torch.from_numpy(normals).to(dev)
    seg = torch.tensor([[0, P.shape[0]]], dtype=I32, device=dev)
    out, comp = orient_normals_packed(Pd, nd, seg, k=15, viewpoint=torch.tensor(O.VIEWPOINT, device=dev), return_components=True)
    assert torch.equal(nd.cpu(), torch.from_numpy(normals)) and out.data_ptr() != nd.data_ptr()
    assert_same(out.cpu().numpy(), comp.cpu().numpy(), want, "wrapper")
    assert len(np.unique(comp.cpu().numpy())) == 2
    assert torch.equal(orient_normals_packed(Pd, nd, seg, viewpoint=torch.tensor(O.VIEWPOINT, device=dev)), out)      # k = 15 is the default
    with pytest.raises(ValueError):
        orient_normals_packed(Pd, nd, seg, k=1)
    with pytest.raises(ValueError):
        orient_normals_packed(Pd, nd, seg, k=33)


# ---- surfaces: the property, through the public estimate ----------------------------------------------------------------------------
@pytest.mark.parametrize("search", ["brute", "grid"])
@pytest.mark.parametrize("name", ["sphere", "torus", "two_spheres"])
def test_consistent_orientation_turns_every_normal_of_a_closed_surface_outwards(dev, name, search):
    P, outward, components = O.surfaces()[name]
    Pd = torch.from_numpy(P).to(dev)
    seg = torch.tensor([[0, P.shape[0]]], dtype=I32, device=dev)
    outward = torch.from_numpy(outward).to(dev)
    independent = estimate_normals_packed(Pd, seg, max_nn=12, radius=None, search=search)
    frac = float(((independent.double() * outward).sum(dim=1) > 0).double().mean())
    assert 0.3 < frac < 0.7, f"{name}: the independent rule already gives {frac:.3f} outwards"
    consistent = estimate_normals_packed(Pd, seg, max_nn=12, radius=None, search=search, orientation="consistent", orient_k=15)
    agree = (consistent.double() * outward).sum(dim=1) > 0
    assert bool(agree.all()), f"{name}: {int((~agree).sum())} of {P.shape[0]} normals point inwards"
    assert torch.equal(consistent.abs(), independent.abs())
    _, comp = orient_normals_packed(Pd, independent, seg, k=15, return_components=True)
    seeds = np.unique(comp.cpu().numpy()).tolist()
    assert len(seeds) == components and (name != "two_spheres" or seeds == [0, 500]), seeds
    if name == "sphere":                                                 # the reference's signature, one cloud
        one = estimate_point_normals(Pd, k_neighbors=12, radius=None, search=search, orientation="consistent", orient_k=15)
        assert torch.equal(one, consistent)


@pytest.mark.parametrize("search", ["brute", "grid"])
def test_independent_orientation_is_the_call_without_the_argument(dev, search):
    P = torch.from_numpy(O.surfaces()["torus"][0]).to(dev)
    seg = torch.tensor([[0, 1500], [1500, 1500]], dtype=I32, device=dev)
    vp = torch.tensor([[0.0, 0.0, 9.0], [1.0, 2.0, 3.0]], device=dev)
    for kw in (dict(), dict(viewpoint=vp), dict(return_eigenvalues=True)):
        a = estimate_normals_packed(P, seg, max_nn=12, radius=0.5, search=search, **kw)
        b = estimate_normals_packed(P, seg, max_nn=12, radius=0.5, search=search, orientation="independent", **kw)
        for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
            assert torch.equal(x.view(I32), y.view(I32))
    assert torch.equal(estimate_point_normals(P, search=search).view(I32), estimate_point_normals(P, search=search, orientation="independent").view(I32))
    with pytest.raises(ValueError):
        estimate_normals_packed(P, seg, orientation="mst")


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_return_their_code_and_write_nothing(lib, dev):
    P, normals = cloud("cloud257")
    rows = [(0, 257)]
    need = lib.rap_orient_normals_workspace_bytes(257, 1)
    cases = [(dict(k=1), -1), (dict(k=33), -1), (dict(P=None), -1), (dict(seg=None), -1), (dict(normals=None), -1), (dict(ws=None), -2),
             (dict(ws_bytes=need - 1), -2)]
    for over, code in cases:
        rc, out, comp, a = call(lib, dev, P, normals, rows, 15, O.VIEWPOINT, over=over)
        assert rc == code, (over, rc)
        if a["normals"] is not None:
            assert np.array_equal(bits(out), bits(normals)), over
        assert (comp == COMP_FILL).all(), over
        if a["ws"] is not None:
            assert bool((a["ws"] == 0xFF).all()), over
