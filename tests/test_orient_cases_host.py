"""CPU: what the GPU tests of the consistent normal orientation (tests/test_orient_gpu.py, tests/test_guards_orient_gpu.py) rely on,
measured from the yardstick (tests/orient_cases.py) and never from the code under test; and the argument checks and the workspace
arithmetic of rap_orient_normals, which return before any launch."""
import ctypes

import numpy as np

import orient_cases as O
from rap_amd import _lib

N, ONE = ctypes.c_void_p(0), ctypes.c_void_p(256)      # NULL; a non-NULL sentinel -- every call below fails before a pointer is used


def test_exact_inputs_are_exact_in_fp32():
    assert (O.NORMAL_SET * 4 == np.round(O.NORMAL_SET * 4)).all() and np.abs(O.NORMAL_SET).max() <= 1.5
    d = O.NORMAL_SET.astype(np.float64) @ O.NORMAL_SET.astype(np.float64).T
    assert np.array_equal(O.dot32(O.NORMAL_SET[:, None], O.NORMAL_SET[None]).astype(np.float64), d)      # every d is an fp32 number
    assert (d == 0).any() and (np.abs(d) > 1).any() and (d < 0).any()
    sizes = {}
    for name, (P, normals) in O.exact_clouds().items():
        assert P.dtype == normals.dtype == np.float32 and P.shape == normals.shape, name
        assert (P * 4 == np.round(P * 4)).all() and (normals * 4 == np.round(normals * 4)).all(), name
        assert name == "chain1000" or (np.abs(P).max() <= 64 and np.abs(normals).max() <= 1.5), name
        sizes[name] = P.shape[0]
    assert sizes == {"lattice7": 343, "lattice7_dup": 343, "line40": 40, "copies33": 33, "single": 1, "pair": 2, "cloud257": 257,
                     "cloud4099": 4099, "two_clusters": 340, "chain1000": 1000}
    assert min(sizes.values()) < min(O.KS)                               # a segment shorter than every k
    P, normals, rows = O.poisoned()
    assert (~O.vertices(P, normals)).nonzero()[0].tolist() == rows.tolist()


def test_exact_inputs_hold_ties_zero_dots_and_several_components():
    ties = zeros = 0
    components = {}
    for name, (P, normals) in O.exact_clouds().items():
        for k in O.KS:
            lo, hi, d, w = O.graph(P, normals, k)
            # edges that share their weight with the next one in the order: the row indices alone decide between them
            ties += int((w[1:] == w[:-1]).sum())
            zeros += int((d == 0).sum())
            components[name, k] = O.expected(name, k, False)[2]
    print(f"tied neighbours in the edge order {ties}, edges with d == 0 {zeros}, components {components}")
    assert ties > 1000 and zeros > 100
    assert components["two_clusters", 15] == components["two_clusters", 32] == 2
    assert components["lattice7_dup", 2] > 1 and components["cloud4099", 3] > 1 and components["lattice7", 15] == 1
    assert components["single", 2] == 1 and components["pair", 32] == 1


def test_the_chain_makes_one_hook_chain_of_its_whole_length():
    """what makes chain1000 the case for the pointer jumping: a path whose weights fall strictly, all exact in fp32"""
    P, normals = O.exact_clouds()["chain1000"]
    x, a = P[:, 0].astype(np.float64), normals[:, 0].astype(np.float64)
    assert (x.max() - x.min()) ** 2 * 16 < 2 ** 24 and a.max() ** 2 * 16 < 2 ** 24      # every d2 and every d in sixteenths, below 2^24
    lo, hi, d, w = O.graph(P, normals, 2)                               # a row's 2-list: itself and its left neighbour (row 0: its right one)
    order = np.argsort(lo)
    assert np.array_equal(lo[order], np.arange(999)) and np.array_equal(hi[order], np.arange(1, 1000))      # the path, nothing else
    assert np.array_equal(w[order].astype(np.float64), 1 - a[:-1] * a[1:]) and (np.diff(w[order]) < 0).all()
    lo3, hi3, _, _ = O.graph(P, normals, 3)                             # k = 3 adds the two end rows' second neighbours
    assert set(zip(lo3.tolist(), hi3.tolist())) == set(zip(lo.tolist(), hi.tolist())) | {(0, 2), (997, 999)}
    # so at k = 2 the lightest edge at row i is (i, i + 1) for every i < 999: 998 roots hook onto their right neighbour in round 0
    assert O.expected("chain1000", 3, False)[2] == 1 and O.expected("chain1000", 15, False)[2] == 1


def test_the_tie_break_decides_the_forest():
    """ordering tied edges by (w, hi, lo) in place of (w, lo, hi) changes signs on the exact inputs: a GPU result that ties differently
    does not pass by accident"""
    P, normals = O.exact_clouds()["lattice7"]
    want = O.expected("lattice7", 15, False)[0]
    lo, hi, d, w = O.graph(P, normals, 15)
    order = np.lexsort((-lo, -hi, w))
    parent, sign = list(range(343)), [0] * 343

    def find(x):
        s = 0
        while parent[x] != x:
            s ^= sign[x]
            x = parent[x]
        return x, s
    for a, b, dd in zip(lo[order].tolist(), hi[order].tolist(), d[order].tolist()):
        (ra, sa), (rb, sb) = find(a), find(b)
        if ra != rb:
            parent[ra], sign[ra] = rb, sa ^ sb ^ int(dd < 0)
    rel = np.asarray([find(v)[1] ^ find(0)[1] for v in range(343)])
    ref = (np.signbit(want) != np.signbit(normals)).any(axis=1).astype(int)
    assert (rel != ref ^ ref[0]).any()


def test_the_yardstick_turns_every_surface_normal_outwards():
    for name, (P, outward, components) in O.surfaces().items():
        normals = O.plane_fit_normals(P)
        mixed = ((normals * outward).sum(axis=1) > 0).mean()
        out, comp, count = O.orient(P, normals, 15)
        frac = ((out * outward).sum(axis=1) > 0).mean()
        print(f"{name}: independent rule {mixed:.3f} outwards, yardstick {frac:.3f}, components {count}, seeds {np.unique(comp).tolist()}")
        assert 0.3 < mixed < 0.7 and frac == 1.0 and count == components, name
        assert np.array_equal(np.abs(out), np.abs(normals))
    assert np.unique(O.orient(O.surfaces()["two_spheres"][0], O.plane_fit_normals(O.surfaces()["two_spheres"][0]), 15)[1]).tolist() == [0, 500]


# ---- the entry point, without a GPU ----------------------------------------------------------------------------------------------------
def orient_call(lib, **kw):
    a = dict(P=ONE, seg=ONE, K=2, n=1000, k=15, vp=N, normals=ONE, comp=N, ws=ONE, wsb=1 << 30)
    a.update(kw)
    return lib.rap_orient_normals(a["P"], a["seg"], a["K"], a["n"], a["k"], a["vp"], a["normals"], a["comp"], a["ws"], a["wsb"], N)


def test_rap_orient_normals_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    for name in ("P", "seg", "normals"):
        assert orient_call(lib, **{name: N}) == -1, name
    for bad in (dict(k=1), dict(k=33), dict(k=0), dict(k=-3), dict(K=0), dict(K=65536), dict(n=0), dict(n=1 << 31)):
        assert orient_call(lib, **bad) == -1, bad
    need = lib.rap_orient_normals_workspace_bytes(1000, 2)
    assert orient_call(lib, ws=N) == -2 and orient_call(lib, wsb=need - 1) == -2 and orient_call(lib, wsb=0) == -2


def up(n):
    return -(-n // 256) * 256


def test_workspace_query_is_host_arithmetic_on_top_of_the_normal_estimation():
    lib = _lib.load()
    q = lib.rap_orient_normals_workspace_bytes
    assert q(0, 1) == 0 and q(9, 0) == 0 and q(-1, 3) == 0
    for n, K in ((1, 1), (300, 2), (20_000, 6), (200_000, 1)):
        forest = 2 * up(n * 32 * 4) + 4 * up(n * 4) + 2 * up(n * 8) + up(33 * 32 * 4)      # lists, weights; count, lab, ptr, besthi; best, seed; flags
        assert q(n, K) == lib.rap_normals_grid_workspace_bytes(n, K) + forest, (n, K)
