"""Inputs and float64 references that the host test (tests/test_boundary_cases_host.py) and the GPU edge file of the batch-boundary kernels
(tests/test_boundary_edges_gpu.py) share: collate (collate.hip), the output transforms and transform errors (transforms.hip,
pair_metrics.hip), generation selection (rigidity.hip) and the batch tables (sampler_kernels.hip).  Seeded, pure torch / numpy; every
builder is cached and its result is not to be modified.

No bound here is tuned to a device result.  The collate and relative-transform bounds follow from the number formats; the bounds of the
fp32 transform errors are MEASURED ON THE CPU (the committed oracle in float32 against itself in float64 on these cases) and written
down as constants below -- the host test re-derives them and asserts that the constants are not below 4x what it measures."""
import functools
import itertools

import numpy as np
import torch

from caller_edge_cases import random_rotation
from oracle import rap_oracle as O

F32_ULP = 2.0 ** -23            # spacing of fp32 numbers in [1, 2)
F32_HALF = 2.0 ** -24           # one rounding to fp32, relative


def ulp32(x):
    """spacing of the fp32 numbers at |x| (numpy float64 array) -- the ulp of the value itself, never below the smallest normal's"""
    return np.spacing(np.maximum(np.abs(np.asarray(x, dtype=np.float64)), 2.0 ** -126).astype(np.float32)).astype(np.float64)


# ---------------------------------------------------------------------------------------------
# 1. collate: rap_collate_transform
# ---------------------------------------------------------------------------------------------
# A batch is {"counts": (B,P) int64, "parts": [the (n,3) array of every NON-EMPTY part, flat order], "feats": [(n,F)] or None,
# "perms": [within-part permutation per non-empty part] or None (no order), "P", "F", "order": the kind of the permutations,
# "np_seed": the numpy seed of the kind "numpy" (the reference's own np.random.permutation draws), ...}
COLLATE_SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 4097, 70001]
COLLATE_FLOAT_KEYS = ("pointclouds", "pointclouds_gt", "rotations", "translations", "scales", "global_translation")
COLLATE_EXACT_KEYS = ("features", "part_indices", "anchor_indices", "anchor_parts", "points_per_part", "cu_seqlens")
EXTENT_PLACEMENTS = [0, 63, 64, 255, 256, -1]          # index of the extent-defining point inside the 300-point primary part (-1: n-1)
EXTENT_N = 300
PART_COUNT_SHAPES = [(1, 1), (1, 65), (2, 2), (3, 65), (64, 2), (255, 1), (255, 2), (256, 1), (256, 65)]       # (P, B)


def _cloud(rng, n, centre=(0.0, 0.0, 0.0), spread=(1.0, 0.7, 0.4), dtype=np.float64):
    return (np.asarray(centre) + rng.standard_normal((n, 3)) * np.asarray(spread)).astype(dtype)


def _perms(counts_flat, kind, rng, np_seed=0):
    ns = [int(n) for n in counts_flat if int(n) > 0]
    if kind == "none":
        return None
    if kind == "identity":
        return [np.arange(n) for n in ns]
    if kind == "reverse":
        return [np.arange(n)[::-1].copy() for n in ns]
    if kind == "random":
        return [rng.permutation(n) for n in ns]
    assert kind == "numpy"                             # what rap_amd.data.draw_part_permutations draws after np.random.seed(np_seed)
    state = np.random.get_state()
    np.random.seed(np_seed)
    out = [np.random.permutation(n) for n in ns]
    np.random.set_state(state)
    return out


def _batch(rows, P, rng, order, F, centre=None, dtype=np.float64, np_seed=0, spread=(1.0, 0.7, 0.4)):
    """rows: per sample the list of part sizes (zeros allowed anywhere), padded to P columns"""
    counts = np.zeros((len(rows), P), dtype=np.int64)
    parts, feats = [], []
    for b, row in enumerate(rows):
        assert len(row) <= P
        counts[b, :len(row)] = row
        c = (0.0, 0.0, 0.0) if centre is None else np.asarray(centre) * np.array([1.0, -0.6, 0.3]) + 3.0 * rng.standard_normal(3)
        for i, n in enumerate(row):
            if n > 0:
                parts.append(_cloud(rng, n, np.asarray(c) + 2.0 * rng.standard_normal(3), spread, dtype))
                feats.append(rng.standard_normal((n, F)).astype(np.float32))
    return {"counts": counts, "parts": parts, "feats": feats if F > 0 else None, "perms": _perms(counts.reshape(-1), order, rng, np_seed),
            "P": P, "F": F, "order": order, "np_seed": np_seed}


def as_samples(batch):
    """the batch as rap_amd.transform_and_collate takes it (the wrapper knows trailing padding only)"""
    samples, k = [], 0
    for row in batch["counts"]:
        n = int((row > 0).sum())
        assert n > 0 and bool((row[:n] > 0).all()), "the wrapper cannot express an empty part in front of a non-empty one"
        s = {"parts": [torch.from_numpy(x) for x in batch["parts"][k:k + n]]}
        if batch["feats"] is not None:
            s["features"] = [torch.from_numpy(x) for x in batch["feats"][k:k + n]]
        samples.append(s); k += n
    return samples


def flat_order(batch):
    return None if batch["perms"] is None else torch.from_numpy(np.concatenate(batch["perms"]).astype(np.int64))


def primary_of(row):
    """first arg-max of the part sizes (dataset.py:764)"""
    return int(np.argmax(np.asarray(row)))


def collate_expected(batch, flip=False):
    """O.transform_sample in float64 on the float64 upcast of the batch's own values, sample by sample on the NON-EMPTY parts, with the
    part columns mapped back (empty parts: zero rotation / translation rows, not an anchor; part_indices keep the original column); a
    sample without any point: scale 0, global translation 0, zero rows, a repeated cu_seqlens entry.  `flip`: the same computation with
    the point order of every part reversed (and the permutations adjusted so that the outputs stay in place) -- the summation order of
    every mean changes, nothing else.  -> dict of numpy arrays"""
    counts = batch["counts"]
    B, P = counts.shape
    F = batch["F"]
    out = {k: [] for k in ("pointclouds", "pointclouds_gt", "features", "part_indices", "anchor_indices")}
    tab = {"rotations": np.zeros((B, P, 3, 3), np.float32), "translations": np.zeros((B, P, 3), np.float32),
           "anchor_parts": np.zeros((B, P), bool), "scales": np.zeros(B, np.float32), "global_translation": np.zeros((B, 3), np.float32)}
    k = 0
    for b in range(B):
        cols = [p for p in range(P) if counts[b, p] > 0]
        if not cols:
            continue
        parts = [np.asarray(x, dtype=np.float64) for x in batch["parts"][k:k + len(cols)]]
        feats = [x for x in batch["feats"][k:k + len(cols)]] if F > 0 else [np.zeros((len(x), 0), np.float32) for x in parts]
        perms = [np.arange(len(x)) for x in parts] if batch["perms"] is None else batch["perms"][k:k + len(cols)]
        if flip:
            parts, feats, perms = [x[::-1] for x in parts], [x[::-1] for x in feats], [len(o) - 1 - o for o in perms]
        with np.errstate(all="ignore"):
            o = O.transform_sample(parts, feats, P, perms)
        for key in out:
            out[key].append(np.asarray(cols)[o[key]] if key == "part_indices" else o[key])
        for j, p in enumerate(cols):
            tab["rotations"][b, p], tab["translations"][b, p], tab["anchor_parts"][b, p] = o["rotations"][j], o["translations"][j], o["anchor_parts"][j]
        tab["scales"][b], tab["global_translation"][b] = o["scales"], o["global_translation"]
        k += len(cols)
    res = {key: np.concatenate(v) for key, v in out.items()}
    res.update(tab)
    res["points_per_part"] = counts.copy()
    res["cu_seqlens"] = np.concatenate([[0], np.cumsum(counts.sum(1))]).astype(np.int64)
    return res


def collate_tolerance(ref):
    """both sides round ONE float64 value to fp32 and differ only in float64 summation order: one fp32 ulp of the reference element,
    max(1, |ref|) as the floor of the magnitude (like the golden test of tests/test_kernels_gpu.py)"""
    return F32_ULP * np.maximum(1.0, np.abs(np.asarray(ref, dtype=np.float64)))


def size_rows():
    """every size of COLLATE_SIZES once as the primary and once as a non-primary part; the primary alternates between the columns"""
    S = COLLATE_SIZES
    rows = [[1, 1]]                                                    # 1 as the primary (a tie: the first wins) and as the other part
    for k in range(1, len(S) - 1):
        rows.append([S[k - 1], S[k]] if k % 2 else [S[k], S[k - 1]])
    rows.append([S[-1], S[-2], S[-1]])                                 # 70001 primary (first of a tie) and non-primary
    return rows


@functools.lru_cache(maxsize=None)
def collate_sizes_batch():
    return _batch(size_rows(), 3, np.random.default_rng(101), "random", 3)


def extent_part(rng, n, index, axis, sign):
    """n points strictly inside the cube |x| < 0.5 around their centre, one of them moved out to sign * 2 on `axis`"""
    p = rng.uniform(-0.5, 0.5, (n, 3))
    p[index] = rng.uniform(-0.2, 0.2, 3)
    p[index, axis] = sign * 2.0
    return p


@functools.lru_cache(maxsize=None)
def collate_primary_batch():
    """P = 5, the reference's own np.random.permutation draws, F = 1.  Samples 0-2: the largest part first, in the middle, last; 3-5:
    two, three parts tied for largest and a tie of the last two; 6-11: the extent-defining point at EXTENT_PLACEMENTS of the primary
    part, the axis and the sign of the extreme coordinate varying (odd samples: a NEGATIVE extreme).  -> batch + "extent": [(sample,
    index in the primary part, axis, sign)]"""
    rng = np.random.default_rng(202)
    rows = [[300, 100, 120], [100, 300, 120, 50], [100, 50, 120, 40, 300], [200, 200, 50], [150, 150, 150], [50, 200, 200]]
    rows += [[40, EXTENT_N]] * len(EXTENT_PLACEMENTS)
    b = _batch(rows, 5, rng, "numpy", 1, np_seed=4711)
    extent, k = [], sum(len(r) for r in rows[:6])
    for j, idx in enumerate(EXTENT_PLACEMENTS):
        axis, sign = j % 3, (-1.0 if j % 2 else 1.0)
        b["parts"][k + 1] = extent_part(rng, EXTENT_N, idx, axis, sign) + np.array([3.0, -1.0, 2.0])
        extent.append((6 + j, idx % EXTENT_N, axis, sign))
        k += 2
    b["extent"] = extent
    return b


@functools.lru_cache(maxsize=None)
def collate_part_count_batches():
    """(P, B) of PART_COUNT_SHAPES: parts of 1..6 points (ties for the largest are common), samples with fewer than P parts (trailing
    padding) except the first, which fills every column when P is 64 or more; reversed order, no features"""
    out = {}
    for P, B in PART_COUNT_SHAPES:
        rng = np.random.default_rng(1000 * P + B)
        rows = []
        for b in range(B):
            n = P if (b == 0 and P >= 64) or P == 1 else int(rng.integers(1, P))
            rows.append([int(x) for x in rng.integers(1, 7, n)])
        out[(P, B)] = _batch(rows, P, rng, "reverse", 0)
    return out


@functools.lru_cache(maxsize=None)
def collate_empty_parts_batch():
    """C ABI only: empty parts in front of and between the non-empty ones, a sample of empty parts only between two normal samples, a
    primary part behind a run of empty parts; identity order, F = 32"""
    rows = [[0, 0, 50, 0, 70, 30], [40, 60, 0, 0, 0, 0], [0] * 6, [0, 20, 0, 0, 90, 0], [33, 0, 0, 0, 0, 33]]
    return _batch(rows, 6, np.random.default_rng(303), "identity", 32)


@functools.lru_cache(maxsize=None)
def collate_dtype_batches():
    """fp64 clouds 1e5 from the origin (world-frame scans), fp32 clouds 3e2 from it, and a mixed batch in which ONE fp64 part promotes
    the whole batch; no order, F = 3"""
    rows = [[500, 300], [129, 700, 64]]
    f64 = _batch(rows, 3, np.random.default_rng(404), "none", 3, centre=(1e5, 1e5, 1e5), dtype=np.float64, spread=(9.0, 6.0, 2.0))
    f32 = _batch(rows, 3, np.random.default_rng(405), "none", 3, centre=(3e2, 3e2, 3e2), dtype=np.float32, spread=(9.0, 6.0, 2.0))
    mixed = _batch(rows, 3, np.random.default_rng(406), "none", 3, centre=(3e2, 3e2, 3e2), dtype=np.float32, spread=(9.0, 6.0, 2.0))
    mixed["parts"][3] = mixed["parts"][3].astype(np.float64) + 1e-9          # not representable in fp32: the promotion is visible
    return {"f64_far": f64, "f32": f32, "mixed": mixed}


@functools.lru_cache(maxsize=None)
def collate_single_point_batch():
    """a sample whose primary part has ONE point (scale 0: the reference divides by it) between two normal samples"""
    return _batch([[80, 120], [1, 1, 1], [90, 30, 10]], 3, np.random.default_rng(505), "random", 1)


# ---------------------------------------------------------------------------------------------
# 2. output transforms: rap_relative_transforms
# ---------------------------------------------------------------------------------------------
REL_SHAPES = [(1, 1), (1, 63), (1, 64), (1, 65), (5, 13), (3, 64), (70, 3), (2, 130)]
REL_FRAMES = ("none", "rigid", "general")


def _rotations(g, n):
    return torch.stack([random_rotation(g) for _ in range(n)])


@functools.lru_cache(maxsize=None)
def relative_case(B, P):
    """-> dict of fp32 / int64 tensors: R_pred, t_pred, R_gt, t_gt (B,P,..), scales (B,) (0.02 and 80 among them), ppp (B,P) with empty
    parts scattered -- flat index 63 empty and 64 not where B*P > 64 and B is odd, the other way round where B is even -- and the
    global frames G_rigid / G_general (B,3,3) (a rotation; a rotation times diag(2, 0.5, 1.5)), g_rigid / g_general (B,3) (the general
    one 300 long)"""
    g = torch.Generator().manual_seed(7000 + 131 * B + P)
    n = B * P
    c = {"R_pred": _rotations(g, n).reshape(B, P, 3, 3).float(), "R_gt": _rotations(g, n).reshape(B, P, 3, 3).float(),
         "t_pred": torch.randn(B, P, 3, generator=g), "t_gt": torch.randn(B, P, 3, generator=g)}
    sc = torch.exp(torch.empty(B).uniform_(-1.0, 3.0, generator=g))
    sc[0] = 0.02
    if B > 1:
        sc[B - 1] = 80.0
    ppp = torch.randint(1, 100, (n,), generator=g)
    ppp[torch.rand(n, generator=g) < 0.15] = 0
    if n > 64:
        ppp[63], ppp[64] = (0, 5) if B % 2 else (5, 0)
    elif n == 64:
        ppp[63] = 0
    if n == 1:
        ppp[0] = 7
    Gr = _rotations(g, B)
    c.update(scales=sc, ppp=ppp.reshape(B, P), G_rigid=Gr.float(), g_rigid=torch.randn(B, 3, generator=g) * 5,
             G_general=(_rotations(g, B) @ torch.diag(torch.tensor([2.0, 0.5, 1.5], dtype=torch.float64))).float(),
             g_general=300.0 * torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=1))
    return c


def relative_frame(c, frame):
    return (None, None) if frame == "none" else (c["G_" + frame], c["g_" + frame])


def relative_transforms_f64(R_pred, t_pred, R_gt, t_gt, scales, ppp, G=None, g=None):
    """O.relative_transforms (eval/evaluator.py:436-474) restated in float64 throughout -- the committed oracle, like the reference, holds
    the 4x4 in float32 and inverts and multiplies there.  -> (ref (B,P,4,4), bound (B,P,4,4)), float64 numpy.
    The device rounds the 4x4 m = [R_rel | t_rel] to fp32 and multiplies by inv(G) in double, then rounds again: per entry
    bound = 2 * 2^-24 * (sum_k |m_rk| |Ginv_kc| + |ref|), the factor 2 the margin over the two roundings."""
    B, P = ppp.shape
    ref, bound = np.zeros((B, P, 4, 4)), np.zeros((B, P, 4, 4))
    for b in range(B):
        s = float(scales[b])
        Ginv = np.eye(4)
        if G is not None:
            Gm = np.eye(4)
            Gm[:3, :3], Gm[:3, 3] = G[b].double().numpy(), g[b].double().numpy()
            Ginv = np.linalg.inv(Gm)
        for p in range(P):
            if ppp[b, p] == 0:
                continue
            Rp, Rg = R_pred[b, p].double().numpy(), R_gt[b, p].double().numpy()
            tp, tg = t_pred[b, p].double().numpy() * s, t_gt[b, p].double().numpy() * s
            RrT = Rg @ Rp.T
            M = np.eye(4)
            M[:3, :3], M[:3, 3] = RrT.T, tp - tg @ RrT
            ref[b, p] = M @ Ginv
            bound[b, p] = 2 * F32_HALF * (np.abs(M) @ np.abs(Ginv) + np.abs(ref[b, p]))
    return ref, bound


# ---------------------------------------------------------------------------------------------
# 3. transform errors: rap_transform_errors, rap_transform_errors_direct
# ---------------------------------------------------------------------------------------------
TE_SHAPES = [(1, 1), (3, 2), (70, 3), (1, 63), (3, 64), (3, 65), (1, 130), (3, 130)]          # (B, P)
TE_ANGLES = [0.0, 1e-3, 0.3, 5.0, 90.0, 175.0, 179.99, 180.0]                                   # degrees; the class of a part is its index here
TE_ROLES = ("anchor_first", "anchor_middle", "anchor_last", "two_anchors", "no_anchor", "anchor_only", "anchor_on_empty")
TE_MATCHED = ("none", "identity", "permuted", "out_of_range")
TE_OUT_OF_RANGE = (-1, None, 2 ** 40)                                                           # None: P itself

# Measured by tests/test_boundary_cases_host.py::test_transform_error_bounds_are_the_measured_ones: the largest deviation of
# O.compute_transform_errors evaluated in float32 on the CPU from the same function in float64, over every case below (all shapes, all
# matched kinds, with and without scale).  d(theta) = d(cos) / sin(theta): the classes differ by orders of magnitude.  Rotation error
# per angle class of TE_ANGLES, degrees (measured 2.798e-2 2.798e-2 1.888e-3 1.125e-4 4.801e-6 7.881e-5 2.797e-2 2.146e-2, translation
# 1.262e-5, means 1.819e-2 degrees and 4.618e-6; written here rounded up to two digits.  At both ends of the range one step of the fp32
# cosine next to +-1 is sqrt(2 * 2^-24) rad = 0.02 degrees):
TE_ROT_MEASURED = (2.8e-2, 2.8e-2, 1.9e-3, 1.2e-4, 4.9e-6, 7.9e-5, 2.8e-2, 2.2e-2)
TE_TRANS_MEASURED = 1.3e-5                                # translation error per part, all cases
TE_ROT_MEAN_MEASURED = 1.9e-2                             # the per-sample means
TE_TRANS_MEAN_MEASURED = 4.7e-6
TE_MARGIN = 4.0          # the device evaluates a different but equally valid fp32 association (fma chains against separate roundings)
TE_ROT_BOUND = tuple(TE_MARGIN * x for x in TE_ROT_MEASURED)
TE_TRANS_BOUND = TE_MARGIN * TE_TRANS_MEASURED
TE_ROT_MEAN_BOUND = TE_MARGIN * TE_ROT_MEAN_MEASURED
TE_TRANS_MEAN_BOUND = TE_MARGIN * TE_TRANS_MEAN_MEASURED
TE_DIRECT_ULPS = 2.0     # rap_transform_errors_direct computes in double: 2 fp32 ulp of the reference value


def axis_angle(g, deg):
    """float64 rotation by `deg` degrees about a random axis (Rodrigues); exactly the identity for 0"""
    if deg == 0.0:
        return torch.eye(3, dtype=torch.float64)
    k = torch.nn.functional.normalize(torch.randn(3, generator=g, dtype=torch.float64), dim=0)
    K = torch.tensor([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]], dtype=torch.float64)
    th = torch.deg2rad(torch.tensor(deg, dtype=torch.float64))
    return torch.eye(3, dtype=torch.float64) + torch.sin(th) * K + (1 - torch.cos(th)) * (K @ K)


@functools.lru_cache(maxsize=None)
def transform_error_case(B, P, matched):
    """-> dict: R_gt, t_gt, R_pred, t_pred fp32 (the pred arrays AS HANDED TO THE KERNEL, i.e. already laid out so that
    pred[matched[p]] is part p's prediction), ppp (B,P) int64, anchor (B,P) bool, matched (B,P) int64 or None, clamped (the ids
    clamped to [0, P-1]) or None, scale (B,), cls (B,P) int64: the index into TE_ANGLES of part p's constructed error angle (-1
    where an out-of-range id redirects the part, or its sample's anchor, to another part's prediction), roles [per sample].
    Sample b plays role TE_ROLES[(b + P) % 7]; part p of sample b carries the angle TE_ANGLES[(p + b) % 8]; every anchor-flagged part
    is predicted exactly (angle 0, class 0), so that the error relative to the anchor IS the constructed angle.  Columns 63 and 64
    are empty in alternating samples."""
    g = torch.Generator().manual_seed(9000 + 977 * B + 13 * P + TE_MATCHED.index(matched))
    ppp = torch.randint(1, 50, (B, P), generator=g)
    ppp[torch.rand(B, P, generator=g) < 0.1] = 0
    anchor = torch.zeros(B, P, dtype=torch.bool)
    roles = []
    for b in range(B):
        role = TE_ROLES[(b + P) % len(TE_ROLES)]
        roles.append(role)
        if P > 64:
            ppp[b, 63], ppp[b, 64] = (0, 9) if b % 2 == 0 else (9, 0)
        elif P == 64:
            ppp[b, 63] = 0 if b % 2 == 0 else 9
        mid = P // 2 if P // 2 not in (63, 64) else 62
        a = {"anchor_first": 0, "anchor_middle": mid, "anchor_last": P - 1, "two_anchors": mid, "anchor_only": mid,
             "anchor_on_empty": mid, "no_anchor": None}[role]
        if a is not None:
            anchor[b, a] = True
            ppp[b, a] = 0 if role == "anchor_on_empty" else 11
        if role == "two_anchors" and P > 1:
            anchor[b, P - 1] = True
            ppp[b, P - 1] = 12
        if role == "anchor_only":
            ppp[b] = 0
            ppp[b, a] = 11
        if role == "no_anchor" and P == 1:
            ppp[b, 0] = 5
    cls = (torch.arange(P)[None, :] + torch.arange(B)[:, None]) % len(TE_ANGLES)
    cls[anchor] = 0
    R_gt = torch.stack([random_rotation(g) for _ in range(B * P)]).reshape(B, P, 3, 3)
    R_nom = torch.stack([R_gt[b, p] @ axis_angle(g, TE_ANGLES[int(cls[b, p])]) for b in range(B) for p in range(P)]).reshape(B, P, 3, 3)
    t_gt = torch.randn(B, P, 3, generator=g)
    t_nom = t_gt + 0.05 * torch.randn(B, P, 3, generator=g)
    R_gt, R_nom = R_gt.float(), R_nom.float()
    R_nom[cls == 0] = R_gt[cls == 0]                                   # angle 0 exactly: the same fp32 matrix
    ids = clamped = None
    R_pred, t_pred = R_nom, t_nom
    if matched != "none":
        ids = torch.arange(P).repeat(B, 1)
        if matched == "permuted":
            ids = torch.stack([torch.randperm(P, generator=g) for _ in range(B)])
            R_pred, t_pred = torch.empty_like(R_nom), torch.empty_like(t_nom)
            bi = torch.arange(B)[:, None]
            R_pred[bi, ids], t_pred[bi, ids] = R_nom, t_nom            # pred[matched[p]] = the prediction of part p
        clamped = ids.clone()
        if matched == "out_of_range":
            cls = cls.clone()
            for b in range(B):
                # -1 at column 0 and P / 2^40 at column P-1 clamp to the column itself; at any other column they redirect the part
                cols = sorted({0, P - 1} | {int(x) for x in torch.randint(0, P, (3,), generator=g)})
                for j, p in enumerate(cols):
                    if P == 1:
                        bad = TE_OUT_OF_RANGE[b % 3]
                    elif p == 0:
                        bad = -1
                    elif p == P - 1:
                        bad = TE_OUT_OF_RANGE[1 + b % 2]
                    else:
                        bad = TE_OUT_OF_RANGE[(j + b) % 3]
                    bad = P if bad is None else bad
                    ids[b, p] = bad
                    clamped[b, p] = min(max(bad, 0), P - 1)
                    if clamped[b, p] != p:
                        if anchor[b, p] and int(anchor[b].nonzero()[0]) == p:
                            cls[b] = -1                                # the sample's frame is another part's prediction
                        cls[b, p] = -1
    scale = 0.5 + 40.0 * torch.rand(B, generator=g)
    return {"R_gt": R_gt, "t_gt": t_gt, "R_pred": R_pred.contiguous(), "t_pred": t_pred.contiguous(), "ppp": ppp, "anchor": anchor,
            "matched": ids, "clamped": clamped, "scale": scale, "cls": cls, "roles": roles}


def transform_error_cases():
    """(B, P, matched kind, with scale) of every case: every shape with every matched kind, the scale alternating"""
    return [(B, P, m, (i + j) % 2 == 0) for i, (B, P) in enumerate(TE_SHAPES) for j, m in enumerate(TE_MATCHED)]


def transform_errors_oracle(c, dtype, with_scale):
    """O.compute_transform_errors in `dtype` on the fp32 inputs, the ids clamped to [0, P-1] -> (rot_mean, trans_mean, rot, trans)"""
    f = lambda x: x.to(dtype)
    return O.compute_transform_errors(f(c["R_gt"]), f(c["t_gt"]), f(c["R_pred"]), f(c["t_pred"]), c["ppp"], c["anchor"], c["clamped"],
                                      f(c["scale"]) if with_scale else None)


def transform_errors_direct_f64(c, with_scale):
    """compute_transform_errors_direct (eval/metrics.py:305-383) restated in float64: no anchor frame, every non-empty part counts,
    delta_R = R_gt^T R_pred, delta_t = (t_pred - t_gt) scale -> (rot_mean, trans_mean, rot (B,P), trans (B,P)), float64"""
    B, P = c["ppp"].shape
    Rg, tg, Rp, tp = c["R_gt"].double(), c["t_gt"].double(), c["R_pred"].double(), c["t_pred"].double()
    if c["clamped"] is not None:
        bi = torch.arange(B)[:, None]
        Rp, tp = Rp[bi, c["clamped"]], tp[bi, c["clamped"]]
    s = c["scale"].double() if with_scale else torch.ones(B, dtype=torch.float64)
    valid = c["ppp"] != 0
    tr = torch.einsum("bpij,bpij->bp", Rg, Rp)
    rot = torch.rad2deg(torch.acos((0.5 * (tr - 1)).clamp(-1, 1))) * valid
    trans = torch.linalg.norm((tp - tg) * s[:, None, None], dim=-1) * valid
    n = valid.sum(1)
    return rot.sum(1) / n, trans.sum(1) / n, rot, trans


def angle_class_of(cls, ref_deg):
    """classes (B,P) with every -1 (a part redirected by a clamped id: its angle is whatever two unrelated rotations give) replaced by
    the class that brackets the float64 reference angle on the side of the SMALLER sine, i.e. of the wider bound's neighbour that is
    at least as ill-conditioned as the angle itself"""
    out = cls.clone()
    for b, p in (cls < 0).nonzero().tolist():
        a = float(ref_deg[b, p])
        lo = max(i for i, t in enumerate(TE_ANGLES) if t <= a)
        hi = min(i for i, t in enumerate(TE_ANGLES) if t >= a)
        out[b, p] = lo if np.sin(np.radians(TE_ANGLES[lo])) <= np.sin(np.radians(TE_ANGLES[hi])) else hi
    return out


# ---------------------------------------------------------------------------------------------
# 4. generation selection: rap_select_generation
# ---------------------------------------------------------------------------------------------
SEL_G = [1, 2, 5, 17]
SEL_B = [1, 63, 64, 65, 200]
SEL_KINDS = ("tie", "inf", "neg_inf", "nan")
SEL_LEFT = {"tie": 63, "inf": 62, "neg_inf": 61, "nan": 60}            # samples of the first 64-sample block ...
SEL_RIGHT = {"tie": 64, "inf": 65, "neg_inf": 66, "nan": 67}           # ... and of the second
GATHER_COUNTS = [0, 1, 85, 86, 1365, 1366, 5000]                       # points per sample: 3 n floats around 256 and around 16 x 256
GATHER_P = [1, 28, 29, 86]                                             # P*9 and P*3 cross 256 at 29 and 86


@functools.lru_cache(maxsize=None)
def selection_values(G, B):
    """(G,B) fp32: small integers (ties everywhere), and at the samples of SEL_LEFT / SEL_RIGHT that exist: a column of equal values;
    +inf in generation 0 (and a finite value elsewhere); -inf in generation (G - 1) // 2 and in the last one; NaN in generation
    (G - 1) // 2 and in the last one (the FIRST NaN wins)"""
    g = torch.Generator().manual_seed(100 * G + B)
    v = torch.randint(0, 4, (G, B), generator=g).float()
    for kind in SEL_KINDS:
        for b in (SEL_LEFT[kind], SEL_RIGHT[kind]):
            if b >= B:
                continue
            if kind == "tie":
                v[:, b] = 2.0
            elif kind == "inf":
                v[0, b] = float("inf")
            elif kind == "neg_inf":
                v[G - 1, b] = v[(G - 1) // 2, b] = float("-inf")
            else:
                v[G - 1, b] = v[(G - 1) // 2, b] = float("nan")
    return v


def first_extremum(v, largest):
    """the documented rule in plain Python: the first NaN if there is one, else the first index of the minimum / maximum"""
    out = []
    for col in v.T.tolist():
        nan = [i for i, x in enumerate(col) if x != x]
        ext = max(col) if largest else min(col)
        out.append(nan[0] if nan else col.index(ext))
    return torch.tensor(out, dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def gather_case(P, counts=tuple(GATHER_COUNTS), G=3):
    """clouds (G,TP,3), R (G,B,P,3,3), t (G,B,P,3) from arange (all below 2^24: exact in fp32, every element unique inside its array),
    rmse (G,B) with a different winner from sample to sample, cu (B+1,) int64"""
    B = len(counts)
    cu = torch.tensor([0] + list(np.cumsum(counts)), dtype=torch.int64)
    TP = int(cu[-1])
    mk = lambda *shape: torch.arange(int(np.prod(shape)), dtype=torch.float32).reshape(shape) + 1.0
    assert G * max(TP * 3, B * P * 9) < 2 ** 24
    g = torch.Generator().manual_seed(31 * P + B)
    return {"clouds": mk(G, TP, 3), "R": mk(G, B, P, 3, 3), "t": mk(G, B, P, 3), "rmse": torch.rand(G, B, generator=g), "cu": cu}


# ---------------------------------------------------------------------------------------------
# 5. batch tables: rap_token_sample, rap_check_batch
# ---------------------------------------------------------------------------------------------
TOKEN_LENGTHS = [1, 255, 256, 257, 16383, 16384, 16385, 40000]          # around the 64 x 256 grid stride of one sample's blocks


@functools.lru_cache(maxsize=None)
def token_tables():
    """-> {name: (B+1,) int32 cu}.  `many`: B = 1000, cu[0] = 7 (entries in front of the first sample are not the kernel's), empty
    samples first (two in a row), in the middle (a run of three), last (two), the named lengths in between small samples"""
    rng = np.random.default_rng(606)
    lens = rng.integers(0, 6, 1000)
    lens[[0, 1, 500, 501, 502, 998, 999]] = 0
    lens[2] = 3
    for i, n in enumerate(TOKEN_LENGTHS):
        lens[100 + 97 * i] = n
    cu = lambda first, l: torch.tensor(np.concatenate([[first], first + np.cumsum(l)]), dtype=torch.int32)
    return {"many": cu(7, lens), "one_40000": cu(0, [40000]), "one_1": cu(3, [1]), "one_16385": cu(0, [16385])}


def check_batch_bits(ppp, cu, TP):
    """the documented bit table of rap_check_batch (include/rapflow.h) in plain Python: bit 0 sum != TP, bit 1 cu_seqlens ends, bit 2
    cu_seqlens decreasing, bit 3 a sample's parts against its span, bit 4 a negative size"""
    B = len(ppp)
    f = 0
    if sum(sum(r) for r in ppp) != TP:
        f |= 1
    if cu[0] != 0 or cu[B] != TP:
        f |= 2
    for b in range(B):
        if cu[b + 1] < cu[b]:
            f |= 4
        if sum(ppp[b]) != cu[b + 1] - cu[b]:
            f |= 8
        if any(n < 0 for n in ppp[b]):
            f |= 16
    return f


CHECK_BASE = ([[3, 2], [0, 4], [1, 1]], [0, 5, 9, 11], 11)


def check_batch_cases():
    """-> {name: (ppp, cu, TP, the bit the defect is named for)}.  Bits 1, 3 and 4 can be raised ALONE; bits 0 and 2 cannot: with
    cu[0] = 0, cu[B] = TP and every sample's parts equal to its span the total IS TP (bit 0 needs bit 1 or 3), and a decreasing cu has a
    negative span, which only negative sizes can match (bit 2 needs bit 3 or 4).  The host test proves this by enumeration; for those two
    bits the case is the minimal defect, and every case asserts the whole flag."""
    ppp, cu, TP = CHECK_BASE
    edit = lambda b, p, d: [[n + (d if (i, j) == (b, p) else 0) for j, n in enumerate(r)] for i, r in enumerate(ppp)]
    return {
        "consistent": (ppp, cu, TP, 0),
        "sum": (edit(1, 1, 1), cu, TP, 1),                              # one point too many in a part
        "ends": (ppp, cu, TP + 1, 2),                                   # the caller's point count one larger than the table's
        "first_entry": (ppp, [1, 5, 9, 11], TP, 2),
        "ends_alone": (ppp, [1, 6, 10, 12], TP, 2),                     # the whole table shifted by one
        "decreasing": (ppp, [0, 5, 4, 11], TP, 4),
        "span_alone": ([[4, 2], [0, 3], [1, 1]], cu, TP, 8),            # a point moved to the neighbouring sample
        "negative_alone": ([[3, 2], [-2, 6], [1, 1]], cu, TP, 16),      # sizes that still add up
        "negative_and_sum": (edit(2, 0, -3), cu, TP, 16),
        "everything": ([[3, 2], [-1, 4], [1, 1]], [2, 5, 4, 12], TP, 4),
    }


def small_check_tables():
    """every table with (B, P) = (2, 1) and (1, 2), sizes in -1..2, cu entries in 0..3 and TP in 0..3: what the enumeration of the host
    test runs over"""
    for a, b in itertools.product(range(-1, 3), repeat=2):
        for cu in itertools.product(range(4), repeat=2):
            for TP in range(4):
                yield [[a, b]], list(cu), TP
    for a, b in itertools.product(range(-1, 3), repeat=2):
        for cu in itertools.product(range(4), repeat=3):
            for TP in range(4):
                yield [[a], [b]], list(cu), TP
