"""Inputs that the host test (tests/test_caller_edge_cases_host.py) and the three GPU edge files of the kernels around the sampler share:
Procrustes / rigidity (test_procrustes_edges_gpu.py), the brute-force nearest-neighbour kernels (test_nn_edges_gpu.py) and voxel
down-sampling (test_voxel_edges_gpu.py).  Seeded, pure torch / numpy; every builder is cached and its result is not to be modified.

Thresholds are never tuned to a device result: where a count must be exact, the threshold is put in the middle of the widest gap of the
float64 distances near its nominal value, so that every distance is further from it than fp32 arithmetic can move it (the host test
asserts the margins with the oracle)."""
import functools

import numpy as np
import torch

# ---------------------------------------------------------------------------------------------
# Procrustes / rigidity
# ---------------------------------------------------------------------------------------------
PROC_BATCH, PROC_CHUNKS = 2048, 16          # points per batch of the moments kernel's chunk walk, RAP_PROC_CHUNKS
P_SWEEP = 8
SIZES_NAMED = [1, 2, 3, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 32767, 32768, 32769, 40000, 65537, 70001]
# the named sizes reach the chunk counts 1, 2, 3 and 16 only: one size that splits evenly and one that does not for every other count
# (c * 2000 points are c chunks of 2000; c * 2000 + 1 leave a remainder), and the even split that 3 lacks
SIZES_FILL = [6000] + [n for c in range(4, 16) for n in (c * 2000, c * 2000 + 1)]
SWEEP_SIZES = SIZES_NAMED + SIZES_FILL


def proc_chunks_of(n):
    """procrustes.hip: chunks a part of n points is cut into"""
    return min(max((n + PROC_BATCH - 1) // PROC_BATCH, 1), PROC_CHUNKS)


def chunk_lengths(n):
    nc = proc_chunks_of(n)
    return [n * (c + 1) // nc - n * c // nc for c in range(nc)]


def random_rotation(g):
    """a proper rotation (float64) from the QR factorisation of a Gaussian matrix"""
    q, r = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
    q = q * torch.sign(torch.diagonal(r))
    if torch.det(q) < 0:
        q[:, 0] *= -1
    return q


def noisy_rigid_image(src, g, noise, t_scale=0.5, about=None):
    """src (n,3) fp32 -> fp32 (src - c) R^T + c + t + noise * N(0,1), R a random proper rotation about c (the origin by default)"""
    R = random_rotation(g)
    t = t_scale * (2 * torch.rand(3, generator=g, dtype=torch.float64) - 1)
    c = torch.zeros(3, dtype=torch.float64) if about is None else about.double()
    return ((src.double() - c) @ R.T + c + t + noise * torch.randn(src.shape, generator=g, dtype=torch.float64)).float()


def sweep_layout():
    """rows of P_SWEEP part sizes: an empty part leading row 0, one in the middle of row 1, row 2 all empty, one trailing row 3, the
    rest filled in order and padded with trailing empty parts"""
    s = list(SWEEP_SIZES)
    take = lambda k: [s.pop(0) for _ in range(min(k, len(s)))]
    rows = [[0] + take(7), None, [0] * P_SWEEP, None]
    rows[1] = take(3) + [0] + take(4)
    rows[3] = take(7) + [0]
    while s:
        r = take(P_SWEEP)
        rows.append(r + [0] * (P_SWEEP - len(r)))
    return rows


def offsets_of(ppp):
    """(B,P) sizes -> (B*P+1,) part offsets and (B+1,) sample offsets, int64"""
    flat = ppp.reshape(-1).long()
    off = torch.cat([torch.zeros(1, dtype=torch.int64), flat.cumsum(0)])
    return off, off[:: ppp.shape[1]].clone()


@functools.lru_cache(maxsize=None)
def procrustes_sweep():
    """-> dict: src, tgt (TP,3) fp32, ppp (B,8) int64, cu (B+1,) int64, off (B*8+1,), traj (3,TP,3) fp32, scales (B,) fp32.
    Every part is a noisy rigid image of its source (spread 1, noise 0.05)."""
    g = torch.Generator().manual_seed(20240607)
    ppp = torch.tensor(sweep_layout(), dtype=torch.int64)
    off, cu = offsets_of(ppp)
    TP = int(off[-1])
    src = torch.randn(TP, 3, generator=g)
    tgt = torch.empty_like(src)
    for k in range(ppp.numel()):
        a, e = int(off[k]), int(off[k + 1])
        if e > a:
            tgt[a:e] = noisy_rigid_image(src[a:e], g, 0.05)
    traj = torch.stack([tgt + 0.01 * (s + 1) * torch.randn(TP, 3, generator=g) for s in range(2)] + [tgt])
    scales = 0.5 + 2.0 * torch.rand(ppp.shape[0], generator=g)
    return {"src": src, "tgt": tgt, "ppp": ppp, "cu": cu, "off": off, "traj": traj, "scales": scales}


def compacted(ppp):
    """The oracle (like the reference) indexes a sample's NON-EMPTY parts by position, i.e. it assumes that empty parts trail.  -> the
    table with every row's empty parts moved behind (same points, same order) and `where` (B,P): the original column of every compacted
    column (-1 for the trailing empties), so that oracle_out[b, j] belongs to part where[b, j]."""
    B, P = ppp.shape
    out, where = torch.zeros_like(ppp), torch.full((B, P), -1, dtype=torch.int64)
    for b in range(B):
        keep = [p for p in range(P) if int(ppp[b, p]) > 0]
        for j, p in enumerate(keep):
            out[b, j], where[b, j] = ppp[b, p], p
    return out, where


def uncompact(x, where):
    """oracle output (B,P,...) on the compacted table -> rows at their original columns, zeros for empty parts"""
    out = torch.zeros_like(x)
    for b in range(where.shape[0]):
        for j in range(where.shape[1]):
            if where[b, j] >= 0:
                out[b, where[b, j]] = x[b, j]
    return out


def compact_like(x, where):
    """(B,P,...) at original columns -> at compacted columns (what the oracle's rigidity functions index)"""
    out = torch.zeros_like(x)
    for b in range(where.shape[0]):
        for j in range(where.shape[1]):
            if where[b, j] >= 0:
                out[b, j] = x[b, where[b, j]]
    return out


DEGENERATE_UNIQUE = ("uncorrelated", "rigid_noise", "reflection", "planar")          # rotation and translation are determined
DEGENERATE_FREE = ("collinear", "single_point", "coincident", "two_points")           # only the residual is


@functools.lru_cache(maxsize=None)
def degenerate_parts():
    """The kinds of tests/test_host_logic.py::test_device_kabsch_code_matches_oracle_svd plus `coincident` (every source point the same:
    H = 0) and `two_points`, at n in {3, 300, 2049} where the kind allows it, packed as the parts of one batch.
    -> dict: src, tgt (TP,3) fp32, ppp (B,5), cu, off, cases [(kind, n)] in part order"""
    g = torch.Generator().manual_seed(977)
    cases = [(k, n) for k in DEGENERATE_UNIQUE + ("collinear", "coincident") for n in (3, 300, 2049)] + [("single_point", 1), ("two_points", 2)]
    S, T = [], []
    for kind, n in cases:
        src = torch.randn(n, 3, generator=g)
        q = random_rotation(g).float()
        if kind == "uncorrelated":
            tgt = torch.randn(n, 3, generator=g)
        elif kind == "rigid_noise":
            tgt = src @ q.T + torch.randn(3, generator=g) + 0.01 * torch.randn(n, 3, generator=g)
        elif kind == "reflection":
            m = q.clone(); m[:, 0] *= -1
            tgt = src @ m.T + 0.05 * torch.randn(n, 3, generator=g)
        elif kind == "planar":
            src[:, 2] = 0
            tgt = src @ q.T
        elif kind == "collinear":
            src = torch.outer(torch.randn(n, generator=g), torch.tensor([1.0, 2.0, -0.5]))
            tgt = src @ q.T
        elif kind == "coincident":
            src = src[:1].repeat(n, 1)
            tgt = src @ q.T + torch.randn(3, generator=g) + 0.05 * torch.randn(n, 3, generator=g)
        elif kind == "single_point":
            tgt = torch.randn(1, 3, generator=g)
        else:
            tgt = src @ q.T + 0.05 * torch.randn(n, 3, generator=g)
        S.append(src.contiguous()); T.append(tgt.contiguous())
    assert len(cases) % 5 == 0
    ppp = torch.tensor([n for _, n in cases], dtype=torch.int64).reshape(-1, 5)
    off, cu = offsets_of(ppp)
    return {"src": torch.cat(S), "tgt": torch.cat(T), "ppp": ppp, "cu": cu, "off": off, "cases": cases}


FAR_CASES = [(300.0, 5.0, 4097), (300.0, 5.0, 70001), (1000.0, 5.0, 4097), (1000.0, 5.0, 70001)]
FAR_FRAMES = ("origin", "centre")


@functools.lru_cache(maxsize=None)
def far_parts():
    """Parts far from the origin: centre offset * (1, -0.6, 0.3), Gaussian of the given spread, a noisy rigid image (noise 0.05 of the
    spread).  Sample 0: the image is rotated about the ORIGIN (the target is as far out as the source, the translation of the fit is
    small); sample 1: about the part's own centre (the translation of the fit is of the size of the offset, so its fp32 rounding shows).
    The four cases are the parts of each sample.  -> dict: src, tgt, ppp (2,4), cu, off"""
    g = torch.Generator().manual_seed(31337)
    S, T = [], []
    for frame in FAR_FRAMES:
        for offset, spread, n in FAR_CASES:
            c = offset * torch.tensor([1.0, -0.6, 0.3], dtype=torch.float64)
            src = (spread * torch.randn(n, 3, generator=g, dtype=torch.float64) + c).float()
            S.append(src); T.append(noisy_rigid_image(src, g, 0.05 * spread, about=c if frame == "centre" else None))
    ppp = torch.tensor([[n for _, _, n in FAR_CASES]] * len(FAR_FRAMES), dtype=torch.int64)
    off, cu = offsets_of(ppp)
    return {"src": torch.cat(S), "tgt": torch.cat(T), "ppp": ppp, "cu": cu, "off": off}


# ---------------------------------------------------------------------------------------------
# the brute-force nearest-neighbour kernels: a 256-slot candidate tile each
# ---------------------------------------------------------------------------------------------
NN_TILE = 256
NN_SIZES = [1, 2, 255, 256, 257, 511, 512, 513, 769]
MARGIN = 1e-5                               # every distance is at least this far from every threshold (fp32 moves a distance by < 1e-6)
F32_BELOW_QUARTER = float(np.nextafter(np.float32(0.25), np.float32(0)))


def gap_threshold(values, nominal, rel=0.3):
    """the middle of the widest gap between consecutive sorted `values` (float64, finite) inside nominal * (1 -+ rel), end points
    included; nominal itself where no value is near"""
    lo, hi = nominal * (1 - rel), nominal * (1 + rel)
    v = np.sort(np.asarray(values, dtype=np.float64))
    v = np.concatenate([[lo], v[(v > lo) & (v < hi)], [hi]])
    k = int(np.argmax(np.diff(v)))
    return float(0.5 * (v[k] + v[k + 1]))


def min_other_part_distance(pts, sizes):
    """numpy float64: distance of every point of one sample to the nearest point of a DIFFERENT part (inf where there is none)"""
    p = np.asarray(pts, dtype=np.float64)
    pid = np.repeat(np.arange(len(sizes)), sizes)
    d = np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(-1))
    d[pid[:, None] == pid[None, :]] = np.inf
    return d.min(axis=1) if len(p) else np.zeros(0)


def overlap_splits(N):
    return [(N - 1, 1, 0), (1, 0, N - 1), (N // 2, 0, N - N // 2)]


@functools.lru_cache(maxsize=None)
def overlap_batch():
    """P = 3.  Every total of NN_SIZES in the three splits; a sample with one non-empty part; a sample of one point; and for N in
    {257, 513} two tail-slot samples each: parts 0 and 1 fill the unit cube, ONE query of them sits at (10, 10, 10) + 0.02 and its only
    near neighbour of another part is the sample's LAST point (part 2, one point, the single occupied slot of the last tile) -- or the
    sample's FIRST point (part 0, one point), the query then being in part 2.
    -> dict: pts (TP,3) fp32, ppp (B,3), cu, taus (3 floats), tail [(sample, query row in the batch, 'last' | 'first')]"""
    g = torch.Generator().manual_seed(4242)
    rows, clouds, tail = [], [], []
    for N in NN_SIZES:
        for sp in overlap_splits(N):
            rows.append(sp); clouds.append(torch.rand(N, 3, generator=g))
    rows.append((300, 0, 0)); clouds.append(torch.rand(300, 3, generator=g))
    rows.append((0, 1, 0)); clouds.append(torch.rand(1, 3, generator=g))
    far = torch.tensor([10.0, 10.0, 10.0])
    for N in (257, 513):
        for which in ("last", "first"):
            c = torch.rand(N, 3, generator=g)
            n0 = (N - 1) // 2
            if which == "last":
                sp, q = (n0, N - 1 - n0, 1), 7
                c[N - 1] = far
            else:
                sp, q = (1, n0, N - 1 - n0), N - 3
                c[0] = far
            c[q] = far + torch.tensor([0.02, 0.0, 0.0])
            tail.append((len(rows), q, which))
            rows.append(sp); clouds.append(c)
    ppp = torch.tensor(rows, dtype=torch.int64)
    off, cu = offsets_of(ppp)
    tail = [(b, int(cu[b]) + q, w) for b, q, w in tail]
    mind = np.concatenate([min_other_part_distance(c.numpy(), list(r)) for c, r in zip(clouds, rows)])
    fin = mind[np.isfinite(mind)]
    taus = tuple(gap_threshold(fin, nom) for nom in (0.05, 0.1, 0.25))
    return {"pts": torch.cat(clouds), "ppp": ppp, "cu": cu, "taus": taus, "tail": tail}


@functools.lru_cache(maxsize=None)
def overlap_lattice():
    """8 x 7 x 5 lattice of spacing 0.25, part = parity of the x index (P = 2, packed part-major): the nearest point of the other part is
    the x neighbour at exactly 0.25 -- every coordinate is a multiple of 1/4 below 2, so d^2 = 1/16 and its root are exact in fp32.
    -> dict: pts (280,3), ppp (1,2), cu, taus (0.25, the fp32 number below it)"""
    g = np.stack(np.meshgrid(np.arange(8), np.arange(7), np.arange(5), indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(5)
    even, odd = g[g[:, 0] % 2 == 0], g[g[:, 0] % 2 == 1]
    even, odd = even[rng.permutation(len(even))], odd[rng.permutation(len(odd))]
    pts = torch.from_numpy((np.concatenate([even, odd]) * 0.25).astype(np.float32))
    ppp = torch.tensor([[len(even), len(odd)]], dtype=torch.int64)
    return {"pts": pts, "ppp": ppp, "cu": torch.tensor([0, len(g)]), "taus": (0.25, F32_BELOW_QUARTER)}


@functools.lru_cache(maxsize=None)
def chamfer_batch():
    """the size sweep as the objects of one cu; gt and pred are different clouds -> gt, pred (TP,3) fp32, cu (B+1,) int64"""
    g = torch.Generator().manual_seed(808)
    TP = sum(NN_SIZES)
    gt = torch.rand(TP, 3, generator=g)
    pred = torch.rand(TP, 3, generator=g) + torch.tensor([0.05, -0.02, 0.01])
    cu = torch.tensor([0] + list(np.cumsum(NN_SIZES)), dtype=torch.int64)
    return {"gt": gt, "pred": pred, "cu": cu}


CORR_PAIRS = [(1, 1), (1, 300), (300, 1), (255, 257), (256, 256), (257, 255), (513, 1000)]


def nearest_f64(src, tgt):
    """numpy float64, direct differences: (first arg-min, its distance) per row of src"""
    s, t = np.asarray(src, dtype=np.float64), np.asarray(tgt, dtype=np.float64)
    d = np.sqrt(((s[:, None, :] - t[None, :, :]) ** 2).sum(-1))
    i = d.argmin(axis=1)
    return i, d[np.arange(len(s)), i]


@functools.lru_cache(maxsize=None)
def correspondence_pairs():
    """-> list of dict: sg (Ns,3), tg (Nt,3), sp, tp fp32 and thr: the threshold in the widest gap of the nearest distances around their
    median (a single source: its distance + 0.01), so that roughly half of the sources count"""
    g = torch.Generator().manual_seed(1717)
    out = []
    for ns, nt in CORR_PAIRS:
        sg, tg = torch.rand(ns, 3, generator=g), torch.rand(nt, 3, generator=g)
        sp = sg + 0.03 * torch.randn(ns, 3, generator=g)
        tp = tg + 0.03 * torch.randn(nt, 3, generator=g)
        _, d = nearest_f64(sg.numpy(), tg.numpy())
        thr = float(d[0]) + 0.01 if ns == 1 else gap_threshold(d, float(np.median(d)))
        out.append({"sg": sg, "tg": tg, "sp": sp, "tp": tp, "thr": thr})
    return out


@functools.lru_cache(maxsize=None)
def correspondence_ties():
    """A target cloud of 300 points followed by the SAME 300 points in another order (600 rows, three candidate tiles), every row with
    its own target_pred; 257 sources, each 0.01 from one of the points.  Both copies of the nearest point are at the same distance: the
    rule (first arg-min, torch.min on the CPU) decides which target_pred row enters.
    -> dict sg, tg, sp, tp, thr and first / last (257,): the lower and the higher index of the nearest point"""
    g = torch.Generator().manual_seed(2323)
    base = torch.rand(300, 3, generator=g)
    perm = torch.randperm(300, generator=g)
    tg = torch.cat([base, base[perm]])
    pick = torch.randperm(300, generator=g)[:257]
    sg = base[pick] + 0.01 * torch.nn.functional.normalize(torch.randn(257, 3, generator=g), dim=1)
    sp = sg + 0.03 * torch.randn(257, 3, generator=g)
    tp = torch.rand(600, 3, generator=g)
    inv = torch.empty(300, dtype=torch.int64); inv[perm] = torch.arange(300)
    return {"sg": sg, "tg": tg, "sp": sp, "tp": tp, "thr": 0.05, "first": pick.numpy(), "last": (300 + inv[pick]).numpy()}


@functools.lru_cache(maxsize=None)
def correspondence_lattice():
    """sources on a 7 x 6 x 7 lattice of spacing 0.5 (294 points), targets = the sources moved by (0.25, 0, 0) in another order: the
    nearest target of every source is at exactly 0.25 (d^2 = 1/16 and its root exact in fp32) -> dict sg, tg, sp, tp"""
    g = np.stack(np.meshgrid(np.arange(7), np.arange(6), np.arange(7), indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(6)
    sg = torch.from_numpy((g * 0.5).astype(np.float32))
    tg = (sg + torch.tensor([0.25, 0.0, 0.0]))[torch.from_numpy(rng.permutation(len(g)))]
    gen = torch.Generator().manual_seed(66)
    return {"sg": sg, "tg": tg, "sp": torch.rand(len(g), 3, generator=gen), "tp": torch.rand(len(g), 3, generator=gen)}


@functools.lru_cache(maxsize=None)
def pair_batch():
    """CORR_PAIRS as the samples of one packed batch with P = 2 for compute_pair_metrics in direct mode: one threshold (0.25 m) for the
    batch, every pair scaled so that its own threshold lands there.  -> (data dict without device placement, cloud, thr)"""
    pairs = correspondence_pairs()
    ppp = torch.tensor(CORR_PAIRS, dtype=torch.int64)
    off, cu = offsets_of(ppp)
    B = len(pairs)
    data = {"pointclouds_gt": torch.cat([x for p in pairs for x in (p["sg"], p["tg"])]), "points_per_part": ppp,
            "cu_seqlens_batch": cu.to(torch.int32), "scales": torch.tensor([0.25 / p["thr"] for p in pairs], dtype=torch.float32),
            "rotations": torch.eye(3).repeat(B, 2, 1, 1), "translations": torch.zeros(B, 2, 3)}
    cloud = torch.cat([x for p in pairs for x in (p["sp"], p["tp"])])
    return data, cloud, 0.25


LARGE_PAIRS = [(16_700, 300), (300, 257)]      # 66 items of 256 sources: a second round of pair_finish_kernel's lane-strided sum; then
#                                                an ordinary pair, whose first item is therefore not item 0


@functools.lru_cache(maxsize=None)
def large_pair_batch():
    """LARGE_PAIRS as one packed batch for compute_pair_metrics in direct mode (the layout of pair_batch).  Every source lies either
    0.005 .. 0.02 or 0.04 .. 0.05 from a target point and the threshold sits in the widest gap of the nearest distances around 0.03.
    -> (data, cloud, thr, pairs): pairs as correspondence_pairs() gives them, for the float64 oracle"""
    g = torch.Generator().manual_seed(3131)
    pairs = []
    for ns, nt in LARGE_PAIRS:
        tg = torch.rand(nt, 3, generator=g)
        pick = torch.randint(0, nt, (ns,), generator=g)
        r = torch.where(torch.rand(ns, generator=g) < 0.5, 0.005 + 0.015 * torch.rand(ns, generator=g), 0.04 + 0.01 * torch.rand(ns, generator=g))
        sg = tg[pick] + r[:, None] * torch.nn.functional.normalize(torch.randn(ns, 3, generator=g), dim=1)
        sp = sg + 0.03 * torch.randn(ns, 3, generator=g)
        tp = tg + 0.03 * torch.randn(nt, 3, generator=g)
        d = torch.cdist(sg.double(), tg.double()).min(dim=1).values.numpy()
        pairs.append({"sg": sg, "tg": tg, "sp": sp, "tp": tp, "thr": gap_threshold(d, 0.03)})
    ppp = torch.tensor(LARGE_PAIRS, dtype=torch.int64)
    off, cu = offsets_of(ppp)
    B = len(pairs)
    data = {"pointclouds_gt": torch.cat([x for p in pairs for x in (p["sg"], p["tg"])]), "points_per_part": ppp,
            "cu_seqlens_batch": cu.to(torch.int32), "scales": torch.tensor([0.25 / p["thr"] for p in pairs], dtype=torch.float32),
            "rotations": torch.eye(3).repeat(B, 2, 1, 1), "translations": torch.zeros(B, 2, 3)}
    cloud = torch.cat([x for p in pairs for x in (p["sp"], p["tp"])])
    return data, cloud, 0.25, pairs


# ---------------------------------------------------------------------------------------------
# voxel down-sampling and coverage
# ---------------------------------------------------------------------------------------------
VX_CHUNK = 4096


def voxel_slots(v):
    """slots of the dense key table: the largest key gx + gy v + gz v^2 with every g <= v, plus one"""
    return v + v * v + v * v * v + 1


def grid_extent(points, vs):
    """largest grid coordinate after the shift to the cloud's corner: the reference's `v`"""
    g = np.floor(np.asarray(points, dtype=np.float32) / np.float32(vs)).astype(np.int64)
    return int((g - g.min(axis=0)).max())


@functools.lru_cache(maxsize=None)
def voxel_cases():
    """-> {name: (points (N,3) fp32 numpy, voxel size)}"""
    rng = np.random.default_rng(99)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    cases = {}
    cell = lambda n: f32(0.25 + 0.25 * (0.02 + 0.96 * rng.random((n, 3))))               # inside the cell [0.25, 0.5)^3
    cases["one_voxel_n1"] = (cell(1), 0.25)
    cases["one_voxel_n50"] = (cell(50), 0.25)
    cases["v1_block"] = (f32(0.5 * (0.01 + 0.98 * rng.random((200, 3))) - 0.25), 0.25)     # cells -1 and 0 on every axis
    centres = (np.stack(np.meshgrid(np.arange(5), np.arange(5), np.arange(3), indexing="ij"), -1).reshape(-1, 3) + 0.5) * 0.25
    cases["all_centres_twice"] = (f32(np.concatenate([centres, centres[::-1]])), 0.25)
    ks = (np.arange(-8, 9) * 0.25).astype(np.float32)
    faces = ks[[0, 3, 7, 8, 9, 13, 16]]
    vals = np.concatenate([ks, [np.float32(-0.0)], np.nextafter(faces, np.float32(np.inf)), np.nextafter(faces, np.float32(-np.inf))]).astype(np.float32)
    pts = vals[rng.integers(0, len(vals), (600, 3))]
    pts[:len(vals), 0] = vals                                                             # every value occurs at least once on every axis
    pts[len(vals):2 * len(vals), 1] = vals
    pts[2 * len(vals):3 * len(vals), 2] = vals
    cases["faces_and_signs"] = (f32(pts), 0.25)
    for v in (15, 16):
        p = 0.25 * (v + 1) * rng.random((3000, 3))
        p[1234] = 0.25 * np.array([0.3, 0.6, 0.2])                                                  # the corner cell (0,0,0): key 0
        p[77] = 0.25 * np.array([v + 0.4, v + 0.7, v + 0.1])                                        # the cell (v,v,v): the last slot
        cases[f"table_v{v}"] = (f32(p), 0.25)
    for n in (255, 256, 257):
        cases[f"n{n}"] = (f32(rng.random((n, 3))), 0.1)
    others = rng.random((500, 3))
    one = np.array([[0.4321, 0.1234, 0.8765]])
    cases["crowded"] = (f32(np.concatenate([others[:250], np.repeat(one, 10000, axis=0), others[250:]])), 0.1)
    return cases
