"""The shapes, the form each one is there for and the fp64 references that the host and the GPU tests of the GEMM kernels' edges share
(tests/test_gemm_cases_host.py, tests/test_gemm_edges_gpu.py).  Pure Python / torch: nothing here touches a GPU.

A FORM is what the launchers decide from a call's shape (include/rapflow.h, rap_gemm_f32_form / rap_gemm_h16_form):
100 * kernel + 10 * stages + splits with kernel 1 = 128 x 128 tiles, 2 = 256 x 256 one tile per block, 3 = 256 x 256 persistent; stages the
LDS stages of the 128 x 128 kernel (2, or 4 for the 16-bit four-stage ring), 0 otherwise; splits the blocks per tile that K is divided
over.  Every case below carries the form it is meant to reach -- written down from the thresholds of the dispatch as documented (512 / 256
tiles of 256 x 256, 256 blocks for the ring, 64 / 128 tiles of 128 x 128 for split-K on a 256-CU part), NOT computed by the library -- and
tests/test_gemm_cases_host.py asks the library whether that is still where the shape goes, so that a retuned threshold cannot silently
move a case onto another kernel.

Families: "f32" (rap_gemm_f32, rap_gemm_f32_splitk), "bf16" / "f16" (rap_gemm_h16, rap_gemm_h16_qkvnorm, rap_gemm_h16_splitk; dtype 1 / 2)
and "x2" (rap_x2_gemm, split precision, dtype 3).  K of a case is LOGICAL; the split-precision calls see 2 K physical fp16 columns.
"""
import collections

import torch

DTYPE = {"bf16": 1, "f16": 2, "x2": 3}
H16 = ("bf16", "f16")
F128_2, F128_4, F256, F256P = 121, 141, 201, 301       # unsplit forms; + 1 / + 3 on the 128 x 128 forms: K over 2 / 4 blocks per tile

# epilogue numbers -> what the reference below computes
F32_EPI = {0: "bias", 1: "resid", 2: "silu", 3: "geglu", 4: "qkv", 5: "anchor", 6: "relu"}
H16_EPI = {0: "bias", 1: "resid", 3: "geglu", 4: "qkv", 5: "qkvnorm", 7: "resid16"}
X2_EPI = {1: "resid", 3: "geglu", 5: "qkvnorm"}

# sect: which sweep of test_gemm_edges_gpu.py runs the case; tune: ((key, value), ...) set around the call (restored after); ws: the call goes
# through the split-K entry point with exactly the workspace it reports; planes: the SiLU planes of rap_gemm_f32_splitk; H: heads of a QKV case
Case = collections.namedtuple("Case", "sect fam epi M N K form tune ws planes H")


def case(sect, fam, epi, M, N, K, form, tune=(), ws=0, planes=0, H=0):
    return Case(sect, fam, epi, M, N, K, form, tuple(tune), ws, planes, H)


def epi_name(c):
    return (F32_EPI if c.fam == "f32" else X2_EPI if c.fam == "x2" else H16_EPI)[c.epi]


def phys_k(c):
    return 2 * c.K if c.fam == "x2" else c.K


def tile_rows(form):
    return 128 if form // 100 == 1 else 256


def tiles(c):
    """output tiles of the kernel the case reaches (the QKV epilogues of the 128 x 128 kernel cover whole 256-row groups)"""
    t = tile_rows(c.form)
    mt = -(-c.M // 256) * (256 // t) if epi_name(c) in ("qkv", "qkvnorm") and c.fam != "f32" else -(-c.M // t)
    return mt * (c.N // t)


def ragged(c):
    return c.M % tile_rows(c.form) != 0


# ---- 1. row-tail sweep, 128 x 128 kernels ----
ROW_TAIL_MS = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 385]
# 5 and 7 row tiles at N = 128: with the lists of the sweep (1-4 row tiles by 1, 2, 3 or 6 column tiles; 512 .. 780 tiles of 256 x 256)
# no tile count is 5 or 7 (mod 8), and xcd_remap gives the eight XCDs chunks of different lengths exactly when the count is no multiple of 8
RESIDUE_MS = [600, 800]


def row_tail_cases():
    out = []
    for N in (128, 384):
        for K in (32, 96):
            for epi in (0, 1, 2, 3, 5, 6):
                out += [case("rowtail", "f32", epi, M, N, K, F128_2) for M in ROW_TAIL_MS]
            if N == 384:
                out += [case("rowtail", "f32", 4, M, N, K, F128_2, H=2) for M in ROW_TAIL_MS]
        for fam in H16:
            for K in (64, 192):
                for epi in (0, 1, 3, 7):
                    out += [case("rowtail", fam, epi, M, N, K, F128_4) for M in ROW_TAIL_MS]
                if N == 384:
                    out += [case("rowtail", fam, 4, M, N, K, F128_4, H=2) for M in ROW_TAIL_MS]
    for fam in H16:                                        # the fused qk-norm needs K >= 128
        out += [case("rowtail", fam, 5, M, 768, 128, F128_4, H=4) for M in ROW_TAIL_MS]
    for K in (64, 96):                                     # split precision: N % 256 == 0, physical K >= 128; the fused QKV needs N = 192 H: H = 4
        for epi in (1, 3):
            out += [case("rowtail", "x2", epi, M, 256, K, F128_4) for M in ROW_TAIL_MS]
        out += [case("rowtail", "x2", 5, M, 768, K, F128_4, H=4) for M in ROW_TAIL_MS]
    out += [case("rowtail", "f32", 0, M, 128, 32, F128_2) for M in RESIDUE_MS]
    out += [case("rowtail", fam, 0, M, 128, 64, F128_4) for fam in H16 for M in RESIDUE_MS]
    return out


# ---- 2. k-tile sweep on the four-stage ring (and the same calls on two stages: tuning key 18 = 0) ----
RING_MS = [1, 129, 300]
RING_KTILES = [1, 2, 3, 4, 5, 6, 7, 8, 9, 16]             # physical K / 64


def ring_cases():
    out = []
    for fam in ("bf16", "f16", "x2"):
        for kt in RING_KTILES:
            if fam == "x2" and kt < 2:
                continue
            K = 64 * kt // (2 if fam == "x2" else 1)
            for M in RING_MS:
                out.append(case("ring", fam, 1, M, 256, K, F128_4))
                out.append(case("ring", fam, 1, M, 256, K, F128_2, tune=((18, 0),)))
    # the two-stage kernel at its natural size: 65 x 4 = 260 blocks, one k-tile (K < 128) and an odd count (8320 = 65 x 128: its full-tile case)
    for M in (8200, 8320):
        for fam in H16:
            out += [case("ring", fam, 1, M, 512, K, F128_2) for K in (64, 192)]
        out.append(case("ring", "x2", 1, M, 512, 96, F128_2))
    return out


# ---- 3. ragged M on 256 x 256, one tile per block; the same operands one row tile below the threshold on 128 x 128 ----
RAGGED_F32_MS = [16129, 16255, 16257, 16383]               # 1, 127, 129, 255 rows in the 64th row tile: 64 x 8 = 512 tiles
RAGGED_F32_QKV_MS = [10753, 11007]                         # 43 x 12 = 516 tiles at N = 3072
RAGGED_H16_MS = [7937, 8063, 8065, 8191]                   # the 32nd row tile: 32 x 8 = 256 tiles
RAGGED_H16_QKV_MS = [5377, 5631]                           # 22 x 12 = 264 tiles at N = 3072


def ragged256_cases():
    out = []
    for K in (256, 288):
        for epi in (0, 1, 2, 3, 5, 6):
            out += [case("ragged256", "f32", epi, M, 2048, K, F256) for M in RAGGED_F32_MS]
            out.append(case("ragged256", "f32", epi, RAGGED_F32_MS[0] - 256, 2048, K, F128_2))        # 63 x 8 = 504 tiles
    out += [case("ragged256", "f32", 4, M, 3072, 256, F256, H=16) for M in RAGGED_F32_QKV_MS]
    out.append(case("ragged256", "f32", 4, RAGGED_F32_QKV_MS[0] - 256, 3072, 256, F128_2, H=16))       # 42 x 12 = 504 tiles
    for fam in H16:
        for K in (128, 192, 512):
            for epi in (0, 1, 3, 7):
                out += [case("ragged256", fam, epi, M, 2048, K, F256) for M in RAGGED_H16_MS]
                out.append(case("ragged256", fam, epi, RAGGED_H16_MS[0] - 256, 2048, K, F128_2))       # 31 x 8 = 248 tiles; 61 x 16 blocks
        for K in (128, 192):
            for epi in (4, 5):
                out += [case("ragged256", fam, epi, M, 3072, K, F256, H=16) for M in RAGGED_H16_QKV_MS]
                out.append(case("ragged256", fam, epi, RAGGED_H16_QKV_MS[0] - 256, 3072, K, F128_2, H=16))     # 21 x 12 = 252 tiles
        # 6 heads: N = 1152 is no multiple of 256, so the 256 x 256 kernels cannot tile it however many rows there are (64 x 4 = 256 of their
        # tiles here: the fused qk-norm used to go to the one-tile kernel all the same and left the last 128 columns unwritten)
        out.append(case("ragged256", fam, 5, 16129, 1152, 128, F128_2, H=6))
    for K in (64, 96, 256):
        for epi in (1, 3):
            out += [case("ragged256", "x2", epi, M, 2048, K, F256) for M in RAGGED_H16_MS]
            out.append(case("ragged256", "x2", epi, RAGGED_H16_MS[0] - 256, 2048, K, F128_2))
        # (the fused QKV needs N = 192 H: N = 2048 cannot hold it, so it runs at the 16-bit QKV shapes)
        out += [case("ragged256", "x2", 5, M, 3072, K, F256, H=16) for M in RAGGED_H16_QKV_MS]
        out.append(case("ragged256", "x2", 5, RAGGED_H16_QKV_MS[0] - 256, 3072, K, F128_2, H=16))
    return out


# ---- 4. uneven persistent walk and short K; the same calls with the persistent key off (tuning 12 fp32, 11 the others) ----
WALK_MS = [16640, 16384]                                   # 520 = 2 x 256 + 8 and 512 tiles at N = 2048; 780 and 768 at N = 3072


def walk_cases():
    out = []

    def both(fam, epi, N, K, H=0):
        key = 12 if fam == "f32" else 11
        for M in WALK_MS:
            out.append(case("walk", fam, epi, M, N, K, F256P, H=H))
            out.append(case("walk", fam, epi, M, N, K, F256, tune=((key, 0),), H=H))
    for K in (256, 288):
        for epi in (0, 1, 3):
            both("f32", epi, 2048, K)
    for fam in H16:
        for K in (128, 192, 512):
            for epi in (0, 1, 3, 7):
                both(fam, epi, 2048, K)
            both(fam, 5, 3072, K, H=16)
    for K in (64, 96):
        for epi in (1, 3):
            both("x2", epi, 2048, K)
    return out


# ---- 5. split-K edges, through the split-K entry points with exactly the reported workspace ----
SPLITK_H16_MS = [1, 2048, 2049, 4096, 4097]                # 4, 64 | 68, 128 | 132 tiles of 128 x 128 at N = 512
SPLITK_F32_MS = [1, 100, 2048, 2049, 4096, 4097]
SILU_MS = [1, 129, 257, 256]                              # (256: the full-tile case of the two- and four-plane forms)


def splitk_cases():
    out = []
    t128 = lambda M, N: -(-M // 128) * (N // 128)
    for fam in H16:
        for K in (1024, 1280, 1088):                       # 16, 20 and 17 k-tiles of 64: 17 is no multiple of 4 (nor of 2) -> unsplit, no workspace
            for M in SPLITK_H16_MS:
                t = t128(M, 512)
                s = 1 if K == 1088 else 4 if t <= 64 else 2 if t <= 128 else 1
                for epi in (1, 7):
                    out.append(case("splitk", fam, epi, M, 512, K, F128_4 - 1 + s, ws=1))     # (at most 132 x 1 or 128 x 2 blocks: the ring)
    for K in (480, 512, 544, 1024, 1056):                  # 15, 16, 17, 32, 33 k-tiles of 32: the shares of 17 are 4, 4, 4, 5
        for M in SPLITK_F32_MS:
            t = t128(M, 512)
            s = 4 if (K >= 1024 and t <= 128) or (K >= 512 and t <= 64) else 1
            out.append(case("splitk", "f32", 1, M, 512, K, F128_2 - 1 + s, ws=1))
    for planes in (2, 4):
        for N in (128, 384):
            for K in (512, 576, 544):                      # 16, 18, 17 k-tiles: 18 divides by 2 only, 17 by neither
                s = planes if (K // 32) % planes == 0 else 1
                out += [case("splitk", "f32", 2, M, N, K, F128_2 - 1 + s, ws=1, planes=planes) for M in SILU_MS]
    return out


# ---- 6. leading dimensions: one ragged case per family and form (the persistent form has no ragged M: its uneven walk) ----
def ld_cases():
    out = [case("ld", "f32", 1, 257, 384, 96, F128_2), case("ld", "f32", 1, 16129, 2048, 288, F256), case("ld", "f32", 1, 16640, 2048, 288, F256P),
           case("ld", "f32", 1, 2048 - 37, 512, 544, F128_2 + 3, ws=1), case("ld", "f32", 2, 257, 384, 576, F128_2 + 1, ws=1, planes=2)]
    for fam in H16:
        out += [case("ld", fam, 1, 257, 384, 192, F128_4), case("ld", fam, 1, 8200, 512, 192, F128_2), case("ld", fam, 1, 7937, 2048, 192, F256),
                case("ld", fam, 1, 16640, 2048, 192, F256P), case("ld", fam, 1, 2049, 512, 1280, F128_4 + 1, ws=1),
                case("ld", fam, 1, 2048 - 37, 512, 1280, F128_4 + 3, ws=1)]
    out += [case("ld", "x2", 1, 257, 256, 96, F128_4), case("ld", "x2", 1, 8200, 512, 96, F128_2), case("ld", "x2", 1, 7937, 2048, 96, F256),
            case("ld", "x2", 1, 16640, 2048, 96, F256P)]
    return out


def all_cases():
    return row_tail_cases() + ring_cases() + ragged256_cases() + walk_cases() + splitk_cases() + ld_cases()


# the threshold pairs of the dispatch: (family, epilogue, N, K logical, M below, M above, has_ws) -- the two M land on DIFFERENT forms.  One
# column tile (N = 256 for the 256 x 256 kernels, N = 128 for the 128 x 128 ones), so that the two M are EXACT neighbours in the count the
# rule looks at: a threshold moved by one tile or block fails
THRESHOLD_PAIRS = [
    ("f32", 0, 256, 256, 510 * 256 + 1, 511 * 256 + 1, 0),              # 511 | 512 tiles of 256 x 256, ragged: 128 x 128 | one tile per block
    ("f32", 0, 256, 256, 511 * 256, 512 * 256, 0),                      # 511 | 512 full tiles: 128 x 128 | persistent
    ("bf16", 0, 256, 128, 255 * 256, 255 * 256 + 1, 0),                 # 255 | 256 tiles: 128 x 128 | one tile per block
    ("f16", 0, 256, 128, 511 * 256 + 255, 512 * 256, 0),                # ragged 512 | full 512 tiles: one tile per block | persistent
    ("bf16", 0, 256, 128, 511 * 256, 512 * 256, 0),                     # 511 | 512 full tiles: one tile per block | persistent
    ("x2", 1, 256, 64, 255 * 256, 255 * 256 + 1, 0),                    # 255 | 256 tiles
    ("x2", 1, 256, 64, 511 * 256, 512 * 256, 0),                        # 511 | 512 full tiles
    ("bf16", 1, 128, 64, 256 * 128, 256 * 128 + 1, 0),                  # 256 | 257 blocks of 128 x 128: four-stage ring | two stages
    ("x2", 1, 256, 64, 128 * 128, 128 * 128 + 1, 0),                    # 256 | 258 blocks (split precision has N % 256 == 0: two column tiles)
    ("f16", 1, 128, 1024, 64 * 128, 64 * 128 + 1, 1),                   # 64 | 65 tiles: K over 4 | 2 blocks
    ("f16", 7, 128, 1024, 128 * 128, 128 * 128 + 1, 1),                 # 128 | 129 tiles: K over 2 | unsplit
    ("f32", 1, 128, 512, 64 * 128, 64 * 128 + 1, 1),                    # 64 | 65 tiles, K >= 512: K over 4 | unsplit
    ("f32", 1, 128, 1024, 128 * 128, 128 * 128 + 1, 1),                 # 128 | 129 tiles, K >= 1024
    ("f32", 1, 128, 992, 65 * 128, 64 * 128, 1),                        # (K < 1024 splits only up to 64 tiles)
]


def form_of(lib, c, M=None):
    """the library's decision for the call the GPU test makes for this case (contiguous operands)"""
    M = c.M if M is None else M
    if c.fam == "f32":
        cols = c.N // 2 if c.epi == 3 else c.N
        return lib.rap_gemm_f32_form(c.epi, M, c.N, c.K, c.K, c.K, cols, c.N if c.epi == 1 else 0, c.ws, c.planes)
    return lib.rap_gemm_h16_form(DTYPE[c.fam], c.epi, M, c.N, phys_k(c), phys_k(c), phys_k(c), c.ws)


class tuned:
    """with tuned(lib, ((key, value), ...)): the keys are set inside and back at their defaults afterwards (the library has no getter;
    tests/test_gemm_cases_host.py checks DEFAULTS against the initialisers in the library's source)"""
    DEFAULTS = {5: 1, 6: 1, 11: 1, 12: 1, 17: 1024, 18: 256, 19: 1, 20: 1}
    VARIABLES = {5: ("attn_f32.hip", "g_rap_attn_split"), 6: ("gemm_f32.hip", "g_rap_gemm_splitk"), 11: ("gemm_h16.hip", "g_rap_gemm_h16_persistent"),
                 12: ("gemm_f32.hip", "g_rap_gemm_f32_persistent"), 17: ("api.hip", "g_rap_x2_min_rows"), 18: ("gemm_h16.hip", "g_rap_ring_blocks"),
                 19: ("api.hip", "g_rap_small_fused"), 20: ("attn_h16.hip", "g_rap_attn_h16_small")}

    def __init__(self, lib, pairs):
        self.lib, self.pairs = lib, tuple(pairs)

    def __enter__(self):
        for k, v in self.pairs:
            assert self.lib.rap_set_tuning(k, v) == 0, (k, v)

    def __exit__(self, *exc):
        for k, _ in self.pairs:
            assert self.lib.rap_set_tuning(k, self.DEFAULTS[k]) == 0, k
        return False


# ---- common.h: xcd_remap, transcribed ----
def xcd_remap(bid, nblk):
    q, r = nblk >> 3, nblk & 7
    xcd, idx = bid & 7, bid >> 3
    base = xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q
    return base + idx


# ---- the split rules, restated (gemm_f32.hip: gemm_f32_splits_by_shape; gemm_h16.hip: gemm_h16_splits_by_shape) ----
def f32_kshares(K, splits):
    """k-tiles (of 32 columns) per block of a split fp32 GEMM: block y takes [nk y / splits, nk (y + 1) / splits)"""
    nk = K // 32
    return [nk * (y + 1) // splits - nk * y // splits for y in range(splits)]


# ---- fp64 references: u = A W^T (+ bias) in float64, (M, N), on whatever device the operands are ----
def base64(A, W, bias=None):
    u = A.double() @ W.double().T
    return u if bias is None else u + bias.double()


def ref_epilogue(name, u, resid=None, anchor=None, emb=None, H=0, gq=None, gk=None, q_mul=8.0):
    """the epilogue `name` of F32_EPI / H16_EPI / X2_EPI applied to u (float64): what the call has to return, before any output rounding.
    geglu: u has the value columns first, then the gate columns (the kernels take the interleaved W; the result is the same (M, N / 2)).
    qkv / qkvnorm: [3][H][M][64]; qkvnorm normalises the q and k rows over the 64 dims, times gamma, times q_mul (q) or 8 (k)."""
    if name == "bias":
        return u
    if name in ("resid", "resid16"):
        return u + resid.double()
    if name == "silu":
        return u * torch.sigmoid(u)
    if name == "relu":
        return u.clamp_min(0.0)
    if name == "geglu":
        inner = u.shape[1] // 2
        g = u[:, inner:]
        return u[:, :inner] * (0.5 * g * (1.0 + torch.erf(g * 0.5 ** 0.5)))
    if name == "anchor":
        return u + torch.where(anchor.bool()[:, None], emb[1][None].double(), emb[0][None].double())
    x = u.reshape(u.shape[0], 3, H, 64).permute(1, 2, 0, 3)
    if name == "qkv":
        return x
    assert name == "qkvnorm"
    if gq is None:
        return x
    nrm = x[:2].norm(dim=-1, keepdim=True).clamp_min(1e-12)
    mul = torch.tensor([q_mul, 8.0], dtype=torch.float64, device=u.device)[:, None, None, None]
    qk = x[:2] / nrm * torch.stack([gq, gk])[:, :, None, :].double() * mul
    return torch.cat([qk, x[2:]], dim=0)
