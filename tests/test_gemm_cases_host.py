"""CPU: the cases of tests/test_gemm_edges_gpu.py are what they are there for -- every shape reaches the kernel form it is listed under
(through rap_gemm_f32_form / rap_gemm_h16_form: the launchers' own decision as host arithmetic), each dispatch threshold separates two forms,
every form of every family has a ragged-M and a full-tile case, the tile counts exercise every chunking of xcd_remap, the split-K rules are
host arithmetic, the new entry points refuse bad arguments before anything touches the device, and the fp64 references of the GPU tests
agree with a plain float64 evaluation."""
import ctypes
import collections

import pytest
import torch
import torch.nn.functional as F

import gemm_cases as GC
from rap_amd import _lib

N, ONE = ctypes.c_void_p(0), ctypes.c_void_p(256)      # NULL; a non-NULL sentinel -- every call below fails before a pointer is used


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_every_case_reaches_the_form_it_is_there_for(lib):
    cases = GC.all_cases()
    assert len(cases) > 1500
    wrong = []
    for c in cases:
        with GC.tuned(lib, c.tune):
            got = GC.form_of(lib, c)
        if got != c.form:
            wrong.append((c, got))
    assert not wrong, wrong[:10]
    # the decision is taken with the CURRENT tuning keys, and the defaults are back
    c = GC.case("x", "bf16", 1, 300, 256, 512, GC.F128_4)
    assert GC.form_of(lib, c) == 141
    with GC.tuned(lib, ((18, 0),)):
        assert GC.form_of(lib, c) == 121
    assert GC.form_of(lib, c) == 141


def test_the_defaults_that_tuned_restores_are_the_librarys_own(lib):
    """the library has no getter for a tuning key: the initialisers in its source are the statement of the defaults, and the table of
    rap_set_tuning ties each key to its variable"""
    import os
    import re
    from conftest import ROOT
    csrc = os.path.join(ROOT, "rap_amd", "csrc")
    table = open(os.path.join(csrc, "api.hip")).read()
    assert set(GC.tuned.DEFAULTS) == set(GC.tuned.VARIABLES)
    for key, (fname, var) in GC.tuned.VARIABLES.items():
        assert re.search(r"\{\s*%d\s*,\s*&%s\s*," % (key, var), table), (key, var)
        m = re.findall(r"^rap_tuning_t\s+%s\s*=\s*(-?\d+)\s*;" % var, open(os.path.join(csrc, fname)).read(), flags=re.M)
        assert m == [str(GC.tuned.DEFAULTS[key])], (key, var, m)


def test_each_threshold_pair_lands_on_different_forms(lib):
    seen = set()
    for fam, epi, Nn, K, lo, hi, ws in GC.THRESHOLD_PAIRS:
        a, b = (GC.form_of(lib, GC.case("pair", fam, epi, M, Nn, K, 0, ws=ws)) for M in (lo, hi))
        assert a > 0 and b > 0 and a != b, (fam, epi, Nn, K, lo, hi, a, b)
        seen.add((fam if fam == "f32" else "x2" if fam == "x2" else "h16", a, b))
    # 511 | 512 tiles (fp32: 128 x 128 below; 16-bit, split precision: one tile per block below), 255 | 256 tiles, 256 | 257 blocks, 64 | 65 and 128 | 129 tiles
    assert {("f32", 121, 201), ("f32", 121, 301), ("h16", 121, 201), ("h16", 201, 301), ("x2", 121, 201), ("x2", 201, 301), ("h16", 141, 121),
            ("x2", 141, 121), ("h16", 144, 142), ("h16", 142, 141), ("f32", 124, 121)} <= seen
    # the persistent forms never take a ragged M, whatever the tile count
    for fam, K in (("f32", 256), ("bf16", 128), ("x2", 64)):
        for M in (16385, 16639, 65537):
            assert GC.form_of(lib, GC.case("pair", fam, 1, M, 2048, K, 0)) == GC.F256
    # refused shapes are negative, an empty call is 0
    assert lib.rap_gemm_f32_form(0, 100, 100, 64, 64, 64, 100, 0, 0, 0) == -1 and lib.rap_gemm_f32_form(0, 100, 128, 48, 48, 48, 128, 0, 0, 0) == -1
    assert lib.rap_gemm_f32_form(0, 100, 128, 64, 66, 64, 128, 0, 0, 0) == -1 and lib.rap_gemm_f32_form(7, 100, 128, 64, 64, 64, 128, 0, 0, 0) == -1
    assert lib.rap_gemm_f32_form(0, 0, 128, 64, 64, 64, 128, 0, 0, 0) == 0 and lib.rap_gemm_h16_form(1, 0, 0, 128, 64, 64, 64, 0) == 0
    assert lib.rap_gemm_h16_form(1, 0, 100, 128, 96, 96, 96, 0) == -1 and lib.rap_gemm_h16_form(1, 0, 100, 128, 64, 32, 64, 0) == -1      # K % 64; lda < K
    assert lib.rap_gemm_h16_form(1, 6, 100, 128, 64, 64, 64, 0) == -1 and lib.rap_gemm_h16_form(4, 0, 100, 128, 64, 64, 64, 0) == -1      # retired epilogue; no such dtype
    assert lib.rap_gemm_h16_form(1, 5, 100, 768, 64, 64, 64, 0) == -1                                                                  # fused qk-norm: K >= 128
    assert lib.rap_gemm_h16_form(3, 1, 100, 384, 128, 128, 128, 0) == -1 and lib.rap_gemm_h16_form(3, 1, 100, 256, 64, 64, 64, 0) == -1   # split precision: N % 256, K physical >= 128
    assert lib.rap_gemm_h16_form(3, 0, 100, 256, 128, 128, 128, 0) == -1 and lib.rap_gemm_h16_form(3, 7, 100, 256, 128, 128, 128, 0) == -1


def test_every_form_of_every_family_has_a_ragged_and_a_full_tile_case():
    by_form = collections.defaultdict(lambda: {"ragged": 0, "full": 0})
    for c in GC.all_cases():
        fam = "h16" if c.fam in GC.H16 else c.fam
        by_form[(fam, c.form)]["ragged" if GC.ragged(c) else "full"] += 1
    want = {"f32": [121, 124, 122, 201, 301], "h16": [121, 141, 142, 144, 201, 301], "x2": [121, 141, 201, 301]}
    for fam, forms in want.items():
        assert {f for (a, f) in by_form if a == fam} == set(forms), fam
        for f in forms:
            n = by_form[(fam, f)]
            assert n["full"] > 0, (fam, f)
            # (the persistent walk takes full row tiles only -- the test above pins that a ragged M never reaches it; its "ragged" case is the
            # UNEVEN walk: 520 and 780 tiles on 256 blocks)
            if f == 301:
                assert n["ragged"] == 0
                assert {GC.tiles(c) % 256 for c in GC.walk_cases() if c.fam in ((fam,) if fam != "h16" else GC.H16) and c.form == 301} >= {0, 8}
            else:
                assert n["ragged"] > 0, (fam, f)
        # ... and the leading-dimension sweep runs every one of them with padded strides
        assert {c.form for c in GC.ld_cases() if c.fam in ((fam,) if fam != "h16" else GC.H16)} == set(forms), fam
        assert all(GC.ragged(c) for c in GC.ld_cases() if c.form != 301)
    for dt in GC.H16:
        assert {c.form for c in GC.ld_cases() if c.fam == dt} == set(want["h16"])
    # both bf16 and fp16 run every 16-bit form
    for dt in GC.H16:
        assert {c.form for c in GC.all_cases() if c.fam == dt} == set(want["h16"])


def test_the_sweeps_hold_the_row_tails_k_tile_counts_and_epilogues_they_claim():
    rt = GC.row_tail_cases()
    assert {c.M for c in rt} >= set(GC.ROW_TAIL_MS) and {c.epi for c in rt if c.fam == "f32"} == set(range(7))
    assert {c.epi for c in rt if c.fam == "bf16"} == {0, 1, 3, 4, 5, 7} and {c.epi for c in rt if c.fam == "x2"} == {1, 3, 5}
    ring = GC.ring_cases()
    for fam in ("bf16", "f16", "x2"):
        kts = {GC.phys_k(c) // 64 for c in ring if c.fam == fam and c.N == 256}
        assert kts == set(GC.RING_KTILES) - ({1} if fam == "x2" else set()), fam
    assert {(c.M, c.N, c.K) for c in ring if c.fam == "f16" and c.N == 512} >= {(8200, 512, 64), (8200, 512, 192)}
    r3 = GC.ragged256_cases()
    assert {c.M % 256 for c in r3 if c.form == GC.F256 and c.N == 2048} == {1, 127, 129, 255}
    assert {c.K for c in r3 if c.fam == "f32"} == {256, 288} and {c.K for c in r3 if c.fam == "f16"} == {128, 192, 512}
    assert {c.K for c in r3 if c.fam == "x2"} == {64, 96, 256}
    # short K on the pipelined 256 x 256 loops: 2 k-tiles (the accepted minimum) and an odd count, on both forms, plain and split precision
    for form in (GC.F256, GC.F256P):
        for fams in (GC.H16, ("x2",)):
            assert {GC.phys_k(c) // 64 for c in GC.all_cases() if c.form == form and c.fam in fams} >= {2, 3}
    assert max(c.M * (c.N if c.epi != 3 else c.N // 2) for c in GC.all_cases()) <= 16640 * 3072
    sk = GC.splitk_cases()
    assert {GC.f32_kshares(c.K, 4) == [4, 4, 4, 5] for c in sk if c.fam == "f32" and c.epi == 1 and c.K == 544} == {True}
    assert GC.f32_kshares(1056, 4) == [8, 8, 8, 9] and GC.f32_kshares(512, 4) == [4, 4, 4, 4] and GC.f32_kshares(576, 2) == [9, 9]


def test_xcd_remap_is_a_bijection_and_the_tile_counts_cover_every_residue():
    for n in range(1, 4097):
        assert sorted(GC.xcd_remap(b, n) for b in range(n)) == list(range(n)), n
    # every XCD's chunk is contiguous: blocks b, b + 8, b + 16, ... map to consecutive tiles
    for n in (5, 8, 13, 520, 780):
        for x in range(min(8, n)):
            chunk = [GC.xcd_remap(b, n) for b in range(x, n, 8)]
            assert chunk == list(range(chunk[0], chunk[0] + len(chunk))), (n, x)
    for fams in (("f32",), GC.H16, ("x2",)):
        res = {GC.tiles(c) % 8 for c in GC.all_cases() if c.fam in fams}
        assert res == set(range(8)) or (fams == ("x2",) and res >= {0, 2, 4, 6}), (fams, res)      # (split precision has even column-tile counts only)
    assert {GC.tiles(c) % 8 for c in GC.all_cases()} == set(range(8))


def test_splitk_rule_of_the_fp32_gemms_is_host_arithmetic(lib):
    """rap_gemm_f32_splitk_workspace_bytes states the few-row split-K rules of the fp32 GEMMs (gemm_f32.hip: gemm_f32_splits_by_shape):
    bias + residual: K >= 1024 with at most 128 tiles of 128 x 128, or K >= 512 with at most 64 -> 4 partial planes (uneven k shares
    allowed); bias + SiLU: `planes` (2 or 4) planes when K >= 512, K / 32 divides by planes and there are at most 64 tiles.  A function of
    the SHAPE alone: tuning key 6 gates the launch, not the reservation."""
    q = lib.rap_gemm_f32_splitk_workspace_bytes
    plane = lambda m, n: m * n * 4
    assert q(1, 2048, 512, 512, 0) == 4 * plane(2048, 512) and q(1, 2049, 512, 512, 0) == 0            # 64 | 68 tiles at K >= 512
    assert q(1, 2048, 512, 544, 0) == 4 * plane(2048, 512)                                             # 17 k-tiles: 4, 4, 4, 5
    assert q(1, 2048, 512, 480, 0) == 0 and q(1, 1, 512, 480, 0) == 0                                  # K < 512
    assert q(1, 4096, 512, 1024, 0) == 4 * plane(4096, 512) and q(1, 4097, 512, 1024, 0) == 0          # 128 | 132 tiles at K >= 1024
    assert q(1, 4096, 512, 992, 0) == 0 and q(1, 4096, 512, 1056, 0) == 4 * plane(4096, 512)
    assert q(1, 100, 500, 512, 0) == 0 and q(1, 100, 512, 520, 0) == 0 and q(1, 0, 512, 512, 0) == 0 and q(1, -3, 512, 512, 0) == 0
    assert q(1, 100, 512, 512, 2) == 4 * plane(100, 512)                                               # planes is a SiLU argument
    assert q(2, 257, 384, 512, 2) == 2 * plane(257, 384) and q(2, 257, 384, 512, 4) == 4 * plane(257, 384)
    assert q(2, 257, 384, 576, 2) == 2 * plane(257, 384) and q(2, 257, 384, 576, 4) == 0               # 18 k-tiles
    assert q(2, 257, 384, 544, 2) == 0 and q(2, 257, 384, 544, 4) == 0                                 # 17 k-tiles
    assert q(2, 257, 384, 512, 3) == 0 and q(2, 257, 384, 512, 0) == 0 and q(2, 257, 384, 480, 2) == 0
    assert q(2, 2048, 512, 512, 4) == 4 * plane(2048, 512) and q(2, 2049, 512, 512, 4) == 0            # 64 | 68 tiles
    assert q(0, 100, 512, 512, 4) == 0 and q(3, 100, 512, 512, 4) == 0                                 # the other epilogues never split
    # ... and the form says the same, for every case of the sweep; a workspace that is not handed in never splits
    for c in GC.splitk_cases():
        if c.fam == "f32":
            need = q(c.epi, c.M, c.N, c.K, c.planes)
            assert need == (c.form % 10 if c.form % 10 > 1 else 0) * plane(c.M, c.N), c
            assert lib.rap_gemm_f32_form(c.epi, c.M, c.N, c.K, c.K, c.K, c.N, c.N, 0, c.planes) == 121
        else:
            need = lib.rap_gemm_h16_splitk_workspace_bytes(c.M, c.N, c.K)
            assert need == (c.form % 10 if c.form % 10 > 1 else 0) * plane(c.M, c.N), c
    with GC.tuned(lib, ((6, 0),)):
        assert q(1, 2048, 512, 512, 0) == 4 * plane(2048, 512)                                         # still reserved
        assert lib.rap_gemm_f32_form(1, 2048, 512, 512, 512, 512, 512, 512, 1, 0) == 121               # but not launched
        assert lib.rap_gemm_h16_form(1, 1, 2048, 512, 1024, 1024, 1024, 1) == 141
    assert lib.rap_gemm_f32_form(1, 2048, 512, 512, 512, 512, 512, 512, 1, 0) == 124
    # rows leave the combine pass as 16-byte pieces: other strides run unsplit
    assert lib.rap_gemm_f32_form(1, 2048, 512, 512, 512, 512, 514, 512, 1, 0) == 121 and lib.rap_gemm_f32_form(1, 2048, 512, 512, 512, 512, 512, 513, 1, 0) == 121


def test_the_fp32_splitk_entry_point_refuses_bad_arguments_without_a_gpu(lib):
    def call(epi=1, A=ONE, W=ONE, C=ONE, resid=ONE, planes=0, ws=ONE, ws_bytes=1 << 30, M=2048, Nn=512, K=512):
        return lib.rap_gemm_f32_splitk(epi, A, K, W, K, C, Nn, M, Nn, K, N, resid, Nn, planes, ws, ws_bytes, N)
    assert call(A=N) == -1 and call(W=N) == -1 and call(C=N) == -1
    assert call(resid=N) == -1                                                       # the residual epilogue needs its residual
    for epi in (0, 3, 4, 5, 6, 7, -1):
        assert call(epi=epi) == -1, epi
    for planes in (0, 1, 3, 5, 8, -2):
        assert call(epi=2, planes=planes, M=257, Nn=384) == -1, planes
    need = lib.rap_gemm_f32_splitk_workspace_bytes(1, 2048, 512, 512, 0)
    assert need == 4 * 2048 * 512 * 4
    assert call(ws_bytes=need - 1) == -2 and call(ws=N) == -2 and call(ws=N, ws_bytes=0) == -2
    need2 = lib.rap_gemm_f32_splitk_workspace_bytes(2, 257, 384, 512, 2)
    assert call(epi=2, planes=2, M=257, Nn=384, ws_bytes=need2 - 1) == -2
    # an empty call is done before anything is launched, with or without a workspace
    assert call(M=0) == 0 and call(M=0, ws=N, ws_bytes=0) == 0


def test_the_fp64_references_agree_with_a_plain_float64_evaluation():
    g = torch.Generator().manual_seed(7)
    M, H, K = 37, 2, 96
    Nn = 3 * H * 64
    A = torch.randn(M, K, generator=g); W = torch.randn(Nn, K, generator=g) / K ** 0.5; b = torch.randn(Nn, generator=g)
    h = torch.randn(M, Nn, generator=g); anchor = torch.rand(M, generator=g) < 0.4; emb = torch.randn(2, Nn, generator=g)
    gq, gk = torch.rand(H, 64, generator=g) + 0.5, torch.rand(H, 64, generator=g) + 0.5
    u = torch.matmul(A.to(torch.float64), W.to(torch.float64).T) + b.to(torch.float64)
    got_u = GC.base64(A, W, b)
    close = lambda a, w: float((a - w).abs().max()) <= 1e-12 * float(w.abs().max())
    assert got_u.dtype == torch.float64 and close(got_u, u)
    x = u.reshape(M, 3, H, 64)
    qn = F.normalize(x[:, 0], dim=-1, eps=1e-12) * gq.double() * 1.5
    kn = F.normalize(x[:, 1], dim=-1, eps=1e-12) * gk.double() * 8.0
    want = {"bias": u, "resid": u + h.double(), "resid16": u + h.to(torch.float16).double(), "silu": F.silu(u), "relu": F.relu(u),
            "geglu": u[:, :Nn // 2] * F.gelu(u[:, Nn // 2:]), "anchor": u + torch.stack([emb[int(a)] for a in anchor]).double(),
            "qkv": x.permute(1, 2, 0, 3), "qkvnorm": torch.stack([qn, kn, x[:, 2]]).permute(0, 2, 1, 3)}
    assert set(want) == set(GC.F32_EPI.values()) | set(GC.H16_EPI.values()) | set(GC.X2_EPI.values())
    for name, w in want.items():
        got = GC.ref_epilogue(name, got_u, resid=h.to(torch.float16) if name == "resid16" else h, anchor=anchor, emb=emb, H=H, gq=gq, gk=gk, q_mul=1.5)
        assert got.shape == w.shape and got.dtype == torch.float64 and close(got, w), name
    plain = GC.ref_epilogue("qkvnorm", got_u, H=H)                      # gamma_q = gamma_k = NULL: no norm
    assert torch.equal(plain, want["qkv"])
