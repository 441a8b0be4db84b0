"""GPU: the edge sweep of the GEMM kernels through the C ABI -- row tails, k-tile counts, ragged M on the 256 x 256 kernels, the uneven
persistent tile walk, split-K edges and leading dimensions -- for the exact-fp32, the bf16 / fp16 and the split-precision family.

The cases are the tables of tests/gemm_cases.py; tests/test_gemm_cases_host.py pins (on the CPU) that each one reaches the kernel form it
is listed under, and every call here asks rap_gemm_*_form once more before it runs.  Every comparison is a FULL-matrix comparison with an
fp64 evaluation of the same formula on the same (rounded, for 16-bit) operands, on outputs that start as NaN (the in-place residual
epilogues start as the residual, as the model runs them) -- a tile the kernel never wrote, or wrote with another tile's rows, fails.  The
reference is formed on the CPU, or by torch in float64 on the device when M N K exceeds 1e9.  The bounds are the ones of
tests/test_kernels_gpu.py, test_h16_gpu.py and test_x2_gpu.py; split-K only re-associates the k-sum and gets the unsplit bound.

Every figure is printed before it is asserted (pytest -s).  Measured on an MI355X, worst over all 1 800 comparisons, as a fraction of
the bound: the one-rounding bounds of the 16-bit outputs 0.82 - 0.98 (a rounding error reaches its ULP by construction); fp32 GEGLU 0.95
(1.9e-5 of GEMM_BOUND at 16 640 x 2 048 x 288: the 4.5e-6 accumulation error of that shape times |h| up to 7 at the extremes of 17 M
outputs; 6.2e-6 at the row-tail shapes); every other fp32 epilogue at most 0.37 (7.4e-6, residual in place); fp32 outputs of the 16-bit
kernels at most 0.17; split precision at most 0.48 of X2_GEMM_BOUND / X2_GEGLU_BOUND.
"""
import ctypes

import pytest
import torch

import gemm_cases as GC
from rap_amd import _lib
from test_h16_gpu import F32_OUT_BOUND, GEGLU_ROUNDINGS, NORM_SLACK, ONE_ROUNDING, TORCH_DT, ULP, gemm_h, to_h, vt_pos
from test_kernels_gpu import GEMM_BOUND, gemm
from test_x2_gpu import X2_GEGLU_BOUND, X2_GEMM_BOUND, X2_QKV_BOUND, pack_dev, unpack_ref, weight_scale, x2_gemm

pytestmark = pytest.mark.gpu

Q_MUL = 8.0
DEVICE_REF_ABOVE = 1e9          # M N K above which torch forms the fp64 reference on the device


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def stream(dev):
    return _lib.current_stream(dev)


def sync():
    torch.cuda.synchronize()


def nan(dev, shape, dtype=torch.float32):
    return torch.full(tuple(shape), float("nan"), dtype=dtype, device=dev)


def bits(t):
    return t.contiguous().view(torch.uint8)


def interleave(lib, dev, W, b, inner, K):
    Wi, bi = torch.empty_like(W), torch.empty_like(b)
    _lib.check(lib.rap_geglu_interleave(_lib.ptr(W), _lib.ptr(b), _lib.ptr(Wi), _lib.ptr(bi), inner, K, stream(dev)), "interleave")
    sync()
    return Wi, bi


# ---------------------------------------------------------------------------------------------
# operands: one set per (family, N, K, heads), made once at the largest row count any case asks for and sliced by rows
# ---------------------------------------------------------------------------------------------
class Operands:
    def __init__(self, lib, dev, fam, N, K, H, rows):
        g = torch.Generator(device=dev).manual_seed(1000 + N + 7 * K + H)
        r = lambda *s: torch.randn(*s, device=dev, generator=g)
        self.fam, self.N, self.K, self.H, self.rows, self.dev = fam, N, K, H, rows, dev
        A, W = r(rows, K), r(N, K) / K ** 0.5 * (0.5 if fam == "x2" else 1.0)
        self.b = r(N) * (0.1 if fam == "x2" else 1.0)
        self.h = r(rows, N) * (1.0 if fam in ("f32", "x2") else 3.0)
        self.h16 = self.h.to(torch.float16)
        self.anchor = (torch.rand(rows, device=dev, generator=g) < 0.4).to(torch.uint8)
        self.emb = r(2, N)
        self.gq = torch.rand(max(H, 1), 64, device=dev, generator=g) + 0.5
        self.gk = torch.rand(max(H, 1), 64, device=dev, generator=g) + 0.5
        Wi, self.bi = interleave(lib, dev, W, self.b, N // 2, K)
        if fam == "f32":
            self.A, self.W, self.Wi = A, W, Wi
            self.A64, self.W64 = A, W                                  # what the fp64 reference multiplies
        elif fam == "x2":
            self.sc = weight_scale(W)
            self.A, self.W, self.Wi = pack_dev(lib, dev, A), pack_dev(lib, dev, W, self.sc), pack_dev(lib, dev, Wi, self.sc)
            self.A64, self.W64 = A, W                                  # fp32-accurate on the ORIGINAL operands
        else:
            dt = GC.DTYPE[fam]
            self.A, self.W, self.Wi = to_h(A, dt), to_h(W, dt), to_h(Wi, dt)
            self.A64, self.W64 = self.A, self.W                        # the ROUNDED operands
        self._u = (None, None)

    def where(self, M):
        return self.dev if float(M) * self.N * self.K > DEVICE_REF_ABOVE else torch.device("cpu")

    def u(self, M, bias=True):
        """A W^T (+ bias) of the first M rows in float64, on where(M); the product is kept until another M is asked for"""
        w = self.where(M)
        if self._u[0] != M:
            self._u = (None, None)
            self._u = (M, GC.base64(self.A64[:M].to(w), self.W64.to(w)))
        return self._u[1] + self.b.to(w).double() if bias else self._u[1]

    def scale(self, M):
        """max of sum |a w|: what an fp32 rounding of the product is relative to (the split-precision residual bound)"""
        w = self.where(M)
        return float((self.A64[:M].to(w).double().abs() @ self.W64.to(w).double().abs().T).max())


_OPS = {}


@pytest.fixture(scope="module", autouse=True)
def _free_the_operands_afterwards():
    """the cached operand sets hold a few hundred MB of device memory each: the files that run after this one get it back"""
    yield
    _OPS.clear()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


def operands(lib, dev, c, rows=None):
    rows = rows or (1024 if c.M <= 1024 else 16640)
    key = (c.fam, c.N, c.K, c.H, rows)
    if key not in _OPS:
        while len(_OPS) >= 3:                                           # a few sets at a time: the big ones hold a few hundred MB each
            _OPS.pop(next(iter(_OPS)))
        _OPS[key] = Operands(lib, dev, c.fam, c.N, c.K, c.H, rows)
    return _OPS[key]


# ---------------------------------------------------------------------------------------------
# one call of a case; outputs {"C": ..., "vt": ...}
# ---------------------------------------------------------------------------------------------
def vt_blocks(M):
    return (M + 255) // 256 * 256 // 64


def launch(lib, dev, c, o, M=None):
    M = c.M if M is None else M
    name, N, K, H = GC.epi_name(c), c.N, c.K, c.H
    assert GC.form_of(lib, c, M) == c.form or M != c.M, (c, GC.form_of(lib, c, M))          # the shape still reaches the kernel it is here for
    A, st = o.A[:M], stream(dev)
    vt = None
    if c.ws:
        return launch_splitk(lib, dev, c, o, M)
    if c.fam == "f32":
        if name == "geglu":
            C = nan(dev, (M, N // 2)); gemm(lib, dev, 3, A, o.Wi, C, M, N, K, bias=o.bi, ldc=N // 2)
        elif name == "qkv":
            C = nan(dev, (3, H, M, 64)); gemm(lib, dev, 4, A, o.W, C, M, N, K, heads=H)
        elif name == "resid":
            C = o.h[:M].clone(); gemm(lib, dev, 1, A, o.W, C, M, N, K, bias=o.b, resid=C)                 # in place, as the model runs it
        elif name == "anchor":
            C = nan(dev, (M, N)); gemm(lib, dev, 5, A, o.W, C, M, N, K, bias=o.b, anchor=o.anchor[:M], emb=o.emb)
        else:
            C = nan(dev, (M, N)); gemm(lib, dev, c.epi, A, o.W, C, M, N, K, bias=o.b)
    elif c.fam == "x2":
        if name == "resid":
            C = nan(dev, (M, N)); x2_gemm(lib, dev, 1, A, o.W, C, M, N, 2 * K, N, bias=o.b, resid=o.h[:M], acc_scale=1.0 / o.sc)
        elif name == "geglu":
            C = nan(dev, (M, N), torch.float16); x2_gemm(lib, dev, 3, A, o.Wi, C, M, N, 2 * K, N, bias=o.bi, acc_scale=1.0 / o.sc)
        else:
            C = nan(dev, (2, H, 2, M, 64), torch.float16); vt = nan(dev, (H, vt_blocks(M), 2, 64, 64), torch.float16)
            x2_gemm(lib, dev, 5, A, o.W, C, M, N, 2 * K, 0, acc_scale=1.0 / o.sc, heads=H, gq=o.gq, gk=o.gk, q_mul=Q_MUL, vt=vt, vt_nblk=vt_blocks(M))
    else:
        dt = GC.DTYPE[c.fam]
        hdt = TORCH_DT[dt]
        if name == "bias":
            C = nan(dev, (M, N), hdt); gemm_h(lib, dev, dt, 0, A, o.W, C, M, N, K, bias=o.b)
        elif name == "resid":
            C = nan(dev, (M, N)); gemm_h(lib, dev, dt, 1, A, o.W, C, M, N, K, bias=o.b, resid=o.h[:M])
        elif name == "resid16":
            C = o.h16[:M].clone(); gemm_h(lib, dev, dt, 7, A, o.W, C, M, N, K, bias=o.b, resid=C)          # in place: the 16-bit residual stream
        elif name == "geglu":
            C = nan(dev, (M, N // 2), hdt); gemm_h(lib, dev, dt, 3, A, o.Wi, C, M, N, K, bias=o.bi, ldc=N // 2)
        else:
            C = nan(dev, (2, H, M, 64), hdt); vt = nan(dev, (H, vt_blocks(M), 64, 64), hdt)
            if name == "qkv":
                gemm_h(lib, dev, dt, 4, A, o.W, C, M, N, K, heads=H, vt=vt, vt_nblk=vt_blocks(M))
            else:
                _lib.check(lib.rap_gemm_h16_qkvnorm(dt, _lib.ptr(A), K, _lib.ptr(o.W), K, _lib.ptr(C), M, K, H, _lib.ptr(o.gq), _lib.ptr(o.gk), Q_MUL,
                                                    _lib.ptr(vt), vt_blocks(M), st), "rap_gemm_h16_qkvnorm")
                sync()
    return {"C": C, "vt": vt}


def splitk_need(lib, c, M):
    if c.fam == "f32":
        return lib.rap_gemm_f32_splitk_workspace_bytes(c.epi, M, c.N, c.K, c.planes)
    return lib.rap_gemm_h16_splitk_workspace_bytes(M, c.N, c.K)


def call_splitk(lib, dev, c, a, w, C, ldc, bias, resid, M):
    """the split-K entry point of the case's family with EXACTLY the workspace it reports (none when the rule does not split)"""
    need = splitk_need(lib, c, M)
    assert need == (c.form % 10 if c.form % 10 > 1 else 0) * M * c.N * 4, (c, need)
    ws = torch.full((max(need, 1),), 0xFF, dtype=torch.uint8, device=dev)
    ldr = resid.stride(0) if resid is not None else 0
    if c.fam == "f32":
        rc = lib.rap_gemm_f32_splitk(c.epi, _lib.ptr(a), a.stride(0), _lib.ptr(w), w.stride(0), _lib.ptr(C), ldc, M, c.N, c.K, _lib.ptr(bias), _lib.ptr(resid),
                                     ldr, c.planes, _lib.ptr(ws) if need else ctypes.c_void_p(0), need, stream(dev))
    else:
        rc = lib.rap_gemm_h16_splitk(GC.DTYPE[c.fam], c.epi, _lib.ptr(a), a.stride(0), _lib.ptr(w), w.stride(0), _lib.ptr(C), ldc, M, c.N, c.K, _lib.ptr(bias),
                                     _lib.ptr(resid), ldr, _lib.ptr(ws) if need else ctypes.c_void_p(0), need, stream(dev))
    _lib.check(rc, "split-K entry point")
    sync()


def launch_splitk(lib, dev, c, o, M):
    name = GC.epi_name(c)
    if name == "silu":
        C = nan(dev, (M, c.N)); call_splitk(lib, dev, c, o.A[:M], o.W, C, c.N, o.b, None, M)
    elif name == "resid16":
        C = o.h16[:M].clone(); call_splitk(lib, dev, c, o.A[:M], o.W, C, c.N, o.b, C, M)
    elif c.fam == "f32":
        C = o.h[:M].clone(); call_splitk(lib, dev, c, o.A[:M], o.W, C, c.N, o.b, C, M)                   # bias + residual, in place
    else:
        C = nan(dev, (M, c.N)); call_splitk(lib, dev, c, o.A[:M], o.W, C, c.N, o.b, o.h[:M], M)
    return {"C": C, "vt": None}


# ---------------------------------------------------------------------------------------------
# the comparison with fp64
# ---------------------------------------------------------------------------------------------
def rel_err(got, ref):
    return ((got.double() - ref).abs() / (ref.abs() + 1e-2)).max().item()


def reference(c, o, M):
    name, w = GC.epi_name(c), o.where(M)
    on = lambda t: t.to(w)
    return GC.ref_epilogue(name, o.u(M, bias=name not in ("qkv", "qkvnorm")), resid=on((o.h16 if name == "resid16" else o.h)[:M]),
                           anchor=on(o.anchor[:M]), emb=on(o.emb), H=c.H, gq=on(o.gq), gk=on(o.gk), q_mul=Q_MUL)


def check_vt_h16(vt, want_v, M, bound, what):
    """vt [H][blk][64 d][64 pos]: token t at block t >> 6, position vt_pos(t & 63); rows M .. align_up(M, 256) read back as zeros"""
    vtc = vt.double()
    t = torch.arange(M, device=vt.device)
    got = vtc[:, t >> 6, :, vt_pos(t & 63)]                             # (M, H, 64)
    e = rel_err(got, want_v.permute(1, 0, 2))
    assert e < bound, (what, "V^T", e)
    tp = torch.arange(M, vt.shape[1] * 64, device=vt.device)
    if tp.numel():
        pad = vt[:, tp >> 6, :, vt_pos(tp & 63)]
        assert torch.equal(pad, torch.zeros_like(pad)), (what, "rows beyond M of the V^T image are not zeros")


def check_x2_qkv(c, C, vt, ref, M, what):
    """q, k: [2][H][2 chunks][M][64 physical] (chunk = head dims 32c .. 32c+31 as 32 heads | 32 tails); v: [H][blk][2 chunks][64 d][64 physical]"""
    got = torch.cat([C[:, :, ch, :, :32].double() + C[:, :, ch, :, 32:].double() for ch in range(2)], dim=-1)           # [2][H][M][64]
    e = float((got - ref[:2]).abs().max()) / float(ref[:2].abs().max())
    assert e < X2_QKV_BOUND, (what, "q/k", e)
    vsum = vt[..., :32].double() + vt[..., 32:].double()                # [H][blk][2][64 d][32 in-chunk positions]
    t = torch.arange(M, device=vt.device)
    pos = vt_pos(t & 63)
    gotv = vsum[:, t >> 6, pos >> 5, :, pos & 31]                       # (M, H, 64)
    want = ref[2].permute(1, 0, 2)
    ev = float((gotv - want).abs().max()) / float(want.abs().max())
    assert ev < X2_QKV_BOUND, (what, "V^T", ev)
    tile = GC.tile_rows(c.form)                                         # filler rows of the last row tile that was touched are zeros
    tp = torch.arange(M, (M + tile - 1) // tile * tile, device=vt.device)
    if tp.numel():
        pp = vt_pos(tp & 63)
        pad = torch.stack([vt[:, tp >> 6, pp >> 5, :, pp & 31], vt[:, tp >> 6, pp >> 5, :, 32 + (pp & 31)]])       # heads and tails
        assert torch.equal(pad, torch.zeros_like(pad)), (what, "filler rows of the V^T image are not zeros")


def verify(c, o, outs, M=None):
    """the outputs of one call of case c against fp64, under the project's bound for that family and epilogue"""
    M = c.M if M is None else M
    name, w = GC.epi_name(c), o.where(M)
    ref = reference(c, o, M)
    C = outs["C"].to(w)
    vt = None if outs["vt"] is None else outs["vt"].to(w)
    what = (c.fam, name, M, c.N, c.K, c.form)
    if c.fam == "f32":
        err = (C.double() - ref).abs().max().item()
        print(f"{what}: err {err:.3e} (bound {GEMM_BOUND * max(1.0, (c.K / 2048) ** 0.5):.3e})")
        assert err < GEMM_BOUND * max(1.0, (c.K / 2048) ** 0.5), (what, err)
    elif c.fam == "x2":
        if name == "resid":
            err = (C.double() - ref).abs().max().item() / o.scale(M)
            print(f"{what}: err {err:.3e} (bound {X2_GEMM_BOUND:.3e})")
            assert err < X2_GEMM_BOUND, (what, err)
        elif name == "geglu":
            err = float((unpack_ref(C, c.N // 2) - ref).abs().max()) / float(ref.abs().max())
            print(f"{what}: err {err:.3e} (bound {X2_GEGLU_BOUND:.3e})")
            assert err < X2_GEGLU_BOUND, (what, err)
        else:
            check_x2_qkv(c, C, vt, ref, M, what)
    else:
        dt = GC.DTYPE[c.fam]
        if name == "resid":
            err = (C.double() - ref).abs().max().item()
            print(f"{what}: err {err:.3e} (bound {F32_OUT_BOUND:.3e})")
            assert err < F32_OUT_BOUND, (what, err)
        elif name == "bias":
            err = ((C.double() - ref).abs() - ULP[dt] * ONE_ROUNDING * ref.abs()).max().item()            # one rounding on top of the fp32 accumulation
            print(f"{what}: err {err:.3e} (bound {F32_OUT_BOUND:.3e})")
            assert err < F32_OUT_BOUND, (what, err)
        elif name == "resid16":
            err = rel_err(C, ref)
            print(f"{what}: err {err:.3e} (bound {ONE_ROUNDING * ULP[2] + NORM_SLACK:.3e})")
            assert err < ONE_ROUNDING * ULP[2] + NORM_SLACK, (what, err)
        elif name == "geglu":
            err = rel_err(C, ref)
            print(f"{what}: err {err:.3e} (bound {GEGLU_ROUNDINGS * ULP[dt]:.3e})")
            assert err < GEGLU_ROUNDINGS * ULP[dt], (what, err)
        else:
            err = rel_err(C, ref[:2])
            bound = ONE_ROUNDING * ULP[dt] + (NORM_SLACK if name == "qkvnorm" else 0.0)
            print(f"{what}: err {err:.3e} (bound {bound:.3e})")
            assert err < bound, (what, err)
            check_vt_h16(vt, ref[2], M, ONE_ROUNDING * ULP[dt], what)


def same_bits(a, b, what):
    for k in ("C", "vt"):
        if a[k] is not None:
            assert torch.equal(bits(a[k]), bits(b[k])), (what, k)


def groups(cases):
    """(family, epilogue) -> its cases, in table order: one test each"""
    out = {}
    for c in cases:
        out.setdefault((c.fam, c.epi), []).append(c)
    return out


def ids(g):
    return [f"{fam}-{GC.epi_name(cs[0])}" for (fam, _), cs in g.items()]


# ---------------------------------------------------------------------------------------------
# 1. row tails on the 128 x 128 kernels
# ---------------------------------------------------------------------------------------------
ROW_TAIL = groups(GC.row_tail_cases())


@pytest.mark.parametrize("cases", list(ROW_TAIL.values()), ids=ids(ROW_TAIL))
def test_row_tails_on_the_128x128_kernels(lib, dev, cases):
    """M = 1 .. 385 around every multiple of the 32-row wave tile and the 128-row block tile, 1 and 3 (2 and 6) column tiles"""
    for c in cases:
        o = operands(lib, dev, c)
        verify(c, o, launch(lib, dev, c, o))


# ---------------------------------------------------------------------------------------------
# 2. k-tile counts on the four-stage ring; two stages give the same bits
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ["bf16", "f16", "x2"])
def test_ring_ktile_sweep_is_right_and_bit_identical_to_two_stages(lib, dev, fam):
    """1 .. 9 and 16 k-tiles of 64 physical columns through the four-stage ring (counted waits, a peeled last tile: fewer k-tiles than
    stages, exactly as many, one more, odd counts) at one row, a ragged second row tile and three row tiles; rap_set_tuning(18, 0) runs the
    same call on two stages -- same MFMA order, same epilogue: the same bits"""
    ring = [c for c in GC.ring_cases() if c.fam == fam and c.N == 256]
    for c in [c for c in ring if not c.tune]:
        twin = [t for t in ring if t.tune and (t.M, t.K) == (c.M, c.K)]
        assert len(twin) == 1 and twin[0].form == GC.F128_2
        o = operands(lib, dev, c)
        four = launch(lib, dev, c, o)
        with GC.tuned(lib, twin[0].tune):
            two = launch(lib, dev, twin[0], o)
        verify(c, o, four)
        same_bits(four, two, (fam, c.M, c.K))


@pytest.mark.parametrize("fam", ["bf16", "f16", "x2"])
def test_two_stage_kernel_at_its_natural_size(lib, dev, fam):
    """260 blocks (one more than the ring takes): one k-tile (K < 128, 16-bit only) and an odd count, ragged and full row tiles"""
    for c in [c for c in GC.ring_cases() if c.fam == fam and c.N == 512]:
        o = operands(lib, dev, c)
        verify(c, o, launch(lib, dev, c, o))


# ---------------------------------------------------------------------------------------------
# 3. ragged M on the 256 x 256 one-tile-per-block kernels, and one row tile below the threshold on 128 x 128
# ---------------------------------------------------------------------------------------------
RAGGED256 = groups(GC.ragged256_cases())


@pytest.mark.parametrize("cases", list(RAGGED256.values()), ids=ids(RAGGED256))
def test_ragged_m_on_the_256x256_one_tile_per_block_kernels(lib, dev, cases):
    """1, 127, 129 and 255 rows in the last row tile (clamped source rows, predicated stores) at 2, 3, 4, 8 and 9 k-tiles; the same
    operands one row tile below the tile-count threshold run on the 128 x 128 kernel and meet the same bound.  The 16-bit QKV epilogues also
    own the V^T image up to align_up(M, 256) rows: zeros beyond M."""
    for c in cases:
        o = operands(lib, dev, c)
        verify(c, o, launch(lib, dev, c, o))


# ---------------------------------------------------------------------------------------------
# 4. the persistent tile walk with unequal tile counts per block, and short K
# ---------------------------------------------------------------------------------------------
WALK = groups([c for c in GC.walk_cases() if not c.tune])


@pytest.mark.parametrize("cases", list(WALK.values()), ids=ids(WALK))
def test_uneven_persistent_walk_is_right_and_bit_identical_to_one_tile_per_block(lib, dev, cases):
    """520 (780) tiles on 256 blocks: eight (twelve) blocks walk one tile more than their neighbours and hand their last k-tiles over to a
    tile the others do not have; 512 (768) tiles beside it.  Full matrix against fp64, and the same bits with the persistent key off."""
    for c in cases:
        twin = [t for t in GC.walk_cases() if t.tune and (t.fam, t.epi, t.M, t.N, t.K) == (c.fam, c.epi, c.M, c.N, c.K)]
        assert len(twin) == 1 and twin[0].form == GC.F256
        o = operands(lib, dev, c)
        persistent = launch(lib, dev, c, o)
        with GC.tuned(lib, twin[0].tune):
            one_tile = launch(lib, dev, twin[0], o)
        verify(c, o, persistent)
        same_bits(persistent, one_tile, (c.fam, c.epi, c.M, c.K))


# ---------------------------------------------------------------------------------------------
# 5. split-K edges through the split-K entry points
# ---------------------------------------------------------------------------------------------
SPLITK = groups(GC.splitk_cases())


@pytest.mark.parametrize("cases", list(SPLITK.values()), ids=ids(SPLITK))
def test_splitk_edges_with_exactly_the_reported_workspace(lib, dev, cases):
    """Either side of the 64- and 128-tile edges of the rules, even and uneven k shares (fp32: 17 k-tiles over 4 blocks), k-tile counts the
    rule refuses (the call then runs unsplit with no workspace at all); each result against fp64 under the UNSPLIT bound, and the unsplit
    call (tuning key 6 = 0, same entry point, same workspace) under the same bound"""
    for c in cases:
        o = operands(lib, dev, c)
        split = launch(lib, dev, c, o)
        verify(c, o, split)
        with GC.tuned(lib, ((6, 0),)):
            unsplit = c._replace(form=GC.F128_2 if c.fam == "f32" else GC.F128_4)
            assert GC.form_of(lib, unsplit) == unsplit.form
            plain = launch_splitk(lib, dev, c, o, c.M)                  # (the reservation follows the shape: the same workspace is handed in)
        verify(c, o, plain)
        a, b = split["C"].double(), plain["C"].double()
        if c.form % 10 == 1:                                            # the rule did not split: the key changes nothing
            same_bits(split, plain, c)
        elif GC.epi_name(c) == "resid16":                               # the fp32 sums differ in the last places: at most the neighbouring fp16 value
            assert ((a - b).abs() / (b.abs() + 1e-2)).max().item() < 2.01 * ULP[2], c
        else:
            assert (a - b).abs().max().item() < (GEMM_BOUND if c.fam == "f32" else F32_OUT_BOUND), c


# ---------------------------------------------------------------------------------------------
# 6. leading dimensions: lda > K, ldw > K, ldc > N and an independent ldr give the bits of the contiguous call
# ---------------------------------------------------------------------------------------------
def slack_filled(src, extra):
    """src as the leading columns of a buffer `extra` columns wider whose other columns hold NaN (fp32) / 0x7FFF (16-bit: a NaN too)"""
    rows, cols = src.shape
    if src.dtype == torch.float32:
        wide = torch.full((rows, cols + extra), float("nan"), device=src.device)
    else:
        wide = torch.full((rows, cols + extra), 0x7FFF, dtype=torch.int16, device=src.device).view(src.dtype)
    wide[:, :cols] = src
    return wide[:, :cols]


def resid_call(lib, dev, c, a, w, C, ldc, bias, resid, o):
    M = c.M
    if c.ws:
        call_splitk(lib, dev, c, a, w, C, ldc, bias, resid, M)
    elif c.fam == "f32":
        gemm(lib, dev, 1, a, w, C, M, c.N, c.K, bias=bias, resid=resid, ldc=ldc)
    elif c.fam == "x2":
        x2_gemm(lib, dev, 1, a, w, C, M, c.N, 2 * c.K, ldc, bias=bias, resid=resid, acc_scale=1.0 / o.sc)
    else:
        gemm_h(lib, dev, GC.DTYPE[c.fam], 1, a, w, C, M, c.N, c.K, bias=bias, resid=resid, ldc=ldc)


LD = GC.ld_cases()
assert all(c.ws for c in LD if GC.epi_name(c) != "resid")               # resid_call: anything but bias + residual goes through call_splitk


@pytest.mark.parametrize("c", LD, ids=[f"{c.fam}-{c.form}-M{c.M}-K{c.K}" for c in LD])
def test_leading_dimensions_give_the_bits_of_the_contiguous_call(lib, dev, c):
    """A and W as column slices of wider buffers (lda = K + 64, ldw = K + 128 physical columns, the slack NaN), C with ldc = N + 64 and a
    separate residual with ldr = N + 128: the bias + residual epilogue of every family and form (and the bias + SiLU epilogue of the fp32
    two-plane split form), bit for bit the contiguous call; the columns between the rows of C stay untouched"""
    assert GC.form_of(lib, c) == c.form
    o = operands(lib, dev, c)
    M, Nn = c.M, c.N
    silu = GC.epi_name(c) == "silu"                                      # (the SiLU split form has no residual: lda, ldw and ldc only)
    a, w, h = o.A[:M], o.W, None if silu else o.h[:M]
    plain = nan(dev, (M, Nn))
    resid_call(lib, dev, c, a, w, plain, Nn, o.b, h, o)
    verify(c, o, {"C": plain, "vt": None})
    a2, w2, h2 = slack_filled(a, 64), slack_filled(w, 128), None if silu else slack_filled(h, 128)
    assert a2.stride(0) == a.shape[1] + 64 and w2.stride(0) == w.shape[1] + 128 and (silu or h2.stride(0) == Nn + 128)
    wide = nan(dev, (M, Nn + 64))
    resid_call(lib, dev, c, a2, w2, wide, Nn + 64, o.b, h2, o)
    assert torch.equal(bits(wide[:, :Nn]), bits(plain))
    assert bool(torch.isnan(wide[:, Nn:]).all())
