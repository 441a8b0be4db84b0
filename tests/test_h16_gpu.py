"""GPU tests of the reduced-precision (bf16 / fp16 MFMA, fp32 accumulate) twins of the transformer-block kernels,
through the C ABI.

What is compared with what:
  * kernel level: the kernel on 16-bit operands vs an fp64 evaluation of the same formula ON THE SAME ROUNDED
    OPERANDS -- the difference is accumulation order plus the rounding of 16-bit outputs, so the bounds are a few
    ulps of the output type (bf16 ulp 2^-8 relative, fp16 2^-11) or fp32-class for fp32 outputs;
  * model level: velocity / sampling results vs the fp32 golden vectors of the reference; north_star asks for a
    MEASURED deviation for the bf16 path, not a fixed bar -- the asserted bounds below are
    what was measured on MI355X with margin, and the measured values are printed.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import rap_amd
from conftest import load_golden
from oracle import rap_oracle as O
from rap_amd import _lib, synthetic as S
from rap_amd.flow_model import workspace

pytestmark = pytest.mark.gpu
RAP_ERR_WORKSPACE = -2

TORCH_DT = {1: torch.bfloat16, 2: torch.float16}
ULP = {1: 2.0 ** -8, 2: 2.0 ** -11}     # largest relative error of one round-to-nearest into the type
# the bounds of this file's kernel-level comparisons with fp64 on the rounded operands (stated per test below); tests/test_guards_gpu.py
# holds the same calls to them
F32_OUT_BOUND = 2e-5     # fp32 outputs: exact products, fp32 accumulation of K O(1/sqrt(K)) terms
ONE_ROUNDING = 1.01      # x ULP[dt]: one rounding into the output type, relative to |ref| + 1e-2
GEGLU_ROUNDINGS = 1.2    # x ULP[dt]
NORM_SLACK = 1e-4        # added where the rounded value was normalised / accumulated in fp32 first
ATTN_ULPS = 8            # x ULP[dt], absolute, on |v| ~ 4: P rounded before P V and the output rounded once more


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def stream(dev):
    return _lib.current_stream(dev)


def vt_pos(t):
    return (t & ~12) | ((t & 4) << 1) | ((t & 8) >> 1)


def to_h(x, dt):
    """fp32 tensor -> rounded 16-bit tensor (torch's RNE == v_cvt_pk_*)"""
    return x.to(TORCH_DT[dt])


def gemm_h(lib, dev, dt, epi, A, W, C, M, N, K, bias=None, resid=None, heads=0, vt=None, vt_nblk=0, ldc=None):
    rc = lib.rap_gemm_h16(dt, epi, _lib.ptr(A), A.stride(0), _lib.ptr(W), W.stride(0), _lib.ptr(C), ldc if ldc else N, M, N, K,
                          _lib.ptr(bias), _lib.ptr(resid), resid.stride(0) if resid is not None else 0, heads, _lib.ptr(vt),
                          vt_nblk, stream(dev))
    _lib.check(rc, "rap_gemm_h16")
    torch.cuda.synchronize()


# Kernels that ship (gemm_h16.hip: launch_variant): the phase-split 256 x 256 kernel (persistent for full-tile shapes with >= 512 tiles and
# K <= 2048; one tile per block from 256 tiles on) and the two-stage 128 x 128 kernel for everything else -- the shapes of this file reach
# all three (the small parity shapes the 128 x 128 kernel; the full-size / persistent tests the other two).
# ---------------------------------------------------------------------------------------------
# conversion, GEMM
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [1, 2])
def test_convert_is_round_to_nearest_even(lib, dev, dt):
    g = torch.Generator().manual_seed(1)
    x = torch.cat([torch.randn(4096, generator=g) * 10.0 ** torch.randint(-6, 5, (4096,), generator=g).float(),
                   torch.tensor([0.0, -0.0, 1.0, 1.00390625, 1.001953125, 65504.0, 1e-8, -3.0])])
    x = x[: x.numel() // 4 * 4].contiguous()
    out = torch.empty(x.numel(), dtype=torch.int16, device=dev)
    xd = x.to(dev)     # keep every device operand alive until the synchronize (the caching allocator recycles temporaries)
    _lib.check(lib.rap_convert_h16(dt, _lib.ptr(xd), _lib.ptr(out), x.numel(), stream(dev)), "convert")
    torch.cuda.synchronize()
    ref = to_h(x, dt).view(torch.int16)
    assert torch.equal(out.cpu(), ref)


@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("M,N,K", [(1, 256, 64), (100, 256, 128), (300, 512, 512), (1000, 512, 2048), (257, 1536, 512)])
def test_gemm_h16_fp32_out_matches_fp64_on_rounded_operands(lib, dev, dt, M, N, K):
    g = torch.Generator().manual_seed(M * 7 + N + K)
    A = to_h(torch.randn(M, K, generator=g), dt); W = to_h(torch.randn(N, K, generator=g) / K ** 0.5, dt)
    b = torch.randn(N, generator=g); h = torch.randn(M, N, generator=g)
    ref = A.double() @ W.double().T + b.double()
    C = torch.full((M, N), float("nan"), device=dev)
    gemm_h(lib, dev, dt, 1, A.to(dev), W.to(dev), C, M, N, K, bias=b.to(dev))
    # exact products (16-bit x 16-bit fits fp32), fp32 accumulation of K O(1/sqrt(K)) terms
    assert (C.cpu().double() - ref).abs().max().item() < F32_OUT_BOUND
    C = h.to(dev).clone()
    gemm_h(lib, dev, dt, 1, A.to(dev), W.to(dev), C, M, N, K, bias=b.to(dev), resid=C)      # in place
    assert (C.cpu().double() - (ref + h.double())).abs().max().item() < F32_OUT_BOUND
    # 16-bit output
    Ch = torch.full((M, N), float("nan"), dtype=TORCH_DT[dt], device=dev)
    gemm_h(lib, dev, dt, 0, A.to(dev), W.to(dev), Ch, M, N, K, bias=b.to(dev))
    err = (Ch.cpu().double() - ref).abs() - ULP[dt] * 1.01 * ref.abs()     # one rounding into the output type ...
    assert err.max().item() < 2e-5, err.max().item()                       # ... on top of the fp32 accumulation error


@pytest.mark.parametrize("dt", [1, 2])
def test_gemm_h16_is_transpose_safe_identity_check(lib, dev, dt):
    """A = I with an asymmetric W catches a swapped row/col in the MFMA C/D mapping and a wrong k-slot order."""
    K = 256; N = 256; M = 256
    A = to_h(torch.eye(M, K), dt)
    W = to_h((torch.arange(N * K, dtype=torch.float32).reshape(N, K) % 251) / 64.0, dt)     # exactly representable
    C = torch.empty((M, N), device=dev)
    gemm_h(lib, dev, dt, 1, A.to(dev), W.to(dev), C, M, N, K)
    assert torch.equal(C.cpu(), W.float().T.contiguous())


@pytest.mark.parametrize("dt", [1, 2])
def test_gemm_h16_geglu(lib, dev, dt):
    g = torch.Generator().manual_seed(4)
    M, K, inner = 200, 128, 256
    A = torch.randn(M, K, generator=g); W = torch.randn(2 * inner, K, generator=g) / K ** 0.5; b = torch.randn(2 * inner, generator=g)
    Wd, bd = W.to(dev), b.to(dev)
    Wp, bp = torch.empty_like(Wd), torch.empty_like(bd)
    _lib.check(lib.rap_geglu_interleave(_lib.ptr(Wd), _lib.ptr(bd), _lib.ptr(Wp), _lib.ptr(bp), inner, K, stream(dev)), "interleave")
    Ah, Wh, Wph = to_h(A, dt), to_h(W, dt), to_h(Wp.cpu(), dt)
    u = Ah.double() @ Wh.double().T + b.double()
    ref = u[:, :inner] * F.gelu(u[:, inner:])
    C = torch.full((M, inner), float("nan"), dtype=TORCH_DT[dt], device=dev)
    gemm_h(lib, dev, dt, 3, Ah.to(dev), Wph.to(dev), C, M, 2 * inner, K, bias=bp, ldc=inner)
    err = (C.cpu().double() - ref).abs() / (ref.abs() + 1e-2)
    assert err.max().item() < GEGLU_ROUNDINGS * ULP[dt], err.max().item()


@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("M", [150, 256, 1000])
def test_gemm_h16_qkv_split_and_transposed_v(lib, dev, dt, M):
    g = torch.Generator().manual_seed(5)
    H, K = 4, 128                      # N = 768: a multiple of every tile width
    N = 3 * H * 64
    A = to_h(torch.randn(M, K, generator=g), dt); W = to_h(torch.randn(N, K, generator=g) / K ** 0.5, dt)
    ref = (A.double() @ W.double().T).reshape(M, 3, H, 64).permute(1, 2, 0, 3)   # [3][H][M][64]
    nblk = (M + 255) // 256 * 256 // 64
    qk = torch.full((2, H, M, 64), float("nan"), dtype=TORCH_DT[dt], device=dev)
    vt = torch.full((H, nblk, 64, 64), float("nan"), dtype=TORCH_DT[dt], device=dev)
    gemm_h(lib, dev, dt, 4, A.to(dev), W.to(dev), qk, M, N, K, heads=H, vt=vt, vt_nblk=nblk)
    err = (qk.cpu().double() - ref[:2]).abs() / (ref[:2].abs() + 1e-2)
    assert err.max().item() < ONE_ROUNDING * ULP[dt], err.max().item()
    # vt[h][t >> 6][d][vt_pos(t & 63)] == v[h][t][d]; padding rows of every M tile that was touched are zero
    vtc = vt.cpu().double()
    t = torch.arange(M)
    got = vtc[:, t >> 6, :, vt_pos(t & 63)]            # (M, H, 64): advanced indices first
    want = ref[2].permute(1, 0, 2)                     # (M, H, 64)
    errv = (got - want).abs() / (want.abs() + 1e-2)
    assert errv.max().item() < ONE_ROUNDING * ULP[dt], errv.max().item()
    m_tiles = 256 if ((M + 255) // 256) * (1536 // 256) >= 256 else 128      # which kernel ran (launch_variant): rows up to its M tile are written
    tp = torch.arange(M, (M + m_tiles - 1) // m_tiles * m_tiles)
    if tp.numel():
        pad = vtc[:, tp >> 6, :, vt_pos(tp & 63)]
        assert torch.equal(pad, torch.zeros_like(pad))


@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("M,K,q_mul", [(256, 128, 8.0), (1000, 512, 1.4426950408889634), (37, 192, 8.0)])
def test_gemm_h16_qkv_with_fused_qknorm(lib, dev, dt, M, K, q_mul):
    """EPI_H_QKV_NORM: q and k = MultiHeadRMSNorm(x W^T) (norm.py:28-33: normalize * gamma * 8; q times q_mul / 8 instead) from the fp32
    accumulators, rounded once; v exactly as the un-fused epilogue.  Reference: fp64 on the same rounded operands."""
    _check_gemm_h16_qkv_with_fused_qknorm(lib, dev, dt, M, K, q_mul, 4)


@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("M", [37, 1000])
@pytest.mark.parametrize("H", [12, 16])
def test_gemm_h16_qkv_with_fused_qknorm_at_other_head_counts(lib, dev, dt, M, H):
    """N = 192 H at the head counts of d = 768 / 1024 (K = d): a few-row M (128 x 128 tiles) and an M that is not a multiple of 256"""
    _check_gemm_h16_qkv_with_fused_qknorm(lib, dev, dt, M, 64 * H, 8.0, H)


def _check_gemm_h16_qkv_with_fused_qknorm(lib, dev, dt, M, K, q_mul, H):
    g = torch.Generator().manual_seed(15)
    N = 3 * H * 64
    A = to_h(torch.randn(M, K, generator=g), dt); W = to_h(torch.randn(N, K, generator=g) / K ** 0.5, dt)
    gq, gk = torch.rand(H, 64, generator=g) + 0.5, torch.rand(H, 64, generator=g) + 0.5
    x = (A.double() @ W.double().T).reshape(M, 3, H, 64).permute(1, 2, 0, 3)        # [3][H][M][64]
    nrm = x[:2].norm(dim=-1, keepdim=True).clamp_min(1e-12)
    mul = torch.tensor([q_mul, 8.0], dtype=torch.float64)[:, None, None, None]
    ref_qk = x[:2] / nrm * torch.stack([gq, gk])[:, :, None, :].double() * mul
    nblk = (M + 255) // 256 * 256 // 64
    qk = torch.full((2, H, M, 64), float("nan"), dtype=TORCH_DT[dt], device=dev)
    vt = torch.full((H, nblk, 64, 64), float("nan"), dtype=TORCH_DT[dt], device=dev)
    Ad, Wd, gqd, gkd = A.to(dev), W.to(dev), gq.to(dev), gk.to(dev)
    rc = lib.rap_gemm_h16_qkvnorm(dt, _lib.ptr(Ad), K, _lib.ptr(Wd), K, _lib.ptr(qk), M, K, H, _lib.ptr(gqd), _lib.ptr(gkd), float(q_mul),
                                  _lib.ptr(vt), nblk, stream(dev))
    _lib.check(rc, "rap_gemm_h16_qkvnorm")
    torch.cuda.synchronize()
    err = (qk.cpu().double() - ref_qk).abs() / (ref_qk.abs() + 1e-2)
    assert err.max().item() < ONE_ROUNDING * ULP[dt] + NORM_SLACK, err.max().item()            # one rounding of the normalised value
    vtc = vt.cpu().double()
    t = torch.arange(M)
    got = vtc[:, t >> 6, :, vt_pos(t & 63)]
    want = x[2].permute(1, 0, 2)
    errv = (got - want).abs() / (want.abs() + 1e-2)
    assert errv.max().item() < ONE_ROUNDING * ULP[dt], errv.max().item()
    tp = torch.arange(M, (M + 255) // 256 * 256)
    if tp.numel():
        pad = vtc[:, tp >> 6, :, vt_pos(tp & 63)]
        assert torch.equal(pad, torch.zeros_like(pad))


@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("M,K", [(100, 512), (1000, 512), (777, 2048)])
def test_gemm_h16_fp16_residual_epilogue(lib, dev, dt, M, K):
    """Epilogue 7 (the residual GEMMs of the 16-bit residual stream): C fp16 = fp16(resid fp16 + A W^T + bias), in place, the sum
    formed in fp32 and rounded ONCE -- within one fp16 rounding of the fp64 evaluation on the same rounded operands, for both operand
    dtypes and both shipped kernels (M <= 128: 128 x 128 tiles; above: the phase-split 256 x 256 kernel)."""
    g = torch.Generator().manual_seed(41)
    N = 512
    A = to_h(torch.randn(M, K, generator=g), dt); W = to_h(torch.randn(N, K, generator=g) / K ** 0.5, dt)
    bias = torch.randn(N, generator=g)
    h0 = (torch.randn(M, N, generator=g) * 3).to(torch.float16)
    ref = h0.double() + A.double() @ W.double().T + bias.double()
    Ad, Wd, bd, hd = A.to(dev), W.to(dev), bias.to(dev), h0.to(dev).clone()
    gemm_h(lib, dev, dt, 7, Ad, Wd, hd, M, N, K, bias=bd, resid=hd)
    err = (hd.cpu().double() - ref).abs() / (ref.abs() + 1e-2)
    assert err.max().item() < ONE_ROUNDING * ULP[2] + NORM_SLACK, err.max().item()      # ULP[2]: one fp16 rounding (+ fp32 accumulation noise)
    # the stream SATURATES instead of overflowing to inf (round 4): residual rows near the fp16 maximum plus a positive
    # product stay at +-65504 (and finite values below it are untouched, as the comparison above shows)
    big = torch.full((M, N), 65000.0).to(torch.float16); big[::2] = -65000.0
    sgn = torch.where(torch.arange(M) % 2 == 0, -1.0, 1.0)[:, None]
    A2 = to_h(torch.ones(M, K) * sgn, dt); W2 = to_h(torch.full((N, K), 4.0), dt)         # |A W^T| = 4 K >= 2048: the sum leaves the fp16 range
    A2d, W2d, bigd = A2.to(dev), W2.to(dev), big.to(dev).clone()
    gemm_h(lib, dev, dt, 7, A2d, W2d, bigd, M, N, K, resid=bigd)
    assert torch.isfinite(bigd).all() and bool((bigd.abs().float() == 65504.0).all())
    assert bool((torch.sign(bigd.float()) == sgn.to(dev)).all())
    # ... and NaN stays NaN (round 5, ADVICE r04: v_med3_f32 alone returns the minimum of the other two operands for a NaN input, i.e. the
    # saturation laundered a NaN of the stream into -65504 where the reference's fp16 arithmetic propagates it): a NaN in the residual
    # and a NaN in the operands both reach the output; the finite rows next to them are untouched
    h1 = (torch.randn(M, N, generator=g) * 3).to(torch.float16)
    h1[1, 5] = float("nan")
    A3 = A.clone(); A3[3, 7] = float("nan")
    ref3 = h1.double() + A3.double() @ W.double().T + bias.double()
    A3d, h1d = A3.to(dev), h1.to(dev).clone()
    gemm_h(lib, dev, dt, 7, A3d, Wd, h1d, M, N, K, bias=bd, resid=h1d)
    out3 = h1d.cpu()
    assert torch.isnan(out3[1, 5]) and bool(torch.isnan(out3[3]).all())
    keep = torch.ones(M, N, dtype=torch.bool); keep[1, 5] = False; keep[3] = False
    assert bool(torch.isfinite(out3[keep]).all())
    err3 = ((out3.double() - ref3).abs() / (ref3.abs() + 1e-2))[keep]
    assert err3.max().item() < 1.01 * ULP[2] + 1e-4
    # the epilogue needs its residual: without one the call is refused (a plain fp16-output GEMM is epilogue 0 with dtype fp16)
    rc = lib.rap_gemm_h16(dt, 7, _lib.ptr(Ad), K, _lib.ptr(Wd), K, _lib.ptr(hd), N, M, N, K, _lib.ptr(bd), _lib.ptr(None), 0, 0, _lib.ptr(None), 0,
                          stream(dev))
    assert rc == -1


@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("epi,M,N,K", [(0, 16384, 2048, 512), (1, 65536, 512, 2048), (3, 16384, 2048, 512), (4, 32768, 1536, 512),
                                       (5, 32768, 1536, 512), (7, 65536, 512, 512), (7, 65536, 512, 128)])
def test_persistent_gemm_is_bit_identical_to_the_one_tile_per_block_kernel(lib, dev, dt, epi, M, N, K):
    """Round 3: full-tile shapes (M % 256 == 0, at least 512 tiles) run on the PERSISTENT phase-split kernel (one block per CU walks its
    XCD's tiles, the k-tiles of consecutive output tiles form one DMA stream); rap_set_tuning(11, 0) restores one 256 x 256 tile per
    block.  Same MFMA order, same epilogue arithmetic: every epilogue must come out BIT-identical (the one-tile kernel's own parity
    with fp64 is the subject of the tests above).  Random rows are also checked against fp64 directly."""
    g = torch.Generator(device=dev).manual_seed(100 + epi)
    A = to_h(torch.randn(M, K, device=dev, generator=g), dt); W = to_h(torch.randn(N, K, device=dev, generator=g) / K ** 0.5, dt)
    bias = torch.randn(N, device=dev, generator=g)
    H = 8
    nblk = M // 64
    gq = torch.rand(H, 64, device=dev, generator=g) + 0.5; gk = torch.rand(H, 64, device=dev, generator=g) + 0.5
    outs = []
    try:
        for persistent in (1, 0):
            assert lib.rap_set_tuning(11, persistent) == 0
            vt = None
            if epi == 0:
                C = torch.zeros(M, N, dtype=TORCH_DT[dt], device=dev); gemm_h(lib, dev, dt, 0, A, W, C, M, N, K, bias=bias)
            elif epi == 1:
                g2 = torch.Generator(device=dev).manual_seed(5)
                C = torch.randn(M, N, device=dev, generator=g2); gemm_h(lib, dev, dt, 1, A, W, C, M, N, K, bias=bias, resid=C)
            elif epi == 7:
                g2 = torch.Generator(device=dev).manual_seed(5)
                C = torch.randn(M, N, device=dev, generator=g2).to(torch.float16); gemm_h(lib, dev, dt, 7, A, W, C, M, N, K, bias=bias, resid=C)
            elif epi == 3:
                C = torch.zeros(M, N // 2, dtype=TORCH_DT[dt], device=dev); gemm_h(lib, dev, dt, 3, A, W, C, M, N, K, bias=bias, ldc=N // 2)
            else:
                C = torch.zeros(2, H, M, 64, dtype=TORCH_DT[dt], device=dev)
                vt = torch.zeros(H, nblk, 64, 64, dtype=TORCH_DT[dt], device=dev)
                if epi == 4:
                    gemm_h(lib, dev, dt, 4, A, W, C, M, N, K, heads=H, vt=vt, vt_nblk=nblk, ldc=2 * H * 64)
                else:
                    _lib.check(lib.rap_gemm_h16_qkvnorm(dt, _lib.ptr(A), K, _lib.ptr(W), K, _lib.ptr(C), M, K, H, _lib.ptr(gq), _lib.ptr(gk), 8.0,
                                                        _lib.ptr(vt), nblk, stream(dev)), "qkvnorm")
                    torch.cuda.synchronize()
            outs.append((C.clone(), None if vt is None else vt.clone()))
    finally:
        assert lib.rap_set_tuning(11, 1) == 0
    (c1, v1), (c0, v0) = outs
    assert torch.equal(c1.view(torch.int16) if c1.dtype != torch.float32 else c1, c0.view(torch.int16) if c0.dtype != torch.float32 else c0)
    if v1 is not None:
        assert torch.equal(v1.view(torch.int16), v0.view(torch.int16))
    if epi in (0, 1, 7):                         # spot check against fp64 on rows from every part of the tile walk
        rows = torch.randint(0, M, (64,), generator=torch.Generator().manual_seed(3)).to(dev)
        ref = A[rows].double() @ W.double().T + bias.double()
        if epi != 0:
            g2 = torch.Generator(device=dev).manual_seed(5)
            r0 = torch.randn(M, N, device=dev, generator=g2)
            ref = ref + (r0.to(torch.float16) if epi == 7 else r0)[rows].double()
        if epi == 1:                             # fp32 out: absolute error of the fp32 accumulation of K exact 16-bit products
            err = (c1[rows].double() - ref).abs().max().item()
            assert err < 5e-5 * max(1.0, K / 512), err
        else:
            err = ((c1[rows].double() - ref).abs() / (ref.abs() + 1e-2)).max().item()
            assert err < 1.01 * ULP[dt if epi == 0 else 2] + 1e-4, err


@pytest.mark.parametrize("dt", [1, 2])
def test_gemm_h16_full_size_linearity_property(lib, dev, dt):
    """BASELINE configs[1]/[2] row count: C(A1 + A2) == C(A1) + C(A2) when A1, A2 have disjoint supports (exact in any
    arithmetic: every product is either x*w or 0*w), plus agreement with the exact-fp32 GEMM on the same rounded data."""
    M, N, K = 262144, 512, 512
    g = torch.Generator(device=dev).manual_seed(0)
    A = torch.randn(M, K, device=dev, generator=g); W = torch.randn(N, K, device=dev, generator=g) / K ** 0.5
    Ah, Wh = to_h(A, dt), to_h(W, dt)
    mask = (torch.rand(M, K, device=dev, generator=g) < 0.5)
    A1, A2 = torch.where(mask, Ah, torch.zeros_like(Ah)), torch.where(mask, torch.zeros_like(Ah), Ah)
    C, C1, C2, Cf = (torch.empty(M, N, device=dev) for _ in range(4))
    gemm_h(lib, dev, dt, 1, Ah, Wh, C, M, N, K)
    gemm_h(lib, dev, dt, 1, A1, Wh, C1, M, N, K)
    gemm_h(lib, dev, dt, 1, A2, Wh, C2, M, N, K)
    assert (C - (C1 + C2)).abs().max().item() < 2e-5
    Af, Wf = Ah.float(), Wh.float()
    _lib.check(lib.rap_gemm_f32(0, _lib.ptr(Af), K, _lib.ptr(Wf), K, _lib.ptr(Cf), N, M, N, K, _lib.ptr(None), _lib.ptr(None), 0,
                                _lib.ptr(None), _lib.ptr(None), 0, stream(dev)), "gemm_f32")
    torch.cuda.synchronize()
    assert (C - Cf).abs().max().item() < 2e-5


@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("epi", [1, 7], ids=["fp32-stream", "fp16-stream"])
@pytest.mark.parametrize("M,splits", [(100, 4), (2048, 4), (3000, 2), (9000, 1)])
def test_gemm_h16_splitk_of_the_residual_gemm(lib, dev, dt, epi, M, splits):
    """Few-token calls (round 3): ff2 (N = 512, K = 2048) has at most 128 tiles of 128 x 128 and a chain of 32 k-tiles per tile, so K is
    split over 4 (<= 64 tiles) or 2 blocks per tile and a combine pass forms resid + (bias + partials) in a fixed order.  Checked: the
    split count the workspace query implies, the result within one rounding of the fp64 evaluation, agreement with the unsplit kernel
    (tuning key 6 = 0) to fp32-association level, run-to-run determinism, and that a short workspace is refused."""
    _check_gemm_h16_splitk_of_the_residual_gemm(lib, dev, dt, epi, M, 512, 2048, splits)


# ff2 of the other model widths: N = d, K = 4 d = 1024 / 3072 / 4096, at M that give 4, 2 and 1 splits
WIDTH_FF2 = [(100, 256, 1024, 4), (5000, 256, 1024, 2), (300, 768, 3072, 4), (2048, 768, 3072, 2), (777, 1024, 4096, 4),
             (2048, 1024, 4096, 2), (3000, 1024, 4096, 1)]


@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("epi", [1, 7], ids=["fp32-stream", "fp16-stream"])
@pytest.mark.parametrize("M,N,K,splits", WIDTH_FF2, ids=[f"M{m}-N{n}-K{k}" for m, n, k, _ in WIDTH_FF2])
def test_gemm_h16_splitk_of_the_residual_gemm_at_other_widths(lib, dev, dt, epi, M, N, K, splits):
    _check_gemm_h16_splitk_of_the_residual_gemm(lib, dev, dt, epi, M, N, K, splits)


def _check_gemm_h16_splitk_of_the_residual_gemm(lib, dev, dt, epi, M, N, K, splits):
    g = torch.Generator().manual_seed(43)
    need = lib.rap_gemm_h16_splitk_workspace_bytes(M, N, K)
    assert need == (splits * M * N * 4 if splits > 1 else 0)
    A = to_h(torch.randn(M, K, generator=g), dt); W = to_h(torch.randn(N, K, generator=g) / K ** 0.5, dt)
    bias = torch.randn(N, generator=g)
    h0 = (torch.randn(M, N, generator=g) * 3)
    h0 = h0.to(torch.float16) if epi == 7 else h0
    ref = h0.double() + A.double() @ W.double().T + bias.double()
    Ad, Wd, bd = A.to(dev), W.to(dev), bias.to(dev)
    ws = workspace(dev, max(need, 256))
    bits = torch.int16 if epi == 7 else torch.int32

    def run(ws_bytes=None):
        hd = h0.to(dev).clone()
        rc = lib.rap_gemm_h16_splitk(dt, epi, _lib.ptr(Ad), K, _lib.ptr(Wd), K, _lib.ptr(hd), N, M, N, K, _lib.ptr(bd), _lib.ptr(hd), N,
                                     _lib.ptr(ws), ws.numel() if ws_bytes is None else ws_bytes, stream(dev))
        torch.cuda.synchronize()
        return rc, hd.cpu()

    rc, out = run()
    assert rc == 0
    if epi == 7:
        err = (out.double() - ref).abs() / (ref.abs() + 1e-2)
        assert err.max().item() < ONE_ROUNDING * ULP[2] + NORM_SLACK, err.max().item()     # one fp16 rounding (+ fp32 accumulation noise)
    else:
        assert (out.double() - ref).abs().max().item() < F32_OUT_BOUND               # fp32 accumulation of K exact products
    rc2, out2 = run()
    assert rc2 == 0 and torch.equal(out.view(bits), out2.view(bits))
    try:
        assert lib.rap_set_tuning(6, 0) == 0
        assert lib.rap_gemm_h16_splitk_workspace_bytes(M, N, K) == need      # round 4: the reservation follows the SHAPE; key 6 gates the launch
        rc3, unsplit = run()
    finally:
        assert lib.rap_set_tuning(6, 1) == 0
    assert rc3 == 0
    if epi == 7:
        d = (out.double() - unsplit.double()).abs() / (ref.abs() + 1e-2)
        assert d.max().item() < 2.01 * ULP[2], d.max().item()                # at most the neighbouring fp16 value
    else:
        assert (out.double() - unsplit.double()).abs().max().item() < 1e-5   # the k-sum re-associated
    if splits > 1:
        assert run(ws_bytes=need - 4)[0] == RAP_ERR_WORKSPACE


# ---------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------
def pack_qkv(q, k, v, dt, dev):
    """q,k,v (H,TP,64) fp32 -> (qk [2][H][TP][64], vt [H][nblk][64][64], nblk) as the QKV GEMM epilogue writes them."""
    H, TP, _ = q.shape
    nblk = (TP + 255) // 256 * 256 // 64
    qk = torch.stack([to_h(q, dt), to_h(k, dt)]).contiguous().to(dev)
    vt = torch.zeros((H, nblk, 64, 64), dtype=TORCH_DT[dt])
    t = torch.arange(TP)
    vt[:, t >> 6, :, vt_pos(t & 63)] = to_h(v, dt).permute(1, 0, 2)
    return qk, vt.to(dev), nblk


def run_attention_h(lib, dev, dt, q, k, v, cu, bound=None):
    H, TP, _ = q.shape
    qk, vt, nblk = pack_qkv(q, k, v, dt, dev)
    cu_d = cu.to(device=dev, dtype=torch.int32)
    nseg = cu.numel() - 1
    ws = workspace(dev, lib.rap_attention_workspace_bytes(TP, nseg))
    out = torch.full((TP, H * 64), float("nan"), dtype=TORCH_DT[dt], device=dev)
    bound_d = None if bound is None else bound.to(device=dev, dtype=torch.float32)
    rc = lib.rap_attention_h16(dt, _lib.ptr(qk), _lib.ptr(vt), nblk, _lib.ptr(cu_d), nseg, _lib.ptr(out), TP, H, _lib.ptr(bound_d),
                               _lib.ptr(ws), ws.numel(), stream(dev))
    _lib.check(rc, "rap_attention_h16")
    torch.cuda.synchronize()
    return out.cpu()


def attention_ref64(q, k, v, cu, dt):
    """fp64 softmax attention per segment on the ROUNDED operands; returns (TP, H*64) and the per-row bound scale."""
    qh, kh, vh = (to_h(x, dt).double() for x in (q, k, v))
    H, TP, _ = q.shape
    out = torch.zeros(TP, H * 64, dtype=torch.float64)
    for a, b in zip(cu[:-1].tolist(), cu[1:].tolist()):
        if b == a:
            continue
        s = qh[:, a:b] @ kh[:, a:b].transpose(1, 2) / 8.0
        p = torch.softmax(s, dim=-1)
        out[a:b] = (p @ vh[:, a:b]).permute(1, 0, 2).reshape(b - a, H * 64)
    return out


def logit_bound(q, k):
    """per-head bound on q.k/8 by Cauchy-Schwarz (what 8 max|gamma_q| max|gamma_k| is after qk-norm)"""
    return q.norm(dim=-1).amax(dim=1) * k.norm(dim=-1).amax(dim=1) / 8.0 * 1.01


@pytest.mark.parametrize("bounded", [False, True], ids=["online-max", "bounded"])
@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("H", [1, 8, 4, 12, 16])      # (4 / 12 / 16: the head counts of d = 256 / 768 / 1024)
def test_attention_h16_ragged_segments(lib, dev, dt, H, bounded):
    g = torch.Generator().manual_seed(11 + H)
    lens = [1, 63, 64, 65, 300, 0, 257, 1000, 31, 512]          # unaligned starts, empty segment, multi-block segments
    cu = torch.tensor([0] + lens).cumsum(0)
    TP = int(cu[-1])
    q = F.normalize(torch.randn(H, TP, 64, generator=g), dim=-1) * 8 * (0.5 + torch.rand(H, 1, 64, generator=g))
    k = F.normalize(torch.randn(H, TP, 64, generator=g), dim=-1) * 8 * (0.5 + torch.rand(H, 1, 64, generator=g))
    v = torch.randn(H, TP, 64, generator=g)
    out = run_attention_h(lib, dev, dt, q, k, v, cu, bound=logit_bound(q, k) if bounded else None)
    ref = attention_ref64(q, k, v, cu, dt)
    assert not torch.isnan(out.float()).any()
    err = (out.double() - ref).abs().max().item()
    # P is rounded to the operand type before P*V (1 ulp relative per probability, signs of v random) and the output is
    # rounded once more: a few ulps of max|v| ~ 4
    assert err < ATTN_ULPS * ULP[dt], err
    print(f"attention dt={dt} H={H}: max abs err vs fp64 {err:.2e}")


@pytest.mark.parametrize("dt", [1, 2])
def test_attention_h16_single_token_segments_return_v(lib, dev, dt):
    g = torch.Generator().manual_seed(3)
    TP, H = 130, 2
    q, k, v = (torch.randn(H, TP, 64, generator=g) for _ in range(3))
    out = run_attention_h(lib, dev, dt, q, k, v, torch.arange(TP + 1))
    want = to_h(v, dt).permute(1, 0, 2).reshape(TP, H * 64)
    assert torch.equal(out, want)        # softmax over one key is exactly 1
    outb = run_attention_h(lib, dev, dt, q, k, v, torch.arange(TP + 1), bound=logit_bound(q, k))
    assert (outb.float() - want.float()).abs().max().item() <= 2 * ULP[dt] * want.float().abs().max().item()


@pytest.mark.parametrize("dt", [1, 2])
def test_attention_h16_sharp_softmax_and_late_maximum(lib, dev, dt):
    """One key dominates, placed in the LAST tile (forces the running-max rescale on the final step) and the first tile."""
    g = torch.Generator().manual_seed(9)
    H, L = 2, 700
    for spike_at in (L - 1, 0, 350):
        q = torch.randn(H, L, 64, generator=g); k = torch.randn(H, L, 64, generator=g) * 0.1; v = torch.randn(H, L, 64, generator=g)
        k[:, spike_at] = q[:, 5] * 4.0      # q5 . k_spike / 8 is huge for query 5, large for the others' projections
        ref = attention_ref64(q, k, v, torch.tensor([0, L]), dt)
        for bound in (None, logit_bound(q, k).clamp(max=40.0)):
            out = run_attention_h(lib, dev, dt, q, k, v, torch.tensor([0, L]), bound=bound)
            err = (out.double() - ref).abs().max().item()
            assert err < 8 * ULP[dt], (spike_at, bound is not None, err)


@pytest.mark.parametrize("dt", [1, 2])
def test_attention_h16_full_size_agrees_with_fp32_kernel(lib, dev, dt):
    """BASELINE geometry (segments of 4096 and 8192 tokens, 8 heads): the 16-bit kernel vs the exact-fp32 kernel on the
    same rounded q,k,v; rows of the implied softmax sum to one (v = ones -> out = 1)."""
    H, L, nseg = 8, 4096, 4
    TP = L * nseg
    g = torch.Generator().manual_seed(21)
    q = F.normalize(torch.randn(H, TP, 64, generator=g), dim=-1) * 8
    k = F.normalize(torch.randn(H, TP, 64, generator=g), dim=-1) * 8
    v = torch.randn(H, TP, 64, generator=g)
    for seg in (L, 2 * L):
        cu = torch.arange(0, TP + 1, seg)
        out = run_attention_h(lib, dev, dt, q, k, v, cu, bound=torch.full((H,), 8.01))
        qkv32 = torch.stack([to_h(q, dt).float(), to_h(k, dt).float(), to_h(v, dt).float()]).contiguous().to(dev)
        o32 = torch.empty(TP, H * 64, device=dev)
        ws = workspace(dev, lib.rap_attention_workspace_bytes(TP, cu.numel() - 1))
        _lib.check(lib.rap_attention_f32(_lib.ptr(qkv32), _lib.ptr(cu.to(device=dev, dtype=torch.int32)), cu.numel() - 1, _lib.ptr(o32),
                                         TP, H, _lib.ptr(None), _lib.ptr(ws), ws.numel(), stream(dev)), "attention_f32")
        torch.cuda.synchronize()
        err = (out.float() - o32.cpu()).abs().max().item()
        assert err < 4 * ULP[dt], (seg, err)
        ones = run_attention_h(lib, dev, dt, q, k, torch.ones_like(v), cu, bound=torch.full((H,), 8.01))
        assert (ones.float() - 1.0).abs().max().item() <= 2 * ULP[dt]


# ---------------------------------------------------------------------------------------------
# normalisation kernels
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [1, 2])
def test_layernorm_h16(lib, dev, dt):
    _check_layernorm_h16(lib, dev, dt, 512)


@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("d", [256, 768, 1024])
def test_layernorm_h16_at_other_widths(lib, dev, dt, d):
    """d / 256 = 1, 3, 4 float4 per lane (layernorm_h16_kernel<NV>)"""
    _check_layernorm_h16(lib, dev, dt, d)


def _check_layernorm_h16(lib, dev, dt, d):
    g = torch.Generator().manual_seed(2)
    TP, rows = 777, 3
    x = torch.randn(TP, d, generator=g) * 3 + 0.5
    mod = torch.randn(rows, 4, 2 * d, generator=g) * 0.3
    token_row = torch.randint(0, rows, (TP,), generator=g, dtype=torch.int32)
    out = torch.empty(TP, d, dtype=TORCH_DT[dt], device=dev)
    md, xd, trd = mod.to(dev), x.to(dev), token_row.to(dev)
    j = 2
    rc = lib.rap_layernorm_mod_h16(dt, _lib.ptr(xd), _lib.ptr(out), TP, d, _lib.ptr(md[0, j]), 4 * 2 * d, _lib.ptr(trd), stream(dev))
    _lib.check(rc, "ln_mod_h16"); torch.cuda.synchronize()
    xn = F.layer_norm(x.double(), (d,), eps=1e-5)
    ref = xn * (1 + mod[token_row.long(), j, :d].double()) + mod[token_row.long(), j, d:].double()
    err = (out.cpu().double() - ref).abs() / (ref.abs() + 1e-2)
    assert err.max().item() < ONE_ROUNDING * ULP[dt] + NORM_SLACK, err.max().item()
    gain, shift = torch.randn(d, generator=g), torch.randn(d, generator=g)
    gd, sd = gain.to(dev), shift.to(dev)
    rc = lib.rap_layernorm_affine_h16(dt, _lib.ptr(xd), _lib.ptr(out), TP, d, _lib.ptr(gd), _lib.ptr(sd), stream(dev))
    _lib.check(rc, "ln_affine_h16"); torch.cuda.synchronize()
    ref = xn * gain.double() + shift.double()
    err = (out.cpu().double() - ref).abs() / (ref.abs() + 1e-2)
    assert err.max().item() < ONE_ROUNDING * ULP[dt] + NORM_SLACK, err.max().item()


@pytest.mark.parametrize("dt", [1, 2])
def test_qknorm_h16(lib, dev, dt):
    _check_qknorm_h16(lib, dev, dt, 8)


@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("H", [4, 12, 16])
def test_qknorm_h16_at_other_head_counts(lib, dev, dt, H):
    _check_qknorm_h16(lib, dev, dt, H)


def _check_qknorm_h16(lib, dev, dt, H):
    g = torch.Generator().manual_seed(6)
    TP = 301
    qk = to_h(torch.randn(2, H, TP, 64, generator=g) * 2, dt)
    gq, gk = torch.rand(H, 64, generator=g) + 0.5, torch.rand(H, 64, generator=g) + 0.5
    buf = qk.to(dev).clone()
    gqd, gkd = gq.to(dev), gk.to(dev)
    _lib.check(lib.rap_qknorm_h16(dt, _lib.ptr(buf), TP, H, _lib.ptr(gqd), _lib.ptr(gkd), stream(dev)), "qknorm_h16")
    torch.cuda.synchronize()
    x = qk.double()
    ref = x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12) * torch.stack([gq, gk])[:, :, None, :].double() * 8.0
    err = (buf.cpu().double() - ref).abs() / (ref.abs() + 1e-2)
    assert err.max().item() < ONE_ROUNDING * ULP[dt] + NORM_SLACK, err.max().item()


# ---------------------------------------------------------------------------------------------
# model level: measured deviation of the 16-bit paths from the fp32 reference goldens
# ---------------------------------------------------------------------------------------------
_MODELS = {}


def get_model(num_layers, seed, dev, compute_dtype, residual_dtype="float32"):
    key = (num_layers, seed, compute_dtype, residual_dtype)
    if key not in _MODELS:
        cfg = dict(S.RAP_12); cfg["num_layers"] = num_layers
        sd = S.make_weights(cfg, seed)
        m = rap_amd.PointCloudDiT(in_dim=0, out_dim=3, embed_dim=512, num_layers=num_layers, num_heads=8, local_feat_dim=32,
                                  compute_dtype=compute_dtype, residual_dtype=residual_dtype)
        m.load_state_dict(sd)
        _MODELS[key] = (cfg, sd, m.to(dev))
    return _MODELS[key]


# bounds = measured worst case on MI355X x ~3.5 (r01 run 4: bf16 0.9-2.2e-3, fp16 1.2-2.7e-4 of max|v|; the measured
# numbers are printed; DESIGN.md section 2 quotes them)
FWD_REL_BOUND = {"bfloat16": 8e-3, "float16": 1e-3}


@pytest.mark.parametrize("rdt", ["float32", "float16"], ids=["fp32-stream", "fp16-stream"])
@pytest.mark.parametrize("cdt", ["bfloat16", "float16"])
@pytest.mark.parametrize("name", ["l2_ragged_rigid", "l2_emptypart_rigid", "l12_small_rigid", "l12_pair512_free"])
def test_forward_h16_deviation_from_fp32_golden(name, cdt, rdt, dev):
    g, inp = load_golden(name)
    cfg, sd, model = get_model(int(g["num_layers"]), int(g["weight_seed"]), dev, cdt, rdt)
    cu_b, cu_p = O.prepare_cu_seqlens(inp)
    d = {k: v.to(dev) for k, v in inp.items()}
    out = model(x=d["x_1"], timesteps=torch.from_numpy(g["fwd_timesteps"]).to(dev), cond_coord=d["pointclouds"],
                local_features=d["features"], latent_features=None, scales=d["scales"], anchor_indices=d["anchor_indices"],
                cu_seqlens_batch=cu_b.to(dev), cu_seqlens_part=cu_p.to(dev), return_transformer_features=True)
    v_ref = torch.from_numpy(g["fwd_velocity"])
    v = out["velocity"].cpu()
    assert torch.isfinite(v).all()
    rel = (v - v_ref).abs().max().item() / v_ref.abs().max().item()
    rms = ((v - v_ref).pow(2).mean().sqrt() / v_ref.pow(2).mean().sqrt()).item()
    f_ref = torch.from_numpy(g["fwd_features"])
    frel = (out["transformer_features"].cpu() - f_ref).abs().max().item() / f_ref.abs().max().item()
    print(f"{name} {cdt} ({rdt} residual stream): velocity max-abs/max {rel:.3e}  rel-rms {rms:.3e}  features max-abs/max {frel:.3e}")
    # the fp16 residual stream under fp16 operands (NOT the default pairing, see rap_amd/flow_model.py) roughly doubles that mode's deviation
    bound = FWD_REL_BOUND[cdt] * (2.0 if (cdt, rdt) == ("float16", "float16") else 1.0)
    assert rel < bound, rel
    assert frel < 4 * bound, frel


@pytest.mark.parametrize("cdt", ["bfloat16", "float16"])
def test_sample_h16_deviation_and_invariants(cdt, dev):
    """Whole sampling call in 16-bit arithmetic on a golden case with rigidity forcing: the deviation of the registered
    cloud / poses from the fp32 reference is REPORTED and loosely bounded; the invariants that do not depend on
    precision are asserted exactly: with rigidity forcing the last x_t is a rigid image of cond, rotations are proper."""
    g, inp = load_golden("l12_small_rigid")
    cfg, sd, model = get_model(int(g["num_layers"]), int(g["weight_seed"]), dev, cdt)
    flow = rap_amd.RectifiedPointFlow(flow_model=model, inference_sampling_steps=int(g["num_steps"]), rigidity_forcing=True)
    d = {k: v.to(dev) for k, v in inp.items()}
    res = flow.sample_rectified_flow(d, None, x_1=d["x_1"])
    R, t = flow.last_poses
    x0 = res["end_point_trajectory"].cpu(); x0_ref = torch.from_numpy(g["end_point_trajectory"])
    assert torch.isfinite(x0).all()
    e0 = (x0[-1] - x0_ref[-1]).abs().max().item()
    eR = torch.linalg.matrix_norm(R.cpu() - torch.from_numpy(g["R"])).max().item()
    print(f"l12_small_rigid {cdt}: final x0 max abs dev {e0:.3e}, |dR|_F {eR:.3e}")
    valid = torch.from_numpy(g["in_points_per_part"]) > 0
    Rv = R.cpu()[valid]
    assert (torch.linalg.det(Rv) - 1).abs().max().item() < 1e-4
    assert (Rv @ Rv.transpose(1, 2) - torch.eye(3)).abs().max().item() < 1e-4
    # measured (r01 run 4): bf16 1.1e-3 / 8.0e-4, fp16 1.0e-4 / 6.2e-5; normalised units, the cloud spans ~[-0.67, 0.67]
    assert e0 < {"bfloat16": 5e-3, "float16": 5e-4}[cdt] and eR < {"bfloat16": 5e-3, "float16": 5e-4}[cdt], (e0, eR)


def test_autocast_selects_the_16bit_path(dev):
    """compute_dtype=None follows torch autocast like the reference's nn.Linear layers (Lightning '16-mixed')."""
    g, inp = load_golden("l2_ragged_rigid")
    cfg, sd, m32 = get_model(2, int(g["weight_seed"]), dev, "float32")
    _, _, mauto = get_model(2, int(g["weight_seed"]), dev, None)
    cu_b, cu_p = O.prepare_cu_seqlens(inp)
    d = {k: v.to(dev) for k, v in inp.items()}
    args = dict(x=d["x_1"], timesteps=torch.from_numpy(g["fwd_timesteps"]).to(dev), cond_coord=d["pointclouds"],
                local_features=d["features"], latent_features=None, scales=d["scales"], anchor_indices=d["anchor_indices"],
                cu_seqlens_batch=cu_b.to(dev), cu_seqlens_part=cu_p.to(dev))
    v32 = m32(**args)
    v_plain = mauto(**args)
    assert torch.equal(v32, v_plain)                       # no autocast -> the exact fp32 path
    with torch.autocast("cuda", dtype=torch.bfloat16):
        v_bf = mauto(**args)
    _, _, mbf = get_model(2, int(g["weight_seed"]), dev, "bfloat16")
    assert torch.equal(v_bf, mbf(**args))
    assert not torch.equal(v_bf, v32)


@pytest.mark.parametrize("cdt", ["bfloat16", "float16"])
@pytest.mark.parametrize("label,batch,views,points,steps", [("configs[1]/[2] geometry", 2, 2, 4096, 20), ("configs[3] geometry", 1, 8, 2048, 30),
                                                             ("configs[4] geometry", 1, 2, 32768, 50)])
def test_baseline_geometries_h16_agrees_with_fp32_path(label, batch, views, points, steps, cdt, dev):
    """Full BASELINE point counts (rap_12 depth is not needed for the property: 2 layers), first 2 flow steps of the
    config's time grid are enough to exercise every kernel at that geometry: the 16-bit path must stay within the
    measured 16-bit deviation of the exact-fp32 path ON THE GPU (itself pinned to the oracle elsewhere), produce proper
    rotations, and -- rigidity forcing on -- a last x_t that is a rigid image of cond."""
    cfg, sd, m32 = get_model(2, 3, dev, "float32")
    _, _, mh = get_model(2, 3, dev, cdt)
    inp = S.make_uniform_inputs(batch, views, points, seed=4321)
    d = {k: v.to(dev) for k, v in inp.items()}
    outs = {}
    for tag, model in (("f32", m32), (cdt, mh)):
        flow = rap_amd.RectifiedPointFlow(flow_model=model, inference_sampling_steps=2, rigidity_forcing=True)
        outs[tag] = flow.sample_and_register(d, x_1=d["x_1"])
    a, b = outs[cdt], outs["f32"]
    assert torch.isfinite(a["end_point_trajectory"]).all()
    e0 = (a["end_point_trajectory"] - b["end_point_trajectory"]).abs().max().item()
    eR = torch.linalg.matrix_norm(a["R"] - b["R"]).max().item()
    print(f"{label} {cdt}: x0 dev {e0:.3e}  |dR|_F {eR:.3e}")
    bound = {"bfloat16": 2e-2, "float16": 3e-3}[cdt]
    assert e0 < bound and eR < bound, (e0, eR)
    R = a["R"].reshape(-1, 3, 3)
    assert (R @ R.transpose(1, 2) - torch.eye(3, device=dev)).abs().max().item() < 1e-4
    assert (torch.linalg.det(R) - 1).abs().max().item() < 1e-4
    rig = rap_amd.rigidify_prediction_with_procrustes(a["end_point_trajectory"][-1], d["pointclouds"], inp["points_per_part"],
                                                      inp["cu_seqlens"])
    assert (a["trajectory"][-1] - rig).abs().max().item() < 1e-5


@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("bounded", [False, True], ids=["online", "bounded"])
def test_attention_h16_lds_dma_stream_is_bit_identical_to_register_staging(lib, dev, dt, bounded):
    """Round 3: the K / V^T tiles reach the LDS by global_load_lds (128-byte rows, slot ^ ((row >> 1) & 7) swizzle) instead of through
    staging registers (rap_set_tuning(13, 0) restores those).  Data movement only: outputs BIT-identical on ragged segments."""
    g = torch.Generator().manual_seed(78)
    H = 4
    cu = torch.tensor([0] + [1, 63, 64, 65, 128, 129, 192, 300, 0, 257, 384, 31, 449, 700]).cumsum(0)
    TP = int(cu[-1])
    q = F.normalize(torch.randn(H, TP, 64, generator=g), dim=-1) * 8
    k = F.normalize(torch.randn(H, TP, 64, generator=g), dim=-1) * 8
    v = torch.randn(H, TP, 64, generator=g)
    outs = []
    try:
        for dma in (1, 0):
            assert lib.rap_set_tuning(13, dma) == 0
            outs.append(run_attention_h(lib, dev, dt, q, k, v, cu, bound=logit_bound(q, k) if bounded else None))
    finally:
        assert lib.rap_set_tuning(13, 1) == 0
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))


@pytest.mark.parametrize("dt", [1, 2])
def test_attention_h16_bounded_and_online_softmax_agree(lib, dev, dt):
    """The two shipped softmax evaluations of the 16-bit attention (bounded / offset-free when logit bounds are supplied, online with
    running maxima otherwise; fp16 always takes the online one): same function, results within rounding of each other, on segment
    lengths around every key-tile count 1..7, unaligned starts and one-query segments."""
    g = torch.Generator().manual_seed(31)
    H = 4
    for cu in (torch.tensor([0, 100, 164, 700, 1213, 1214, 2000]),
               torch.tensor([0] + [1, 63, 64, 65, 128, 129, 192, 300, 0, 257, 384, 31, 449]).cumsum(0)):
        TP = int(cu[-1])
        q = F.normalize(torch.randn(H, TP, 64, generator=g), dim=-1) * 8
        k = F.normalize(torch.randn(H, TP, 64, generator=g), dim=-1) * 8
        v = torch.randn(H, TP, 64, generator=g)
        base = run_attention_h(lib, dev, dt, q, k, v, cu, bound=logit_bound(q, k))
        alt = run_attention_h(lib, dev, dt, q, k, v, cu, bound=None)
        ref = attention_ref64(q, k, v, cu, dt)
        assert (alt.double() - ref).abs().max().item() < 8 * ULP[dt]
        assert (base.double() - ref).abs().max().item() < 8 * ULP[dt]
        assert (alt.float() - base.float()).abs().max().item() < 4 * ULP[dt]


def test_fused_qknorm_model_path_agrees_with_the_unfused_one(dev):
    """rap_set_tuning(7, .): the whole velocity network with qk-norm inside the QKV epilogue vs as its own kernel (the r01 path) --
    same function, one 16-bit rounding fewer on q and k."""
    lib = _lib.load()
    g, inp = load_golden("l12_small_rigid")
    outs = {}
    try:
        for fused in (1, 0):
            assert lib.rap_set_tuning(7, fused) == 0
            cfg, sd, model = get_model(12, int(g["weight_seed"]), dev, "bfloat16")
            cu_b, cu_p = O.prepare_cu_seqlens(inp)
            d = {k: v.to(dev) for k, v in inp.items()}
            outs[fused] = model(x=d["x_1"], timesteps=torch.from_numpy(g["fwd_timesteps"]).to(dev), cond_coord=d["pointclouds"],
                                local_features=d["features"], latent_features=None, scales=d["scales"], anchor_indices=d["anchor_indices"],
                                cu_seqlens_batch=cu_b.to(dev), cu_seqlens_part=cu_p.to(dev)).cpu()
    finally:
        assert lib.rap_set_tuning(7, 1) == 0
    v_ref = torch.from_numpy(g["fwd_velocity"])
    vmax = v_ref.abs().max().item()
    e_fused, e_unfused = (outs[1] - v_ref).abs().max().item() / vmax, (outs[0] - v_ref).abs().max().item() / vmax
    print(f"bf16 forward vs fp32 golden: fused {e_fused:.2e}, unfused {e_unfused:.2e}")
    assert e_fused < FWD_REL_BOUND["bfloat16"] and e_unfused < FWD_REL_BOUND["bfloat16"]
    assert (outs[1] - outs[0]).abs().max().item() / vmax < FWD_REL_BOUND["bfloat16"]


@pytest.mark.parametrize("name", ["l12_small_rigid", "l2_ragged_rigid"])
def test_few_token_split_k_model_path_agrees_with_the_unsplit_one(name, dev):
    """Few-token calls in the 16-bit modes (round 3): ff2 splits K over up to 4 blocks per 128 x 128 tile (tuning key 6; fp32 partial
    planes in the call's workspace, one combine pass).  Same function, the k-sum re-associated: the velocity field of the whole network
    agrees with the unsplit path far inside the bf16 deviation bound, and both stay inside it against the fp32 golden."""
    lib = _lib.load()
    g, inp = load_golden(name)
    outs = {}
    try:
        for on in (1, 0):
            assert lib.rap_set_tuning(6, on) == 0
            cfg, sd, model = get_model(int(g["num_layers"]), int(g["weight_seed"]), dev, "bfloat16")
            cu_b, cu_p = O.prepare_cu_seqlens(inp)
            d = {k: v.to(dev) for k, v in inp.items()}
            TP = int(d["x_1"].shape[0])
            assert lib.rap_gemm_h16_splitk_workspace_bytes(TP, 512, 2048) > 0      # the fixture IS a few-token call (reserved whatever key 6 says)
            outs[on] = model(x=d["x_1"], timesteps=torch.from_numpy(g["fwd_timesteps"]).to(dev), cond_coord=d["pointclouds"],
                             local_features=d["features"], latent_features=None, scales=d["scales"], anchor_indices=d["anchor_indices"],
                             cu_seqlens_batch=cu_b.to(dev), cu_seqlens_part=cu_p.to(dev)).cpu()
    finally:
        assert lib.rap_set_tuning(6, 1) == 0
    v_ref = torch.from_numpy(g["fwd_velocity"])
    vmax = v_ref.abs().max().item()
    e_on, e_off = (outs[1] - v_ref).abs().max().item() / vmax, (outs[0] - v_ref).abs().max().item() / vmax
    between = (outs[1] - outs[0]).abs().max().item() / vmax
    print(f"bf16 forward vs fp32 golden: split-K ff2 {e_on:.2e}, unsplit {e_off:.2e}, between them {between:.2e}")
    assert not torch.isnan(outs[1]).any()
    assert e_on < FWD_REL_BOUND["bfloat16"] and e_off < FWD_REL_BOUND["bfloat16"]
    assert between < FWD_REL_BOUND["bfloat16"]
