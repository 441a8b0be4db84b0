"""Guard-band tests of the kernel-level entry points, through the C ABI: no call writes outside its outputs or its workspace, no result
depends on what lies beyond its inputs, and a refused call writes nothing.

Every case is ONE call with
  * every OUTPUT in a ``guards.Guarded`` (interior 0xFF = NaN / -1, pads and row gaps 0xA5), checked after the call;
  * every INPUT in a ``Guarded`` whose pads hold 0x00 in one run and 0xFF (NaN as a float, -1 as an index) in a second run: the outputs
    of the two runs must be bitwise identical, and the input pads must be unchanged too;
  * every workspace at exactly the bytes its ``rap_*_workspace_bytes`` query returned, in a ``Guarded``;
  * the value assertion the existing test of that entry point makes (same fp64 reference, same bound, imported from that test's module),
    so that a case cannot pass by writing nothing.

What this does NOT see: a stray write further away than the pad (one 256-row tile at the tested row pitch, 64 KiB at least), and a
read past an input that does not reach a result.  The read itself is deliberately not hunted (no buffer is placed at the end of a
mapping, nothing here can fault): only dependence on it is.  Every byte these tests may see overwritten is memory they own.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import guards as G
import test_h16_gpu as TH
import test_kernels_gpu as TK
import test_x2_gpu as TX
from oracle import rap_oracle as O
from rap_amd import _lib

pytestmark = pytest.mark.gpu

RAP_ERR_INVALID, RAP_ERR_WORKSPACE = -1, -2
PADS = (0x00, 0xFF)
MS = (1, 100, 129, 257)                 # one row; below, one past and two past a 128-row tile / one past a 256-row tile
SEGMENTS = {"one-token": [0, 1], "63-1-1-268": [0, 63, 64, 65, 333], "empty-and-257": [0, 40, 40, 297, 300]}
F32, F16, BF16, I32, I64, U8 = torch.float32, torch.float16, torch.bfloat16, torch.int32, torch.int64, torch.uint8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def stream(dev):
    return _lib.current_stream(dev)


def isz(dtype):
    return torch.empty((), dtype=dtype).element_size()


class Case:
    """the guarded buffers of one call: inputs between `pad` bytes, outputs and workspaces between 0xA5"""

    def __init__(self, dev, pad):
        self.dev, self.pad, self.guards = dev, pad, []

    def inp(self, t, name="input"):
        if t is None:
            return None
        g, v = G.guarded_like(t, self.dev, guard=self.pad, name=name)
        self.guards.append(g)
        return v

    def out(self, nbytes, pitch=0, name="output"):
        g = G.Guarded(nbytes, self.dev, 0xFF, pitch=pitch, name=name)
        self.guards.append(g)
        return g

    def out_view(self, dtype, shape, name="output"):
        shape = tuple(int(s) for s in shape)
        n = 1
        for s in shape:
            n *= s
        return self.out(n * isz(dtype), pitch=shape[-1] * isz(dtype) if len(shape) > 1 else 0, name=name).view(dtype, shape)

    def out_rows(self, dtype, rows, cols, ld, name="output"):
        """(rows, cols) output with row pitch ld: the ld - cols elements after every row are guard bytes"""
        return self.out(rows * ld * isz(dtype), pitch=ld * isz(dtype), name=name).strided(dtype, rows, cols, ld)

    def check(self):
        torch.cuda.synchronize()
        for g in self.guards:
            g.check()


def bits(t):
    return t.contiguous().cpu().view(torch.uint8).clone()


def run_both(dev, run):
    """run(case) -> the output tensors, having made its value assertions.  Once with 0x00 and once with 0xFF around every input."""
    results = []
    for pad in PADS:
        case = Case(dev, pad)
        outs = run(case)
        case.check()
        results.append([bits(t) for t in outs])
    for i, (a, b) in enumerate(zip(*results)):
        assert torch.equal(a, b), f"output {i} depends on the bytes beyond the inputs (0x00 against 0xFF)"


def interleave(lib, dev, W, b, inner, K):
    Wd, bd = W.to(dev), b.to(dev)
    Wp, bp = torch.empty_like(Wd), torch.empty_like(bd)
    _lib.check(lib.rap_geglu_interleave(_lib.ptr(Wd), _lib.ptr(bd), _lib.ptr(Wp), _lib.ptr(bp), inner, K, stream(dev)), "interleave")
    torch.cuda.synchronize()
    return Wp.cpu(), bp.cpu()


# ---------------------------------------------------------------------------------------------
# rap_gemm_f32
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [0, 64], ids=["ldc=N", "ldc=N+64"])
@pytest.mark.parametrize("N,K", [(128, 32), (512, 128)])
@pytest.mark.parametrize("epi", ["bias", "resid", "geglu"])
def test_gemm_f32_writes_only_the_rows_and_columns_of_c(lib, dev, epi, N, K, extra):
    for M in MS:
        g = torch.Generator().manual_seed(M * 7 + N + K)
        A = torch.randn(M, K, generator=g); W = torch.randn(N, K, generator=g) / K ** 0.5; b = torch.randn(N, generator=g)
        h = torch.randn(M, N, generator=g)
        u = A.double() @ W.double().T + b.double()
        cols, code, Wk, bk = N, {"bias": 0, "resid": 1, "geglu": 3}[epi], W, b
        if epi == "resid":
            ref = h.double() + u
        elif epi == "geglu":
            cols = N // 2
            ref = u[:, :cols] * F.gelu(u[:, cols:])
            Wk, bk = interleave(lib, dev, W, b, cols, K)
        else:
            ref = u
        ldc = cols + extra

        def run(c):
            C = c.out_rows(F32, M, cols, ldc, "C")
            TK.gemm(lib, dev, code, c.inp(A, "A"), c.inp(Wk, "W"), C, M, N, K, bias=c.inp(bk, "bias"),
                    resid=c.inp(h, "resid") if epi == "resid" else None, ldc=ldc)
            err = (C.cpu().double() - ref).abs().max().item()
            assert err < TK.GEMM_BOUND, (M, err)          # NaN (an element never written) fails this too
            return [C]
        run_both(dev, run)


@pytest.mark.parametrize("extra", [0, 64], ids=["ldc=N", "ldc=N+64"])         # (the scatter does not use ldc: neither value may matter)
@pytest.mark.parametrize("H,K", [(4, 32), (8, 128)])
def test_gemm_f32_qkv_scatter_writes_only_the_three_planes(lib, dev, H, K, extra):
    N = 3 * H * 64
    for M in MS:
        g = torch.Generator().manual_seed(5 + H + M)
        A = torch.randn(M, K, generator=g); W = torch.randn(N, K, generator=g) / K ** 0.5
        ref = (A.double() @ W.double().T).reshape(M, 3, H, 64).permute(1, 2, 0, 3)

        def run(c):
            C = c.out_view(F32, (3, H, M, 64), "qkv")
            TK.gemm(lib, dev, 4, c.inp(A, "A"), c.inp(W, "W"), C, M, N, K, heads=H, ldc=N + extra)
            assert (C.cpu().double() - ref).abs().max().item() < TK.GEMM_BOUND, M
            return [C]
        run_both(dev, run)


# ---------------------------------------------------------------------------------------------
# rap_gemm_h16, rap_gemm_h16_qkvnorm, rap_gemm_h16_splitk
# ---------------------------------------------------------------------------------------------
def rel_err(got, ref):
    return ((got.double() - ref).abs() / (ref.abs() + 1e-2)).max().item()


@pytest.mark.parametrize("extra", [0, 64], ids=["ldc=N", "ldc=N+64"])
@pytest.mark.parametrize("K", [128, 256])
@pytest.mark.parametrize("epi", ["f32-out", "h16-out", "fp16-resid", "geglu"])
@pytest.mark.parametrize("dt", [1, 2], ids=["bf16", "f16"])
def test_gemm_h16_writes_only_the_rows_and_columns_of_c(lib, dev, dt, epi, K, extra):
    N = 256
    for M in MS:
        g = torch.Generator().manual_seed(M * 7 + N + K)
        A = TH.to_h(torch.randn(M, K, generator=g), dt); W32 = torch.randn(N, K, generator=g) / K ** 0.5
        b = torch.randn(N, generator=g); h = torch.randn(M, N, generator=g) * 3
        W = TH.to_h(W32, dt)
        u = A.double() @ W.double().T + b.double()
        cols, Wk, bk = N, W, b
        if epi == "geglu":
            cols = N // 2
            Wi, bk = interleave(lib, dev, W32, b, cols, K)
            Wk = TH.to_h(Wi, dt)
            ref = u[:, :cols] * F.gelu(u[:, cols:])
        elif epi == "fp16-resid":
            h = h.to(F16)
            ref = h.double() + u
        elif epi == "f32-out":
            ref = h.double() + u
        else:
            ref = u
        ldc = cols + extra
        code, cdt = {"f32-out": (1, F32), "h16-out": (0, TH.TORCH_DT[dt]), "fp16-resid": (7, F16), "geglu": (3, TH.TORCH_DT[dt])}[epi]

        def run(c):
            C = c.out_rows(cdt, M, cols, ldc, "C")
            TH.gemm_h(lib, dev, dt, code, c.inp(A, "A"), c.inp(Wk, "W"), C, M, N, K, bias=c.inp(bk, "bias"),
                      resid=c.inp(h, "resid") if epi in ("f32-out", "fp16-resid") else None, ldc=ldc)
            got = C.cpu()
            assert not torch.isnan(got.float()).any(), M
            if epi == "f32-out":
                assert (got.double() - ref).abs().max().item() < TH.F32_OUT_BOUND, M
            elif epi == "h16-out":
                assert ((got.double() - ref).abs() - TH.ULP[dt] * 1.01 * ref.abs()).max().item() < TH.F32_OUT_BOUND, M
            elif epi == "fp16-resid":
                assert rel_err(got, ref) < TH.ONE_ROUNDING * TH.ULP[2] + TH.NORM_SLACK, M
            else:
                assert rel_err(got, ref) < TH.GEGLU_ROUNDINGS * TH.ULP[dt], M
            return [C]
        run_both(dev, run)


def check_vt(vt_cpu, want, M, nblk, bound):
    """vt [H][nblk][64 d][64 pos]: rows < M hold v, EVERY row >= M of the image reads back 0 (include/rapflow.h)"""
    vtc = vt_cpu.double()
    t = torch.arange(M)
    got = vtc[:, t >> 6, :, TH.vt_pos(t & 63)]              # (M, H, 64)
    assert rel_err(got, want) < bound
    tp = torch.arange(M, nblk * 64)
    if tp.numel():
        tail = vtc[:, tp >> 6, :, TH.vt_pos(tp & 63)]
        assert torch.equal(tail, torch.zeros_like(tail)), f"rows >= M = {M} of the transposed-V image are not all zero"


@pytest.mark.parametrize("K", [128, 256])
@pytest.mark.parametrize("fused_norm", [False, True], ids=["qkv", "qkvnorm"])
@pytest.mark.parametrize("dt", [1, 2], ids=["bf16", "f16"])
def test_gemm_h16_qkv_writes_only_the_planes_and_the_transposed_v_image(lib, dev, dt, fused_norm, K):
    H = 4
    N = 3 * H * 64
    for M in MS:
        g = torch.Generator().manual_seed(15 + M)
        A = TH.to_h(torch.randn(M, K, generator=g), dt); W = TH.to_h(torch.randn(N, K, generator=g) / K ** 0.5, dt)
        gq, gk = torch.rand(H, 64, generator=g) + 0.5, torch.rand(H, 64, generator=g) + 0.5
        x = (A.double() @ W.double().T).reshape(M, 3, H, 64).permute(1, 2, 0, 3)         # [3][H][M][64]
        ref_qk = x[:2]
        if fused_norm:
            ref_qk = x[:2] / x[:2].norm(dim=-1, keepdim=True).clamp_min(1e-12) * torch.stack([gq, gk])[:, :, None, :].double() * 8.0
        nblk = (M + 255) // 256 * 256 // 64                 # vt_nblk * 64 == M rounded up to 256: the documented extent, exactly

        def run(c):
            qk = c.out_view(TH.TORCH_DT[dt], (2, H, M, 64), "qk")
            vt = c.out_view(TH.TORCH_DT[dt], (H, nblk, 64, 64), "vt")
            Ad, Wd = c.inp(A, "A"), c.inp(W, "W")
            if fused_norm:
                gqd, gkd = c.inp(gq, "gamma_q"), c.inp(gk, "gamma_k")
                _lib.check(lib.rap_gemm_h16_qkvnorm(dt, _lib.ptr(Ad), K, _lib.ptr(Wd), K, _lib.ptr(qk), M, K, H, _lib.ptr(gqd), _lib.ptr(gkd),
                                                    8.0, _lib.ptr(vt), nblk, stream(dev)), "rap_gemm_h16_qkvnorm")
            else:
                TH.gemm_h(lib, dev, dt, 4, Ad, Wd, qk, M, N, K, heads=H, vt=vt, vt_nblk=nblk)
            torch.cuda.synchronize()
            assert rel_err(qk.cpu(), ref_qk) < TH.ONE_ROUNDING * TH.ULP[dt] + (TH.NORM_SLACK if fused_norm else 0.0), M
            check_vt(vt.cpu(), x[2].permute(1, 0, 2), M, nblk, TH.ONE_ROUNDING * TH.ULP[dt])
            return [qk, vt]
        run_both(dev, run)


@pytest.mark.parametrize("M", [5, 100])
@pytest.mark.parametrize("epi", [1, 7], ids=["fp32-stream", "fp16-stream"])
@pytest.mark.parametrize("dt", [1, 2], ids=["bf16", "f16"])
def test_gemm_h16_splitk_stays_inside_its_exact_workspace(lib, dev, dt, epi, M):
    N, K = 256, 1024
    need = lib.rap_gemm_h16_splitk_workspace_bytes(M, N, K)
    assert need == 4 * M * N * 4                           # four partial planes (tests/test_h16_gpu.py WIDTH_FF2)
    g = torch.Generator().manual_seed(43 + M)
    A = TH.to_h(torch.randn(M, K, generator=g), dt); W = TH.to_h(torch.randn(N, K, generator=g) / K ** 0.5, dt)
    bias = torch.randn(N, generator=g)
    h0 = torch.randn(M, N, generator=g) * 3
    h0 = h0.to(F16) if epi == 7 else h0
    ref = h0.double() + A.double() @ W.double().T + bias.double()

    def call(c, ws_bytes):
        C = c.out_view(h0.dtype, (M, N), "C")
        ws = c.out(need, pitch=N * 4, name="split-K workspace")
        Ad, Wd, bd, hd = c.inp(A, "A"), c.inp(W, "W"), c.inp(bias, "bias"), c.inp(h0, "resid")
        rc = lib.rap_gemm_h16_splitk(dt, epi, _lib.ptr(Ad), K, _lib.ptr(Wd), K, _lib.ptr(C), N, M, N, K, _lib.ptr(bd), _lib.ptr(hd), N,
                                     ctypes.c_void_p(ws.ptr), ws_bytes, stream(dev))
        torch.cuda.synchronize()
        return rc, C, ws

    def run(c):
        rc, C, _ = call(c, need)
        assert rc == 0
        if epi == 7:
            assert rel_err(C.cpu(), ref) < TH.ONE_ROUNDING * TH.ULP[2] + TH.NORM_SLACK
        else:
            assert (C.cpu().double() - ref).abs().max().item() < TH.F32_OUT_BOUND
        return [C]
    run_both(dev, run)
    # one byte short: refused, nothing written
    c = Case(dev, 0x00)
    rc, C, ws = call(c, need - 1)
    assert rc == RAP_ERR_WORKSPACE
    c.check()
    assert all(g.untouched() for g in c.guards if g.fill == 0xFF and g.guard == G.GUARD)


# ---------------------------------------------------------------------------------------------
# rap_x2_gemm
# ---------------------------------------------------------------------------------------------
def pack_cpu(lib, dev, x, scale=1.0):
    return TX.pack_dev(lib, dev, x, scale).cpu()


@pytest.mark.parametrize("extra", [0, 64], ids=["ldc=N", "ldc=N+64"])
@pytest.mark.parametrize("K", [128, 256])
@pytest.mark.parametrize("epi", ["resid", "geglu"])
def test_x2_gemm_writes_only_the_rows_and_columns_of_c(lib, dev, epi, K, extra):
    N = 256
    for M in MS:
        g = torch.Generator().manual_seed(2 + M + K)
        A = torch.randn(M, K, generator=g); W = torch.randn(N, K, generator=g) * 0.03
        bias = torch.randn(N, generator=g) * 0.1; resid = torch.randn(M, N, generator=g)
        sc = TX.weight_scale(W)
        u = A.double() @ W.double().T + bias.double()
        Wk, bk = W, bias
        if epi == "geglu":
            ref = u[:, :N // 2] * F.gelu(u[:, N // 2:])
            Wk, bk = interleave(lib, dev, W, bias, N // 2, K)
        else:
            ref = u + resid.double()
        Ap, Wp = pack_cpu(lib, dev, A), pack_cpu(lib, dev, Wk, sc)
        ldc = N + extra                                     # (GEGLU: the N / 2 outputs as N paired fp16 columns)

        def run(c):
            C = c.out_rows(F32 if epi == "resid" else F16, M, N, ldc, "C")
            TX.x2_gemm(lib, dev, 1 if epi == "resid" else 3, c.inp(Ap, "A"), c.inp(Wp, "W"), C, M, N, 2 * K, ldc, bias=c.inp(bk, "bias"),
                       resid=c.inp(resid, "resid") if epi == "resid" else None, acc_scale=1.0 / sc)
            if epi == "resid":
                scale = float((A.double().abs() @ W.double().abs().T).max())
                assert float((C.cpu().double() - ref).abs().max()) / scale < TX.X2_GEMM_BOUND, M
            else:
                got = TX.unpack_ref(C.cpu(), N // 2)
                assert float((got - ref).abs().max()) / float(ref.abs().max()) < TX.X2_GEGLU_BOUND, M
            return [C]
        run_both(dev, run)


@pytest.mark.parametrize("K", [128, 256])
def test_x2_gemm_qkv_writes_only_the_planes_and_the_transposed_v_image(lib, dev, K):
    H = 4
    N = 3 * H * 64
    for M in MS:
        g = torch.Generator().manual_seed(15 + M)
        A = torch.randn(M, K, generator=g); W = torch.randn(N, K, generator=g) / K ** 0.5 * 0.3
        gq, gk = torch.rand(H, 64, generator=g) + 0.5, torch.rand(H, 64, generator=g) + 0.5
        sc = TX.weight_scale(W)
        Ap, Wp = pack_cpu(lib, dev, A), pack_cpu(lib, dev, W, sc)
        x = (A.double() @ W.double().T).reshape(M, 3, H, 64).permute(1, 2, 0, 3)
        ref_qk = x[:2] / x[:2].norm(dim=-1, keepdim=True).clamp_min(1e-12) * torch.stack([gq, gk])[:, :, None, :].double() * 8.0
        nblk = (M + 255) // 256 * 256 // 64

        def run(c):
            qk = c.out_view(F16, (2, H, 2, M, 64), "qk")
            vt = c.out_view(F16, (H, nblk, 2, 64, 64), "vt")
            TX.x2_gemm(lib, dev, 5, c.inp(Ap, "A"), c.inp(Wp, "W"), qk, M, N, 2 * K, 0, acc_scale=1.0 / sc, heads=H, gq=c.inp(gq, "gamma_q"),
                       gk=c.inp(gk, "gamma_k"), q_mul=8.0, vt=vt, vt_nblk=nblk)
            qkc = qk.cpu()
            got = torch.cat([qkc[:, :, ch, :, :32].double() + qkc[:, :, ch, :, 32:].double() for ch in range(2)], dim=-1)
            assert float((got - ref_qk).abs().max()) / float(ref_qk.abs().max()) < TX.X2_QKV_BOUND, M
            vtc = vt.cpu()
            vsum = vtc[..., :32].double() + vtc[..., 32:].double()          # [H][blk][2][64 d][32]
            t = torch.arange(M)
            pos = TX.vt_pos(t & 63)
            want = x[2].permute(1, 0, 2)
            assert float((vsum[:, t >> 6, pos >> 5, :, pos & 31] - want).abs().max()) / float(want.abs().max()) < TX.X2_QKV_BOUND, M
            tp = torch.arange(M, nblk * 64)
            pp = TX.vt_pos(tp & 63)
            for half in (0, 32):                                              # head and tail planes of every row >= M: zero
                tail = vtc[:, tp >> 6, pp >> 5, :, half + (pp & 31)]
                assert torch.equal(tail, torch.zeros_like(tail)), f"rows >= M = {M} of the paired transposed-V image are not all zero"
            return [qk, vt]
        run_both(dev, run)


# ---------------------------------------------------------------------------------------------
# attention: rap_attention_f32, rap_attention_h16, rap_x2_attention, and the split forms rap_attention_f32_split, rap_x2_attention_split
# ---------------------------------------------------------------------------------------------
def attention_operands(H, cu, seed):
    g = torch.Generator().manual_seed(seed)
    TP = cu[-1]
    q = F.normalize(torch.randn(H, TP, 64, generator=g), dim=-1) * 8 * (0.5 + torch.rand(H, 1, 64, generator=g))
    k = F.normalize(torch.randn(H, TP, 64, generator=g), dim=-1) * 8 * (0.5 + torch.rand(H, 1, 64, generator=g))
    v = torch.randn(H, TP, 64, generator=g)
    return q, k, v


def attention_ws(c, lib, TP, nseg):
    need = lib.rap_attention_workspace_bytes(TP, nseg)
    return c.out(need, name="attention workspace"), need


@pytest.mark.parametrize("bounded", [False, True], ids=["online-max", "bounded"])
@pytest.mark.parametrize("H", [1, 4])
@pytest.mark.parametrize("seg", list(SEGMENTS))
def test_attention_f32_stays_inside_out_and_its_exact_workspace(lib, dev, seg, H, bounded):
    cu = SEGMENTS[seg]
    TP, nseg = cu[-1], len(cu) - 1
    q, k, v = attention_operands(H, cu, 11 + H)
    qkv = torch.stack([q, k, v])                                                 # [3][H][TP][64]
    ref = O.varlen_attention(qkv.permute(2, 0, 1, 3).double(), torch.tensor(cu, dtype=I32)).reshape(TP, H * 64)
    bound = TH.logit_bound(q, k) if bounded else None
    assert bound is None or float(bound.max()) <= 40.0

    def call(c, short=0):
        out = c.out_view(F32, (TP, H * 64), "out")
        ws, need = attention_ws(c, lib, TP, nseg)
        qd, cud, bd = c.inp(qkv, "qkv"), c.inp(torch.tensor(cu, dtype=I32), "cu_seqlens"), c.inp(bound, "logit_bound")
        rc = lib.rap_attention_f32(_lib.ptr(qd), _lib.ptr(cud), nseg, _lib.ptr(out), TP, H, _lib.ptr(bd), ctypes.c_void_p(ws.ptr), need - short,
                                   stream(dev))
        torch.cuda.synchronize()
        return rc, out

    def run(c):
        rc, out = call(c)
        assert rc == 0
        err = (out.cpu().double() - ref).abs().max().item()
        assert err < TK.ATTN_BOUND, err
        return [out]
    run_both(dev, run)
    refused_call_wrote_nothing(dev, call)


def refused_call_wrote_nothing(dev, call):
    """the same call with ws_bytes = need - 1: RAP_ERR_WORKSPACE, and every output and workspace byte still 0xFF, every guard intact"""
    c = Case(dev, 0x00)
    rc = call(c, 1)[0]
    assert rc == RAP_ERR_WORKSPACE, rc
    c.check()
    for g in c.guards:
        if g.guard == G.GUARD:
            assert g.untouched(), f"{g.name}: a refused call wrote into it"


H16_ATTN_KEY20 = [1, 64, 66, 130]       # the default rule; forced 64-row items; 64 rows x 4 / 128 rows x 2 key groups (the longest work lists)


@pytest.mark.parametrize("key20", H16_ATTN_KEY20, ids=[f"key20={v}" for v in H16_ATTN_KEY20])
@pytest.mark.parametrize("bounded", [False, True], ids=["online-max", "bounded"])
@pytest.mark.parametrize("H", [1, 4])
@pytest.mark.parametrize("dt", [1, 2], ids=["bf16", "f16"])
def test_attention_h16_stays_inside_out_and_its_exact_workspace(lib, dev, dt, H, bounded, key20):
    try:
        assert lib.rap_set_tuning(20, key20) == 0
        for seg, cu in SEGMENTS.items():
            TP, nseg = cu[-1], len(cu) - 1
            q, k, v = attention_operands(H, cu, 11 + H)
            ref = TH.attention_ref64(q, k, v, torch.tensor(cu), dt)
            qk, vt, nblk = TH.pack_qkv(q, k, v, dt, torch.device("cpu"))         # vt: exactly nblk * 64 = TP rounded up to 256 rows
            bound = TH.logit_bound(q, k) if bounded else None

            def call(c, short=0):
                out = c.out_view(TH.TORCH_DT[dt], (TP, H * 64), "out")
                ws, need = attention_ws(c, lib, TP, nseg)
                qkd, vtd = c.inp(qk, "qk"), c.inp(vt, "vt")
                cud, bd = c.inp(torch.tensor(cu, dtype=I32), "cu_seqlens"), c.inp(bound, "logit_bound")
                rc = lib.rap_attention_h16(dt, _lib.ptr(qkd), _lib.ptr(vtd), nblk, _lib.ptr(cud), nseg, _lib.ptr(out), TP, H, _lib.ptr(bd),
                                           ctypes.c_void_p(ws.ptr), need - short, stream(dev))
                torch.cuda.synchronize()
                return rc, out

            def run(c):
                rc, out = call(c)
                assert rc == 0
                got = out.cpu()
                assert not torch.isnan(got.float()).any(), seg
                err = (got.double() - ref).abs().max().item()
                assert err < TH.ATTN_ULPS * TH.ULP[dt], (seg, err)
                return [out]
            run_both(dev, run)
            if key20 == 1:
                refused_call_wrote_nothing(dev, call)
    finally:
        assert lib.rap_set_tuning(20, 1) == 0


@pytest.mark.parametrize("H", [1, 4])
@pytest.mark.parametrize("seg", list(SEGMENTS))
def test_x2_attention_stays_inside_out_and_its_exact_workspace(lib, dev, seg, H):
    cu = SEGMENTS[seg]
    TP, nseg = cu[-1], len(cu) - 1
    q, k, v = attention_operands(H, cu, 11 + H)
    ref = TX.attention_ref64(q, k, v, torch.tensor(cu))
    qk, vt, nblk = TX.make_x2_attention_operands(q, k, v)

    def call(c, short=0):
        out = c.out_view(F16, (TP, 2 * H * 64), "out")
        ws, need = attention_ws(c, lib, TP, nseg)
        qkd, vtd, cud = c.inp(qk, "qk"), c.inp(vt, "vt"), c.inp(torch.tensor(cu, dtype=I32), "cu_seqlens")
        rc = lib.rap_x2_attention(_lib.ptr(qkd), _lib.ptr(vtd), nblk, _lib.ptr(cud), nseg, _lib.ptr(out), TP, H, ctypes.c_void_p(ws.ptr),
                                  need - short, stream(dev))
        torch.cuda.synchronize()
        return rc, out

    def run(c):
        rc, out = call(c)
        assert rc == 0
        got = TX.unpack_ref(out.cpu(), H * 64)
        assert not torch.isnan(got).any()
        assert float((got - ref).abs().max()) < TX.X2_ATTN_BOUND
        return [out]
    run_both(dev, run)
    refused_call_wrote_nothing(dev, call)


def split_attention_ws(c, lib, TP, nseg, H, splits):
    need = lib.rap_attention_split_workspace_bytes(TP, nseg, H, splits)
    assert need > lib.rap_attention_workspace_bytes(TP, nseg)
    return c.out(need, name="split attention workspace"), need


@pytest.mark.parametrize("splits", [2, 4])
@pytest.mark.parametrize("H", [1, 4])
@pytest.mark.parametrize("seg", list(SEGMENTS))
def test_attention_f32_split_stays_inside_out_and_its_exact_workspace(lib, dev, seg, H, splits):
    cu = SEGMENTS[seg]
    TP, nseg = cu[-1], len(cu) - 1
    q, k, v = attention_operands(H, cu, 11 + H)
    qkv = torch.stack([q, k, v])                                                 # [3][H][TP][64]
    ref = O.varlen_attention(qkv.permute(2, 0, 1, 3).double(), torch.tensor(cu, dtype=I32)).reshape(TP, H * 64)
    bound = TH.logit_bound(q, k)
    assert float(bound.max()) <= 40.0

    def call(c, short=0):
        out = c.out_view(F32, (TP, H * 64), "out")
        ws, need = split_attention_ws(c, lib, TP, nseg, H, splits)
        qd, cud, bd = c.inp(qkv, "qkv"), c.inp(torch.tensor(cu, dtype=I32), "cu_seqlens"), c.inp(bound, "logit_bound")
        rc = lib.rap_attention_f32_split(_lib.ptr(qd), _lib.ptr(cud), nseg, _lib.ptr(out), TP, H, _lib.ptr(bd), splits, ctypes.c_void_p(ws.ptr),
                                         need - short, stream(dev))
        torch.cuda.synchronize()
        return rc, out

    def run(c):
        rc, out = call(c)
        assert rc == 0
        err = (out.cpu().double() - ref).abs().max().item()
        assert err < TK.ATTN_BOUND, err
        return [out]
    run_both(dev, run)
    refused_call_wrote_nothing(dev, call)


@pytest.mark.parametrize("splits", [2, 4])
@pytest.mark.parametrize("H", [1, 4])
@pytest.mark.parametrize("seg", list(SEGMENTS))
def test_x2_attention_split_stays_inside_out_and_its_exact_workspace(lib, dev, seg, H, splits):
    cu = SEGMENTS[seg]
    TP, nseg = cu[-1], len(cu) - 1
    q, k, v = attention_operands(H, cu, 11 + H)
    ref = TX.attention_ref64(q, k, v, torch.tensor(cu))
    qk, vt, nblk = TX.make_x2_attention_operands(q, k, v)

    def call(c, short=0):
        out = c.out_view(F16, (TP, 2 * H * 64), "out")
        ws, need = split_attention_ws(c, lib, TP, nseg, H, splits)
        qkd, vtd, cud = c.inp(qk, "qk"), c.inp(vt, "vt"), c.inp(torch.tensor(cu, dtype=I32), "cu_seqlens")
        rc = lib.rap_x2_attention_split(_lib.ptr(qkd), _lib.ptr(vtd), nblk, _lib.ptr(cud), nseg, _lib.ptr(out), TP, 0, H, splits,
                                        ctypes.c_void_p(ws.ptr), need - short, stream(dev))
        torch.cuda.synchronize()
        return rc, out

    def run(c):
        rc, out = call(c)
        assert rc == 0
        got = TX.unpack_ref(out.cpu(), H * 64)
        assert not torch.isnan(got).any()
        assert float((got - ref).abs().max()) < TX.X2_ATTN_BOUND
        return [out]
    run_both(dev, run)
    refused_call_wrote_nothing(dev, call)


# ---------------------------------------------------------------------------------------------
# LayerNorm (modulated and affine) and qk-norm: fp32, bf16, fp16 and the split-precision plane layout
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("TP", [1, 333])
@pytest.mark.parametrize("mode", [0, 1, 2, 3], ids=["f32", "bf16", "f16", "f32x2"])
def test_layernorm_writes_only_its_tp_rows(lib, dev, mode, TP):
    d, rows, j = 256, 3, 2
    g = torch.Generator().manual_seed(6)
    x = torch.randn(TP, d, generator=g) * 3 + 0.5
    mod = torch.randn(rows, 4, 2 * d, generator=g) * 0.3
    tok = torch.randint(0, rows, (TP,), generator=g, dtype=I32)
    gain, shift = torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g)
    xn = F.layer_norm(x.double(), (d,), eps=1e-5)
    ref_mod = xn * (1 + mod[tok.long(), j, :d].double()) + mod[tok.long(), j, d:].double()
    ref_aff = xn * gain.double() + shift.double()
    odt, ocols = {0: (F32, d), 1: (BF16, d), 2: (F16, d), 3: (F16, 2 * d)}[mode]

    def value_ok(out, ref):
        got = out.cpu()
        if mode == 0:
            assert (got.double() - ref).abs().max().item() < TK.NORM_BOUND
        elif mode == 3:
            assert float((TX.unpack_ref(got, d) - ref).abs().max()) / float(ref.abs().max()) < TX.X2_NORM_BOUND
        else:
            assert rel_err(got, ref) < TH.ONE_ROUNDING * TH.ULP[mode] + TH.NORM_SLACK

    def run_mod(c):
        out = c.out_view(odt, (TP, ocols), "out")
        xd, md, td = c.inp(x, "x"), c.inp(mod, "mod"), c.inp(tok, "token_row")
        mp = ctypes.c_void_p(md.data_ptr() + j * 2 * d * 4)
        if mode == 0:
            rc = lib.rap_layernorm_mod(_lib.ptr(xd), _lib.ptr(out), TP, d, mp, 4 * 2 * d, _lib.ptr(td), stream(dev))
        else:
            rc = lib.rap_layernorm_mod_h16(mode, _lib.ptr(xd), _lib.ptr(out), TP, d, mp, 4 * 2 * d, _lib.ptr(td), stream(dev))
        _lib.check(rc, "layernorm_mod"); torch.cuda.synchronize()
        value_ok(out, ref_mod)
        return [out]

    def run_affine(c):
        out = c.out_view(odt, (TP, ocols), "out")
        xd, gd, sd = c.inp(x, "x"), c.inp(gain, "gain"), c.inp(shift, "shift")
        if mode == 0:
            rc = lib.rap_layernorm_affine(_lib.ptr(xd), _lib.ptr(out), TP, d, _lib.ptr(gd), _lib.ptr(sd), stream(dev))
        else:
            rc = lib.rap_layernorm_affine_h16(mode, _lib.ptr(xd), _lib.ptr(out), TP, d, _lib.ptr(gd), _lib.ptr(sd), stream(dev))
        _lib.check(rc, "layernorm_affine"); torch.cuda.synchronize()
        value_ok(out, ref_aff)
        return [out]
    run_both(dev, run_mod)
    run_both(dev, run_affine)


@pytest.mark.parametrize("TP", [1, 333])
@pytest.mark.parametrize("mode", [0, 1, 2], ids=["f32", "bf16", "f16"])
def test_qknorm_writes_only_the_q_and_k_planes(lib, dev, mode, TP):
    """in place on [3][H][TP][64] (fp32) / [2][H][TP][64] (16 bit); fp32: the V plane is part of the check, unchanged bit for bit"""
    H = 4
    g = torch.Generator().manual_seed(7)
    planes = 3 if mode == 0 else 2
    x = torch.randn(planes, H, TP, 64, generator=g) * 2
    x[0, 3, TP // 2] = 0.0                                  # an all-zero row exercises the eps clamp
    if mode:
        x = TH.to_h(x, mode)
    gq, gk = torch.rand(H, 64, generator=g) + 0.5, torch.rand(H, 64, generator=g) + 0.5
    xd64 = x.double()
    ref = xd64[:2] / xd64[:2].norm(dim=-1, keepdim=True).clamp_min(1e-12) * torch.stack([gq, gk])[:, :, None, :].double() * 8.0

    def run(c):
        buf = c.inp(x, "qkv")                               # in / out: the pads around it are checked like an output's
        gqd, gkd = c.inp(gq, "gamma_q"), c.inp(gk, "gamma_k")
        if mode == 0:
            rc = lib.rap_qknorm(_lib.ptr(buf), TP, H, _lib.ptr(gqd), _lib.ptr(gkd), stream(dev))
        else:
            rc = lib.rap_qknorm_h16(mode, _lib.ptr(buf), TP, H, _lib.ptr(gqd), _lib.ptr(gkd), stream(dev))
        _lib.check(rc, "qknorm"); torch.cuda.synchronize()
        got = buf.cpu()
        if mode == 0:
            assert (got[:2].double() - ref).abs().max().item() < TK.NORM_BOUND
            assert torch.equal(got[2].view(I32), x[2].view(I32))               # v untouched, bit for bit
        else:
            assert rel_err(got, ref) < TH.ONE_ROUNDING * TH.ULP[mode] + TH.NORM_SLACK
        return [buf]
    run_both(dev, run)


# ---------------------------------------------------------------------------------------------
# positional encodings and the small elementwise / table entry points
# ---------------------------------------------------------------------------------------------
def test_posenc_x_and_token_sample_write_only_their_rows(lib, dev):
    g = torch.Generator().manual_seed(8)
    TP, B = 333, 3
    x = torch.randn(TP, 3, generator=g) * 1.5
    cu = torch.tensor([0, 100, 101, TP], dtype=I32)
    tok_ref = torch.repeat_interleave(torch.arange(B), (cu[1:] - cu[:-1]).long()).to(I32)
    ref_x = O.posenc(x.double())

    def run(c):
        ax = c.out_view(F32, (TP, 64), "ax")
        tok = c.out_view(I32, (TP,), "token_sample")
        xd, cud = c.inp(x, "x"), c.inp(cu, "cu_batch")
        _lib.check(lib.rap_posenc_x(_lib.ptr(xd), _lib.ptr(ax), TP, stream(dev)), "posenc_x")
        _lib.check(lib.rap_token_sample(_lib.ptr(cud), B, _lib.ptr(tok), stream(dev)), "token_sample")
        torch.cuda.synchronize()
        assert (ax.cpu()[:, :63].double() - ref_x).abs().max().item() < TK.POSENC_BOUND
        assert torch.equal(ax.cpu()[:, 63], torch.zeros(TP))
        assert torch.equal(tok.cpu(), tok_ref)
        return [ax, tok]
    run_both(dev, run)


@pytest.mark.parametrize("Fd", [0, 4, 40])
def test_posenc_static_writes_only_its_rows_of_128(lib, dev, Fd):
    g = torch.Generator().manual_seed(8 + Fd)
    TP, B = 333, 3
    cond = (torch.rand(TP, 3, generator=g) - 0.5) * 1.4
    feat = F.normalize(torch.randn(TP, Fd, generator=g), dim=1) if Fd else None
    scales = torch.rand(B, generator=g) * 45 + 5
    tok = torch.repeat_interleave(torch.arange(B), torch.tensor([100, 1, TP - 101])).to(I32)
    parts = [O.posenc(cond.double()), O.posenc(scales[tok.long()].double().unsqueeze(-1))] + ([feat.double()] if Fd else [])
    ref = torch.cat(parts, dim=-1)
    used = ref.shape[1]
    assert used == 84 + Fd

    def run(c):
        ast = c.out_view(F32, (TP, 128), "astatic")
        cd, sd, td, fd = c.inp(cond, "cond"), c.inp(scales, "scales"), c.inp(tok, "token_sample"), c.inp(feat, "feat")
        _lib.check(lib.rap_posenc_static(_lib.ptr(cd), _lib.ptr(sd), _lib.ptr(td), _lib.ptr(fd), Fd, _lib.ptr(ast), TP, stream(dev)), "posenc_static")
        torch.cuda.synchronize()
        got = ast.cpu()
        assert (got[:, :used].double() - ref).abs().max().item() < TK.POSENC_BOUND
        assert torch.equal(got[:, used:], torch.zeros(TP, 128 - used))
        return [ast]
    run_both(dev, run)


@pytest.mark.parametrize("dt", [1, 2], ids=["bf16", "f16"])
def test_convert_h16_writes_n_values_and_refuses_an_n_that_is_no_multiple_of_4(lib, dev, dt):
    g = torch.Generator().manual_seed(1)
    n = 4 * 251                                              # no multiple of the block's 1024 values
    x = torch.randn(n + 3, generator=g) * 10.0 ** torch.randint(-6, 5, (n + 3,), generator=g).float()

    def run(c):
        out = c.out_view(torch.int16, (n,), "dst")
        xd = c.inp(x[:n], "src")
        _lib.check(lib.rap_convert_h16(dt, _lib.ptr(xd), _lib.ptr(out), n, stream(dev)), "convert")
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), TH.to_h(x[:n], dt).view(torch.int16))
        return [out]
    run_both(dev, run)
    # values move four at a time (include/rapflow.h): an odd n is refused before any launch, nothing is written
    c = Case(dev, 0x00)
    out = c.out_view(torch.int16, (n + 3,), "dst")
    xd = c.inp(x, "src")
    assert lib.rap_convert_h16(dt, _lib.ptr(xd), _lib.ptr(out), n + 3, stream(dev)) == RAP_ERR_INVALID
    c.check()
    assert c.guards[0].untouched()


def test_x2_pack_and_unpack_write_only_their_rows(lib, dev):
    g = torch.Generator().manual_seed(1)
    rows, cols, ld = 37, 96, 160
    src = torch.randn(rows, ld, generator=g) * 10.0 ** torch.randint(-4, 3, (rows, ld), generator=g).float()
    want = TX.pack_ref(src[:, :cols].contiguous())

    def run(c):
        dst = c.out_view(F16, (rows, 2 * cols), "paired")
        sd = c.inp(src, "src")
        _lib.check(lib.rap_x2_pack(_lib.ptr(sd), ld, rows, cols, 1.0, _lib.ptr(dst), stream(dev)), "rap_x2_pack")
        torch.cuda.synchronize()
        assert torch.equal(dst.cpu().view(torch.int16), want.view(torch.int16))
        back = c.out_view(F32, (rows, cols), "unpacked")
        pd = c.inp(want, "paired in")
        _lib.check(lib.rap_x2_unpack(_lib.ptr(pd), rows, cols, 1.0, _lib.ptr(back), stream(dev)), "rap_x2_unpack")
        torch.cuda.synchronize()
        assert torch.equal(back.cpu(), (want[:, TX.x2_col(torch.arange(cols))].float() + want[:, TX.x2_col(torch.arange(cols)) + 32].float()))
        return [dst, back]
    run_both(dev, run)


def test_euler_step_writes_n_floats_when_n_is_no_multiple_of_4(lib, dev):
    g = torch.Generator().manual_seed(9)
    n = 3 * 333                                              # 999
    x, v = torch.randn(n, generator=g), torch.randn(n, generator=g)
    dt_ = 1.0 / 20
    t = 1 - 3 * dt_
    xn_ref, x0_ref = O.euler_step(x, t, dt_, lambda a, b: v)

    def run(c):
        x0, xn, tr = (c.out_view(F32, (n,), name) for name in ("x0_hat", "x_next", "traj_xt_slot"))
        xd, vd = c.inp(x, "x_t"), c.inp(v, "v")
        _lib.check(lib.rap_euler_step(_lib.ptr(xd), _lib.ptr(vd), t, dt_, _lib.ptr(x0), _lib.ptr(xn), _lib.ptr(tr), n, stream(dev)), "euler")
        torch.cuda.synchronize()
        assert torch.equal(x0.cpu(), x0_ref) and torch.equal(xn.cpu(), xn_ref) and torch.equal(tr.cpu(), xn_ref)
        return [x0, xn, tr]
    run_both(dev, run)


def test_geglu_interleave_writes_only_the_packed_weights_and_bias(lib, dev):
    g = torch.Generator().manual_seed(4)
    inner, K = 128, 96
    W = torch.randn(2 * inner, K, generator=g); b = torch.randn(2 * inner, generator=g)
    # rows [32 value | 32 gate] per 64 packed rows (kernels.h EPI_GEGLU): packed row 64 i + j = value row 32 i + j, 64 i + 32 + j = gate row
    src = torch.cat([torch.cat([torch.arange(32 * i, 32 * i + 32), inner + torch.arange(32 * i, 32 * i + 32)]) for i in range(inner // 32)])

    def run(c):
        Wp, bp = c.out_view(F32, (2 * inner, K), "Wp"), c.out_view(F32, (2 * inner,), "bp")
        Wd, bd = c.inp(W, "W"), c.inp(b, "b")
        _lib.check(lib.rap_geglu_interleave(_lib.ptr(Wd), _lib.ptr(bd), _lib.ptr(Wp), _lib.ptr(bp), inner, K, stream(dev)), "interleave")
        torch.cuda.synchronize()
        assert torch.equal(Wp.cpu(), W[src]) and torch.equal(bp.cpu(), b[src])
        return [Wp, bp]
    run_both(dev, run)


def test_adaln_table_stays_inside_its_table_and_its_documented_scratch(lib, dev):
    import rap_amd
    from rap_amd import synthetic as S
    d, L, rows = 256, 2, 5
    cfg = dict(S.RAP_12); cfg.update(embed_dim=d, num_heads=d // 64, num_layers=L, local_feat_dim=8)
    sd = S.make_weights(cfg, 4)
    m = rap_amd.PointCloudDiT(in_dim=0, out_dim=3, embed_dim=d, num_layers=L, num_heads=d // 64, local_feat_dim=8)
    m.load_state_dict(sd)
    m.to(dev)
    t = torch.tensor([1.0, 0.95, 0.5, 0.05, 0.3])
    sd64 = {k: v.double() for k, v in sd.items()}
    refs = {(i, a): torch.cat(O.adaln_scale_shift(sd64, f"transformer_layers.{i}.{which}_prenorm.", t), dim=-1)
            for i in range(L) for a, which in enumerate(("self", "global"))}

    def run(c):
        out = c.out_view(F32, (rows, 2 * L, 2 * d), "table")
        scratch = c.out_view(F32, (rows * (256 + 4 * L * d),), "scratch")      # exactly the extent include/rapflow.h documents
        td = c.inp(t, "t")
        _lib.check(lib.rap_adaln_table(m._handle, _lib.ptr(td), rows, _lib.ptr(scratch), _lib.ptr(out), stream(dev)), "adaln")
        torch.cuda.synchronize()
        got = out.cpu().double()
        for (i, a), ref in refs.items():
            assert (got[:, 2 * i + a] - ref).abs().max().item() < TK.ADALN_BOUND, (i, a)
        return [out]
    run_both(dev, run)


# ---------------------------------------------------------------------------------------------
# the small kernels between the GEMMs: rap_head_out3, rap_max_abs, rap_qk_logit_bound, rap_sanitize_cu (cases and references of
# tests/ring_cases.py, the bounds of tests/test_ring_edges_gpu.py)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [0, 64], ids=["ldy=K", "ldy=K+64"])
@pytest.mark.parametrize("TP,K", [(1, 128), (5, 384), (333, 512)])
def test_head_out3_writes_only_its_tp_rows_of_3(lib, dev, TP, K, extra):
    import ring_cases as RC
    y, W = RC.head_inputs(TP, K, extra)
    y[:, K:] = 0.0                                               # (the row gaps of the guarded input take the pad byte below)
    ref = RC.head_ref64(y, W)

    def run(c):
        v = c.out_view(F32, (TP, 3), "v")
        g = G.Guarded(TP * (K + extra) * 4, dev, fill=0, pitch=(K + extra) * 4, guard=c.pad, name="y")
        c.guards.append(g)
        yd = g.strided(F32, TP, K, K + extra)                    # the ldy - K floats after every row hold the pad byte: 0x00, then NaN
        yd.copy_(y[:, :K])
        Wd = c.inp(W, "W")
        _lib.check(lib.rap_head_out3(ctypes.c_void_p(yd.data_ptr()), K + extra, _lib.ptr(Wd), _lib.ptr(v), TP, K, stream(dev)), "head_out3")
        torch.cuda.synchronize()
        assert (v.cpu().double() - ref).abs().max().item() < TK.GEMM_BOUND
        return [v]
    run_both(dev, run)


@pytest.mark.parametrize("n", [1, 65, 999])
def test_max_abs_writes_one_float_and_reads_n(lib, dev, n):
    import ring_cases as RC
    x = RC.maxabs_input(RC.MaxAbsCase(n, "last", True))
    want = RC.maxabs_ref_bits(x)

    def run(c):
        g = c.out(4, name="max")
        g.interior.zero_()                                       # the contract: *out holds +0 before the call
        out = g.view(F32, (1,))
        xd = c.inp(x, "x")                                       # (pads of 0xFF are NaN beyond x: ignored if read, never a maximum)
        _lib.check(lib.rap_max_abs(_lib.ptr(xd), n, _lib.ptr(out), stream(dev)), "max_abs")
        torch.cuda.synchronize()
        assert int(out.view(I32).cpu()[0]) == want
        return [out]
    run_both(dev, run)


@pytest.mark.parametrize("H", [1, 12])
def test_qk_logit_bound_writes_one_float_per_head(lib, dev, H):
    import ring_cases as RC
    gq, gk = RC.bound_gammas(H, False)
    ref = RC.bound_ref64(gq, gk)

    def run(c):
        out = c.out_view(F32, (H,), "logit bound")
        gqd, gkd = c.inp(gq, "gamma_q"), c.inp(gk, "gamma_k")
        _lib.check(lib.rap_qk_logit_bound(_lib.ptr(gqd), _lib.ptr(gkd), H, _lib.ptr(out), stream(dev)), "qk_logit_bound")
        torch.cuda.synchronize()
        got = out.cpu().double()
        assert bool((got >= ref).all()) and bool((got <= ref * RC.BOUND_SLACK * (1 + 2.0 ** -22)).all())
        return [out]
    run_both(dev, run)


@pytest.mark.parametrize("n", [1, 1025, 5001])
def test_sanitize_cu_writes_n_entries(lib, dev, n):
    import ring_cases as RC
    cu, limit = RC.san_table(n, "dip_on_boundary" if n > 1 else "negative")
    ref = RC.san_ref(cu, limit)

    def run(c):
        out = c.out_view(I32, (n,), "sanitised")
        cud = c.inp(cu, "cu_seqlens")
        _lib.check(lib.rap_sanitize_cu(_lib.ptr(cud), n, limit, _lib.ptr(out), stream(dev)), "sanitize_cu")
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), ref)
        return [out]
    run_both(dev, run)
    # a refused call writes nothing
    c = Case(dev, 0x00)
    out = c.out_view(I32, (n,), "sanitised")
    cud = c.inp(cu, "cu_seqlens")
    assert lib.rap_sanitize_cu(_lib.ptr(cud), n, -1, _lib.ptr(out), stream(dev)) == RAP_ERR_INVALID
    c.check()
    assert c.guards[0].untouched()
