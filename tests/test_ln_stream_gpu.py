"""GPU: the residual-stream LayerNorm kernels of the 16-bit block at kernel level (norm_h16.hip: layernorm_h16_kernel<NV, DT, XH, COMB>,
layernorm_x2_kernel<NV, COMB>) and the two stream conversions, through rap_layernorm_*_h16_stream, rap_resid_combine_layernorm_h16,
rap_convert_f16_sat and rap_convert_f16_to_f32.

What is compared with what (cases and CPU references: tests/ln_stream_cases.py; tests/test_ln_stream_cases_host.py proves their claims):
  * the stream value a fused call stores: BITWISE against the kernel's own fp32 adds in the kernel's own order on the CPU (an fp16 stream:
    clamp to +-65504 and one rounding), NaN positions included;
  * every LayerNorm output: against fp64 on the STORED stream value, at the bounds tests/test_h16_gpu.py and tests/test_x2_gpu.py hold the
    same outputs to (rows holding +-65504 included: no wider yardstick was needed);
  * the fused output: also BITWISE against the plain LayerNorm entry point run on the stored stream value -- "combine, then LayerNorm,
    bit-identical" at every width, dtype, stream, split count and row tail;
  * the conversions: bitwise against torch on the CPU over every fp16 bit pattern / the saturation table.
Every call runs with its stream and its output inside guard bands of exactly `rows` rows (tests/guards.py), so a write by a row of the last
block's tail lands in a guard, and with its read-only operands compared bit for bit afterwards.

Measured on MI355X, worst LayerNorm error against fp64 over the plain, fused and special cases (bound beside it; the fp32 torch LayerNorm
rounded once gives 3.881e-3, 4.864e-4 and 2.65e-7 on the plain and fused cases):
  bf16 operands, fp32 stream 3.881e-3 (4.045e-3)      bf16, fp16 stream 3.880e-3 (4.045e-3)
  fp16 operands, fp32 stream 4.863e-4 (5.932e-4)      fp16, fp16 stream 4.864e-4 (5.932e-4)
  split precision, fp32 stream 2.855e-7 (5e-7)
Every stream-value and every fused-against-unfused comparison was bitwise.  Six arithmetic-only mutants of norm_h16.hip (built outside the
tree) each fail tests of this file: gain / shift through the narrow column map where the kernel uses the wide one (the plain, fused and
special tests at d = 512, 1024 on the fp16 stream); the plane loop starting at plane 1, the bias skipped, the plane stride from rows rounded
up to 4 (every fused and special test); the LayerNorm normalising the fp32 sum instead of the stored fp16 value (fused and special tests
on the fp16 stream, through the bitwise comparison with the unfused LayerNorm); an unsaturated store (the special test at every width).
"""
import ctypes
import itertools

import pytest
import torch

import guards as G
import ln_stream_cases as C
from rap_amd import _lib

pytestmark = pytest.mark.gpu

MODE_D = list(itertools.product(C.MODES, C.WIDTHS))
MODE_IDS = [f"dt{dt}-{s}-d{d}" for (dt, s), d in MODE_D]
F16_MODE_D = [((dt, s), d) for (dt, s), d in MODE_D if s == "f16"]
F16_MODE_IDS = [f"dt{dt}-{s}-d{d}" for (dt, s), d in F16_MODE_D]
WORST = {}      # (what, dtype, stream) -> worst LN error seen, printed per test


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def stream(dev):
    return _lib.current_stream(dev)


def bits(t):
    """integer view of a tensor's bytes on the CPU: NaN == NaN, -0 != +0"""
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


class Operands:
    """read-only device operands of one call, kept to be compared bit for bit afterwards"""

    def __init__(self, dev):
        self.dev, self.kept = dev, []

    def put(self, t, name):
        if t is None:
            return None
        d = t.to(self.dev).contiguous()
        self.kept.append((name, d, bits(t)))
        return d

    def unchanged(self):
        torch.cuda.synchronize()
        for name, d, before in self.kept:
            assert torch.equal(bits(d), before), f"{name} was written by the call"


def out_cols(dtype, d):
    return 2 * d if dtype == 3 else d


def out_dtype(dtype):
    return torch.bfloat16 if dtype == 1 else torch.float16


def guarded_stream(dev, h):
    """the stream tensor inside guard bands of exactly its own rows"""
    g = G.Guarded(h.numel() * h.element_size(), dev, fill=0, pitch=h.shape[1] * h.element_size(), name="stream")
    return g, g.put(h.to(dev))


def guarded_out(dev, dtype, rows, d):
    cols = out_cols(dtype, d)
    g = G.Guarded(rows * cols * 2, dev, fill=0xFF, pitch=cols * 2, name="out")
    return g, g.view(out_dtype(dtype), (rows, cols))


def ln_args(ops, form, d, rows):
    """-> the device operands of an LN form: (mod pointer or None, mod_stride, token_row, gain, shift)"""
    mod, gain, shift = C.ln_params(d)
    if form == "affine":
        return None, 0, None, ops.put(gain, "gain"), ops.put(shift, "shift")
    md = ops.put(mod, "mod")
    tok = ops.put(C.token_rows(rows), "token_row") if form == "mod_rows" else None
    mp = ctypes.c_void_p(md.data_ptr() + C.MOD_SLOT * 2 * d * 4)          # the LayerNorm's slot of table row 0
    return mp, C.TABLE_SLOTS * 2 * d, tok, None, None


def run_plain(lib, dev, dtype, stream_name, form, x, old_entry_point=False):
    """x: the stream as it is held (fp32 or fp16), CPU -> out on the CPU.  The stream is an input here: unchanged bit for bit."""
    rows, d = x.shape
    ops = Operands(dev)
    xd = ops.put(x, "x")
    mp, stride, tok, gain, shift = ln_args(ops, form, d, rows)
    go, out = guarded_out(dev, dtype, rows, d)
    f16 = int(stream_name == "f16")
    if form == "affine":
        if old_entry_point:
            rc = lib.rap_layernorm_affine_h16(dtype, _lib.ptr(xd), _lib.ptr(out), rows, d, _lib.ptr(gain), _lib.ptr(shift), stream(dev))
        else:
            rc = lib.rap_layernorm_affine_h16_stream(dtype, _lib.ptr(xd), f16, _lib.ptr(out), rows, d, _lib.ptr(gain), _lib.ptr(shift), stream(dev))
    elif old_entry_point:
        rc = lib.rap_layernorm_mod_h16(dtype, _lib.ptr(xd), _lib.ptr(out), rows, d, mp, stride, _lib.ptr(tok), stream(dev))
    else:
        rc = lib.rap_layernorm_mod_h16_stream(dtype, _lib.ptr(xd), f16, _lib.ptr(out), rows, d, mp, stride, _lib.ptr(tok), stream(dev))
    _lib.check(rc, "layernorm_h16_stream")
    go.check(); ops.unchanged()
    return out.cpu()


def run_fused(lib, dev, c, part, bias, h):
    """-> (the stream after the call, out), both on the CPU.  part, bias, the LN operands: unchanged bit for bit; nothing written beyond
    h[:rows] and out[:rows]"""
    ops = Operands(dev)
    pd, bd = ops.put(part, "part"), ops.put(bias, "bias")
    mp, stride, tok, gain, shift = ln_args(ops, c.form, c.d, c.rows)
    gh, hd = guarded_stream(dev, h)
    go, out = guarded_out(dev, c.dtype, c.rows, c.d)
    rc = lib.rap_resid_combine_layernorm_h16(c.dtype, _lib.ptr(pd), part.shape[0], _lib.ptr(bd), _lib.ptr(hd), int(c.stream == "f16"), _lib.ptr(out),
                                             c.rows, c.d, mp, stride, _lib.ptr(tok), _lib.ptr(gain), _lib.ptr(shift), stream(dev))
    _lib.check(rc, "resid_combine_layernorm_h16")
    gh.check(); go.check(); ops.unchanged()
    return hd.cpu(), out.cpu()


def logical(lib, dev, dtype, out, d):
    """the output as fp64 (rows, d): dtype 3 through rap_x2_unpack (head + tail)"""
    if dtype != 3:
        return out.double()
    od = out.to(dev)
    un = torch.empty(out.shape[0], d, device=dev)
    _lib.check(lib.rap_x2_unpack(_lib.ptr(od), out.shape[0], d, 1.0, _lib.ptr(un), stream(dev)), "rap_x2_unpack")
    torch.cuda.synchronize()
    return un.cpu().double()


def assert_ln(lib, dev, what, dtype, stream_name, out, stored, form, ctx):
    ref = C.ln_ref64(stored, form)
    err, bound = C.ln_error(dtype, logical(lib, dev, dtype, out, stored.shape[1]), ref)
    key = (what, dtype, stream_name)
    WORST[key] = max(WORST.get(key, 0.0), err)
    assert err < bound, (ctx, err, bound)


def report(what, dtype, stream_name, d, extra=""):
    bound = C.X2_NORM_BOUND if dtype == 3 else C.ONE_ROUNDING * C.ULP[dtype] + C.NORM_SLACK
    print(f"{what} dtype {dtype} stream {stream_name} d {d}: worst LN error vs fp64 so far {WORST.get((what, dtype, stream_name), 0.0):.3e} "
          f"(bound {bound:.3e}){extra}")


# ---------------------------------------------------------------------------------------------
# plain LayerNorm on either stream
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,d", MODE_D, ids=MODE_IDS)
def test_layernorm_on_either_stream_matches_fp64_at_every_row_tail(lib, dev, mode, d):
    """all three LN forms (adaLN through token_row, adaLN with token_row = NULL, affine) on an fp32 and an fp16 stream; on the fp32 stream the
    new entry points ARE the old ones, bit for bit"""
    dtype, stream_name = mode
    for c in C.plain_cases(dtype, stream_name, d):
        x = C.as_stream(C.stream_input(d, c.rows), stream_name)
        out = run_plain(lib, dev, dtype, stream_name, c.form, x)
        assert_ln(lib, dev, "plain", dtype, stream_name, out, x, c.form, c)
        if stream_name == "f32":
            assert same_bits(out, run_plain(lib, dev, dtype, stream_name, c.form, x, old_entry_point=True)), c
    report("plain", dtype, stream_name, d)


# ---------------------------------------------------------------------------------------------
# the fused combine + LayerNorm
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,d", MODE_D, ids=MODE_IDS)
def test_fused_combine_layernorm_stream_is_bitwise_and_out_equals_the_unfused_layernorm(lib, dev, mode, d):
    dtype, stream_name = mode
    for c in C.fused_cases(dtype, stream_name, d):
        part, bias, h = C.fused_inputs(c)
        stored = C.store(C.combine_sum(part, bias, h), stream_name)
        h_after, out = run_fused(lib, dev, c, part, bias, h)
        assert same_bits(h_after, stored), (c, "stream value", int((bits(h_after) != bits(stored)).sum()))
        assert_ln(lib, dev, "fused", dtype, stream_name, out, stored, c.form, c)
        assert same_bits(out, run_plain(lib, dev, dtype, stream_name, c.form, h_after)), (c, "fused out != LayerNorm of the stored stream")
    report("fused", dtype, stream_name, d, "; every stream value and every fused-vs-unfused comparison bitwise")


@pytest.mark.parametrize("mode,d", F16_MODE_D, ids=F16_MODE_IDS)
def test_fused_store_saturates_keeps_nan_and_leaves_the_other_rows_alone(lib, dev, mode, d):
    """sums beyond +-65504 (finite, by the residual alone, by overflow of fp32, +-inf), a sum that ROUNDS to 65504, one NaN, an fp16 subnormal,
    -0 and both halfway cases, each produced by the sum of two planes, bias and residual (tests/ln_stream_cases.py SPECIALS)"""
    dtype, stream_name = mode
    part, bias, h = C.special_inputs(d)
    part0, bias0, h0 = C.special_inputs(d, with_specials=False)
    stored = C.store(C.combine_sum(part, bias, h), "f16")
    nan_row, nan_col = C.SPECIALS["nan"][0], C.special_column("nan", d)
    clean = C.SPECIAL_CLEAN_ROWS
    for form in C.FORMS:
        c = C.FusedCase(dtype, stream_name, d, C.SPECIAL_ROWS, form, C.SPECIAL_SPLITS, True)
        h_after, out = run_fused(lib, dev, c, part, bias, h)
        assert same_bits(h_after, stored), (form, int((bits(h_after) != bits(stored)).sum()))
        hb = bits(h_after).to(torch.int32) & 0xFFFF
        for name, (r, _, _, _, _, want) in C.SPECIALS.items():
            col = C.special_column(name, d)
            if want is not None:
                assert int(hb[r, col]) == want, (name, hex(int(hb[r, col])))
            if name in C.SATURATED:
                assert float(h_after[r, col]) == C.SATURATED[name], name
        assert torch.isnan(h_after[nan_row, nan_col]) and int(torch.isnan(h_after).sum()) == 1
        assert not torch.isinf(h_after).any()
        assert torch.isnan(out[nan_row].float()).all(), "the NaN's own row"
        others = [r for r in range(C.SPECIAL_ROWS) if r != nan_row]
        assert torch.isfinite(out[others].float()).all()
        assert_ln(lib, dev, "special", dtype, stream_name, out, stored, form, form)         # the rows holding +-65504 at the ordinary bound
        assert same_bits(out, run_plain(lib, dev, dtype, stream_name, form, h_after)), form
        h_base, out_base = run_fused(lib, dev, c, part0, bias0, h0)
        assert same_bits(h_after[clean], h_base[clean]) and same_bits(out[clean], out_base[clean]), form
    report("special", dtype, stream_name, d)


# ---------------------------------------------------------------------------------------------
# conversions
# ---------------------------------------------------------------------------------------------
def convert_sat(lib, dev, xd, n):
    g = G.Guarded(n * 2, dev, fill=0xFF, name="fp16 stream")
    dst = g.view(torch.float16, (n,))
    _lib.check(lib.rap_convert_f16_sat(_lib.ptr(xd), _lib.ptr(dst), n, stream(dev)), "rap_convert_f16_sat")
    g.check()
    return g, dst


def convert_widen(lib, dev, hd, n):
    g = G.Guarded(n * 4, dev, fill=0xFF, name="fp32 image")
    dst = g.view(torch.float32, (n,))
    _lib.check(lib.rap_convert_f16_to_f32(_lib.ptr(hd), _lib.ptr(dst), n, stream(dev)), "rap_convert_f16_to_f32")
    g.check()
    return g, dst


def test_saturating_conversion_is_clamp_and_one_rounding(lib, dev):
    """every fp16 value, every midpoint between neighbours and one fp32 step either side, the edges of the range, NaN, +-inf; and prefixes of
    4 .. 1028 elements: nothing beyond n is written"""
    x = C.sat_table()
    ref = C.sat_ref(x)
    xd = x.to(dev)
    _, dst = convert_sat(lib, dev, xd, x.numel())
    got = dst.cpu()
    bad = (bits(got) != bits(ref)).nonzero().flatten()
    assert bad.numel() == 0, [(float(x[i]), float(got[i]), float(ref[i])) for i in bad[:8].tolist()]
    assert not torch.isinf(got).any() and torch.equal(torch.isnan(got), torch.isnan(x))
    for n in (4, 8, 1020, 1028):
        _, dst = convert_sat(lib, dev, xd, n)
        assert same_bits(dst.cpu(), ref[:n]), n
    assert same_bits(xd, x)


def test_widening_conversion_is_exact_on_every_bit_pattern(lib, dev):
    """all 65 536 fp16 bit patterns against torch's .float() on the CPU as int32: NaN payloads count"""
    h = C.all_f16_patterns()
    ref = C.widen_ref()
    hd = h.to(dev)
    _, dst = convert_widen(lib, dev, hd, h.numel())
    got = dst.cpu()
    bad = (bits(got) != bits(ref)).nonzero().flatten()
    assert bad.numel() == 0, [(hex(int(bits(h)[i]) & 0xFFFF), hex(int(bits(got)[i]) & 0xFFFFFFFF), hex(int(bits(ref)[i]) & 0xFFFFFFFF)) for i in bad[:8].tolist()]
    for n in (8, 16, 1016, 1032):
        _, dst = convert_widen(lib, dev, hd, n)
        assert same_bits(dst.cpu(), ref[:n]), n
    assert same_bits(hd, h)


def test_conversions_past_one_pass_of_the_grid(lib, dev):
    """n beyond 65 536 blocks x 256 threads x 4 (8) values: the grid-stride loops take a second trip.  The sources are the CPU tables tiled on
    the device with a period that is no divisor of the grid's stride, the references the CPU references tiled the same way."""
    x = C.sat_table()
    n = C.SAT_WRAP_N
    reps = -(-n // x.numel())
    xd = x.to(dev).repeat(reps)[:n].contiguous()
    want = C.sat_ref(x).to(dev).repeat(reps)[:n].view(torch.int16)
    g, dst = convert_sat(lib, dev, xd, n)
    assert torch.equal(dst.view(torch.int16), want)
    del xd, want, dst, g
    period = 65528                                                          # (tests/test_ln_stream_cases_host.py: 2^27 % 65528 != 0)
    h = C.all_f16_patterns()[4:4 + period].contiguous()
    n = C.WIDEN_WRAP_N
    reps = -(-n // period)
    hd = h.to(dev).repeat(reps)[:n].contiguous()
    want = C.widen_ref()[4:4 + period].to(dev).repeat(reps)[:n].view(torch.int32)
    g, dst = convert_widen(lib, dev, hd, n)
    assert torch.equal(dst.view(torch.int32), want)
    del hd, want, dst, g
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------
def test_refused_calls_return_invalid_and_write_nothing(lib, dev):
    """every refusal of include/rapflow.h with real device operands, at 4 rows and at none; rows = 0 / n = 0 with valid arguments is RAP_OK and
    writes nothing either"""
    d, rows = 1024, 4
    N = ctypes.c_void_p(0)
    gh = G.Guarded(rows * d * 4, dev, fill=0xFF, name="stream")
    go = G.Guarded(rows * 2 * d * 2, dev, fill=0xFF, name="out")
    src = torch.zeros(8 * rows * d, device=dev)                      # part / mod / gain / shift / x / conversion source
    H, O, S = ctypes.c_void_p(gh.ptr), ctypes.c_void_p(go.ptr), _lib.ptr(src)

    def ln_mod(dtype=2, x=S, f16=1, out=O, TP=rows, d=d, mod=S):
        return lib.rap_layernorm_mod_h16_stream(dtype, x, f16, out, TP, d, mod, 0, N, stream(dev))

    def ln_aff(dtype=2, x=S, f16=1, out=O, TP=rows, d=d, gain=S, shift=S):
        return lib.rap_layernorm_affine_h16_stream(dtype, x, f16, out, TP, d, gain, shift, stream(dev))

    def comb(dtype=2, part=S, splits=2, h=H, f16=1, out=O, rows=rows, d=d, mod=S, gain=N, shift=N):
        return lib.rap_resid_combine_layernorm_h16(dtype, part, splits, N, h, f16, out, rows, d, mod, 0, N, gain, shift, stream(dev))

    for r in (rows, 0):
        refused = [ln_mod(TP=r, x=N), ln_mod(TP=r, out=N), ln_mod(TP=r, mod=N),
                   ln_aff(TP=r, x=N), ln_aff(TP=r, out=N), ln_aff(TP=r, gain=N), ln_aff(TP=r, shift=N),
                   comb(rows=r, part=N), comb(rows=r, h=N), comb(rows=r, out=N),
                   comb(rows=r, mod=N), comb(rows=r, mod=N, gain=S), comb(rows=r, mod=N, shift=S)]
        for f, rk in ((ln_mod, "TP"), (ln_aff, "TP"), (comb, "rows")):
            refused += [f(dtype=v, **{rk: r}) for v in (0, 4, -1)] + [f(dtype=3, f16=1, **{rk: r})]
            refused += [f(f16=v, **{rk: r}) for v in (2, -1)] + [f(d=v, **{rk: r}) for v in (0, 128, 384, 1280, 2048)]
        refused += [comb(rows=r, splits=v) for v in (0, 9, -1)]
        assert refused and all(rc == -1 for rc in refused), (r, refused)
    assert ln_mod(TP=-1) == -1 and ln_aff(TP=-1) == -1 and comb(rows=-1) == -1
    sat, wid = lib.rap_convert_f16_sat, lib.rap_convert_f16_to_f32
    refused = [sat(N, O, 8, stream(dev)), sat(S, N, 8, stream(dev)), wid(N, H, 8, stream(dev)), wid(S, N, 8, stream(dev)),
               sat(S, O, -4, stream(dev)), wid(S, H, -8, stream(dev))]
    refused += [sat(S, O, n, stream(dev)) for n in (1, 2, 3, 6, 9)] + [wid(S, H, n, stream(dev)) for n in (1, 4, 7, 12, 20)]
    assert all(rc == -1 for rc in refused), refused
    # nothing to do, valid arguments: RAP_OK
    assert ln_mod(TP=0) == 0 and ln_aff(TP=0) == 0 and comb(rows=0) == 0 and comb(rows=0, dtype=3, f16=0, splits=8) == 0
    assert sat(S, O, 0, stream(dev)) == 0 and wid(S, H, 0, stream(dev)) == 0
    gh.check(); go.check()
    assert gh.untouched() and go.untouched(), "a refused or empty call wrote into its stream / output"
    assert not src.any()
