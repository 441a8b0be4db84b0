"""GPU: edge sweep of the kernels that run BETWEEN the GEMMs on every flow step, through the C ABI, against the references of
tests/ring_cases.py (tests/test_ring_cases_host.py proves on the CPU that the cases reach what they are listed for and that the references
hold their bounds).  Every output is NaN- or sentinel-initialised and compared in full; every case is a handful of small launches.

Which case catches which wrong kernel:
  * a one-pass variance (E[x^2] - mean^2)            test_layernorm_f32_row_families[mean1000-*] (and mean50)
  * head = r / (TP + 1) in either qk-norm           test_qknorm_edges[*-H3|H8|H16] (per-head gammas, every TP)
  * a dropped second grid pass                      the 32 769 / 40 001-row head tail, n = 524 289 / 786 432 Euler, n = 262 145 / 1 000 003
                                                    max |x| (maximum inside the second pass), the three *_past_one_grid_pass conversions
  * swapped sin / cos columns                       test_posenc_edges (every TP)
  * a chunk-boundary slip in the sanitiser          test_sanitize_cu[*] table dip_on_boundary
  * an Euler update that reads x_t after writing it test_euler_step_forms[*-in_place]
"""
import ctypes

import pytest
import torch

import ln_stream_cases as L
import ring_cases as C
from rap_amd import _lib

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENTINEL16 = 0x5A5A          # a finite value in fp16 and in bf16: what a 16-bit output holds before the call


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def run(rc, dev, what):
    _lib.check(rc, what)
    torch.cuda.synchronize(dev)


def st(dev):
    return _lib.current_stream(dev)


def same16(got, want):
    """16-bit tensors on one device: the same bits, or NaN on both sides"""
    return bool(((got.view(torch.int16) == want.view(torch.int16)) | (torch.isnan(got) & torch.isnan(want))).all())


def tiled(t, rows):
    """the first `rows` rows of t repeated along dim 0"""
    reps = -(-rows // t.shape[0])
    return t.repeat(reps, *([1] * (t.dim() - 1)))[:rows].contiguous()


# ---------------------------------------------------------------------------------------------
# fp32 LayerNorm
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", C.LN_FAMILIES)
@pytest.mark.parametrize("d", C.LN_WIDTHS)
def test_layernorm_f32_row_families(lib, dev, d, family):
    mod, gain, shift = (t.to(dev) for t in C.ln_params(d))
    slot = ctypes.c_void_p(mod.data_ptr() + L.MOD_SLOT * 2 * d * 4)
    worst = 0.0
    for rows in C.LN_ROWS:
        x = C.ln_input(d, rows, family)
        xd, tok = x.to(dev), L.token_rows(rows).to(dev)
        for form in C.LN_FORMS:
            out = torch.full((rows, d), NAN, device=dev)
            if form == "affine":
                rc = lib.rap_layernorm_affine(_lib.ptr(xd), _lib.ptr(out), rows, d, _lib.ptr(gain), _lib.ptr(shift), st(dev))
            else:
                rc = lib.rap_layernorm_mod(_lib.ptr(xd), _lib.ptr(out), rows, d, slot, L.TABLE_SLOTS * 2 * d,
                                           _lib.ptr(tok if form == "mod_rows" else None), st(dev))
            run(rc, dev, "layernorm")
            got = out.cpu()
            assert not torch.isnan(got).any(), (rows, form)
            err, bound = float((got.double() - C.ln_ref64(x, form)).abs().max()), C.ln_bound(x, form)
            worst = max(worst, err / bound)
            assert err < bound, (rows, form, err, bound)
            if family in C.LN_EXACT:
                assert torch.equal(got, C.ln_shift_rows(form, d, rows)), (rows, form)      # x - mean == 0: the shift, exactly
    print(f"LayerNorm d {d} {family}: worst error {worst:.2f} of the bound")


# ---------------------------------------------------------------------------------------------
# qk-norm
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", C.QK_HEADS, ids=lambda h: f"H{h}")
@pytest.mark.parametrize("mode", [0, 1, 2], ids=["f32", "bf16", "f16"])
def test_qknorm_edges(lib, dev, mode, H):
    gq, gk = (g.to(dev) for g in C.qk_gammas(H))
    worst = 0.0
    for TP in C.QK_ROWS:
        x = C.qk_input(H, TP, mode)
        buf = x.to(dev).clone()
        if mode == 0:
            rc = lib.rap_qknorm(_lib.ptr(buf), TP, H, _lib.ptr(gq), _lib.ptr(gk), st(dev))
        else:
            rc = lib.rap_qknorm_h16(mode, _lib.ptr(buf), TP, H, _lib.ptr(gq), _lib.ptr(gk), st(dev))
        run(rc, dev, "qknorm")
        got = buf.cpu()
        assert torch.isfinite(got.float()).all(), TP
        err, bound = C.qk_error(mode, got[:2], C.qk_ref64(x), H)
        worst = max(worst, err / bound)
        assert err < bound, (TP, err, bound)
        assert C.same_bits_or_both_nan(got[2], x[2]), TP                        # the plane behind q and k: untouched, bit for bit
    print(f"qk-norm mode {mode} H {H}: worst error {worst:.2f} of the bound")


# ---------------------------------------------------------------------------------------------
# positional encodings
# ---------------------------------------------------------------------------------------------
def posenc_x(lib, dev, x):
    xd = x.to(dev)
    ax = torch.full((x.shape[0], 64), NAN, device=dev)
    run(lib.rap_posenc_x(_lib.ptr(xd), _lib.ptr(ax), x.shape[0], st(dev)), dev, "posenc_x")
    return ax.cpu()


def posenc_static(lib, dev, cond, Fd):
    TP = cond.shape[0]
    cd, sc, tok = cond.to(dev), C.PE_SCALES.to(dev), C.pe_token_sample(TP).to(dev)
    feat = C.pe_feat(TP, Fd)
    fd = feat.to(dev) if Fd else None
    out = torch.full((TP, 128), NAN, device=dev)
    run(lib.rap_posenc_static(_lib.ptr(cd), _lib.ptr(sc), _lib.ptr(tok), _lib.ptr(fd), Fd, _lib.ptr(out), TP, st(dev)), dev, "posenc_static")
    return out.cpu()


def check_nan_stays_in_its_columns(clean, dirty, row, comp):
    cols = C.pe_columns_of_component(comp)
    others = [c for c in range(clean.shape[1]) if c not in cols]
    assert bool(torch.isnan(dirty[row, cols]).all())
    assert torch.equal(C.bits32(dirty[row, others]), C.bits32(clean[row, others]))
    keep = torch.arange(clean.shape[0]) != row
    assert torch.equal(C.bits32(dirty[keep]), C.bits32(clean[keep]))


@pytest.mark.parametrize("TP", C.PE_ROWS)
def test_posenc_edges(lib, dev, TP):
    x = C.pe_coords(TP, "x")
    ax = posenc_x(lib, dev, x)
    err = float((ax.double() - C.pe_x_ref64(x)).abs().max())
    assert err < C.POSENC_BOUND, err
    assert torch.equal(C.bits32(ax[:, :3]), C.bits32(x)) and torch.equal(C.bits32(ax[:, 63]), C.bits32(torch.zeros(TP)))
    worst = err
    cond = C.pe_coords(TP, "cond")
    for Fd in C.PE_FEAT_DIMS:
        got = posenc_static(lib, dev, cond, Fd)
        ref = C.pe_static_ref64(cond, Fd)
        err = float((got.double() - ref).abs().max())
        worst = max(worst, err)
        assert err < C.POSENC_BOUND, (Fd, err)
        raw = C.pe_raw_columns_static(Fd)
        assert torch.equal(C.bits32(got[:, raw]), C.bits32(ref[:, raw].float())), Fd
        assert torch.equal(C.bits32(got[:, 84 + Fd:]), C.bits32(torch.zeros(TP, 44 - Fd))), Fd       # every pad column: +0
    # one NaN coordinate: NaN in the columns that depend on it, every other element unchanged bit for bit
    row, comp = TP // 2, 1
    bad = x.clone()
    bad[row, comp] = NAN
    check_nan_stays_in_its_columns(ax, posenc_x(lib, dev, bad), row, comp)
    badc = cond.clone()
    badc[row, comp] = NAN
    check_nan_stays_in_its_columns(posenc_static(lib, dev, cond, 8), posenc_static(lib, dev, badc, 8), row, comp)
    print(f"posenc TP {TP}: worst error {worst:.2e}")


# ---------------------------------------------------------------------------------------------
# adaLN table
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,L_", C.ADALN_MODELS, ids=[f"d{d}-L{n}" for d, n in C.ADALN_MODELS])
def test_adaln_table_row_chunks(lib, dev, d, L_):
    import rap_amd
    sd = C.adaln_weights(d, L_)
    m = rap_amd.PointCloudDiT(in_dim=0, out_dim=3, embed_dim=d, num_layers=L_, num_heads=d // 64, local_feat_dim=8)
    m.load_state_dict(sd)
    m.to(dev)
    ref_all = C.adaln_ref(sd, L_, C.adaln_t(max(C.ADALN_ROWS)))
    worst = 0.0
    for rows in C.ADALN_ROWS:
        td = C.adaln_t(rows).to(dev)
        out = torch.full((rows, 2 * L_, 2 * d), NAN, device=dev)
        scratch = torch.full((rows * (256 + 4 * L_ * d),), NAN, device=dev)
        run(lib.rap_adaln_table(m._handle, _lib.ptr(td), rows, _lib.ptr(scratch), _lib.ptr(out), st(dev)), dev, "adaln")
        got = out.cpu()
        err = float((got.double() - ref_all[:rows]).abs().max())
        worst = max(worst, err)
        assert err < C.ADALN_BOUND, (rows, err)
        # a row's result does not depend on which chunk of 8 it is in, nor on where in the chunk: the same t gives the same bits
        for r in range(C.ADALN_CHUNK, rows):
            assert torch.equal(C.bits32(got[r]), C.bits32(got[r % C.ADALN_CHUNK])), (rows, r)
        if rows >= 5:
            assert torch.equal(C.bits32(got[3]), C.bits32(got[4]))              # t[3] == t[4]
    print(f"adaLN d {d} L {L_}: worst error {worst:.2e}")


# ---------------------------------------------------------------------------------------------
# head tail
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", C.HEAD_LD_EXTRA, ids=["ldy=K", "ldy=K+64"])
@pytest.mark.parametrize("K", C.HEAD_KS)
def test_head_out3_lane_edges_and_second_pass(lib, dev, K, extra):
    worst = 0.0
    for TP in C.HEAD_ROWS:
        y, W = C.head_inputs(TP, K, extra)
        yd, Wd = y.to(dev), W.to(dev)
        v = torch.full((TP, 3), NAN, device=dev)
        run(lib.rap_head_out3(_lib.ptr(yd), K + extra, _lib.ptr(Wd), _lib.ptr(v), TP, K, st(dev)), dev, "head_out3")
        got = v.cpu()
        assert not torch.isnan(got).any(), TP                                   # (the columns between K and ldy hold NaN: never read)
        err = float((got.double() - C.head_ref64(y, W)).abs().max())
        worst = max(worst, err)
        assert err < C.GEMM_BOUND, (TP, err)
    print(f"head tail K {K} ldy {K + extra}: worst error {worst:.2e}")


# ---------------------------------------------------------------------------------------------
# Euler update
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", C.EULER_FORMS)
@pytest.mark.parametrize("n", C.EULER_NS)
def test_euler_step_forms(lib, dev, n, form):
    x, v = C.euler_inputs(n)
    xn_ref, x0_ref = C.euler_ref(x, v)
    xd, vd = x.to(dev), v.to(dev)
    x0 = torch.full((n,), NAN, device=dev)
    xn = xd if form == "in_place" else torch.full((n,), NAN, device=dev)       # in place: x_next IS x_t, as rap_sample calls it
    tr = torch.full((n,), NAN, device=dev) if form == "trajectory" else None
    run(lib.rap_euler_step(_lib.ptr(xd), _lib.ptr(vd), C.EULER_T, C.EULER_DT, _lib.ptr(x0), _lib.ptr(xn), _lib.ptr(tr), n, st(dev)), dev, "euler")
    assert torch.equal(C.bits32(x0.cpu()), C.bits32(x0_ref)) and torch.equal(C.bits32(xn.cpu()), C.bits32(xn_ref))
    assert torch.equal(vd.cpu(), v)
    if form == "trajectory":
        assert torch.equal(C.bits32(tr.cpu()), C.bits32(xn_ref))
    if form != "in_place":
        assert torch.equal(xd.cpu(), x)


# ---------------------------------------------------------------------------------------------
# conversions
# ---------------------------------------------------------------------------------------------
def convert(lib, dev, dt, xd):
    out = torch.full((xd.numel(),), SENTINEL16, dtype=torch.int16, device=dev)
    run(lib.rap_convert_h16(dt, _lib.ptr(xd), _lib.ptr(out), xd.numel(), st(dev)), dev, "convert_h16")
    return out.view(C.TORCH_DT[dt])


@pytest.mark.parametrize("dt", [1, 2], ids=["bf16", "f16"])
def test_convert_h16_every_pattern_tie_and_edge(lib, dev, dt):
    x = C.convert_table(dt)
    got = convert(lib, dev, dt, x.to(dev)).cpu()
    want = C.convert_ref(x, dt)
    bad = ~((got.view(torch.int16) == want.view(torch.int16)) | (torch.isnan(got) & torch.isnan(want)))
    assert not bad.any(), (int(bad.sum()), x[bad][:8].tolist(), got[bad][:8].tolist(), want[bad][:8].tolist())


@pytest.mark.parametrize("dt", [1, 2], ids=["bf16", "f16"])
def test_convert_h16_past_one_grid_pass(lib, dev, dt):
    x = C.convert_table(dt)
    n = C.CONVERT_WRAP_N
    got = convert(lib, dev, dt, tiled(x.to(dev), n))
    assert same16(got, tiled(C.convert_ref(x, dt).to(dev), n))


@pytest.mark.parametrize("cols", C.X2_COLS)
def test_x2_pack_unpack_edges(lib, dev, cols):
    src = C.x2_source(cols)
    x = src[:, :cols].contiguous()
    want = C.x2_pack_ref(x)
    sd = src.to(dev)
    dst = torch.full((C.X2_ROWS, 2 * cols), SENTINEL16, dtype=torch.int16, device=dev).view(torch.float16)
    run(lib.rap_x2_pack(_lib.ptr(sd), cols + C.X2_LD_EXTRA, C.X2_ROWS, cols, 1.0, _lib.ptr(dst), st(dev)), dev, "x2_pack")
    got = dst.cpu()
    assert C.same_bits_or_both_nan(got, want)
    # head + tail in fp64 is the clipped input; beyond +-65504 the pair clips (finite head, zero tail); NaN stays NaN in both planes
    k = torch.arange(cols)
    hi, lo = got[:, L.x2_col(k)].double(), got[:, L.x2_col(k) + 32].double()
    clip, ok = C.x2_clipped(x), ~torch.isnan(x)
    assert bool(((hi + lo - clip.double()).abs()[ok] <= C.x2_pair_bound(clip)[ok]).all())
    big = ok & (x.abs() > C.F16_MAX)
    assert bool((hi[big] == torch.sign(x[big]).double() * C.F16_MAX).all()) and bool((lo[big] == 0).all()) and int(big.sum()) >= 4
    assert bool(torch.isnan(hi[~ok]).all()) and bool(torch.isnan(lo[~ok]).all())
    back = torch.full((C.X2_ROWS, cols), NAN, device=dev)
    wd = want.to(dev)
    run(lib.rap_x2_unpack(_lib.ptr(wd), C.X2_ROWS, cols, 1.0, _lib.ptr(back), st(dev)), dev, "x2_unpack")
    assert C.same_bits_or_both_nan(back.cpu(), C.x2_unpack_ref(want, cols))
    assert bool(torch.isnan(back.cpu()[~ok]).all()) and not torch.isnan(back.cpu()[ok]).any()


def test_x2_pack_past_one_grid_pass(lib, dev):
    rows, cols = C.X2_PACK_WRAP
    x = C.x2_source(cols)[:, :cols].contiguous()
    sd = tiled(x.to(dev), rows)
    dst = torch.full((rows, 2 * cols), SENTINEL16, dtype=torch.int16, device=dev).view(torch.float16)
    run(lib.rap_x2_pack(_lib.ptr(sd), cols, rows, cols, 1.0, _lib.ptr(dst), st(dev)), dev, "x2_pack")
    assert same16(dst, tiled(C.x2_pack_ref(x).to(dev), rows))


def test_x2_unpack_past_one_grid_pass(lib, dev):
    rows, cols = C.X2_UNPACK_WRAP
    p = C.x2_pack_ref(C.x2_source(cols)[:, :cols].contiguous())
    pd = tiled(p.to(dev), rows)
    out = torch.full((rows, cols), NAN, device=dev)
    run(lib.rap_x2_unpack(_lib.ptr(pd), rows, cols, 1.0, _lib.ptr(out), st(dev)), dev, "x2_unpack")
    want = tiled(C.x2_unpack_ref(p, cols).to(dev), rows)
    assert bool(((out.view(torch.int32) == want.view(torch.int32)) | (torch.isnan(out) & torch.isnan(want))).all())
    assert int(torch.isnan(out).sum()) == int(torch.isnan(want).sum())


# ---------------------------------------------------------------------------------------------
# max |x|
# ---------------------------------------------------------------------------------------------
def max_abs_bits(lib, dev, x):
    xd = x.to(dev)
    out = torch.zeros(1, device=dev)                                            # pre-zeroed, as the contract says
    run(lib.rap_max_abs(_lib.ptr(xd), x.numel(), _lib.ptr(out), st(dev)), dev, "max_abs")
    return int(out.view(torch.int32).cpu()[0])


@pytest.mark.parametrize("case", C.maxabs_cases(), ids=lambda c: f"n{c.n}-{c.place}-{'neg' if c.negative else 'pos'}")
def test_max_abs_places(lib, dev, case):
    x = C.maxabs_input(case)
    assert max_abs_bits(lib, dev, x) == C.maxabs_ref_bits(x) == int(C.bits32(torch.tensor([77.5]))[0])


@pytest.mark.parametrize("name", list(C.MAXABS_SPECIALS))
def test_max_abs_special_values(lib, dev, name):
    vals, want = C.MAXABS_SPECIALS[name]
    x = torch.tensor(vals).repeat(100)
    assert max_abs_bits(lib, dev, x) == want == C.maxabs_ref_bits(x)


# ---------------------------------------------------------------------------------------------
# segment-table sanitiser
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.SAN_NS)
def test_sanitize_cu(lib, dev, n):
    for table in C.SAN_TABLES:
        cu, limit = C.san_table(n, table)
        cud = cu.to(dev)
        out = torch.full((n + 8,), -1, dtype=torch.int32, device=dev)
        run(lib.rap_sanitize_cu(_lib.ptr(cud), n, limit, _lib.ptr(out), st(dev)), dev, "sanitize_cu")
        got = out.cpu()
        assert torch.equal(got[:n], C.san_ref(cu, limit)), table
        assert bool((got[n:] == -1).all()), table
        if table == "consistent":
            assert torch.equal(got[:n], cu)                                     # a consistent table comes back as it went in


# ---------------------------------------------------------------------------------------------
# logit bound of the bounded softmax
# ---------------------------------------------------------------------------------------------
def logit_bound(lib, dev, gq, gk):
    H = gq.shape[0]
    gqd, gkd = gq.to(dev), gk.to(dev)
    out = torch.full((H + 4,), NAN, device=dev)
    run(lib.rap_qk_logit_bound(_lib.ptr(gqd), _lib.ptr(gkd), H, _lib.ptr(out), st(dev)), dev, "qk_logit_bound")
    got = out.cpu()
    assert bool(torch.isnan(got[H:]).all())
    return got[:H]


@pytest.mark.parametrize("H", C.BOUND_HEADS, ids=lambda h: f"H{h}")
def test_qk_logit_bound_value(lib, dev, H):
    for aligned in (False, True):
        gq, gk = C.bound_gammas(H, aligned)
        B, ref = logit_bound(lib, dev, gq, gk), C.bound_ref64(gq, gk)
        for h in range(H):
            want = float(ref[h]) * C.BOUND_SLACK
            assert float(B[h]) >= float(ref[h]), (h, float(B[h]), float(ref[h]))                # never below the exact bound
            assert abs(float(B[h]) - want) <= 2 * C.ulp32(want), (h, float(B[h]), want)


def scores(qk):
    """(2, H, TP, 64) -> q.k / 8 in fp64 for every query / key pair of a head: (H, TP, TP)"""
    q, k = qk[0].double(), qk[1].double()
    return (q[:, :, None, :] * k[:, None, :, :]).sum(-1) / 8.0


@pytest.mark.parametrize("H", C.BOUND_HEADS, ids=lambda h: f"H{h}")
def test_qk_logit_bound_holds_for_what_the_kernels_write(lib, dev, H):
    """The property the bound exists for, on its tight case: rows that are one-hot on the column holding the largest |gamma| of both planes.
    q.k / 8 from what each kernel WROTE: at most B in fp32 and fp16 (two roundings of unit roundoff 2^-11 fit inside the 0.1 % slack), at
    most B (1 + 2^-7) in bf16 (two roundings of 2^-8; include/rapflow.h states exactly that).  Heads 0 and 1 carry the gammas that round
    up by nearly the whole unit roundoff in bf16 and in fp16.  The fused projection needs N = 192 H to be a multiple of 128: not H = 1."""
    gq, gk = C.bound_gammas(H, True)
    B = logit_bound(lib, dev, gq, gk).double()
    gqd, gkd = gq.to(dev), gk.to(dev)
    x = C.bound_onehot_rows(H)
    TP = x.shape[2]
    ratios = {}
    buf = torch.cat([x, torch.zeros(1, H, TP, 64)]).to(dev)
    run(lib.rap_qknorm(_lib.ptr(buf), TP, H, _lib.ptr(gqd), _lib.ptr(gkd), st(dev)), dev, "qknorm")
    ratios[("rap_qknorm", 0)] = scores(buf.cpu()[:2]) / B[:, None, None]
    K = max(128, 64 * H)
    for dt in (1, 2):
        T = C.TORCH_DT[dt]
        buf = x.to(T).to(dev)
        run(lib.rap_qknorm_h16(dt, _lib.ptr(buf), TP, H, _lib.ptr(gqd), _lib.ptr(gkd), st(dev)), dev, "qknorm_h16")
        ratios[("rap_qknorm_h16", dt)] = scores(buf.cpu()) / B[:, None, None]
        # the fused projection with identity-like weights: token m is one-hot per head in A, the q block of W is the identity, the k block
        # the identity times the sign that makes q.k positive
        A, W = torch.zeros(TP, K), torch.zeros(3 * H * 64, K)
        for h in range(H):
            c = C.bound_lane(h)
            A[:, h * 64 + c] = x[0, h, :, c]
            sgn = float(torch.sign(x[1, h, -1, c] * x[0, h, 0, c]))
            j = torch.arange(64)
            W[h * 64 + j, h * 64 + j] = 1.0
            W[H * 64 + h * 64 + j, h * 64 + j] = sgn
            W[2 * H * 64 + h * 64 + j, h * 64 + j] = 1.0
        if H % 2:
            continue
        Ad, Wd = A.to(T).to(dev), W.to(T).to(dev)
        qk = torch.full((2, H, TP, 64), NAN, dtype=T, device=dev)
        vt = torch.full((H, 4, 64, 64), NAN, dtype=T, device=dev)
        run(lib.rap_gemm_h16_qkvnorm(dt, _lib.ptr(Ad), K, _lib.ptr(Wd), K, _lib.ptr(qk), TP, K, H, _lib.ptr(gqd), _lib.ptr(gkd), 8.0,
                                     _lib.ptr(vt), 4, st(dev)), dev, "gemm_h16_qkvnorm")
        ratios[("rap_gemm_h16_qkvnorm", dt)] = scores(qk.cpu()) / B[:, None, None]
    for (path, mode), r in ratios.items():
        print(f"H {H} {path} mode {mode}: worst q.k / 8 / B = {float(r.max()):.5f} (smallest {float(r.min()):.5f})")
        assert torch.isfinite(r).all() and float(r.min()) > 0.99, (path, mode)               # the tight case: every pair sits at the bound
        assert float(r.max()) <= C.BOUND_EXCESS[mode], (path, mode, float(r.max()))


# ---------------------------------------------------------------------------------------------
# GEGLU interleave
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inner", C.GEGLU_INNERS)
def test_geglu_interleave_is_an_exact_permutation(lib, dev, inner):
    src = C.geglu_source_rows(inner)
    for K in C.GEGLU_KS:
        W, b = C.geglu_inputs(inner, K)
        Wd, bd = W.to(dev), b.to(dev)
        Wp, bp = torch.full((2 * inner, K), NAN, device=dev), torch.full((2 * inner,), NAN, device=dev)
        run(lib.rap_geglu_interleave(_lib.ptr(Wd), _lib.ptr(bd), _lib.ptr(Wp), _lib.ptr(bp), inner, K, st(dev)), dev, "geglu_interleave")
        assert torch.equal(C.bits32(Wp.cpu()), C.bits32(W[src])) and torch.equal(C.bits32(bp.cpu()), C.bits32(b[src])), K
