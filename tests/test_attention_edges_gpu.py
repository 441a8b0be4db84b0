"""GPU: the attention kernels at their segment edges and, through rap_attention_f32_split / rap_x2_attention_split, the split-KV forms
that few-token model calls run (attention_f32_kernel<4, true, true> + attention_combine_kernel, attention_x2_kernel<2, true> +
attention_x2_combine_kernel), each against an fp64 evaluation of the same segments.

  a. every (start mod 64, length) pair of tests/attention_cases.py through every unsplit kernel: fp32 online / bounded, split precision
     with one / two blocks per CU, bf16 / fp16 with every item size and key-group form of tuning key 20, online / bounded;
  b. the same tables through the split forms at 2 and 4 key ranges; 1 range is the unsplit entry point bit for bit; a repeated call
     is bit-identical (fixed merge order);
  c. a softmax whose partial maxima differ by far more than the deferred-rescale threshold when they meet in the combine pass: one
     dominant key at the first, the last and the interior key of every range; partial maxima further apart than fp32's exponent range;
     all logits close to minus the declared bound;
  d. rows outside the segment table come out as zeros, rows from n_tokens on are not written;
  e. a bound above 40 is refused with NaN by the split form too.

Bounds: those of the kernels' own ragged tests (imported); the two fp32 cases of (c) as attention_cases.FP32_SHARP_FACTOR states.
Every workspace is handed over full of 0xFF, every output full of NaN."""
import functools

import pytest
import torch

import attention_cases as A
import test_h16_gpu as TH
import test_kernels_gpu as TK
import test_x2_gpu as TX
from rap_amd import _lib

pytestmark = pytest.mark.gpu

H16_KEY20 = [0, 64, 128, 66, 130]       # 256-row items; forced 64 / 128-row items; 64 rows x 4 / 128 rows x 2 key groups
DT_NAME = {1: "bf16", 2: "f16"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def stream(dev):
    return _lib.current_stream(dev)


def report(family, case, err, bound):
    print(f"EDGES {family:<28} {case:<40} max abs err vs fp64 {err:.3e}  (bound {bound:.3e})")


def err_vs(out, ref):
    assert not torch.isnan(out).any(), "NaN left in covered rows"
    return float((out.double() - ref).abs().max())


def raw_bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ---- one fp64 reference per (table, rounding), shared by every parametrisation ----
@functools.lru_cache(maxsize=None)
def sweep_ref(start, dt=0):
    q, k, v = A.sweep_operands(start)
    cu = torch.tensor(A.sweep_table(start))
    return TH.attention_ref64(q, k, v, cu, dt) if dt else TX.attention_ref64(q, k, v, cu)


def qkv_thd(q, k, v):
    return torch.stack([q, k, v]).permute(2, 0, 1, 3).contiguous()      # (T, 3, H, 64), what test_kernels_gpu.run_attention takes


def fresh_ws(dev, nbytes):
    return torch.full((max(int(nbytes), 1),), 0xFF, dtype=torch.uint8, device=dev)


def run_f32_split(lib, dev, q, k, v, cu, bound, splits, entry="split"):
    """(H, TP, 64) fp32 -> out (TP, H * 64) fp32 on the CPU, NaN wherever the call wrote nothing.  entry "unsplit": rap_attention_f32"""
    Hh, TP, _ = q.shape
    hm = torch.stack([q, k, v]).contiguous().to(dev)                     # [3][H][TP][64]
    cu_d = torch.tensor(cu, dtype=torch.int32, device=dev)
    bound_d = None if bound is None else bound.to(device=dev, dtype=torch.float32)
    out = torch.full((TP, Hh * 64), float("nan"), device=dev)
    nseg = len(cu) - 1
    if entry == "unsplit":
        ws = fresh_ws(dev, lib.rap_attention_workspace_bytes(TP, nseg))
        rc = lib.rap_attention_f32(_lib.ptr(hm), _lib.ptr(cu_d), nseg, _lib.ptr(out), TP, Hh, _lib.ptr(bound_d), _lib.ptr(ws), ws.numel(), stream(dev))
    else:
        need = lib.rap_attention_split_workspace_bytes(TP, nseg, Hh, splits)
        assert need > 0
        ws = fresh_ws(dev, need)
        rc = lib.rap_attention_f32_split(_lib.ptr(hm), _lib.ptr(cu_d), nseg, _lib.ptr(out), TP, Hh, _lib.ptr(bound_d), splits, _lib.ptr(ws), need,
                                         stream(dev))
    _lib.check(rc, "rap_attention_f32" + ("" if entry == "unsplit" else "_split"))
    torch.cuda.synchronize()
    return out.cpu()


class X2Operands:
    """the paired planes of one (q, k, v) on the device, packed once"""

    def __init__(self, dev, q, k, v):
        self.H, self.TP = q.shape[0], q.shape[1]
        qk, vt, self.nblk = TX.make_x2_attention_operands(q, k, v)
        self.qk, self.vt = qk.to(dev), vt.to(dev)


def run_x2_split(lib, dev, op, cu, splits, n_tokens=0, entry="split"):
    """-> the raw paired fp16 out (TP, 2 * H * 64) on the CPU, NaN wherever the call wrote nothing.  entry "unsplit": rap_x2_attention"""
    cu_d = torch.tensor(cu, dtype=torch.int32, device=dev)
    nseg = len(cu) - 1
    out = torch.full((op.TP, 2 * op.H * 64), float("nan"), dtype=torch.float16, device=dev)
    if entry == "unsplit":
        ws = fresh_ws(dev, lib.rap_attention_workspace_bytes(op.TP, nseg))
        rc = lib.rap_x2_attention(_lib.ptr(op.qk), _lib.ptr(op.vt), op.nblk, _lib.ptr(cu_d), nseg, _lib.ptr(out), op.TP, op.H, _lib.ptr(ws), ws.numel(),
                                  stream(dev))
    else:
        need = lib.rap_attention_split_workspace_bytes(op.TP, nseg, op.H, splits)
        assert need > 0
        ws = fresh_ws(dev, need)
        rc = lib.rap_x2_attention_split(_lib.ptr(op.qk), _lib.ptr(op.vt), op.nblk, _lib.ptr(cu_d), nseg, _lib.ptr(out), op.TP, n_tokens, op.H, splits,
                                        _lib.ptr(ws), need, stream(dev))
    _lib.check(rc, "rap_x2_attention" + ("" if entry == "unsplit" else "_split"))
    torch.cuda.synchronize()
    return out.cpu()


def x2_values(raw, heads):
    return TX.unpack_ref(raw, heads * 64)


# ---------------------------------------------------------------------------------------------
# a. the sweep through the unsplit kernels
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", A.STARTS)
def test_sweep_fp32_online_and_bounded(lib, dev, start):
    q, k, v = A.sweep_operands(start)
    cu = torch.tensor(A.sweep_table(start))
    bound = TH.logit_bound(q, k)
    assert float(bound.max()) <= 40.0
    for name, b in (("online", None), ("bounded", bound)):
        out = TK.run_attention(lib, dev, qkv_thd(q, k, v), cu, bound=b).reshape(-1, A.H * 64)
        err = err_vs(out, sweep_ref(start))
        report("sweep fp32 " + name, f"start {start}", err, TK.ATTN_BOUND)
        assert err < TK.ATTN_BOUND, (start, name, err)


@pytest.mark.parametrize("start", A.STARTS)
def test_sweep_x2_one_and_two_blocks_per_cu(lib, dev, start):
    q, k, v = A.sweep_operands(start)
    cu = torch.tensor(A.sweep_table(start))
    try:
        for wpe in (2, 4):
            assert lib.rap_set_tuning(16, wpe) == 0
            err = err_vs(TX.run_x2_attention(lib, dev, q, k, v, cu), sweep_ref(start))
            report(f"sweep x2 key16={wpe}", f"start {start}", err, TX.X2_ATTN_BOUND)
            assert err < TX.X2_ATTN_BOUND, (start, wpe, err)
    finally:
        assert lib.rap_set_tuning(16, 2) == 0


@pytest.mark.parametrize("dt", [1, 2], ids=["bf16", "f16"])
@pytest.mark.parametrize("start", A.STARTS)
def test_sweep_h16_every_item_size_and_key_group_form(lib, dev, start, dt):
    q, k, v = A.sweep_operands(start)
    cu = torch.tensor(A.sweep_table(start))
    ref = sweep_ref(start, dt)                  # on the operands rounded to dt
    bound = TH.logit_bound(q, k)
    tol = TH.ATTN_ULPS * TH.ULP[dt]
    try:
        for key20 in H16_KEY20:
            assert lib.rap_set_tuning(20, key20) == 0
            for name, b in (("online", None), ("bounded", bound)):
                out = TH.run_attention_h(lib, dev, dt, q, k, v, cu, bound=b)
                err = err_vs(out.float(), ref)
                report(f"sweep {DT_NAME[dt]} key20={key20} {name}", f"start {start}", err, tol)
                assert err < tol, (start, dt, key20, name, err)
    finally:
        assert lib.rap_set_tuning(20, 1) == 0


# ---------------------------------------------------------------------------------------------
# b. the sweep through the split forms
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", A.STARTS)
def test_sweep_fp32_split(lib, dev, start):
    q, k, v = A.sweep_operands(start)
    cu = A.sweep_table(start)
    bound = TH.logit_bound(q, k)
    assert float(bound.max()) <= 40.0
    for splits in (2, 4):
        out = run_f32_split(lib, dev, q, k, v, cu, bound, splits)
        err = err_vs(out, sweep_ref(start))
        report(f"sweep fp32 split {splits}", f"start {start}", err, TK.ATTN_BOUND)
        assert err < TK.ATTN_BOUND, (start, splits, err)
        again = run_f32_split(lib, dev, q, k, v, cu, bound, splits)
        assert torch.equal(raw_bits(out), raw_bits(again)), (start, splits)                 # fixed merge order
    for b in (bound, None):                                                                     # one range: the unsplit entry point, bit for bit
        one = run_f32_split(lib, dev, q, k, v, cu, b, 1)
        old = run_f32_split(lib, dev, q, k, v, cu, b, 1, entry="unsplit")
        assert not torch.isnan(one).any() and torch.equal(raw_bits(one), raw_bits(old)), (start, b is not None)


def test_sweep_fp32_split_plain_launch_above_384_blocks(lib, dev):
    """With two heads every table stays in the one-block-per-CU launch form of launch_attention_f32; four heads and four key ranges do not."""
    start, Hh = A.WIDE_START, A.WIDE_HEADS
    cu = A.sweep_table(start)
    assert A.f32_split_blocks(cu[-1], len(cu) - 1, Hh, 4) > 384
    q, k, v = A.operands(cu[-1], 300, heads=Hh)
    bound = TH.logit_bound(q, k)
    ref = TX.attention_ref64(q, k, v, torch.tensor(cu))
    out = run_f32_split(lib, dev, q, k, v, cu, bound, 4)
    err = err_vs(out, ref)
    report("sweep fp32 split 4, H=4", f"start {start}", err, TK.ATTN_BOUND)
    assert err < TK.ATTN_BOUND, err


@pytest.mark.parametrize("start", A.STARTS)
def test_sweep_x2_split(lib, dev, start):
    q, k, v = A.sweep_operands(start)
    cu = A.sweep_table(start)
    op = X2Operands(dev, q, k, v)
    for splits in (2, 4):
        raw = run_x2_split(lib, dev, op, cu, splits)
        err = err_vs(x2_values(raw, A.H), sweep_ref(start))
        report(f"sweep x2 split {splits}", f"start {start}", err, TX.X2_ATTN_BOUND)
        assert err < TX.X2_ATTN_BOUND, (start, splits, err)
        assert torch.equal(raw_bits(raw), raw_bits(run_x2_split(lib, dev, op, cu, splits))), (start, splits)
    one = run_x2_split(lib, dev, op, cu, 1)
    assert not torch.isnan(one.float()).any() and torch.equal(raw_bits(one), raw_bits(run_x2_split(lib, dev, op, cu, 1, entry="unsplit"))), start


# ---------------------------------------------------------------------------------------------
# c. a sharp softmax across key ranges
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", list(A.SHARP_TABLES))
def test_sharp_softmax_x2_split(lib, dev, table):
    cu = A.SHARP_TABLES[table]
    L = cu[-1] - cu[-2]
    for spike in A.sharp_spikes(L):
        q, k, v, row5, at = A.sharp_case_x2(cu, spike, 9)
        ref = TX.attention_ref64(q, k, v, torch.tensor(cu))
        op = X2Operands(dev, q, k, v)
        for splits in (2, 4):
            out = x2_values(run_x2_split(lib, dev, op, cu, splits), A.H)
            err = err_vs(out, ref)
            one_hot = float((out[row5].reshape(A.H, 64) - v[:, at].double()).abs().max())
            report(f"sharp x2 split {splits}", f"{table} spike {spike}", err, 5e-6)
            assert err < 5e-6, (table, spike, splits, err)
            assert one_hot < 5e-6, (table, spike, splits, one_hot)                              # one-hot attention: row 5 is v of that key


@pytest.mark.parametrize("table", list(A.SHARP_TABLES))
def test_partial_maxima_further_apart_than_the_fp32_exponent_range_x2_split(lib, dev, table):
    """The sharp case above leaves exp2(m_y - m) finite whichever range's maximum m is (2^46 at most): it does not tell the maximum
    from any other reference.  Here the ranges' maxima are 93 apart (attention_cases.far_apart_case_x2): only the largest one works."""
    cu = A.SHARP_TABLES[table]
    L = cu[-1] - cu[-2]
    for spike in (0, L // 2, L - 1):
        q, k, v, at = A.far_apart_case_x2(cu, spike, 9)
        ref = TX.attention_ref64(q, k, v, torch.tensor(cu))
        op = X2Operands(dev, q, k, v)
        for splits in (2, 4):
            out = x2_values(run_x2_split(lib, dev, op, cu, splits), A.H)
            err = err_vs(out, ref)
            one_hot = float((out[cu[-2]:].reshape(L, A.H, 64) - v[:, at].double()).abs().max())
            report(f"far-apart maxima x2 split {splits}", f"{table} spike {spike}", err, TX.X2_ATTN_BOUND)
            assert err < TX.X2_ATTN_BOUND, (table, spike, splits, err)
            assert one_hot < TX.X2_ATTN_BOUND, (table, spike, splits, one_hot)                  # every row of the segment is v of that key


def fp32_case_tolerance(q, k, v, cu, ref):
    yard = float((A.attention_f32_plain(q, k, v, cu).double() - ref).abs().max())
    return yard, max(TK.ATTN_BOUND, A.FP32_SHARP_FACTOR * yard)


@pytest.mark.parametrize("table", list(A.SHARP_TABLES))
def test_sharp_softmax_fp32_split(lib, dev, table):
    cu = A.SHARP_TABLES[table]
    L = cu[-1] - cu[-2]
    for spike in A.sharp_spikes(L):
        q, k, v, row5, at = A.sharp_case_f32(cu, spike, 9)
        bound = TH.logit_bound(q, k)
        assert float(bound.max()) <= 40.0
        ref = TX.attention_ref64(q, k, v, torch.tensor(cu))
        yard, tol = fp32_case_tolerance(q, k, v, cu, ref)
        for splits in (2, 4):
            out = run_f32_split(lib, dev, q, k, v, cu, bound, splits)
            err = err_vs(out, ref)
            one_hot = float((out[row5].reshape(A.H, 64).double() - v[:, at].double()).abs().max())
            report(f"sharp fp32 split {splits}", f"{table} spike {spike} yardstick {yard:.2e}", err, tol)
            assert err < tol, (table, spike, splits, err, yard)
            assert one_hot < tol, (table, spike, splits, one_hot)


@pytest.mark.parametrize("table", list(A.SHARP_TABLES))
def test_all_logits_near_minus_the_bound_fp32_split(lib, dev, table):
    cu = A.SHARP_TABLES[table]
    q, k, v = A.near_bound_case(cu, 9)
    lo, hi = A.logits_range(q, k, cu)
    assert -39.0 <= lo and hi <= -30.0
    bound = torch.full((A.H,), A.NEAR_BOUND)
    ref = TX.attention_ref64(q, k, v, torch.tensor(cu))
    yard, tol = fp32_case_tolerance(q, k, v, cu, ref)
    for splits in (2, 4):
        out = run_f32_split(lib, dev, q, k, v, cu, bound, splits)
        err = err_vs(out, ref)
        report(f"near -bound fp32 split {splits}", f"{table} yardstick {yard:.2e}", err, tol)
        assert err < tol, (table, splits, err, yard)


# ---------------------------------------------------------------------------------------------
# d. rows outside the table, and n_tokens
# ---------------------------------------------------------------------------------------------
OUTSIDE_CU = [5, 100, 100, 170]


@pytest.mark.parametrize("splits", [2, 4])
def test_rows_outside_the_table_are_zero_in_the_fp32_split_form(lib, dev, splits):
    TP = 200
    q, k, v = A.operands(TP, 41)
    ref = TX.attention_ref64(q, k, v, torch.tensor(OUTSIDE_CU))
    out = run_f32_split(lib, dev, q, k, v, OUTSIDE_CU, TH.logit_bound(q, k), splits)
    assert (raw_bits(out[:5]) == 0).all() and (raw_bits(out[170:]) == 0).all()                # exactly +0, not NaN, not stale workspace
    err = err_vs(out[5:170], ref[5:170])
    report(f"outside rows fp32 split {splits}", "cu 5,100,100,170 of 200", err, TK.ATTN_BOUND)
    assert err < TK.ATTN_BOUND, err


@pytest.mark.parametrize("splits", [2, 4])
def test_rows_outside_the_table_and_beyond_n_tokens_in_the_x2_split_form(lib, dev, splits):
    for TP, n_tokens in ((200, 0), (256, 170)):
        q, k, v = A.operands(TP, 43)
        ref = TX.attention_ref64(q, k, v, torch.tensor(OUTSIDE_CU))
        raw = run_x2_split(lib, dev, X2Operands(dev, q, k, v), OUTSIDE_CU, splits, n_tokens=n_tokens)
        last = n_tokens if n_tokens else TP
        assert (raw_bits(raw[:5]) == 0).all() and (raw_bits(raw[170:last]) == 0).all()
        prefill = torch.full((TP - last, raw.shape[1]), float("nan"), dtype=torch.float16)
        assert torch.equal(raw_bits(raw[last:]), raw_bits(prefill))                           # rows from n_tokens on: not written
        err = err_vs(x2_values(raw[5:170], A.H), ref[5:170])
        report(f"outside rows x2 split {splits}", f"TP {TP} n_tokens {n_tokens}", err, TX.X2_ATTN_BOUND)
        assert err < TX.X2_ATTN_BOUND, err


# ---------------------------------------------------------------------------------------------
# e. the refusal contract
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splits", [2, 4])
def test_split_attention_bound_above_40_is_refused_loudly(lib, dev, splits):
    """test_attention_bound_above_40_is_refused_loudly's inputs through the split form: the main kernel writes a NaN row sum for the
    refused head, and the combine pass has to let it through (it used to turn it into zeros)."""
    g = torch.Generator().manual_seed(4)
    qkv = torch.randn(300, 3, 2, 64, generator=g)
    q, k, v = (qkv[:, i].permute(1, 0, 2).contiguous() for i in range(3))
    ref = TX.attention_ref64(q, k, v, torch.tensor([0, 300]))
    out = run_f32_split(lib, dev, q, k, v, [0, 300], torch.tensor([39.0, 41.0]), splits)
    assert float((out[:, :64].double() - ref[:, :64]).abs().max()) < 5e-6
    assert torch.isnan(out[:, 64:]).all()
