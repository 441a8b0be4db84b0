"""CPU: the constructor contract of softcap / final_mlp_act, the C ABI's argument checks for them, the fixtures' sensitivity to the
switches they carry, and the float64 softcap-attention oracle the GPU tests compare against (tests/softcap_cases.py)."""
import ctypes
import math

import pytest
import torch
import torch.nn as nn

import attention_cases as A
import rap_amd
import softcap_cases as SC
from rap_amd import _lib


def make(**kw):
    return rap_amd.PointCloudDiT(in_dim=0, out_dim=3, embed_dim=512, num_layers=2, num_heads=8, local_feat_dim=32, **kw)


# ---------------------------------------------------------------------------------------------
# constructor contract
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [0.0, 0, 1.0, 0.1, 30, 1e-3, 1e6])
def test_softcap_values_that_construct(cap):
    m = make(softcap=cap)
    assert m.softcap == float(cap)


@pytest.mark.parametrize("cap", [-1.0, -1e-9, float("nan"), float("inf"), float("-inf")])
def test_softcap_values_that_are_refused(cap):
    with pytest.raises(ValueError):
        make(softcap=cap)


def test_dropout_is_still_refused():
    with pytest.raises(NotImplementedError):
        make(dropout_rate=0.1)
    with pytest.raises(NotImplementedError):
        make(dropout_rate=0.1, softcap=1.0)


@pytest.mark.parametrize("act,code", [(None, 0), (nn.SiLU, 0), (nn.SiLU(), 0), (nn.GELU, 1), (nn.GELU(), 1), (nn.GELU(approximate="none"), 1),
                                      (nn.ReLU, 2), (nn.ReLU(), 2), (nn.ReLU(inplace=True), 2)],
                         ids=["None", "SiLU", "SiLU()", "GELU", "GELU()", "GELU(none)", "ReLU", "ReLU()", "ReLU(inplace)"])
def test_final_mlp_act_values_that_construct(act, code):
    m = make(final_mlp_act=act)
    assert m._final_act == code and m.final_mlp_act is act


@pytest.mark.parametrize("act", [nn.GELU(approximate="tanh"), nn.Tanh, nn.Tanh(), nn.LeakyReLU, nn.Mish(), "gelu", torch.nn.functional.gelu, 1, nn.Module],
                         ids=["GELU(tanh)", "Tanh", "Tanh()", "LeakyReLU", "Mish()", "str", "function", "int", "Module"])
def test_final_mlp_act_values_that_are_refused_never_ignored(act):
    with pytest.raises(NotImplementedError):
        make(final_mlp_act=act)


def test_both_switches_leave_the_state_dict_contract_alone():
    from rap_amd.synthetic import RAP_12, weight_spec
    cfg = dict(RAP_12); cfg["num_layers"] = 2
    m = make(softcap=1.0, final_mlp_act=nn.GELU)
    assert m._spec == weight_spec(cfg)


# ---------------------------------------------------------------------------------------------
# C ABI: a model handle needs a device, so what the host can hold the setters to is their NULL-handle contract and the
# argument checks of the kernel-level entry points (the setters on a live handle: tests/test_softcap_gpu.py)
# ---------------------------------------------------------------------------------------------
def test_setters_and_getters_refuse_a_null_handle():
    lib = _lib.load()
    N = ctypes.c_void_p(0)
    assert lib.rap_model_set_softcap(N, 1.0) == -1 and lib.rap_model_set_final_act(N, 1) == -1
    assert lib.rap_model_softcap(N) < 0 and lib.rap_model_final_act(N) < 0
    assert lib.rap_version() == 6          # the additions are additive


def test_softcap_entry_points_check_their_arguments_before_any_launch():
    lib = _lib.load()
    N, one = ctypes.c_void_p(0), ctypes.c_void_p(1)      # `one`: a non-NULL sentinel; every call below must fail on another argument first
    big = 1 << 20
    for cap in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.rap_attention_f32_softcap(one, one, 1, one, 256, 2, cap, one, big, N) == -1, cap
        assert lib.rap_attention_h16_softcap(1, one, one, 4, one, 1, one, 256, 2, cap, one, big, N) == -1, cap
        assert lib.rap_x2_attention_softcap(one, one, 4, one, 1, one, 256, 2, cap, one, big, N) == -1, cap
    assert lib.rap_attention_f32_softcap(N, one, 1, one, 256, 2, 5.0, one, big, N) == -1
    assert lib.rap_attention_h16_softcap(3, one, one, 4, one, 1, one, 256, 2, 5.0, one, big, N) == -1       # no such 16-bit dtype
    assert lib.rap_x2_attention_softcap(one, one, 3, one, 1, one, 256, 2, 5.0, one, big, N) == -1           # V^T image shorter than TP
    need = lib.rap_attention_workspace_bytes(256, 1)
    assert lib.rap_attention_f32_softcap(one, one, 1, one, 256, 2, 5.0, one, need - 1, N) == -2
    assert lib.rap_attention_h16_softcap(1, one, one, 4, one, 1, one, 256, 2, 5.0, one, need - 1, N) == -2
    assert lib.rap_x2_attention_softcap(one, one, 4, one, 1, one, 256, 2, 5.0, one, need - 1, N) == -2
    assert lib.rap_attention_f32_softcap(one, one, 1, one, 256, 2, 5.0, N, big, N) == -2                    # no workspace at all


def test_gelu_epilogue_has_a_form_and_the_internal_one_stays_refused():
    lib = _lib.load()
    assert lib.rap_gemm_f32_form(8, 300, 512, 512, 512, 512, 512, 0, 0, 0) == lib.rap_gemm_f32_form(6, 300, 512, 512, 512, 512, 512, 0, 0, 0) > 0
    assert lib.rap_gemm_f32_form(8, 300, 512, 512, 512, 512, 512, 0, 1, 4) == lib.rap_gemm_f32_form(8, 300, 512, 512, 512, 512, 512, 0, 0, 0)   # never split
    assert lib.rap_gemm_f32_form(7, 300, 512, 512, 512, 512, 512, 0, 0, 0) == -1 and lib.rap_gemm_f32_form(9, 300, 512, 512, 512, 512, 512, 0, 0, 0) == -1


# ---------------------------------------------------------------------------------------------
# fixtures
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SC.FIXTURES))
def test_fixture_tells_an_ignored_switch_from_an_honoured_one(name):
    g, inp = SC.load_fixture(name)
    kw = SC.FIXTURES[name]
    assert float(g["softcap"]) == kw["softcap"] and bool(g["qk_norm"]) == kw["qk_norm"] and str(g["final_mlp_act"]) == kw["final_mlp_act"]
    assert kw["softcap"] > 0 or kw["final_mlp_act"] != "SiLU"
    v, plain = torch.from_numpy(g["fwd_velocity"]), torch.from_numpy(g["fwd_velocity_plain"])
    assert v.shape == plain.shape == (inp["x_1"].shape[0], 3)
    moved, tol = float((v - plain).abs().max()), 1e-4 * float(v.abs().max())
    print(f"{name}: the switch moves the velocity by {moved:.2e} = {moved / tol:.0f} x the fp32 assert {tol:.2e}")
    assert moved >= SC.SENSITIVITY * tol, (moved, tol)
    assert int(inp["points_per_part"].sum()) == 328                                                       # [[60, 41], [130, 20, 77]]
    assert int(g["num_steps"]) == 3 and bool(g["rigidity"])


# ---------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------
def plain_ref64(q, k, v, cu):
    """attention_cases-style plain attention in float64 (tests/attention_cases.py: attention_f32_plain, in double)"""
    out = torch.zeros(q.shape[1], q.shape[0] * 64, dtype=torch.float64)
    for a, n in A.segments(cu):
        if n:
            p = torch.softmax(q[:, a:a + n].double() @ k[:, a:a + n].double().transpose(1, 2) / 8.0, dim=-1)
            out[a:a + n] = (p @ v[:, a:a + n].double()).permute(1, 0, 2).reshape(n, q.shape[0] * 64)
    return out


def test_oracle_is_plain_attention_as_the_cap_goes_to_infinity():
    cu = A.sweep_table(33)
    q, k, v = A.sweep_operands(33)
    err = float((SC.attention_ref64(q, k, v, cu, 1e9) - plain_ref64(q, k, v, cu)).abs().max())
    assert err < 1e-12, err
    assert torch.equal(SC.attention_ref64(q, k, v, cu, 0.0), plain_ref64(q, k, v, cu))                     # 0 = off
    bent = float((SC.attention_ref64(q, k, v, cu, 10.0) - plain_ref64(q, k, v, cu)).abs().max())
    assert bent > 1e-2, bent                                                                                # logits reach ~18: 10 bends them hard


def test_oracle_saturates_to_the_mean_of_v_over_the_argmax_tied_keys():
    """c = 1e-3 on logits of +-50: tanh(s / c) is +-1 exactly in float64, so every capped logit is +-c and the keys on the positive side
    are tied at the maximum.  (a) every key on the positive side: all tied, the result is the mean of v over them, i.e. over the segment;
    (b) keys on both sides: the tied keys weigh e^c, the others e^-c -- the cap leaves a 2e-3 preference, exactly; (c) the same logits
    under a cap of 20, large against 1 but small against the gap: the other keys weigh e^-39 and the tied ones carry the row."""
    g = torch.Generator().manual_seed(5)
    L, Hh = 96, 2
    u = torch.nn.functional.normalize(torch.randn(Hh, 1, 64, generator=g), dim=-1)
    q = (u * 20.0).expand(Hh, L, 64).contiguous()
    v = torch.randn(Hh, L, 64, generator=g)
    k_all = (u * 20.0).expand(Hh, L, 64).contiguous()                            # every logit +50: 400 / 8
    out = SC.attention_ref64(q, k_all, v, [0, L], 1e-3).reshape(L, Hh, 64)
    assert float((out - v.double().mean(dim=1)[None]).abs().max()) < 1e-12                                 # (a)
    tied = torch.zeros(L, dtype=torch.bool); tied[[3, 40, 41, 95]] = True
    k = torch.where(tied[None, :, None], u * 20.0, -u * 20.0)                    # logits +50 on the tied keys, -50 elsewhere
    out = SC.attention_ref64(q, k, v, [0, L], 1e-3).reshape(L, Hh, 64)
    w = torch.where(tied, torch.tensor(math.exp(1e-3), dtype=torch.float64), torch.tensor(math.exp(-1e-3), dtype=torch.float64))
    want = (w[None, :, None] * v.double()).sum(dim=1) / w.sum()
    assert float((out - want[None]).abs().max()) < 1e-12                                                    # (b)
    out = SC.attention_ref64(q, k, v, [0, L], 20.0).reshape(L, Hh, 64)
    assert float((out - v[:, tied].double().mean(dim=1)[None]).abs().max()) < 1e-12                         # (c)
