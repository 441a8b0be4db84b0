"""What the host and the GPU tests of softcap / final_mlp_act share (tests/test_softcap_host.py, tests/test_softcap_gpu.py): the float64
oracle of soft-capped attention, its plain-fp32 yardstick, and the fixtures scripts/make_softcap_golden.py wrote from the unmodified
reference.  Pure Python / torch on the CPU: nothing here touches a GPU.

softcap, as flash-attn documents it: s = (q . k) * softmax_scale;  softcap > 0: s <- softcap * tanh(s / softcap);  then the softmax."""
import os

import numpy as np
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# fixture -> the PointCloudDiT keyword arguments it was generated with (final_mlp_act by the name the fixture stores)
FIXTURES = {
    "l2_softcap1_rigid": dict(qk_norm=True, softcap=1.0, final_mlp_act="SiLU"),
    "l2_softcap01_noqknorm_rigid": dict(qk_norm=False, softcap=0.1, final_mlp_act="SiLU"),
    "l2_gelu_rigid": dict(qk_norm=True, softcap=0.0, final_mlp_act="GELU"),
    "l2_softcap1_relu_rigid": dict(qk_norm=True, softcap=1.0, final_mlp_act="ReLU"),
}
ACT_CODE = {"SiLU": 0, "GELU": 1, "ReLU": 2}          # rap_model_set_final_act
# A fixture must not pass when its switch is ignored: the switched velocity differs from the plain model's (softcap = 0, SiLU; stored
# next to it) by at least this multiple of the fp32 assert on the velocity, 1e-4 max|v|.
SENSITIVITY = 50.0


def act_class(name):
    return getattr(torch.nn, name)


def load_fixture(name):
    """-> (the arrays, the inputs as tensors)"""
    g = dict(np.load(os.path.join(GOLDEN_DIR, name + ".npz")))
    return g, {k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("in_")}


def segments(cu):
    cu = [int(c) for c in cu]
    return [(a, b - a) for a, b in zip(cu[:-1], cu[1:])]


def _attention(q, k, v, cu, softcap, dtype):
    heads, TP, _ = q.shape
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    out = torch.zeros(TP, heads * 64, dtype=dtype)
    for a, n in segments(cu):
        if n:
            s = q[:, a:a + n] @ k[:, a:a + n].transpose(1, 2) / 8.0
            if softcap > 0:
                s = softcap * torch.tanh(s / softcap)
            out[a:a + n] = (torch.softmax(s, dim=-1) @ v[:, a:a + n]).permute(1, 0, 2).reshape(n, heads * 64)
    return out


def attention_ref64(q, k, v, cu, softcap):
    """q, k, v (H, TP, 64) -> (TP, H * 64) float64: soft-capped softmax attention inside every segment of cu (softcap = 0: plain)"""
    return _attention(q, k, v, cu, softcap, torch.float64)


def attention_f32_plain(q, k, v, cu, softcap):
    """the yardstick of the fp32 bounds (attention_cases.py:18-26): the same capped attention in plain float32 on the CPU"""
    return _attention(q, k, v, cu, softcap, torch.float32)
