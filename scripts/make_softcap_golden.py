#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY -- the fixtures of tests/test_softcap_*.py: the UNMODIFIED reference PointCloudDiT built with softcap > 0 and /
or another final_mlp_act, run on the CPU through oracle.ref_loader.load_reference().

    python scripts/make_softcap_golden.py [--case=NAME ...]        (needs the reference checkout, RAP_REFERENCE_ROOT; no GPU)

oracle/ is not changed: its flash-attn stand-in asserts softcap == 0, and ref_loader installs it only when sys.modules has no
`flash_attn` -- so this script installs its own first: the same signature, every segment evaluated in float64, the cap applied as
flash-attn documents it (s = q.k * softmax_scale; softcap > 0: s <- softcap * tanh(s / softcap); then the softmax).
ref_loader.build_reference_dit does not forward the two constructor arguments either, so it is wrapped here for the duration of a case.

Layout and keys follow oracle/make_golden.py:main (RAP_12, L = 2, rap_amd.synthetic weights and inputs) plus softcap, qk_norm,
final_mlp_act (the class name) and fwd_velocity_plain: the same forward with softcap = 0 and SiLU.  Every fixture must tell an ignored
switch from an honoured one: max|fwd_velocity - fwd_velocity_plain| >= 50 x the fp32 assert on the velocity (1e-4 max|v|), checked here
and again by tests/test_softcap_host.py from the stored arrays.  The transformer features are not stored (the plain fixtures of the same
geometry carry them): each file stays far below 1 MiB.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def flash_attn_varlen_qkvpacked_func(qkv, cu_seqlens, max_seqlen, dropout_p=0.0, softmax_scale=None, causal=False, window_size=(-1, -1),
                                     softcap=0.0, alibi_slopes=None, deterministic=False, return_attn_probs=False):
    """qkv (T, 3, H, D), cu_seqlens (S + 1,) -> (T, H, D): dense softmax attention inside every segment, in float64"""
    assert dropout_p == 0.0 and not causal and tuple(window_size) == (-1, -1) and alibi_slopes is None and not return_attn_probs
    T, three, H, D = qkv.shape
    assert three == 3
    scale = softmax_scale if softmax_scale is not None else D ** -0.5
    out = torch.zeros((T, H, D), dtype=torch.float64)
    cu = cu_seqlens.tolist()
    for a, b in zip(cu[:-1], cu[1:]):
        if b == a:
            continue
        q, k, v = (qkv[a:b, i].transpose(0, 1).double() for i in range(3))
        s = (q @ k.transpose(1, 2)) * scale
        if softcap > 0:
            s = softcap * torch.tanh(s / softcap)
        out[a:b] = (torch.softmax(s, dim=-1) @ v).transpose(0, 1)
    return out.to(qkv.dtype)


_fa = types.ModuleType("flash_attn")
_fa.flash_attn_varlen_qkvpacked_func = flash_attn_varlen_qkvpacked_func
sys.modules["flash_attn"] = _fa          # before ref_loader looks: _install_stubs keeps a module that is already there

from oracle import ref_loader                      # noqa: E402
from oracle import rap_oracle as O                 # noqa: E402
from rap_amd import synthetic as S                 # noqa: E402

GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
PARTS, INPUT_SEED, WEIGHT_SEED, STEPS, RIGID, LAYERS = [[60, 41], [130, 20, 77]], 51, 4, 3, True, 2
# name -> qk_norm, softcap, final_mlp_act.  The caps: softcap = 30 moves the velocity by 1.4e-5, less than its fp32 assert -- such a
# fixture passes with the switch ignored; 1.0 with qk-norm (logits up to 8) and 0.1 without (logits << 1) bend them hard.
CASES = {
    "l2_softcap1_rigid": (True, 1.0, "SiLU"),
    "l2_softcap01_noqknorm_rigid": (False, 0.1, "SiLU"),
    "l2_gelu_rigid": (True, 0.0, "GELU"),
    "l2_softcap1_relu_rigid": (True, 1.0, "ReLU"),
}
SENSITIVITY = 50.0


def reference_dit(cfg, sd, softcap, act):
    ns = ref_loader.load_reference()
    m = ns.PointCloudDiT(in_dim=0, out_dim=3, embed_dim=cfg["embed_dim"], num_layers=cfg["num_layers"], num_heads=cfg["num_heads"],
                         attn_dtype="float32", qk_norm=cfg.get("qk_norm", True), local_feat_dim=cfg["local_feat_dim"],
                         softcap=softcap, final_mlp_act=getattr(torch.nn, act))
    m.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    return m.eval()


def forward(model, inp, ts):
    cu_b, cu_p = O.prepare_cu_seqlens(inp)
    with torch.inference_mode():
        return model(x=inp["x_1"], timesteps=ts, cond_coord=inp["pointclouds"], local_features=inp["features"], latent_features=None,
                     scales=inp["scales"], anchor_indices=inp["anchor_indices"], cu_seqlens_batch=cu_b, cu_seqlens_part=cu_p)


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    only = [a.split("=", 1)[1] for a in sys.argv if a.startswith("--case=")]
    for name, (qk_norm, softcap, act) in CASES.items():
        if only and name not in only:
            continue
        cfg = dict(S.RAP_12); cfg["num_layers"] = LAYERS; cfg["qk_norm"] = qk_norm
        sd = S.make_weights(cfg, WEIGHT_SEED)
        inp = S.make_inputs(PARTS, seed=INPUT_SEED, feat_dim=cfg["local_feat_dim"])
        ts = torch.linspace(0.15, 0.9, len(PARTS))
        v = forward(reference_dit(cfg, sd, softcap, act), inp, ts)
        v_plain = forward(reference_dit(cfg, sd, 0.0, "SiLU"), inp, ts)
        moved, tol = float((v - v_plain).abs().max()), 1e-4 * float(v.abs().max())
        print(f"{name}: max|v| {float(v.abs().max()):.3f}  the switch moves the velocity by {moved:.2e} = {moved / tol:.0f} x its fp32 assert")
        assert moved >= SENSITIVITY * tol, (name, moved, tol)
        build = ref_loader.build_reference_dit
        ref_loader.build_reference_dit = lambda c, s, dtype=torch.float32: reference_dit(c, s, softcap, act)      # reference_sample builds through it
        try:
            ref = ref_loader.reference_sample(cfg, sd, inp, STEPS, RIGID)
        finally:
            ref_loader.build_reference_dit = build
        out = {
            "num_layers": np.int64(LAYERS), "weight_seed": np.int64(WEIGHT_SEED), "num_steps": np.int64(STEPS), "rigidity": np.int64(int(RIGID)),
            "weights_checksum": np.float64(sum(t.double().sum().item() for t in sd.values())),
            "softcap": np.float64(softcap), "qk_norm": np.int64(int(qk_norm)), "final_mlp_act": np.str_(act),
            "fwd_timesteps": ts.numpy(), "fwd_velocity": v.numpy(), "fwd_velocity_plain": v_plain.numpy(),
            "end_point_trajectory": ref["end_point_trajectory"].numpy(), "trajectory": ref["trajectory"].numpy(),
            "R": ref["R"].numpy(), "t": ref["t"].numpy(),
        }
        for k, t in inp.items():
            out["in_" + k] = t.numpy()
        path = os.path.join(GOLDEN_DIR, name + ".npz")
        np.savez_compressed(path, **out)
        print(name, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
