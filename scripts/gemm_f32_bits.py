"""The bits the fp32 GEMM kernels write, as one SHA-256 per output buffer: run it on two builds of the library and compare the two files
(on the CPU) to show that a change of gemm_f32.hip computes exactly what its parent computed.

A fixed, seeded list of rap_gemm_f32 / rap_gemm_f32_splitk calls -- the smallest shapes at which each form can go wrong (the f32 tables of
tests/gemm_cases.py) and what those lack: epilogue 8, the stagger prologue, the persistent kernel under every epilogue.  Operands are seeded
normal values, outputs start as NaN (an element the kernel never wrote is hashed too), and every call first asks rap_gemm_f32_form
whether the shape still reaches the form it is listed under.

  128 x 128      epilogues 0-6 and 8, M in {1, 129, 300}, N in {128, 384} (QKV: N = 384, H = 2), K in {32, 96} (32: one k-tile, the loop
                 body is skipped); one call of 1024 tiles (M = 131072, N = 128, K = 32: the stagger prologue)
  split-K        rap_gemm_f32_splitk with exactly the reported workspace: epilogue 1 at K = 512 and K = 1056 (33 k-tiles over 4 blocks),
                 epilogue 2 with 2 and 4 planes at K = 512
  256 x 256      M in {16129, 16383}, N = 2048, K in {256, 288}, epilogues 0-6 and 8; QKV at M = 10753, N = 3072, H = 16
  persistent     M in {16384, 16640} (520 tiles: an uneven walk), N = 2048, K = 256, and the same calls with tuning key 12 = 0
  rap_sample     the smallest fp32 fixture of tests/golden (l2_gelu_rigid: qk-norm fused into the QKV GEMM -- the kernel-level entry point
                 takes no gains -- and a GELU head), final cloud hashed

One process, no retries.  Writes {call name: sha256} as JSON to --out and prints the number of calls.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F128, F256, F256P = 121, 201, 301
EPILOGUES = [0, 1, 2, 3, 4, 5, 6, 8]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch
    import rap_amd
    import plan_cases as PC
    import softcap_cases as SC
    from rap_amd import _lib, synthetic as S
    lib = _lib.load()
    dev = torch.device("cuda:0")
    P, st = _lib.ptr, lambda: _lib.current_stream(dev)
    hashes = {}

    def record(name, t):
        torch.cuda.synchronize()
        assert name not in hashes, name
        hashes[name] = hashlib.sha256(t.cpu().contiguous().numpy().tobytes()).hexdigest()

    nan = lambda *shape: torch.full(shape, float("nan"), device=dev)
    ops = {}

    def operands(N, K, rows):
        """one seeded set per (N, K), made at the largest row count asked for first and sliced by rows"""
        if (N, K) not in ops:
            ops.clear()                                             # the big sets hold a few hundred MB
            g = torch.Generator().manual_seed(1000 + N + 7 * K)
            r = lambda *s: torch.randn(*s, generator=g).to(dev)
            o = dict(A=r(rows, K), W=r(N, K) / K ** 0.5, b=r(N), h=r(rows, N), emb=r(2, N),
                     anchor=(torch.rand(rows, generator=g) < 0.4).to(torch.uint8).to(dev))
            o["Wi"], o["bi"] = torch.empty_like(o["W"]), torch.empty_like(o["b"])
            _lib.check(lib.rap_geglu_interleave(P(o["W"]), P(o["b"]), P(o["Wi"]), P(o["bi"]), N // 2, K, st()), "rap_geglu_interleave")
            ops[(N, K)] = o
        assert ops[(N, K)]["A"].shape[0] >= rows
        return ops[(N, K)]

    def gemm(tag, form, epi, M, N, K, rows, H=0):
        o = operands(N, K, rows)
        W, b, ldc, resid, anchor, emb = o["W"], o["b"], N, None, None, None
        if epi == 3:
            C, W, b, ldc = nan(M, N // 2), o["Wi"], o["bi"], N // 2
        elif epi == 4:
            C, b = nan(3, H, M, 64), None
        else:
            C = nan(M, N)
        if epi == 1:
            resid = o["h"][:M]
        if epi == 5:
            anchor, emb = o["anchor"][:M], o["emb"]
        got = lib.rap_gemm_f32_form(epi, M, N, K, K, K, ldc, N if epi == 1 else 0, 0, 0)
        assert got == form, (tag, epi, M, N, K, got, form)
        _lib.check(lib.rap_gemm_f32(epi, P(o["A"]), K, P(W), K, P(C), ldc, M, N, K, P(b), P(resid), N if epi == 1 else 0, P(anchor), P(emb), H,
                                    st()), "rap_gemm_f32")
        record(f"{tag} epi{epi} M{M} N{N} K{K}", C)

    def splitk(epi, M, N, K, planes, form, rows):
        o = operands(N, K, rows)
        need = lib.rap_gemm_f32_splitk_workspace_bytes(epi, M, N, K, planes)
        assert need > 0, (epi, M, N, K, planes)
        got = lib.rap_gemm_f32_form(epi, M, N, K, K, K, N, N if epi == 1 else 0, 1, planes)
        assert got == form, (epi, M, N, K, planes, got, form)
        ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)
        C, resid = nan(M, N), (o["h"][:M] if epi == 1 else None)
        _lib.check(lib.rap_gemm_f32_splitk(epi, P(o["A"]), K, P(o["W"]), K, P(C), N, M, N, K, P(o["b"]), P(resid), N if epi == 1 else 0, planes,
                                           P(ws), need, st()), "rap_gemm_f32_splitk")
        record(f"splitk epi{epi} planes{planes} M{M} N{N} K{K}", C)

    # ---- 128 x 128
    for N in (128, 384):
        for K in (32, 96):
            for epi in EPILOGUES:
                if epi == 4 and N != 384:
                    continue
                for M in (1, 129, 300):
                    gemm("128", F128, epi, M, N, K, 300, H=2)
    gemm("128 stagger", F128, 0, 131072, 128, 32, 131072)
    # ---- split-K
    for K in (512, 1056):
        for M in (100, 2048):
            splitk(1, M, 512, K, 0, F128 + 3, 2048)
    for N in (128, 384):
        for planes in (2, 4):
            for M in (129, 256):
                splitk(2, M, N, 512, planes, F128 - 1 + planes, 256)
    # ---- 256 x 256, one tile per block, and the persistent walk (key 12 = 0: the same shapes one tile per block)
    for K in (256, 288):
        for epi in EPILOGUES:
            if epi != 4:
                for M in (16129, 16383):
                    gemm("256", F256, epi, M, 2048, K, 16640)
        if K == 256:
            for epi in EPILOGUES:
                if epi != 4:
                    for M in (16384, 16640):
                        gemm("persistent", F256P, epi, M, 2048, K, 16640)
                        assert lib.rap_set_tuning(12, 0) == 0
                        try:
                            gemm("persistent key12=0", F256, epi, M, 2048, K, 16640)
                        finally:
                            assert lib.rap_set_tuning(12, 1) == 0
    gemm("256", F256, 4, 10753, 3072, 256, 11264, H=16)
    gemm("persistent", F256P, 4, 11264, 3072, 256, 11264, H=16)
    ops.clear()
    torch.cuda.empty_cache()

    # ---- one sampling call of the smallest fp32 fixture
    name = "l2_gelu_rigid"
    g, inp = SC.load_fixture(name)
    kw = SC.FIXTURES[name]
    cfg = dict(S.RAP_12); cfg["num_layers"] = int(g["num_layers"]); cfg["qk_norm"] = kw["qk_norm"]
    model = rap_amd.PointCloudDiT(in_dim=0, out_dim=3, embed_dim=512, num_layers=cfg["num_layers"], num_heads=8, local_feat_dim=32,
                                  attn_dtype="float32", compute_dtype="float32", qk_norm=kw["qk_norm"], softcap=kw["softcap"],
                                  final_mlp_act=SC.act_class(kw["final_mlp_act"]))
    model.load_state_dict(S.make_weights(cfg, int(g["weight_seed"])))
    model.to(dev)
    flow = rap_amd.RectifiedPointFlow(flow_model=model, inference_sampling_steps=int(g["num_steps"]), rigidity_forcing=bool(g["rigidity"]))
    # the fixture's QKV projection (with the gains) has to be a call of the 128 x 128 form: ask the plan the launch path runs by
    TP, B, nseg = inp["x_1"].shape[0], inp["points_per_part"].shape[0], inp["points_per_part"].numel()
    plan = PC.lib_plan(lib, "f32", TP, B, nseg, L=cfg["num_layers"], rows=int(g["num_steps"]))
    assert plan.f_qkv == F128 and kw["qk_norm"], plan
    d = {k: v.to(dev) for k, v in inp.items()}
    res = flow.sample_rectified_flow(d, None, x_1=d["x_1"])
    record(f"rap_sample {name} final cloud", res["end_point_trajectory"])

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(hashes, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(hashes)} output buffers hashed -> {a.out}")


if __name__ == "__main__":
    main()
