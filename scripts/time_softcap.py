"""Time the soft-capped attention kernels against the uncapped online-softmax kernel of the same family, launch by launch, at the
attention geometry of BASELINE configs[1]: 32 samples x 2 parts x 4096 points = 262 144 tokens, 8 heads -- the per-part launch (64
segments of 4096 keys) and the per-sample launch (32 segments of 8192 keys).

Families: fp32 (rap_attention_f32 without a logit bound / rap_attention_f32_softcap), x2 (rap_x2_attention / rap_x2_attention_softcap),
bf16 and f16 (rap_attention_h16 without a bound / rap_attention_h16_softcap).  The operands are random planes in each kernel's own
layout (the time does not depend on the values; the cap's instruction count does not depend on the cap).

Per launch: GPU time (HIP events around the call) after --warmup calls, the median and the 10th / 90th percentile over --calls, and the
ratio of the two medians.  Prints one JSON line per (family, branch); --out FILE also writes them.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

SAMPLES, PARTS, POINTS, HEADS = 32, 2, 4096, 8
BRANCHES = {"per_part": POINTS, "per_sample": PARTS * POINTS}      # branch -> segment length
FAMILIES = ["fp32", "x2", "bf16", "f16"]


def time_calls(torch, call, warmup, calls):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    gpu = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        gpu.append(e0.elapsed_time(e1))
    return gpu


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--family", choices=FAMILIES + ["all"], default="all")
    ap.add_argument("--softcap", type=float, default=30.0)
    ap.add_argument("--calls", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from rap_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    st = lambda: _lib.current_stream(dev)
    TP, H = SAMPLES * PARTS * POINTS, HEADS
    nblk = TP // 64
    g = torch.Generator(device=dev).manual_seed(7)
    rnd = lambda shape, dtype: (torch.randn(shape, generator=g, device=dev) * 0.5).to(dtype)
    pct = lambda v, p: sorted(v)[min(len(v) - 1, int(round(p * (len(v) - 1))))]
    lines = []
    for fam in (FAMILIES if a.family == "all" else [a.family]):
        if fam == "fp32":
            qkv = rnd((3, H, TP, 64), torch.float32)
            out = torch.empty((TP, H * 64), device=dev)
        elif fam == "x2":
            qk, vt = rnd((2, H, 2, TP, 64), torch.float16), rnd((H, nblk, 2, 64, 64), torch.float16)
            out = torch.empty((TP, 2 * H * 64), dtype=torch.float16, device=dev)
        else:
            dt = 1 if fam == "bf16" else 2
            tdt = torch.bfloat16 if dt == 1 else torch.float16
            qk, vt = rnd((2, H, TP, 64), tdt), rnd((H, nblk, 64, 64), tdt)
            out = torch.empty((TP, H * 64), dtype=tdt, device=dev)
        for branch, seg in BRANCHES.items():
            nseg = TP // seg
            cu = torch.arange(0, TP + 1, seg, dtype=torch.int32, device=dev)
            ws = torch.empty(lib.rap_attention_workspace_bytes(TP, nseg), dtype=torch.uint8, device=dev)
            P = _lib.ptr
            if fam == "fp32":
                plain = lambda: lib.rap_attention_f32(P(qkv), P(cu), nseg, P(out), TP, H, None, P(ws), ws.numel(), st())
                capped = lambda: lib.rap_attention_f32_softcap(P(qkv), P(cu), nseg, P(out), TP, H, a.softcap, P(ws), ws.numel(), st())
            elif fam == "x2":
                plain = lambda: lib.rap_x2_attention(P(qk), P(vt), nblk, P(cu), nseg, P(out), TP, H, P(ws), ws.numel(), st())
                capped = lambda: lib.rap_x2_attention_softcap(P(qk), P(vt), nblk, P(cu), nseg, P(out), TP, H, a.softcap, P(ws), ws.numel(), st())
            else:
                plain = lambda: lib.rap_attention_h16(dt, P(qk), P(vt), nblk, P(cu), nseg, P(out), TP, H, None, P(ws), ws.numel(), st())
                capped = lambda: lib.rap_attention_h16_softcap(dt, P(qk), P(vt), nblk, P(cu), nseg, P(out), TP, H, a.softcap, P(ws), ws.numel(), st())
            res = {}
            for name, call in (("uncapped_online", plain), ("softcap", capped)):
                assert call() == 0, (fam, branch, name)
                gpu = time_calls(torch, call, a.warmup, a.calls)
                res[name] = {"median": statistics.median(gpu), "p10": pct(gpu, 0.1), "p90": pct(gpu, 0.9)}
            assert bool(torch.isfinite(out.float()).all())
            lines.append(json.dumps({"family": fam, "branch": branch, "tokens": TP, "heads": H, "segments": nseg, "segment_length": seg,
                                     "softcap": a.softcap, "calls": a.calls, "warmup": a.warmup, "gpu_ms": res,
                                     "ratio": res["softcap"]["median"] / res["uncapped_online"]["median"]}))
            print(lines[-1], flush=True)
        del out
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
