"""FP8 expert-weight kernels against their bf16 twins at the 30b shapes.

E = 128 experts, H = 2048, I = 768, random top-8 routing. Narrow decode
(moe_gemv_h / moe_gemv_down and their _fp8 twins) at B in --narrow (default
1, 5, 8) tokens; wide decode (moe_grouped_gemm_skinny and its _fp8 twin,
gate/up and down shapes) at M in --wide (default 16, 64) rows.

Method: --layers independent layers of weights (default 8, 9.7 GB bf16 + 4.8
GB fp8), each with its own routing, so that a call streams its experts from
HBM as a decode step does, not from the 256 MB last-level cache a single
layer's touched experts would fit in. One timed unit is a captured graph that
runs the kernel once per layer; the per-call time is the unit's device-event
time over the layer count. Every variant is warmed up, then the variants are
timed alternately for --reps rounds and the median is reported, with the
weight bytes the routing touches (unique experts x panel bytes) over that
time. Row order of the table: bf16 twin first, then fp8.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from room_amd import ops  # noqa: E402
from room_amd.ops.reference import quantize_fp8_block  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--narrow", default="1,5,8")
ap.add_argument("--wide", default="16,64")
ap.add_argument("--layers", type=int, default=8)
ap.add_argument("--reps", type=int, default=60)
ap.add_argument("--experts", type=int, default=128)
ap.add_argument("--hidden", type=int, default=2048)
ap.add_argument("--inter", type=int, default=768)
ap.add_argument("--out", default=None)
args = ap.parse_args()

assert torch.cuda.is_available(), "needs a GPU"
DEV = torch.device("cuda", 0)
BF = torch.bfloat16
E, H, I, TOPK, L = args.experts, args.hidden, args.inter, 8, args.layers
torch.manual_seed(5)

layers = []
for _ in range(L):
    w13 = torch.empty(E, 2 * I, H, dtype=BF, device=DEV).normal_(0, 0.02)
    w2 = torch.empty(E, H, I, dtype=BF, device=DEV).normal_(0, 0.02)
    w13_q, w13_s = quantize_fp8_block(w13)
    w2_q, w2_s = quantize_fp8_block(w2)
    layers.append(dict(w13=w13, w2=w2, w13_q=w13_q, w13_s=w13_s, w2_q=w2_q,
                       w2_s=w2_s))
torch.cuda.synchronize()


def routing(T):
    """Per layer: top-8 of random logits -> ids [T, 8] int32."""
    return [torch.randn(T, E, device=DEV).topk(TOPK, dim=-1).indices.int()
            for _ in range(L)]


def capture(fn):
    """Graph of fn(layer) over every layer; returns a replay callable."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for li in range(L):
            fn(li)                                   # warm-up, first launches
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for li in range(L):
            fn(li)
    return g.replay


def time_variants(variants):
    """variants: {name: replay}. Alternating rounds; median µs per call."""
    for r in variants.values():
        for _ in range(3):
            r()
    torch.cuda.synchronize()
    times = {n: [] for n in variants}
    for _ in range(args.reps):
        for n, r in variants.items():
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record()
            r()
            b.record()
            b.synchronize()
            times[n].append(a.elapsed_time(b) * 1e3 / L)
    return {n: (statistics.median(t), min(t), max(t)) for n, t in times.items()}


lines = []


def report(title, res, nbytes, base):
    for n, (med, lo, hi) in res.items():
        b = nbytes[n]
        lines.append(
            f"{title:<26} {n:<10} {med:8.2f} us  (min {lo:7.2f} max {hi:7.2f})"
            f"  {b / 1e6:8.1f} MB  {b / med / 1e6:6.2f} TB/s"
            f"  x{res[base][0] / med:5.2f} vs {base}")
        print(lines[-1], flush=True)


# ------------------------------------------------------------- narrow
for B in [int(v) for v in args.narrow.split(",")]:
    ids = routing(B)
    P = B * TOPK
    x = torch.randn(B, H, dtype=BF, device=DEV) * 0.5
    hin = torch.randn(P, I, dtype=BF, device=DEV) * 0.5
    pair_token = torch.arange(B, device=DEV, dtype=torch.int32
                              ).repeat_interleave(TOPK)
    pe = [i.flatten().contiguous() for i in ids]
    pw = torch.full((P,), 1.0 / TOPK, device=DEV)
    h = torch.empty(P, I, dtype=BF, device=DEV)
    out = torch.zeros(B, H, dtype=torch.float32, device=DEV)
    # bytes: an expert picked by two tokens is counted once (the second
    # read hits cache), PERF_NOTES' unique-expert-bytes convention
    res = time_variants({
        "bf16": capture(lambda li: ops.moe_gemv_h(
            h, x, layers[li]["w13"], pair_token, pe[li], out_zero=out)),
        "fp8": capture(lambda li: ops.moe_gemv_h_fp8(
            h, x, layers[li]["w13_q"], layers[li]["w13_s"], pair_token,
            pe[li], out_zero=out)),
    })
    uniq = sum(int(p.unique().numel()) for p in pe) / L
    report(f"gemv_h    B={B}", res,
           {"bf16": uniq * 2 * I * H * 2, "fp8": uniq * 2 * I * H}, "bf16")
    res = time_variants({
        "bf16": capture(lambda li: ops.moe_gemv_down(
            out, hin, layers[li]["w2"], pw, pair_token, pe[li])),
        "fp8": capture(lambda li: ops.moe_gemv_down_fp8(
            out, hin, layers[li]["w2_q"], layers[li]["w2_s"], pw, pair_token,
            pe[li])),
    })
    report(f"gemv_down B={B}", res,
           {"bf16": uniq * H * I * 2, "fp8": uniq * H * I}, "bf16")

# --------------------------------------------------------------- wide
for M in [int(v) for v in args.wide.split(",")]:
    ids = routing(M)
    P = M * TOPK
    x = torch.randn(M, H, dtype=BF, device=DEV) * 0.5
    hin = torch.randn(P, I, dtype=BF, device=DEV) * 0.5
    tok = torch.arange(M, device=DEV, dtype=torch.int32).repeat_interleave(TOPK)
    pair_row = torch.arange(P, device=DEV, dtype=torch.int32)
    pts, descs, uniq = [], [], 0
    for i in ids:
        flat = i.flatten()
        order = torch.argsort(flat)
        pe = flat[order].int().contiguous()
        pts.append(tok[order].contiguous())
        descs.append(ops.moe_build_desc_device(pe, E, bm=16))
        uniq += int(pe.unique().numel()) / L
    gateup = torch.empty(P, 2 * I, dtype=BF, device=DEV)
    z = torch.empty(P, H, dtype=BF, device=DEV)

    res = time_variants({
        "bf16": capture(lambda li: ops.moe_grouped_gemm_skinny(
            gateup, x, layers[li]["w13"], pts[li], descs[li])),
        "fp8": capture(lambda li: ops.moe_grouped_gemm_skinny_fp8(
            gateup, x, layers[li]["w13_q"], layers[li]["w13_s"], pts[li],
            descs[li]))})
    b8 = uniq * 2 * I * H
    report(f"skinny gate/up M={M}", res, {"bf16": 2 * b8, "fp8": b8}, "bf16")
    res = time_variants({
        "bf16": capture(lambda li: ops.moe_grouped_gemm_skinny(
            z, hin, layers[li]["w2"], pair_row, descs[li])),
        "fp8": capture(lambda li: ops.moe_grouped_gemm_skinny_fp8(
            z, hin, layers[li]["w2_q"], layers[li]["w2_s"], pair_row,
            descs[li]))})
    b8 = uniq * H * I
    report(f"skinny down    M={M}", res, {"bf16": 2 * b8, "fp8": b8}, "bf16")

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
