"""Prefill grouped GEMM on fp8 expert weights against the bf16 image, at the
30b shapes: moe_grouped_gemm128 on dequantize_fp8_block(q, s).to(bf16) against
moe_grouped_gemm128_fp8 on (q, s).

E = 128 experts, gate/up (N = 1536, K = 2048) and down (N = 2048, K = 768),
random top-8 routing, T in --tokens (default 64, 512, 2048, 4096).

Method (that of gpu_fp8_moe_micro.py): --layers independent layers of weights
(default 8: 9.7 GB of image + 4.8 GB of fp8), each with its own routing, so a
call streams its experts from HBM as a prefill layer does and not from the
last-level cache. One timed unit is a captured graph that runs the kernel once
per layer; the per-call time is the unit's device-event time over the layer
count. Both variants are warmed up, then timed alternately for --reps rounds
and the median taken; that is repeated --rounds times. Reported per variant:
the median of those medians, and their min and max (the spread).

Every T runs in a child process of its own under --step-timeout seconds, one
after the other; the first one that fails or runs out of time ends the run
with its exit status.
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--tokens", default="64,512,2048,4096")
ap.add_argument("--layers", type=int, default=8)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--experts", type=int, default=128)
ap.add_argument("--hidden", type=int, default=2048)
ap.add_argument("--inter", type=int, default=768)
ap.add_argument("--step-timeout", type=int, default=240)
ap.add_argument("--out", default=None)
ap.add_argument("--worker", type=int, default=None,
                help="internal: measure this one T and print its lines")
args = ap.parse_args()


def driver() -> int:
    lines = []
    for T in [int(v) for v in args.tokens.split(",")]:
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", str(T),
               "--layers", str(args.layers), "--reps", str(args.reps),
               "--rounds", str(args.rounds), "--experts", str(args.experts),
               "--hidden", str(args.hidden), "--inter", str(args.inter)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True,
                               timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            print(f"T={T}: no result after {args.step_timeout} s; stopping",
                  flush=True)
            return 124
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:
            print(f"T={T}: exit status {r.returncode}; stopping", flush=True)
            return r.returncode if r.returncode > 0 else 1
        lines += r.stdout.splitlines()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


def worker(T: int) -> int:
    import torch

    from room_amd import ops
    from room_amd.ops.reference import (dequantize_fp8_block,
                                        quantize_fp8_block)

    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    bf = torch.bfloat16
    E, H, I, topk, L = args.experts, args.hidden, args.inter, 8, args.layers
    torch.manual_seed(5)

    layers = []
    for _ in range(L):
        lay = {}
        for name, shape in (("w13", (E, 2 * I, H)), ("w2", (E, H, I))):
            w = torch.empty(*shape, dtype=bf, device=dev).normal_(0, 0.02)
            q, s = quantize_fp8_block(w)
            del w
            lay[name + "_q"], lay[name + "_s"] = q, s
            lay[name] = dequantize_fp8_block(q, s).to(bf)
        layers.append(lay)
    torch.cuda.synchronize()

    P = T * topk
    x = torch.randn(T, H, dtype=bf, device=dev) * 0.5
    hin = torch.randn(P, I, dtype=bf, device=dev) * 0.5
    tok = torch.arange(T, device=dev, dtype=torch.int32).repeat_interleave(topk)
    pair_row = torch.arange(P, device=dev, dtype=torch.int32)
    pts, descs, uniq, tiles = [], [], 0.0, 0.0
    for _ in range(L):
        flat = torch.randn(T, E, device=dev).topk(topk, dim=-1).indices.flatten()
        order = torch.argsort(flat)
        pe = flat[order].int().contiguous()
        pts.append(tok[order].contiguous())
        descs.append(ops.moe_build_desc_device(pe, E))
        uniq += int(pe.unique().numel()) / L
        tiles += int((descs[-1][:, 2] > 0).sum()) / L
    gateup = torch.empty(P, 2 * I, dtype=bf, device=dev)
    z = torch.empty(P, H, dtype=bf, device=dev)

    def capture(fn):
        """Graph of fn(layer) over every layer; returns a replay callable."""
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for li in range(L):
                fn(li)                               # warm-up, first launches
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for li in range(L):
                fn(li)
        return g.replay

    def time_variants(variants):
        """Alternating timing; per variant the --rounds medians, µs/call."""
        for r in variants.values():
            for _ in range(3):
                r()
        torch.cuda.synchronize()
        meds = {n: [] for n in variants}
        for _ in range(args.rounds):
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
            for n, t in times.items():
                meds[n].append(statistics.median(t))
        return meds

    def report(title, meds, wbytes):
        base = statistics.median(meds["image"])
        for n, m in meds.items():
            med = statistics.median(m)
            print(f"{title:<16} T={T:<5} {n:<6} {med:9.2f} us  (medians min "
                  f"{min(m):9.2f} max {max(m):9.2f})  {wbytes[n] / 1e6:7.1f} MB"
                  f" of weights  x{base / med:5.2f} vs image", flush=True)

    print(f"T={T}: {uniq:.1f} experts touched, {tiles:.1f} m-tiles per layer",
          flush=True)
    # weight bytes a call must stream: one panel per touched expert
    meds = time_variants({
        "image": capture(lambda li: ops.moe_grouped_gemm128(
            gateup, x, layers[li]["w13"], pts[li], descs[li])),
        "fp8": capture(lambda li: ops.moe_grouped_gemm128_fp8(
            gateup, x, layers[li]["w13_q"], layers[li]["w13_s"], pts[li],
            descs[li]))})
    b8 = uniq * 2 * I * H
    report("gate/up 1536x2048", meds, {"image": 2 * b8, "fp8": b8})
    meds = time_variants({
        "image": capture(lambda li: ops.moe_grouped_gemm128(
            z, hin, layers[li]["w2"], pair_row, descs[li])),
        "fp8": capture(lambda li: ops.moe_grouped_gemm128_fp8(
            z, hin, layers[li]["w2_q"], layers[li]["w2_s"], pair_row,
            descs[li]))})
    b8 = uniq * H * I
    report("down 2048x768", meds, {"image": 2 * b8, "fp8": b8})
    return 0


if __name__ == "__main__":
    sys.exit(driver() if args.worker is None else worker(args.worker))
