#!/usr/bin/env python3
"""flash_prefill device timings at the 30b head counts (32 q heads, 4 kv heads,
head_dim 128), this build against an extension built from the parent commit.

    python scripts/gpu_flash_prefill_micro.py [--parent-ext PATH/_C*.so]
                                              [--reps 24] [--table FILE]

Per shape and cache type (bf16, e4m3 rows with per-row scales) the op is
captured as one graph that runs it once per layer over independent caches,
enough layers that the fp8 caches alone are past the 256 MB last-level cache
(at most 48), so K and V stream from HBM as in a prefill forward. The builds
are warmed up and then timed alternately, one graph replay each, for --reps
rounds with device events; the table gives median and min-max µs per call
and TF/s of the causal work 4 * Hq * D * sum over rows of (position + 1).

    one sequence from zero                 T = 2048, T = 4096
    5 sequences x 704 new rows             on prefixes of 1k, 4k, 8k
    one 512-row chunk                      on a 14k prefix

Without --parent-ext only this build is timed.
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

HQ, HK, D, BS = 32, 4, 128, 16
SCALE = D ** -0.5
LLC_BYTES = 600e6

# name -> [(prefix, new rows)] per sequence
SHAPES = {
    "1 seq T=2048": [(0, 2048)],
    "1 seq T=4096": [(0, 4096)],
    "5 x 704 rows on 1k": [(1024, 704)] * 5,
    "5 x 704 rows on 4k": [(4096, 704)] * 5,
    "5 x 704 rows on 8k": [(8192, 704)] * 5,
    "512 rows on 14k": [(14336, 512)],
}


def _capture(torch, run):
    """A graph of run(). The graph holds raw pointers only: the caller keeps
    every tensor run() touches alive for as long as it replays."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    return g.replay


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--parent-ext", default=None,
                   help="_C*.so of an extension built from the parent commit")
    p.add_argument("--reps", type=int, default=24)
    p.add_argument("--only", default=None, help="substring of a shape name")
    p.add_argument("--table", metavar="FILE", default=None)
    args = p.parse_args()

    import torch
    from room_amd import ops
    from room_amd.ops import reference as ref

    assert torch.cuda.is_available(), "timing needs a GPU"
    dev = torch.device("cuda", 0)
    torch.manual_seed(11)
    builds = {"new": ops._require()}
    if args.parent_ext:
        spec = importlib.util.spec_from_file_location("_C", args.parent_ext)
        parent = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(parent)
        builds = {"parent": parent, "new": builds["new"]}
    i32 = dict(dtype=torch.int32, device=dev)
    lines = ["| shape | cache | build | median µs | min µs | max µs | TF/s | "
             "x parent |", "|---|---|---|---|---|---|---|---|"]
    print("\n".join(lines), flush=True)

    for name, seqs in SHAPES.items():
        if args.only and args.only not in name:
            continue
        per_seq = [(pre + n + BS - 1) // BS for pre, n in seqs]
        nb = sum(per_seq) + 1
        perm = torch.randperm(nb - 1) + 1
        bt = torch.zeros(len(seqs), max(per_seq), dtype=torch.int32)
        at = 0
        for s, k in enumerate(per_seq):
            bt[s, :k] = perm[at:at + k].int()
            at += k
        bt = bt.to(dev)
        seq = torch.cat([torch.full((n,), s, dtype=torch.int32)
                         for s, (_, n) in enumerate(seqs)]).to(dev)
        pos = torch.cat([torch.arange(pre, pre + n, dtype=torch.int32)
                         for pre, n in seqs]).to(dev)
        T = seq.numel()
        flop = 4.0 * HQ * D * float((pos.double() + 1).sum())
        segments, row0 = [], 0
        for _, n in seqs:
            segments.append((row0, n))
            row0 += n
        desc = ops.build_qtile_desc(segments, dev)
        q = torch.randn(T, HQ, D, device=dev).to(torch.bfloat16)
        out = torch.empty(T, HQ, D, dtype=torch.bfloat16, device=dev)
        L = int(max(2, min(48, -(-LLC_BYTES // (2 * nb * HK * BS * (D + 4))))))
        for mode in ("bf16", "e4m3"):
            layers = []
            for _ in range(L):
                k = torch.randn(nb, HK, BS, D, device=dev).to(torch.bfloat16)
                v = torch.randn(nb, HK, BS, D, device=dev).to(torch.bfloat16)
                if mode == "e4m3":
                    (k, ks), (v, vs) = (ref.quantize_kv_rows(k),
                                        ref.quantize_kv_rows(v))
                    layers.append((k, v, ks, vs))
                else:
                    layers.append((k, v, None, None))
            replays = {}
            for b, C in builds.items():
                def run(C=C):
                    for kc, vc, ks, vs in layers:
                        C.flash_prefill(out, q, kc, vc, bt, seq, pos, desc,
                                        SCALE, ks, vs)
                replays[b] = _capture(torch, run)
            for r in replays.values():
                for _ in range(2):
                    r()
            torch.cuda.synchronize()
            times = {b: [] for b in replays}
            for _ in range(args.reps):
                for b, r in replays.items():
                    e0 = torch.cuda.Event(enable_timing=True)
                    e1 = torch.cuda.Event(enable_timing=True)
                    e0.record()
                    r()
                    e1.record()
                    e1.synchronize()
                    times[b].append(e0.elapsed_time(e1) * 1e3 / L)
            base = statistics.median(times.get("parent", times["new"]))
            for b, t in times.items():
                med = statistics.median(t)
                lines.append(
                    f"| {name} | {mode} | {b} | {med:.1f} | {min(t):.1f} | "
                    f"{max(t):.1f} | {flop / med / 1e6:.0f} | "
                    f"{base / med:.2f} |")
                print(lines[-1], flush=True)
            del replays, layers
            torch.cuda.empty_cache()

    if args.table:
        os.makedirs(os.path.dirname(os.path.abspath(args.table)), exist_ok=True)
        with open(args.table, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
