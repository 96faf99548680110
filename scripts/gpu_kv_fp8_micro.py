#!/usr/bin/env python3
"""The KV-cache kernels on a bf16 cache against an fp8 one (e4m3 rows, one f32
scale per row), at the 30b shapes (32 q heads, 4 kv heads, head_dim 128).

    python scripts/gpu_kv_fp8_micro.py [--reps 40] [--table FILE]

Per case, the bf16 op and its fp8 twin are each captured as one graph that
runs the op once per layer over independent caches, enough layers that the
fp8 caches alone are past the 256 MB last-level cache (at most 48), so K and
V stream from HBM as in a decode step. The variants are warmed up and timed
alternately for --reps rounds with device events; the table gives median and
min-max µs per call.

    paged_attention_split   B = 5, contexts 2k, 8k, 16k, 32 splits
    flash_prefill           T = 2048, one sequence
    qk_rope_write_kv        T = 5 and T = 2048

On a build without the fp8 cache (no reference.quantize_kv_rows) only the
bf16 column is timed, which is how the parent's kernels are measured.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

HQ, HK, D, BS = 32, 4, 128, 16
SCALE = D ** -0.5
LLC_BYTES = 600e6


def _layers(fp8_bytes_per_layer):
    return int(max(2, min(48, -(-LLC_BYTES // fp8_bytes_per_layer))))


def _capture(torch, run):
    """A graph of run(). The graph holds raw pointers only: the caller keeps
    every tensor run() touches alive for as long as it replays."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()                                # first launches
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    return g.replay


def _time(torch, variants, reps, calls, label, lines):
    for r in variants.values():
        for _ in range(3):
            r()
    torch.cuda.synchronize()
    times = {n: [] for n in variants}
    for _ in range(reps):
        for n, r in variants.items():
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record()
            r()
            b.record()
            b.synchronize()
            times[n].append(a.elapsed_time(b) * 1e3 / calls)
    base = statistics.median(times["bf16"])
    for n, t in times.items():
        med = statistics.median(t)
        lines.append(f"{label:<34} {n:<5} {med:8.2f} us/call  "
                     f"(min {min(t):7.2f} max {max(t):7.2f})  "
                     f"x{med / base:5.3f} of bf16")
        print(lines[-1], flush=True)


def _caches(torch, ref, nb, L, dev, fp8):
    """L layers of (kc, vc, ks, vs): random rows, or their quantised form."""
    out = []
    for _ in range(L):
        k = torch.randn(nb, HK, BS, D, device=dev).to(torch.bfloat16)
        v = torch.randn(nb, HK, BS, D, device=dev).to(torch.bfloat16)
        if fp8:
            (kq, ks), (vq, vs) = ref.quantize_kv_rows(k), ref.quantize_kv_rows(v)
            out.append((kq, vq, dict(k_scale=ks, v_scale=vs)))
        else:
            out.append((k, v, {}))
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--reps", type=int, default=40)
    p.add_argument("--table", metavar="FILE", default=None,
                   help="also write the timing table to FILE")
    args = p.parse_args()

    import torch
    from room_amd import ops
    from room_amd.ops import reference as ref

    assert torch.cuda.is_available(), "timing needs a GPU"
    dev = torch.device("cuda", 0)
    torch.manual_seed(11)
    modes = ["bf16"] + (["fp8"] if hasattr(ref, "quantize_kv_rows") else [])
    i32 = dict(dtype=torch.int32, device=dev)
    bf = dict(dtype=torch.bfloat16, device=dev)
    lines = []

    # ---- split decode, B = 5
    B = 5
    for ctx in (2048, 8192, 16384):
        per_seq = ctx // BS
        nb = B * per_seq + 1
        L = _layers(2 * nb * HK * BS * (D + 4))
        perm = torch.randperm(nb - 1) + 1
        bt = perm.view(B, per_seq).to(**i32)
        seq, pos = torch.arange(B, **i32), torch.full((B,), ctx - 1, **i32)
        q = torch.randn(B, HQ, D, **bf)
        out = torch.empty(B, HQ, D, **bf)
        part = torch.empty(B, HQ, ops.attn_nsplits(), D, device=dev)
        part_ml = torch.empty(B, HQ, ops.attn_nsplits(), 2, device=dev)
        caches = {m: _caches(torch, ref, nb, L, dev, m == "fp8")
                  for m in modes}        # alive until the case is timed
        variants = {}
        for m in modes:
            def run(layers=caches[m]):
                for kc, vc, kw in layers:
                    ops.paged_attention_split(out, q, kc, vc, bt, seq, pos,
                                              part, part_ml, SCALE, splits=32,
                                              **kw)
            variants[m] = _capture(torch, run)
        _time(torch, variants, args.reps, L,
              f"paged_attention_split B=5 ctx={ctx}", lines)
        del variants, caches
        torch.cuda.empty_cache()

    # ---- flash prefill, T = 2048, one sequence
    T = 2048
    nb = T // BS + 1
    L = 8
    bt = (torch.randperm(nb - 1) + 1).view(1, -1).to(**i32)
    seq, pos = torch.zeros(T, **i32), torch.arange(T, **i32)
    q = torch.randn(T, HQ, D, **bf)
    out = torch.empty(T, HQ, D, **bf)
    desc = ops.build_qtile_desc([(0, T)], dev)
    caches = {m: _caches(torch, ref, nb, L, dev, m == "fp8") for m in modes}
    variants = {}
    for m in modes:
        def run(layers=caches[m]):
            for kc, vc, kw in layers:
                ops.flash_prefill(out, q, kc, vc, bt, seq, pos, desc, SCALE,
                                  **kw)
        variants[m] = _capture(torch, run)
    _time(torch, variants, args.reps, L, "flash_prefill T=2048", lines)
    del variants, caches

    # ---- fused rope + KV write
    cos_t, sin_t = (t.to(dev) for t in ref.rope_tables(4096, D, 1e7))
    w = (1 + 0.1 * torch.randn(D, device=dev)).to(torch.bfloat16)
    for T in (5, 2048):
        nb = 2048 // BS + 1
        L = 16
        bt = (torch.randperm(nb - 1) + 1).view(1, -1).to(**i32)
        seq = torch.zeros(T, **i32)
        pos = torch.arange(T, **i32) if T > 5 else torch.arange(
            1000, 1005, **i32)
        qkv = torch.randn(T, (HQ + 2 * HK) * D, **bf)
        caches = {m: _caches(torch, ref, nb, L, dev, m == "fp8")
                  for m in modes}
        variants = {}
        for m in modes:
            def run(layers=caches[m]):
                for kc, vc, kw in layers:
                    ops.qk_rope_write_kv(qkv, HQ, kc, vc, w, w, cos_t, sin_t,
                                         bt, seq, pos, 1e-6, **kw)
            variants[m] = _capture(torch, run)
        _time(torch, variants, args.reps, L, f"qk_rope_write_kv T={T}", lines)
        del variants, caches

    if args.table:
        os.makedirs(os.path.dirname(os.path.abspath(args.table)), exist_ok=True)
        with open(args.table, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
