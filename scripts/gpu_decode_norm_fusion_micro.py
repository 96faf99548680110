#!/usr/bin/env python3
"""The decode layer's two norm fusions, unfused against fused, at the 30b
shapes (H = 2048, qdim = 4096, QKV rows = 5120, E = 128, K = 8).

    python scripts/gpu_decode_norm_fusion_micro.py [--batches 1,2,5,8]
    python scripts/gpu_decode_norm_fusion_micro.py --out DIR
    python scripts/gpu_decode_norm_fusion_micro.py --compare DIR_A DIR_B

Timing (default): per B, two variants of the chain from the attention output
to the router's top-k,
    old    gemv (O) -> fused_add_rmsnorm -> router_gemv_topk      4 kernels
    fused  gemv_residual -> router_norm_gemv_topk                 3 kernels
and two of the input norm + QKV projection,
    old    fused_add_rmsnorm (f32 delta) -> gemv                  2 kernels
    fused  gemv_addnorm                                           1 kernel
each captured as one graph that runs the chain once per layer over --layers
independent layers of weights (default 16: 16 x 17.3 MB, or 16 x 21 MB of QKV
weights, is more than the 256 MB last-level cache, so W streams from HBM as in
a decode step). The variants are warmed up and then timed alternately for --reps rounds with
device events; the table gives median and min-max µs per layer.

--out runs both chains from fixed seeds and saves the raw bits of the
residual, the normed rows and the router's ids and weights of the first, and
the QKV rows and residual of the second, as DIR/<name>.npy. The post-attention
chain is the fused one where the build has the ops and the old composition
otherwise. The input chain is gemv_addnorm at every B on a build with the
rebuilt kernel (more than its decode layer does, which takes the two launches
at B >= 3); on an older build it is gemv_addnorm at B <= 2 and the two
launches above, as that build's decode layer runs it. --compare needs no GPU: two such directories must hold the
same files with the same bytes; exits 1 otherwise. Every array here is
upstream of moe_gemv_down's float atomics, so all are expected bit-identical.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

H, QDIM, NQKV, E, K, EPS = 2048, 4096, 5120, 128, 8, 1e-6


def _bits(t):
    import torch
    t = t.detach().contiguous()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    elif t.dtype == torch.float32:
        t = t.view(torch.int32)
    return t.cpu().numpy()


def _old_chain(ops, torch, x, attn, obuf, hbuf, gamma, wo, wr):
    ops.gemv(obuf, attn, wo)
    ops.fused_add_rmsnorm(hbuf, x, obuf, gamma, EPS)
    return ops.router_gemv_topk(hbuf, wr, K)


def _fused_chain(ops, torch, x, attn, obuf, hbuf, gamma, wo, wr):
    ops.gemv_residual(x, attn, wo)
    return ops.router_norm_gemv_topk(hbuf, x, gamma, wr, K, EPS)


def _inputs(torch, B, L, dev):
    bf = dict(dtype=torch.bfloat16, device=dev)
    layers = [dict(wo=torch.empty(H, QDIM, **bf).normal_(0, 0.02),
                   wr=torch.empty(E, H, **bf).normal_(0, 0.02),
                   gamma=(1 + 0.1 * torch.randn(H, device=dev)).to(torch.bfloat16))
              for _ in range(L)]
    return dict(layers=layers, x=torch.randn(B, H, **bf),
                attn=torch.randn(B, QDIM, **bf),
                obuf=torch.empty(B, H, **bf), hbuf=torch.empty(B, H, **bf))


def time_all(batches, L, reps, out_path):
    import torch
    from room_amd import ops

    assert torch.cuda.is_available(), "timing needs a GPU"
    dev = torch.device("cuda", 0)
    torch.manual_seed(7)
    lines = []
    for B in batches:
        c = _inputs(torch, B, L, dev)

        def capture(chain):
            def run():
                for ly in c["layers"]:
                    chain(ops, torch, c["x"], c["attn"], c["obuf"], c["hbuf"],
                          ly["gamma"], ly["wo"], ly["wr"])
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

        variants = {"old": capture(_old_chain)}
        if hasattr(ops, "gemv_residual"):        # absent on an older build
            variants["fused"] = capture(_fused_chain)
        for r in variants.values():
            for _ in range(3):
                r()
        torch.cuda.synchronize()
        times = {n: [] for n in variants}
        for _ in range(reps):
            for n, r in variants.items():
                # the residual is updated in place by every replay: restart
                # it so both variants always see finite, comparable rows
                c["x"].normal_()
                a = torch.cuda.Event(enable_timing=True)
                b = torch.cuda.Event(enable_timing=True)
                a.record()
                r()
                b.record()
                b.synchronize()
                times[n].append(a.elapsed_time(b) * 1e3 / L)
        base = statistics.median(times["old"])
        for n, t in times.items():
            med = statistics.median(t)
            lines.append(f"post-attn chain B={B}  {n:<6} {med:7.2f} us/layer  "
                         f"(min {min(t):6.2f} max {max(t):6.2f})  "
                         f"{med - base:+6.2f} us vs old")
            print(lines[-1], flush=True)
    # ---- input norm + QKV
    for B in batches:
        bf = dict(dtype=torch.bfloat16, device=dev)
        wq = [torch.empty(NQKV, H, **bf).normal_(0, 0.02) for _ in range(L)]
        gam = (1 + 0.1 * torch.randn(H, device=dev)).to(torch.bfloat16)
        xa, xb = torch.randn(B, H, **bf), torch.empty(B, H, **bf)
        delta = torch.randn(B, H, dtype=torch.float32, device=dev) * 0.1
        hb = torch.empty(B, H, **bf)
        qkv = torch.empty(B, NQKV, **bf)

        def old_pair():
            for wl in wq:
                ops.fused_add_rmsnorm(hb, xa, delta, gam, EPS)
                ops.gemv(qkv, hb, wl)

        def fused():
            for wl in wq:
                ops.gemv_addnorm(qkv, xa, delta, xb, gam, wl, EPS)

        def capture2(run):
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

        variants = {"old": capture2(old_pair), "fused": capture2(fused)}
        for r in variants.values():
            for _ in range(3):
                r()
        torch.cuda.synchronize()
        times = {n: [] for n in variants}
        for _ in range(reps):
            for n, r in variants.items():
                xa.normal_()                 # old_pair adds delta in place
                a = torch.cuda.Event(enable_timing=True)
                b = torch.cuda.Event(enable_timing=True)
                a.record()
                r()
                b.record()
                b.synchronize()
                times[n].append(a.elapsed_time(b) * 1e3 / L)
        base = statistics.median(times["old"])
        for n, t in times.items():
            med = statistics.median(t)
            lines.append(f"input norm + QKV B={B}  {n:<8} {med:7.2f} us/layer  "
                         f"(min {min(t):6.2f} max {max(t):6.2f})  "
                         f"{med - base:+6.2f} us vs old")
            print(lines[-1], flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


def dump(out_dir, batches):
    import torch
    from room_amd import ops

    assert torch.cuda.is_available(), "--out needs a GPU"
    dev = torch.device("cuda", 0)
    os.makedirs(out_dir, exist_ok=True)
    fused = hasattr(ops, "gemv_residual")
    chain = _fused_chain if fused else _old_chain
    n = 0
    for B in batches:
        torch.manual_seed(200 + B)
        c = _inputs(torch, B, 2, dev)
        # exact copies of one router row: bit-equal logits among the leaders
        wr = c["layers"][1]["wr"]
        wr[[40, 41, 90]] = wr[7].clone()
        for li, ly in enumerate(c["layers"]):
            ids, w = chain(ops, torch, c["x"], c["attn"], c["obuf"],
                           c["hbuf"], ly["gamma"], ly["wo"], ly["wr"])
            for name, t in (("res", c["x"]), ("hbuf", c["hbuf"]),
                            ("ids", ids), ("w", w)):
                np.save(os.path.join(out_dir, f"post_B{B}_L{li}_{name}.npy"),
                        _bits(t))
                n += 1
        # input norm + QKV: the rebuilt gemv_addnorm (it came with
        # gemv_residual) at every B; an older build's only at B <= 2
        any_b = fused
        bf = dict(dtype=torch.bfloat16, device=dev)
        wq = torch.empty(NQKV, H, **bf).normal_(0, 0.02)
        gam = (1 + 0.1 * torch.randn(H, device=dev)).to(torch.bfloat16)
        xin = torch.randn(B, H, **bf)
        delta = torch.randn(B, H, dtype=torch.float32, device=dev) * 0.1
        qkv = torch.empty(B, NQKV, **bf)
        xo = torch.empty(B, H, **bf)
        if any_b or B <= 2:
            ops.gemv_addnorm(qkv, xin, delta, xo, gam, wq, EPS)
        else:
            xo.copy_(xin)
            hb = torch.empty(B, H, **bf)
            ops.fused_add_rmsnorm(hb, xo, delta, gam, EPS)
            ops.gemv(qkv, hb, wq)
        for name, t in (("qkv", qkv), ("xout", xo)):
            np.save(os.path.join(out_dir, f"input_B{B}_{name}.npy"), _bits(t))
            n += 1
    torch.cuda.synchronize()
    print(f"saved {n} arrays to {out_dir} "
          f"({'fused' if fused else 'unfused'} chain)")


def compare(dir_a, dir_b):
    names_a = sorted(f for f in os.listdir(dir_a) if f.endswith(".npy"))
    names_b = sorted(f for f in os.listdir(dir_b) if f.endswith(".npy"))
    bad = 0
    if names_a != names_b:
        print("file lists differ:", sorted(set(names_a) ^ set(names_b)))
        bad += 1
    both = sorted(set(names_a) & set(names_b))
    for name in both:
        a = np.load(os.path.join(dir_a, name))
        b = np.load(os.path.join(dir_b, name))
        if not (a.shape == b.shape and a.dtype == b.dtype
                and a.tobytes() == b.tobytes()):
            nd = int((a != b).sum()) if a.shape == b.shape else -1
            print(f"DIFF  {name}: {nd} of {a.size} elements differ")
            bad += 1
    print(f"{max(len(both) - bad, 0)} of {len(both)} arrays bit-identical "
          f"({dir_a} vs {dir_b})")
    return 1 if bad or not both else 0


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--batches", default="1,2,5,8")
    p.add_argument("--layers", type=int, default=16)
    p.add_argument("--reps", type=int, default=60)
    p.add_argument("--table", metavar="FILE", default=None,
                   help="also write the timing table to FILE")
    p.add_argument("--out", metavar="DIR")
    p.add_argument("--compare", nargs=2, metavar=("DIR_A", "DIR_B"))
    args = p.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    batches = [int(v) for v in args.batches.split(",")]
    if args.out:
        dump(args.out, batches)
    else:
        time_all(batches, args.layers, args.reps, args.table)


if __name__ == "__main__":
    main()
