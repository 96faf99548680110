#!/usr/bin/env python3
"""Bit-level A/B of the decode step's short kernels between two builds.

    python scripts/gpu_decode_chain_ab.py --out DIR     # run on one build
    python scripts/gpu_decode_chain_ab.py --compare DIR_A DIR_B

--out runs split+merge attention, the dense GEMVs (plain, LDS-staged,
add+norm-fused), the MoE gate/up GEMV and both routers at the decode shapes
from fixed seeds with
the build this copy of the script sits in, and saves every output's raw bits
as DIR/<name>.npy. --compare needs no GPU: it checks that two such
directories hold the same files with the same bytes and exits 1 otherwise.

Shapes: B in {1, 2, 5, 8}, H=2048, qdim=4096, E=128, K=8; attention contexts
1, 33, 1000, 1024 tokens at 32 splits and 2048 at 64.
"""
from __future__ import annotations

import argparse
import os
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

BATCHES = (1, 2, 5, 8)
H, QDIM, NQKV, E, K = 2048, 4096, 5120, 128, 8
HQ, HK, D, BS = 32, 4, 128, 16


def _bits(t):
    """Raw bits of a tensor as a numpy integer array."""
    import torch
    t = t.detach().contiguous()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    elif t.dtype == torch.float32:
        t = t.view(torch.int32)
    return t.cpu().numpy()


def run(out_dir: str) -> None:
    import torch

    from room_amd import ops

    assert torch.cuda.is_available(), "--out needs a GPU"
    dev = "cuda"
    os.makedirs(out_dir, exist_ok=True)
    saved = []

    def save(name, t):
        np.save(os.path.join(out_dir, name + ".npy"), _bits(t))
        saved.append(name)

    def randn(*shape, dtype=torch.bfloat16, scale=1.0):
        return (torch.randn(*shape, dtype=torch.float32, device=dev)
                * scale).to(dtype)

    # ---- dense GEMV: QKV (H=2048), O (H=4096), an LDS-staged wide-N shape
    torch.manual_seed(100)
    wqkv = randn(NQKV, H, scale=0.05)
    wo = randn(H, QDIM, scale=0.05)
    wide = randn(16388, H, scale=0.05)
    gamma = randn(H)
    for B in BATCHES:
        x = randn(B, H)
        a = randn(B, QDIM)
        for tag, xx, w in (("qkv", x, wqkv), ("o", a, wo), ("wide", x, wide)):
            for dt, dn in ((torch.bfloat16, "bf16"), (torch.float32, "f32")):
                y = torch.empty(B, w.size(0), dtype=dt, device=dev)
                ops.gemv(y, xx, w)
                save(f"gemv_{tag}_B{B}_{dn}", y)
        if B <= 2:
            delta = randn(B, H, dtype=torch.float32, scale=0.1)
            none = torch.empty(0, dtype=torch.float32, device=dev)
            for tag, dl in (("delta", delta), ("plain", none)):
                y = torch.empty(B, NQKV, dtype=torch.bfloat16, device=dev)
                x_out = torch.empty_like(x)
                ops.gemv_addnorm(y, x.clone(), dl, x_out, gamma, wqkv, 1e-6)
                save(f"addnorm_{tag}_B{B}_y", y)
                if dl.numel():
                    save(f"addnorm_{tag}_B{B}_xout", x_out)

    # ---- routers: decode (H-split GEMV + top-k) and prefill (logits) entry
    torch.manual_seed(101)
    wr = randn(E, H, scale=0.05)
    wr_tie = wr.clone()
    wr_tie[[40, 41, 90]] = wr_tie[7].clone()      # exact copies: bit-equal logits
    for B in BATCHES:
        x = randn(B, H, scale=0.5)
        for tag, w in (("rand", wr), ("tie", wr_tie)):
            ids, wts = ops.router_gemv_topk(x, w, K)
            save(f"router_{tag}_B{B}_ids", ids)
            save(f"router_{tag}_B{B}_w", wts)
    logits = torch.randn(33, E, dtype=torch.float32, device=dev) * 2
    logits[:, [40, 41, 90]] = logits[:, 7:8].clone()
    ids, wts = ops.moe_router(logits, K)
    save("moe_router_T33_ids", ids)
    save("moe_router_T33_w", wts)

    # ---- MoE gate/up GEMV (the down GEMV accumulates with float atomics in
    # no fixed order, so its bits are not comparable; its tests carry it)
    torch.manual_seed(103)
    NE, I = 16, 768
    w13 = randn(NE, 2 * I, H, scale=0.02)
    for B in BATCHES:
        x = randn(B, H, scale=0.5)
        pair_token = torch.arange(B, device=dev).repeat_interleave(K).int()
        pair_expert = torch.stack(
            [torch.randperm(NE, device=dev)[:K] for _ in range(B)]
        ).flatten().int()
        h = torch.empty(B * K, I, dtype=torch.bfloat16, device=dev)
        ops.moe_gemv_h(h, x, w13, pair_token, pair_expert)
        save(f"moe_gemv_h_B{B}", h)

    # ---- split-KV attention + merge
    torch.manual_seed(102)
    max_len = 2048
    max_blocks = max_len // BS
    nsp = ops.attn_nsplits()
    for B in BATCHES:
        nb = B * max_blocks + 1
        kcache = randn(nb, HK, BS, D)
        vcache = randn(nb, HK, BS, D)
        bt = torch.arange(1, nb, dtype=torch.int32, device=dev
                          ).reshape(B, max_blocks)
        q = randn(B, HQ, D)
        seq_ids = torch.arange(B, dtype=torch.int32, device=dev)
        part = torch.empty(B, HQ, nsp, D, dtype=torch.float32, device=dev)
        part_ml = torch.empty(B, HQ, nsp, 2, dtype=torch.float32, device=dev)
        for splits, ctxs in ((32, (1, 33, 1000, 1024)), (64, (2048,))):
            for i, ctx in enumerate(ctxs):
                # every context at every batch row once: rotate the list
                lens = [ctxs[(i + b) % len(ctxs)] for b in range(B)]
                q_pos = torch.tensor([l - 1 for l in lens], dtype=torch.int32,
                                     device=dev)
                out = torch.empty_like(q)
                ops.paged_attention_split(out, q, kcache, vcache, bt, seq_ids,
                                          q_pos, part, part_ml, D ** -0.5,
                                          splits=splits)
                save(f"attn_s{splits}_B{B}_rot{i}", out)
    torch.cuda.synchronize()
    print(f"saved {len(saved)} arrays to {out_dir}")


def compare(dir_a: str, dir_b: str) -> int:
    names_a = sorted(f for f in os.listdir(dir_a) if f.endswith(".npy"))
    names_b = sorted(f for f in os.listdir(dir_b) if f.endswith(".npy"))
    bad = 0
    if names_a != names_b:
        print("file lists differ:", sorted(set(names_a) ^ set(names_b)))
        bad += 1
    for name in sorted(set(names_a) & set(names_b)):
        a = np.load(os.path.join(dir_a, name))
        b = np.load(os.path.join(dir_b, name))
        same = a.shape == b.shape and a.dtype == b.dtype and \
            a.tobytes() == b.tobytes()
        if not same:
            ndiff = int((a != b).sum()) if a.shape == b.shape else -1
            print(f"DIFF  {name}: {ndiff} of {a.size} elements differ")
            bad += 1
    total = len(set(names_a) & set(names_b))
    print(f"{total - bad if bad <= total else 0} of {total} arrays bit-identical"
          f" ({dir_a} vs {dir_b})")
    return 1 if bad else 0


def main() -> None:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    g = p.add_mutually_exclusive_group(required=True)
    g.add_argument("--out", metavar="DIR")
    g.add_argument("--compare", nargs=2, metavar=("DIR_A", "DIR_B"))
    args = p.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    run(args.out)


if __name__ == "__main__":
    main()
