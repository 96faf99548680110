"""vs_topk vs vs_topk_scoped device timings at N = 1M × 384 bf16 (0.77 GB).

Variants, alternated round-robin in one process after warm-up, each timed
with device events around ITERS back-to-back calls (score + merge kernels,
through the ops wrappers):
  a   vs_topk, Q=1                         (the unscoped single-query kernel)
  b   vs_topk_scoped, Q=1, scope -1
  c   vs_topk_scoped, Q=5, scope -1        (compare with 5 × a)
  c8  vs_topk_scoped, Q=8, scope -1
  d   vs_topk_scoped, Q=1, scoped to a room holding 1/8 of the rows
Bytes are what the algorithm must read, from shapes: admitted rows × 768 B,
plus 4 B/row of tags for the scoped kernel. Prints a markdown table
(median / min / max over rounds); --out also writes it to a file.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from room_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--k", type=int, default=20)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--seed", type=int, default=40)
ap.add_argument("--out", default=None)
args = ap.parse_args()

assert torch.cuda.is_available(), "needs a GPU"
dev = torch.device("cuda")
N, K = args.n, args.k
g = torch.Generator(device=dev)
g.manual_seed(args.seed)
mat = torch.nn.functional.normalize(
    torch.empty(N, 384, device=dev).normal_(generator=g), dim=-1).to(torch.bfloat16)
tags = torch.randint(1, 9, (N,), generator=g, device=dev, dtype=torch.int32)
qs = torch.nn.functional.normalize(
    torch.empty(8, 384, device=dev).normal_(generator=g), dim=-1)
room_rows = int((tags == 1).sum())


def scopes(vals):
    return torch.tensor(vals, dtype=torch.int32, device=dev)


q1, q5 = qs[:1].contiguous(), qs[:5].contiguous()
s1, s5, s8, sroom = scopes([-1]), scopes([-1] * 5), scopes([-1] * 8), scopes([1])
ROW = 768
variants = {
    "a": ("vs_topk Q=1", lambda: ops.vs_topk(mat, qs[0], K), N * ROW),
    "b": ("scoped Q=1 scope -1",
          lambda: ops.vs_topk_scoped(mat, tags, q1, s1, K), N * (ROW + 4)),
    "c": ("scoped Q=5 scope -1",
          lambda: ops.vs_topk_scoped(mat, tags, q5, s5, K), N * (ROW + 4)),
    "c8": ("scoped Q=8 scope -1",
           lambda: ops.vs_topk_scoped(mat, tags, qs, s8, K), N * (ROW + 4)),
    "d": (f"scoped Q=1 room 1/8 ({room_rows} rows)",
          lambda: ops.vs_topk_scoped(mat, tags, q1, sroom, K),
          room_rows * ROW + N * 4),
}

# results must agree before the timings mean anything
va, ia = ops.vs_topk(mat, qs[0], K)
vb, ib = ops.vs_topk_scoped(mat, tags, q1, s1, K)
vc, _ = ops.vs_topk_scoped(mat, tags, q5, s5, K)
vd, idd = ops.vs_topk_scoped(mat, tags, q1, sroom, K)
torch.cuda.synchronize()
print(f"max |a-b| values {float((va - vb[0]).abs().max()):.2e}, "
      f"same rows {bool((ia == ib[0]).all())}; "
      f"max |b-c[0]| {float((vb[0] - vc[0]).abs().max()):.2e}; "
      f"d rows all in room 1: {bool((tags[idd[0]] == 1).all())}", flush=True)

for _, fn, _ in variants.values():          # warm-up: every variant, every shape
    for _ in range(5):
        fn()
torch.cuda.synchronize()

times = {name: [] for name in variants}
for _ in range(args.rounds):
    for name, (_, fn, _) in variants.items():
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        e1.synchronize()
        times[name].append(e0.elapsed_time(e1) * 1e3 / args.iters)   # µs/call

lines = [f"N={N} K={K} iters={args.iters} rounds={args.rounds} seed={args.seed}",
         "",
         "| variant | what | median µs | min µs | max µs | GB read | TB/s at median |",
         "|---|---|---|---|---|---|---|"]
med = {}
for name, (what, _, nbytes) in variants.items():
    t = times[name]
    med[name] = statistics.median(t)
    lines.append(f"| {name} | {what} | {med[name]:.1f} | {min(t):.1f} | "
                 f"{max(t):.1f} | {nbytes / 1e9:.3f} | "
                 f"{nbytes / med[name] / 1e6:.2f} |")
lines += ["",
          f"b/a = {med['b'] / med['a']:.2f}; c/(5a) = {med['c'] / (5 * med['a']):.2f}; "
          f"c8/(8a) = {med['c8'] / (8 * med['a']):.2f}; d/b = {med['d'] / med['b']:.2f}"]
text = "\n".join(lines)
print(text, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
