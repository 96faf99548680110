"""Sampler pair (scan + finaliser) device timings at B = 5, V = 151936.

Variants, alternated round-robin in one process after warm-up, each timed
with device events around ITERS back-to-back calls of the C++ op (so a call
is the two launches and nothing else):
  off     sample_rows, penalties off (the default request)
  pen64   sample_rows, repetition 1.1 + presence/frequency, repeat_last_n 64
  pen256  the same with repeat_last_n 256 (full ring)
  parent  sample_tokens of an extension built from the parent commit, when
          --parent-ext names its _C*.so (old and new in one process)
Back-to-back calls overlap launch gaps with kernel time; for the summed kernel
time of the pair run one variant under the kernel tracer in a run of its own:
  rocprofv3 --kernel-trace --stats -d OUT -- python scripts/... --only off
Prints a markdown table (median / min / max µs per call over rounds); --out
also writes it to a file.
"""
import argparse
import importlib.util
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from room_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--b", type=int, default=5)
ap.add_argument("--v", type=int, default=151936)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--seed", type=int, default=41)
ap.add_argument("--only", default=None, help="time this variant alone")
ap.add_argument("--parent-ext", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()

assert torch.cuda.is_available(), "needs a GPU"
dev = torch.device("cuda")
B, V = args.b, args.v
g = torch.Generator(device=dev)
g.manual_seed(args.seed)
logits = torch.empty(B, V, device=dev).normal_(generator=g)
f32 = dict(dtype=torch.float32, device=dev)
i32 = dict(dtype=torch.int32, device=dev)
temperature = torch.full((B,), 0.7, **f32)
top_p = torch.full((B,), 0.95, **f32)
top_k = torch.full((B,), 40, **i32)
seeds = torch.randint(1, 2**62, (B,), generator=g, device=dev)
ctr = torch.zeros(B, **i32)
ring = torch.randint(0, V, (B, ops.RING), generator=g, device=dev,
                     dtype=torch.int32)
ring_len = torch.full((B,), 1000, **i32)
out = torch.empty(B, **i32)
C = ops._require()


def rows(rep, pres, freq, n):
    cols = (torch.full((B,), rep, **f32), torch.full((B,), pres, **f32),
            torch.full((B,), freq, **f32), torch.full((B,), n, **i32))
    return lambda: C.sample_rows(out, logits, temperature, top_p, top_k, seeds,
                                 ctr, *cols, ring, ring_len, False)


variants = {
    "off": ("sample_rows, penalties off", rows(1.0, 0.0, 0.0, 64)),
    "pen64": ("sample_rows, repeat_last_n 64", rows(1.1, 0.2, 0.1, 64)),
    "pen256": ("sample_rows, repeat_last_n 256", rows(1.1, 0.2, 0.1, 256)),
}
if args.parent_ext:
    spec = importlib.util.spec_from_file_location("_C", args.parent_ext)
    P = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(P)
    pseeds = seeds.clone()
    variants["parent"] = (
        "parent sample_tokens",
        lambda: P.sample_tokens(out, logits, pseeds, 40, 0.7, 0.95))
if args.only:
    variants = {args.only: variants[args.only]}

for _, fn in variants.values():             # warm-up: every variant
    for _ in range(20):
        fn()
torch.cuda.synchronize()

times = {name: [] for name in variants}
for _ in range(args.rounds):
    for name, (_, fn) in variants.items():
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        e1.synchronize()
        times[name].append(e0.elapsed_time(e1) * 1e3 / args.iters)  # µs/call

lines = [f"B={B} V={V} iters={args.iters} rounds={args.rounds} seed={args.seed}",
         "",
         "| variant | what | median µs | min µs | max µs |",
         "|---|---|---|---|---|"]
for name, (what, _) in variants.items():
    t = times[name]
    lines.append(f"| {name} | {what} | {statistics.median(t):.1f} | "
                 f"{min(t):.1f} | {max(t):.1f} |")
text = "\n".join(lines)
print(text, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
