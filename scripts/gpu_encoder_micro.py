"""MiniEncoder forward: impl="torch" (fp32 torch ops) against impl="hip" (bf16,
the project's HIP kernels) of this same commit, in one process.

Points:
  B=1   one 12-piece query
  B=8   mixed lengths (3 .. 128 pieces)
  B=64  128 pieces each
Both encoders share weights (same seed). The piece caches are warm. The two
variants are timed alternately, round-robin, after warm-up; per round and
variant one encode(texts) call is timed on the host clock twice: up to the
return of the last kernel launch ("host", measured on the un-synchronised
device forward) and up to the [B, 384] CPU result ("result", the whole
encode()). Prints a markdown table (median / min / max over rounds); --out
also writes it to a file.
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from room_amd.memory.encoder import MiniEncoder, tokenize  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=40)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()

assert torch.cuda.is_available(), "needs a GPU"


def words(n, tag):
    return " ".join(f"{tag}{i}" for i in range(n))


points = {
    "B=1, 12 pieces": [words(12, "q")],
    "B=8, mixed": [words(n, f"m{n}x") for n in (3, 12, 17, 31, 48, 64, 100, 128)],
    "B=64, 128 pieces": [words(128, f"t{b}x") for b in range(64)],
}
for name, texts in points.items():
    print(name, "pieces:", [len(tokenize(t)) for t in texts][:8], flush=True)

enc = {"torch": MiniEncoder(device="cuda", impl="torch"),
       "hip": MiniEncoder(device="cuda", impl="hip")}


def launch_only(impl, texts):
    """The device forward without the final copy to the host."""
    if impl == "hip":
        return enc[impl]._hip_forward(texts)
    return enc[impl]._pool_device(texts)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    del r
    return (t1 - t0) * 1e3


lines = [f"rounds={args.rounds} warmup={args.warmup}", "",
         "| point | impl | result ms median | min | max | host-to-last-launch "
         "ms median | min | max |",
         "|---|---|---|---|---|---|---|---|"]
summary = []
for name, texts in points.items():
    got = {k: e.encode(texts) for k, e in enc.items()}
    cosd = 1 - (got["hip"].double() * got["torch"].double()).sum(-1)
    print(f"{name}: max 1-cos hip vs torch {float(cosd.max()):.2e}", flush=True)
    for _ in range(args.warmup):
        for k in enc:
            enc[k].encode(texts)
            launch_only(k, texts)
    res = {k: [] for k in enc}
    host = {k: [] for k in enc}
    for _ in range(args.rounds):
        for k in enc:
            # encode() ends in .cpu(), so its return is the result
            res[k].append(timed(lambda: enc[k].encode(texts)))
            host[k].append(timed(lambda: launch_only(k, texts)))
    for k in enc:
        lines.append(
            f"| {name} | {k} | {statistics.median(res[k]):.3f} | "
            f"{min(res[k]):.3f} | {max(res[k]):.3f} | "
            f"{statistics.median(host[k]):.3f} | {min(host[k]):.3f} | "
            f"{max(host[k]):.3f} |")
    summary.append(
        f"{name}: torch/hip = "
        f"{statistics.median(res['torch']) / statistics.median(res['hip']):.2f}x "
        f"(result), slowest hip {max(res['hip']):.3f} ms vs fastest torch "
        f"{min(res['torch']):.3f} ms")
text = "\n".join(lines + [""] + summary)
print(text, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
