"""Decode rate as the number of concurrent requests grows past eight.

For each B in --batches (default 8, 9, 12, 16, 24, 32, 48, 63), B concurrent
requests of --tokens new tokens each run as one batch: a warm-up round (which
captures whatever graphs the engine uses at that size), then --rounds timed
rounds. The rate is the engine's own decode_tokens / decode_time over the
round (host clock around steps that end in a device sync), so prefill is left
out; ms/step is decode_time / decode_steps. Also prints how many of the
round's decode steps ran in graph blocks and in wide mode where the engine
counts them. Uses only generate()'s long-standing arguments, so the same file
measures an older checkout for comparison (ROOMAMD_WIDE_DECODE=0 gives the
same routing on a new one). Prints one line per round and a median / min /
max summary per B; --out also writes it to a file.
"""
import argparse
import os
import statistics
import sys
import threading

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from room_amd.engine import tokenizer as tok  # noqa: E402
from room_amd.engine.llm import LocalEngine  # noqa: E402
from room_amd.models.qwen3_moe import Qwen3MoEConfig  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--model-config", choices=["30b", "tiny"], default="30b")
ap.add_argument("--batches", default="8,9,12,16,24,32,48,63")
ap.add_argument("--tokens", type=int, default=64)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--label", default="")
ap.add_argument("--out", default=None)
args = ap.parse_args()

assert torch.cuda.is_available(), "needs a GPU"
cfg = (Qwen3MoEConfig.tiny() if args.model_config == "tiny"
       else Qwen3MoEConfig.qwen3_coder_30b())
BATCHES = [int(b) for b in args.batches.split(",")]
eng = LocalEngine(cfg=cfg, kv_gb=8.0, max_seqs=64)
PROMPTS = [tok.encode(f"agent {i} observes the room, weighs the goals and "
                      "acts on the next task " * 4) for i in range(max(BATCHES))]


def one_round(nreq):
    before = dict(eng.stats)
    errs = []

    def run(i):
        try:
            r = eng.generate(PROMPTS[i], max_new_tokens=args.tokens,
                             temperature=0.7)
            assert len(r.out_tokens) == args.tokens
        except Exception as e:
            errs.append(str(e))

    ts = [threading.Thread(target=run, args=(i,)) for i in range(nreq)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(600)
    assert not errs, errs
    d = {k: eng.stats[k] - before[k] for k in before}
    return (d["decode_tokens"] / d["decode_time"],
            1e3 * d["decode_time"] / d["decode_steps"], d["decode_steps"],
            d.get("decode_graph_steps"), d.get("decode_wide_steps"))


lines = []
try:
    for nreq in BATCHES:
        one_round(nreq)                     # warm-up: captures, first launches
        rates, mss = [], []
        for rnd in range(args.rounds):
            rate, ms, steps, gsteps, wsteps = one_round(nreq)
            rates.append(rate)
            mss.append(ms)
            lines.append(f"{args.label} B={nreq} round {rnd}: {rate:.1f} tok/s, "
                         f"{ms:.2f} ms/step, {steps} decode steps, graph "
                         f"steps {gsteps}, wide steps {wsteps}")
            print(lines[-1], flush=True)
        lines.append(f"{args.label} B={nreq}: median {statistics.median(rates):.1f} "
                     f"min {min(rates):.1f} max {max(rates):.1f} tok/s, "
                     f"median {statistics.median(mss):.2f} ms/step "
                     f"({args.model_config}, {nreq} × {args.tokens} tokens)")
        print(lines[-1], flush=True)
finally:
    eng.shutdown()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
