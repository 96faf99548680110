"""Decode rate of five concurrent requests: one parameter set vs five.

Two batches, alternated round-robin in one process after a warm-up round of
each (which captures the decode graphs): `uniform` gives all five requests
temperature 0.7, `mixed` gives them 0.0 / 0.3 / 0.7 / 1.0 / 1.3. The rate is
the engine's own decode_tokens / decode_time over the round (host clock
around steps that end in a device sync), so prefill is left out. Also prints
how many of the round's decode steps ran in graph blocks where the engine
counts them. Uses only generate()'s long-standing arguments, so the same
file measures an older checkout for comparison. Prints one line per round and
a median / min / max summary; --out also writes it to a file.
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
ap.add_argument("--tokens", type=int, default=128)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--label", default="")
ap.add_argument("--out", default=None)
args = ap.parse_args()

assert torch.cuda.is_available(), "needs a GPU"
cfg = (Qwen3MoEConfig.tiny() if args.model_config == "tiny"
       else Qwen3MoEConfig.qwen3_coder_30b())
eng = LocalEngine(cfg=cfg, kv_gb=8.0, max_seqs=16)
TEMPS = {"uniform": [0.7] * 5, "mixed": [0.0, 0.3, 0.7, 1.0, 1.3]}
PROMPTS = [tok.encode(f"agent {i} observes the room, weighs the goals and "
                      "acts on the next task " * 12) for i in range(5)]


def one_round(temps):
    before = dict(eng.stats)
    errs = []

    def run(i):
        try:
            r = eng.generate(PROMPTS[i], max_new_tokens=args.tokens,
                             temperature=temps[i])
            assert len(r.out_tokens) == args.tokens
        except Exception as e:
            errs.append(str(e))

    ts = [threading.Thread(target=run, args=(i,)) for i in range(5)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(600)
    assert not errs, errs
    d = {k: eng.stats[k] - before[k] for k in before}
    return (d["decode_tokens"] / d["decode_time"], d["decode_steps"],
            d.get("decode_graph_steps"))


lines = []
try:
    for name, temps in TEMPS.items():       # warm-up: captures, first launches
        one_round(temps)
    rates = {name: [] for name in TEMPS}
    for rnd in range(args.rounds):
        for name, temps in TEMPS.items():
            rate, steps, gsteps = one_round(temps)
            rates[name].append(rate)
            lines.append(f"{args.label} round {rnd} {name}: {rate:.1f} tok/s, "
                         f"{steps} decode steps, graph steps {gsteps}")
            print(lines[-1], flush=True)
    for name, r in rates.items():
        lines.append(f"{args.label} {name}: median {statistics.median(r):.1f} "
                     f"min {min(r):.1f} max {max(r):.1f} tok/s "
                     f"({args.model_config}, 5 × {args.tokens} tokens, "
                     f"graphs captured {eng.stats['graphs_captured']})")
        print(lines[-1], flush=True)
finally:
    eng.shutdown()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
