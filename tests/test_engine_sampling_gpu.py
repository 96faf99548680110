"""Per-request sampling through the engine on the GPU (tiny Qwen3-MoE config):
mixed parameters stay on the multi-step decode graphs, and penalties reach
both the first token after prefill and the captured decode loop.

No test here compares two runs with one seed: logits differ in their last
bits from run to run (atomic accumulation), so seed determinism is shown at
the kernel level in test_sampling_rows_gpu.py."""
import threading

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from room_amd.engine import tokenizer as tok
from room_amd.engine.llm import LocalEngine
from room_amd.models.qwen3_moe import Qwen3MoEConfig


@pytest.fixture(scope="module")
def engine():
    eng = LocalEngine(cfg=Qwen3MoEConfig.tiny(), kv_gb=2.0, max_seqs=16)
    yield eng
    eng.shutdown()


def _run_all(engine, jobs):
    """Start one generate() per job dict concurrently; returns the requests."""
    results, errors = {}, []

    def run(i, kw):
        try:
            results[i] = engine.generate(**kw)
        except Exception as e:  # pragma: no cover - surfaced below
            errors.append(f"{i}: {e}")

    threads = [threading.Thread(target=run, args=(i, kw))
               for i, kw in enumerate(jobs)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    assert not errors, errors
    assert len(results) == len(jobs)
    return [results[i] for i in range(len(jobs))]


def test_mixed_parameters_stay_on_graphs(engine):
    params = [(0.0, 1.0, 40), (0.7, 0.95, 40), (1.0, 0.9, 64), (0.3, 0.5, 8),
              (1.3, 1.0, 2)]
    jobs = [dict(prompt_tokens=tok.encode(f"agent {i} reports to the room " * 6),
                 max_new_tokens=24, temperature=t, top_p=p, top_k=k)
            for i, (t, p, k) in enumerate(params)]
    before = dict(engine.stats)
    keys_before = set(engine._graphs)
    reqs = _run_all(engine, jobs)
    assert all(len(r.out_tokens) == 24 for r in reqs)
    V = engine.cfg.vocab_size
    assert all(0 <= t < V for r in reqs for t in r.out_tokens)
    steps = engine.stats["decode_steps"] - before["decode_steps"]
    gsteps = engine.stats["decode_graph_steps"] - before["decode_graph_steps"]
    assert steps > 0 and gsteps == steps, (steps, gsteps)
    # one graph per (bucket, band) pair used: every key is such a pair (at
    # most buckets 1..5 in the short band) and captures grew by the new pairs
    assert all(len(key) == 2 for key in engine._graphs)
    new_pairs = set(engine._graphs) - keys_before
    assert new_pairs <= {(b, 32) for b in range(1, 6)}, new_pairs
    assert (engine.stats["graphs_captured"] - before["graphs_captured"]
            <= len(new_pairs))


def test_presence_penalty_reaches_prefill_and_decode_loop(engine):
    V = engine.cfg.vocab_size
    prompt = [(37 * j + 11) % V for j in range(100)]      # 100 distinct ids
    assert len(set(prompt)) == 100
    before = dict(engine.stats)
    r = engine.generate(prompt, max_new_tokens=48, temperature=0.0,
                        presence_penalty=1e3, repeat_last_n=64)
    out = r.out_tokens
    assert len(out) == 48
    assert len(set(out)) == 48, "a token repeated inside its own window"
    stream = prompt + out
    for i, t in enumerate(out):
        at = len(prompt) + i
        assert t not in stream[at - 64:at], (i, t)
    gsteps = engine.stats["decode_graph_steps"] - before["decode_graph_steps"]
    assert gsteps == engine.stats["decode_steps"] - before["decode_steps"] == 47


def test_top_k_one_at_temperature_one_next_to_default(engine):
    jobs = [dict(prompt_tokens=tok.encode("the clerk sums up the day " * 5),
                 max_new_tokens=12, temperature=1.0, top_k=1),
            dict(prompt_tokens=tok.encode("the queen plans the week " * 5),
                 max_new_tokens=12)]
    reqs = _run_all(engine, jobs)
    V = engine.cfg.vocab_size
    for r in reqs:
        assert len(r.out_tokens) == 12
        assert all(0 <= t < V for t in r.out_tokens)
