"""Wide decode (9..64 concurrent sequences) on the GPU: the model's wide
layer against the narrow one, the engine's captured multi-step graphs for
buckets above 8, graph against eager token for token, the kill switch, and
the narrow path left alone. Tiny configs; every context stays under 1024
tokens (the split-KV kernel's long-context defect, see PERF_NOTES, is not
this file's subject)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from room_amd import ops
from room_amd.engine.kv_cache import PagedKVCache
from room_amd.engine.llm import GenRequest, LocalEngine
from room_amd.models.qwen3_moe import Qwen3MoEConfig, Qwen3MoEModel

DEV = torch.device("cuda", 0)


# ------------------------------------------------------------------ model

def test_model_wide_matches_narrow_and_ignores_batch_mates():
    # every expert always selected: routing cannot flip on a rounding
    # difference, so wide and narrow logits differ continuously
    cfg = Qwen3MoEConfig(vocab_size=4096, hidden_size=512, num_layers=2,
                         num_q_heads=8, num_kv_heads=1, head_dim=128,
                         num_experts=8, num_experts_per_tok=8,
                         moe_intermediate_size=256, max_position=1024)
    model = Qwen3MoEModel(cfg, DEV, seed=7)
    nseq = 33
    cache = PagedKVCache(cfg.num_layers, cfg.num_kv_heads, cfg.head_dim,
                         nseq * 4 + 1, nseq, cfg.max_position // 16, DEV)
    g = torch.Generator().manual_seed(3)
    lens = [1, 40, 7, 16, 17, 33, 2, 25, 12, 31, 9, 38] + [
        int(v) for v in torch.randint(1, 41, (nseq - 12,), generator=g)]
    toks, seqs, pos, segments = [], [], [], []
    for s, n in enumerate(lens):
        assert cache.alloc_seq() == s
        cache.ensure_capacity(s, n + 1)
        segments.append((len(toks), n))
        toks += torch.randint(0, cfg.vocab_size, (n,), generator=g).tolist()
        seqs += [s] * n
        pos += list(range(n))
    i32 = dict(dtype=torch.int32, device=DEV)
    model.forward(torch.tensor(toks, device=DEV), torch.tensor(seqs, **i32),
                  torch.tensor(pos, **i32), cache.block_table, cache.kcaches,
                  cache.vcaches,
                  logits_rows=torch.zeros(0, dtype=torch.int64, device=DEV),
                  qtile_desc=ops.build_qtile_desc(segments, DEV))

    step_tok = torch.randint(0, cfg.vocab_size, (nseq,), generator=g).to(DEV)
    seq_t = torch.arange(nseq, **i32)
    pos_t = torch.tensor(lens, **i32)

    def step(rows):
        # each call rewrites the KV of position len before reading it, and
        # nothing older: every call starts from the same cache state
        return model.forward(step_tok[rows], seq_t[rows], pos_t[rows],
                             cache.block_table, cache.kcaches, cache.vcaches)

    wide12 = step(slice(0, 12))
    wide33 = step(slice(0, 33))
    narrow = torch.cat([step(slice(0, 6)), step(slice(6, 12))])
    assert wide12.shape == narrow.shape == (12, cfg.vocab_size)
    assert wide12.dtype == torch.float32
    diff = (wide12 - narrow).abs().max().item()
    print(f"wide vs narrow logits: max abs diff {diff:.3e}, "
          f"max |logit| {narrow.abs().max().item():.3f}")
    # the project's bound for a bf16 MoE chain; catches structural errors
    assert torch.allclose(wide12, narrow, atol=6e-2, rtol=6e-2), diff
    # a request's logits do not depend on who shares its batch
    assert torch.equal(wide33[:12], wide12)
    # and wide mode has no atomics: the same call gives the same bits
    assert torch.equal(step(slice(0, 12)), wide12)


# ----------------------------------------------------------------- engine

def _tiny_engine():
    return LocalEngine(cfg=Qwen3MoEConfig.tiny(), kv_gb=1.0, max_seqs=32)


@pytest.fixture(scope="module")
def engine():
    eng = _tiny_engine()
    yield eng
    eng.shutdown()


def _prompt(i, V=4096):
    """Request i's prompt: 20 + 7i distinct-ish ids (all contexts < 1024)."""
    return [(31 * i + 17 * j + 5) % V for j in range(20 + 7 * i)]


def _run_together(engine, jobs):
    """Make every job active in the same decode block by construction: the
    scheduler admits under engine._lock, so while the test holds it the
    first request waits at admission and the rest queue up behind it in
    order; on release one scheduler pass admits and prefills them all."""
    reqs = [GenRequest(**kw) for kw in jobs]
    with engine._lock:
        for r in reqs:
            engine._queue.put(r)
    for r in reqs:
        assert r.done.wait(120), "request did not finish"
        assert r.error is None, r.error
    return reqs


MIXED = [dict(temperature=0.0), dict(temperature=0.7, top_p=0.95, top_k=40),
         dict(temperature=1.0, top_p=0.9, top_k=64),
         dict(temperature=0.3, top_p=0.5, top_k=8),
         dict(temperature=1.3, top_k=2),
         dict(temperature=0.8, repetition_penalty=1.3, repeat_last_n=32),
         dict(temperature=0.0, presence_penalty=0.5, frequency_penalty=0.2)]


@pytest.mark.parametrize("n", [12, 16])     # a padded bucket, the exact one
def test_engine_wide_batches_run_on_graphs(engine, n):
    jobs = [dict(prompt_tokens=_prompt(i), max_new_tokens=16, seed=100 + i,
                 **MIXED[i % len(MIXED)]) for i in range(n)]
    before = dict(engine.stats)
    reqs = _run_together(engine, jobs)
    V = engine.cfg.vocab_size
    for r in reqs:
        assert len(r.out_tokens) == 16
        assert all(0 <= t < V for t in r.out_tokens)
    d = {k: engine.stats[k] - before[k] for k in before}
    assert d["decode_steps"] > 0
    assert d["decode_graph_steps"] == d["decode_steps"], d
    assert d["decode_wide_steps"] == d["decode_steps"], d
    assert (16, 32) in engine._graphs
    assert not engine._wide_graphs_broken and not engine._graphs_broken


def test_narrow_path_untouched(engine):
    jobs = [dict(prompt_tokens=_prompt(i), max_new_tokens=12, seed=i)
            for i in range(5)]
    before = dict(engine.stats)
    keys_before = set(engine._graphs)
    reqs = _run_together(engine, jobs)
    assert all(len(r.out_tokens) == 12 for r in reqs)
    assert engine.stats["decode_wide_steps"] == before["decode_wide_steps"]
    assert (engine.stats["decode_graph_steps"] - before["decode_graph_steps"]
            == engine.stats["decode_steps"] - before["decode_steps"] > 0)
    new = set(engine._graphs) - keys_before
    assert new <= {(b, 32) for b in range(1, 6)}, new


def test_graph_matches_eager_token_for_token():
    # wide mode is deterministic and row-independent, so K captured steps
    # with padded lanes give the tokens of K eager steps
    outs = []
    for graphs in (True, False):
        eng = _tiny_engine()
        try:
            eng.graphs_enabled = graphs
            jobs = [dict(prompt_tokens=_prompt(i), max_new_tokens=24,
                         temperature=0.0) for i in range(12)]
            reqs = _run_together(eng, jobs)
            steps = eng.stats["decode_steps"]
            assert eng.stats["decode_wide_steps"] == steps > 0
            assert eng.stats["decode_graph_steps"] == (steps if graphs else 0)
            outs.append([r.out_tokens for r in reqs])
        finally:
            eng.shutdown()
    for i, (a, b) in enumerate(zip(*outs)):
        assert len(a) == 24
        assert a == b, f"request {i}: graph {a} != eager {b}"


def test_kill_switch(monkeypatch):
    monkeypatch.setenv("ROOMAMD_WIDE_DECODE", "0")
    eng = _tiny_engine()
    try:
        assert eng.wide_rows is None and eng.model.wide_rows is None
        jobs = [dict(prompt_tokens=_prompt(i), max_new_tokens=8, seed=i)
                for i in range(12)]
        reqs = _run_together(eng, jobs)
        assert all(len(r.out_tokens) == 8 for r in reqs)
        assert eng.stats["decode_steps"] > 0
        assert eng.stats["decode_wide_steps"] == 0
        assert all(b <= 8 for b, _band in eng._graphs)
    finally:
        eng.shutdown()
