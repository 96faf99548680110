"""The engine with ROOMAMD_EXPERT_DTYPE=fp8 (tiny config): narrow and wide
decode on captured graphs, graph against eager token for token, and the
default mode left without fp8 tensors."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from room_amd.engine.llm import GenRequest, LocalEngine
from room_amd.models.qwen3_moe import Qwen3MoEConfig


def _tiny_engine():
    return LocalEngine(cfg=Qwen3MoEConfig.tiny(), kv_gb=1.0, max_seqs=32)


@pytest.fixture(scope="module")
def engine():
    mp = pytest.MonkeyPatch()
    mp.setenv("ROOMAMD_EXPERT_DTYPE", "fp8")
    eng = _tiny_engine()
    mp.undo()            # read once at construction
    yield eng
    eng.shutdown()


def _prompt(i, V=4096):
    """Request i's prompt: 20 + 7i distinct-ish ids (all contexts < 1024)."""
    return [(31 * i + 17 * j + 5) % V for j in range(20 + 7 * i)]


def _run_together(engine, jobs):
    """Every job active in the same decode block: the scheduler admits under
    engine._lock, so while the test holds it the requests queue up in order
    and one scheduler pass admits and prefills them all."""
    reqs = [GenRequest(**kw) for kw in jobs]
    with engine._lock:
        for r in reqs:
            engine._queue.put(r)
    for r in reqs:
        assert r.done.wait(120), "request did not finish"
        assert r.error is None, r.error
    return reqs


def _greedy(n, new):
    return [dict(prompt_tokens=_prompt(i), max_new_tokens=new,
                 temperature=0.0) for i in range(n)]


def test_engine_reports_fp8(engine):
    assert engine.expert_dtype == "fp8"
    assert engine.model.expert_dtype == "fp8"
    layer = engine.model.layers[0]
    assert layer.w13_q.dtype == torch.float8_e4m3fn
    assert layer.w2_s.dtype == torch.float32


def test_narrow_requests_finish_on_graphs(engine):
    before = dict(engine.stats)
    reqs = _run_together(engine, _greedy(5, 12))
    V = engine.cfg.vocab_size
    for r in reqs:
        assert len(r.out_tokens) == 12
        assert all(0 <= t < V for t in r.out_tokens)
    d = {k: engine.stats[k] - before[k] for k in before}
    assert d["decode_graph_steps"] > 0
    assert d["decode_wide_steps"] == 0
    assert not engine._graphs_broken


def test_wide_requests_run_wide_graph_steps(engine):
    before = dict(engine.stats)
    reqs = _run_together(engine, _greedy(12, 16))
    V = engine.cfg.vocab_size
    for r in reqs:
        assert len(r.out_tokens) == 16
        assert all(0 <= t < V for t in r.out_tokens)
    d = {k: engine.stats[k] - before[k] for k in before}
    assert d["decode_wide_steps"] > 0
    assert d["decode_graph_steps"] == d["decode_steps"], d
    assert not engine._wide_graphs_broken and not engine._graphs_broken


def test_graph_matches_eager_token_for_token(monkeypatch):
    # the fp8 wide path is deterministic and row-independent like its twin
    outs = []
    for no_graphs in ("0", "1"):
        monkeypatch.setenv("ROOMAMD_EXPERT_DTYPE", "fp8")
        monkeypatch.setenv("ROOMAMD_NO_GRAPHS", no_graphs)
        eng = _tiny_engine()
        try:
            assert eng.expert_dtype == "fp8"
            assert eng.graphs_enabled == (no_graphs == "0")
            reqs = _run_together(eng, _greedy(12, 24))
            steps = eng.stats["decode_steps"]
            assert eng.stats["decode_wide_steps"] == steps > 0
            assert eng.stats["decode_graph_steps"] == (
                steps if no_graphs == "0" else 0)
            outs.append([r.out_tokens for r in reqs])
        finally:
            eng.shutdown()
    for i, (a, b) in enumerate(zip(*outs)):
        assert len(a) == 24
        assert a == b, f"request {i}: graph {a} != eager {b}"


def test_default_engine_has_no_fp8_tensors(monkeypatch):
    monkeypatch.delenv("ROOMAMD_EXPERT_DTYPE", raising=False)
    eng = _tiny_engine()
    try:
        assert eng.expert_dtype == "bf16"
        assert eng.model.expert_dtype == "bf16"
        for layer in eng.model.layers:
            assert not hasattr(layer, "w13_q") and not hasattr(layer, "w2_q")
    finally:
        eng.shutdown()
