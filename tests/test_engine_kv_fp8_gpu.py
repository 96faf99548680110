"""The engine and the model with an fp8 KV cache (ROOMAMD_KV_DTYPE=fp8, tiny
config): pool sizing, narrow and wide decode on captured graphs, session
rollback onto fp8 rows, the layer-0 rows against the quantiser, and how far
the whole model's logits move."""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from room_amd import ops
from room_amd.engine.kv_cache import BLOCK_SIZE, PagedKVCache
from room_amd.engine.llm import GenRequest, LocalEngine
from room_amd.models.qwen3_moe import Qwen3MoEConfig, Qwen3MoEModel
from room_amd.ops.reference import quantize_kv_rows

DEV = "cuda"
KV_GB = 0.05


@pytest.fixture(scope="module")
def engine():
    mp = pytest.MonkeyPatch()
    mp.setenv("ROOMAMD_KV_DTYPE", "fp8")
    mp.delenv("ROOMAMD_NO_GRAPHS", raising=False)
    eng = LocalEngine(cfg=Qwen3MoEConfig.tiny(), kv_gb=KV_GB, max_seqs=32)
    mp.undo()            # read once at construction
    yield eng
    eng.shutdown()
    del eng
    gc.collect()
    torch.cuda.empty_cache()


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


def test_engine_reports_fp8_kv_and_sizes_the_pool(engine):
    cfg, cache = engine.cfg, engine.cache
    assert engine.kv_dtype == "fp8" and cache.kv_dtype == "fp8"
    assert engine.expert_dtype == "bf16"
    assert len(cache.kscales) == len(cache.vscales) == cfg.num_layers
    for rows, scales in zip(cache.kcaches + cache.vcaches,
                            cache.kscales + cache.vscales):
        assert rows.dtype == torch.float8_e4m3fn and rows.is_cuda
        assert scales.dtype == torch.float32
        assert scales.shape == rows.shape[:3]
    bpb = PagedKVCache.bytes_per_block(cfg.num_layers, cfg.num_kv_heads,
                                       cfg.head_dim, "fp8")
    assert bpb == cfg.num_layers * 2 * cfg.num_kv_heads * BLOCK_SIZE * 132
    assert cache.num_blocks == int(KV_GB * (1 << 30)) // bpb
    bf = PagedKVCache.bytes_per_block(cfg.num_layers, cfg.num_kv_heads,
                                      cfg.head_dim)
    assert cache.num_blocks > 1.9 * (int(KV_GB * (1 << 30)) // bf)


def test_narrow_requests_finish_on_graphs(engine):
    before = dict(engine.stats)
    reqs = _run_together(engine, _greedy(3, 24))
    V = engine.cfg.vocab_size
    for r in reqs:
        assert len(r.out_tokens) == 24
        assert all(0 <= t < V for t in r.out_tokens)
    d = {k: engine.stats[k] - before[k] for k in before}
    assert d["decode_graph_steps"] > 0
    assert not engine._graphs_broken


def test_wide_requests_run_wide_steps(engine):
    before = dict(engine.stats)
    reqs = _run_together(engine, _greedy(12, 16))
    V = engine.cfg.vocab_size
    for r in reqs:
        assert len(r.out_tokens) == 16
        assert all(0 <= t < V for t in r.out_tokens)
    d = {k: engine.stats[k] - before[k] for k in before}
    assert d["decode_wide_steps"] > 0
    assert not engine._wide_graphs_broken and not engine._graphs_broken


def test_session_rollback_onto_fp8_rows(engine):
    base = _prompt(9)
    r1 = engine.generate(base, max_new_tokens=4, temperature=0.0,
                         session_key="kv8")
    assert r1.prefill_tokens_run == len(base)
    ext = base + r1.out_tokens[:-1] + _prompt(2)
    r2 = engine.generate(ext, max_new_tokens=4, temperature=0.0,
                         session_key="kv8")
    assert len(r2.out_tokens) == 4
    assert all(0 <= t < engine.cfg.vocab_size for t in r2.out_tokens)
    # only the tail is prefilled: its rows and scales land on rolled-back rows
    assert 0 < r2.prefill_tokens_run < len(ext) / 2
    engine.release_session("kv8")


# ------------------------------------------------------------------- model

def _cache(cfg, kv_dtype, nblocks=32):
    cache = PagedKVCache(cfg.num_layers, cfg.num_kv_heads, cfg.head_dim,
                         nblocks, 2, cfg.max_position // BLOCK_SIZE, DEV,
                         kv_dtype=kv_dtype)
    assert cache.alloc_seq() == 0
    return cache


def _prefill(model, cache, toks):
    n = len(toks)
    cache.ensure_capacity(0, n)
    i32 = dict(dtype=torch.int32, device=DEV)
    return model.forward(
        torch.tensor(toks, device=DEV), torch.zeros(n, **i32),
        torch.arange(n, **i32), cache.block_table, cache.kcaches,
        cache.vcaches, logits_rows=torch.tensor([n - 1], device=DEV),
        qtile_desc=ops.build_qtile_desc([(0, n)], DEV),
        kscales=cache.kscales, vscales=cache.vscales)


def _step(model, cache, tok, pos):
    cache.ensure_capacity(0, pos + 1)
    i32 = dict(dtype=torch.int32, device=DEV)
    return model.forward(torch.tensor([tok], device=DEV), torch.zeros(1, **i32),
                         torch.tensor([pos], **i32), cache.block_table,
                         cache.kcaches, cache.vcaches, kscales=cache.kscales,
                         vscales=cache.vscales)


def test_layer0_rows_are_the_quantised_bf16_rows():
    """Layer 0's K and V rows depend only on the embedding, the first norm
    and the QKV GEMM, so the fp8 model's layer-0 bytes and scales are exactly
    quantize_kv_rows of the bf16 model's layer-0 rows."""
    cfg = Qwen3MoEConfig.tiny()
    g = torch.Generator().manual_seed(40)
    toks = torch.randint(0, cfg.vocab_size, (40,), generator=g).tolist()
    cb, c8 = _cache(cfg, "bf16"), _cache(cfg, "fp8")
    _prefill(Qwen3MoEModel(cfg, DEV, seed=5), cb, toks)
    _prefill(Qwen3MoEModel(cfg, DEV, seed=5), c8, toks)
    assert torch.equal(cb.block_table, c8.block_table)
    blocks = cb.block_table[0, :3].long()
    for bf, q8, sc in ((cb.kcaches[0], c8.kcaches[0], c8.kscales[0]),
                       (cb.vcaches[0], c8.vcaches[0], c8.vscales[0])):
        rows = bf[blocks].transpose(0, 1).reshape(cfg.num_kv_heads, 48, -1)[:, :40]
        got_q = q8.view(torch.uint8)[blocks].transpose(0, 1).reshape(
            cfg.num_kv_heads, 48, -1)[:, :40]
        got_s = sc[blocks].transpose(0, 1).reshape(cfg.num_kv_heads, 48)[:, :40]
        assert rows.float().abs().max() > 0
        want_q, want_s = quantize_kv_rows(rows)
        assert torch.equal(got_s, want_s)
        assert torch.equal(got_q, want_q.view(torch.uint8))


# worst 1 - cos measured on an MI355X over the three seeds below (per seed:
# 1.49e-3, 9.1e-4, 1.00e-3; the other rows lie between 4.0e-4 and 1.3e-3)
MEASURED_ONE_MINUS_COS = 1.493e-3


def test_whole_model_logits_stay_close():
    """1 - cos between the logits of the tiny model with an fp8 KV cache and
    with a bf16 one: after a 200-token prefill and after each of 8 decode
    steps on the same tokens, three seeds. The weights are random, so this
    bounds plumbing errors (a wrong row, a wrong scale, a missed layer); it
    is not a quality claim. Measured worst value: 1.493e-3
    (MEASURED_ONE_MINUS_COS); the bound is 10 x that, 1.5e-2, which covers
    seed-to-seed spread."""
    cfg = Qwen3MoEConfig.tiny()
    worst = 0.0
    for seed in (1, 2, 3):
        g = torch.Generator().manual_seed(seed)
        toks = torch.randint(0, cfg.vocab_size, (208,), generator=g).tolist()
        logits = {}
        for kv in ("bf16", "fp8"):
            model, cache = Qwen3MoEModel(cfg, DEV, seed=seed), _cache(cfg, kv)
            out = [_prefill(model, cache, toks[:200])]
            out += [_step(model, cache, toks[200 + i], 200 + i)
                    for i in range(8)]
            logits[kv] = torch.cat(out).double()
        cos = torch.nn.functional.cosine_similarity(logits["fp8"],
                                                    logits["bf16"], dim=-1)
        assert cos.shape == (9,)
        print(f"seed {seed}: 1 - cos per row {(1 - cos).tolist()}")
        worst = max(worst, float((1 - cos).max()))
    print(f"worst 1 - cos: {worst:.3e}")
    assert worst > 0, "the fp8 cache changed nothing: is it in use?"
    assert worst <= 10 * MEASURED_ONE_MINUS_COS
