"""expert_dtype="fp8" without the bf16 image (expert_image=False): the model
holds its expert weights only as block-scaled e4m3, prefill's grouped GEMM
reads them through moe_grouped_gemm128_fp8, and everything it computes has the
bits of the model that keeps the image.

Config A (8 experts, top-8) sends every token to every expert, so with more
than 128 tokens every expert fills a 128-row tile and ends in a ragged one.
Config B (Qwen3MoEConfig.tiny(), 16 experts, top-4) has live routing.

Memory is read from torch.cuda.memory_allocated around each build, in this
process. The three builds stay resident next to each other, so a build's peak
is taken relative to what was allocated when it began.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from room_amd import ops
from room_amd.engine.kv_cache import PagedKVCache
from room_amd.engine.llm import GenRequest, LocalEngine
from room_amd.models.qwen3_moe import Qwen3MoEConfig, Qwen3MoEModel

DEV = "cuda"
FP8 = torch.float8_e4m3fn


def _config(name):
    if name == "A":
        return Qwen3MoEConfig(vocab_size=4096, hidden_size=512, num_layers=2,
                              num_q_heads=8, num_kv_heads=1, head_dim=128,
                              num_experts=8, num_experts_per_tok=8,
                              moe_intermediate_size=256, max_position=1024)
    return Qwen3MoEConfig.tiny()


def _measured_build(cfg, **kw):
    # every build starts from an allocator without cached free blocks, so
    # none of them is handed the previous build's leftovers
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    req = torch.cuda.memory_stats().get("requested_bytes.all.current", 0)
    torch.cuda.reset_peak_memory_stats()
    model = Qwen3MoEModel(cfg, DEV, seed=7, **kw)
    torch.cuda.synchronize()
    req = torch.cuda.memory_stats().get("requested_bytes.all.current", 0) - req
    return model, dict(size=torch.cuda.memory_allocated() - base,
                       peak=torch.cuda.max_memory_allocated() - base,
                       requested=req)


@pytest.fixture(scope="module", params=["A", "B"])
def built(request):
    cfg = _config(request.param)
    image, mem_image = _measured_build(cfg, expert_dtype="fp8")
    lean, mem_lean = _measured_build(cfg, expert_dtype="fp8",
                                     expert_image=False)
    bf16, mem_bf16 = _measured_build(cfg)
    del bf16
    return dict(cfg=cfg, image=image, lean=lean,
                mem=dict(image=mem_image, lean=mem_lean, bf16=mem_bf16))


def test_lean_layers_hold_only_fp8(built):
    image, lean = built["image"], built["lean"]
    assert image.expert_image is True and lean.expert_image is False
    assert image.expert_dtype == lean.expert_dtype == "fp8"
    for li, ll in zip(image.layers, lean.layers):
        assert not hasattr(ll, "w13") and not hasattr(ll, "w2")
        assert hasattr(li, "w13") and hasattr(li, "w2")
        assert ll.w13_q.dtype == FP8 and ll.w2_q.dtype == FP8
        for name in ("w13_q", "w2_q"):
            assert torch.equal(getattr(ll, name).view(torch.uint8),
                               getattr(li, name).view(torch.uint8))
        for name in ("w13_s", "w2_s", "wqkv", "wo", "router_w"):
            assert torch.equal(getattr(ll, name), getattr(li, name))
    assert torch.equal(lean.lm_head, image.lm_head)
    assert lean.num_params() == image.num_params()


def test_bf16_without_image_is_refused():
    with pytest.raises(ValueError, match="expert_image"):
        Qwen3MoEModel(_config("B"), DEV, seed=7, expert_image=False)


def test_memory(built):
    """Image minus lean is at least 99 % of the image's 2 B per expert
    element, the lean model is smaller than the bf16 one, and the lean build
    peaks no higher than the image build.

    Measured on an MI355X. Config B: image 98 651 136 B, lean 48 319 488 B,
    bf16 70 595 584 B; saved 50 331 648 of 50 331 648 image bytes (100 %).
    Config A depends on what ran before in the process. After the rest of
    the GPU suite it passes. When this file runs alone (twice, same figures)
    it MISSES the first bound: image 33 317 888 B, lean 22 307 840 B, saved
    11 010 048 of 12 582 912 image bytes (87.5 %). The bytes the two builds
    *requested* (memory_stats()["requested_bytes.all.current"], also
    printed) differ by exactly 12 582 912 there too: every image byte is
    gone. What memory_allocated adds is the caching allocator's block
    rounding, which does not split a free block when less than about 1 MiB
    would remain: config A's 1 MiB tensors (a layer's w2_q, wo) can land in
    2 MiB blocks, and alone the lean build carries 2.36 MB of such rounding
    against the image build's 0.79 MB. At config B's sizes the rounding was
    the same in both builds. The bound is kept as it is. The other two
    bounds hold on both configs either way."""
    cfg, mem = built["cfg"], built["mem"]
    H, I = cfg.hidden_size, cfg.moe_intermediate_size
    expert_elems = cfg.num_layers * cfg.num_experts * 3 * I * H
    saved = mem["image"]["size"] - mem["lean"]["size"]
    print(f"requested bytes: {mem['image']['requested']} image, "
          f"{mem['lean']['requested']} lean, {mem['bf16']['requested']} bf16")
    print(f"model bytes: image {mem['image']['size']}, lean "
          f"{mem['lean']['size']}, bf16 {mem['bf16']['size']}; saved {saved} "
          f"of {2 * expert_elems} image bytes; build peaks: image "
          f"{mem['image']['peak']}, lean {mem['lean']['peak']}")
    assert saved >= 0.99 * 2 * expert_elems
    assert mem["lean"]["size"] < mem["bf16"]["size"]
    assert mem["lean"]["peak"] <= mem["image"]["peak"]


def _packed_prefill(cfg):
    """The ragged segments of test_model_fp8_matches_bf16_image_model."""
    nseq = 33
    g = torch.Generator().manual_seed(3)
    lens = [1, 40, 7, 16, 17, 33, 2, 25, 12, 31, 9, 38] + [
        int(v) for v in torch.randint(1, 41, (nseq - 12,), generator=g)]
    toks, seqs, pos, segments = [], [], [], []
    for sq, n in enumerate(lens):
        segments.append((len(toks), n))
        toks += torch.randint(0, cfg.vocab_size, (n,), generator=g).tolist()
        seqs += [sq] * n
        pos += list(range(n))
    step_tok = torch.randint(0, cfg.vocab_size, (nseq,), generator=g)
    return lens, toks, seqs, pos, segments, step_tok


def test_forwards_are_bit_equal(built):
    cfg, image, lean = built["cfg"], built["image"], built["lean"]
    lens, toks, seqs, pos, segments, step_tok = _packed_prefill(cfg)
    nseq, T = len(lens), len(toks)
    # every expert of config A gets T rows: full tiles and a ragged one
    assert T > 128 * cfg.num_experts // cfg.num_experts_per_tok and T % 128
    i32 = dict(dtype=torch.int32, device=DEV)
    last_rows = torch.tensor([r0 + n - 1 for r0, n in segments], device=DEV)
    step_tok = step_tok.to(DEV)
    seq_t = torch.arange(nseq, **i32)
    pos_t = torch.tensor(lens, **i32)

    def run(model):
        cache = PagedKVCache(cfg.num_layers, cfg.num_kv_heads, cfg.head_dim,
                             nseq * 4 + 1, nseq, cfg.max_position // 16, DEV)
        for sq, n in enumerate(lens):
            assert cache.alloc_seq() == sq
            cache.ensure_capacity(sq, n + 1)
        logits = model.forward(
            torch.tensor(toks, device=DEV), torch.tensor(seqs, **i32),
            torch.tensor(pos, **i32), cache.block_table, cache.kcaches,
            cache.vcaches, logits_rows=last_rows,
            qtile_desc=ops.build_qtile_desc(segments, DEV))
        kv = [t.clone() for t in cache.kcaches + cache.vcaches]
        # each step rewrites the KV of position len before reading it, and
        # nothing older: both start from the prefill's cache state
        steps = [model.forward(step_tok[:n], seq_t[:n], pos_t[:n],
                               cache.block_table, cache.kcaches,
                               cache.vcaches) for n in (5, 12)]
        return logits, kv, steps

    want_logits, want_kv, want_steps = run(image)
    got_logits, got_kv, got_steps = run(lean)
    assert want_logits.shape == (nseq, cfg.vocab_size)
    assert not torch.isnan(want_logits).any() and want_logits.abs().max() > 0
    assert any(t.any() for t in want_kv)
    assert torch.equal(got_logits, want_logits)
    for a, b in zip(got_kv, want_kv):
        assert torch.equal(a, b)
    for name, a, b in zip(("narrow T=5", "wide T=12"), got_steps, want_steps):
        assert a.shape[0] == int(name.split("=")[1])
        diff = (a - b).abs().max().item()
        print(f"lean vs image logits, {name}: max abs diff {diff:.3e}")
        assert torch.equal(a, b), name


# ------------------------------------------------------------------- engine

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


def _fp8_engine(monkeypatch, image):
    monkeypatch.setenv("ROOMAMD_EXPERT_DTYPE", "fp8")
    monkeypatch.setenv("ROOMAMD_EXPERT_IMAGE", image)
    monkeypatch.setenv("ROOMAMD_NO_GRAPHS", "1")
    monkeypatch.delenv("ROOMAMD_PREFILL_GRAPHS", raising=False)
    return LocalEngine(cfg=Qwen3MoEConfig.tiny(), kv_gb=1.0, max_seqs=32)


def test_engine_without_image_matches_engine_with_it(monkeypatch):
    outs = {}
    for image in ("0", "1"):
        eng = _fp8_engine(monkeypatch, image)
        try:
            assert eng.expert_dtype == "fp8"
            assert eng.expert_image is (image == "1")
            assert eng.model.expert_image is eng.expert_image
            assert not eng.prefill_graphs_enabled and not eng.graphs_enabled
            V = eng.cfg.vocab_size
            if image == "0":
                assert not hasattr(eng.model.layers[0], "w13")
                for r in _run_together(eng, _greedy(5, 12)):
                    assert len(r.out_tokens) == 12
                    assert all(0 <= t < V for t in r.out_tokens)
            before = dict(eng.stats)
            reqs = _run_together(eng, _greedy(12, 16))
            d = {k: eng.stats[k] - before[k] for k in before}
            assert d["decode_wide_steps"] == d["decode_steps"] > 0, d
            for r in reqs:
                assert len(r.out_tokens) == 16
                assert all(0 <= t < V for t in r.out_tokens)
            outs[image] = [r.out_tokens for r in reqs]
        finally:
            eng.shutdown()
    for i, (a, b) in enumerate(zip(outs["0"], outs["1"])):
        assert a == b, f"request {i}: lean {a} != image {b}"


def test_engine_refuses_image_off_with_bf16(monkeypatch):
    monkeypatch.delenv("ROOMAMD_EXPERT_DTYPE", raising=False)
    monkeypatch.setenv("ROOMAMD_EXPERT_IMAGE", "0")
    with pytest.raises(ValueError, match="ROOMAMD_EXPERT_IMAGE"):
        LocalEngine(cfg=Qwen3MoEConfig.tiny(), kv_gb=1.0, max_seqs=32)
