"""embedder.embed_many and its callers (CPU): one encoder call per batch when
the encoder runs its hip implementation, the per-text loop otherwise."""
import pytest

from room_amd.db import LockedDb
from room_amd.db import queries as q
from room_amd.memory import embedder, encoder
from room_amd.memory.vector_store import GpuVectorStore, MemoryService


@pytest.fixture(autouse=True)
def _clean_cache():
    embedder._EMBED_CACHE.clear()
    yield
    embedder._EMBED_CACHE.clear()


@pytest.fixture
def calls(monkeypatch):
    """encoder.encode_texts replaced by a counting fake (hash vectors)."""
    seen: list[list[str]] = []

    def fake(texts):
        seen.append(list(texts))
        return [embedder.embed_hash(t) for t in texts]

    monkeypatch.setattr(encoder, "encode_texts", fake)
    monkeypatch.setenv("ROOMAMD_EMBEDDER", "encoder")
    monkeypatch.delenv("ROOMAMD_ENCODER_IMPL", raising=False)
    return seen


def _svc(db):
    return MemoryService(LockedDb(db),
                         store=GpuVectorStore(capacity=200, device="cpu"))


def _pending(db, n):
    for i in range(n):
        q.create_entity(db, f"pending {i}", observations=[f"alpha words {i}"])


def test_hash_mode_equals_embed_loop(monkeypatch):
    monkeypatch.setenv("ROOMAMD_EMBEDDER", "hash")
    ts = ["deploy the service", "", "deploy the service", "garden notes"]
    assert embedder.embed_many(ts) == [embedder.embed(t) for t in ts]
    assert embedder.embed_many([]) == []


def test_hip_mode_one_call_with_the_misses(monkeypatch, calls):
    monkeypatch.setenv("ROOMAMD_ENCODER_IMPL", "hip")
    embedder.embed("t1")
    embedder.embed("t3")
    del calls[:]
    ts = ["t0", "t1", "t2", "t3", "t4"]
    out = embedder.embed_many(ts)
    assert calls == [["t0", "t2", "t4"]]
    assert out == [embedder.embed_hash(t) for t in ts]
    # everything is cached now: no further call, same vectors
    assert embedder.embed_many(ts) == out and len(calls) == 1
    assert embedder.embed("t2") == out[2] and len(calls) == 1
    # a text repeated inside one batch is encoded once
    del calls[:]
    assert embedder.embed_many(["n", "n", "t0"]) == [
        embedder.embed_hash("n"), embedder.embed_hash("n"), out[0]]
    assert calls == [["n"]]


def test_hip_mode_callers_batch(monkeypatch, calls, db):
    monkeypatch.setenv("ROOMAMD_ENCODER_IMPL", "hip")
    _pending(db, 7)
    svc = _svc(db)
    assert svc.index_pending() == 7
    assert len(calls) == 1 and len(calls[0]) == 7
    del calls[:]
    hits = svc.recall_many([None] * 4, ["alpha 1", "words 2", "alpha 3", "q 4"])
    assert len(hits) == 4
    assert calls == [["alpha 1", "words 2", "alpha 3", "q 4"]]


def test_default_impl_one_call_per_miss(monkeypatch, calls, db):
    monkeypatch.delenv("ROOMAMD_ENCODER_IMPL", raising=False)
    embedder.embed("t1")
    del calls[:]
    embedder.embed_many(["t0", "t1", "t2"])
    assert calls == [["t0"], ["t2"]]
    del calls[:]
    _pending(db, 7)
    svc = _svc(db)
    assert svc.index_pending() == 7
    assert len(calls) == 7 and all(len(c) == 1 for c in calls)
    del calls[:]
    svc.recall_many([None] * 4, ["alpha 1", "words 2", "alpha 3", "q 4"])
    assert calls == [["alpha 1"], ["words 2"], ["alpha 3"], ["q 4"]]


def test_impls_cache_apart(monkeypatch, calls):
    """The implementations agree to bf16 precision only: a vector cached
    under one is not served under the other."""
    embedder.embed("shared text")
    monkeypatch.setenv("ROOMAMD_ENCODER_IMPL", "hip")
    embedder.embed("shared text")
    assert calls == [["shared text"], ["shared text"]]


def test_hip_impl_needs_a_gpu_device():
    with pytest.raises(RuntimeError):
        encoder.MiniEncoder(device="cpu", impl="hip")


def test_impl_names(monkeypatch):
    with pytest.raises(ValueError):
        encoder.MiniEncoder(device="cpu", impl="triton")
    monkeypatch.setenv("ROOMAMD_ENCODER_IMPL", "hip")
    assert encoder.default_impl() == "hip"
    monkeypatch.setenv("ROOMAMD_ENCODER_IMPL", "fast")
    with pytest.raises(ValueError):
        encoder.default_impl()
    monkeypatch.delenv("ROOMAMD_ENCODER_IMPL")
    assert encoder.default_impl() == "torch"
