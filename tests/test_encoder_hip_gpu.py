"""MiniEncoder(impl="hip"): the bf16 forward on the project's HIP kernels
against the fp32 reference implementation with the same weights, its batch
invariance, retrieval quality, and the batched memory-service callers."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from room_amd.memory import embedder
from room_amd.memory.encoder import MiniEncoder

LONG = " ".join(f"deploying{i} servers" for i in range(35))    # 70 words
TEXTS = [
    "deploy the service to production",
    "benchmark results for matrix kernels",
    "a completely unrelated gardening note",
    "x",                                          # one piece
    "",                                           # empty: the <empty> piece
    LONG,                                         # truncates at 128 pieces
    "the deployment pipeline failed on the server",
    "server deployment pipeline failure",
]
CORPUS = [
    "deploy the web server to production now",     # target
    "benchmark results for the matrix kernels",
    "quarterly financial report draft two",
    "notes about the garden watering schedule",
    "refactor database query layer for speed",
]
QUERIES = [
    "production web server deployment",
    "deploying servers into production",
]


@pytest.fixture(scope="module")
def hip():
    return MiniEncoder(device="cuda", impl="hip")


@pytest.fixture(scope="module")
def cpu():
    return MiniEncoder(device="cpu")


def test_hip_matches_fp32_reference(hip, cpu):
    """Bound: a CPU emulation of this pipeline (bf16 weights, bf16 rounding at
    every kernel boundary, bf16 residual, f32 accumulation) gave a largest
    1 - cos of 3.9e-5 over these text shapes; 5x that for accumulation order
    and exp/erf differences. Per-component differences (emulation: up to
    1.6e-3) are printed, not asserted."""
    from room_amd.memory.encoder import tokenize
    assert len(LONG.split()) == 70 and len(tokenize(LONG)) == 128
    got = hip.encode(TEXTS)
    want = cpu.encode(TEXTS)
    assert got.shape == want.shape == (len(TEXTS), 384)
    assert got.dtype == torch.float32 and got.device.type == "cpu"
    one_minus_cos = 1.0 - (got.double() * want.double()).sum(-1) / (
        got.double().norm(dim=-1) * want.double().norm(dim=-1))
    print(f"hip vs fp32 reference: max 1-cos {float(one_minus_cos.max()):.3e}, "
          f"max |component diff| {float((got - want).abs().max()):.3e}")
    for row in got:
        assert abs(float(row.norm()) - 1.0) < 1e-3
    assert float(one_minus_cos.max()) <= 2e-4, one_minus_cos.tolist()


def test_hip_batch_invariance(hip):
    texts = [
        "x", "", "deploy the service", LONG,
        "benchmark results for matrix kernels on the new machine",
        "a completely unrelated gardening note about tomatoes and basil",
        " ".join(f"word{i}" for i in range(16)),
        " ".join(f"token{i}" for i in range(17)),
        "server deployment pipeline failure",
        " ".join(f"piece{i}" for i in range(40)),
    ]
    fwd = hip.encode(texts)
    rev = hip.encode(list(reversed(texts)))
    for i, t in enumerate(texts):
        alone = hip.encode([t])[0]
        assert torch.equal(alone, fwd[i]), i
        assert torch.equal(alone, rev[len(texts) - 1 - i]), i


def test_hip_concurrent_encode(hip):
    """No scratch shared between calls: two threads encoding at once get the
    bits of the serial calls."""
    import threading
    batches = [TEXTS, list(reversed(CORPUS)) + QUERIES]
    want = [hip.encode(b) for b in batches]
    got = [[], []]

    def work(i):
        for _ in range(8):
            got[i].append(hip.encode(batches[i]))

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for i in range(2):
        assert len(got[i]) == 8
        for g in got[i]:
            assert torch.equal(g, want[i]), i


def test_hip_retrieval_quality(hip, cpu):
    def cos(a, b):
        return sum(x * y for x, y in zip(a, b))

    cvecs_e = hip.encode(CORPUS).tolist()
    cvecs_t = cpu.encode(CORPUS).tolist()
    cvecs_h = [embedder.embed_hash(t) for t in CORPUS]
    for q in QUERIES:
        qe = hip.encode([q]).tolist()[0]
        qt = cpu.encode([q]).tolist()[0]
        qh = embedder.embed_hash(q)
        scores_e = [cos(qe, v) for v in cvecs_e]
        scores_t = [cos(qt, v) for v in cvecs_t]
        scores_h = [cos(qh, v) for v in cvecs_h]
        assert max(range(5), key=lambda i: scores_e[i]) == 0, (q, scores_e)
        margin_e = scores_e[0] - max(scores_e[1:])
        margin_h = scores_h[0] - max(scores_h[1:])
        assert margin_e > margin_h, (q, margin_e, margin_h)
        rank = lambda s: sorted(range(5), key=lambda i: -s[i])   # noqa: E731
        assert rank(scores_e) == rank(scores_t), (q, scores_e, scores_t)


def test_store_recall_many_equals_recall(monkeypatch):
    """12 remembers, then recall_many over 9 (room, query) pairs (one packed
    encoder call) returns what nine recall calls (one text each) return."""
    from room_amd.core import room
    from room_amd.db import LockedDb, init_test_db
    from room_amd.memory.vector_store import GpuVectorStore, MemoryService
    monkeypatch.setenv("ROOMAMD_EMBEDDER", "encoder")
    monkeypatch.setenv("ROOMAMD_ENCODER_IMPL", "hip")
    embedder._EMBED_CACHE.clear()
    conn = init_test_db()
    try:
        r1 = room.create_room(conn, "enc-a", worker_model="stub")["id"]
        r2 = room.create_room(conn, "enc-b", worker_model="stub")["id"]
        svc = MemoryService(LockedDb(conn),
                            store=GpuVectorStore(capacity=100, device="cuda"))
        notes = [
            (r1, "a garden", "water the tomato plants every morning"),
            (r1, "a deploy", "blue green deployment on the cluster"),
            (r1, "a bench", "kernel benchmark numbers for mfma"),
            (r1, "a budget", "quarterly budget review with finance"),
            (r2, "b secret", "rotate the production database password monthly"),
            (r2, "b ledger", "quarterly ledger reconciliation totals"),
            (r2, "b deploy", "production web server deployment steps"),
            (r2, "b garden", "watering schedule for the garden"),
            (None, "house rules", "every room files expense reports weekly"),
            (None, "style guide", "write commit messages in plain words"),
            (None, "oncall", "the oncall engineer restarts failed servers"),
            (None, "lunch", "the canteen serves soup on thursdays"),
        ]
        for rid, name, content in notes:
            svc.remember(rid, name, content)
        rooms = [r1, r1, r2, r2, None, None, r1, r2, None]
        texts = ["tomato plants", "deploying to the cluster",
                 "ledger totals", "database password rotation",
                 "expense reports", "restarting servers",
                 "expense reports", "garden watering", "tomato plants"]
        many = svc.recall_many(rooms, texts, limit=3)
        assert len(many) == 9 and all(many)
        embedder._EMBED_CACHE.clear()       # recall must embed each text alone
        for rid, text, got in zip(rooms, texts, many):
            want = svc.recall(rid, text, limit=3)
            assert [h["id"] for h in got] == [h["id"] for h in want], (rid, text)
            for g, w in zip(got, want):
                assert g["score"] == pytest.approx(w["score"], abs=1e-5)
    finally:
        conn.close()
        embedder._EMBED_CACHE.clear()
