"""Room scoping of the vector store and of MemoryService recall (CPU store:
the host logic and the scope rule are the same on every device).

Scope rule: a room sees rows tagged with its own id plus global rows
(entity room_id IS NULL, tag 0); room_id=None sees every row."""
import pytest
import torch

from room_amd.core import room
from room_amd.db import LockedDb
from room_amd.db import queries as q
from room_amd.memory import embedder
from room_amd.memory.vector_store import GpuVectorStore, MemoryService

SECRET = "rotate the production database password monthly"


@pytest.fixture(autouse=True)
def _hash_embedder(monkeypatch):
    """The scenarios are stated for the deterministic hash embedder; a GPU
    host would otherwise default to the (randomly initialised) encoder."""
    monkeypatch.setenv("ROOMAMD_EMBEDDER", "hash")


def _svc(db):
    return MemoryService(LockedDb(db),
                         store=GpuVectorStore(capacity=200, device="cpu"))


def _two_rooms(db):
    r1 = room.create_room(db, "scope-a", worker_model="stub")
    r2 = room.create_room(db, "scope-b", worker_model="stub")
    return r1["id"], r2["id"]


# ------------------------------------------------------------ MemoryService

def test_recall_does_not_leak_other_rooms(db):
    r1, r2 = _two_rooms(db)
    svc = _svc(db)
    svc.remember(r1, "a garden", "water the tomato plants every morning")
    svc.remember(r2, "b secret", SECRET)
    hits = svc.recall(r1, SECRET)
    assert hits, "room 1's own note must still be returned"
    assert all(h["room_id"] != r2 for h in hits), hits
    assert [h["name"] for h in hits] == ["a garden"]


def test_recall_not_crowded_out_by_other_room(db):
    r1, r2 = _two_rooms(db)
    svc = _svc(db)
    for i in range(25):
        svc.remember(r2, f"ledger entry {i}",
                     f"quarterly ledger reconciliation totals batch {i}")
    svc.remember(r1, "our ledger", "quarterly ledger reconciliation totals")
    hits = svc.recall(r1, "quarterly ledger reconciliation totals", limit=3)
    assert "our ledger" in [h["name"] for h in hits], hits
    assert all(h["room_id"] != r2 for h in hits), hits
    # the room's own note gets its cosine term (0.6·cos), not just FTS rank
    own = next(h for h in hits if h["name"] == "our ledger")
    assert own["score"] > 0.3


def test_global_entity_visible_from_both_rooms(db):
    r1, r2 = _two_rooms(db)
    svc = _svc(db)
    svc.remember(None, "house rules", "every room files expense reports weekly")
    svc.remember(r1, "r1 note", "alpha team standup at nine")
    svc.remember(r2, "r2 note", "beta team retro on friday")
    for rid in (r1, r2):
        hits = svc.recall(rid, "expense reports weekly", limit=3)
        assert hits[0]["name"] == "house rules", (rid, hits)


def test_unscoped_recall_sees_everything(db):
    r1, r2 = _two_rooms(db)
    svc = _svc(db)
    svc.remember(r1, "a garden", "water the tomato plants every morning")
    svc.remember(r2, "b secret", SECRET)
    names = [h["name"] for h in svc.recall(None, SECRET, limit=5)]
    assert names[0] == "b secret"
    names = [h["name"] for h in svc.recall(None, "tomato plants", limit=5)]
    assert names[0] == "a garden"


def test_index_pending_tags_rows(db):
    r1, r2 = _two_rooms(db)
    q.create_entity(db, "pending one", room_id=r1, observations=["alpha words"])
    q.create_entity(db, "pending two", room_id=r2, observations=["alpha words"])
    q.create_entity(db, "pending glob", observations=["alpha words"])
    svc = _svc(db)
    assert svc.index_pending() == 3
    got = {h["name"] for h in svc.recall(r1, "alpha words", limit=5)}
    assert got == {"pending one", "pending glob"}


def test_recall_many_equals_per_query_recall(db):
    r1, r2 = _two_rooms(db)
    svc = _svc(db)
    svc.remember(r1, "a garden", "water the tomato plants every morning")
    svc.remember(r1, "a deploy", "blue green deployment on the cluster")
    svc.remember(r2, "b secret", SECRET)
    svc.remember(r2, "b ledger", "quarterly ledger reconciliation totals")
    svc.remember(None, "house rules", "every room files expense reports weekly")
    texts = [SECRET, "tomato plants", "ledger totals", "expense reports",
             "deployment cluster", SECRET, "tomato plants", "ledger totals",
             "expense reports", "deployment cluster"]
    rooms = [r1, r1, r2, r2, None, r2, None, r1, None, r1]
    many = svc.recall_many(rooms, texts, limit=3)
    assert len(many) == len(texts)
    for rid, text, got in zip(rooms, texts, many):
        want = svc.recall(rid, text, limit=3)
        assert [h["id"] for h in got] == [h["id"] for h in want], (rid, text)
        for g, w in zip(got, want):
            assert g["score"] == pytest.approx(w["score"], abs=1e-5)
    with pytest.raises(ValueError):
        svc.recall_many([r1], ["x", "y"])


# ------------------------------------------------------------ store level

def _filled_store():
    """ids 1..30: id i lives in room (i % 3) + 1; ids 31..33 are global."""
    vs = GpuVectorStore(capacity=64, device="cpu")
    for i in range(1, 31):
        vs.upsert(i, embedder.embed(f"topic {i} subject matter w{i}x"),
                  room_id=(i % 3) + 1)
    for i in range(31, 34):
        vs.upsert(i, embedder.embed(f"topic {i} subject matter w{i}x"))
    return vs


def _room_of(i):
    return 0 if i > 30 else (i % 3) + 1


def test_store_tags_live_with_the_matrix():
    vs = _filled_store()
    assert vs.tags.dtype == torch.int32
    assert vs.tags.numel() == vs.capacity
    assert vs.tags.device == vs.mat.device
    assert vs.tags[:33].tolist() == [_room_of(i) for i in range(1, 34)]


def test_scoped_search_excludes_foreign_rows():
    vs = _filled_store()
    # id 4 lives in room 2: the exact text of id 4, searched from room 1
    qv = embedder.embed("topic 4 subject matter w4x")
    assert vs.search(qv, k=5)[0][0] == 4
    assert vs.search(qv, k=5, room_id=2)[0][0] == 4
    for rid in (1, 2, 3):
        hits = vs.search(qv, k=33, room_id=rid)
        assert len(hits) == 13            # 10 own rows + 3 global
        assert {_room_of(i) for i, _ in hits} == {rid, 0}
        scores = [s for _, s in hits]
        assert scores == sorted(scores, reverse=True)


def test_empty_scope_and_short_scope():
    vs = GpuVectorStore(capacity=16, device="cpu")
    assert vs.search(embedder.embed("x"), k=3, room_id=1) == []
    assert vs.search_batch([embedder.embed("x")], k=3, room_ids=[1]) == [[]]
    vs.upsert(1, embedder.embed("alpha"), room_id=1)
    vs.upsert(2, embedder.embed("beta"), room_id=1)
    vs.upsert(3, embedder.embed("gamma"), room_id=2)
    # a room with no rows and no global rows: nothing, not foreign rows
    assert vs.search(embedder.embed("alpha"), k=3, room_id=9) == []
    # fewer than k rows in scope: just those rows
    hits = vs.search(embedder.embed("alpha"), k=3, room_id=1)
    assert [i for i, _ in hits] == [1, 2]
    assert [i for i, _ in vs.search(embedder.embed("alpha"), k=3, room_id=2)] == [3]


def test_tag_survives_swap_delete():
    vs = GpuVectorStore(capacity=16, device="cpu")
    vs.upsert(1, embedder.embed("alpha one"), room_id=1)
    vs.upsert(2, embedder.embed("alpha two"), room_id=1)
    vs.upsert(3, embedder.embed("alpha three"), room_id=2)   # last row
    vs.remove(1)            # row 0 vacated, room 2's row 2 moves into it
    assert vs.size == 2
    assert vs.tags[:3].tolist() == [2, 1, 0]   # vacated slot cleared
    qv = embedder.embed("alpha")
    assert [i for i, _ in vs.search(qv, k=5, room_id=1)] == [2]
    assert [i for i, _ in vs.search(qv, k=5, room_id=2)] == [3]
    # the cleared slot is reused with the new row's own tag
    vs.upsert(4, embedder.embed("alpha four"), room_id=3)
    assert [i for i, _ in vs.search(qv, k=5, room_id=3)] == [4]
    assert sorted(i for i, _ in vs.search(qv, k=5)) == [2, 3, 4]


def test_reupsert_with_and_without_room():
    vs = GpuVectorStore(capacity=16, device="cpu")
    qv = embedder.embed("alpha")
    vs.upsert(1, qv, room_id=1)
    vs.upsert(1, embedder.embed("alpha again"))         # no room: tag kept
    assert vs.size == 1
    assert [i for i, _ in vs.search(qv, k=5, room_id=1)] == [1]
    assert vs.search(qv, k=5, room_id=2) == []
    vs.upsert(1, qv, room_id=2)                          # room given: retagged
    assert vs.search(qv, k=5, room_id=1) == []
    assert [i for i, _ in vs.search(qv, k=5, room_id=2)] == [1]
    vs.upsert(7, qv)                                     # new row, no room: global
    assert [i for i, _ in vs.search(qv, k=5, room_id=1)] == [7]
    # batch form follows the same rule
    vecs = torch.tensor([embedder.embed("beta"), embedder.embed("gamma"),
                         embedder.embed("delta")])
    vs.upsert_batch([1, 8, 9], vecs)                     # 1 keeps room 2
    vs.upsert_batch([8, 10], vecs[:2], room_ids=[3, None])
    assert [int(t) for t in vs.tags[:vs.size]] == [2, 0, 3, 0, 0]
    assert vs.ids[:vs.size].tolist() == [1, 7, 8, 9, 10]


def test_rebuild_from_db_restores_tags(db):
    r1, r2 = _two_rooms(db)
    ldb = LockedDb(db)
    svc = MemoryService(ldb, store=GpuVectorStore(capacity=32, device="cpu"))
    e1 = svc.remember(r1, "a garden", "water the tomato plants every morning")
    e2 = svc.remember(r2, "b secret", SECRET)
    e0 = svc.remember(None, "house rules", "expense reports weekly")
    vs2 = GpuVectorStore(capacity=32, device="cpu")
    with ldb as conn:
        assert vs2.rebuild_from_db(conn) == 3
    qv = embedder.embed(SECRET)
    assert {i for i, _ in vs2.search(qv, k=5, room_id=r1)} == {e1, e0}
    assert {i for i, _ in vs2.search(qv, k=5, room_id=r2)} == {e2, e0}
    assert {i for i, _ in vs2.search(qv, k=5)} == {e0, e1, e2}


def test_search_batch_equals_single_searches():
    vs = _filled_store()
    scopes = [None, 1, 2, 3, 1, None, 9, 2, 3, 3, 1]      # 11 → groups of 8 + 3
    qvs = [embedder.embed(f"topic {3 * j + 1} subject matter w{3 * j + 1}x")
           for j in range(len(scopes))]
    got = vs.search_batch(qvs, k=6, room_ids=scopes)
    assert len(got) == 11
    for qv, rid, g in zip(qvs, scopes, got):
        want = vs.search(qv, k=6, room_id=rid)
        assert [i for i, _ in g] == [i for i, _ in want], rid
        for (_, gs), (_, ws) in zip(g, want):
            assert gs == pytest.approx(ws, abs=1e-5)
    assert {i for i, _ in got[6]} == {31, 32, 33}          # room 9: globals only
    # a [Q, 384] tensor is accepted as well as a list of vectors
    assert vs.search_batch(torch.tensor(qvs), k=6, room_ids=scopes) == got
    with pytest.raises(ValueError):
        vs.search_batch(qvs, k=6, room_ids=[1])
