"""HBM-resident semantic vector store (BASELINE config 4).

The reference scans embedding BLOBs in SQLite with sqlite-vec's
vec_distance_cosine (src/shared/db-queries.ts:995-1010). Here the hot index
is a [capacity, 384] bf16 matrix resident in GPU HBM (10M rows = 7.4 GB of
the 288 GB HBM3E). SQLite's embeddings table remains the durable copy;
this store is rebuilt from it on boot.

Every row carries a room tag (int32, device-resident next to the matrix):
the entity's room id, or 0 for a global entity (room_id IS NULL). The scope
rule matches the durable host path (`e.room_id = ? OR e.room_id IS NULL`):

    search(q, k, room_id=R)    -> rows tagged R plus global rows
    search(q, k, room_id=None) -> every row

Unscoped single-query search runs the vs_topk HIP kernel (wave-per-row dot +
per-block top-k + merge). Scoped search and search_batch run vs_topk_scoped:
up to 8 queries share one pass over the matrix, each with its own scope, and
rows that no query in the batch admits are never read.

On CPU-only environments the store falls back to a torch CPU (masked) matmul
with identical semantics so the engine logic (and tests) run anywhere; the
GPU path is exercised by tests/test_memory_gpu.py and
tests/test_vector_scope_gpu.py.
"""
from __future__ import annotations

import threading

import torch

from ..core.constants import EMBEDDING_DIM

MAX_BATCH_QUERIES = 8   # vs_topk_scoped's compile-time query batch limit


class GpuVectorStore:
    def __init__(self, capacity: int = 1_000_000, device: str | None = None):
        self.device = torch.device(device or
                                   ("cuda" if torch.cuda.is_available() else "cpu"))
        self.capacity = capacity
        dtype = torch.bfloat16 if self.device.type == "cuda" else torch.float32
        self.mat = torch.zeros(capacity, EMBEDDING_DIM, dtype=dtype,
                               device=self.device)
        # room tag per row: room id, 0 = global entity
        self.tags = torch.zeros(capacity, dtype=torch.int32, device=self.device)
        self.ids = torch.zeros(capacity, dtype=torch.int64)  # host-side id map
        self.size = 0
        self._lock = threading.Lock()
        self._id_to_row: dict[int, int] = {}
        self._scope_cache: dict[tuple[int, ...], torch.Tensor] = {}

    def _place(self, entity_id: int, room_id: int | None) -> int:
        """Row of entity_id, appended if new (lock held). A new row takes tag
        `room_id or 0`; an existing row keeps its tag unless room_id is given."""
        row = self._id_to_row.get(entity_id)
        if row is None:
            if self.size >= self.capacity:
                raise RuntimeError("vector store full")
            row = self.size
            self.size += 1
            self._id_to_row[entity_id] = row
            self.ids[row] = entity_id
            self.tags[row] = int(room_id or 0)
        elif room_id is not None:
            self.tags[row] = int(room_id)
        return row

    def upsert(self, entity_id: int, vector: list[float] | torch.Tensor,
               room_id: int | None = None) -> int:
        v = torch.as_tensor(vector, dtype=torch.float32)
        v = torch.nn.functional.normalize(v, dim=-1)
        with self._lock:
            row = self._place(entity_id, room_id)
            self.mat[row] = v.to(self.mat.dtype).to(self.device)
        return row

    def upsert_batch(self, entity_ids: list[int], vectors: torch.Tensor,
                     room_ids: list[int | None] | None = None) -> None:
        v = torch.nn.functional.normalize(vectors.float(), dim=-1)
        with self._lock:
            for i, eid in enumerate(entity_ids):
                row = self._place(eid, room_ids[i] if room_ids is not None
                                  else None)
                self.mat[row] = v[i].to(self.mat.dtype).to(self.device)

    def remove(self, entity_id: int) -> None:
        with self._lock:
            row = self._id_to_row.pop(entity_id, None)
            if row is None:
                return
            last = self.size - 1
            if row != last:  # swap-delete
                self.mat[row] = self.mat[last]
                self.tags[row] = self.tags[last]
                last_id = int(self.ids[last])
                self.ids[row] = last_id
                self._id_to_row[last_id] = row
            self.mat[last].zero_()
            self.tags[last] = 0
            self.size = last

    def search(self, query: list[float] | torch.Tensor, k: int = 5,
               room_id: int | None = None) -> list[tuple[int, float]]:
        """Returns [(entity_id, cosine)] sorted desc. With a room_id only that
        room's rows and global rows are candidates; None searches every row."""
        if room_id is not None:
            return self.search_batch([query], k=k, room_ids=[room_id])[0]
        if self.size == 0:
            return []
        q = torch.as_tensor(query, dtype=torch.float32)
        q = torch.nn.functional.normalize(q, dim=-1).to(self.device)
        k = min(k, self.size)
        if self.device.type == "cuda":
            from .. import ops
            v, i = ops.vs_topk(self.mat[:self.size].contiguous(), q, k)
            rows = i.cpu().tolist()
            vals = v.cpu().tolist()
        else:
            scores = self.mat[:self.size] @ q
            vals_t, rows_t = scores.topk(k)
            rows, vals = rows_t.tolist(), vals_t.tolist()
        out = []
        for r, s in zip(rows, vals):
            if r < 0:
                continue
            out.append((int(self.ids[r]), float(s)))
        return out

    def _scopes(self, scopes: tuple[int, ...]) -> torch.Tensor:
        # rooms are few and recur every cycle: keep their scope vectors on the
        # device instead of paying a host→device copy per search
        t = self._scope_cache.get(scopes)
        if t is None:
            if len(self._scope_cache) >= 1024:
                self._scope_cache.clear()
            t = torch.tensor(scopes, dtype=torch.int32).to(self.device)
            self._scope_cache[scopes] = t
        return t

    def search_batch(self, queries, k: int = 5,
                     room_ids: list[int | None] | None = None
                     ) -> list[list[tuple[int, float]]]:
        """One result list per query, each as `search` would return it for
        (queries[i], k, room_ids[i]). Queries go to the device in groups of
        up to 8 that share one pass over the matrix and one host read-back."""
        if isinstance(queries, torch.Tensor):
            qs = queries.to(torch.float32).reshape(-1, EMBEDDING_DIM)
        else:
            qs = torch.stack([torch.as_tensor(x, dtype=torch.float32)
                              for x in queries]) if len(queries) else \
                torch.zeros(0, EMBEDDING_DIM)
        n = qs.size(0)
        if room_ids is None:
            room_ids = [None] * n
        if len(room_ids) != n:
            raise ValueError("room_ids must have one entry per query")
        if self.size == 0 or n == 0:
            return [[] for _ in range(n)]
        qs = torch.nn.functional.normalize(qs, dim=-1)
        k = min(k, self.size)
        out: list[list[tuple[int, float]]] = []
        for g in range(0, n, MAX_BATCH_QUERIES):
            scopes = self._scopes(tuple(
                -1 if r is None else int(r)
                for r in room_ids[g:g + MAX_BATCH_QUERIES]))
            qg = qs[g:g + MAX_BATCH_QUERIES].contiguous().to(self.device)
            if self.device.type == "cuda":
                from .. import ops
                v, i = ops.vs_topk_scoped(self.mat[:self.size],
                                          self.tags[:self.size], qg, scopes, k)
                # one read-back per group: indices ride along as f64 (exact
                # below 2^53, rows are < 2^31)
                both = torch.stack([v.double(), i.double()]).cpu()
                vals, rows = both[0].tolist(), both[1].long().tolist()
            else:
                scores = (self.mat[:self.size] @ qg.T).T          # [Q, size]
                tg = self.tags[:self.size].view(1, -1)
                sc = scopes.view(-1, 1)
                admit = (sc < 0) | (tg == 0) | (tg == sc)
                scores = scores.masked_fill(~admit, float("-inf"))
                vals_t, rows_t = scores.topk(k, dim=1)
                rows_t = rows_t.masked_fill(vals_t == float("-inf"), -1)
                rows, vals = rows_t.tolist(), vals_t.tolist()
            for rr, vv in zip(rows, vals):
                out.append([(int(self.ids[r]), float(s))
                            for r, s in zip(rr, vv) if r >= 0])
        return out

    def rebuild_from_db(self, db) -> int:
        """Load all durable embeddings, with each entity's room, from SQLite
        into HBM (boot path)."""
        from ..db import queries as q
        rows = q.all_embeddings_with_room(db)
        count = 0
        for r in rows:
            vec = q.blob_to_vector(r["vector"])
            if len(vec) == EMBEDDING_DIM:
                self.upsert(r["entity_id"], vec, room_id=r["room_id"] or 0)
                count += 1
        return count


class MemoryService:
    """Binds the durable SQLite memory to the GPU store + embedder: the
    remember/recall surface the agent tools and API use. Hybrid fusion stays
    host-side and identical to the reference (FTS RRF×0.4 + cosine×0.6).
    The semantic side is scoped like the FTS side: a room sees its own
    entities plus global ones; room_id=None sees everything."""

    def __init__(self, ldb, store: GpuVectorStore | None = None,
                 capacity: int = 1_000_000):
        from . import embedder
        self.ldb = ldb
        self.embedder = embedder
        self.store = store or GpuVectorStore(capacity=capacity)

    def embed(self, text: str) -> list[float]:
        return self.embedder.embed(text)

    def remember(self, room_id: int | None, name: str, content: str,
                 category: str | None = None, source: str = "agent") -> int:
        from ..db import queries as q
        with self.ldb as db:
            ent = q.get_entity_by_name(db, name, room_id)
            if ent is None:
                ent = q.create_entity(db, name, category=category, room_id=room_id)
            q.add_observation(db, ent["id"], content, source=source)
            vec = self.embedder.embed(f"{name} {content}")
            q.upsert_embedding(db, ent["id"], vec,
                               self.embedder.text_hash(content))
        # tag with the entity's own room (a name lookup with room_id=None can
        # resolve to an entity that lives in a room)
        self.store.upsert(ent["id"], vec, room_id=ent["room_id"] or 0)
        return ent["id"]

    def _swarm_merge(self, ctx, hits: list[dict], limit: int) -> list[dict]:
        payload = [{"name": h.get("name"), "category": h.get("category"),
                    "score": h.get("score"),
                    "observations": h.get("observations", [])[:5],
                    "shard": ctx.rank} for h in hits]
        merged = [h for shard in ctx.allgather_obj(payload) for h in shard]
        merged.sort(key=lambda h: -(h.get("score") or 0.0))
        # dedupe by name (same entity remembered on several shards)
        seen, out = set(), []
        for h in merged:
            if h["name"] in seen:
                continue
            seen.add(h["name"])
            out.append(h)
            if len(out) >= limit:
                break
        return out

    def recall(self, room_id: int | None, query: str, limit: int = 5) -> list[dict]:
        """Hybrid recall. In the multi-GPU swarm each rank owns a memory
        shard: every shard fuses its local FTS+cosine hits, then the fused
        top-k rides one RCCL all-gather and the global list is re-ranked by
        score — the topk-merge semantics of SURVEY §2c, integrated here so
        every agent recall is swarm-wide."""
        from ..db import queries as q
        qvec = self.embedder.embed(query)
        semantic = self.store.search(qvec, k=20, room_id=room_id)
        with self.ldb as db:
            hits = q.hybrid_search(db, query, qvec, limit=limit, room_id=room_id,
                                   semantic_hits=semantic)
        from ..parallel.swarm import get_swarm_context
        ctx = get_swarm_context()
        if ctx is not None and ctx.collective_safe:
            return self._swarm_merge(ctx, hits, limit)
        return hits

    def recall_many(self, room_ids: list[int | None], queries: list[str],
                    limit: int = 5) -> list[list[dict]]:
        """`recall` for several (room, query) pairs with one batched pass over
        the vector store: result[i] is what recall(room_ids[i], queries[i],
        limit) returns. Under a collective-safe swarm context the all-gather
        merge runs once per query, in order, so every rank must pass the same
        number of queries."""
        from ..db import queries as q
        if len(room_ids) != len(queries):
            raise ValueError("room_ids and queries must have the same length")
        qvecs = self.embedder.embed_many(list(queries))
        semantic = self.store.search_batch(qvecs, k=20, room_ids=list(room_ids))
        with self.ldb as db:
            fused = [q.hybrid_search(db, text, qvec, limit=limit, room_id=rid,
                                     semantic_hits=sem)
                     for rid, text, qvec, sem
                     in zip(room_ids, queries, qvecs, semantic)]
        from ..parallel.swarm import get_swarm_context
        ctx = get_swarm_context()
        if ctx is not None and ctx.collective_safe:
            return [self._swarm_merge(ctx, hits, limit) for hits in fused]
        return fused

    def index_pending(self, batch: int = 64) -> int:
        """Background indexing of unembedded entities (reference:
        embedding-indexer.ts — name + first 5 observations, 2000-char cap)."""
        from ..db import queries as q
        with self.ldb as db:
            pending = q.get_unembedded_entities(db, limit=batch)
            done = 0
            texts = []
            for ent in pending:
                obs = q.get_observations(db, ent["id"])[:5]
                texts.append((ent["name"] + " " +
                              " ".join(o["content"] for o in obs))[:2000])
            # one encoder call for the batch where the embedder batches
            vecs = self.embedder.embed_many(texts)
            for ent, text, vec in zip(pending, texts, vecs):
                q.upsert_embedding(db, ent["id"], vec,
                                   self.embedder.text_hash(text))
                try:
                    self.store.upsert(ent["id"], vec,
                                      room_id=ent["room_id"] or 0)
                except RuntimeError:
                    # GPU index at capacity: SQLite row is still embedded
                    # (durable + FTS-searchable); hot-index misses degrade
                    # recall to keyword-only for the overflow, not an error
                    pass
                done += 1
        return done
