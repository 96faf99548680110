"""vs_topk_scoped (room-scoped, batched cosine top-k) vs the plain fp32
reference, and the GPU store's scoped search vs the CPU store. GPU-only."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from room_amd import ops
    from room_amd.ops import reference as ref
else:
    pytest.skip("no GPU", allow_module_level=True)

from room_amd.memory import embedder
from room_amd.memory.vector_store import GpuVectorStore

DEV = "cuda"
NEG_INF = float("-inf")
SCOPE_MIX = [-1, 1, 2, 3, -1, 2, 1, 3]
TOL = 1e-2      # bf16 rows × f32 query, as test_vector_store_topk


def _problem(n, seed):
    g = torch.Generator().manual_seed(seed)
    mat = torch.nn.functional.normalize(
        torch.randn(n, 384, generator=g), dim=-1).to(torch.bfloat16)
    tags = torch.randint(0, 4, (n,), generator=g, dtype=torch.int32)
    queries = torch.nn.functional.normalize(
        torch.randn(8, 384, generator=g), dim=-1)
    return mat.to(DEV), tags.to(DEV), queries.to(DEV)


@pytest.fixture(scope="module")
def big():
    return _problem(5003, 30)


def _check(mat, tags, queries, scopes, k, nblocks=512):
    """Properties (a)-(e): admitted tags, no duplicates, value == reference
    score of the returned row, sorted and equal to the reference top-k
    values, valid count == min(k, rows in scope)."""
    sc = torch.tensor(scopes, dtype=torch.int32, device=DEV)
    v, i = ops.vs_topk_scoped(mat, tags, queries, sc, k, nblocks=nblocks)
    torch.cuda.synchronize()
    assert v.shape == i.shape == (len(scopes), k)
    assert v.dtype == torch.float32 and i.dtype == torch.int64
    v_ref, _ = ref.vs_topk_scoped_ref(mat, tags, queries, sc, k)
    full = (mat.float() @ queries.float().T).T.cpu()      # [Q, N] fp32 scores
    v, i, v_ref, tags_h = v.cpu(), i.cpu(), v_ref.cpu(), tags.cpu()
    for q, s in enumerate(scopes):
        valid = i[q] >= 0
        idx = i[q][valid]
        assert idx.numel() == 0 or int(idx.max()) < mat.size(0)
        t = tags_h[idx]
        if s >= 0:                                                    # (a)
            assert bool(((t == 0) | (t == s)).all()), (q, s)
        assert idx.unique().numel() == idx.numel(), (q, s)            # (b)
        assert torch.allclose(v[q][valid], full[q][idx], atol=TOL, rtol=0)  # (c)
        in_scope = mat.size(0) if s < 0 else int(((tags_h == 0) | (tags_h == s)).sum())
        nvalid = min(k, in_scope)
        assert int(valid.sum()) == nvalid, (q, s)                     # (e)
        assert bool(valid[:nvalid].all())
        assert bool((v[q][nvalid:] == NEG_INF).all())
        assert bool((v[q][:-1] >= v[q][1:]).all()), (q, s)            # (d)
        assert torch.allclose(v[q][:nvalid], v_ref[q][:nvalid], atol=TOL, rtol=0)
        assert bool((v_ref[q][nvalid:] == NEG_INF).all())
    return v, i


@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("nq", [1, 2, 3, 4, 5, 6, 7, 8])
def test_scoped_topk_vs_reference(big, nq, k):
    mat, tags, queries = big
    # rotate the scope mix so every Q sees scoped and unscoped queries
    scopes = (SCOPE_MIX[nq % 4:] + SCOPE_MIX)[:nq]
    _check(mat, tags, queries[:nq].contiguous(), scopes, k)


@pytest.mark.parametrize("nblocks", [1, 3])
def test_scoped_topk_more_rows_than_waves(big, nblocks):
    """5003 rows (79 tiles of 64) over nblocks*8 waves: every wave
    grid-strides several tiles, the last one ragged."""
    mat, tags, queries = big
    _check(mat, tags, queries[:5].contiguous(), [-1, 1, 1, 2, 3], 10,
           nblocks=nblocks)


@pytest.mark.parametrize("n", [40_000, 131_077])
def test_scoped_topk_many_blocks(n):
    """More than 64 blocks: the merge wave owns several lists per lane
    (157 blocks = a ragged third list; 131077 rows = all 512 blocks)."""
    mat, tags, queries = _problem(n, 33)
    _check(mat, tags, queries[:3].contiguous(), [2, -1, 3], 64)
    _check(mat, tags, queries[:1].contiguous(), [1], 20)


@pytest.mark.parametrize("n", [1, 70])
def test_scoped_topk_tiny_n_pads(n):
    mat, tags, queries = _problem(n, 31 + n)
    v, i = _check(mat, tags, queries[:4].contiguous(), [-1, 1, 2, 3], 64)
    assert bool((i[0][n:] == -1).all()) and bool((i[0][:n] >= 0).all())


def test_planted_rows(big):
    mat, tags, queries = big
    mat, tags = mat.clone(), tags.clone()
    # query q's vector planted once in each room: rows 100q+r carry tag r
    scopes = [1, 2, 3, 1, 2, 3, 1, 2]
    for q in range(8):
        for r in (1, 2, 3):
            mat[100 * q + r] = queries[q].to(torch.bfloat16)
            tags[100 * q + r] = r
    sc = torch.tensor(scopes, dtype=torch.int32, device=DEV)
    v, i = ops.vs_topk_scoped(mat, tags, queries, sc, 10)
    i = i.cpu()
    planted = {100 * q + r: r for q in range(8) for r in (1, 2, 3)}
    for q, s in enumerate(scopes):
        assert int(i[q][0]) == 100 * q + s
        for row in i[q].tolist():
            assert planted.get(row, s) == s, (q, row)


def test_empty_scope_leaves_other_queries_alone(big):
    mat, tags, queries = big
    tags = tags.clamp(min=1)                    # no global rows: scope 9 is empty
    qs = queries[:3].contiguous()
    sc = torch.tensor([1, 9, -1], dtype=torch.int32, device=DEV)
    v, i = ops.vs_topk_scoped(mat, tags, qs, sc, 10)
    assert bool((i[1] == -1).all()) and bool((v[1] == NEG_INF).all())
    for q, s in ((0, 1), (2, -1)):
        v1, i1 = ops.vs_topk_scoped(
            mat, tags, qs[q:q + 1].contiguous(),
            torch.tensor([s], dtype=torch.int32, device=DEV), 10)
        assert torch.allclose(v[q], v1[0], atol=1e-5, rtol=0)
    # a batch in which no query admits anything
    v, i = ops.vs_topk_scoped(mat, tags, qs[:2].contiguous(),
                              torch.tensor([9, 8], dtype=torch.int32, device=DEV), 5)
    assert bool((i == -1).all()) and bool((v == NEG_INF).all())


def test_mixed_batch_equals_singles(big):
    mat, tags, queries = big
    scopes = [-1, 1, 1, 2, 3]
    qs = queries[:5].contiguous()
    v, _ = ops.vs_topk_scoped(
        mat, tags, qs, torch.tensor(scopes, dtype=torch.int32, device=DEV), 20)
    for q, s in enumerate(scopes):
        v1, _ = ops.vs_topk_scoped(
            mat, tags, qs[q:q + 1].contiguous(),
            torch.tensor([s], dtype=torch.int32, device=DEV), 20)
        assert torch.allclose(v[q], v1[0], atol=1e-5, rtol=0), (q, s)


def test_argument_checks(big):
    mat, tags, queries = big
    sc = torch.tensor([-1], dtype=torch.int32, device=DEV)
    q1 = queries[:1].contiguous()
    with pytest.raises(RuntimeError):                       # wrong tag length
        ops.vs_topk_scoped(mat, tags[:-1].contiguous(), q1, sc, 5)
    with pytest.raises(RuntimeError):                       # wrong tag dtype
        ops.vs_topk_scoped(mat, tags.long(), q1, sc, 5)
    with pytest.raises(RuntimeError):                       # scopes != Q
        ops.vs_topk_scoped(mat, tags, queries[:2].contiguous(), sc, 5)
    with pytest.raises(RuntimeError):                       # K > 64
        ops.vs_topk_scoped(mat, tags, q1, sc, 65)
    with pytest.raises(RuntimeError):                       # Q > 8
        ops.vs_topk_scoped(mat, tags, torch.cat([queries, q1]),
                           torch.full((9,), -1, dtype=torch.int32, device=DEV), 5)


def test_gpu_store_scoped_matches_cpu():
    gpu = GpuVectorStore(capacity=2500, device="cuda")
    cpu = GpuVectorStore(capacity=2500, device="cpu")
    texts = [f"doc {i} unique subject {i} with marker w{i}x" for i in range(2000)]
    embed = embedder.embed_hash
    vecs = torch.tensor([embed(t) for t in texts])
    ids = list(range(1, 2001))
    rooms = [(i % 3) + 1 for i in range(2000)]              # doc i → room i%3+1
    gpu.upsert_batch(ids, vecs, room_ids=rooms)
    cpu.upsert_batch(ids, vecs, room_ids=rooms)
    assert gpu.tags.device.type == "cuda" and gpu.tags.dtype == torch.int32

    def same(g, c, top=None):
        assert g and len(g) == len(c)
        if top is not None:
            assert g[0][0] == c[0][0] == top
        # scores agree to bf16 precision even where near-ties reorder ids
        for (_, gv), (_, cv) in zip(g, c):
            assert abs(gv - cv) < 2e-2

    # doc 5 lives in room 3 (entity id 6): an exact hit from its own room
    qv = embed(texts[5])
    same(gpu.search(qv, k=10, room_id=3), cpu.search(qv, k=10, room_id=3), 6)
    # from room 1 the exact hit is out of scope; what is left are near-ties
    g1 = gpu.search(qv, k=10, room_id=1)
    assert all(rooms[eid - 1] == 1 for eid, _ in g1)
    same(g1, cpu.search(qv, k=10, room_id=1))
    # 11 queries (two device groups), mixed scopes; each query is the text of
    # a doc inside its own scope, so the top id is unambiguous
    scopes = [None, 1, 2, 3, 1, None, 2, 2, 3, 3, 1]
    docs = [30 * j + ((s or 1) - 1) for j, s in enumerate(scopes)]
    qvs = [embed(texts[d]) for d in docs]
    gb = gpu.search_batch(qvs, k=10, room_ids=scopes)
    cb = cpu.search_batch(qvs, k=10, room_ids=scopes)
    assert len(gb) == len(cb) == 11
    for d, s, g, c in zip(docs, scopes, gb, cb):
        if s is not None:
            assert rooms[d] == s
            assert all(rooms[eid - 1] == s for eid, _ in g)
        same(g, c, d + 1)
