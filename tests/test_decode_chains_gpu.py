"""The decode step's short kernels after their serial chains were broken up:
split-KV merge (all loads in flight, branch-free), dense GEMV (W loads hoisted
for H/512 in {4, 8}, interleaved reductions), router top-k by rank counting,
MoE gate/up and down GEMVs (loads hoisted for the model's shapes). Each is
checked against the fp32 references of room_amd/ops/reference.py with the
tolerances tests/test_kernels_gpu.py uses. GPU-only."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from room_amd import ops
    from room_amd.ops import reference as ref
else:
    pytest.skip("no GPU", allow_module_level=True)

DEV = "cuda"


def bf16_close(a, b, atol=2e-2, rtol=2e-2):
    return torch.allclose(a.float(), b.float(), atol=atol, rtol=rtol)


# ------------------------------------------------------- split + merge
# span = ceil(len / splits) rounded up to 32 stays 32 for every length here,
# the range in which the split kernel scores each position once.
ATTN_LENS = [1, 32, 1023, 1024, 2048]


@pytest.fixture(scope="module")
def attn_case():
    """One cache and query set for every attention test; the fp32 reference is
    computed once. Row i attends to ATTN_LENS[i] tokens."""
    torch.manual_seed(40)
    B, Hq, Hk, D, BS = len(ATTN_LENS), 32, 4, 128, 16
    max_blocks = max(ATTN_LENS) // BS
    nb = B * max_blocks + 1
    kcache = torch.randn(nb, Hk, BS, D, dtype=torch.bfloat16, device=DEV)
    vcache = torch.randn(nb, Hk, BS, D, dtype=torch.bfloat16, device=DEV)
    bt = torch.arange(1, nb, dtype=torch.int32, device=DEV).reshape(B, max_blocks)
    q = torch.randn(B, Hq, D, dtype=torch.bfloat16, device=DEV)
    seq_ids = torch.arange(B, dtype=torch.int32, device=DEV)
    q_pos = torch.tensor([l - 1 for l in ATTN_LENS], dtype=torch.int32, device=DEV)
    scale = D ** -0.5
    expect = ref.paged_attention_ref(q, kcache, vcache, bt, seq_ids, q_pos, scale)
    return dict(q=q, kcache=kcache, vcache=vcache, bt=bt, seq_ids=seq_ids,
                q_pos=q_pos, scale=scale, expect=expect)


@pytest.mark.parametrize("splits,rows", [(32, 4), (64, 5)])
def test_split_merge_matches_ref(attn_case, splits, rows):
    """32 splits: lengths 1 (all splits but one empty), 32, 1023 (last split
    partial), 1024 (every split exactly one full chunk). 64 splits: the same
    plus 2048."""
    c = attn_case
    q = c["q"][:rows].contiguous()
    Hq, D = q.size(1), q.size(2)
    nsp = ops.attn_nsplits()
    # poison the partial buffers: the merge must read only what this launch's
    # split kernel wrote (its empty splits included)
    part = torch.full((rows, Hq, nsp, D), float("nan"), dtype=torch.float32,
                      device=DEV)
    part_ml = torch.full((rows, Hq, nsp, 2), float("nan"), dtype=torch.float32,
                         device=DEV)
    out = torch.empty_like(q)
    ops.paged_attention_split(out, q, c["kcache"], c["vcache"], c["bt"],
                              c["seq_ids"][:rows], c["q_pos"][:rows], part,
                              part_ml, c["scale"], splits=splits)
    err = (out.float() - c["expect"][:rows].float()).abs().max().item()
    print(f"splits={splits}: max abs err {err:.4g}")
    assert torch.isfinite(out.float()).all()
    assert bf16_close(out, c["expect"][:rows], atol=3e-2)


# ------------------------------------------------------------- dense GEMV
@pytest.mark.parametrize("H", [512, 1536, 2048, 4096])
def test_gemv_trip_counts_vs_matmul(H):
    """H/512 = 1, 3 (generic loop), 4 and 8 (hoisted loads); N=130 crosses the
    n >= N guard inside the last workgroup; bf16 and f32 outputs."""
    torch.manual_seed(41)
    for N in (130, 512):
        w = torch.randn(N, H, dtype=torch.bfloat16, device=DEV) * 0.05
        for B in (1, 5, 8):
            x = torch.randn(B, H, dtype=torch.bfloat16, device=DEV)
            expect = x.float() @ w.float().T
            # guard cells around y: a store past row B or column N shows up
            yf = torch.full((B + 1, N), 7.0, dtype=torch.float32, device=DEV)
            ops.gemv(yf[:B], x, w)
            assert torch.allclose(yf[:B], expect, atol=5e-2, rtol=5e-2), (B, N)
            assert (yf[B] == 7.0).all(), (B, N)
            y = torch.full((B + 1, N), 7.0, dtype=torch.bfloat16, device=DEV)
            ops.gemv(y[:B], x, w)
            assert bf16_close(y[:B], expect.to(torch.bfloat16), atol=5e-2,
                              rtol=5e-2), (B, N)
            assert (y[B] == 7.0).all(), (B, N)


def test_gemv_lds_staged_vs_matmul():
    """N >= 16384 at B >= 3 takes the LDS-staged kernel."""
    torch.manual_seed(42)
    B, H, N = 3, 512, 16388
    x = torch.randn(B, H, dtype=torch.bfloat16, device=DEV)
    w = torch.randn(N, H, dtype=torch.bfloat16, device=DEV) * 0.05
    expect = x.float() @ w.float().T
    yf = torch.empty(B, N, dtype=torch.float32, device=DEV)
    ops.gemv(yf, x, w)
    assert torch.allclose(yf, expect, atol=5e-2, rtol=5e-2)
    y = torch.empty(B, N, dtype=torch.bfloat16, device=DEV)
    ops.gemv(y, x, w)
    assert bf16_close(y, expect.to(torch.bfloat16), atol=5e-2, rtol=5e-2)


@pytest.mark.parametrize("B", [1, 2])
def test_gemv_addnorm_vs_reference(B):
    torch.manual_seed(43)
    H, N = 2048, 1028
    x = torch.randn(B, H, dtype=torch.bfloat16, device=DEV)
    gamma = torch.randn(H, dtype=torch.bfloat16, device=DEV)
    w = torch.randn(N, H, dtype=torch.bfloat16, device=DEV) * 0.05
    for delta in (torch.randn(B, H, dtype=torch.float32, device=DEV) * 0.1,
                  torch.randn(B, H, dtype=torch.bfloat16, device=DEV) * 0.1,
                  torch.empty(0, dtype=torch.float32, device=DEV)):
        if delta.numel():
            hb, res = ref.fused_add_rmsnorm_ref(x, delta, gamma)
        else:
            hb, res = ref.rmsnorm_ref(x, gamma), None
        expect = hb.float() @ w.float().T
        for dt in (torch.bfloat16, torch.float32):
            x_out = torch.empty_like(x)
            y = torch.empty(B, N, dtype=dt, device=DEV)
            ops.gemv_addnorm(y, x.clone(), delta, x_out, gamma, w, 1e-6)
            assert bf16_close(y, expect, atol=6e-2, rtol=6e-2)
            if res is not None:
                assert bf16_close(x_out, res)


# --------------------------------------------------------------- MoE GEMVs
@pytest.mark.parametrize("H,I", [(2048, 768), (1024, 256)])
def test_moe_gemv_path_shapes(H, I):
    """(2048, 768) takes the kernels with all loads hoisted, (1024, 256) their
    generic loops; T=3 tokens, the last pair rows end inside a workgroup."""
    torch.manual_seed(47)
    T, E, K = 3, 8, 4
    x = torch.randn(T, H, dtype=torch.bfloat16, device=DEV) * 0.5
    w13 = torch.randn(E, 2 * I, H, dtype=torch.bfloat16, device=DEV) * 0.02
    w2 = torch.randn(E, H, I, dtype=torch.bfloat16, device=DEV) * 0.02
    ids, w = ref.moe_router_ref(
        torch.randn(T, E, dtype=torch.float32, device=DEV), K)
    pair_token = torch.arange(T, device=DEV).repeat_interleave(K).int()
    pair_expert = ids.flatten().int()
    h = torch.empty(T * K, I, dtype=torch.bfloat16, device=DEV)
    out = torch.full((T, H), float("nan"), dtype=torch.float32, device=DEV)
    ops.moe_gemv_h(h, x, w13, pair_token, pair_expert, out_zero=out)
    assert (out == 0).all()               # the side job cleared the accumulator
    ops.moe_gemv_down(out, h, w2, w.flatten().float(), pair_token, pair_expert)
    expect = ref.moe_ref(x, w13, w2, ids, w)
    assert bf16_close(out, expect, atol=5e-2, rtol=5e-2)


# ----------------------------------------------------------------- router
def _stable_topk(logits, K):
    """ids of a stable descending sort: lowest index first among equals."""
    return torch.sort(-logits.float(), dim=-1, stable=True).indices[:, :K]


def _check_weights(ids, w, logits, K):
    ids_ref, w_ref = ref.moe_router_ref(logits, K)
    for t in range(ids.size(0)):
        assert w[t].sum().item() == pytest.approx(1.0, abs=1e-5)
        # both lists are in descending order of value and tied experts carry
        # equal weights, so the slots line up even where the ref broke a tie
        # differently
        for k in range(K):
            assert float(w[t, k]) == pytest.approx(float(w_ref[t, k]), abs=5e-3)


@pytest.mark.parametrize("T,E,H,K", [(1, 16, 512, 4), (5, 128, 2048, 8),
                                     (8, 128, 2048, 8)])
def test_router_gemv_topk_vs_reference(T, E, H, K):
    torch.manual_seed(44)
    x = torch.randn(T, H, dtype=torch.bfloat16, device=DEV) * 0.5
    wr = torch.randn(E, H, dtype=torch.bfloat16, device=DEV) * 0.05
    logits = x.float() @ wr.float().t()
    ids, w = ops.router_gemv_topk(x, wr, K)
    ids_ref, _ = ref.moe_router_ref(logits, K)
    for t in range(T):
        assert set(ids[t].tolist()) == set(ids_ref[t].tolist())
    _check_weights(ids, w, logits, K)


def _tie_columns(logits0, K):
    """Pick tie groups from one row of logits (ranked descending):
    a pair (2i, 2i+1) that copies a top-3 column, and two far columns that
    copy the column which then ranks K-1 from the top, so that three equal
    logits hold places K-2, K-1, K: two are picked, one is not.
    Returns [(source, [copies...]), ...] to apply in order."""
    order = torch.argsort(-logits0).tolist()
    src = order[2]
    pair = next(i for i in range(0, len(order), 2)
                if order.index(i) > 40 and order.index(i + 1) > 40)
    # with the pair raised to rank 2..4, the old rank-4 column ranks K-2 = 6
    a = order[K - 4]
    far = [c for c in order[50:] if c not in (pair, pair + 1)][:2]
    return [(src, [pair, pair + 1]), (a, far)], a, far


def test_router_gemv_topk_exact_ties():
    """Rows of the router weight that are exact copies give bit-equal logits:
    three copies straddle the K-th place, two sit in one lane's pair."""
    torch.manual_seed(45)
    T, E, H, K = 5, 128, 2048, 8
    x = torch.randn(T, H, dtype=torch.bfloat16, device=DEV) * 0.5
    wr = torch.randn(E, H, dtype=torch.bfloat16, device=DEV) * 0.05
    groups, a, far = _tie_columns((x.float() @ wr.float().t())[0], K)
    for s, copies in groups:
        wr[copies] = wr[s].clone()
    logits = x.float() @ wr.float().t()
    for s, copies in groups:              # equal by construction, not by luck
        logits[:, copies] = logits[:, s:s + 1].clone()
    expect = _stable_topk(logits, K)
    # the inputs do what the test is about: in row 0 the group of `a` has
    # members inside and outside the top K, and the decided places are not
    # within fp32 summation noise of each other
    members = sorted([a] + far)
    inside = [m for m in members if m in expect[0].tolist()]
    assert 0 < len(inside) < 3 and inside == members[:len(inside)]
    top = torch.sort(logits, dim=-1, descending=True).values[:, :K + 3]
    gaps = (top[:, :-1] - top[:, 1:])
    assert gaps[gaps > 0].min().item() > 1e-4

    ids, w = ops.router_gemv_topk(x, wr, K)
    assert ids.tolist() == expect.tolist()
    _check_weights(ids, w, logits, K)


def test_moe_router_exact_ties_t33():
    torch.manual_seed(46)
    T, E, K = 33, 128, 8
    logits = torch.randn(T, E, dtype=torch.float32, device=DEV) * 2
    groups, a, far = _tie_columns(logits[0], K)
    for s, copies in groups:
        logits[:, copies] = logits[:, s:s + 1].clone()
    expect = _stable_topk(logits, K)
    members = sorted([a] + far)
    inside = [m for m in members if m in expect[0].tolist()]
    assert 0 < len(inside) < 3 and inside == members[:len(inside)]

    ids, w = ops.moe_router(logits, K)
    assert ids.tolist() == expect.tolist()
    _check_weights(ids, w, logits, K)
