"""The prefill MoE chain at its tile edges: moe_build_desc ->
moe_grouped_gemm128 -> silu_mul -> moe_grouped_gemm128 -> moe_combine_gather,
and dense_grouped_gemm (the same kernel with one expert) as the model's
capture-safe dense projection.

The GEMM tiles 128 pair rows by 64 output columns; an expert's last tile is
ragged and guarded by `r < msize`. The cases put experts at exactly 0, 1,
127, 128, 129 and 257 rows, empty experts first, between busy ones and last,
N at one, two and three n-tiles and K at one and four k-steps.

Exact cases take x and w from {-1, 0, 1} with K <= 256: every dot product is
an integer of magnitude at most 256, which f32 accumulation and the bf16
output hold exactly, so the output must `torch.equal` the integer matmul
whatever the summation order, and every pair row is compared. The combine is
exact in the same way with power-of-two routing weights: products and their
sum are exact in f32, so the output is the exact sum rounded once to bf16.
Random-value cases use the project's grouped tolerance (atol = rtol = 6e-2 of
test_moe_grouped_gemm128_vs_matmul), on every row, with values scaled so that
outputs are of magnitude 1 and the bound means something (measured on an
MI355X: GEMM max-abs error 0.0078 at outputs up to 3.2, the whole chain
0.067 at outputs up to 11.7; the tests print theirs).

Inputs are built on the CPU from a seeded generator. Every output buffer
starts from a sentinel, so an unwritten row shows, and rows past the live
tiles must keep it.
"""
from types import SimpleNamespace

import pytest
import torch

from room_amd import ops
from room_amd.engine.kv_cache import PagedKVCache
from room_amd.engine.step_plan import (PREFILL_MAX_ROWS, prefill_graph_shape,
                                       qtile_list)
from room_amd.models.qwen3_moe import Qwen3MoEConfig, Qwen3MoEModel, _Step
from room_amd.ops import reference as ref

DEV = "cuda"
BF = torch.bfloat16
SENTINEL = -1024.0
TOL = 6e-2          # the project's grouped-GEMM / MoE-chain tolerance
EDGE_COUNTS = [0, 1, 127, 128, 129, 0]


def gpu(fn):
    fn = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")(fn)
    return pytest.mark.gpu(fn)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _tern(g, *shape):
    """Values from {-1, 0, 1} as bf16."""
    return (torch.randint(0, 3, shape, generator=g) - 1).to(BF)


def _host_desc(counts, bm):
    """The descriptor rule in plain Python: experts in order, each cut into
    tiles of bm rows with a ragged last one; (expert, first pair row, rows)."""
    desc, row = [], 0
    for e, c in enumerate(counts):
        for m0 in range(0, c, bm):
            desc.append([e, row + m0, min(bm, c - m0)])
        row += c
    return desc


def _sorted_experts(counts):
    return torch.repeat_interleave(torch.arange(len(counts)),
                                   torch.tensor(counts)).int()


def _desc_counts(bm):
    # empty first, in the middle and last; 1, bm - 1, bm, bm + 1, 2 bm + 1
    return [0, 1, bm - 1, 0, bm, bm + 1, 2 * bm + 1, 0]


# --------------------------------------------------------------- CPU tests

@pytest.mark.parametrize("bm", [128, 16])
def test_desc_gmax_covers_the_host_rule(bm):
    """moe_desc_gmax rows suffice for the host rule, worst cases included:
    every expert ending in a ragged tile, one row per expert, one expert."""
    g = _gen(1)
    shapes = [_desc_counts(bm), [bm + 1] * 7, [1] * 9, [2 * bm + 1], [0, 0, 3],
              [bm] * 5]
    shapes += [torch.randint(0, 3 * bm, (6,), generator=g).tolist()
               for _ in range(20)]
    for counts in shapes:
        live = _host_desc(counts, bm)
        assert sum(d[2] for d in live) == sum(counts)
        assert len(live) <= ops.moe_desc_gmax(sum(counts), len(counts), bm)
    # and the bound is reached: E ragged one-row tiles on top of full ones
    counts = [bm + 1] * bm
    assert len(_host_desc(counts, bm)) == 2 * bm
    assert ops.moe_desc_gmax(sum(counts), bm, bm) == 2 * bm + 1


# --------------------------------------------------------------- GPU tests

@gpu
@pytest.mark.parametrize("bm", [128, 16])
def test_build_desc_matches_host_rule(bm):
    for counts in (_desc_counts(bm), [bm + 1] * 7, [1] * 9, [0, 0, 3]):
        E, P = len(counts), sum(counts)
        desc = ops.moe_build_desc_device(_sorted_experts(counts).to(DEV), E,
                                         bm).cpu()
        live = _host_desc(counts, bm)
        assert desc.shape == (ops.moe_desc_gmax(P, E, bm), 3)
        assert len(live) <= desc.size(0)
        assert desc[:len(live)].tolist() == live
        assert (desc[len(live):, 2] == 0).all()


def _grouped_inputs(g, counts, K, N, identity, exact, spare=7):
    """x, w, pair_token, desc and the fp32 expectation [P, N] of one grouped
    call, on the CPU. pair_token and out carry `spare` rows past the live
    tiles. identity: the down call's map (x has one row per pair); otherwise
    the gate/up call's, a non-identity map with repeated tokens."""
    E, P = len(counts), sum(counts)
    T = P + spare if identity else P // 3 + 5
    if exact:
        x, w = _tern(g, T, K), _tern(g, E, N, K)
    else:
        x = (torch.randn(T, K, generator=g) * 0.3).to(BF)
        w = (torch.randn(E, N, K, generator=g) * 0.05).to(BF)
    if identity:
        pair_token = torch.arange(P + spare, dtype=torch.int32)
    else:
        pair_token = torch.randint(0, T, (P + spare,), generator=g).int()
        assert not torch.equal(pair_token[:P], torch.arange(P).int())
        assert pair_token[:P].unique().numel() < P
    pair_expert = _sorted_experts(counts)
    expect, row = torch.empty(P, N), 0
    for e, c in enumerate(counts):
        rows = pair_token[row:row + c].long()
        expect[row:row + c] = x[rows].float() @ w[e].float().T
        row += c
    return x, w, pair_token, pair_expert, expect


def _grouped_run(x, w, pair_token, pair_expert, E, N):
    desc = ops.moe_build_desc_device(pair_expert.to(DEV), E)
    out = torch.full((pair_token.numel(), N), SENTINEL, dtype=BF, device=DEV)
    ops.moe_grouped_gemm128(out, x.to(DEV), w.to(DEV), pair_token.to(DEV),
                            desc)
    return out.cpu()


@gpu
@pytest.mark.parametrize("identity", [False, True], ids=["gather", "identity"])
@pytest.mark.parametrize("counts", [EDGE_COUNTS, [257]], ids=["edges", "257"])
@pytest.mark.parametrize("K", [64, 256])
@pytest.mark.parametrize("N", [64, 128, 192])
def test_grouped_gemm128_integer_exact(N, K, counts, identity):
    g = _gen(1000 + N + K + len(counts) + identity)
    x, w, pt, pe, expect = _grouped_inputs(g, counts, K, N, identity, True)
    assert expect.abs().max() <= K and (expect != 0).any()
    out = _grouped_run(x, w, pt, pe, len(counts), N)
    P = sum(counts)
    assert torch.equal(out[:P].float(), expect)
    assert (out[P:] == SENTINEL).all()       # nothing past the live tiles


@gpu
@pytest.mark.parametrize("K,N", [(2048, 1536), (768, 2048)])
def test_grouped_gemm128_random_every_row(K, N):
    """The model's gate/up and down shapes, values of
    test_moe_grouped_gemm128_vs_matmul, every pair row."""
    g = _gen(2000 + K)
    x, w, pt, pe, expect = _grouped_inputs(g, EDGE_COUNTS, K, N, False, False)
    out = _grouped_run(x, w, pt, pe, len(EDGE_COUNTS), N)
    P = sum(EDGE_COUNTS)
    err = (out[:P].float() - expect).abs()
    print(f"K={K} N={N}: max-abs err {err.max().item():.4f}, "
          f"max |expect| {expect.abs().max().item():.3f}")
    assert not torch.isnan(out[:P].float()).any()
    assert torch.allclose(out[:P].float(), expect, atol=TOL, rtol=TOL)
    assert (out[P:] == SENTINEL).all()


@gpu
def test_grouped_gemm128_row_independence():
    """A pair row's bits do not depend on where it sits: alone in its tile,
    last in a 129-row expert, in the middle and at the end of a full tile.
    Every wave owns 16 rows of the tile and runs the same k loop."""
    K, N = 2048, 128
    g = _gen(31)
    w = (torch.randn(1, N, K, generator=g) * 0.05).to(BF)
    probe = (torch.randn(K, generator=g) * 0.3).to(BF)
    rows = []
    for count, at in ((1, 0), (129, 128), (128, 77), (128, 127), (257, 200)):
        x = (torch.randn(count, K, generator=g) * 0.3).to(BF)
        x[at] = probe
        pt = torch.arange(count, dtype=torch.int32)
        out = _grouped_run(x, w, pt, _sorted_experts([count]), 1, N)
        rows.append(out[at])
    expect = w[0].float() @ probe.float()
    assert torch.allclose(rows[0].float(), expect, atol=TOL, rtol=TOL)
    for r in rows[1:]:
        assert torch.equal(r.view(torch.int16), rows[0].view(torch.int16))


@pytest.fixture(scope="module")
def model():
    """A tiny model, built the way test_wide_decode_gpu.py builds its own."""
    cfg = Qwen3MoEConfig.tiny()
    return Qwen3MoEModel(cfg, torch.device("cuda", 0), seed=7)


@gpu
@pytest.mark.parametrize("N", [64, 16])
@pytest.mark.parametrize("T", [9, 128, 129, 300])
def test_dense_capture_gemm_exact(model, T, N):
    """Qwen3MoEModel._dense with capture_gemm on, eager: one expert, the
    descriptor and identity map cached per T, and for N = 16 the weight
    padded to 64 rows and the result sliced back."""
    K = 256
    g = _gen(3000 + T + N)
    x, w = _tern(g, T, K).to(DEV), _tern(g, N, K).to(DEV)
    expect = x.float().cpu() @ w.float().cpu().T
    model.capture_gemm = True
    try:
        y1 = model._dense(x, w)
        desc, pt = model._dense_desc[T]
        wpad = model._dense_wpad.get(id(w))
        y2 = model._dense(x, w)
    finally:
        model.capture_gemm = False
    assert y1.shape == (T, N) and y1.dtype == BF
    assert torch.equal(y1.float().cpu(), expect)
    assert torch.equal(y2.float().cpu(), expect)
    # the second call reuses what the first one built
    assert model._dense_desc[T][0] is desc and model._dense_desc[T][1] is pt
    assert pt.tolist() == list(range(T))
    assert desc.cpu().tolist()[:(T + 127) // 128] == _host_desc([T], 128)
    if N % 64:
        assert wpad is not None and model._dense_wpad[id(w)] is wpad
        assert wpad.shape == (64, K) and torch.equal(wpad[:N], w)
        assert not wpad[N:].any()
    else:
        assert wpad is None
    model._dense_wpad.pop(id(w), None)     # w dies with this test


def _combine_inputs(g, T, K, H, exact):
    P = T * K
    if exact:
        z = torch.randint(-64, 65, (P, H), generator=g).to(BF)
        topk_w = torch.ldexp(torch.ones(T, K),
                             -torch.randint(0, 4, (T, K), generator=g))
    else:
        z = torch.randn(P, H, generator=g).to(BF)
        topk_w = torch.softmax(torch.randn(T, K, generator=g), -1)
    inv_order = torch.randperm(P, generator=g).int()
    expect = (topk_w.double()[:, :, None]
              * z[inv_order.long()].view(T, K, H).double()).sum(1)
    return z, topk_w.float(), inv_order, expect


def _combine_run(z, topk_w, inv_order, T, H):
    out = torch.full((T, H), SENTINEL, dtype=BF, device=DEV)
    ops.moe_combine_gather(out, z.to(DEV), topk_w.to(DEV), inv_order.to(DEV))
    return out.cpu()


@gpu
@pytest.mark.parametrize("T", [1, 37])
@pytest.mark.parametrize("H", [2048, 512])
@pytest.mark.parametrize("K", [8, 2])
def test_combine_gather_exact(K, H, T):
    """Weights 2^0 .. 2^-3 on integers up to 64: every product and the sum
    (below 2^10, a multiple of 2^-3) are exact in f32."""
    g = _gen(4000 + K + H + T)
    z, topk_w, inv_order, expect = _combine_inputs(g, T, K, H, True)
    out = _combine_run(z, topk_w, inv_order, T, H)
    assert torch.equal(expect.float().double(), expect)
    assert torch.equal(out.view(torch.int16),
                       expect.float().to(BF).view(torch.int16))


@gpu
def test_combine_gather_random():
    T, K, H = 37, 8, 2048
    z, topk_w, inv_order, expect = _combine_inputs(_gen(41), T, K, H, False)
    out = _combine_run(z, topk_w, inv_order, T, H)
    assert torch.allclose(out.float(), expect.float(), atol=2e-2, rtol=2e-2)


@gpu
def test_moe_chain_with_tile_edges(model):
    """Qwen3MoEModel._moe itself, ids chosen so that experts 0, 2, 6 and 7 get
    no pair (first, between busy ones, last), expert 1 exactly 128 and expert
    3 exactly 129, against ref.moe_ref on every row. Weights are scaled so
    that outputs are of magnitude 1."""
    cfg = model.cfg
    T, K, E = 150, 2, 8
    H, I = cfg.hidden_size, cfg.moe_intermediate_size
    g = _gen(51)
    ids = torch.empty(T, K, dtype=torch.int32)
    ids[:128] = torch.tensor([1, 3])
    ids[128] = torch.tensor([3, 4])
    ids[129:] = torch.tensor([5, 4])
    ids[::2] = ids[::2].flip(1)              # either order within a token
    counts = torch.bincount(ids.flatten().long(), minlength=E).tolist()
    assert counts == [0, 128, 0, 129, 22, 21, 0, 0]
    topk_w = torch.softmax(torch.randn(T, K, generator=g), -1)
    x = (torch.randn(T, H, generator=g) * 0.5).to(BF).to(DEV)
    layer = SimpleNamespace(
        w13=(torch.randn(E, 2 * I, H, generator=g) * 0.1).to(BF).to(DEV),
        w2=(torch.randn(E, H, I, generator=g) * 0.2).to(BF).to(DEV))
    st = _Step(seq_ids=None, q_pos=None, block_table=None, qtile_desc=None,
               hbuf=x,
               pair_token=torch.arange(T, dtype=torch.int32,
                                       device=DEV).repeat_interleave(K),
               pair_row=torch.arange(T * K, dtype=torch.int32, device=DEV))
    saved = cfg.num_experts, cfg.num_experts_per_tok
    cfg.num_experts, cfg.num_experts_per_tok = E, K
    try:
        out = model._moe(x, layer, ids.to(DEV), topk_w.to(DEV), st)
    finally:
        cfg.num_experts, cfg.num_experts_per_tok = saved
    assert out.dtype == BF and out.shape == (T, H)
    expect = ref.moe_ref(x, layer.w13, layer.w2, ids.to(DEV), topk_w.to(DEV))
    err = (out.float() - expect).abs()
    print(f"chain: max-abs err {err.max().item():.4f}, "
          f"max |expect| {expect.abs().max().item():.3f}")
    assert expect.abs().max().item() > 1.0
    assert not torch.isnan(out.float()).any()
    assert torch.allclose(out.float(), expect, atol=TOL, rtol=TOL)


@gpu
def test_padded_forward_equals_unpadded(model):
    """A 40-row chunk of two sequences run eagerly with capture_gemm on, and
    the same rows padded to 512 the way _PrefillGraph pads them (pad rows on a
    scrap slot at pos 0 in a segment of their own, zero-count q-tiles up to
    gmax, logits rows padded with row 0): the logits of the two last rows are
    bit-equal. Every op on the path is row-wise or has a row order fixed by
    (N, K): the norms, the grouped GEMM (test_grouped_gemm128_row_independence),
    rope + KV write, flash_prefill (tile cuts of the real rows are the same),
    the router, the combine (K terms in slot order) and the lm_head GEMV."""
    cfg = model.cfg
    dev = model.device
    g = _gen(61)
    lens = [25, 15]
    n = sum(lens)
    toks = torch.randint(0, cfg.vocab_size, (n,), generator=g).tolist()
    segments, seqs, pos = [], [], []
    for s, L in enumerate(lens):
        segments.append((len(seqs), L))
        seqs += [s] * L
        pos += list(range(L))
    last_rows = [lens[0] - 1, n - 1]
    i32 = dict(dtype=torch.int32, device=dev)

    def fresh_cache():
        cache = PagedKVCache(cfg.num_layers, cfg.num_kv_heads, cfg.head_dim,
                             16, 3, 8, dev)
        for s, L in enumerate(lens):
            assert cache.alloc_seq() == s
            cache.ensure_capacity(s, L)
        scrap = cache.alloc_seq()
        cache.ensure_capacity(scrap, 1)
        return cache, scrap

    model.capture_gemm = True
    try:
        cache, _ = fresh_cache()
        plain = model.forward(
            torch.tensor(toks, device=dev), torch.tensor(seqs, **i32),
            torch.tensor(pos, **i32), cache.block_table, cache.kcaches,
            cache.vcaches,
            logits_rows=torch.tensor(last_rows, device=dev),
            qtile_desc=ops.build_qtile_desc(segments, dev))

        cache, scrap = fresh_cache()
        tb, seg_graph = prefill_graph_shape(n, segments)
        assert tb == 512 and seg_graph[-1] == (n, tb - n)
        qt = ops.flash_prefill_qtile()
        tiles = qtile_list(seg_graph, qt)
        gmax = tb // qt + PREFILL_MAX_ROWS + 2
        desc = torch.zeros(gmax, 2, dtype=torch.int32)
        desc[:len(tiles)] = torch.tensor(tiles, dtype=torch.int32)
        rows = last_rows + [0] * (PREFILL_MAX_ROWS - len(last_rows))
        padded = model.forward(
            torch.tensor(toks + [0] * (tb - n), device=dev),
            torch.tensor(seqs + [scrap] * (tb - n), **i32),
            torch.tensor(pos + [0] * (tb - n), **i32), cache.block_table,
            cache.kcaches, cache.vcaches,
            logits_rows=torch.tensor(rows, device=dev),
            qtile_desc=desc.to(dev))
    finally:
        model.capture_gemm = False
    assert plain.shape == (2, cfg.vocab_size)
    assert padded.shape == (PREFILL_MAX_ROWS, cfg.vocab_size)
    assert not torch.isnan(plain).any() and plain.abs().max() > 0
    assert torch.equal(padded[:2].cpu(), plain.cpu())


@gpu
def test_grouped_gemm128_wrapper_errors():
    """Every call here is rejected by a TORCH_CHECK of the wrapper, which all
    stand before the launch: none reaches the kernel."""
    P, T, K, N, E = 5, 4, 64, 64, 2
    i32 = dict(dtype=torch.int32, device=DEV)

    def z(*shape, dtype=BF):
        return torch.zeros(*shape, dtype=dtype, device=DEV)

    def good():
        return dict(out=z(P, N), x=z(T, K), w=z(E, N, K),
                    pt=torch.zeros(P, **i32),
                    desc=torch.tensor([[0, 0, 3], [1, 3, 2]], **i32))

    def call(**bad):
        a = dict(good(), **bad)
        ops.moe_grouped_gemm128(a["out"], a["x"], a["w"], a["pt"], a["desc"])

    bad_calls = {
        "x f16": dict(x=z(T, K, dtype=torch.float16)),
        "w f32": dict(w=z(E, N, K, dtype=torch.float32)),
        "out f32": dict(out=z(P, N, dtype=torch.float32)),
        "x strided": dict(x=z(T, 2 * K)[:, :K]),
        "w strided": dict(w=z(E, N, 2 * K)[:, :, :K]),
        "out strided": dict(out=z(P, 2 * N)[:, :N]),
        "x 3-D": dict(x=z(2, 2, K)),
        "w 2-D": dict(w=z(N, K)),
        "w rows": dict(w=z(E, N + 64, K)),
        "w K": dict(w=z(E, N, K + 64)),
        "K % 64": dict(x=z(T, 96), w=z(E, N, 96)),
        "N % 64": dict(out=z(P, 96), w=z(E, 96, K)),
        "pair_token short": dict(pt=torch.zeros(P - 1, **i32)),
        "pair_token int64": dict(pt=torch.zeros(P, dtype=torch.int64,
                                                device=DEV)),
        "desc [G,2]": dict(desc=torch.zeros(2, 2, **i32)),
        "desc 1-D": dict(desc=torch.zeros(6, **i32)),
        "desc strided": dict(desc=torch.zeros(2, 6, **i32)[:, :3]),
        "desc int64": dict(desc=torch.zeros(2, 3, dtype=torch.int64,
                                            device=DEV)),
    }
    for what, bad in bad_calls.items():
        with pytest.raises(RuntimeError):
            call(**bad)
            pytest.fail(f"accepted: {what}")
    call()      # the unspoiled arguments are accepted
    torch.cuda.synchronize()


@gpu
def test_combine_gather_wrapper_errors():
    """As above for moe_combine_gather."""
    T, K, H = 3, 2, 64
    P = T * K

    def z(*shape, dtype=BF):
        return torch.zeros(*shape, dtype=dtype, device=DEV)

    def good():
        return dict(out=z(T, H), z=z(P, H), w=z(T, K, dtype=torch.float32),
                    inv=z(P, dtype=torch.int32))

    def call(**bad):
        a = dict(good(), **bad)
        ops.moe_combine_gather(a["out"], a["z"], a["w"], a["inv"])

    bad_calls = {
        "out f32": dict(out=z(T, H, dtype=torch.float32)),
        "out strided": dict(out=z(T, 2 * H)[:, :H]),
        "z f32": dict(z=z(P, H, dtype=torch.float32)),
        "z strided": dict(z=z(P, 2 * H)[:, :H]),
        "z width": dict(z=z(P, H + 8)),
        "inv_order short": dict(inv=z(P - 1, dtype=torch.int32)),
        "inv_order long": dict(inv=z(P + 1, dtype=torch.int32)),
        "inv_order int64": dict(inv=z(P, dtype=torch.int64)),
        "topk_w bf16": dict(w=z(T, K)),
        "topk_w f64": dict(w=z(T, K, dtype=torch.float64)),
        "topk_w rows": dict(w=z(T + 1, K, dtype=torch.float32)),
        "topk_w 1-D": dict(w=z(P, dtype=torch.float32)),
        "topk_w strided": dict(w=z(T, 2 * K, dtype=torch.float32)[:, :K]),
        "K = 9": dict(w=z(T, 9, dtype=torch.float32),
                      inv=z(T * 9, dtype=torch.int32), z=z(T * 9, H)),
        "H % 8": dict(out=z(T, 60), z=z(P, 60)),
    }
    for what, bad in bad_calls.items():
        with pytest.raises(RuntimeError):
            call(**bad)
            pytest.fail(f"accepted: {what}")
    call()
    torch.cuda.synchronize()
