"""FP8 expert weights on the GPU: the three block-scaled e4m3 kernels against
their bf16 twins run on the bf16 image and against fp32 torch, then the model
with expert_dtype="fp8" against a bf16 model holding the image.

Exact cases: x and w are small integers and every 128x128 block of w carries
its own power-of-two factor (2^-6..2^2), so w is exactly representable as
e4m3 times a power-of-two scale and in bf16. With |x| <= 2, |w| <= 4 a block's
integer dot is at most 128*2*4 = 2^10, so over K <= 2048 (16 blocks, factors
up to 2^2) every partial sum, in any order, is a multiple of 2^-6 of magnitude
at most 2^16: 22 bits, exact in f32."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from room_amd import ops
from room_amd.engine.kv_cache import PagedKVCache
from room_amd.models.qwen3_moe import Qwen3MoEConfig, Qwen3MoEModel
from room_amd.ops.reference import dequantize_fp8_block, quantize_fp8_block

DEV = torch.device("cuda", 0)
BF = torch.bfloat16
FP8 = torch.float8_e4m3fn


def _gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def _block_factors(E, N, K, lo=-6, hi=2):
    """Power-of-two factor per 128x128 block; neighbours in e, n and k always
    differ: steps (5, 3, 1) modulo 9 exponents, (1, 2, 1) modulo 6."""
    R = hi - lo + 1
    assert R in (6, 9)
    se, sn = (5, 3) if R == 9 else (1, 2)
    e = torch.arange(E, device=DEV).view(E, 1, 1)
    n = torch.arange(N // 128, device=DEV).view(1, -1, 1)
    k = torch.arange(K // 128, device=DEV).view(1, 1, -1)
    ex = lo + (se * e + sn * n + k) % R
    return torch.ldexp(torch.ones(ex.shape, device=DEV), ex)


def _int_weights(g, E, N, K, lo=-6, hi=2):
    """(w f32 exact, q, s, bf16 image): integers -4..4 times block factors."""
    w = torch.randint(-4, 5, (E, N, K), generator=g, device=DEV).float()
    f = _block_factors(E, N, K, lo, hi)
    w = w * f.repeat_interleave(128, -2).repeat_interleave(128, -1)
    q, s = quantize_fp8_block(w)
    deq = dequantize_fp8_block(q, s)
    assert torch.equal(deq, w)                  # the fp8 form holds w exactly
    img = deq.to(BF)
    assert torch.equal(img.float(), w)          # and so does the bf16 image
    assert s.unique().numel() >= 6              # the scales really vary
    return w, q, s, img


def _int_x(g, T, K):
    return torch.randint(-2, 3, (T, K), generator=g, device=DEV).to(BF)


def _pairs(g, T, E, k=4):
    """k distinct experts per token, expert E-1 always among them."""
    ids = torch.stack([torch.randperm(E, generator=g, device=DEV)[:k]
                       for _ in range(T)])
    ids[0, 0] = E - 1 if (ids[0] != E - 1).all() else ids[0, 0]
    assert (ids == E - 1).any()
    pair_token = torch.arange(T, device=DEV).repeat_interleave(k).int()
    return pair_token, ids.flatten().int().contiguous()


def _h_ref(x, w13, pair_token, pair_expert, I):
    """fp32 silu(x·Wg)·(x·Wu) per pair."""
    gu = torch.stack([x[int(t)].float() @ w13[int(e)].T
                      for t, e in zip(pair_token.tolist(),
                                      pair_expert.tolist())])
    return gu[:, :I], gu[:, I:]


# --------------------------------------------------------------- GEMV h

@pytest.mark.parametrize("T", [1, 5, 8])
@pytest.mark.parametrize("H,I", [(512, 256), (640, 256), (2048, 768),
                                 (2048, 256), (512, 768), (640, 768)])
def test_gemv_h_integer_exact(H, I, T):
    E = 4
    g = _gen(H + I + T)
    w, q, s, img = _int_weights(g, E, 2 * I, H)
    x = _int_x(g, T, H)
    pair_token, pair_expert = _pairs(g, T, E)
    P = pair_token.numel()
    h8 = torch.full((P, I), float("nan"), dtype=BF, device=DEV)
    zero = torch.full((T, H), float("nan"), dtype=torch.float32, device=DEV)
    ops.moe_gemv_h_fp8(h8, x, q, s, pair_token, pair_expert, out_zero=zero)
    assert (zero == 0).all()
    assert not h8.float().isnan().any()
    if H % 512 == 0:
        # the bf16 twin on the image: the same exact dots, the same epilogue
        hb = torch.empty(P, I, dtype=BF, device=DEV)
        ops.moe_gemv_h(hb, x, img, pair_token, pair_expert)
        assert torch.equal(h8, hb)
    # fp32 torch on the exact dots. The kernel's __expf and torch's sigmoid
    # differ by a few f32 ulps, which can move the bf16 rounding of silu·up
    # by one bf16 ulp (2^-7 relative), never more; a saturated silu (dot
    # below -87) is -0 in the kernel and a denormal-sized value in torch.
    dg, du = _h_ref(x, w, pair_token, pair_expert, I)
    expect = (F.silu(dg) * du).to(BF).float()
    assert torch.allclose(h8.float(), expect, rtol=2.0 ** -7, atol=1e-30)


def test_gemv_h_random():
    # shapes, values and bounds of test_moe_gemv_path (bf16 chain)
    torch.manual_seed(80)
    T, E, H, I = 5, 16, 2048, 768
    x = torch.randn(T, H, dtype=BF, device=DEV) * 0.5
    w13 = torch.randn(E, 2 * I, H, dtype=BF, device=DEV) * 0.02
    q, s = quantize_fp8_block(w13)
    pair_token, pair_expert = _pairs(_gen(81), T, E, 8)
    h8 = torch.empty(T * 8, I, dtype=BF, device=DEV)
    ops.moe_gemv_h_fp8(h8, x, q, s, pair_token, pair_expert)
    dg, du = _h_ref(x, dequantize_fp8_block(q, s), pair_token, pair_expert, I)
    assert torch.allclose(h8.float(), F.silu(dg) * du, atol=5e-2, rtol=5e-2)


# ------------------------------------------------------------ GEMV down

def _down_ref(h, w2, pair_w, pair_token, pair_expert, T):
    out = torch.zeros(T, w2.size(1), dtype=torch.float32, device=DEV)
    for p, (t, e) in enumerate(zip(pair_token.tolist(), pair_expert.tolist())):
        out[t] += pair_w[p] * (h[p].float() @ w2[e].T)
    return out


@pytest.mark.parametrize("T", [1, 5, 8])
@pytest.mark.parametrize("H,I", [(512, 256), (640, 128), (2048, 768),
                                 (256, 640)])
def test_gemv_down_integer_exact(H, I, T):
    # block factors 2^-4..2^1, pair weights 2^-1..2^1, 4 pairs per token:
    # |sum| <= 6 blocks * 2^10 * 2 * 2 * 4 < 2^17 in steps of 2^-5: 22 bits,
    # so the f32 atomics are exact in any order
    E = 4
    g = _gen(3 * H + I + T)
    w, q, s, _img = _int_weights(g, E, H, I, lo=-4, hi=1)
    pair_token, pair_expert = _pairs(g, T, E)
    P = pair_token.numel()
    h = _int_x(g, P, I)
    pair_w = torch.ldexp(torch.ones(P, device=DEV),
                         torch.randint(-1, 2, (P,), generator=g, device=DEV))
    out = torch.zeros(T, H, dtype=torch.float32, device=DEV)
    ops.moe_gemv_down_fp8(out, h, q, s, pair_w, pair_token, pair_expert)
    assert torch.equal(out, _down_ref(h, w, pair_w, pair_token, pair_expert, T))


def test_gemv_down_random():
    torch.manual_seed(82)
    T, E, H, I = 5, 16, 2048, 768
    w2 = torch.randn(E, H, I, dtype=BF, device=DEV) * 0.02
    q, s = quantize_fp8_block(w2)
    pair_token, pair_expert = _pairs(_gen(83), T, E, 8)
    P = pair_token.numel()
    h = torch.randn(P, I, dtype=BF, device=DEV) * 0.5
    pair_w = torch.softmax(torch.randn(T, 8, device=DEV), -1).flatten()
    out = torch.zeros(T, H, dtype=torch.float32, device=DEV)
    ops.moe_gemv_down_fp8(out, h, q, s, pair_w, pair_token, pair_expert)
    expect = _down_ref(h, dequantize_fp8_block(q, s), pair_w, pair_token,
                       pair_expert, T)
    assert torch.allclose(out, expect, atol=5e-2, rtol=5e-2)


# ------------------------------------------------------- skinny grouped

# 8 experts: empty ones, one row, a full tile, full + 1, 15 rows, full + 15
COUNTS = [0, 1, 16, 17, 0, 15, 31, 2]
LIVE = [[1, 0, 1], [2, 1, 16], [3, 17, 16], [3, 33, 1], [5, 34, 15],
        [6, 49, 16], [6, 65, 15], [7, 80, 2]]


def _grouped_setup(g, T=24):
    E, P = len(COUNTS), sum(COUNTS)
    pair_expert = torch.tensor(
        [e for e, c in enumerate(COUNTS) for _ in range(c)],
        dtype=torch.int32, device=DEV)
    pair_token = torch.randint(0, T, (P,), generator=g, device=DEV).int()
    desc = ops.moe_build_desc_device(pair_expert, E, bm=16)
    assert desc[desc[:, 2] > 0].tolist() == LIVE
    return E, P, T, pair_expert, pair_token, desc


def _grouped_ref(x, w, pair_token, pair_expert):
    return torch.stack([x[int(t)].float() @ w[int(e)].T
                        for t, e in zip(pair_token.tolist(),
                                        pair_expert.tolist())])


@pytest.mark.parametrize("K,N", [(512, 256), (768, 256), (2048, 256),
                                 (512, 1536), (768, 1536), (2048, 1536)])
def test_skinny_integer_exact(K, N):
    g = _gen(7 * K + N)
    E, P, T, pair_expert, pair_token, desc = _grouped_setup(g)
    w, q, s, img = _int_weights(g, E, N, K)
    x = _int_x(g, T, K)
    out = torch.full((P, N), float("nan"), dtype=torch.float32, device=DEV)
    ops.moe_grouped_gemm_skinny_fp8(out, x, q, s, pair_token, desc)
    assert torch.equal(out, _grouped_ref(x, w, pair_token, pair_expert))
    twin = torch.empty(P, N, dtype=torch.float32, device=DEV)
    ops.moe_grouped_gemm_skinny(twin, x, img, pair_token, desc)
    assert torch.equal(out, twin)


@pytest.mark.parametrize("K,N", [(768, 2048), (2048, 1536)])
def test_skinny_random(K, N):
    # values and bound of test_grouped_random
    g = _gen(9 + K)
    E, P, T, pair_expert, pair_token, desc = _grouped_setup(g)
    x = (torch.randn(T, K, generator=g, device=DEV) * 0.3).to(BF)
    w = (torch.randn(E, N, K, generator=g, device=DEV) * 0.05).to(BF)
    q, s = quantize_fp8_block(w)
    out = torch.full((P, N), float("nan"), dtype=BF, device=DEV)
    ops.moe_grouped_gemm_skinny_fp8(out, x, q, s, pair_token, desc)
    expect = _grouped_ref(x, dequantize_fp8_block(q, s), pair_token,
                          pair_expert)
    assert torch.allclose(out.float(), expect.to(BF).float(),
                          atol=6e-2, rtol=6e-2)


@pytest.mark.parametrize("K", [512, 768, 2048])
def test_skinny_row_independence_and_determinism(K):
    """A token's output row has the same bits alone in a 1-row tile, in a full
    tile at any position, and in a 15-row tile; two calls agree bit for bit."""
    N, E = 256, 2
    g = _gen(31 + K)
    x = (torch.randn(16, K, generator=g, device=DEV) * 0.3).to(BF)
    w = (torch.randn(E, N, K, generator=g, device=DEV) * 0.05).to(BF)
    q, s = quantize_fp8_block(w)
    i32 = dict(dtype=torch.int32, device=DEV)

    def run(pair_token, tiles, dt):
        out = torch.full((pair_token.numel(), N), float("nan"), dtype=dt,
                         device=DEV)
        ops.moe_grouped_gemm_skinny_fp8(
            out, x, q, s, pair_token, torch.tensor(tiles, **i32))
        return out

    ident = torch.arange(16, **i32)
    perm = torch.randperm(16, generator=g, device=DEV).int()
    for dt in (torch.float32, BF):
        full = run(ident, [[1, 0, 16]], dt)
        assert not full.float().isnan().any()
        assert torch.equal(run(ident, [[1, 0, 16]], dt), full)
        singles = run(ident, [[1, i, 1] for i in range(16)], dt)
        assert torch.equal(singles, full)
        ragged = run(ident, [[1, 0, 15], [1, 15, 1]], dt)
        assert torch.equal(ragged, full)
        moved = run(perm, [[1, 0, 16]], dt)
        assert torch.equal(moved, full[perm.long()])


# -------------------------------------------------------- wrapper errors

def test_wrapper_errors():
    E, N, K, T = 2, 256, 256, 4
    i32 = dict(dtype=torch.int32, device=DEV)
    x = torch.zeros(T, K, dtype=BF, device=DEV)
    q = torch.zeros(E, N, K, dtype=BF, device=DEV).to(FP8)
    s = torch.ones(E, N // 128, K // 128, device=DEV)
    pt = torch.arange(T, **i32)
    pe = torch.zeros(T, **i32)
    desc = torch.tensor([[0, 0, 4]], **i32)

    def grouped(x=x, q=q, s=s, N=N):
        ops.moe_grouped_gemm_skinny_fp8(
            torch.empty(T, N, dtype=BF, device=DEV), x, q, s, pt, desc)

    def gemv_h(x=x, q=q, s=s, N=N):
        ops.moe_gemv_h_fp8(torch.empty(T, N // 2, dtype=BF, device=DEV), x, q,
                           s, pt, pe)

    def gemv_down(x=x, q=q, s=s, N=N):
        ops.moe_gemv_down_fp8(torch.zeros(T, N, device=DEV), x, q, s,
                              torch.ones(T, device=DEV), pt, pe)

    for call in (grouped, gemv_h, gemv_down):
        call()                                            # the good call runs
        with pytest.raises(RuntimeError):                 # bf16 weights
            call(q=torch.zeros(E, N, K, dtype=BF, device=DEV))
        with pytest.raises(RuntimeError):                 # scale shape
            call(s=torch.ones(E, N // 128, K // 128 + 1, device=DEV))
        with pytest.raises(RuntimeError):                 # scale shape
            call(s=torch.ones(E, N // 128 * K // 128, device=DEV))
        with pytest.raises(RuntimeError):                 # scale dtype
            call(s=s.to(BF))
        with pytest.raises(RuntimeError):                 # K = 192
            call(x=torch.zeros(T, 192, dtype=BF, device=DEV),
                 q=torch.zeros(E, N, 192, dtype=BF, device=DEV).to(FP8),
                 s=torch.ones(E, N // 128, 1, device=DEV))
        with pytest.raises(RuntimeError):                 # f16 activations
            call(x=x.to(torch.float16))
        with pytest.raises(RuntimeError):                 # non-contiguous w
            call(q=torch.zeros(E, N, 2 * K, dtype=BF,
                               device=DEV).to(FP8)[:, :, :K])
    torch.cuda.synchronize()


# ----------------------------------------------------------------- model

def test_model_fp8_matches_bf16_image_model():
    # every expert always selected (8 experts, top-8): routing cannot flip on
    # a rounding difference, so the two models' logits differ continuously
    cfg = Qwen3MoEConfig(vocab_size=4096, hidden_size=512, num_layers=2,
                         num_q_heads=8, num_kv_heads=1, head_dim=128,
                         num_experts=8, num_experts_per_tok=8,
                         moe_intermediate_size=256, max_position=1024)
    m8 = Qwen3MoEModel(cfg, DEV, seed=7, expert_dtype="fp8")
    mb = Qwen3MoEModel(cfg, DEV, seed=7)
    assert m8.expert_dtype == "fp8" and mb.expert_dtype == "bf16"
    for l8, lb in zip(m8.layers, mb.layers):
        assert l8.w13_q.dtype == FP8 and l8.w2_q.dtype == FP8
        assert l8.w13_s.shape == (8, 4, 4) and l8.w2_s.shape == (8, 4, 2)
        assert torch.equal(l8.w13.float(),
                           dequantize_fp8_block(l8.w13_q, l8.w13_s))
        assert torch.equal(l8.w2.float(),
                           dequantize_fp8_block(l8.w2_q, l8.w2_s))
        assert not hasattr(lb, "w13_q") and not hasattr(lb, "w2_s")
        assert torch.equal(l8.wqkv, lb.wqkv)      # same seed, same stream
        lb.w13, lb.w2 = l8.w13, l8.w2
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
    i32 = dict(dtype=torch.int32, device=DEV)
    step_tok = torch.randint(0, cfg.vocab_size, (nseq,), generator=g).to(DEV)
    seq_t = torch.arange(nseq, **i32)
    pos_t = torch.tensor(lens, **i32)

    def prepare(model):
        cache = PagedKVCache(cfg.num_layers, cfg.num_kv_heads, cfg.head_dim,
                             nseq * 4 + 1, nseq, cfg.max_position // 16, DEV)
        for sq, n in enumerate(lens):
            assert cache.alloc_seq() == sq
            cache.ensure_capacity(sq, n + 1)
        model.forward(torch.tensor(toks, device=DEV),
                      torch.tensor(seqs, **i32), torch.tensor(pos, **i32),
                      cache.block_table, cache.kcaches, cache.vcaches,
                      logits_rows=torch.zeros(0, dtype=torch.int64, device=DEV),
                      qtile_desc=ops.build_qtile_desc(segments, DEV))

        def step(rows):
            # each call rewrites the KV of position len before reading it,
            # and nothing older: every call starts from the same cache state
            return model.forward(step_tok[rows], seq_t[rows], pos_t[rows],
                                 cache.block_table, cache.kcaches,
                                 cache.vcaches)
        return step

    step8, stepb = prepare(m8), prepare(mb)
    for name, rows in (("narrow T=5", slice(0, 5)), ("wide T=12", slice(0, 12))):
        a, b = step8(rows), stepb(rows)
        diff = (a - b).abs().max().item()
        print(f"fp8 vs bf16-image logits, {name}: max abs diff {diff:.3e}, "
              f"max |logit| {b.abs().max().item():.3f}")
        # the project's bound for a bf16 MoE chain
        assert torch.allclose(a, b, atol=6e-2, rtol=6e-2), (name, diff)
    wide12 = step8(slice(0, 12))
    assert torch.equal(step8(slice(0, 12)), wide12)       # bit-reproducible
    assert torch.equal(step8(slice(0, 33))[:12], wide12)  # ignores batch mates
