"""Skinny grouped MFMA GEMM (wide-decode projections and MoE) against plain
matmuls. Integer-valued inputs make the exact cases exact: with x, w in
{-1, 0, 1} and K = 256 every partial sum is an integer of magnitude ≤ 256,
which f32 and bf16 both hold without rounding. GPU-only."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from room_amd import ops
else:
    pytest.skip("no GPU", allow_module_level=True)

DEV = "cuda"
BF = torch.bfloat16


def _ints(gen, *shape):
    """Non-symmetric random matrix over {-1, 0, 1}."""
    return torch.randint(-1, 2, shape, generator=gen, device=DEV).to(BF)


def _gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


# the edges of every tile-height template and its ragged last fragment
@pytest.mark.parametrize("M", [9, 16, 17, 32, 33, 48, 49, 64])
def test_dense_integer_exact(M):
    K = 256
    # one fragment / a count no workgroup width divides / the router. All
    # but (16, 16) are non-square and the values are non-symmetric, so a
    # transposed C mapping cannot hide.
    for N in (16, 80, 128):
        g = _gen(1000 * M + N)
        x, w = _ints(g, M, K), _ints(g, N, K)
        expect = x.float() @ w.float().T
        assert expect.abs().max() <= K
        yf = torch.full((M, N), float("nan"), dtype=torch.float32, device=DEV)
        ops.skinny_gemm(yf, x, w)
        assert torch.equal(yf, expect), (M, N, "f32")
        yb = torch.full((M, N), float("nan"), dtype=BF, device=DEV)
        ops.skinny_gemm(yb, x, w)
        assert torch.equal(yb.float(), expect), (M, N, "bf16")


@pytest.mark.parametrize("K", [256, 768, 2048, 4096])
def test_dense_random(K):
    # values and tolerance of test_gemv_vs_matmul
    N = 1024
    for M in (9, 64):
        g = _gen(K + M)
        x = torch.randn(M, K, generator=g, device=DEV).to(BF)
        w = (torch.randn(N, K, generator=g, device=DEV) * 0.05).to(BF)
        expect = x.float() @ w.float().T
        yf = torch.empty(M, N, dtype=torch.float32, device=DEV)
        ops.skinny_gemm(yf, x, w)
        assert torch.allclose(yf, expect, atol=5e-2, rtol=5e-2), (M, K)
        yb = torch.empty(M, N, dtype=BF, device=DEV)
        ops.skinny_gemm(yb, x, w)
        assert torch.allclose(yb.float(), expect.to(BF).float(),
                              atol=5e-2, rtol=5e-2), (M, K)


@pytest.mark.parametrize("K", [256, 768, 2048])
def test_row_independence(K):
    N = 512
    g = _gen(77 + K)
    x = torch.randn(64, K, generator=g, device=DEV).to(BF)
    w = (torch.randn(N, K, generator=g, device=DEV) * 0.05).to(BF)
    for dt in (torch.float32, BF):
        y64 = torch.empty(64, N, dtype=dt, device=DEV)
        ops.skinny_gemm(y64, x, w)
        y9 = torch.empty(9, N, dtype=dt, device=DEV)
        ops.skinny_gemm(y9, x[:9].contiguous(), w)
        assert torch.equal(y64[:9], y9)
        perm = torch.randperm(64, generator=g, device=DEV)
        yp = torch.empty(64, N, dtype=dt, device=DEV)
        ops.skinny_gemm(yp, x[perm].contiguous(), w)
        assert torch.equal(yp, y64[perm])


def test_wrapper_errors():
    K, N = 256, 64
    w = torch.zeros(N, K, dtype=BF, device=DEV)
    with pytest.raises((ValueError, RuntimeError)):       # 65 rows
        ops.skinny_gemm(torch.empty(65, N, dtype=BF, device=DEV),
                        torch.zeros(65, K, dtype=BF, device=DEV), w)
    with pytest.raises(RuntimeError):                     # f16 input
        ops.skinny_gemm(torch.empty(16, N, dtype=BF, device=DEV),
                        torch.zeros(16, K, dtype=torch.float16, device=DEV), w)
    with pytest.raises(RuntimeError):                     # non-contiguous x
        ops.skinny_gemm(torch.empty(16, N, dtype=BF, device=DEV),
                        torch.zeros(16, 2 * K, dtype=BF, device=DEV)[:, :K], w)
    with pytest.raises(RuntimeError):                     # K % 64 != 0
        ops.skinny_gemm(torch.empty(16, N, dtype=BF, device=DEV),
                        torch.zeros(16, 96, dtype=BF, device=DEV),
                        torch.zeros(N, 96, dtype=BF, device=DEV))
    with pytest.raises(RuntimeError):                     # N % 16 != 0
        ops.skinny_gemm(torch.empty(16, 24, dtype=BF, device=DEV),
                        torch.zeros(16, K, dtype=BF, device=DEV),
                        torch.zeros(24, K, dtype=BF, device=DEV))


# empty expert, one row, a full tile, a spill into a second tile
COUNTS = [0, 1, 16, 17]


def _grouped_case(g, K, N, integer, out_dtype=BF):
    E, P, T = len(COUNTS), sum(COUNTS), 20
    pair_expert = torch.tensor(
        [e for e, c in enumerate(COUNTS) for _ in range(c)],
        dtype=torch.int32, device=DEV)
    pair_token = torch.randint(0, T, (P,), generator=g, device=DEV).int()
    assert pair_token.unique().numel() < P          # drawn with repeats
    if integer:
        x, w = _ints(g, T, K), _ints(g, E, N, K)
    else:
        x = (torch.randn(T, K, generator=g, device=DEV) * 0.3).to(BF)
        w = (torch.randn(E, N, K, generator=g, device=DEV) * 0.05).to(BF)
    desc = ops.moe_build_desc_device(pair_expert, E, bm=16)
    assert desc.shape == (E + 3, 3)                 # trailing zero-size tiles
    live = desc[desc[:, 2] > 0].tolist()
    assert live == [[1, 0, 1], [2, 1, 16], [3, 17, 16], [3, 33, 1]]
    out = torch.full((P, N), float("nan"), dtype=out_dtype, device=DEV)
    ops.moe_grouped_gemm_skinny(out, x, w, pair_token, desc)
    expect = torch.stack([x[int(t)].float() @ w[int(e)].float().T
                          for t, e in zip(pair_token.tolist(),
                                          pair_expert.tolist())])
    return out.float(), expect


# tiny's w13 and w2 shapes, and the 30b down-projection K once
@pytest.mark.parametrize("K,N", [(512, 512), (256, 512), (768, 2048)])
def test_grouped_integer_exact(K, N):
    # |sum| ≤ K: exact in f32 at every K here, in bf16 up to 256
    out, expect = _grouped_case(_gen(5 + K), K, N, True, torch.float32)
    assert torch.equal(out, expect)
    if K <= 256:
        out, expect = _grouped_case(_gen(6 + K), K, N, True, BF)
        assert torch.equal(out, expect)


@pytest.mark.parametrize("K,N", [(512, 512), (256, 512), (768, 2048)])
def test_grouped_random(K, N):
    # the project's grouped tolerance (test_moe_grouped_gemm128_vs_matmul)
    out, expect = _grouped_case(_gen(9 + K), K, N, False)
    assert torch.allclose(out, expect.to(BF).float(), atol=6e-2, rtol=6e-2)
