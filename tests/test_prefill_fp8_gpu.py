"""moe_grouped_gemm128_fp8: the prefill grouped GEMM on block-scaled e4m3
expert weights.

The kernel stages a weight tile in LDS as bf16_rne(f32(q) * s), the bits of
dequantize_fp8_block(q, s).to(bf16), and from there runs the MFMA sequence of
moe_grouped_gemm128. So its output must equal moe_grouped_gemm128 on that
image bit for bit, for power-of-two scales (the product is exact) and for any
other scale (one f32 multiply and one rounding to nearest even, as torch's).

Shapes: the tile is 128 pair rows by 64 columns by 64 k, a scale block 128 by
128. Experts get 0, 1, 127, 128, 129 and 257 rows, with empty experts first,
between and last. N = 256 puts n-tiles 0-1 and 2-3 in different scale blocks,
N = 384 adds a third; K = 512 crosses three k-block edges.

Scales. (a) powers of two from 2^-12 to 2^-2. The range holds 11 of them and
a case has up to 48 blocks, so they cycle over the flat block index
(e, n/128, k/128); the helper asserts that two blocks next to each other
along any of the three axes never share a scale, which is what an index that
is off by one block, or that mixes two axes up, would read. (b) a random
scale per block, uniform in [0.7, 1.9] * 2^-6, no power of two.

Weight bytes are drawn uniformly from the 254 finite e4m3 codes (0x7F and
0xFF, the NaNs, left out; subnormals and both zeros included). Inputs are
built on the CPU from a seeded generator. Outputs start from a sentinel, and
out and pair_token carry spare rows past the live tiles, which must keep it.
"""
import pytest
import torch

from room_amd import ops
from room_amd.ops.reference import dequantize_fp8_block, quantize_fp8_block

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

DEV = "cuda"
BF = torch.bfloat16
FP8 = torch.float8_e4m3fn
SENTINEL = -1024.0
SPARE = 7
TOL = 6e-2          # the project's grouped-GEMM tolerance
COUNTS = {"edges": [0, 1, 127, 128, 129, 0], "257": [257, 0, 3]}
FINITE_CODES = torch.tensor([b for b in range(256) if b not in (0x7F, 0xFF)],
                            dtype=torch.uint8)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _random_codes(g, *shape):
    idx = torch.randint(0, FINITE_CODES.numel(), shape, generator=g)
    return FINITE_CODES[idx].view(FP8)


def _pow2_scales(E, N, K):
    """Scales (a): 2^(-12 + i mod 11) over the flat block index i."""
    nb, kb = N // 128, K // 128
    i = torch.arange(E * nb * kb).view(E, nb, kb)
    s = torch.ldexp(torch.ones(E, nb, kb), (i % 11) - 12)
    for dim in range(3):
        if s.size(dim) > 1:
            a = s.narrow(dim, 0, s.size(dim) - 1)
            b = s.narrow(dim, 1, s.size(dim) - 1)
            assert (a != b).all()
    assert s.min() >= 2.0 ** -12 and s.max() <= 2.0 ** -2
    return s


def _odd_scales(g, E, N, K):
    """Scales (b): distinct, none a power of two."""
    s = (0.7 + 1.2 * torch.rand(E, N // 128, K // 128, generator=g)) * 2.0 ** -6
    assert s.unique().numel() == s.numel()
    assert (torch.frexp(s)[0] != 0.5).all()
    return s.float()


def _sorted_experts(counts):
    return torch.repeat_interleave(torch.arange(len(counts)),
                                   torch.tensor(counts)).int()


def _pair_map(g, P, identity):
    """(pair_token with SPARE rows past the live ones, rows of x)."""
    if identity:
        return torch.arange(P + SPARE, dtype=torch.int32), P + SPARE
    T = P // 3 + 5
    pt = torch.randint(0, T, (P + SPARE,), generator=g).int()
    assert pt[:P].unique().numel() < P          # rows of x reused
    assert not torch.equal(pt[:P], torch.arange(P).int())
    return pt, T


def _run_fp8(x, q, s, pair_token, counts):
    N = q.size(1)
    desc = ops.moe_build_desc_device(_sorted_experts(counts).to(DEV),
                                     len(counts))
    out = torch.full((pair_token.numel(), N), SENTINEL, dtype=BF, device=DEV)
    r = ops.moe_grouped_gemm128_fp8(out, x.to(DEV), q.to(DEV), s.to(DEV),
                                    pair_token.to(DEV), desc)
    assert r is out
    return out.cpu()


def _run_image(x, q, s, pair_token, counts):
    N = q.size(1)
    image = dequantize_fp8_block(q, s).to(BF)
    desc = ops.moe_build_desc_device(_sorted_experts(counts).to(DEV),
                                     len(counts))
    out = torch.full((pair_token.numel(), N), SENTINEL, dtype=BF, device=DEV)
    ops.moe_grouped_gemm128(out, x.to(DEV), image.to(DEV), pair_token.to(DEV),
                            desc)
    return out.cpu()


def _expect_f32(x, w_f32, pair_token, counts):
    P, row = sum(counts), 0
    expect = torch.empty(P, w_f32.size(1))
    for e, c in enumerate(counts):
        rows = pair_token[row:row + c].long()
        expect[row:row + c] = x[rows].float() @ w_f32[e].T
        row += c
    return expect


# ------------------------------------------------ bit equality with the image

@pytest.mark.parametrize("identity", [False, True], ids=["gather", "identity"])
@pytest.mark.parametrize("scales", ["pow2", "odd"])
@pytest.mark.parametrize("N,K", [(128, 128), (256, 512), (384, 128)])
@pytest.mark.parametrize("counts", list(COUNTS), ids=list(COUNTS))
def test_bit_equal_to_image_path(counts, N, K, scales, identity):
    counts = COUNTS[counts]
    E, P = len(counts), sum(counts)
    g = _gen(100 + N + K + E + 2 * identity + (scales == "odd"))
    q = _random_codes(g, E, N, K)
    s = _pow2_scales(E, N, K) if scales == "pow2" else _odd_scales(g, E, N, K)
    pt, T = _pair_map(g, P, identity)
    x = (torch.randn(T, K, generator=g) * 0.3).to(BF)
    got = _run_fp8(x, q, s, pt, counts)
    want = _run_image(x, q, s, pt, counts)
    assert not torch.isnan(want[:P].float()).any()
    assert (want[:P] != 0).any() and (want[:P] != SENTINEL).any()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert (got[P:] == SENTINEL).all()        # nothing past the live tiles


# --------------------------------------- scale addressing, without the image

@pytest.mark.parametrize("counts", list(COUNTS), ids=list(COUNTS))
def test_planted_scales_come_back(counts):
    """Every weight is 1.0 and x row p is a one-hot at column k_p, so
    out[p][n] is the scale of block (e, n/128, k_p/128) itself: a power of
    two from 2^-12 up, exact in bf16. k_p walks over the first and last
    column of every k-block."""
    counts = COUNTS[counts]
    E, P, N, K = len(counts), sum(counts), 256, 512
    q = torch.full((E, N, K), 0x38, dtype=torch.uint8).view(FP8)
    assert (q.float() == 1.0).all()
    s = _pow2_scales(E, N, K)
    cols = [c for b in range(K // 128) for c in (128 * b, 128 * b + 127)]
    kp = torch.tensor([cols[(p * 3 + p // 8) % len(cols)] for p in range(P)])
    assert set(kp.tolist()) == set(cols)
    x = torch.zeros(P + SPARE, K, dtype=BF)
    x[torch.arange(P), kp] = 1.0
    pt = torch.arange(P + SPARE, dtype=torch.int32)
    got = _run_fp8(x, q, s, pt, counts)
    pe = _sorted_experts(counts).long()
    expect = s[pe, :, kp // 128].repeat_interleave(128, dim=1)
    assert expect.shape == (P, N)
    assert expect[0, 0] == s[pe[0], 0, kp[0] // 128]
    assert expect[-1, -1] == s[pe[-1], -1, kp[-1] // 128]
    assert torch.equal(got[:P].float(), expect)
    assert (got[P:] == SENTINEL).all()


# ------------------------------------------------- against the fp32 reference

@pytest.mark.parametrize("identity", [False, True], ids=["gather", "identity"])
def test_against_fp32_reference(identity):
    counts = COUNTS["edges"]
    E, P, N, K = len(counts), sum(counts), 256, 512
    g = _gen(300 + identity)
    q, s = quantize_fp8_block(torch.randn(E, N, K, generator=g) * 0.15)
    pt, T = _pair_map(g, P, identity)
    x = (torch.randn(T, K, generator=g) * 0.3).to(BF)
    expect = _expect_f32(x, dequantize_fp8_block(q, s), pt, counts)
    got = _run_fp8(x, q, s, pt, counts)
    err = (got[:P].float() - expect).abs()
    print(f"fp8 grouped vs fp32: max-abs err {err.max().item():.4f}, "
          f"max |expect| {expect.abs().max().item():.3f}")
    assert expect.abs().max() > 1.0
    assert not torch.isnan(got[:P].float()).any()
    assert torch.allclose(got[:P].float(), expect, atol=TOL, rtol=TOL)
    assert (got[P:] == SENTINEL).all()


# ------------------------------------------------------------ exact integers

@pytest.mark.parametrize("identity", [False, True], ids=["gather", "identity"])
@pytest.mark.parametrize("N,K", [(128, 128), (384, 256)])
@pytest.mark.parametrize("counts", list(COUNTS), ids=list(COUNTS))
def test_integer_exact(counts, N, K, identity):
    """Weights and x from {-1, 0, 1}, scale 1.0, K <= 256: every dot product
    is an integer that f32 and bf16 hold exactly."""
    counts = COUNTS[counts]
    E, P = len(counts), sum(counts)
    g = _gen(400 + N + K + E + identity)
    codes = torch.tensor([0xB8, 0x00, 0x38], dtype=torch.uint8)   # -1, 0, 1
    q = codes[torch.randint(0, 3, (E, N, K), generator=g)].view(FP8)
    s = torch.ones(E, N // 128, K // 128)
    pt, T = _pair_map(g, P, identity)
    x = (torch.randint(0, 3, (T, K), generator=g) - 1).to(BF)
    expect = _expect_f32(x, q.float(), pt, counts)
    assert expect.abs().max() <= K and (expect != 0).any()
    got = _run_fp8(x, q, s, pt, counts)
    assert torch.equal(got[:P].float(), expect)
    assert (got[P:] == SENTINEL).all()


# ------------------------------------------------------------ argument checks

def test_wrapper_errors():
    """Every bad call is rejected by a TORCH_CHECK that stands before the
    launch: none reaches the kernel."""
    P, T, K, N, E = 5, 4, 256, 128, 2
    i32 = dict(dtype=torch.int32, device=DEV)

    def z(*shape, dtype=BF):
        return torch.zeros(*shape, dtype=dtype, device=DEV)

    def zq(*shape):
        return torch.zeros(*shape, dtype=torch.uint8, device=DEV).view(FP8)

    def good():
        return dict(out=z(P, N), x=z(T, K), q=zq(E, N, K),
                    s=torch.ones(E, N // 128, K // 128, device=DEV),
                    pt=torch.zeros(P, **i32),
                    desc=torch.tensor([[0, 0, 3], [1, 3, 2]], **i32))

    def call(**bad):
        a = dict(good(), **bad)
        ops.moe_grouped_gemm128_fp8(a["out"], a["x"], a["q"], a["s"],
                                    a["pt"], a["desc"])

    bad_calls = {
        "bf16 as w_q": dict(q=z(E, N, K)),
        "scale shape": dict(s=torch.ones(E, N // 128, K // 128 + 1,
                                         device=DEV)),
        "scale 2-D": dict(s=torch.ones(E, N // 128 * (K // 128), device=DEV)),
        "scale dtype": dict(s=torch.ones(E, N // 128, K // 128, dtype=BF,
                                         device=DEV)),
        "K = 192": dict(x=z(T, 192), q=zq(E, N, 192),
                        s=torch.ones(E, N // 128, 1, device=DEV)),
        "w_q strided": dict(q=zq(E, N, 2 * K)[:, :, :K]),
        "x f16": dict(x=z(T, K, dtype=torch.float16)),
        "x strided": dict(x=z(T, 2 * K)[:, :K]),
        "x K": dict(x=z(T, K + 128)),
        "out f32": dict(out=z(P, N, dtype=torch.float32)),
        "out N": dict(out=z(P, N + 128)),
        "pair_token short": dict(pt=torch.zeros(P - 1, **i32)),
        "pair_token int64": dict(pt=torch.zeros(P, dtype=torch.int64,
                                                device=DEV)),
        "desc [G,2]": dict(desc=torch.zeros(2, 2, **i32)),
        "desc 1-D": dict(desc=torch.zeros(6, **i32)),
        "desc int64": dict(desc=torch.zeros(2, 3, dtype=torch.int64,
                                            device=DEV)),
        "desc strided": dict(desc=torch.zeros(2, 6, **i32)[:, :3]),
        "scales on the CPU": dict(s=torch.ones(E, N // 128, K // 128)),
    }
    for what, bad in bad_calls.items():
        with pytest.raises(RuntimeError):
            call(**bad)
            pytest.fail(f"accepted: {what}")
    call()      # the unspoiled arguments are accepted
    torch.cuda.synchronize()
