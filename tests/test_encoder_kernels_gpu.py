"""Memory-encoder HIP kernels (csrc/encoder.hip) against their fp32 references,
and moe_grouped_gemm_skinny at the encoder's projection shapes."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from room_amd import ops
from room_amd.ops import reference as ref

DEV = "cuda"
BF = torch.bfloat16
D = 384


def bf16_close(a, b, atol=2e-2, rtol=2e-2):
    return torch.allclose(a.float(), b.float(), atol=atol, rtol=rtol)


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _cu(lens):
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    return cu


# ------------------------------------------------------------- attention
# fragment (16), k-step (32) and tile-pair boundaries; row offsets that are
# no multiple of 16
ATTN_LENS = [1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 64, 65, 127, 128]


def _attn(qkv, cu):
    out = torch.full((qkv.size(0), D), float("nan"), dtype=BF, device=DEV)
    return ops.encoder_attention(out, qkv, _i32(cu), cu_rows_host=cu)


@pytest.fixture(scope="module")
def attn_case():
    g = torch.Generator(device=DEV)
    g.manual_seed(50)
    cu = _cu(ATTN_LENS)
    qkv = torch.randn(cu[-1], 3 * D, generator=g, device=DEV).to(BF)
    return dict(qkv=qkv, cu=cu, out=_attn(qkv, cu),
                expect=ref.encoder_attention_ref(qkv, cu))


def test_attention_matches_ref(attn_case):
    c = attn_case
    assert not c["out"].float().isnan().any()
    err = (c["out"].float() - c["expect"]).abs().max()
    print(f"encoder_attention max |err| {float(err):.3e}")
    assert bf16_close(c["out"], c["expect"], atol=3e-2)


def test_attention_deterministic(attn_case):
    c = attn_case
    assert torch.equal(_attn(c["qkv"], c["cu"]), c["out"])


def test_attention_segment_alone_is_bit_equal(attn_case):
    c = attn_case
    for lo, hi in zip(c["cu"], c["cu"][1:]):
        alone = _attn(c["qkv"][lo:hi].contiguous(), [0, hi - lo])
        assert torch.equal(alone, c["out"][lo:hi]), hi - lo


def test_attention_reads_only_its_segment(attn_case):
    """Every other segment's rows NaN: the mask and the row addressing keep a
    segment's output untouched."""
    c = attn_case
    for lo, hi in zip(c["cu"], c["cu"][1:]):
        poisoned = torch.full_like(c["qkv"], float("nan"))
        poisoned[lo:hi] = c["qkv"][lo:hi]
        assert torch.equal(_attn(poisoned, c["cu"])[lo:hi], c["out"][lo:hi]), \
            hi - lo


def test_attention_wrapper_errors():
    qkv = torch.zeros(20, 3 * D, dtype=BF, device=DEV)
    out = torch.zeros(20, D, dtype=BF, device=DEV)
    cu = _i32([0, 20])
    ops.encoder_attention(out, qkv, cu)                       # sane call
    with pytest.raises(RuntimeError):                          # dtype
        ops.encoder_attention(out, qkv.float(), cu)
    with pytest.raises(RuntimeError):
        ops.encoder_attention(out.float(), qkv, cu)
    with pytest.raises(RuntimeError):                          # contiguity
        wide = torch.zeros(20, 6 * D, dtype=BF, device=DEV)
        ops.encoder_attention(out, wide[:, :3 * D], cu)
    with pytest.raises(RuntimeError):                          # row width
        ops.encoder_attention(out, qkv[:, :D].contiguous(), cu)
    with pytest.raises(RuntimeError):                          # cu dtype
        ops.encoder_attention(out, qkv, cu.long())
    with pytest.raises(RuntimeError):                          # empty segment
        ops.encoder_attention(out, qkv, _i32([0, 0, 20]))
    with pytest.raises(RuntimeError):                          # cu[-1] != R
        ops.encoder_attention(out, qkv, _i32([0, 19]))
    big = torch.zeros(129, 3 * D, dtype=BF, device=DEV)
    with pytest.raises(RuntimeError):                          # length 129
        ops.encoder_attention(torch.zeros(129, D, dtype=BF, device=DEV), big,
                              _i32([0, 129]))


# ----------------------------------------------------------------- embed

def test_embed_bit_equal():
    g = torch.Generator(device=DEV)
    g.manual_seed(51)
    R, P = 37, 256
    idx = torch.randint(0, D, (R, 4), generator=g, device=DEV)
    plus = torch.randint(0, 2, (R, 4), generator=g, device=DEV)
    idx[0] = torch.tensor([5, 5, 9, 200])     # same index, equal signs: +1
    plus[0] = torch.tensor([1, 1, 0, 1])
    idx[1] = torch.tensor([7, 300, 7, 383])   # same index, opposite: cancels
    plus[1] = torch.tensor([1, 0, 0, 0])
    idx[2] = torch.tensor([0, 0, 0, 0])       # four on one index: -2
    plus[2] = torch.tensor([0, 0, 0, 0])
    feats = ((idx << 1) | plus).to(torch.int32)
    pos_ids = torch.randint(0, P, (R,), generator=g, device=DEV).int()
    pos_table = torch.randn(P, D, generator=g, device=DEV) * 0.02
    x = torch.full((R, D), float("nan"), dtype=BF, device=DEV)
    ops.encoder_embed(x, feats, pos_ids, pos_table)
    expect = ref.encoder_embed_ref(feats, pos_ids, pos_table)
    assert torch.equal(x, expect)
    base = pos_table[pos_ids.long()]
    assert float(x[0, 5]) == float((base[0, 5] + 1.0).to(BF))
    assert float(x[1, 7]) == float(base[1, 7].to(BF))
    assert float(x[2, 0]) == float((base[2, 0] - 2.0).to(BF))


def test_embed_matches_piece_vector():
    """The integer features are the draws of _piece_vector."""
    from room_amd.memory.encoder import _piece_vector, piece_features
    pieces = ["deploy", "##ing", "x", "<empty>", "producti~"]
    feats = _i32([piece_features(p) for p in pieces])
    pos_table = torch.zeros(1, D, device=DEV)
    x = torch.empty(len(pieces), D, dtype=BF, device=DEV)
    ops.encoder_embed(x, feats, _i32([0] * len(pieces)), pos_table)
    expect = torch.stack([_piece_vector(p) for p in pieces]).to(BF)
    assert torch.equal(x.cpu(), expect)


# ------------------------------------------------------------------ gelu

def test_gelu():
    ramp = torch.linspace(-6.0, 6.0, 1536 * 7 - 8)
    special = torch.tensor([0.0, -0.0, 8.0, -8.0, 1.0, -1.0, 0.5, -0.5])
    u = torch.cat([special, ramp]).to(BF).to(DEV).view(7, 1536)
    expect = ref.gelu_ref(u)
    got = ops.gelu_(u.clone())
    err = (got.float() - expect.float()).abs().max()
    print(f"gelu_ max |err| {float(err):.3e}")
    # two bf16 ulps
    assert torch.allclose(got.float(), expect.float(), rtol=2 ** -7, atol=1e-5)


# ------------------------------------------------------------------ pool

def test_pool():
    g = torch.Generator(device=DEV)
    g.manual_seed(52)
    lens = [1, 16, 17, 128]
    cu = _cu(lens)
    h = torch.randn(cu[-1], D, generator=g, device=DEV).to(BF)
    mu = 0.1 * torch.randn(D, generator=g, device=DEV)

    def pool(rows, cu_):
        out = torch.full((len(cu_) - 1, D), float("nan"), device=DEV)
        return ops.encoder_pool(out, rows, _i32(cu_), mu, cu_rows_host=cu_)

    out = pool(h, cu)
    expect = ref.encoder_pool_ref(h, cu, mu)
    err = (out - expect).abs().max()
    print(f"encoder_pool max |err| {float(err):.3e}")
    # f32 summation order over at most 128 terms, 10x allowance
    assert torch.allclose(out, expect, atol=1e-4, rtol=0)
    assert torch.allclose(out.norm(dim=-1), torch.ones(4, device=DEV), atol=1e-5)
    for b, (lo, hi) in enumerate(zip(cu, cu[1:])):
        assert torch.equal(pool(h[lo:hi].contiguous(), [0, hi - lo])[0], out[b])
    raw = torch.empty(4, D, device=DEV)
    ops.encoder_pool(raw, h, _i32(cu), mu, cu_rows_host=cu, normalize=False)
    assert torch.allclose(raw, ref.encoder_pool_ref(h, cu, mu, normalize=False),
                          atol=1e-5, rtol=0)
    with pytest.raises(RuntimeError):
        ops.encoder_pool(out, h, _i32([0, cu[-1] - 1]), mu)
    with pytest.raises(RuntimeError):
        ops.encoder_pool(out, h.float(), _i32(cu), mu)


# ----------------------------------------------------------- projections

def _proj(x, w):
    R = x.size(0)
    ident = torch.arange(R, dtype=torch.int32, device=DEV)
    desc = ops.moe_build_desc_device(
        torch.zeros(R, dtype=torch.int32, device=DEV), 1, bm=16)
    out = torch.full((R, w.size(1)), float("nan"), dtype=BF, device=DEV)
    return ops.moe_grouped_gemm_skinny(out, x, w, ident, desc)


@pytest.mark.parametrize("K,N", [(384, 1152), (384, 384), (384, 1536),
                                 (1536, 384)])
def test_projection_shapes(K, N):
    """The encoder's four projections: one "expert", identity pair map,
    16-row tiles. Values and bound of test_skinny_random."""
    g = torch.Generator(device=DEV)
    g.manual_seed(53 + K + N)
    x = (torch.randn(130, K, generator=g, device=DEV) * 0.3).to(BF)
    w = (torch.randn(1, N, K, generator=g, device=DEV) * 0.05).to(BF)
    expect = (x.float() @ w[0].float().T).to(BF)
    outs = {}
    for R in (1, 16, 17, 130):
        outs[R] = _proj(x[:R].contiguous(), w)
        assert torch.allclose(outs[R].float(), expect[:R].float(),
                              atol=6e-2, rtol=6e-2), R
    # row independence: a row of the 130-row run equals the same row alone
    for r in (0, 15, 16, 77, 129):
        assert torch.equal(_proj(x[r:r + 1].contiguous(), w)[0], outs[130][r]), r
    assert torch.equal(outs[17], outs[130][:17])
