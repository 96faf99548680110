"""Row-scaled e4m3 quantiser of the fp8 KV cache (CPU): format, power-of-two
scales, exactness of the bf16 image, the error bound, the edge rows, the
PagedKVCache(kv_dtype="fp8") allocation and the engine's ROOMAMD_KV_DTYPE
parsing."""
import pytest
import torch

from room_amd.engine.kv_cache import BLOCK_SIZE, PagedKVCache
from room_amd.engine.llm import kv_dtype_from_env
from room_amd.ops.reference import (KV_FP8_MIN_EXP, dequantize_kv_rows,
                                    quantize_kv_rows)

ROWS, D = 4096, 128


@pytest.fixture(scope="module")
def case():
    """4096 gaussian rows spread over 32 octaves of magnitude."""
    g = torch.Generator().manual_seed(20)
    x = torch.randn(ROWS, D, generator=g) * torch.exp2(
        torch.randint(-16, 16, (ROWS, 1), generator=g).float())
    q, s = quantize_kv_rows(x)
    return x, q, s


def test_shapes_and_dtypes(case):
    x, q, s = case
    assert q.dtype == torch.float8_e4m3fn and q.shape == x.shape
    assert s.dtype == torch.float32 and s.shape == (ROWS,)
    assert not q.float().isnan().any()
    # leading dimensions are kept; bf16 input gives what its f32 copy gives
    xb = x.view(ROWS // 64, 4, BLOCK_SIZE, D).to(torch.bfloat16)
    qb, sb = quantize_kv_rows(xb)
    assert qb.shape == xb.shape and sb.shape == xb.shape[:-1]
    assert torch.equal(qb.view(torch.uint8).view(ROWS, D), q.view(torch.uint8))
    assert torch.equal(sb.view(ROWS), s)
    with pytest.raises(ValueError):
        quantize_kv_rows(x.to(torch.float16))


def test_scales_are_the_smallest_fitting_powers_of_two(case):
    x, _, s = case
    m, _ = torch.frexp(s)
    assert torch.equal(m, torch.full_like(m, 0.5))
    amax = x.to(torch.bfloat16).float().abs().amax(-1)
    assert (amax <= 448 * s).all()           # nothing saturates
    assert (amax > 448 * (s / 2)).all()      # and half the scale would


def test_scaled_values_stay_within_e4m3(case):
    x, _, s = case
    assert (x.to(torch.bfloat16).float() / s[:, None]).abs().max() <= 448


def test_dequantised_values_are_bf16_exact(case):
    _, q, s = case
    deq = dequantize_kv_rows(q, s)
    assert deq.dtype == torch.float32 and deq.shape == q.shape
    assert torch.equal(deq.to(torch.bfloat16).float(), deq)


def test_error_bound(case):
    """e4m3 keeps 3 mantissa bits (half an ulp is 2^-4 relative) and its
    smallest subnormal step is 2^-9 (half of it 2^-10) times the scale."""
    x, q, s = case
    xb = x.to(torch.bfloat16).float()
    err = (xb - dequantize_kv_rows(q, s)).abs()
    assert (err <= torch.maximum(xb.abs() * 2.0 ** -4,
                                 s[:, None] * 2.0 ** -10)).all()


def test_edge_rows():
    r = torch.zeros(6, D)
    r[1, 5] = 448.0 * 8            # exactly 448 * 2^3: scale 8, byte 448
    r[2, 7] = -(448.0 * 8 + 16)    # one bf16 step above: scale 16, 225 -> 224
    r[3, 9] = 2.0 ** -80           # below the clamp
    r[4, 0] = 2.0 ** -133          # a bf16 subnormal
    r[5, 3], r[5, 4] = 448.0 * 2.0 ** -64, 2.0 ** -64    # at the clamp
    q, s = quantize_kv_rows(r)
    assert s[0] == 1.0 and not q[0].view(torch.uint8).any()
    assert s[1] == 8.0 and q[1, 5].float() == 448.0
    assert s[2] == 16.0 and q[2, 7].float() == -224.0
    clamp = 2.0 ** KV_FP8_MIN_EXP
    assert KV_FP8_MIN_EXP == -64
    assert s[3] == clamp and s[4] == clamp and s[5] == clamp
    assert not q[3].view(torch.uint8).any() and not q[4].view(torch.uint8).any()
    assert q[5, 3].float() == 448.0 and q[5, 4].float() == 1.0


def test_requantising_the_image():
    """Quantising the image returns the same bytes and scales, except where
    the format itself says otherwise: a row whose amax/scale lies in
    (224, 232] has its largest byte rounded down to 224 = 448/2 (e4m3 steps
    by 16 between 128 and 256, ties to even), so its image fits half the
    scale and requantises to the doubled bytes, which is the same image (the
    block quantiser's test notes the same band). The band comes from the
    number format, not from the quantiser's output; both kinds of row are
    among the 4096."""
    g = torch.Generator().manual_seed(20)
    x = torch.randn(ROWS, D, generator=g) * torch.exp2(
        torch.randint(-16, 16, (ROWS, 1), generator=g).float())
    q, s = quantize_kv_rows(x)
    top = x.to(torch.bfloat16).float().abs().amax(-1) / s
    band = (top > 224) & (top <= 232)
    assert band.any() and (~band).sum() > ROWS // 2
    deq = dequantize_kv_rows(q, s)
    for src in (deq, deq.to(torch.bfloat16)):
        q2, s2 = quantize_kv_rows(src)
        assert torch.equal(dequantize_kv_rows(q2, s2), deq)
        assert torch.equal(q2.view(torch.uint8)[~band],
                           q.view(torch.uint8)[~band])
        assert torch.equal(s2[~band], s[~band])
        assert torch.equal(s2[band] * 2, s[band])
        assert torch.equal(q2[band].float(), q[band].float() * 2)


# ------------------------------------------------------------ PagedKVCache

def _cache(kv_dtype):
    return PagedKVCache(num_layers=2, num_kv_heads=4, head_dim=D,
                        num_blocks=9, max_seqs=3, max_blocks_per_seq=4,
                        device=torch.device("cpu"), kv_dtype=kv_dtype)


def test_fp8_cache_tensors():
    c = _cache("fp8")
    assert c.kv_dtype == "fp8"
    for rows, scales in ((c.kcaches, c.kscales), (c.vcaches, c.vscales)):
        assert len(rows) == len(scales) == 2
        for r, s in zip(rows, scales):
            assert r.dtype == torch.float8_e4m3fn
            assert r.shape == (9, 4, BLOCK_SIZE, D)
            assert s.dtype == torch.float32 and s.shape == (9, 4, BLOCK_SIZE)
            assert r.is_contiguous() and s.is_contiguous()
    b = _cache("bf16")
    assert b.kv_dtype == "bf16" and b.kscales is None and b.vscales is None
    assert b.kcaches[0].dtype == torch.bfloat16
    assert _cache("bf16").kcaches[0].shape == c.kcaches[0].shape


def test_bytes_per_block():
    bf = PagedKVCache.bytes_per_block(48, 4, D)
    assert bf == PagedKVCache.bytes_per_block(48, 4, D, "bf16")
    assert bf == 48 * 2 * 4 * BLOCK_SIZE * D * 2
    f8 = PagedKVCache.bytes_per_block(48, 4, D, "fp8")
    assert f8 == 48 * 2 * 4 * BLOCK_SIZE * (D + 4)
    c = _cache("fp8")
    held = sum(t.numel() * t.element_size()
               for t in c.kcaches + c.vcaches + c.kscales + c.vscales)
    assert held == 9 * PagedKVCache.bytes_per_block(2, 4, D, "fp8")


def test_fp8_cache_block_bookkeeping():
    c, b = _cache("fp8"), _cache("bf16")
    for cache in (c, b):
        s0, s1 = cache.alloc_seq(), cache.alloc_seq()
        cache.ensure_capacity(s0, 17)
        cache.ensure_capacity(s1, 1)
        cache.ensure_capacity(s0, 33)
        assert cache.seq_nblocks[s0] == 3 and cache.seq_nblocks[s1] == 1
        with pytest.raises(RuntimeError, match="max length"):
            cache.ensure_capacity(s1, 4 * BLOCK_SIZE + 1)
        cache.free_seq(s0)
    assert torch.equal(c.block_table, b.block_table)
    assert c.free_blocks == b.free_blocks and c.free_slots == b.free_slots
    assert c.blocks_free() == 8 - 1


@pytest.mark.parametrize("bad", ["fp16", "int8", "", "FP8", None])
def test_bad_kv_dtype_raises(bad):
    with pytest.raises(ValueError, match="kv_dtype"):
        _cache(bad)
    with pytest.raises(ValueError, match="kv_dtype"):
        PagedKVCache.bytes_per_block(1, 1, D, bad)


def test_kv_dtype_from_env():
    assert kv_dtype_from_env({}) == "bf16"
    assert kv_dtype_from_env({"ROOMAMD_KV_DTYPE": ""}) == "bf16"
    assert kv_dtype_from_env({"ROOMAMD_KV_DTYPE": "bf16"}) == "bf16"
    assert kv_dtype_from_env({"ROOMAMD_KV_DTYPE": " fp8 "}) == "fp8"
    for bad in ("fp4", "FP8", "e4m3", "1"):
        with pytest.raises(ValueError, match="ROOMAMD_KV_DTYPE"):
            kv_dtype_from_env({"ROOMAMD_KV_DTYPE": bad})
