"""Block-scaled e4m3 quantiser of the fp8 expert-weight mode (CPU): format,
power-of-two scales, exactness of the bf16 image, the error bound, and the
engine's ROOMAMD_EXPERT_DTYPE parsing."""
import pytest
import torch

from room_amd.engine.llm import expert_dtype_from_env
from room_amd.ops.reference import dequantize_fp8_block, quantize_fp8_block


def _gauss():
    g = torch.Generator().manual_seed(11)
    return torch.empty(4, 256, 512).normal_(0, 0.02, generator=g)


def _ints():
    """Integers in -8..8 times one power of two (2^-6..2^2) per 128x128
    block: every value is an e4m3 number times a power of two."""
    g = torch.Generator().manual_seed(12)
    w = torch.randint(-8, 9, (4, 256, 512), generator=g).float()
    f = torch.ldexp(torch.ones(4, 2, 4),
                    torch.randint(-6, 3, (4, 2, 4), generator=g))
    return w * f.repeat_interleave(128, -2).repeat_interleave(128, -1)


@pytest.fixture(scope="module", params=["gauss", "ints"])
def case(request):
    w = _gauss() if request.param == "gauss" else _ints()
    q, s = quantize_fp8_block(w)
    return w, q, s


def test_shapes_and_dtypes(case):
    w, q, s = case
    assert q.dtype == torch.float8_e4m3fn and q.shape == w.shape
    assert s.dtype == torch.float32 and s.shape == (4, 2, 4)
    qb, sb = quantize_fp8_block(w.to(torch.bfloat16))
    assert qb.dtype == torch.float8_e4m3fn and sb.shape == (4, 2, 4)
    assert not q.float().isnan().any()


def test_dequantised_values_are_bf16_exact(case):
    _, q, s = case
    deq = dequantize_fp8_block(q, s)
    assert deq.dtype == torch.float32
    assert torch.equal(deq.to(torch.bfloat16).float(), deq)


def test_requantising_is_idempotent(case):
    w, q, s = case
    # a block whose amax/scale lies in (224, 232) rounds down to 224 = 448/2
    # and would requantise with half the scale; the fixed inputs have none
    amax_q = w.reshape(4, 2, 128, 4, 128).abs().amax(dim=(2, 4)) / s
    assert not ((amax_q > 224) & (amax_q < 232)).any()
    deq = dequantize_fp8_block(q, s)
    for src in (deq, deq.to(torch.bfloat16)):
        q2, s2 = quantize_fp8_block(src)
        assert torch.equal(q2.view(torch.uint8), q.view(torch.uint8))
        assert torch.equal(s2, s)


def test_scales_are_powers_of_two(case):
    w, _, s = case
    m, _e = torch.frexp(s)
    assert (m == 0.5).all() and (s > 0).all()
    # the smallest power of two with amax/scale <= 448
    amax = w.reshape(4, 2, 128, 4, 128).abs().amax(dim=(2, 4))
    assert (amax / s <= 448).all()
    assert (amax / (s / 2) > 448).all()


def test_zero_block():
    w = _gauss()
    w[1, 128:, 256:384] = 0
    q, s = quantize_fp8_block(w)
    assert s[1, 1, 2] == 1.0
    deq = dequantize_fp8_block(q, s)
    assert (deq[1, 128:, 256:384] == 0).all()
    assert (quantize_fp8_block(torch.zeros(128, 128))[1] == 1.0).all()


def test_integer_tensor_round_trips():
    w = _ints()
    q, s = quantize_fp8_block(w)
    assert torch.equal(dequantize_fp8_block(q, s), w)


def test_gaussian_error_bound():
    # relative 2^-4 from e4m3's 3 mantissa bits (half an ulp of a normal);
    # absolute 2^-10·scale from the subnormal spacing 2^-9 (half of it)
    w = _gauss()
    q, s = quantize_fp8_block(w)
    deq = dequantize_fp8_block(q, s)
    se = s.repeat_interleave(128, -2).repeat_interleave(128, -1)
    bound = torch.maximum(w.abs() * 2.0 ** -4, se * 2.0 ** -10)
    err = (deq - w).abs()
    print(f"max err/bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("shape", [(128, 192), (100, 128), (2, 128, 130),
                                   (128,)])
def test_bad_shapes_raise(shape):
    with pytest.raises(ValueError):
        quantize_fp8_block(torch.zeros(*shape))


def test_bad_dtype_raises():
    with pytest.raises(ValueError):
        quantize_fp8_block(torch.zeros(128, 128, dtype=torch.float16))


def test_engine_env_parsing():
    assert expert_dtype_from_env({}) == "bf16"
    assert expert_dtype_from_env({"ROOMAMD_EXPERT_DTYPE": "bf16"}) == "bf16"
    assert expert_dtype_from_env({"ROOMAMD_EXPERT_DTYPE": "fp8"}) == "fp8"
    for bad in ("int8", "FP4", "fp8e5m2"):
        with pytest.raises(ValueError):
            expert_dtype_from_env({"ROOMAMD_EXPERT_DTYPE": bad})


def test_model_rejects_unknown_expert_dtype():
    from room_amd.models.qwen3_moe import Qwen3MoEConfig, Qwen3MoEModel
    with pytest.raises(ValueError):
        Qwen3MoEModel(Qwen3MoEConfig.tiny(), "cpu", expert_dtype="int8")
