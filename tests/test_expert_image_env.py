"""ROOMAMD_EXPERT_IMAGE parsing and the model's expert_image argument checks,
none of which needs a device."""
import pytest

from room_amd.engine import llm
from room_amd.engine.llm import expert_image_from_env
from room_amd.models.qwen3_moe import (Qwen3MoEConfig, Qwen3MoELayer,
                                       Qwen3MoEModel)


def test_expert_image_from_env():
    assert expert_image_from_env({}) is True
    assert expert_image_from_env({"ROOMAMD_EXPERT_IMAGE": ""}) is True
    assert expert_image_from_env({"ROOMAMD_EXPERT_IMAGE": "1"}) is True
    assert expert_image_from_env({"ROOMAMD_EXPERT_IMAGE": "0"}) is False
    assert expert_image_from_env({"ROOMAMD_EXPERT_IMAGE": " 0 "}) is False
    assert expert_image_from_env({"ROOMAMD_EXPERT_IMAGE": " 1\n"}) is True
    assert expert_image_from_env({"ROOMAMD_EXPERT_IMAGE": "  "}) is True


@pytest.mark.parametrize("bad", ["yes", "no", "true", "2", "00", "fp8", "-1"])
def test_expert_image_from_env_rejects(bad):
    with pytest.raises(ValueError, match="ROOMAMD_EXPERT_IMAGE"):
        expert_image_from_env({"ROOMAMD_EXPERT_IMAGE": bad})


def test_expert_image_reads_the_process_environment(monkeypatch):
    monkeypatch.setenv("ROOMAMD_EXPERT_IMAGE", "0")
    assert expert_image_from_env() is False
    monkeypatch.delenv("ROOMAMD_EXPERT_IMAGE")
    assert expert_image_from_env() is True


def test_llm_exports_it_next_to_the_dtype_switch():
    assert llm.expert_image_from_env is expert_image_from_env
    assert hasattr(llm, "expert_dtype_from_env")


def test_model_refuses_bf16_without_image_before_touching_a_device():
    """The argument check stands before the first allocation, so it runs on
    a machine without a GPU (the device named here is never used)."""
    cfg = Qwen3MoEConfig.tiny()
    with pytest.raises(ValueError, match="expert_image"):
        Qwen3MoEModel(cfg, "cuda", expert_dtype="bf16", expert_image=False)
    with pytest.raises(ValueError, match="expert_image"):
        Qwen3MoEModel(cfg, "cuda", expert_image=False)
    with pytest.raises(ValueError, match="expert_image"):
        Qwen3MoELayer(cfg, "cuda", None, "bf16", expert_image=False)
    with pytest.raises(ValueError, match="expert_dtype"):
        Qwen3MoEModel(cfg, "cuda", expert_dtype="fp4", expert_image=False)
