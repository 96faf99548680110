"""The valid arguments of test_op_contracts.py, launched: every op accepts its
minimal contract on the GPU, runs and completes. Numerics are the other
suites' job. Also: check-only mode set and cleared leaves the ops working."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from room_amd import ops
    from op_contract_cases import CASES, build, op_of
else:
    pytest.skip("no GPU", allow_module_level=True)

DEV = "cuda"


def test_every_op_launches_on_its_minimal_arguments():
    assert not ops._C.check_only()
    for case in CASES:
        getattr(ops._C, op_of(case))(*build(case, DEV))
    torch.cuda.synchronize()


def test_check_only_cleared_leaves_ops_launching():
    x = torch.randn(2, 512, device=DEV).bfloat16()
    w = torch.ones(512, dtype=torch.bfloat16, device=DEV)
    out = torch.zeros_like(x)
    with ops.check_only():
        assert ops._C.check_only()
        ops.rmsnorm(out, x, w)
    torch.cuda.synchronize()
    assert not ops._C.check_only()
    assert (out == 0).all()              # checked, not launched
    ops.rmsnorm(out, x, w)
    torch.cuda.synchronize()
    assert (out != 0).any()
