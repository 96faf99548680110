"""The argument contract of every op wrapper (csrc/checks.h), without a launch.

Everything here runs under ops.check_only(): a wrapper returns after its
checks, so a check that is missing shows as "no error raised" and never as a
kernel run on a bad shape, and the tensors may live on the CPU. For every op
the minimal valid arguments of op_contract_cases.py must pass, and every
single-field mutation of every tensor argument (dtype, a non-contiguous view,
each checked size off by one, rank + 1 and - 1, the other device) must raise
a RuntimeError that names the op and the argument.
"""
import re

import pytest
import torch

from room_amd import ops
from op_contract_cases import A, BF, CASES, F16, F32, F64, FP8, I32, I64, \
    NOT_OPS, build, op_of

_C = ops._C
pytestmark = pytest.mark.skipif(_C is None, reason="room_amd._C is not built")

DEV = "cuda" if torch.cuda.is_available() else "cpu"
OTHER = "cpu" if DEV == "cuda" else None      # a second device, if there is one
WRONG = {BF: F16, F32: F64, I32: I64, I64: I32, FP8: BF}


def _strided(a: A):
    """a's shape and dtype as a view with a gap after every innermost run."""
    if len(a.shape) == 1:
        return torch.zeros(2 * a.shape[0]).to(a.dtype).to(DEV)[::2]
    wide = a.shape[:-1] + (2 * a.shape[-1],)
    return torch.zeros(wide).to(a.dtype).to(DEV)[..., :a.shape[-1]]


def _mutations(a: A):
    """(label, tensor) for every single-field mutation of one argument."""
    yield "dtype", a.make(DEV, dtype=WRONG[a.dtype])
    view = _strided(a)
    if not view.is_contiguous():        # a size-1 tensor is always contiguous
        yield "non-contiguous", view
    for d, delta in a.dims:
        shape = list(a.shape)
        shape[d] += delta
        yield f"size({d}) {delta:+d}", a.make(DEV, shape=shape)
    if a.rank:
        yield "rank + 1", a.make(DEV).unsqueeze(0)
        yield "rank - 1", (a.make(DEV).flatten(0, 1) if len(a.shape) > 1
                           else a.make(DEV, shape=()))
    if OTHER is not None:
        yield "other device", a.make(OTHER)


def _tensor_args():
    for case, args in CASES.items():
        for i, (name, v) in enumerate(args):
            if isinstance(v, A):
                yield pytest.param(case, i, name, v, id=f"{case}-{name}")


def test_table_covers_every_binding():
    bound = {n for n in dir(_C) if not n.startswith("_")}
    assert bound == {op_of(c) for c in CASES} | NOT_OPS
    assert not ops._C.check_only()          # off unless a test turns it on


@pytest.mark.parametrize("case", CASES)
def test_valid_arguments_pass(case):
    with ops.check_only():
        getattr(_C, op_of(case))(*build(case, DEV))


@pytest.mark.parametrize("case,i,name,a", _tensor_args())
def test_every_mutation_is_refused(case, i, name, a):
    op = getattr(_C, op_of(case))
    good = build(case, DEV)
    # check-only mode asks for one device, not for the GPU: an op with a
    # single tensor has no second one to disagree with
    alone = sum(isinstance(v, A) for _, v in CASES[case]) == 1
    n = 0
    with ops.check_only():
        for label, bad in _mutations(a):
            if alone and label == "other device":
                continue
            args = good[:i] + [bad] + good[i + 1:]
            with pytest.raises(RuntimeError) as e:
                op(*args)
                pytest.fail(f"{case} accepted {name} with {label}")
            msg = str(e.value).splitlines()[0]
            assert op_of(case) + ":" in msg, (label, msg)
            assert re.search(rf"\b{name}\b", msg), (label, msg)
            n += 1
    assert n >= 2       # dtype and at least one of shape / layout


def test_q_may_be_a_row_view_of_the_packed_qkv():
    """The one layout besides contiguous that an op takes: the attention
    ops' q as rows of the packed qkv buffer."""
    for case in ("paged_attention", "paged_attention_split", "flash_prefill"):
        args = build(case, DEV)
        names = [n for n, _ in CASES[case]]
        q = args[names.index("q")]
        T, hq, d = q.shape
        packed = torch.zeros(T, (hq + 2) * d, dtype=BF, device=DEV)
        args[names.index("q")] = packed[:, :hq * d].view(T, hq, d)
        with ops.check_only():
            getattr(_C, case)(*args)
            args[names.index("q")] = packed[:, 4:hq * d + 4].view(T, hq, d)
            with pytest.raises(RuntimeError, match=rf"{case}: q\b"):
                getattr(_C, case)(*args)      # rows off the 16-byte grid


def test_scalar_arguments_are_checked():
    def call(case, **over):
        args = [over.get(n, v) for (n, _), v in zip(CASES[case], build(case, DEV))]
        getattr(_C, op_of(case))(*args)

    bad = [("moe_router", dict(K=0)), ("moe_router", dict(K=9)),
           ("router_gemv_topk", dict(K=17)), ("router_norm_gemv_topk", dict(K=0)),
           ("paged_attention_split", dict(splits=48)),
           ("qk_norm_rope", dict(head_dim=64)),
           ("moe_build_desc", dict(bm=129)), ("moe_build_desc", dict(bm=0)),
           ("vs_topk", dict(K=65)), ("vs_topk_scoped", dict(K=0)),
           ("hist_append", dict(kmax=3)), ("qk_rope_write_kv", dict(n_qheads=7))]
    with ops.check_only():
        for case, over in bad:
            with pytest.raises(RuntimeError, match=op_of(case) + ":"):
                call(case, **over)
                pytest.fail(f"{case} accepted {over}")


@pytest.mark.skipif(torch.cuda.is_available(), reason="host has a GPU")
@pytest.mark.parametrize("case", CASES)
def test_cpu_tensors_are_refused_outside_check_only(case):
    assert not _C.check_only()
    with pytest.raises(RuntimeError, match=op_of(case) + ":.*must be on the GPU"):
        getattr(_C, op_of(case))(*build(case, "cpu"))
