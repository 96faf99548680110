"""Split-KV decode attention past one 32-position chunk per split.

A split of `paged_attention_split` covers more than 32 positions once the
context is above 32 * splits tokens (1024 at 32 splits, 2048 at 64). Plain
randn inputs cannot tell whether the kernel reads those positions: at a
context in the thousands the softmax weights are diffuse, the output is about
+-0.03 per element, and a kernel that scores each split's first 32 positions
over and over lands inside atol = 3e-2 of the truth. So the main cases plant,
for every (sequence, q head), one key at a position that is NOT among the
first 32 of its split: K there is 1.5 * q_head, which scores about 17 against
N(0, 1) elsewhere, so nearly all softmax mass sits on one randn V row of
magnitude about 1. `test_planted_inputs_discriminate` checks on the CPU that
the inputs really have that property.

Reference: ops.reference.paged_attention_ref (fp32 math). Tolerance: the
project's atol = 3e-2 plus rtol = 2^-7; the relative part covers the bf16
half-ulp roundings of P and of the output (2^-9 each, and one more for the
reference's own bf16 result), which matter at outputs of magnitude 1 to 4.
"""
import pytest
import torch

from room_amd import ops
from room_amd.ops import reference as ref

DEV = "cuda"
HQ, HK, D, BS = 32, 4, 128, 16
GROUP = HQ // HK
CHUNK = 32
SCALE = D ** -0.5
BETA = 1.5
ATOL, RTOL = 3e-2, 2.0 ** -7


def gpu(fn):
    fn = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")(fn)
    return pytest.mark.gpu(fn)


# name -> (context lengths, splits). Spans (positions per split) at 32 splits:
# 1, 33, 1024 -> 32 (one chunk; 1 and 33 leave most splits empty; 33 has a
# one-position last tile); 1025 -> 64 with a one-position last split;
# 1500, 2048 -> 64; 2049 -> 96; 4000 -> 128; 4097 -> 160 (5 chunks, ragged
# last chunk); 8200 -> 288 (9 chunks, ragged last tile). At 64 splits:
# 2049 -> 64, 4097 -> 96, 8200 -> 160.
CASES = {
    "short32": ([1, 33, 1024, 1025], 32),
    "mid32": ([1500, 2048, 2049, 4097], 32),
    "long32": ([8200, 4000], 32),
    "band64": ([2049, 4097, 8200], 64),
}


def _span(L, nsp):
    return ((L + nsp - 1) // nsp + CHUNK - 1) // CHUNK * CHUNK


def _first_chunk_mask(L, nsp):
    """True at the positions a kernel sees that only ever reads the first
    CHUNK positions of every split."""
    pos = torch.arange(L)
    return (pos % _span(L, nsp)) < CHUNK


def _plant_positions(L, nsp, gen):
    """8 positions per kv head, one per q head of the group, outside the
    first chunk of their split wherever the context allows it."""
    span = _span(L, nsp)
    cand = (~_first_chunk_mask(L, nsp)).nonzero().flatten()
    if cand.numel() == 0:              # one chunk per split: anywhere
        cand = torch.arange(L)
    out = torch.empty(HK, GROUP, dtype=torch.long)
    for hk in range(HK):
        if cand.numel() >= GROUP:
            pick = cand[torch.randperm(cand.numel(), generator=gen)[:GROUP]]
        else:
            pick = cand[torch.randint(cand.numel(), (GROUP,), generator=gen)]
        out[hk] = pick
    if cand.numel() >= GROUP:
        # kv head 0, q head 0: the last valid position (or the last candidate)
        last = cand[-1]
        out[0, 0] = last
        # kv head 0, q head 1: last chunk of the first split
        tail = cand[(cand < span) & (cand >= span - CHUNK)]
        if tail.numel():
            out[0, 1] = tail[-1]
        # keep kv head 0's positions distinct
        seen = set()
        for h in range(GROUP):
            p = int(out[0, h])
            while p in seen:
                p = int(cand[torch.randint(cand.numel(), (1,), generator=gen)])
            seen.add(p)
            out[0, h] = p
    return out


def _build(lens, nsp, seed, planted):
    """CPU tensors: q, kcache, vcache, block_table, seq_ids, q_pos. Blocks are
    handed out in shuffled order; rows past a sequence's end hold NaN, as an
    uninitialised cache may."""
    gen = torch.Generator().manual_seed(seed)
    T = len(lens)
    nblk = [(L + BS - 1) // BS for L in lens]
    nb = sum(nblk) + 1
    q = torch.randn(T, HQ, D, generator=gen).to(torch.bfloat16)
    kc = torch.randn(nb, HK, BS, D, generator=gen).to(torch.bfloat16)
    vc = torch.randn(nb, HK, BS, D, generator=gen).to(torch.bfloat16)
    perm = torch.randperm(nb - 1, generator=gen) + 1
    bt = torch.zeros(T, max(nblk), dtype=torch.int32)
    at = 0
    for t, L in enumerate(lens):
        blocks = perm[at:at + nblk[t]]
        at += nblk[t]
        bt[t, :nblk[t]] = blocks.int()
        if planted:
            where = _plant_positions(L, nsp, gen)
            for hk in range(HK):
                for h in range(GROUP):
                    p = int(where[hk, h])
                    kc[blocks[p // BS], hk, p % BS] = \
                        (BETA * q[t, hk * GROUP + h].float()).to(torch.bfloat16)
        tail = L % BS
        if tail:
            kc[blocks[-1], :, tail:] = float("nan")
            vc[blocks[-1], :, tail:] = float("nan")
    seq_ids = torch.arange(T, dtype=torch.int32)
    q_pos = torch.tensor([L - 1 for L in lens], dtype=torch.int32)
    return q, kc, vc, bt, seq_ids, q_pos


def _masked_ref(inputs, lens, nsp):
    """fp32 attention over each split's first CHUNK positions only."""
    q, kc, vc, bt, _, _ = inputs
    out = torch.zeros(len(lens), HQ, D)
    for t, L in enumerate(lens):
        blocks = bt[t, :(L + BS - 1) // BS].long()
        k = kc[blocks].transpose(0, 1).reshape(HK, -1, D)[:, :L].float()
        v = vc[blocks].transpose(0, 1).reshape(HK, -1, D)[:, :L].float()
        keep = _first_chunk_mask(L, nsp)
        s = torch.einsum("khd,kld->khl", q[t].float().view(HK, GROUP, D), k) * SCALE
        s = s.masked_fill(~keep, float("-inf"))
        out[t] = torch.einsum("khl,kld->khd", torch.softmax(s, -1), v).reshape(HQ, D)
    return out


_built = {}


def _inputs(name, planted=True):
    key = (name, planted)
    if key not in _built:
        lens, nsp = CASES[name]
        seed = 100 + sorted(CASES).index(name)
        _built[key] = _build(lens, nsp, seed, planted)
    return _built[key]


def _run(inputs, nsp):
    q, kc, vc, bt, seq_ids, q_pos = (x.to(DEV) for x in inputs)
    T = q.size(0)
    stride = ops.attn_nsplits()
    # NaN-filled: a partial the kernel fails to write poisons the merge
    part = torch.full((T, HQ, stride, D), float("nan"), device=DEV)
    part_ml = torch.full((T, HQ, stride, 2), float("nan"), device=DEV)
    out = torch.empty_like(q)
    ops.paged_attention_split(out, q, kc, vc, bt, seq_ids, q_pos, part, part_ml,
                              SCALE, splits=nsp)
    expect = ref.paged_attention_ref(q, kc, vc, bt, seq_ids, q_pos, SCALE)
    return out, expect, part[:, :, :nsp], part_ml[:, :, :nsp]


def _check(out, expect, lens):
    err = (out.float() - expect.float()).abs()
    for t, L in enumerate(lens):
        print(f"L={L}: max-abs err {err[t].max().item():.4f}, "
              f"max |expect| {expect[t].float().abs().max().item():.3f}")
    assert torch.allclose(out.float(), expect.float(), atol=ATOL, rtol=RTOL)


@pytest.mark.parametrize("name", sorted(CASES))
def test_planted_inputs_discriminate(name):
    """Property of the inputs, checked on the CPU: attention over each
    split's first 32 positions only is far from the full result for every
    sequence whose splits are longer than one chunk."""
    lens, nsp = CASES[name]
    inputs = _inputs(name)
    q, kc, vc, bt, seq_ids, q_pos = inputs
    full = ref.paged_attention_ref(q, kc, vc, bt, seq_ids, q_pos, SCALE).float()
    first = _masked_ref(inputs, lens, nsp)
    multi = [t for t, L in enumerate(lens) if _span(L, nsp) > CHUNK]
    assert multi, "case has no sequence past one chunk per split"
    for t in multi:
        gap = (full[t] - first[t]).abs().max().item()
        assert gap > 0.3, f"L={lens[t]}: gap {gap:.3f}, inputs too weak"
    for t in set(range(len(lens))) - set(multi):
        assert torch.allclose(full[t], first[t], atol=1e-2)


@gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_split_attention_planted(name):
    lens, nsp = CASES[name]
    out, expect, _, _ = _run(_inputs(name), nsp)
    _check(out, expect, lens)


@gpu
def test_split_attention_randn_diffuse():
    """The diffuse regime: plain randn K, outputs of about +-0.03."""
    lens, nsp = CASES["mid32"]
    out, expect, _, _ = _run(_inputs("mid32", planted=False), nsp)
    _check(out, expect, lens)


@gpu
def test_split_attention_wide_grid():
    """T = 16 at contexts 40 to 300: the wide decode path's grid, where most
    splits are empty and at most two of a workgroup's four waves have a tile."""
    lens = [40 + (260 * i) // 15 for i in range(16)]
    out, expect, _, _ = _run(_build(lens, 32, 7, planted=False), 32)
    _check(out, expect, lens)


@gpu
def test_split_attention_deterministic():
    lens, nsp = CASES["mid32"]
    a = _run(_inputs("mid32"), nsp)
    b = _run(_inputs("mid32"), nsp)
    for x, y in zip(a, b):          # out, expect, part, part_ml: bit-equal
        bits = torch.int16 if x.dtype == torch.bfloat16 else torch.int32
        assert torch.equal(x.contiguous().view(bits), y.contiguous().view(bits))
