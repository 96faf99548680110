"""flash_prefill's operand layout, element by element.

The kernel keeps Q, the scores and P in registers, reads K rows from a
swizzled LDS tile and reads V through transposed LDS reads of a differently
swizzled tile. A wrong swizzle or a wrong lane map in the transposed read
can be wrong on some rows or dims only, and the planted-key cases of
test_flash_prefill_long_gpu.py look at designated rows. Here every (position
within a chunk, dim) pair is identifiable and bits are asserted.

One-hot inputs: one sequence of 256 positions (four 64-position chunks, so
both K/V buffers are used twice), prefilled as 256 rows at positions 0..255.
q[p, h] is the same seeded randn bf16 vector for the 8 heads of a group and
K[p, hk] = 6 q of that group, so row p's own key wins its softmax by a gap
of at least 20 in the score (asserted on the CPU, `test_inputs_are_one_hot`):
the other keys' total weight is under 256 e^-20 < 2^-20, far below a bf16
half-ulp (2^-9). V[p, hk, d] = ((131 p + 7 d + 3 hk) mod 240) - 120 with the
values >= 0 moved up by one: nonzero integers of magnitude <= 120, exact in
bf16 (and 131 is a unit mod 240, so rows within a chunk all differ; rows 240
apart carry the same V row, which no mapping error inside a 64-position chunk
can exploit). Expected: out[p, h, :] is V[p, h // 8, :] bit for bit, which is
also what paged_attention_ref returns on these inputs (asserted on the CPU).

Cache blocks are handed out in shuffled order; block 0 and the blocks no
table entry names are NaN. Variants: tiles of 1, 5 and 27 rows (padded lanes
of a short tile against the transposed read), q as the strided view of a
packed buffer whose other columns are NaN, and the fp8 form against the bf16
form on the quantised image (V's integers survive e4m3 only approximately, so
the twin is the yardstick there, and the two must be bit-equal).
"""
import pytest
import torch

from room_amd import ops
from room_amd.ops import reference as ref

DEV = "cuda"
D, BS, GROUP = 128, 16, 8
T = 256
SCALE = D ** -0.5
SEED = 11
MIN_GAP = 20.0
SENTINEL = -1024.0
BF = torch.bfloat16
HEADS = [(16, 2), (32, 4)]


def gpu(fn):
    fn = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")(fn)
    return pytest.mark.gpu(fn)


_built = {}


def _inputs(hq, hk):
    """CPU tensors of the one-hot case at (hq, hk) heads, built once."""
    if (hq, hk) in _built:
        return _built[hq, hk]
    assert hq == hk * GROUP
    gen = torch.Generator().manual_seed(SEED)
    qdim, kvdim = hq * D, hk * D
    qv = torch.randn(T, hk, D, generator=gen).to(BF)
    buf = torch.full((T, qdim + 2 * kvdim), float("nan"), dtype=BF)
    buf[:, :qdim] = qv.repeat_interleave(GROUP, dim=1).reshape(T, qdim)
    q_packed = buf[:, :qdim].view(T, hq, D)
    k = (6.0 * qv.float()).to(BF)                                # [T, hk, D]
    p = torch.arange(T).view(T, 1, 1)
    h = torch.arange(hk).view(1, hk, 1)
    d = torch.arange(D).view(1, 1, D)
    v = (131 * p + 7 * d + 3 * h) % 240 - 120
    v = (v + (v >= 0)).to(BF)                                    # [T, hk, D]
    nblk = T // BS
    nb = nblk + 1 + 3                # block 0 and three blocks never named
    perm = torch.randperm(nb - 1, generator=gen) + 1
    bt = perm[:nblk].int().view(1, nblk)
    kc = torch.full((nb, hk, BS, D), float("nan"), dtype=BF)
    vc = torch.full((nb, hk, BS, D), float("nan"), dtype=BF)
    own = bt[0].long()
    kc[own] = k.view(nblk, BS, hk, D).transpose(1, 2)
    vc[own] = v.view(nblk, BS, hk, D).transpose(1, 2)
    # the fp8 cache of the same rows and its bf16 image; unnamed blocks NaN
    (kq, ks), (vq, vs) = ref.quantize_kv_rows(k), ref.quantize_kv_rows(v)
    ki = ref.dequantize_kv_rows(kq, ks).to(BF)
    vi = ref.dequantize_kv_rows(vq, vs).to(BF)

    def pool(rows, fill, dtype, tail):
        t = torch.full((nb, hk, BS) + tail, fill, dtype=torch.float32).to(dtype)
        rows = rows.view((nblk, BS, hk) + tail).transpose(1, 2)
        if dtype == torch.float8_e4m3fn:     # indexed stores go through bytes
            t.view(torch.uint8)[own] = rows.contiguous().view(torch.uint8)
        else:
            t[own] = rows
        return t

    nan = float("nan")
    _built[hq, hk] = dict(
        hq=hq, hk=hk, q=q_packed.contiguous(), q_packed=q_packed, k=k, v=v,
        kc=kc, vc=vc, bt=bt, own=own,
        seq_ids=torch.zeros(T, dtype=torch.int32),
        q_pos=torch.arange(T, dtype=torch.int32),
        kq=pool(kq, nan, torch.float8_e4m3fn, (D,)),
        vq=pool(vq, nan, torch.float8_e4m3fn, (D,)),
        ks=pool(ks, nan, torch.float32, ()),
        vs=pool(vs, nan, torch.float32, ()),
        ki=pool(ki, nan, BF, (D,)), vi=pool(vi, nan, BF, (D,)),
        want=v.repeat_interleave(GROUP, dim=1))                  # [T, hq, D]
    return _built[hq, hk]


def _bits(x):
    return x.contiguous().view(torch.int16)


# --------------------------------------------------------------- CPU tests

@pytest.mark.parametrize("hq,hk", HEADS)
def test_inputs_are_one_hot(hq, hk):
    """Without a GPU: the reference returns V's own row exactly, and every
    row's own score leads every other visible score by at least 20, so a
    change of seed cannot quietly make the bit assertions vacuous."""
    i = _inputs(hq, hk)
    assert i["v"].float().abs().min() >= 1 and i["v"].float().abs().max() <= 120
    assert torch.equal(i["v"].float(), i["v"].float().round())
    assert i["q_packed"].stride(0) == (hq + 2 * hk) * D
    assert torch.isnan(i["kc"][0].float()).all()
    assert sorted(i["bt"][0].tolist()) != i["bt"][0].tolist()
    # one q head per group is enough for the gap: the 8 heads are equal
    q = i["q"][:, ::GROUP].float()                               # [T, hk, D]
    assert torch.equal(i["q"], i["q"][:, ::GROUP].repeat_interleave(GROUP, 1))
    scores = torch.einsum("phd,khd->hpk", q, i["k"].float()) * SCALE
    own = scores.diagonal(dim1=1, dim2=2)                        # [hk, T]
    hidden = torch.ones(T, T).triu(0).bool()     # the diagonal and the future
    others = scores.masked_fill(hidden, float("-inf")).amax(-1)
    gap = (own - others)[:, 1:].min().item()     # row 0 sees its own key only
    print(f"heads {hq},{hk}: smallest gap {gap:.1f}, largest score "
          f"{scores.masked_fill(hidden.triu(1), 0).max().item():.0f}")
    assert gap >= MIN_GAP
    got = ref.paged_attention_ref(i["q"], i["kc"], i["vc"], i["bt"],
                                  i["seq_ids"], i["q_pos"], SCALE)
    assert got.dtype == BF
    assert torch.equal(_bits(got), _bits(i["want"]))


# --------------------------------------------------------------- GPU tests

def _tiles(n):
    return [(r, min(n, T - r)) for r in range(0, T, n)]


def _launch(i, q, kc, vc, tiles, **scales):
    desc = torch.tensor(tiles, dtype=torch.int32, device=DEV).view(-1, 2)
    out = torch.full((T, i["hq"], D), SENTINEL, dtype=BF, device=DEV)
    ops.flash_prefill(out, q, kc.to(DEV), vc.to(DEV), i["bt"].to(DEV),
                      i["seq_ids"].to(DEV), i["q_pos"].to(DEV), desc, SCALE,
                      **{n: s.to(DEV) for n, s in scales.items()})
    return out.cpu()


def _packed_q(i):
    qdim = i["hq"] * D
    q = i["q_packed"]
    buf = torch.as_strided(q, (T, qdim + 2 * i["hk"] * D),
                           (q.stride(0), 1)).to(DEV)
    assert torch.isnan(buf[:, qdim:].float()).all()
    return buf[:, :qdim].view(T, i["hq"], D)


def _assert_rows(got, want, what):
    bad = (_bits(got) != _bits(want))
    assert not bad.any(), (
        f"{what}: {int(bad.sum())} elements differ, first (row, head, dim) "
        f"{bad.nonzero()[0].tolist()}, rows {bad.any(-1).any(-1).sum().item()}")


@gpu
@pytest.mark.parametrize("hq,hk", HEADS)
def test_one_hot_full_tiles(hq, hk):
    i = _inputs(hq, hk)
    tiles = ops.build_qtile_desc([(0, T)], "cpu").tolist()
    assert tiles == [list(t) for t in _tiles(32)]
    got = _launch(i, i["q"].to(DEV), i["kc"], i["vc"], tiles)
    _assert_rows(got, i["want"], "full tiles")


@gpu
@pytest.mark.parametrize("n", [1, 5, 27])
@pytest.mark.parametrize("hq,hk", HEADS)
def test_one_hot_short_tiles(hq, hk, n):
    i = _inputs(hq, hk)
    got = _launch(i, i["q"].to(DEV), i["kc"], i["vc"], _tiles(n))
    _assert_rows(got, i["want"], f"tiles of {n}")


@gpu
@pytest.mark.parametrize("hq,hk", HEADS)
def test_one_hot_packed_q(hq, hk):
    i = _inputs(hq, hk)
    q = _packed_q(i)
    assert q.stride(0) == (hq + 2 * hk) * D
    for n in (32, 5):
        got = _launch(i, q, i["kc"], i["vc"], _tiles(n))
        _assert_rows(got, i["want"], f"packed q, tiles of {n}")


@gpu
@pytest.mark.parametrize("hq,hk", HEADS)
def test_one_hot_fp8_twin(hq, hk):
    """The fp8 form on the quantised cache and the bf16 form on its image:
    bit-equal, at full and at short tiles."""
    i = _inputs(hq, hk)
    q = i["q"].to(DEV)
    for n in (32, 27, 5):
        f8 = _launch(i, q, i["kq"], i["vq"], _tiles(n),
                     k_scale=i["ks"], v_scale=i["vs"])
        twin = _launch(i, q, i["ki"], i["vi"], _tiles(n))
        assert not torch.isnan(twin.float()).any()
        assert not (twin == SENTINEL).any()
        _assert_rows(f8, twin, f"fp8 against its bf16 twin, tiles of {n}")
