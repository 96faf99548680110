"""fp8 KV cache kernels: e4m3 rows with one f32 scale per row.

Contract (docs/KERNELS.md, "fp8 KV cache"): the image of an fp8 cache is the
bf16 cache holding bf16(f32(q) * scale) in every row, an exact conversion.
Every fp8 attention op must return output bit-equal to the same op on the
image, and the writer must store the bytes and scales that
reference.quantize_kv_rows gives for the rows the bf16 writer stores. So every
comparison here is torch.equal; there is no tolerance.

The block pool is filled end to end with quantize_kv_rows of random rows whose
magnitude follows a fixed power-of-two pattern over (block, head, row):
neighbouring rows, heads and blocks always differ in scale, so a wrong scale
index cannot pass. Block tables are permuted. Rows past a sequence's end in
its last block carry a NaN scale (a NaN row in the image): a kernel that
consumes a byte or a scale of a row it must not read gives NaN.
"""
import gc

import pytest
import torch

from room_amd import ops
from room_amd.ops import reference as ref

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU"),
]

DEV = "cuda"
D, BS, GROUP = 128, 16, 8
SCALE = D ** -0.5
BF, F8 = torch.bfloat16, torch.float8_e4m3fn
LENS = [1, 15, 16, 17, 33, 129, 1000, 4100, 16400]   # one sequence each


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _u8(t):
    return t.view(torch.uint8)


def _pattern(nb, hk):
    """Power-of-two exponent per (block, head, row), -3..3. Consecutive rows
    differ by 3 or 4 octaves, heads by 2 or 5, blocks by 1 or 6; the amax of
    128 gaussians moves a row's scale by at most two."""
    b = torch.arange(nb).view(-1, 1, 1)
    h = torch.arange(hk).view(1, -1, 1)
    r = torch.arange(BS).view(1, 1, -1)
    return ((b + 2 * h + 3 * r) % 7 - 3).float()


class Pool:
    def __init__(self, hk):
        g = torch.Generator().manual_seed(100 + hk)
        nblk = [(n + BS - 1) // BS for n in LENS]
        self.hk, self.nb, self.mb = hk, sum(nblk) + 1, max(nblk)
        mag = torch.exp2(_pattern(self.nb, hk)).unsqueeze(-1)
        self.kq, self.ks = self._fill(g, mag)
        self.vq, self.vs = self._fill(g, mag)
        for s in (self.ks, self.vs):          # the pattern does its job
            assert (s[:, :, 1:] != s[:, :, :-1]).all()
        perm = (torch.randperm(self.nb - 1, generator=g) + 1).tolist()
        bt = torch.zeros(len(LENS), self.mb, dtype=torch.int32)
        for i, n in enumerate(nblk):
            mine, perm = perm[:n], perm[n:]
            bt[i, :n] = torch.tensor(mine, dtype=torch.int32)
            tail = LENS[i] % BS
            if tail:                          # rows past the sequence's end
                self.ks[mine[-1], :, tail:] = float("nan")
                self.vs[mine[-1], :, tail:] = float("nan")
        self.bt = bt.to(DEV)
        self.ki = ref.dequantize_kv_rows(self.kq, self.ks).to(BF)
        self.vi = ref.dequantize_kv_rows(self.vq, self.vs).to(BF)

    def _fill(self, g, mag):
        x = torch.randn(self.nb, self.hk, BS, D, generator=g) * mag
        q, s = ref.quantize_kv_rows(x.to(DEV))
        return q.contiguous(), s.contiguous()

    def q(self, T, seed):
        """Query rows as the engine passes them: a view into packed qkv."""
        g = torch.Generator().manual_seed(seed)
        hq = self.hk * GROUP
        qkv = (torch.randn(T, (hq + 2 * self.hk) * D, generator=g) * 0.3
               ).to(BF).to(DEV)
        return qkv[:, :hq * D].view(T, hq, D)

    def fp8(self):
        return dict(kc=self.kq, vc=self.vq, ks=self.ks, vs=self.vs)

    def image(self):
        return dict(kc=self.ki, vc=self.vi, ks=None, vs=None)


@pytest.fixture(scope="module", params=[1, 4], ids=["hk1", "hk4"])
def pool(request):
    yield Pool(request.param)
    # hand the pool's memory back, so that later modules that measure
    # allocator statistics start from what they started from before
    gc.collect()
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- writer

def _writer_rows(T):
    """(seq, pos) per token. Positions 15, 16, 17 of sequence 0 cross a block
    boundary wherever T allows three rows of one sequence."""
    if T == 1:
        return [(0, 16)]
    if T == 5:
        return [(0, 15), (0, 16), (0, 17), (1, 0), (1, 40)]
    return [(0, p) for p in range(3, 31)] + [(1, p) for p in range(62, 67)]


@pytest.mark.parametrize("hk", [1, 4])
@pytest.mark.parametrize("T", [1, 5, 33])
def test_writer_stores_the_quantised_rows(T, hk):
    g = torch.Generator().manual_seed(7 * T + hk)
    hq, nb, mb = hk * GROUP, 10, 5
    rows = _writer_rows(T)
    assert len(rows) == T
    qkv = torch.randn(T, (hq + 2 * hk) * D, generator=g)
    # per-token magnitudes over 12 octaves: the V scales differ row to row
    qkv = qkv * torch.exp2(torch.randint(-6, 6, (T, 1), generator=g).float())
    qkv[0, (hq + hk) * D:(hq + hk + 1) * D] = 0       # an all-zero V row
    qkv = qkv.to(BF).to(DEV)
    q_w = (1 + 0.1 * torch.randn(D, generator=g)).to(BF).to(DEV)
    k_w = (1 + 0.1 * torch.randn(D, generator=g)).to(BF).to(DEV)
    cos_t, sin_t = (t.to(DEV) for t in ref.rope_tables(128, D, 1e6))
    bt = _i32([[5, 2, 7, 0, 0], [3, 9, 4, 8, 1]])
    seq, pos = _i32([s for s, _ in rows]), _i32([p for _, p in rows])
    args = (q_w, k_w, cos_t, sin_t, bt, seq, pos)

    SENT_BF, SENT_BYTE, SENT_SCALE = -7.0, 0x5A, -3.0
    kb = torch.full((nb, hk, BS, D), SENT_BF, dtype=BF, device=DEV)
    vb = kb.clone()
    k8 = torch.full((nb, hk, BS, D), SENT_BYTE, dtype=torch.uint8,
                    device=DEV).view(F8)
    v8 = k8.clone()
    ks = torch.full((nb, hk, BS), SENT_SCALE, device=DEV)
    vs = ks.clone()
    qkv_b, qkv_8 = qkv.clone(), qkv.clone()
    ops.qk_rope_write_kv(qkv_b, hq, kb, vb, *args)
    ops.qk_rope_write_kv(qkv_8, hq, k8, v8, *args, k_scale=ks, v_scale=vs)
    assert torch.equal(qkv_b, qkv_8)
    assert not torch.equal(qkv_b, qkv)                # Q was rotated

    written = torch.zeros(nb, 1, BS, dtype=torch.bool, device=DEV)
    for s, p in rows:
        written[int(bt[s, p // BS]), 0, p % BS] = True
    assert int(written.sum()) == T
    for cb, c8, cs in ((kb, k8, ks), (vb, v8, vs)):
        assert (cb[written.expand(nb, hk, BS)] != SENT_BF).any()
        want_q, want_s = ref.quantize_kv_rows(cb)
        want_q = torch.where(written.unsqueeze(-1), _u8(want_q),
                             torch.full_like(_u8(want_q), SENT_BYTE))
        want_s = torch.where(written, want_s,
                             torch.full_like(want_s, SENT_SCALE))
        assert torch.equal(cs, want_s)
        assert torch.equal(_u8(c8), want_q)
    # the all-zero V row: scale 1.0 and zero bytes
    b0, r0 = int(bt[rows[0][0], rows[0][1] // BS]), rows[0][1] % BS
    assert vs[b0, 0, r0] == 1.0 and not _u8(v8)[b0, 0, r0].any()


# ---------------------------------------------------------- split decode

def _split(pool, q, seqs, splits, kc, vc, ks, vs):
    T, hq = q.size(0), q.size(1)
    out = torch.empty(T, hq, D, dtype=BF, device=DEV)
    part = torch.empty(T, hq, ops.attn_nsplits(), D, device=DEV)
    part_ml = torch.empty(T, hq, ops.attn_nsplits(), 2, device=DEV)
    ops.paged_attention_split(out, q, kc, vc, pool.bt, _i32(seqs),
                              _i32([LENS[s] - 1 for s in seqs]), part, part_ml,
                              SCALE, splits=splits, k_scale=ks, v_scale=vs)
    return out


# T -> the calls' sequences; every context length appears at every T, and
# T = 5 and 8 mix short and long contexts in one call
SPLIT_CALLS = {
    1: [[i] for i in range(len(LENS))],
    5: [[0, 2, 4, 6, 8], [8, 7, 5, 3, 1]],
    8: [[0, 1, 2, 3, 4, 5, 6, 7], [8, 7, 6, 5, 4, 3, 2, 1]],
}


@pytest.mark.parametrize("splits", [32, 64])
@pytest.mark.parametrize("T", [1, 5, 8])
def test_split_decode_equals_the_image(pool, T, splits):
    for n, seqs in enumerate(SPLIT_CALLS[T]):
        q = pool.q(T, 1000 * T + n)
        want = _split(pool, q, seqs, splits, **pool.image())
        got = _split(pool, q, seqs, splits, **pool.fp8())
        again = _split(pool, q, seqs, splits, **pool.fp8())
        assert not want.float().isnan().any(), seqs
        assert torch.equal(got, want), seqs
        assert torch.equal(again, got), seqs


# --------------------------------------------------------- flash prefill

def _flash(pool, q, segs, kc, vc, ks, vs):
    """segs: [(sequence, prior context, query rows)], packed in order."""
    seq, pos, desc, row0 = [], [], [], 0
    for s, ctx, n in segs:
        seq += [s] * n
        pos += list(range(ctx, ctx + n))
        desc.append((row0, n))
        row0 += n
    out = torch.empty(q.size(0), q.size(1), D, dtype=BF, device=DEV)
    ops.flash_prefill(out, q, kc, vc, pool.bt, _i32(seq), _i32(pos),
                      ops.build_qtile_desc(desc, DEV), SCALE, ks, vs)
    return out


def test_flash_prefill_equals_the_image(pool):
    """Segments of 1..70 query rows (below, at and above the 32-row q tile)
    after 0, 70 and 200 cached positions, so the KV range crosses the
    64-position chunk and the q-tile cut; then two segments of different
    sequences in one call. Sequences 6..8 hold at least 1000 positions."""
    calls = [[(6 + (n + ctx) % 3, ctx, n)]
             for n in (1, 31, 32, 33, 70) for ctx in (0, 70, 200)]
    calls.append([(7, 70, 33), (8, 200, 70)])
    for i, segs in enumerate(calls):
        q = pool.q(sum(n for _, _, n in segs), 2000 + i)
        want = _flash(pool, q, segs, **pool.image())
        got = _flash(pool, q, segs, **pool.fp8())
        assert not want.float().isnan().any(), segs
        assert torch.equal(got, want), segs


# ---------------------------------------------------- paged_attention (VALU)

def test_paged_attention_equals_the_image(pool):
    seqs = list(range(len(LENS)))                     # T = 9, mixed positions
    q = pool.q(len(seqs), 3000)
    pos = [LENS[s] - 1 for s in seqs]
    pos[6], pos[7] = 500, 31                          # and inside a sequence
    outs = []
    for c in (pool.image(), pool.fp8()):
        out = torch.empty(q.size(0), q.size(1), D, dtype=BF, device=DEV)
        ops.paged_attention(out, q, c["kc"], c["vc"], pool.bt, _i32(seqs),
                            _i32(pos), SCALE, c["ks"], c["vs"])
        outs.append(out)
    assert not outs[0].float().isnan().any()
    assert torch.equal(outs[1], outs[0])


# ----------------------------------------------------------- wrapper errors

def test_wrappers_reject_mismatched_caches_and_scales(pool):
    hq = pool.hk * GROUP
    good_s = pool.ks
    T = 2
    q = pool.q(T, 4000)
    out = torch.empty(T, hq, D, dtype=BF, device=DEV)
    seq, pos = _i32([6, 7]), _i32([40, 41])
    part = torch.empty(T, hq, ops.attn_nsplits(), D, device=DEV)
    part_ml = torch.empty(T, hq, ops.attn_nsplits(), 2, device=DEV)
    desc = ops.build_qtile_desc([(0, 1), (1, 1)], DEV)
    qkv = torch.zeros(T, (hq + 2 * pool.hk) * D, dtype=BF, device=DEV)
    w = torch.ones(D, dtype=BF, device=DEV)
    cos_t, sin_t = (t.to(DEV) for t in ref.rope_tables(64, D, 1e6))
    # the writer gets scratch copies: the good call at the end writes rows
    k8, v8 = pool.kq.clone(), pool.vq.clone()
    kb, vb = pool.ki.clone(), pool.vi.clone()
    wr = {id(pool.kq): k8, id(pool.vq): v8, id(pool.ki): kb, id(pool.vi): vb,
          id(pool.ks): pool.ks.clone(), id(pool.vs): pool.vs.clone()}

    def write(kc, vc, ks, vs):
        ops.qk_rope_write_kv(qkv.clone(), hq, wr[id(kc)], wr[id(vc)], w, w,
                             cos_t, sin_t, pool.bt, seq, pos,
                             k_scale=wr.get(id(ks), ks),
                             v_scale=wr.get(id(vs), vs))

    calls = {
        "qk_rope_write_kv": write,
        "paged_attention_split": lambda kc, vc, ks, vs:
            ops.paged_attention_split(out, q, kc, vc, pool.bt, seq, pos, part,
                                      part_ml, SCALE, k_scale=ks, v_scale=vs),
        "flash_prefill": lambda kc, vc, ks, vs:
            ops.flash_prefill(out, q, kc, vc, pool.bt, seq, pos, desc, SCALE,
                              ks, vs),
        "paged_attention": lambda kc, vc, ks, vs:
            ops.paged_attention(out, q, kc, vc, pool.bt, seq, pos, SCALE,
                                ks, vs),
    }
    nb, hk = pool.nb, pool.hk
    bad = {
        "bf16 caches with scales": (pool.ki, pool.vi, good_s, good_s),
        "fp8 caches without scales": (pool.kq, pool.vq, None, None),
        "fp8 caches, one scale": (pool.kq, pool.vq, good_s, None),
        "fp8 K with bf16 V": (pool.kq, pool.vi, good_s, good_s),
        "f64 scales": (pool.kq, pool.vq, good_s.double(), good_s.double()),
        "bf16 v_scale": (pool.kq, pool.vq, good_s, good_s.to(BF)),
        "scales [NB, Hk]": (pool.kq, pool.vq, good_s[:, :, 0].contiguous(),
                            good_s[:, :, 0].contiguous()),
        "scales [NB, Hk, 16, 1]": (pool.kq, pool.vq, good_s.unsqueeze(-1),
                                   good_s.unsqueeze(-1)),
        "scales of fewer blocks": (pool.kq, pool.vq, good_s[1:].contiguous(),
                                   good_s[1:].contiguous()),
        "strided k_scale": (pool.kq, pool.vq, torch.ones(
            nb, hk, 2 * BS, device=DEV)[:, :, :BS], good_s),
    }
    for op, call in calls.items():
        for what, args in bad.items():
            with pytest.raises(RuntimeError, match=op):
                call(*args)
                pytest.fail(f"{op} accepted: {what}")
        call(pool.kq, pool.vq, pool.ks, pool.vs)      # both good forms run
        call(pool.ki, pool.vi, None, None)
    torch.cuda.synchronize()
