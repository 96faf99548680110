"""MFMA flash prefill past one 64-position KV chunk, and at its tile edges.

`flash_prefill_kernel` walks the KV prefix of a q-tile in chunks of 64 from
position 0 and carries an online softmax (running max, running sum, rescale
of the accumulator) from chunk to chunk. A chunk that lies wholly below every
row's causal bound of a full 32-row tile takes an unmasked fast path
(`interior`). The first-round test stops at a causal bound of 57, so neither
the carry nor the fast path ran there. Plain randn inputs could not tell
anyway: at a context in the hundreds the softmax is diffuse, the output is
about +-0.1 per element, and a kernel that drops chunks or forgets a rescale
lands inside the tolerance. So the cases here plant keys (K = beta * q of the
row and head that is to find it, score about beta * sqrt(128)):

* weak early, strong late - kv head 0, q head 0 of a designated row finds a
  weak key (beta 1.25, about 5 % of the mass) in chunk 0 or 1 and a strong
  one (beta 1.5, about 95 %) in a later chunk, both below its bound. The
  second raises the running max by about 2.9, so the rescale factor is about
  0.055: a missing accumulator rescale, a missing sum rescale and a kernel
  that reads only the first chunk each move the row by more than 1.
* causal edge - kv head 1, q head 8 of every row finds a beta 1.5 key at its
  own position, the last it may see. Even rows share q head 8 with the row
  after them, so that row's key, one position past the bound, would score
  the same: a mask one too wide moves the even rows, one too narrow moves
  every row.

`test_planted_inputs_discriminate` proves on the CPU, with a fp32 emulation
of the chunk loop and five switches for those five defects, that each defect
moves every designated row by more than 0.3 (the split-long test's
threshold), and that the emulation without a switch is the reference.

Inputs follow test_attn_split_long_gpu.py: built on the CPU from a seeded
generator, cache blocks handed out in shuffled order, NaN in block 0, in
every block no table entry names and in every cache row past a sequence's
last written position; "packed" cases pass q as the strided view of a
[T, qdim + 2 kvdim] buffer whose other columns are NaN, as the model does.
`out` starts from a sentinel.

Reference: ops.reference.paged_attention_ref on f32 q (so its result stays
f32). Tolerance: atol = 3e-2 plus rtol = 2^-7, the split-long test's; the
relative part covers the bf16 half-ulp roundings of P and of the output
(2^-9 each), which matter at outputs of magnitude 1 to 4. This kernel rounds
once more, q * scale to bf16 at staging: a relative 2^-9 per product, which
moves a score of 17 by at most 0.03 and in practice (128 independent
roundings) by about 0.003, far below what the softmax here resolves, so the
bound is not widened. Measured max-abs error against the fp32 reference on an
MI355X (each test prints its own): deep 0.0078, edges 0.0078, eight 0.0080,
heights 0.0078, shared 0.0083, zero200 0.0087 at outputs up to 4.5 (half a
bf16 ulp of an output between 2 and 4 is 0.0078); the randn case 0.0080 at outputs up to 2.5. At
the designated elements the bound stays under 0.1, a third of the 0.3 gap
(asserted).
"""
import pytest
import torch

from room_amd import ops
from room_amd.engine.step_plan import prefill_graph_shape, qtile_list
from room_amd.ops import reference as ref

DEV = "cuda"
HQ, HK, D, BS = 16, 2, 128, 16
GROUP = HQ // HK
CHUNK, QT = 64, 32
QDIM, KVDIM = HQ * D, HK * D
SCALE = D ** -0.5
BETA, BETA_WEAK = 1.5, 1.25
ATOL, RTOL = 3e-2, 2.0 ** -7
GAP = 0.3
SENTINEL = -1024.0
BF = torch.bfloat16
SWITCHES = ("first_chunk", "bound_plus", "bound_minus", "no_acc_rescale",
            "no_sum_rescale")


def gpu(fn):
    fn = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")(fn)
    return pytest.mark.gpu(fn)


# name -> (packed, [(seq, start, n), ...]); a segment is n rows of sequence
# seq at positions start .. start + n - 1, cut into tiles of <= 32 rows.
CASES = {
    # a full tile deep in a reused prefix: chunks 0..5 interior, chunk 6 holds
    # the diagonal, bound_max = 432 leaves it ragged
    "deep": (True, [(0, 400, 32)]),
    # a prompt from zero: tile 2 (64..95) is the first with an interior chunk,
    # the last tile has 8 rows
    "zero200": (False, [(0, 0, 200)]),
    # full tiles on both sides of `base + 64 <= bound_min` (starts 62, 63, 64)
    # and bound_max of exactly 64, 65, 128, 129
    "edges": (False, [(0, 62, 32), (1, 63, 32), (2, 64, 32), (3, 32, 32),
                      (4, 33, 32), (5, 96, 32), (6, 97, 32)]),
    # tile heights 1, 31, 32 and 33 (= 32 + 1); row offsets 0, 1, 32, 64
    "heights": (True, [(0, 70, 1), (1, 100, 31), (2, 230, 32), (3, 250, 33)]),
    # 8 segments on 8 sequences, not in block order, offsets off the 32 grid
    "eight": (True, [(5, 0, 45), (2, 300, 17), (7, 130, 70), (0, 63, 33),
                     (3, 640, 40), (6, 5, 3), (1, 200, 64), (4, 90, 50)]),
    # sequence 0 is read by tiles of two segments: a first chunk of a prompt
    # and, after another request's rows, its next chunk
    "shared": (False, [(0, 0, 40), (1, 200, 10), (0, 40, 90)]),
}


def _rows(segs):
    """[(row0, n)] segments, seq_ids, q_pos of a case's rows."""
    segments, seq_ids, q_pos = [], [], []
    for s, start, n in segs:
        segments.append((len(seq_ids), n))
        seq_ids += [s] * n
        q_pos += list(range(start, start + n))
    return segments, seq_ids, q_pos


def _build(segs, packed, seed, planted):
    """CPU tensors of one case. The sequence after the last one a segment
    names is a scrap sequence with one written position (the engine's pad
    slot); three blocks are never handed out."""
    gen = torch.Generator().manual_seed(seed)
    segments, seq_ids, q_pos = _rows(segs)
    T = len(seq_ids)
    nseq = max(s for s, _, _ in segs) + 1
    lens = [0] * nseq + [1]
    for s, start, n in segs:
        lens[s] = max(lens[s], start + n)
    assert all(lens), "every sequence id up to the largest must be used"
    nblk = [(L + BS - 1) // BS for L in lens]
    nb = sum(nblk) + 1 + 3
    buf = torch.randn(T, QDIM + 2 * KVDIM, generator=gen).to(BF)
    q = buf[:, :QDIM].view(T, HQ, D)
    kc = torch.randn(nb, HK, BS, D, generator=gen).to(BF)
    vc = torch.randn(nb, HK, BS, D, generator=gen).to(BF)
    perm = torch.randperm(nb - 1, generator=gen) + 1
    bt = torch.zeros(len(lens), max(nblk), dtype=torch.int32)
    at = 0
    for s, L in enumerate(lens):
        bt[s, :nblk[s]] = perm[at:at + nblk[s]].int()
        at += nblk[s]

    def kslot(s, p):
        return int(bt[s, p // BS]), p % BS

    weak_rows, used = [], {}
    if planted:
        # causal edge: kv head 1, q head 8
        for (row0, n), (s, start, _) in zip(segments, segs):
            for j in range(0, n - 1, 2):
                q[row0 + j + 1, GROUP] = q[row0 + j, GROUP]
            for j in range(n):
                b, o = kslot(s, start + j)
                kc[b, 1, o] = (BETA * q[row0 + j, GROUP].float()).to(BF)
        # weak early, strong late: kv head 0, q head 0 of up to three rows of
        # every segment that reaches position 192
        for (row0, n), (s, start, _) in zip(segments, segs):
            taken = used.setdefault(s, set())
            for k, j in enumerate(sorted({0, n // 2, n - 1})):
                pos = start + j
                if pos < 3 * CHUNK:
                    continue
                # the first designated row of a segment has its strong key on
                # the diagonal, the others anywhere from chunk 2 to their bound
                strong = pos
                while k or strong in taken:
                    strong = 2 * CHUNK + int(torch.randint(
                        pos + 1 - 2 * CHUNK, (1,), generator=gen))
                    k = 0
                taken.add(strong)
                weak = int(torch.randint(2 * CHUNK, (1,), generator=gen))
                while weak in taken:
                    weak = int(torch.randint(2 * CHUNK, (1,), generator=gen))
                taken.add(weak)
                for p, beta in ((weak, BETA_WEAK), (strong, BETA)):
                    b, o = kslot(s, p)
                    kc[b, 0, o] = (beta * q[row0 + j, 0].float()).to(BF)
                weak_rows.append(row0 + j)
    # poison last: block 0, the blocks no table entry names, rows past the end
    kc[0] = vc[0] = float("nan")
    for b in perm[at:]:
        kc[b] = vc[b] = float("nan")
    for s, L in enumerate(lens):
        if L % BS:
            b = int(bt[s, nblk[s] - 1])
            kc[b, :, L % BS:] = float("nan")
            vc[b, :, L % BS:] = float("nan")
    if packed:
        buf[:, QDIM:] = float("nan")
    else:
        q = q.contiguous()
    pos_t = torch.tensor(q_pos, dtype=torch.int32)
    even_rows = [row0 + j for row0, n in segments for j in range(0, n - 1, 2)]
    return dict(
        q=q, kc=kc, vc=vc, bt=bt, lens=lens, segments=segments, segs=segs,
        seq_ids=torch.tensor(seq_ids, dtype=torch.int32), q_pos=pos_t,
        tiles=qtile_list(segments, QT), scrap=nseq,
        # (rows, q head) each switch must move
        designated={
            "first_chunk": [(weak_rows, 0),
                            ((pos_t >= CHUNK).nonzero().flatten().tolist(),
                             GROUP)],
            "bound_plus": [(even_rows, GROUP)],
            "bound_minus": [(list(range(T)), GROUP)],
            "no_acc_rescale": [(weak_rows, 0)],
            "no_sum_rescale": [(weak_rows, 0)],
        } if planted else {})


_built, _refs = {}, {}


def _inputs(name, planted=True):
    key = (name, planted)
    if key not in _built:
        packed, segs = CASES[name]
        seed = 300 + sorted(CASES).index(name)
        _built[key] = _build(segs, packed, seed, planted)
    return _built[key]


def _reference(name, planted=True):
    """fp32 reference of a case, computed once on the CPU and never changed."""
    key = (name, planted)
    if key not in _refs:
        i = _inputs(name, planted)
        _refs[key] = ref.paged_attention_ref(
            i["q"].float(), i["kc"], i["vc"], i["bt"], i["seq_ids"],
            i["q_pos"], SCALE)
        assert _refs[key].dtype == torch.float32
    return _refs[key]


def _seq_kv(i, s, upto):
    """K, V of sequence s at positions 0..upto-1 as f32 [HK, upto, D]."""
    blocks = i["bt"][s, :(upto + BS - 1) // BS].long()
    k = i["kc"][blocks].transpose(0, 1).reshape(HK, -1, D)[:, :upto].float()
    v = i["vc"][blocks].transpose(0, 1).reshape(HK, -1, D)[:, :upto].float()
    return k, v


def _emulate(i, switch=None):
    """The kernel's algorithm in fp32: per tile, chunks of 64 from position 0
    up to the tile's bound_max (positions past it staged as zeros), masked
    scores, running max m and sum l, accumulator rescaled by exp(m - m_new).
    `switch` plants one defect."""
    q, q_pos = i["q"].float(), i["q_pos"].long()
    out = torch.zeros(q.shape)
    shift = {"bound_plus": 1, "bound_minus": -1}.get(switch, 0)
    for row0, ntok in i["tiles"]:
        if ntok == 0:
            continue
        rows = slice(row0, row0 + ntok)
        s = int(i["seq_ids"][row0])
        bound = q_pos[rows] + 1
        bound_max = int(bound.max())
        k_all, v_all = _seq_kv(i, s, bound_max)
        for hk in range(HK):
            heads = slice(hk * GROUP, (hk + 1) * GROUP)
            qt = q[rows, heads] * SCALE                       # [n, 8, D]
            m = torch.full((ntok, GROUP), float("-inf"))
            l = torch.zeros(ntok, GROUP)
            acc = torch.zeros(ntok, GROUP, D)
            for base in range(0, bound_max, CHUNK):
                if switch == "first_chunk" and base > 0:
                    break
                k = torch.zeros(CHUNK, D)
                v = torch.zeros(CHUNK, D)
                live = min(CHUNK, bound_max - base)
                k[:live] = k_all[hk, base:base + live]
                v[:live] = v_all[hk, base:base + live]
                sc = torch.einsum("nhd,cd->nhc", qt, k)
                kpos = base + torch.arange(CHUNK)
                masked = kpos[None, :] >= (bound + shift)[:, None]  # [n, 64]
                sc = sc.masked_fill(masked[:, None, :], float("-inf"))
                m_new = torch.maximum(m, sc.amax(-1))
                rs = torch.where(m == float("-inf"), torch.ones_like(m),
                                 torch.exp(m - m_new))
                p = torch.where(sc == float("-inf"), torch.zeros_like(sc),
                                torch.exp(sc - m_new[..., None]))
                l = l * (1.0 if switch == "no_sum_rescale" else rs) + p.sum(-1)
                if switch != "no_acc_rescale":
                    acc = acc * rs[..., None]
                acc = acc + torch.einsum("nhc,cd->nhd", p, v)
                m = m_new
            inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
            out[rows, heads] = acc * inv[..., None]
    return out


# --------------------------------------------------------------- CPU tests

def test_cases_hold_the_edges():
    """The case list really contains the edges its comments name."""
    tiles = []          # (ntok, first pos, bound_max) of every tile
    for name in CASES:
        i = _inputs(name)
        for row0, n in i["tiles"]:
            p = i["q_pos"][row0:row0 + n]
            assert len(set(i["seq_ids"][row0:row0 + n].tolist())) == 1
            tiles.append((n, int(p.min()), int(p.max()) + 1))
    heights = {n for n, _, _ in tiles}
    assert {1, 31, 32, 8} <= heights
    assert {64, 65, 128, 129, 432} <= {bm for _, _, bm in tiles}
    full_starts = {p for n, p, _ in tiles if n == QT}
    assert {62, 63, 64, 400} <= full_starts
    # interior chunks exist (full tile, chunk wholly below bound_min), and so
    # do full tiles with none
    n_interior = [(p + 1) // CHUNK for n, p, _ in tiles if n == QT]
    assert 0 in n_interior and 1 in n_interior and 6 in n_interior
    i = _inputs("eight")
    assert len({s for s, _, _ in i["segs"]}) == 8
    assert [s for s, _, _ in i["segs"]] != sorted(s for s, _, _ in i["segs"])
    assert any(row0 % QT for row0, _ in i["segments"])
    assert len({n for _, n in i["segments"]}) == 8
    i = _inputs("shared")
    assert [s for s, _, _ in i["segs"]].count(0) == 2
    assert _inputs("deep")["q"].stride(0) == QDIM + 2 * KVDIM
    assert _inputs("zero200")["q"].is_contiguous()


@pytest.mark.parametrize("name", sorted(CASES))
def test_planted_inputs_discriminate(name):
    """Property of the inputs, checked on the CPU: the emulated chunk loop is
    the reference, and each of its five defects moves every designated
    (row, head) by more than 0.3."""
    i = _inputs(name)
    expect = _reference(name)
    assert not torch.isnan(expect).any()
    clean = _emulate(i)
    err = (clean - expect).abs().max().item()
    assert err < 1e-4, f"emulation off the reference by {err:.2e}"
    for switch in SWITCHES:
        got = _emulate(i, switch)
        for rows, head in i["designated"][switch]:
            if not rows:
                continue
            gap = (got[rows, head] - expect[rows, head]).abs().amax(-1)
            gap = torch.nan_to_num(gap, nan=float("inf"))
            worst = int(gap.argmin())
            print(f"{name} {switch} head {head}: {len(rows)} rows, "
                  f"smallest gap {gap.min().item():.3f}")
            assert gap.min().item() > GAP, (
                f"{switch}: row {rows[worst]} head {head} moves by only "
                f"{gap.min().item():.3f}")
    # the deep cases must exercise every switch
    if name in ("deep", "eight", "zero200", "heights", "shared"):
        for switch in SWITCHES:
            assert any(rows for rows, _ in i["designated"][switch]), switch
    # the bound at the designated elements stays under a third of the gap
    for switch in SWITCHES:
        for rows, head in i["designated"][switch]:
            if rows:
                top = expect[rows, head].abs().max().item()
                assert ATOL + RTOL * top < GAP / 3, top


# --------------------------------------------------------------- GPU tests

def _dev_inputs(i):
    """Device copies; a packed q stays a strided view of its packed buffer."""
    q = i["q"]
    if not q.is_contiguous():
        buf = torch.as_strided(q, (q.size(0), QDIM + 2 * KVDIM),
                               (q.stride(0), 1)).to(DEV)
        q = buf[:, :QDIM].view(-1, HQ, D)
        assert q.stride(0) == QDIM + 2 * KVDIM
    else:
        q = q.to(DEV)
    return dict(q=q, kc=i["kc"].to(DEV), vc=i["vc"].to(DEV),
                bt=i["bt"].to(DEV), seq_ids=i["seq_ids"].to(DEV),
                q_pos=i["q_pos"].to(DEV))


def _desc(tiles):
    return torch.tensor(tiles, dtype=torch.int32, device=DEV).view(-1, 2)


def _launch(d, desc):
    """One call on device inputs d; out starts from the sentinel."""
    out = torch.full(d["q"].shape, SENTINEL, dtype=BF, device=DEV)
    ops.flash_prefill(out, d["q"], d["kc"], d["vc"], d["bt"], d["seq_ids"],
                      d["q_pos"], desc, SCALE)
    return out.cpu()


def _run(name, planted=True):
    i = _inputs(name, planted)
    desc = ops.build_qtile_desc(i["segments"], DEV)
    assert desc.tolist() == [list(t) for t in i["tiles"]]
    return _launch(_dev_inputs(i), desc)


def _check(name, out, expect):
    err = (out.float() - expect).abs()
    print(f"{name}: max-abs err {err.max().item():.4f}, "
          f"max |expect| {expect.abs().max().item():.3f}")
    bad = err > ATOL + RTOL * expect.abs()     # NaN err compares False:
    assert not torch.isnan(out.float()).any()  # so NaN is its own check
    assert not bad.any(), (
        f"{int(bad.sum())} elements off, first at "
        f"{bad.nonzero()[0].tolist()}, worst {err.max().item():.4f}")


def _bits(x):
    return x.contiguous().view(torch.int16)


@gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_flash_prefill_planted(name):
    _check(name, _run(name), _reference(name))


@gpu
def test_flash_prefill_randn_diffuse():
    """The diffuse regime: plain randn K at contexts up to 680."""
    _check("eight/randn", _run("eight", planted=False),
           _reference("eight", planted=False))


@gpu
def test_tile_cut_invariance():
    """The deep-prefix rows as one 32-row tile, as 32 one-row tiles and as
    5 + 27 rows: every row has the same bits. A row's scores depend on its own
    q row and on the chunk grid, which starts at position 0 whatever the tile;
    a chunk past a row's bound gives rs = exp(0) = 1, p = 0 and exact-zero
    MFMA terms; the interior path only omits compares that would be false.
    One-row tiles are never interior, so this pins the fast path to the
    masked one bit for bit."""
    i = _inputs("deep")
    d = _dev_inputs(i)
    whole = _launch(d, _desc([(0, 32)]))
    single = _launch(d, _desc([(r, 1) for r in range(32)]))
    split = _launch(d, _desc([(0, 5), (5, 27)]))
    assert not (whole == SENTINEL).any()
    assert torch.equal(_bits(whole), _bits(single))
    assert torch.equal(_bits(whole), _bits(split))


@gpu
def test_segment_alone_and_nan_isolation():
    """Each segment of the 8-segment call alone equals its rows in the full
    call, and its rows do not change when every q row, packed column and
    cache block it does not own is NaN."""
    i = _inputs("eight")
    d = _dev_inputs(i)
    full = _launch(d, _desc(i["tiles"]))
    W = QDIM + 2 * KVDIM
    for (row0, n), (s, start, _) in zip(i["segments"], i["segs"]):
        rows = slice(row0, row0 + n)
        # alone: only its rows exist
        buf = torch.full((n, W), float("nan"), dtype=BF, device=DEV)
        buf[:, :QDIM] = d["q"][rows].reshape(n, QDIM)
        alone = dict(d, q=buf[:, :QDIM].view(n, HQ, D),
                     seq_ids=d["seq_ids"][rows].contiguous(),
                     q_pos=d["q_pos"][rows].contiguous())
        got = _launch(alone, _desc(qtile_list([(0, n)], QT)))
        assert torch.equal(_bits(got), _bits(full[rows])), f"segment {s} alone"
        # poisoned: same call, everything foreign NaN
        buf = torch.full((i["q"].size(0), W), float("nan"), dtype=BF,
                         device=DEV)
        buf[rows, :QDIM] = d["q"][rows].reshape(n, QDIM)
        own = i["bt"][s, :(i["lens"][s] + BS - 1) // BS].long().to(DEV)
        kc = torch.full_like(d["kc"], float("nan"))
        vc = torch.full_like(d["vc"], float("nan"))
        kc[own], vc[own] = d["kc"][own], d["vc"][own]
        poisoned = dict(d, q=buf[:, :QDIM].view(-1, HQ, D), kc=kc, vc=vc)
        got = _launch(poisoned, _desc(i["tiles"]))
        assert torch.equal(_bits(got[rows]), _bits(full[rows])), \
            f"segment {s} reads what it does not own"


@gpu
def test_zero_count_tiles_and_pad_segment():
    """The descriptor as _PrefillGraph.run builds it: the real tiles, the pad
    segment of prefill_graph_shape (scrap sequence, pos 0 on every row) and
    zero rows up to gmax. Real rows equal the unpadded call, every pad row is
    V at position 0 of the scrap sequence (a one-key softmax has p = 1
    exactly), and rows no tile names keep the sentinel."""
    i = _inputs("heights")
    d = _dev_inputs(i)
    plain = _launch(d, _desc(i["tiles"]))
    T, spare = i["q"].size(0), 5
    tb, seg_graph = prefill_graph_shape(T, i["segments"], buckets=(160,))
    assert tb == 160 and seg_graph[-1] == (T, tb - T)
    tiles = qtile_list(seg_graph, QT)
    gmax = tb // QT + 8 + 2
    assert len(tiles) < gmax
    desc = torch.zeros(gmax, 2, dtype=torch.int32)
    desc[:len(tiles)] = torch.tensor(tiles, dtype=torch.int32)
    gen = torch.Generator().manual_seed(9)
    buf = torch.full((tb + spare, QDIM + 2 * KVDIM), float("nan"), dtype=BF)
    buf[:, :QDIM] = torch.randn(tb + spare, QDIM, generator=gen).to(BF)
    buf[:T, :QDIM] = i["q"].reshape(T, QDIM)
    buf = buf.to(DEV)
    seq_ids = torch.full((tb + spare,), i["scrap"], dtype=torch.int32)
    seq_ids[:T] = i["seq_ids"]
    q_pos = torch.zeros(tb + spare, dtype=torch.int32)
    q_pos[:T] = i["q_pos"]
    padded = dict(d, q=buf[:, :QDIM].view(-1, HQ, D), seq_ids=seq_ids.to(DEV),
                  q_pos=q_pos.to(DEV))
    got = _launch(padded, desc.to(DEV))
    assert torch.equal(_bits(got[:T]), _bits(plain))
    v0 = i["vc"][int(i["bt"][i["scrap"], 0]), :, 0]             # [HK, D]
    assert not torch.isnan(v0.float()).any()
    want = v0.repeat_interleave(GROUP, dim=0).expand(tb - T, HQ, D)
    assert torch.equal(_bits(got[T:tb]), _bits(want))
    assert (got[tb:] == SENTINEL).all()


@gpu
def test_flash_prefill_deterministic():
    assert torch.equal(_bits(_run("eight")), _bits(_run("eight")))


@gpu
def test_flash_prefill_wrapper_errors():
    """Every call here is rejected by a TORCH_CHECK of the wrapper, which all
    stand before the launch: none reaches the kernel."""
    T, nb, S, mb = 4, 3, 2, 2
    i32 = dict(dtype=torch.int32, device=DEV)

    def good():
        return dict(
            out=torch.empty(T, HQ, D, dtype=BF, device=DEV),
            q=torch.zeros(T, HQ, D, dtype=BF, device=DEV),
            kc=torch.zeros(nb, HK, BS, D, dtype=BF, device=DEV),
            vc=torch.zeros(nb, HK, BS, D, dtype=BF, device=DEV),
            bt=torch.ones(S, mb, **i32), seq_ids=torch.zeros(T, **i32),
            q_pos=torch.zeros(T, **i32),
            desc=torch.tensor([[0, T]], **i32))

    def call(**bad):
        a = dict(good(), **bad)
        ops.flash_prefill(a["out"], a["q"], a["kc"], a["vc"], a["bt"],
                          a["seq_ids"], a["q_pos"], a["desc"], SCALE)

    def bf(*shape):
        return torch.zeros(*shape, dtype=BF, device=DEV)

    bad_calls = {
        "out f32": dict(out=torch.empty(T, HQ, D, device=DEV)),
        "out short": dict(out=bf(T - 1, HQ, D)),
        "out flat": dict(out=bf(T, HQ * D)),
        "out strided": dict(out=bf(T, HQ, 2 * D)[..., :D]),
        "q f16": dict(q=torch.zeros(T, HQ, D, dtype=torch.float16, device=DEV)),
        "q heads": dict(q=bf(T, HQ + 8, D), out=bf(T, HQ + 8, D)),
        "kcache f16": dict(kc=torch.zeros(nb, HK, BS, D, dtype=torch.float16,
                                          device=DEV)),
        "vcache f32": dict(vc=torch.zeros(nb, HK, BS, D, device=DEV)),
        "kcache strided": dict(kc=bf(nb, HK, BS, 2 * D)[..., :D]),
        "vcache strided": dict(vc=bf(nb, HK, 2 * BS, D)[:, :, :BS]),
        "block size 32": dict(kc=bf(nb, HK, 32, D), vc=bf(nb, HK, 32, D)),
        "head dim 64": dict(kc=bf(nb, HK, BS, 64), vc=bf(nb, HK, BS, 64)),
        "caches 3-D": dict(kc=bf(nb, HK * BS, D), vc=bf(nb, HK * BS, D)),
        "vcache fewer blocks": dict(vc=bf(nb - 1, HK, BS, D)),
        "desc [G,3]": dict(desc=torch.tensor([[0, T, 0]], **i32)),
        "desc 1-D": dict(desc=torch.tensor([0, T], **i32)),
        "desc strided": dict(desc=torch.tensor([[0, T, 0, 0], [0, 0, 0, 0]],
                                               **i32)[:, :2]),
        "desc int64": dict(desc=torch.tensor([[0, T]], device=DEV)),
        "seq_ids short": dict(seq_ids=torch.zeros(T - 1, **i32)),
        "q_pos long": dict(q_pos=torch.zeros(T + 1, **i32)),
        "seq_ids int64": dict(seq_ids=torch.zeros(T, dtype=torch.int64,
                                                  device=DEV)),
        "q_pos int64": dict(q_pos=torch.zeros(T, dtype=torch.int64,
                                              device=DEV)),
        "block_table 1-D": dict(bt=torch.ones(S * mb, **i32)),
        "block_table strided": dict(bt=torch.ones(mb, S, **i32).t()),
        "block_table int64": dict(bt=torch.ones(S, mb, dtype=torch.int64,
                                                device=DEV)),
    }
    for what, bad in bad_calls.items():
        with pytest.raises(RuntimeError):
            call(**bad)
            pytest.fail(f"accepted: {what}")
    call()      # the unspoiled arguments are accepted
    torch.cuda.synchronize()
