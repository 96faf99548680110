"""sample_rows on the GPU: per-row parameters, penalties from the history
ring, seeded draws, ring append under hipGraph replay — against the plain
torch reference in room_amd/ops/reference.py.

Inputs are built so that the reference alone decides every answer; each test
asserts that on the reference's own numbers (distinct top logits, argmax gaps
> 1e-3, nucleus prefixes > 1e-3 away from top_p) before it looks at the
kernel's output."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from room_amd import ops
    from room_amd.ops import reference as ref
else:
    pytest.skip("no GPU", allow_module_level=True)

DEV = "cuda"
V_BIG = 151936
SPAN = (V_BIG + 63) // 64          # one scan block's slice
RING = 256


def _cols(B, **over):
    """Per-row parameter columns (host lists) with the 'off' defaults."""
    c = dict(temperature=[1.0] * B, top_p=[1.0] * B, top_k=[40] * B,
             seeds=[1000 + 7 * b for b in range(B)], ctr=[0] * B,
             rep=[1.0] * B, pres=[0.0] * B, freq=[0.0] * B, last_n=[0] * B,
             ring=[[0] * RING for _ in range(B)], ring_len=[0] * B)
    c.update(over)
    return c


def _dev(c):
    f = lambda k: torch.tensor(c[k], dtype=torch.float32, device=DEV)
    i = lambda k: torch.tensor(c[k], dtype=torch.int32, device=DEV)
    return dict(temperature=f("temperature"), top_p=f("top_p"),
                top_k=i("top_k"),
                seeds=torch.tensor(c["seeds"], dtype=torch.int64, device=DEV),
                ctr=i("ctr"), rep=f("rep"), pres=f("pres"), freq=f("freq"),
                last_n=i("last_n"), ring=i("ring"), ring_len=i("ring_len"))


def _call(logits, d, append=False, out=None):
    return ops.sample_rows(logits, d["temperature"], d["top_p"], d["top_k"],
                           d["seeds"], d["ctr"], d["rep"], d["pres"],
                           d["freq"], d["last_n"], d["ring"], d["ring_len"],
                           append=append, out=out)


def _window(c, b):
    return ref.ring_window_ref(torch.tensor(c["ring"][b]), c["ring_len"][b],
                               c["last_n"][b])


def _penalised(logits_cpu, c, b):
    return ref.apply_penalties_ref(logits_cpu[b], _window(c, b), c["rep"][b],
                                   c["pres"][b], c["freq"][b])


def _dist(logits_cpu, c, b):
    return ref.sample_dist_ref(
        logits_cpu[b], _window(c, b),
        dict(temperature=c["temperature"][b], top_p=c["top_p"][b],
             top_k=c["top_k"][b], repetition_penalty=c["rep"][b],
             presence_penalty=c["pres"][b], frequency_penalty=c["freq"][b]))


def _assert_distinct_top65(x):
    top = x.topk(min(65, x.numel())).values
    assert top.unique().numel() == top.numel(), "top-65 logits not distinct"


def _assert_argmax_gap(x):
    top2 = x.topk(2).values
    assert float(top2[0] - top2[1]) > 1e-3, "argmax gap too small"


def _assert_nucleus_clear(x, temperature, top_p, top_k):
    p = torch.softmax(x.double().topk(top_k).values / temperature, -1)
    assert float((p.cumsum(-1) - top_p).abs().min()) > 1e-3, \
        "a prefix's cumulative probability is within 1e-3 of top_p"


# ------------------------------------------------- 1. per-row parameters

def test_per_row_parameters_in_one_call():
    torch.manual_seed(21)
    B = 5
    logits_cpu = torch.randn(B, V_BIG)
    # row 3: peaked, so top_p = 0.5 keeps a nucleus of a few tokens
    for j, t in enumerate([70001, 12, 151000, 4747, 98765, 31337]):
        logits_cpu[3, t] = 9.0 - 0.45 * j
    c = _cols(B, temperature=[0.0, 1.0, 1.0, 1.0, 1.0],
              top_k=[40, 1, 16, 40, 64], top_p=[1.0, 1.0, 1.0, 0.5, 1.0])
    for b in range(B):
        _assert_distinct_top65(logits_cpu[b])
    _assert_argmax_gap(logits_cpu[0])
    _assert_argmax_gap(logits_cpu[1])
    _assert_nucleus_clear(logits_cpu[3], 1.0, 0.5, 40)
    nucleus = set(_dist(logits_cpu, c, 3).nonzero().flatten().tolist())
    assert 1 < len(nucleus) < 6
    top16 = set(logits_cpu[2].topk(16).indices.tolist())
    top64 = set(logits_cpu[4].topk(64).indices.tolist())
    logits = logits_cpu.to(DEV)
    d = _dev(c)
    seen3 = set()
    for draw in range(16):
        d["ctr"].fill_(draw)
        t = _call(logits, d).tolist()
        assert t[0] == int(logits_cpu[0].argmax())
        assert t[1] == int(logits_cpu[1].argmax())
        assert t[2] in top16
        assert t[3] in nucleus
        assert t[4] in top64
        seen3.add(t[3])
    assert len(seen3) > 1, "16 draws from a multi-token nucleus all equal"


# ------------------------------------------------- 2. penalties, greedy

def _penalty_case(sign):
    """Eight greedy rows at V = 151936 whose argmax each hinges on one
    property of the window handling. sign=+1: decisive logits positive
    (divide branch); sign=-1: an all-negative row (multiply branch)."""
    B = 8
    if sign > 0:
        x = torch.randn(B, V_BIG)                 # background max ≈ 4.5
        HI, U, REP, CNT_U, FREQ = 20.0, 12.0, 2.0, 9.0, 4.0
    else:
        x = torch.randn(B, V_BIG) - 10.0          # background max ≈ -5.5
        HI, U, REP, CNT_U, FREQ = -1.0, -1.8, 2.0, -4.0, 1.2
    u, g, h, k, a = 77777, 100003, 60001, 33333, 5000
    filler = [90000 + 13 * j for j in range(RING)]   # harmless window tokens
    c = _cols(B, temperature=[0.0] * B, rep=[REP] * B, pres=[0.1] * B,
              last_n=[64] * B)
    want = [None] * B

    def ring_of(pushes):
        """Ring contents and length after pushing `pushes` in order."""
        r = [0] * RING
        for j, t in enumerate(pushes):
            r[j % RING] = t
        return r, len(pushes)

    # row 0: window tokens at v = 0, V-1, a slice's first and last index and
    # the first index of the slice after it; a miss at any of them wins
    edge = [0, V_BIG - 1, SPAN, 2 * SPAN - 1, 2 * SPAN]
    for j, t in enumerate(edge):
        x[0, t] = HI - 0.05 * j
    x[0, u] = U
    c["ring"][0], c["ring_len"][0] = ring_of(filler[:20] + edge)
    want[0] = u
    # row 1: token `a` three times in the window; only c = 3 lets u win
    x[1, a], x[1, u] = HI, CNT_U
    c["rep"][1], c["pres"][1], c["freq"][1] = 1.0, 0.0, FREQ
    c["ring"][1], c["ring_len"][1] = ring_of(
        filler[:5] + [a] + filler[5:9] + [a, a] + filler[9:12])
    want[1] = u
    # rows 2/3: repeat_last_n = 4 < ring fill 10; g sits one push outside
    # the window (spared, wins) / on its oldest push (penalised, loses)
    for b, at in ((2, 5), (3, 6)):
        x[b, g], x[b, u] = HI, U
        pushes = filler[:10]
        pushes[at] = g
        c["ring"][b], c["ring_len"][b] = ring_of(pushes)
        c["last_n"][b] = 4
    want[2], want[3] = g, u
    # row 4: wrapped ring, len = 300, window = pushes 236..299: g on push
    # 236 and k on push 299 are penalised, h on push 235 is not and wins
    pushes = [filler[j % RING] for j in range(300)]
    pushes[235], pushes[236], pushes[299] = h, g, k
    x[4, g], x[4, h], x[4, k], x[4, u] = HI, HI - 0.05, HI + 0.5, U
    c["ring"][4], c["ring_len"][4] = ring_of(pushes)
    want[4] = h
    # row 5: len = 5; the 251 never-pushed slots hold the argmax id, which
    # must not be penalised
    x[5, g], x[5, u] = HI, U
    c["ring"][5] = filler[:5] + [g] * (RING - 5)
    c["ring_len"][5] = 5
    want[5] = g
    # rows 6/7: same logits and ring; row 6 has repeat_last_n = 0
    x[6, g], x[6, u] = HI, U
    x[7] = x[6]
    for b in (6, 7):
        c["ring"][b], c["ring_len"][b] = ring_of(filler[:30] + [g])
    c["last_n"][6] = 0
    want[6], want[7] = g, u
    return x, c, want


@pytest.mark.parametrize("sign", [1, -1], ids=["positive", "negative"])
def test_penalties_greedy_exact_token(sign):
    torch.manual_seed(22 + sign)
    x, c, want = _penalty_case(sign)
    if sign < 0:
        assert float(x.max()) < 0
    expect = []
    for b in range(x.size(0)):
        y = _penalised(x, c, b)
        _assert_distinct_top65(y)
        _assert_argmax_gap(y)
        expect.append(int(y.argmax()))
    assert expect == want, "the case does not test what it claims"
    got = _call(x.to(DEV), _dev(c)).tolist()
    assert got == expect


# ------------------------------------------------- 3. distribution

def test_distribution_matches_reference():
    torch.manual_seed(23)
    B, V, N = 8, 1000, 8 * 512
    row = torch.randn(V) * 2.0
    top = row.topk(12).indices.tolist()
    window = [top[0], top[0], top[2], top[5], 999, 0, top[9], top[0], 17, 16]
    ring = window + [0] * (RING - len(window))
    gen = torch.Generator().manual_seed(5)
    seeds = torch.randint(1, 2**62, (B,), generator=gen).tolist()
    c = _cols(B, temperature=[0.8] * B, top_p=[0.9] * B, top_k=[8] * B,
              seeds=seeds, rep=[1.3] * B, pres=[0.2] * B, freq=[0.1] * B,
              last_n=[64] * B, ring=[ring] * B, ring_len=[len(window)] * B)
    logits_cpu = row.repeat(B, 1)
    y = _penalised(logits_cpu, c, 0)
    _assert_distinct_top65(y)
    _assert_nucleus_clear(y, 0.8, 0.9, 8)
    p = _dist(logits_cpu, c, 0)
    assert 2 <= int((p > 0).sum()) <= 8
    logits = logits_cpu.to(DEV)
    d = _dev(c)
    draws = torch.empty(512, B, dtype=torch.int32, device=DEV)
    for t in range(512):
        d["ctr"].fill_(t)
        _call(logits, d, out=draws[t])
    counts = torch.bincount(draws.flatten().long().cpu(), minlength=V).double()
    assert int(counts.sum()) == N
    freq = counts / N
    bound = 5.0 * torch.sqrt(p * (1 - p) / N)      # binomial 5σ
    bad = ((freq - p).abs() > bound).nonzero().flatten().tolist()
    assert not bad, [(t, float(freq[t]), float(p[t])) for t in bad]
    assert float(counts[p == 0].sum()) == 0


# ------------------------------------------------- 4. determinism

def test_seeded_draws_are_row_and_batch_independent():
    torch.manual_seed(24)
    V = V_BIG
    big = torch.randn(8, V)
    top = big[5].topk(8).indices.tolist()
    ring = [top[1], top[3], 42] + [0] * (RING - 3)
    c8 = _cols(8, temperature=[0.0, 0.5, 1.0, 1.3, 0.7, 1.0, 0.9, 1.1],
               top_k=[1, 5, 64, 40, 2, 40, 7, 33],
               top_p=[1.0, 0.5, 0.9, 1.0, 0.3, 0.95, 0.8, 1.0],
               seeds=[11, 12, 13, 14, 15, 123456789012345, 17, 18])
    c8["rep"][5], c8["pres"][5], c8["last_n"][5] = 1.5, 0.5, 64
    c8["ring"][5], c8["ring_len"][5] = ring, 3
    c8["pres"][2], c8["last_n"][2] = 1.0, 16
    c8["ring"][2], c8["ring_len"][2] = list(range(RING)), 40
    c1 = {k: [v[5]] for k, v in c8.items()}
    l8, l1 = big.to(DEV), big[5:6].contiguous().to(DEV)
    d8, d1 = _dev(c8), _dev(c1)
    c1b = dict(c1, seeds=[c1["seeds"][0] + 1])
    d1b = _dev(c1b)
    a, b, other = [], [], []
    for t in range(64):
        for d in (d8, d1, d1b):
            d["ctr"].fill_(t)
        a.append(_call(l8, d8)[5])
        b.append(_call(l1, d1)[0])
        other.append(_call(l1, d1b)[0])
    a, b, other = (torch.stack(v).tolist() for v in (a, b, other))
    assert a == b
    assert len(set(a)) > 1
    assert other != a, "two seeds gave the same 64 draws"
    # seeds and ctr are read-only
    assert d8["seeds"].tolist() == c8["seeds"]
    assert d8["ctr"].tolist() == [63] * 8
    assert d1["seeds"].tolist() == c1["seeds"]


# ------------------------------------------------- 5. ring append, replay

def test_ring_append_under_graph_replay():
    torch.manual_seed(25)
    B, V, START = 4, 1000, 252          # 8 appends cross the wrap at 256
    logits = (torch.randn(B, V) * 2.0).to(DEV)
    gen = torch.Generator().manual_seed(9)
    ring0 = torch.randint(0, V, (B, RING), generator=gen, dtype=torch.int32)
    c = _cols(B, temperature=[1.0] * B, top_k=[64] * B, pres=[1e3] * B,
              last_n=[64] * B, ring=ring0.tolist(), ring_len=[START] * B)
    d = _dev(c)
    init = {k: d[k].clone() for k in ("ring", "ring_len", "ctr")}

    def reset():
        for k, v in init.items():
            d[k].copy_(v)

    # eager: 8 calls, ctr = 0..7, the ring advancing on the device
    eager = []
    for t in range(8):
        eager.append(_call(logits, d, append=True).clone())
        d["ctr"].add_(1)
    eager = torch.stack(eager).cpu()
    ring_eager = d["ring"].cpu()
    assert d["ring_len"].tolist() == [START + 8] * B

    out = torch.empty(B, dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _call(logits, d, append=True, out=out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _call(logits, d, append=True, out=out)
        d["ctr"].add_(1)
    reset()
    replay = []
    for t in range(8):
        graph.replay()
        replay.append(out.clone())
    replay = torch.stack(replay).cpu()
    assert torch.equal(replay, eager)
    assert d["ring_len"].tolist() == [START + 8] * B
    assert d["ctr"].tolist() == [8] * B
    ring = d["ring"].cpu()
    assert torch.equal(ring, ring_eager)
    for t in range(8):
        assert torch.equal(ring[:, (START + t) % RING], replay[t])
    # untouched slots keep their contents
    keep = [j for j in range(RING)
            if j not in {(START + t) % RING for t in range(8)}]
    assert torch.equal(ring[:, keep], ring0[:, keep])
    # presence 1e3: a token appended by one replay is out of reach of the next
    for b in range(B):
        toks = replay[:, b].tolist()
        assert len(set(toks)) == 8, toks
        assert not set(toks) & set(
            ref.ring_window_ref(ring0[b], START, 64)), toks


# ------------------------------------------------- 6. sample_tokens contract

def test_sample_tokens_contract_on_rebuilt_path():
    torch.manual_seed(26)
    B, V = 4, 1000
    logits_cpu = torch.randn(B, V)
    for b in range(B):
        _assert_distinct_top65(logits_cpu[b])
        _assert_argmax_gap(logits_cpu[b])
    logits = logits_cpu.to(DEV)
    seeds = torch.randint(1, 2**62, (B,), dtype=torch.int64, device=DEV)
    toks = ops.sample_tokens(logits, seeds, top_k=40, temperature=0.0,
                             top_p=1.0)
    assert toks.dtype == torch.int32
    assert torch.equal(toks.long().cpu(), logits_cpu.argmax(-1))
    k = 16
    topk_sets = [set(logits_cpu[b].topk(k).indices.tolist()) for b in range(B)]
    for trial in range(5):
        seeds = torch.randint(1, 2**62, (B,), dtype=torch.int64, device=DEV)
        before = seeds.clone()
        toks = ops.sample_tokens(logits, seeds, top_k=k, temperature=1.0,
                                 top_p=1.0)
        for b in range(B):
            assert int(toks[b]) in topk_sets[b]
        assert torch.equal(seeds, before), "seeds are read-only now"
    # top-p cut: one dominant logit under a small top_p is always picked
    peaked = torch.full((2, V), -10.0, device=DEV)
    peaked[:, 123] = 10.0
    peaked[:, 456] = 5.0
    for trial in range(3):
        seeds = torch.randint(1, 2**62, (2,), dtype=torch.int64, device=DEV)
        toks = ops.sample_tokens(peaked, seeds, top_k=40, temperature=1.0,
                                 top_p=0.5)
        assert toks.tolist() == [123, 123]
