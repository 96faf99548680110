"""Per-request sampling parameters, CPU side: the plain-torch sampler
reference on hand-computed values, request validation, and the way the new
fields travel through AgentExecutionOptions, chat() and the HTTP payload."""
import pytest
import torch

from room_amd.engine import llm
from room_amd.engine.cloud_providers import HttpChatEngine
from room_amd.engine.types import AgentExecutionOptions
from room_amd.ops import reference as ref

LOGITS = torch.tensor([2.0, -1.0, 0.5, 3.0, -2.0, 1.0])


def test_apply_penalties_positive_and_negative_branches():
    # token 0 (x > 0, once): 2/2 − (1·0.5 + 0.25) = 0.25
    # token 1 (x < 0, once): −1·2 − 0.75 = −2.75
    out = ref.apply_penalties_ref(LOGITS, [0, 1], 2.0, 0.25, 0.5)
    assert torch.allclose(out, torch.tensor([0.25, -2.75, 0.5, 3.0, -2.0, 1.0]))
    assert torch.equal(LOGITS, torch.tensor([2.0, -1.0, 0.5, 3.0, -2.0, 1.0]))


def test_apply_penalties_count_three():
    # token 3 three times: 3/1.5 − (3·0.5 + 0.25) = 0.25; token 4 once:
    # −2·1.5 − (0.5 + 0.25) = −3.75; ids outside the vocabulary are ignored
    out = ref.apply_penalties_ref(LOGITS, [3, 4, 3, 3, 6, -1], 1.5, 0.25, 0.5)
    assert torch.allclose(out, torch.tensor([2.0, -1.0, 0.5, 0.25, -3.75, 1.0]))


def test_apply_penalties_off_is_identity():
    assert torch.equal(ref.apply_penalties_ref(LOGITS, [0, 3], 1.0, 0.0, 0.0),
                       LOGITS)
    assert torch.equal(ref.apply_penalties_ref(LOGITS, [], 2.0, 1.0, 1.0),
                       LOGITS)


def test_sample_dist_top_p_crossing_token_included():
    # probabilities 0.5, 0.25, 0.125, 0.0625, …; top_k = 4 keeps the first
    # four (sum 0.9375 → 8/15, 4/15, 2/15, 1/15). Cumulative 0.533, 0.8,
    # 0.933: top_p = 0.7 is crossed by the second token, which stays.
    x = torch.log(torch.tensor([0.5, 0.25, 0.125, 0.0625, 0.03125, 0.03125]))
    p = ref.sample_dist_ref(x, [], dict(temperature=1.0, top_p=0.7, top_k=4))
    assert torch.allclose(p, torch.tensor([2 / 3, 1 / 3, 0, 0, 0, 0],
                                          dtype=p.dtype))
    # top_p = 1 keeps all four
    p = ref.sample_dist_ref(x, [], dict(temperature=1.0, top_p=1.0, top_k=4))
    assert torch.allclose(p, torch.tensor([8, 4, 2, 1, 0, 0], dtype=p.dtype) / 15)
    # temperature 0.5 squares the ratios: 64 : 16 : 4 : 1
    p = ref.sample_dist_ref(x, [], dict(temperature=0.5, top_p=1.0, top_k=4))
    assert torch.allclose(p, torch.tensor([64, 16, 4, 1, 0, 0], dtype=p.dtype) / 85)


def test_sample_dist_penalties_first_then_greedy():
    # presence 2.5 on token 3 (3.0 → 0.5) leaves token 0 (2.0) on top
    p = ref.sample_dist_ref(LOGITS, [3], dict(
        temperature=0.0, top_p=1.0, top_k=3, presence_penalty=2.5))
    assert p.tolist() == [1, 0, 0, 0, 0, 0]
    # and the penalised token drops out of a top-2
    p = ref.sample_dist_ref(LOGITS, [3], dict(
        temperature=1.0, top_p=1.0, top_k=2, presence_penalty=2.5))
    e = torch.tensor([2.0, 1.0]).exp()
    assert torch.allclose(p[[0, 5]].float(), e / e.sum())
    assert float(p[3]) == 0


def test_ring_window():
    ring = torch.arange(1000, 1256, dtype=torch.int32)       # push j → 1000+j
    assert ref.ring_window_ref(ring, 5, 64) == [1000, 1001, 1002, 1003, 1004]
    assert ref.ring_window_ref(ring, 5, 2) == [1003, 1004]
    assert ref.ring_window_ref(ring, 5, 0) == []
    assert ref.ring_window_ref(ring, 0, 64) == []
    # wrapped: 300 pushes, push j ≥ 256 overwrote slot j − 256
    wrapped = ring.clone()
    for j in range(256, 300):
        wrapped[j % 256] = 5000 + j
    got = ref.ring_window_ref(wrapped, 300, 64)
    want = [1000 + j for j in range(236, 256)] + [5000 + j for j in range(256, 300)]
    assert got == want
    # n = 256: the oldest surviving push is 300 − 256 = 44
    full = ref.ring_window_ref(wrapped, 300, 256)
    assert len(full) == 256 and full[0] == 1044 and full[-1] == 5299


@pytest.mark.parametrize("kw", [
    dict(temperature=-0.1), dict(temperature=float("nan")),
    dict(top_p=0.0), dict(top_p=1.5), dict(top_k=0), dict(top_k=65),
    dict(top_k=2.5), dict(repetition_penalty=0.0),
    dict(repetition_penalty=-1.0), dict(repeat_last_n=-1),
    dict(repeat_last_n=257), dict(seed=-1), dict(seed=2**63),
    dict(temperature=float("inf")), dict(repetition_penalty=float("inf")),
    dict(presence_penalty=float("nan")), dict(presence_penalty=float("inf")),
    dict(frequency_penalty=float("nan")), dict(frequency_penalty=-float("inf")),
])
def test_generate_rejects_out_of_range(kw):
    # validation comes first in generate(): an engine that was never
    # constructed (no device, no queue) is enough to reach it
    eng = object.__new__(llm.LocalEngine)
    with pytest.raises(ValueError):
        eng.generate([1, 2, 3], **kw)


def test_validator_accepts_the_edges():
    llm.validate_sampling(0.0, 1.0, 1, 0.01, 0)
    llm.validate_sampling(2.0, 1e-6, 64, 5.0, 256, seed=2**63 - 1)
    llm.validate_sampling(0.7, 0.95, 40)
    llm.validate_sampling(0.7, 0.95, 40, presence_penalty=-2.0,
                          frequency_penalty=1e3)


def test_request_seed_and_penalty_window():
    r = llm.GenRequest(prompt_tokens=[1, 2, 3])
    assert 0 <= r.seed < 2**62
    assert len({llm.GenRequest(prompt_tokens=[1]).seed for _ in range(4)}) > 1
    assert llm.GenRequest(prompt_tokens=[1], seed=7).seed == 7
    assert not r.penalised and r.penalty_window() == []     # defaults: off
    r = llm.GenRequest(prompt_tokens=[1, 2, 3, 4], presence_penalty=0.5,
                       repeat_last_n=3)
    assert r.penalty_window() == [2, 3, 4]
    r.out_tokens = [9, 8]
    assert r.penalty_window() == [4, 9, 8]
    r.out_tokens = [9, 8, 7, 6]
    assert r.penalty_window() == [8, 7, 6]
    r.repeat_last_n = 0
    assert r.penalty_window() == []
    # lanes: a request with penalties off gets repeat_last_n 0; pads are inert
    a = llm.GenRequest(prompt_tokens=[5, 6], temperature=0.3, top_k=7, seed=3)
    b = llm.GenRequest(prompt_tokens=[5, 6], repetition_penalty=1.1, seed=4)
    i32, f32, seeds, wins = llm._sampling_rows([a, b], pad=1)
    assert i32 == [[7, 40, 1], [0, 64, 0], [0, 2, 0]]
    assert f32[0] == [0.3, 0.7, 0.0] and f32[2] == [1.0, 1.1, 1.0]
    assert seeds == [3, 4, 0] and wins == [[], [5, 6]]


class _Capture(HttpChatEngine):
    def _request(self, payload, headers):
        self.payload = payload
        return {"choices": [{"message": {"content": "ok"}}], "usage": {}}


def test_http_payload_new_keys_only_when_set():
    eng = _Capture("openai:gpt-x", api_key="k")
    msgs = [{"role": "user", "content": "hi"}]
    eng.chat(msgs, [], AgentExecutionOptions(prompt="hi"))
    assert set(eng.payload) == {"model", "messages", "max_tokens", "temperature"}
    eng.chat(msgs, [], AgentExecutionOptions(
        prompt="hi", seed=0, presence_penalty=0.5, frequency_penalty=-0.25))
    assert eng.payload["seed"] == 0
    assert eng.payload["presence_penalty"] == 0.5
    assert eng.payload["frequency_penalty"] == -0.25
    eng.chat(msgs, [], AgentExecutionOptions(prompt="hi", frequency_penalty=1.0))
    assert "seed" not in eng.payload and "presence_penalty" not in eng.payload
    assert eng.payload["frequency_penalty"] == 1.0


def test_options_pass_through_chat():
    seen = {}

    class Req:
        out_tokens = [1, 2]

    eng = object.__new__(llm.LocalEngine)

    def fake_generate(prompt, **kw):
        seen.update(kw)
        return Req()

    eng.generate = fake_generate
    opts = AgentExecutionOptions(prompt="x", seed=42, repetition_penalty=1.1,
                                 presence_penalty=0.2, frequency_penalty=0.3,
                                 repeat_last_n=128, temperature=0.1, top_k=5)
    text, n_in, n_out = eng.chat([{"role": "user", "content": "x"}], [], opts)
    assert n_out == 2
    assert seen["seed"] == 42
    assert seen["repetition_penalty"] == 1.1
    assert seen["presence_penalty"] == 0.2
    assert seen["frequency_penalty"] == 0.3
    assert seen["repeat_last_n"] == 128
    assert seen["temperature"] == 0.1 and seen["top_k"] == 5
    # defaults: penalties off, random seed
    d = AgentExecutionOptions(prompt="x")
    assert (d.seed, d.repetition_penalty, d.presence_penalty,
            d.frequency_penalty, d.repeat_last_n) == (None, 1.0, 0.0, 0.0, 64)
