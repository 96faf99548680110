"""The engine's request type, its sampling-parameter checks, and the per-row
sampler packing the decode graphs and the eager sampler share. Device-free."""
from __future__ import annotations

import math
import random
import threading
from dataclasses import dataclass, field
from typing import Optional

from .. import ops

RING = ops.RING   # token-history ring entries per sampler row


@dataclass
class GenRequest:
    prompt_tokens: list[int]
    max_new_tokens: int = 128
    temperature: float = 0.7
    top_p: float = 0.95
    top_k: int = 40
    seed: Optional[int] = None    # None → a random 62-bit seed per request
    repetition_penalty: float = 1.0
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    repeat_last_n: int = 64
    session_key: Optional[str] = None
    done: threading.Event = field(default_factory=threading.Event)
    out_tokens: list[int] = field(default_factory=list)
    error: Optional[str] = None
    prefill_tokens_run: int = 0   # actually-prefilled (after cache reuse)
    cancelled: bool = False       # set by the caller on timeout; scheduler drops
    # scheduler state
    slot: int = -1
    pos: int = 0                  # next position to write
    pending_prefill: list[int] = field(default_factory=list)
    last_token: int = -1

    def __post_init__(self):
        if self.seed is None:
            self.seed = random.getrandbits(62)

    @property
    def penalised(self) -> bool:
        return self.repeat_last_n > 0 and not (
            self.repetition_penalty == 1.0 and self.presence_penalty == 0.0
            and self.frequency_penalty == 0.0)

    def penalty_window(self) -> list[int]:
        """Tokens the next draw's penalties look at: the last repeat_last_n of
        prompt + output (empty when the request's penalties are off)."""
        if not self.penalised:
            return []
        n = self.repeat_last_n
        tail = self.out_tokens[-n:]
        if len(tail) < n:
            tail = self.prompt_tokens[-(n - len(tail)):] + tail
        return tail


def validate_sampling(temperature: float, top_p: float, top_k: int,
                      repetition_penalty: float = 1.0,
                      repeat_last_n: int = 64, seed: int | None = None,
                      presence_penalty: float = 0.0,
                      frequency_penalty: float = 0.0) -> None:
    """Range checks for a request's sampling parameters (ValueError). Every
    float must be finite: a NaN penalty would silently drop its tokens from
    the scan's compare chain."""
    for name, v in (("temperature", temperature),
                    ("repetition_penalty", repetition_penalty),
                    ("presence_penalty", presence_penalty),
                    ("frequency_penalty", frequency_penalty)):
        if not math.isfinite(v):
            raise ValueError(f"{name} must be finite, got {v}")
    if not temperature >= 0:
        raise ValueError(f"temperature must be >= 0, got {temperature}")
    if not 0 < top_p <= 1:
        raise ValueError(f"top_p must be in (0, 1], got {top_p}")
    if int(top_k) != top_k or not 1 <= top_k <= ops.MAX_TOP_K:
        raise ValueError(f"top_k must be an integer in 1..{ops.MAX_TOP_K}, "
                         f"got {top_k}")
    if not repetition_penalty > 0:
        raise ValueError("repetition_penalty must be > 0, "
                         f"got {repetition_penalty}")
    if int(repeat_last_n) != repeat_last_n or not 0 <= repeat_last_n <= RING:
        raise ValueError(f"repeat_last_n must be an integer in 0..{RING}, "
                         f"got {repeat_last_n}")
    if seed is not None and not 0 <= seed < 2**63:
        raise ValueError(f"seed must be in 0..2^63-1, got {seed}")


def _sampling_rows(reqs: list[GenRequest], pad: int = 0):
    """Host-side per-row sampler parameters for `reqs` plus `pad` inert lanes
    (greedy, penalties off): (i32 rows [top_k, repeat_last_n, ring_len],
    f32 rows [temperature, top_p, repetition, presence, frequency], seeds,
    windows). A request whose penalties are off gets repeat_last_n 0 and an
    empty window, so the scan skips the penalty work for its row."""
    wins = [r.penalty_window() for r in reqs]
    ones, zeros = [1.0] * pad, [0.0] * pad
    i32 = [[r.top_k for r in reqs] + [1] * pad,
           [r.repeat_last_n if r.penalised else 0 for r in reqs] + [0] * pad,
           [len(w) for w in wins] + [0] * pad]
    f32 = [[r.temperature for r in reqs] + zeros,
           [r.top_p for r in reqs] + ones,
           [r.repetition_penalty for r in reqs] + ones,
           [r.presence_penalty for r in reqs] + zeros,
           [r.frequency_penalty for r in reqs] + zeros]
    seeds = [r.seed for r in reqs] + [0] * pad
    return i32, f32, seeds, wins
