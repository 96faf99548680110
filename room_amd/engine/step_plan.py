"""Device-free step planning for LocalEngine: every host-side decision a
prefill chunk or a decode block makes, and the acceptance of sampled tokens.
Like admission.py, arithmetic over Python lists kept apart from the scheduler
thread so that CPU tests run it: it calls no op, touches no KV cache and
allocates no device tensor."""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import tokenizer as tok

PREFILL_CHUNK = 4096          # max tokens per prefill forward
PREFILL_BUCKETS = (512, 1024, 2048, 4096)   # graph-captured chunk shapes
PREFILL_MAX_ROWS = 8                         # fixed logits-row slots
DECODE_BUCKETS = (1, 2, 3, 4, 5, 6, 7, 8, 16, 32, 64)  # hipGraph capture sizes
# ≤8 buckets are exact (padding inflates MoE pair traffic ~linearly); the
# wide ones are multiples of 16, the skinny GEMM's MFMA fragment height
KMAX = 32                     # most decode steps per graph block
LONG_CONTEXT = 16384          # KV span from which decode uses 64 splits


def decode_bucket(n: int) -> int:
    """Graph bucket for n concurrent decode requests (n ≤ 64)."""
    return next(b for b in DECODE_BUCKETS if b >= n)


def qtile_list(segments: list, qt: int) -> list:
    """(row0, count) segments → (row0, rows ≤ qt) q-tile descriptors, one
    sequence per tile."""
    return [(r, min(qt, row0 + count - r))
            for row0, count in segments
            for r in range(row0, row0 + count, qt)]


class PrefillPlan(NamedTuple):
    tokens: list        # the chunk's rows, request after request
    seq_ids: list
    q_pos: list
    segments: list      # (row0, count) per request — host-side q-tile info
    last_rows: list     # row of each completed prompt's last token
    sampled_reqs: list  # the requests those rows sample a first token for
    capacity: list      # (slot, tokens_needed) for cache.ensure_capacity


def plan_prefill(reqs: list, budget: int = PREFILL_CHUNK) -> PrefillPlan:
    """Assemble one prefill chunk from `reqs` in order until the budget is
    spent, advancing each taken request's pos and pending_prefill. The caller
    must ensure_capacity every `capacity` pair before the chunk runs."""
    p = PrefillPlan([], [], [], [], [], [], [])
    for r in reqs:
        if budget <= 0:
            break
        take = min(budget, len(r.pending_prefill))
        chunk = r.pending_prefill[:take]
        r.pending_prefill = r.pending_prefill[take:]
        p.capacity.append((r.slot, r.pos + take))
        p.segments.append((len(p.tokens), take))
        p.tokens.extend(chunk)
        p.seq_ids.extend([r.slot] * take)
        p.q_pos.extend(range(r.pos, r.pos + take))
        r.pos += take
        budget -= take
        if not r.pending_prefill:  # prompt complete → sample first token
            p.last_rows.append(len(p.tokens) - 1)
            p.sampled_reqs.append(r)
    return p


def prefill_graph_shape(n: int, segments: list,
                        buckets: tuple = PREFILL_BUCKETS) -> tuple[int, list]:
    """Bucket tb for an n-row chunk and its segments padded to tb. Pad rows
    live in their own 1-token-context segment — in a COPY: the eager fallback
    reuses `segments` against n-row tensors, so a leaked pad segment would
    read q rows past the tensor end."""
    tb = next(b for b in buckets if b >= n)
    return tb, segments + ([(n, tb - n)] if n < tb else [])


class DecodePlan(NamedTuple):
    wide: bool          # 9..64 requests in the model's wide mode
    use_graph: bool
    steps: int          # decode steps this block runs
    bucket: int | None  # graph lanes (None when eager)
    band: int           # attention splits


def plan_decode(n: int, positions: list, remaining: list, wide_rows,
                graphs_enabled: bool, graphs_broken: bool,
                wide_graphs_broken: bool) -> DecodePlan:
    """How n requests at `positions` with `remaining` token budgets decode."""
    # 9..64 requests: the model's wide mode, graph or eager alike
    wide = wide_rows is not None and wide_rows[0] <= n <= wide_rows[1]
    use_graph = (graphs_enabled and not graphs_broken
                 and (n <= 8 or (wide and not wide_graphs_broken)))
    # multi-step graph block: K bounded by the smallest remaining budget so
    # every request stops exactly at max_new (admission latency is K steps)
    steps = max(1, min(min(remaining), KMAX)) if use_graph else 1
    # context band: 64 attention splits once a sequence's KV span reaches
    # LONG_CONTEXT (shorter per-WG serial chunk chains), by the end of the
    # block on a graph and at its start in an eager step; banded graphs keep
    # each capture's grid fixed
    span = max(positions) + (steps if use_graph else 0)
    return DecodePlan(wide, use_graph, steps,
                      decode_bucket(n) if use_graph else None,
                      64 if span >= LONG_CONTEXT else 32)


def accept_tokens(reqs: list, rows: list, advance_pos: bool) -> list:
    """Append each step's sampled tokens (`rows`: one list per step, lane i
    for reqs[i]) and return the requests that finished, in finishing order:
    max_new_tokens reached, or the token is EOS or IM_END. A finished request
    ignores later rows; its last token is NOT yet in KV (a prompt extension
    re-runs it). advance_pos: a graph block advances pos per accepted token;
    an eager step and a prefill chunk advanced it before the forward."""
    finished, done = [], set()
    for row in rows:
        for i, (r, t) in enumerate(zip(reqs, row)):
            if i in done:
                continue
            t = int(t)
            r.last_token = t
            r.out_tokens.append(t)
            if advance_pos:
                r.pos += 1
            if (len(r.out_tokens) >= r.max_new_tokens
                    or t in (tok.EOS, tok.IM_END)):
                done.add(i)
                finished.append(r)
    return finished


def pack_ring(wins: list, out: torch.Tensor) -> None:
    """Write penalty windows into a [rows, RING] int32 host tensor. Push j
    lives at ring[j % RING]: a window of m ≤ RING tokens with ring_len = m
    sits at ring[0:m]. Rows with an empty window are left as they are."""
    for i, w in enumerate(wins):
        if w:
            out[i, :len(w)] = torch.tensor(w, dtype=torch.int32)
