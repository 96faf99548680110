"""The engine's host-side step planning (engine/step_plan.py), pinned without
a GPU: q-tile cutting, prefill chunk assembly and graph padding, the decode
plan (graph or eager, steps, bucket, attention band), token acceptance and
penalty-ring packing. Every expectation is written out by hand."""
import inspect

import pytest
import torch

from room_amd import ops
from room_amd.engine import llm, step_plan
from room_amd.engine import tokenizer as tok
from room_amd.engine.llm import PREFILL_BUCKETS, PREFILL_MAX_ROWS, RING, GenRequest
from room_amd.engine.step_plan import (accept_tokens, pack_ring, plan_decode,
                                       plan_prefill, prefill_graph_shape,
                                       qtile_list)


def test_planner_is_device_free():
    assert "cuda" not in inspect.getsource(step_plan)


# ---- q-tiles

def test_qtile_list():
    assert qtile_list([(0, 70), (70, 5)], 32) == [(0, 32), (32, 32), (64, 6),
                                                  (70, 5)]
    assert qtile_list([], 32) == []
    assert qtile_list([(0, 32)], 32) == [(0, 32)]
    assert qtile_list([(5, 33)], 32) == [(5, 32), (37, 1)]
    assert qtile_list([(0, 40)], 16) == [(0, 16), (16, 16), (32, 8)]


def test_build_qtile_desc_wraps_the_one_cutter():
    assert ops.flash_prefill_qtile() == 32
    desc = ops.build_qtile_desc([(0, 70), (70, 5)], "cpu")
    assert desc.dtype == torch.int32
    assert desc.tolist() == [[0, 32], [32, 32], [64, 6], [70, 5]]
    empty = ops.build_qtile_desc([], "cpu")
    assert empty.dtype == torch.int32 and tuple(empty.shape) == (0, 2)


# ---- prefill

def _req(pending, slot, pos=0, **kw):
    return GenRequest(prompt_tokens=list(pending), slot=slot, pos=pos,
                      pending_prefill=list(pending), **kw)


def test_plan_prefill_chunks_a_long_prompt():
    a = _req(range(5000), slot=3)
    b = _req(range(7000, 7010), slot=5)
    p = plan_prefill([a, b])
    # the budget is spent on A: B waits for the next chunk
    assert p.tokens == list(range(4096))
    assert p.seq_ids == [3] * 4096
    assert p.q_pos == list(range(4096))
    assert p.segments == [(0, 4096)]
    assert p.last_rows == [] and p.sampled_reqs == []
    assert p.capacity == [(3, 4096)]
    assert a.pos == 4096 and a.pending_prefill == list(range(4096, 5000))
    assert b.pos == 0 and len(b.pending_prefill) == 10

    p = plan_prefill([a, b])
    assert p.segments == [(0, 904), (904, 10)]
    assert p.tokens == list(range(4096, 5000)) + list(range(7000, 7010))
    assert p.seq_ids == [3] * 904 + [5] * 10
    assert p.q_pos == list(range(4096, 5000)) + list(range(10))
    assert p.last_rows == [903, 913]
    assert len(p.sampled_reqs) == 2
    assert p.sampled_reqs[0] is a and p.sampled_reqs[1] is b
    assert p.capacity == [(3, 5000), (5, 10)]
    assert (a.pos, b.pos) == (5000, 10)
    assert a.pending_prefill == [] and b.pending_prefill == []


def test_plan_prefill_starts_at_the_reused_position():
    r = _req([9, 8, 7, 6, 5], slot=2, pos=37)      # session reuse: 37 in KV
    p = plan_prefill([r])
    assert p.q_pos == [37, 38, 39, 40, 41]
    assert p.capacity == [(2, 42)] and r.pos == 42
    assert p.last_rows == [4] and p.sampled_reqs[0] is r


def test_plan_prefill_budget_argument():
    a, b = _req([1, 2, 3], slot=0), _req([4, 5, 6], slot=1)
    p = plan_prefill([a, b], budget=4)
    assert p.tokens == [1, 2, 3, 4] and p.segments == [(0, 3), (3, 1)]
    assert p.last_rows == [2] and p.sampled_reqs[0] is a
    assert b.pending_prefill == [5, 6] and b.pos == 1


def test_prefill_graph_shape_pads_in_a_copy():
    segments = [(0, 600)]
    tb, padded = prefill_graph_shape(600, segments)
    assert tb == 1024 and padded == [(0, 600), (600, 424)]
    assert segments == [(0, 600)]                 # the eager fallback's list
    segments = [(0, 500), (500, 12)]
    tb, padded = prefill_graph_shape(512, segments)
    assert tb == 512 and padded == [(0, 500), (500, 12)]
    assert padded is not segments and segments == [(0, 500), (500, 12)]
    assert prefill_graph_shape(9, [(0, 9)]) == (512, [(0, 9), (9, 503)])
    assert prefill_graph_shape(4096, [(0, 4096)]) == (4096, [(0, 4096)])


@pytest.mark.parametrize("tb", PREFILL_BUCKETS)
def test_padded_tiles_fit_the_graph_descriptor(tb):
    # 8 ragged segments: seven end one row into a fresh tile, the last leaves
    # a single pad row, so every segment and the pad waste most of a tile
    counts = [33] * 7 + [tb - 1 - 7 * 33]
    segments, row = [], 0
    for c in counts:
        segments.append((row, c))
        row += c
    assert row == tb - 1
    got_tb, padded = prefill_graph_shape(row, segments)
    assert got_tb == tb and padded[-1] == (tb - 1, 1) and len(padded) == 9
    tiles = qtile_list(padded, 32)
    assert len(tiles) == 7 * 2 + -(-counts[-1] // 32) + 1
    assert len(tiles) <= tb // 32 + PREFILL_MAX_ROWS + 2


# ---- decode

def _pd(n, positions=None, remaining=None, wide_rows=(11, 64), enabled=True,
        broken=False, wide_broken=False):
    return plan_decode(n, positions or [10] * n, remaining or [40] * n,
                       wide_rows, enabled, broken, wide_broken)


def test_plan_decode_graph_or_eager():
    assert _pd(5) == (False, True, 32, 5, 32)   # wide, graph, steps, bucket, band
    p = _pd(12)
    assert p.use_graph and p.wide and p.bucket == 16 and p.steps == 32
    for n in (9, 10):                    # between the narrow and wide ranges
        assert _pd(n) == (False, False, 1, None, 32)
    p = _pd(12, wide_broken=True)
    assert not p.use_graph and p.wide and p.steps == 1
    assert _pd(5, wide_broken=True).use_graph
    for n in (1, 5, 8, 12, 64):
        assert not _pd(n, broken=True).use_graph
        assert not _pd(n, enabled=False).use_graph
        assert _pd(n, broken=True).wide == (n >= 11)
    p = _pd(12, wide_rows=None)
    assert not p.use_graph and not p.wide
    assert _pd(8).bucket == 8 and _pd(11).bucket == 16
    assert _pd(33).bucket == 64 and _pd(64).use_graph and _pd(64).wide


def test_plan_decode_steps_follow_the_smallest_budget():
    assert _pd(3, remaining=[9, 3, 40]).steps == 3
    assert _pd(3, remaining=[9, 0, 40]).steps == 1
    assert _pd(3, remaining=[500, 600, 700]).steps == 32
    assert _pd(3, remaining=[2, 2, 2], enabled=False).steps == 1


def test_plan_decode_band_edges():
    # graph: the span at the END of the block decides
    assert _pd(1, positions=[16351], remaining=[32]).band == 32   # 16383
    assert _pd(1, positions=[16352], remaining=[32]).band == 64   # 16384
    assert _pd(2, positions=[7, 16380], remaining=[3, 9]).band == 32
    assert _pd(2, positions=[16381, 7], remaining=[3, 9]).band == 64
    # eager: the span at the start of the step
    assert _pd(1, positions=[16383], remaining=[32], enabled=False).band == 32
    assert _pd(1, positions=[16384], remaining=[32], enabled=False).band == 64
    assert _pd(9, positions=[5] * 8 + [16383]).band == 32
    assert _pd(9, positions=[5] * 8 + [16384]).band == 64
    assert step_plan.LONG_CONTEXT == 16384


# ---- token acceptance

def _lanes(hist, bucket, n, steps):
    return [hist[s * bucket: s * bucket + n] for s in range(steps)]


@pytest.mark.parametrize("stop", [tok.EOS, tok.IM_END])
def test_accept_block_stops_at_a_stop_token(stop):
    a = GenRequest(prompt_tokens=[1], max_new_tokens=10, pos=100)
    b = GenRequest(prompt_tokens=[1], max_new_tokens=10, pos=200)
    hist = [999] * 48                    # 3 steps of a 16-lane bucket
    hist[0], hist[1] = 11, 21
    hist[16], hist[17] = stop, 22
    hist[32], hist[33] = 13, 23
    finished = accept_tokens([a, b], _lanes(hist, 16, 2, 3), advance_pos=True)
    assert a.out_tokens == [11, stop] and a.pos == 102 and a.last_token == stop
    assert b.out_tokens == [21, 22, 23] and b.pos == 203 and b.last_token == 23
    assert len(finished) == 1 and finished[0] is a


def test_accept_stops_at_max_new_tokens():
    a = GenRequest(prompt_tokens=[1], max_new_tokens=1, pos=7)
    b = GenRequest(prompt_tokens=[1], max_new_tokens=3, pos=9)
    finished = accept_tokens([a, b], [[11, 21], [12, 22], [13, 23]], True)
    assert a.out_tokens == [11] and a.pos == 8
    assert b.out_tokens == [21, 22, 23] and b.pos == 12
    assert [id(r) for r in finished] == [id(a), id(b)]


def test_accept_orders_finished_by_step_then_request():
    a = GenRequest(prompt_tokens=[1], max_new_tokens=2)
    b = GenRequest(prompt_tokens=[1], max_new_tokens=2)
    c = GenRequest(prompt_tokens=[1], max_new_tokens=9)
    finished = accept_tokens([a, b, c], [[1, 2, 3], [4, 5, 6], [7, 8, 9]], True)
    assert [id(r) for r in finished] == [id(a), id(b)]
    assert c.out_tokens == [3, 6, 9] and a.out_tokens == [1, 4]
    # a later request that finishes first comes first
    a = GenRequest(prompt_tokens=[1], max_new_tokens=2)
    b = GenRequest(prompt_tokens=[1], max_new_tokens=1)
    finished = accept_tokens([a, b], [[1, 2], [3, 4]], True)
    assert [id(r) for r in finished] == [id(b), id(a)]
    assert b.out_tokens == [2] and a.out_tokens == [1, 3]


def test_accept_single_row_leaves_pos_alone():
    a = GenRequest(prompt_tokens=[1], max_new_tokens=5, pos=41)
    b = GenRequest(prompt_tokens=[1], max_new_tokens=5, pos=17)
    finished = accept_tokens([a, b], [[12, tok.EOS]], advance_pos=False)
    assert (a.pos, b.pos) == (41, 17)
    assert a.out_tokens == [12] and a.last_token == 12
    assert b.out_tokens == [tok.EOS]
    assert len(finished) == 1 and finished[0] is b


# ---- penalty ring

def test_pack_ring():
    assert RING == 256
    ring = torch.full((4, RING), -1, dtype=torch.int32)
    full = list(range(1000, 1000 + RING))
    pack_ring([[], [5, 6, 7], full, []], ring)
    assert ring[0].tolist() == [-1] * RING           # empty window: untouched
    assert ring[1].tolist() == [5, 6, 7] + [-1] * (RING - 3)
    assert ring[2].tolist() == full
    assert ring[3].tolist() == [-1] * RING


# ---- what the rest of the project imports from engine.llm

@pytest.mark.parametrize("name", [
    "LocalEngine", "GenRequest", "get_local_engine", "set_local_engine",
    "DECODE_BUCKETS", "WIDE_DECODE_DEFAULT", "WIDE_DECODE_MAX",
    "decode_bucket", "wide_decode_range", "expert_dtype_from_env",
    "validate_sampling", "_sampling_rows", "PREFILL_BUCKETS",
    "PREFILL_MAX_ROWS", "PREFILL_CHUNK", "RING"])
def test_llm_import_surface(name):
    assert hasattr(llm, name)


def test_llm_constants_keep_their_values():
    assert llm.DECODE_BUCKETS == (1, 2, 3, 4, 5, 6, 7, 8, 16, 32, 64)
    assert llm.WIDE_DECODE_DEFAULT == (11, 64) and llm.WIDE_DECODE_MAX == 64
    assert llm.PREFILL_BUCKETS == (512, 1024, 2048, 4096)
    assert llm.PREFILL_MAX_ROWS == 8 and llm.PREFILL_CHUNK == 4096
    assert step_plan.KMAX == 32
