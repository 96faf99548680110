"""Wide decode (9..64 rows): the host-side decisions, pinned without a GPU —
which layer a forward runs, the kill switch, the graph bucket, and the
descriptor count of 16-row MoE tiles."""
from room_amd import ops
from room_amd.engine.llm import (DECODE_BUCKETS, WIDE_DECODE_DEFAULT,
                                 decode_bucket, wide_decode_range)
from room_amd.models.qwen3_moe import WIDE_MAX_ROWS, forward_mode


def test_forward_mode_routing():
    assert forward_mode(1, False) == "decode"
    assert forward_mode(8, False) == "decode"
    assert forward_mode(8, True) == "decode"
    assert forward_mode(9, False) == "wide"
    assert forward_mode(64, False) == "wide"
    assert forward_mode(9, True) == "prefill"      # a prefill chunk: q-tiles
    assert forward_mode(64, True) == "prefill"
    assert forward_mode(65, False) == "prefill"
    assert forward_mode(4096, True) == "prefill"
    assert WIDE_MAX_ROWS == 64 == ops.SKINNY_MAX_ROWS


def test_switch_overrides_routing():
    import pytest
    assert wide_decode_range({}) == WIDE_DECODE_DEFAULT
    assert wide_decode_range({"ROOMAMD_WIDE_DECODE": "1"}) == WIDE_DECODE_DEFAULT
    off = wide_decode_range({"ROOMAMD_WIDE_DECODE": "0"})
    assert off is None
    assert forward_mode(9, False, off) == "prefill"
    assert forward_mode(64, False, off) == "prefill"
    assert forward_mode(8, False, off) == "decode"        # narrow path as ever
    # an explicit range: the A/B lever
    assert wide_decode_range({"ROOMAMD_WIDE_DECODE": "9-64"}) == (9, 64)
    r = wide_decode_range({"ROOMAMD_WIDE_DECODE": "16-32"})
    assert r == (16, 32)
    assert forward_mode(15, False, r) == "prefill"
    assert forward_mode(16, False, r) == forward_mode(32, False, r) == "wide"
    assert forward_mode(33, False, r) == "prefill"
    assert forward_mode(20, True, r) == "prefill"
    for bad in ("8-64", "9-65", "32-16", "on", "12"):
        with pytest.raises(ValueError):
            wide_decode_range({"ROOMAMD_WIDE_DECODE": bad})
    # the measured default lies inside what the kernels serve
    lo, hi = WIDE_DECODE_DEFAULT
    assert 9 <= lo <= hi <= WIDE_MAX_ROWS
    assert forward_mode(lo, False, WIDE_DECODE_DEFAULT) == "wide"


def test_decode_bucket_choice():
    assert [decode_bucket(n) for n in range(1, 9)] == list(range(1, 9))
    assert decode_bucket(9) == 16
    assert decode_bucket(16) == 16
    assert decode_bucket(17) == 32
    assert decode_bucket(64) == 64
    # wide buckets match the MFMA fragment height
    assert all(b % 16 == 0 for b in DECODE_BUCKETS if b > 8)


def test_desc_gmax_for_16_row_tiles():
    # every expert can end in one ragged tile on top of the full ones
    assert ops.moe_desc_gmax(34, 4, bm=16) == 4 + 3
    assert ops.moe_desc_gmax(512, 128, bm=16) == 128 + 32   # 64 tokens, top-8
    assert ops.moe_desc_gmax(72, 128, bm=16) == 128 + 5     # 9 tokens
    assert ops.moe_desc_gmax(16, 1, bm=16) == 2
    # the default stays the 128-row count existing callers get
    assert ops.moe_desc_gmax(300, 4) == 4 + 3
    assert ops.moe_desc_gmax(4096 * 8, 128) == 128 + 256
