"""hipGraph wrappers for LocalEngine: the multi-step decode block and the
bucketed prefill chunk. Each captures the model's forward against device
tensors it owns and replays it from pinned host staging."""
from __future__ import annotations

import sys
import time

import torch

from .. import ops
from .request import RING, GenRequest, _sampling_rows
from .step_plan import KMAX, PREFILL_MAX_ROWS, pack_ring


class _DecodeGraph:
    """One captured hipGraph per (batch bucket, context band), replayed K
    steps per host sync (multi-step decode).

    Inside the capture: forward → fused per-row sampler → token-history
    append (device step counter) → sampled tokens copied into the next step's
    input → positions += 1. The sampler reads every parameter per lane from
    device tensors this graph owns, draws from (lane seed, position) and
    pushes its token into the lane's penalty ring, so one capture serves any
    mix of requests and a block of K replays runs K full decode steps with
    ZERO host work; the host reads the K×B token history once at the end.
    Buckets ≤ 8 are exact; the wide buckets (16/32/64, forwards in the
    model's wide mode) run padded lanes. A padded lane uses the reserved pad
    slot at position 0 with token 0, samples greedily with penalties off,
    and advances with the block like any lane: its KV writes go to the pad
    slot's own block for positions 0..15 and, past that block, through the
    slot's zero block-table entries into the reserved scrap block 0. All
    padded lanes of a step are identical, and no request reads either
    block."""

    def __init__(self, engine, bucket: int):
        self.bucket = bucket
        self.pad_slot = engine.pad_slot
        dev = engine.device
        # lane state packed by dtype: three H2D copies fill a block's inputs.
        # i32: rows seq, pos, top_k, repeat_last_n, ring_len, then the
        # [bucket, RING] ring (copied only when a lane has penalties on)
        # i64 rows: tok, seed;  f32 rows: temperature, top_p, rep, pres, freq
        nrow = 5 * bucket
        self.i32 = torch.zeros(nrow + bucket * RING, dtype=torch.int32,
                               device=dev)
        self.i64 = torch.zeros(2, bucket, dtype=torch.int64, device=dev)
        self.f32 = torch.zeros(5, bucket, dtype=torch.float32, device=dev)
        rows = self.i32[:nrow].view(5, bucket)
        rows[0] = engine.pad_slot
        rows[2] = 1
        self.f32[1:3] = 1.0
        self.h_i32 = self.i32.cpu().pin_memory()
        self.h_i64 = self.i64.cpu().pin_memory()
        self.h_f32 = self.f32.cpu().pin_memory()
        self.h_rows = self.h_i32[:nrow].view(5, bucket)
        self.h_ring = self.h_i32[nrow:].view(bucket, RING)
        self.tok_in, self.seeds = self.i64.unbind(0)
        (self.seq_in, self.pos_in, self.top_k, self.last_n,
         self.ring_len) = rows.unbind(0)
        self.ring = self.i32[nrow:].view(bucket, RING)
        (self.temperature, self.top_p, self.rep, self.pres,
         self.freq) = self.f32.unbind(0)
        self.hist = torch.zeros(KMAX * bucket, dtype=torch.int32, device=dev)
        self.ctr = torch.zeros(1, dtype=torch.int32, device=dev)
        self.hist_host = torch.zeros(KMAX * bucket, dtype=torch.int32,
                                     pin_memory=True)
        model, cache = engine.model, engine.cache
        C = ops._require()

        def run_step():
            logits = model.forward(self.tok_in, self.seq_in, self.pos_in,
                                   cache.block_table, cache.kcaches,
                                   cache.vcaches, kscales=cache.kscales,
                                   vscales=cache.vscales)
            toks = torch.empty(bucket, dtype=torch.int32, device=dev)
            C.sample_rows(toks, logits, self.temperature, self.top_p,
                          self.top_k, self.seeds, self.pos_in, self.rep,
                          self.pres, self.freq, self.last_n, self.ring,
                          self.ring_len, True)
            C.hist_append(self.hist, self.ctr, toks, KMAX)
            self.tok_in.copy_(toks)      # feed the next replay
            self.pos_in.add_(1)

        # warmup on a side stream (required before capture)
        strm = torch.cuda.Stream(dev)
        strm.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(strm):
            for _ in range(2):
                run_step()
        torch.cuda.current_stream(dev).wait_stream(strm)
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        # thread_local: agents' encoder/embedding work on other threads may
        # call the allocator mid-capture; global mode corrupts those calls
        with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
            run_step()

    def run_block(self, reqs: list[GenRequest], k: int) -> list[int]:
        """Run k decode steps; returns the flat K×B token history (host).
        The previous block's closing D2H copy synced the stream, so the
        pinned staging is free to overwrite."""
        n, b = len(reqs), self.bucket
        pad = b - n
        k = min(k, KMAX)
        i32, f32, seeds, wins = _sampling_rows(reqs, pad)
        self.h_rows.copy_(torch.tensor(
            [[r.slot for r in reqs] + [self.pad_slot] * pad,
             [r.pos for r in reqs] + [0] * pad] + i32, dtype=torch.int32))
        self.h_i64.copy_(torch.tensor(
            [[r.last_token for r in reqs] + [0] * pad, seeds],
            dtype=torch.int64))
        self.h_f32.copy_(torch.tensor(f32, dtype=torch.float32))
        nrow = 5 * b
        if any(wins):
            pack_ring(wins, self.h_ring)
            self.i32.copy_(self.h_i32, non_blocking=True)
        else:
            self.i32[:nrow].copy_(self.h_i32[:nrow], non_blocking=True)
        self.i64.copy_(self.h_i64, non_blocking=True)
        self.f32.copy_(self.h_f32, non_blocking=True)
        self.ctr.zero_()
        for _ in range(k):
            self.graph.replay()
        self.hist_host[:k * b].copy_(self.hist[:k * b])  # syncs
        return self.hist_host[:k * b].tolist()


class _PrefillGraph:
    """One captured hipGraph per prefill bucket size.

    The prefill forward was built host-sync-free (device-side MoE tile
    descriptors, tensor-driven rope/attention), but launching its ~700
    python-level ops costs ~30 ms per chunk — more than the GPU compute it
    enqueues, so prefill ran launch-bound. Chunks are padded to a few fixed
    bucket shapes (pad rows target the engine's scrap pad slot; zero-count
    q-tiles no-op in flash_prefill) and each bucket's whole forward replays
    as one graph. logits are always computed for PREFILL_MAX_ROWS fixed row
    slots; the scheduler slices the real ones."""

    def __init__(self, engine, tb: int):
        t0 = time.time()
        print(f"[room_amd] capturing prefill graph tb={tb} ...",
              file=sys.stderr, flush=True)
        dev = engine.device
        self.tb = tb
        self.pad_slot = engine.pad_slot
        # worst case: 8 request segments + 1 pad segment, each wasting <1 tile
        self.gmax = tb // ops.flash_prefill_qtile() + PREFILL_MAX_ROWS + 2
        self.tok = torch.zeros(tb, dtype=torch.int64, device=dev)
        self.seq = torch.full((tb,), engine.pad_slot, dtype=torch.int32,
                              device=dev)
        self.pos = torch.zeros(tb, dtype=torch.int32, device=dev)
        self.rows = torch.zeros(PREFILL_MAX_ROWS, dtype=torch.int64, device=dev)
        self.qtiles = torch.zeros(self.gmax, 2, dtype=torch.int32, device=dev)
        # pinned staging
        self.h_tok = torch.zeros(tb, dtype=torch.int64, pin_memory=True)
        self.h_seq = torch.full((tb,), engine.pad_slot, dtype=torch.int32,
                                pin_memory=True)
        self.h_pos = torch.zeros(tb, dtype=torch.int32, pin_memory=True)
        self.h_rows = torch.zeros(PREFILL_MAX_ROWS, dtype=torch.int64,
                                  pin_memory=True)
        self.h_qtiles = torch.zeros(self.gmax, 2, dtype=torch.int32,
                                    pin_memory=True)
        # guards pinned-staging reuse: back-to-back same-bucket chunks (long
        # prompts, nothing sampled between) would otherwise overwrite h_* on
        # the host while the previous run's async H2D copies are in flight
        self.copied = torch.cuda.Event()
        model, cache = engine.model, engine.cache
        model.capture_gemm = True   # hipBLASLt is not capture-safe

        def run_fwd():
            return model.forward(self.tok, self.seq, self.pos,
                                 cache.block_table, cache.kcaches,
                                 cache.vcaches, logits_rows=self.rows,
                                 qtile_desc=self.qtiles,
                                 kscales=cache.kscales, vscales=cache.vscales)

        # warmup on the CURRENT stream, not a side stream: the canonical
        # side-stream warmup HANGS on the 30b config at tb=512 (bisected in
        # scripts/gpu_pg_bisect.py — warmup-only on a side stream deadlocks;
        # the identical forward on the default stream warms up, captures and
        # replays green). torch.cuda.graph still captures on its own stream.
        for _ in range(2):
            run_fwd()
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(self.graph,
                                  capture_error_mode="thread_local"):
                self.logits = run_fwd()        # [PREFILL_MAX_ROWS, vocab] f32
        finally:
            model.capture_gemm = False
        print(f"[room_amd] prefill graph tb={tb} captured "
              f"in {time.time() - t0:.1f}s", file=sys.stderr, flush=True)

    def run(self, tokens: list[int], seq_ids: list[int], q_pos: list[int],
            last_rows: list[int], qtiles_host: list) -> torch.Tensor:
        n = len(tokens)
        self.copied.synchronize()   # previous call's H2D copies done
        self.h_tok[:n] = torch.tensor(tokens, dtype=torch.int64)
        self.h_tok[n:] = 0
        self.h_seq[:n] = torch.tensor(seq_ids, dtype=torch.int32)
        self.h_seq[n:] = self.pad_slot
        self.h_pos[:n] = torch.tensor(q_pos, dtype=torch.int32)
        self.h_pos[n:] = 0
        k = len(last_rows)
        self.h_rows[:k] = torch.tensor(last_rows, dtype=torch.int64)
        self.h_rows[k:] = 0
        g = len(qtiles_host)
        self.h_qtiles[:g] = torch.tensor(qtiles_host, dtype=torch.int32)
        self.h_qtiles[g:] = 0                  # zero-count tiles: no-op
        self.tok.copy_(self.h_tok, non_blocking=True)
        self.seq.copy_(self.h_seq, non_blocking=True)
        self.pos.copy_(self.h_pos, non_blocking=True)
        self.rows.copy_(self.h_rows, non_blocking=True)
        self.qtiles.copy_(self.h_qtiles, non_blocking=True)
        self.copied.record()
        self.graph.replay()
        return self.logits
