"""In-process GPU inference engine with continuous batching.

Replaces the reference's Ollama sidecar + HTTP hop (src/shared/local-model.ts,
agent-executor.ts:327-338). Agents call chat() from their own threads; a
single scheduler thread owns the GPU and fuses concurrent agents' work into
batched prefill/decode kernel launches — the control inversion SURVEY §7
calls out: per-agent cycle semantics unchanged, per-GPU kernels batched.

Sessions: chat() reuses the sequence slot (and its paged KV blocks) when the
new prompt extends the previous token stream — session-as-KV-cache, with the
agent_sessions SQLite row as the durable fallback.
"""
from __future__ import annotations

import math
import os
import queue
import random
import threading
import time
from dataclasses import dataclass, field
from typing import Optional

import torch

from .. import ops
from ..models.qwen3_moe import Qwen3MoEConfig, Qwen3MoEModel
from . import tokenizer as tok
from .admission import SessionAdmitter
from .kv_cache import BLOCK_SIZE, PagedKVCache
from .types import AgentExecutionOptions, ToolDef

PREFILL_CHUNK = 4096          # max tokens per prefill forward
DEFAULT_MAX_SEQS = 64
DECODE_BUCKETS = (1, 2, 3, 4, 5, 6, 7, 8, 16, 32, 64)  # hipGraph capture sizes
# ≤8 buckets are exact (padding inflates MoE pair traffic ~linearly); the
# wide ones are multiples of 16, the skinny GEMM's MFMA fragment height
WIDE_DECODE_MAX = DECODE_BUCKETS[-1]
# Wide decode runs where it measured faster than the prefill layer it replaces
# (30b, scripts/gpu_wide_decode_micro.py against the parent commit, see
# profiles/PERF_NOTES.md): from 11 concurrent requests up. At 9 the 16-lane
# bucket's padded lanes cost what the graph saves (a tie); 10 wins by less
# than run-to-run noise.
WIDE_DECODE_DEFAULT = (11, WIDE_DECODE_MAX)


def decode_bucket(n: int) -> int:
    """Graph bucket for n concurrent decode requests (n ≤ 64)."""
    return next(b for b in DECODE_BUCKETS if b >= n)


def wide_decode_range(environ=os.environ) -> tuple[int, int] | None:
    """Batch sizes that decode in wide mode, from ROOMAMD_WIDE_DECODE: unset
    or "1" is the measured default, "0" the kill switch (None: batches of
    9..64 requests go back to the prefill layer, one eager step per host
    sync), "LO-HI" an explicit range within 9..64 (the A/B lever)."""
    v = environ.get("ROOMAMD_WIDE_DECODE", "1").strip()
    if v == "0":
        return None
    if v in ("", "1"):
        return WIDE_DECODE_DEFAULT
    lo, sep, hi = v.partition("-")
    if not (sep and lo.isdigit() and hi.isdigit()
            and 9 <= int(lo) <= int(hi) <= WIDE_DECODE_MAX):
        raise ValueError("ROOMAMD_WIDE_DECODE must be 0, 1 or LO-HI with "
                         f"9 <= LO <= HI <= {WIDE_DECODE_MAX}, got {v!r}")
    return int(lo), int(hi)


def expert_dtype_from_env(environ=os.environ) -> str:
    """Expert-weight storage from ROOMAMD_EXPERT_DTYPE: unset or "bf16" is
    the default, "fp8" the block-scaled e4m3 decode mode."""
    v = environ.get("ROOMAMD_EXPERT_DTYPE", "").strip() or "bf16"
    if v not in ("bf16", "fp8"):
        raise ValueError("ROOMAMD_EXPERT_DTYPE must be bf16 or fp8, "
                         f"got {v!r}")
    return v


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


RING = ops.RING   # token-history ring entries per sampler row


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

    KMAX = 32

    def __init__(self, engine: "LocalEngine", bucket: int):
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
        self.hist = torch.zeros(self.KMAX * bucket, dtype=torch.int32, device=dev)
        self.ctr = torch.zeros(1, dtype=torch.int32, device=dev)
        self.hist_host = torch.zeros(self.KMAX * bucket, dtype=torch.int32,
                                     pin_memory=True)
        model, cache = engine.model, engine.cache
        from .. import ops as _ops
        C = _ops._require()

        def run_step():
            logits = model.forward(self.tok_in, self.seq_in, self.pos_in,
                                   cache.block_table, cache.kcaches,
                                   cache.vcaches)
            toks = torch.empty(bucket, dtype=torch.int32, device=dev)
            C.sample_rows(toks, logits, self.temperature, self.top_p,
                          self.top_k, self.seeds, self.pos_in, self.rep,
                          self.pres, self.freq, self.last_n, self.ring,
                          self.ring_len, True)
            C.hist_append(self.hist, self.ctr, toks, self.KMAX)
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
        k = min(k, self.KMAX)
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
            # push j lives at ring[j % RING]: a window of m ≤ RING tokens
            # with ring_len = m sits at ring[0:m]
            for i, w in enumerate(wins):
                if w:
                    self.h_ring[i, :len(w)] = torch.tensor(w, dtype=torch.int32)
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


PREFILL_BUCKETS = (512, 1024, 2048, 4096)   # graph-captured chunk shapes
PREFILL_MAX_ROWS = 8                         # fixed logits-row slots


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

    def __init__(self, engine: "LocalEngine", tb: int):
        import sys as _sys
        _t0 = time.time()
        print(f"[room_amd] capturing prefill graph tb={tb} ...",
              file=_sys.stderr, flush=True)
        dev = engine.device
        self.tb = tb
        self.pad_slot = engine.pad_slot
        qt = 32  # flash_prefill q-tile rows (FP_QTOK)
        # worst case: 8 request segments + 1 pad segment, each wasting <1 tile
        self.gmax = tb // qt + PREFILL_MAX_ROWS + 2
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
                                 qtile_desc=self.qtiles)

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
              f"in {time.time() - _t0:.1f}s", file=_sys.stderr, flush=True)

    def run(self, tokens: list[int], seq_ids: list[int], q_pos: list[int],
            last_rows: list[int], qtiles_host: list) -> torch.Tensor:
        n = len(tokens)
        tb = self.tb
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


class LocalEngine:
    """ChatEngine implementation running qwen3-coder-30b on this GPU."""

    def __init__(self, cfg: Qwen3MoEConfig | None = None,
                 device: str = "cuda", seed: int = 1234,
                 kv_gb: float | None = None, max_seqs: int = DEFAULT_MAX_SEQS):
        if not torch.cuda.is_available():
            raise RuntimeError("LocalEngine requires a GPU (MI355X)")
        if cfg is None:
            cfg = (Qwen3MoEConfig.tiny()
                   if os.environ.get("ROOMAMD_MODEL_CONFIG") == "tiny"
                   else Qwen3MoEConfig.qwen3_coder_30b())
        self.cfg = cfg
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            # resolve NOW, in the constructing thread: the CUDA current
            # device is per-thread, so the scheduler thread would otherwise
            # see device 0 on every rank of a one-process-per-GPU job and
            # launch kernels on rank-0's streams against rank-k's memory
            self.device = torch.device("cuda", torch.cuda.current_device())
        # expert-weight storage, read here once (docs/CONFIG.md)
        self.expert_dtype = expert_dtype_from_env()
        t0 = time.time()
        self.model = Qwen3MoEModel(cfg, self.device, seed=seed,
                                   expert_dtype=self.expert_dtype)
        self.load_seconds = time.time() - t0

        bpb = PagedKVCache.bytes_per_block(cfg.num_layers, cfg.num_kv_heads,
                                           cfg.head_dim)
        if kv_gb is None:
            free_b, _total = torch.cuda.mem_get_info(self.device)
            kv_bytes = max(int(free_b - 8e9), 2 << 30)  # leave 8 GB headroom
        else:
            kv_bytes = int(kv_gb * (1 << 30))
        max_blocks_per_seq = cfg.max_position // BLOCK_SIZE
        num_blocks = min(kv_bytes // bpb, max_seqs * max_blocks_per_seq + 1)
        self.cache = PagedKVCache(cfg.num_layers, cfg.num_kv_heads, cfg.head_dim,
                                  int(num_blocks), max_seqs, max_blocks_per_seq,
                                  self.device)
        # pad slot for hipGraph batch padding (one scrap block absorbs the
        # dummy lanes' KV writes)
        self.pad_slot = self.cache.alloc_seq()
        self.cache.ensure_capacity(self.pad_slot, 1)
        self.graphs_enabled = (os.environ.get("ROOMAMD_NO_GRAPHS") != "1")
        # hipGraph-captured prefill is OPT-IN: capture-safe on the tiny
        # config (multi-bucket, concurrent sessions, prefix reuse all pass —
        # scripts/gpu_prefill_graph_probe*.py) and cuts enqueue 0.53→0.26 s,
        # but on the 30b config the tb=512 bucket's warmup/capture hits an
        # HSAIL memory fault not yet isolated (profiles/PERF_NOTES.md round-2
        # "prefill graphs"); eager prefill is the default until it is.
        self.prefill_graphs_enabled = (
            os.environ.get("ROOMAMD_PREFILL_GRAPHS") == "1")
        self._graphs: dict[tuple, _DecodeGraph] = {}
        self._prefill_graphs: dict[int, _PrefillGraph] = {}
        self._graphs_broken = False
        self._prefill_graphs_broken = False
        # wide decode (9..64 concurrent requests): model mode and graphs,
        # one switch, read here once; a failed wide capture or replay turns
        # off only the wide graphs (the ≤ 8 graphs keep working)
        self.wide_rows = wide_decode_range()
        self.model.wide_rows = self.wide_rows
        self._wide_graphs_broken = False
        self.admitter = SessionAdmitter(self.cache, cfg.max_position)
        self._queue: "queue.Queue[GenRequest]" = queue.Queue()
        self._active: list[GenRequest] = []
        self._waiting: list[GenRequest] = []   # deferred: all slots active
        self._lock = threading.Lock()
        self._stop = False
        self.stats = {"decode_steps": 0, "decode_tokens": 0, "prefill_tokens": 0,
                      "decode_time": 0.0, "prefill_time": 0.0,
                      "prefill_prep_time": 0.0, "prefill_enq_time": 0.0,
                      "graphs_captured": 0, "decode_graph_steps": 0,
                      "decode_wide_steps": 0}
        # capture prefill-bucket graphs up front, before any agent/encoder
        # thread can put concurrent work on the device mid-capture (captures
        # are thread_local-mode too, but boot-time capture removes the window
        # entirely); decode graphs stay lazy (keyed by bucket and band)
        if (self.graphs_enabled and self.prefill_graphs_enabled
                and os.environ.get("ROOMAMD_NO_PRECAPTURE") != "1"):
            try:
                for tb in PREFILL_BUCKETS:
                    self._prefill_graphs[tb] = _PrefillGraph(self, tb)
            except Exception as e:
                import sys as _sys
                print(f"[room_amd] prefill graph pre-capture failed: {e}",
                      file=_sys.stderr)
                self._prefill_graphs.clear()
                self._prefill_graphs_broken = True
                torch.cuda.synchronize(self.device)
        self._thread = threading.Thread(target=self._scheduler_loop, daemon=True,
                                        name="room-amd-engine")
        self._thread.start()

    @property
    def sessions(self):
        return self.admitter.sessions

    # ------------------------------------------------------------ public API

    def generate(self, prompt_tokens: list[int], max_new_tokens: int = 128,
                 temperature: float = 0.7, top_p: float = 0.95, top_k: int = 40,
                 session_key: str | None = None,
                 timeout: float | None = None, seed: int | None = None,
                 repetition_penalty: float = 1.0,
                 presence_penalty: float = 0.0,
                 frequency_penalty: float = 0.0,
                 repeat_last_n: int = 64) -> GenRequest:
        validate_sampling(temperature, top_p, top_k, repetition_penalty,
                          repeat_last_n, seed, presence_penalty,
                          frequency_penalty)
        if timeout is None:
            timeout = float(os.environ.get("ROOMAMD_GEN_TIMEOUT", "600"))
        req = GenRequest(prompt_tokens=list(prompt_tokens),
                         max_new_tokens=max_new_tokens, temperature=temperature,
                         top_p=top_p, top_k=top_k, seed=seed,
                         repetition_penalty=repetition_penalty,
                         presence_penalty=presence_penalty,
                         frequency_penalty=frequency_penalty,
                         repeat_last_n=repeat_last_n, session_key=session_key)
        if os.environ.get("ROOMAMD_CYCLE_PROF") == "1":
            import sys as _sys
            print(f"[cycleprof] enqueue {session_key} {len(prompt_tokens)}tok "
                  f"(t={time.time()%100:.3f})", file=_sys.stderr)
        self._queue.put(req)
        if not req.done.wait(timeout):
            # mark cancelled: the scheduler drops it (admit or next step
            # boundary) and frees its slot — it must NOT keep decoding to
            # max_new_tokens holding KV blocks and GPU time
            req.cancelled = True
            raise TimeoutError("generation timed out")
        if req.error:
            raise RuntimeError(req.error)
        return req

    def chat(self, messages: list[dict], tools: list[ToolDef],
             options: AgentExecutionOptions) -> tuple[str, int, int]:
        """ChatEngine protocol (engine/providers.py)."""
        prompt = tok.encode_chat(messages)
        skey = f"w{options.worker_id}" if options.worker_id is not None else None
        req = self.generate(prompt, max_new_tokens=options.max_new_tokens,
                            temperature=options.temperature, top_p=options.top_p,
                            top_k=options.top_k, seed=options.seed,
                            repetition_penalty=options.repetition_penalty,
                            presence_penalty=options.presence_penalty,
                            frequency_penalty=options.frequency_penalty,
                            repeat_last_n=options.repeat_last_n,
                            session_key=skey)
        text = tok.decode(req.out_tokens)
        return text, len(prompt), len(req.out_tokens)

    def release_session(self, session_key: str) -> None:
        with self._lock:
            self.admitter.release(session_key)

    def shutdown(self) -> None:
        self._stop = True
        self._thread.join(timeout=5)

    # ------------------------------------------------------------ scheduler

    def _admit(self, req: GenRequest) -> None:
        # map token ids into this model's vocab (the synthetic tokenizer emits
        # Qwen-range ids; reduced test configs have a smaller embedding table —
        # out-of-range ids would be an out-of-bounds gather on the GPU)
        V = self.cfg.vocab_size
        req.prompt_tokens = [t % V for t in req.prompt_tokens]
        # slot/session/block bookkeeping lives in the device-free admitter
        # (admission.py) so it has CPU unit-test coverage
        self.admitter.admit(req)

    def _complete(self, req: GenRequest, ok: bool) -> None:
        """Take `req` out of the active set and resolve its future. ok=False
        (cancelled/error) drops the session so the slot/blocks free."""
        kv_tokens = (req.prompt_tokens + req.out_tokens[:-1]) if ok else None
        with self._lock:
            self.admitter.finish(req, kv_tokens)
        self._active.remove(req)
        req.done.set()

    def _scheduler_loop(self) -> None:
        torch.cuda.set_device(self.device.index)   # resolved in __init__
        while not self._stop:
            try:
                self._scheduler_iteration()
            except Exception as e:  # engine errors resolve all active futures
                import sys
                import traceback
                traceback.print_exc(file=sys.stderr)
                for r in list(self._active):
                    r.error = f"engine error: {e}"
                    self._complete(r, ok=False)

    def _try_admit(self, req: GenRequest) -> bool:
        """True = admitted; False = deferred (all slots held by ACTIVE
        requests — retry when one completes). Other failures resolve the
        future with an error (the caller blocks on req.done)."""
        from .admission import CacheFull
        try:
            with self._lock:
                self._admit(req)
            self._active.append(req)
            return True
        except CacheFull:
            self._waiting.append(req)
            return False
        except Exception as e:
            req.error = f"admit failed: {e}"
            req.done.set()
            return True  # resolved, don't retry

    def _scheduler_iteration(self) -> None:
        # re-try deferred admissions first (slots may have freed)
        waiting, self._waiting = self._waiting, []
        for req in waiting:
            if req.cancelled:
                req.done.set()
                continue
            self._try_admit(req)
        # admit new requests
        block = not (self._active or self._waiting)
        try:
            while True:
                req = self._queue.get(timeout=0.05 if block else 0)
                block = False
                if req.cancelled:  # caller gave up before admission
                    req.done.set()
                    continue
                self._try_admit(req)
        except queue.Empty:
            pass
        # drop requests whose caller timed out (a timed-out
        # request must not keep decoding and holding a KV slot)
        for r in [r for r in self._active if r.cancelled]:
            r.error = "cancelled"
            self._complete(r, ok=False)
        if not self._active:
            return

        # phase 1: prefill pending prompts (batched across requests, chunked)
        pre = [r for r in self._active if r.pending_prefill]
        if pre:
            self._prefill_step(pre)
            return  # re-check queue between chunks

        # phase 2: one decode step for all active sequences
        self._decode_step([r for r in self._active if not r.pending_prefill])

    def _prefill_step(self, reqs: list[GenRequest]) -> None:
        t0 = time.time()
        host_t0 = t0
        budget = PREFILL_CHUNK
        tokens, seq_ids, q_pos, last_rows, sampled_reqs = [], [], [], [], []
        segments = []  # (row0, count) per request — host-side q-tile info
        for r in reqs:
            if budget <= 0:
                break
            take = min(budget, len(r.pending_prefill))
            chunk = r.pending_prefill[:take]
            r.pending_prefill = r.pending_prefill[take:]
            self.cache.ensure_capacity(r.slot, r.pos + take)
            segments.append((len(tokens), take))
            tokens.extend(chunk)
            seq_ids.extend([r.slot] * take)
            q_pos.extend(range(r.pos, r.pos + take))
            r.pos += take
            budget -= take
            if not r.pending_prefill:  # prompt complete → sample first token
                last_rows.append(len(tokens) - 1)
                sampled_reqs.append(r)
        dev = self.device
        n = len(tokens)
        graph_ok = (self.graphs_enabled and self.prefill_graphs_enabled
                    and not self._graphs_broken
                    and not self._prefill_graphs_broken
                    and n > 8 and len(sampled_reqs) <= PREFILL_MAX_ROWS)
        if graph_ok:
            # graph path: pad the chunk to a fixed bucket shape and replay
            # the captured forward (the eager forward is python-launch-bound
            # at ~30 ms/chunk — more than the GPU work it enqueues)
            tb = next(b for b in PREFILL_BUCKETS if b >= n)
            # pad rows live in their own 1-token-context segment — in a COPY:
            # the eager fallback below reuses `segments` against n-row tensors,
            # so a leaked pad segment would read q rows past the tensor end
            seg_graph = segments + ([(n, tb - n)] if n < tb else [])
            qtiles_host = self._qtile_list(seg_graph)
            self.stats["prefill_prep_time"] += time.time() - host_t0
            try:
                g = self._prefill_graphs.get(tb)
                if g is None:
                    g = _PrefillGraph(self, tb)
                    self._prefill_graphs[tb] = g
                logits = g.run(tokens, seq_ids, q_pos, last_rows, qtiles_host)
                self.stats["prefill_enq_time"] += time.time() - host_t0
                self.stats["prefill_tokens"] += n
                if sampled_reqs:
                    self._sample_and_append(sampled_reqs,
                                            logits[:len(sampled_reqs)])
                self.stats["prefill_time"] += time.time() - t0
                return
            except Exception as e:
                import sys
                print(f"[room_amd] hipGraph prefill disabled: {e}",
                      file=sys.stderr)
                self._prefill_graphs_broken = True
                # a capture that aborted mid-graph can leave stale stream
                # state; fence the device before falling back to eager
                try:
                    torch.cuda.synchronize(dev)
                except Exception:
                    pass
        tokens_t = torch.tensor(tokens, dtype=torch.int64, device=dev)
        seq_t = torch.tensor(seq_ids, dtype=torch.int32, device=dev)
        pos_t = torch.tensor(q_pos, dtype=torch.int32, device=dev)
        rows_t = torch.tensor(last_rows, dtype=torch.int64, device=dev)
        qtiles = (ops.build_qtile_desc(segments, dev)
                  if len(tokens) > 8 else None)
        self.stats["prefill_prep_time"] += time.time() - host_t0
        logits = self.model.forward(tokens_t, seq_t, pos_t, self.cache.block_table,
                                    self.cache.kcaches, self.cache.vcaches,
                                    logits_rows=rows_t, qtile_desc=qtiles)
        self.stats["prefill_enq_time"] += time.time() - host_t0
        self.stats["prefill_tokens"] += len(tokens)
        if sampled_reqs:
            self._sample_and_append(sampled_reqs, logits)
        self.stats["prefill_time"] += time.time() - t0

    @staticmethod
    def _qtile_list(segments: list) -> list:
        """(row0, count) segments → ≤32-row q-tile descriptors (host list)."""
        out = []
        for row0, count in segments:
            r = row0
            while r < row0 + count:
                take = min(32, row0 + count - r)
                out.append((r, take))
                r += take
        return out

    def _decode_step(self, reqs: list[GenRequest]) -> None:
        if not reqs:
            return
        t0 = time.time()
        dev = self.device
        tokens = [r.last_token for r in reqs]
        slots = [r.slot for r in reqs]
        positions = [r.pos for r in reqs]

        # multi-step graph block: K bounded by the smallest remaining budget so
        # every request stops exactly at max_new (admission latency is K steps)
        steps = 1
        # 9..64 requests: the model's wide mode, graph or eager alike
        wide = (self.wide_rows is not None
                and self.wide_rows[0] <= len(reqs) <= self.wide_rows[1])
        graph_ok = (self.graphs_enabled and not self._graphs_broken
                    and (len(reqs) <= 8
                         or (wide and not self._wide_graphs_broken)))
        if graph_ok:
            steps = max(1, min(min(r.max_new_tokens - len(r.out_tokens)
                                   for r in reqs), _DecodeGraph.KMAX))
            for r in reqs:
                self.cache.ensure_capacity(r.slot, r.pos + steps)
            bucket = decode_bucket(len(reqs))
            # context band: 64 attention splits once any sequence's KV span
            # passes 8k (shorter per-WG serial chunk chains); banded graphs
            # keep each capture's grid fixed
            band = 64 if max(positions) + steps >= 16384 else 32
            self.model.attn_splits = band
            key = (bucket, band)
            try:
                g = self._graphs.get(key)
                if g is None:
                    g = _DecodeGraph(self, bucket)
                    self._graphs[key] = g
                    self.stats["graphs_captured"] = len(self._graphs)
                hist = g.run_block(reqs, steps)
                finished = []
                for si in range(steps):
                    row = hist[si * g.bucket: si * g.bucket + len(reqs)]
                    for r, t in zip(reqs, row):
                        if r in finished:
                            continue
                        r.last_token = int(t)
                        r.out_tokens.append(int(t))
                        r.pos += 1
                        if (len(r.out_tokens) >= r.max_new_tokens
                                or t in (tok.EOS, tok.IM_END)):
                            finished.append(r)
                for r in finished:
                    self._complete(r, ok=True)
                self.stats["decode_steps"] += steps
                self.stats["decode_graph_steps"] += steps
                if wide:
                    self.stats["decode_wide_steps"] += steps
                self.stats["decode_tokens"] += steps * len(reqs)
                self.stats["decode_time"] += time.time() - t0
                return
            except Exception as e:
                import sys
                if wide:
                    print(f"[room_amd] hipGraph wide decode disabled: {e}",
                          file=sys.stderr)
                    self._wide_graphs_broken = True
                    # as for prefill: fence the device after an aborted capture
                    try:
                        torch.cuda.synchronize(dev)
                    except Exception:
                        pass
                else:
                    print(f"[room_amd] hipGraph decode disabled: {e}",
                          file=sys.stderr)
                    self._graphs_broken = True

        # eager fallback: one step
        self.model.attn_splits = 64 if max(positions) >= 16384 else 32
        for r in reqs:
            self.cache.ensure_capacity(r.slot, r.pos + 1)
        for r in reqs:
            r.pos += 1
        tokens_t = torch.tensor(tokens, dtype=torch.int64, device=dev)
        seq_t = torch.tensor(slots, dtype=torch.int32, device=dev)
        pos_t = torch.tensor(positions, dtype=torch.int32, device=dev)
        logits = self.model.forward(tokens_t, seq_t, pos_t,
                                    self.cache.block_table,
                                    self.cache.kcaches, self.cache.vcaches)
        self._sample_and_append(reqs, logits, positions)
        self.stats["decode_steps"] += 1
        if wide:
            self.stats["decode_wide_steps"] += 1
        self.stats["decode_tokens"] += len(reqs)
        self.stats["decode_time"] += time.time() - t0

    def _sample_and_append(self, reqs: list[GenRequest], logits: torch.Tensor,
                           ctrs: list[int] | None = None) -> None:
        """One sample_rows call with per-row parameters, one host sync. The
        draw counter is the position of the token that produced the logits
        row (default: the last prefilled one), as in the decode graphs."""
        dev = self.device
        n = len(reqs)
        if ctrs is None:
            ctrs = [r.pos - 1 for r in reqs]
        i32, f32, seeds, wins = _sampling_rows(reqs)
        ring = torch.zeros(n, RING, dtype=torch.int32)
        for i, w in enumerate(wins):
            if w:
                ring[i, :len(w)] = torch.tensor(w, dtype=torch.int32)
        ti = torch.tensor(i32 + [ctrs], dtype=torch.int32, device=dev)
        tf = torch.tensor(f32, dtype=torch.float32, device=dev)
        toks = ops.sample_rows(
            logits, tf[0], tf[1], ti[0],
            torch.tensor(seeds, dtype=torch.int64, device=dev), ti[3],
            tf[2], tf[3], tf[4], ti[1], ring.to(dev), ti[2], append=False)
        self._finish_host_tokens(reqs, [int(t) for t in toks.tolist()])

    def _finish_host_tokens(self, reqs: list[GenRequest],
                            toks_host: list[int]) -> None:
        finished = []
        for r, t in zip(reqs, toks_host):
            r.last_token = int(t)
            r.out_tokens.append(int(t))
            if (len(r.out_tokens) >= r.max_new_tokens
                    or t in (tok.EOS, tok.IM_END)):
                finished.append(r)
        for r in finished:
            # the sampled token at r.pos is NOT yet in KV; it will be written
            # if the session continues (prompt extension re-runs it)
            self._complete(r, ok=True)


# ------------------------------------------------------------ singleton

_engine: LocalEngine | None = None
_engine_lock = threading.Lock()


def get_local_engine(model: str = "qwen3-coder-30b") -> LocalEngine:
    global _engine
    with _engine_lock:
        if _engine is None:
            _engine = LocalEngine()
        return _engine


def set_local_engine(engine: LocalEngine) -> None:
    global _engine
    _engine = engine
