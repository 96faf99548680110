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

import os
import queue
import sys
import threading
import time
import traceback

import torch

from .. import ops
from ..models.qwen3_moe import Qwen3MoEConfig, Qwen3MoEModel
from . import tokenizer as tok
from .admission import CacheFull, SessionAdmitter
from .graphs import _DecodeGraph, _PrefillGraph
from .kv_cache import BLOCK_SIZE, PagedKVCache
from .request import (RING, GenRequest, _sampling_rows,  # noqa: F401
                      validate_sampling)
from .step_plan import (DECODE_BUCKETS, PREFILL_BUCKETS,  # noqa: F401
                        PREFILL_CHUNK, PREFILL_MAX_ROWS, accept_tokens,
                        decode_bucket, pack_ring, plan_decode, plan_prefill,
                        prefill_graph_shape, qtile_list)
from .types import AgentExecutionOptions, ToolDef

DEFAULT_MAX_SEQS = 64
WIDE_DECODE_MAX = DECODE_BUCKETS[-1]
# Wide decode runs where it measured faster than the prefill layer it replaces
# (30b, scripts/gpu_wide_decode_micro.py against the parent commit, see
# profiles/PERF_NOTES.md): from 11 concurrent requests up. At 9 the 16-lane
# bucket's padded lanes cost what the graph saves (a tie); 10 wins by less
# than run-to-run noise.
WIDE_DECODE_DEFAULT = (11, WIDE_DECODE_MAX)


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


def kv_dtype_from_env(environ=os.environ) -> str:
    """KV-cache storage from ROOMAMD_KV_DTYPE: unset, empty or "bf16" is the
    default, "fp8" the e4m3 rows with one f32 scale per row."""
    v = environ.get("ROOMAMD_KV_DTYPE", "").strip() or "bf16"
    if v not in ("bf16", "fp8"):
        raise ValueError(f"ROOMAMD_KV_DTYPE must be bf16 or fp8, got {v!r}")
    return v


def expert_image_from_env(environ=os.environ) -> bool:
    """Whether an fp8 engine keeps the bf16 image of its expert weights, from
    ROOMAMD_EXPERT_IMAGE: unset, empty or "1" keeps it (prefill reads the
    image), "0" drops it (prefill reads the e4m3 weights; fp8 only)."""
    v = environ.get("ROOMAMD_EXPERT_IMAGE", "").strip()
    if v in ("", "1"):
        return True
    if v == "0":
        return False
    raise ValueError(f"ROOMAMD_EXPERT_IMAGE must be 0 or 1, got {v!r}")


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
        self.expert_image = expert_image_from_env()
        self.kv_dtype = kv_dtype_from_env()
        if not self.expert_image and self.expert_dtype != "fp8":
            raise ValueError(
                "ROOMAMD_EXPERT_IMAGE=0 needs ROOMAMD_EXPERT_DTYPE=fp8: with "
                f"{self.expert_dtype} expert weights the bf16 tensors are the "
                "only copy, there is no image to drop")
        t0 = time.time()
        self.model = Qwen3MoEModel(cfg, self.device, seed=seed,
                                   expert_dtype=self.expert_dtype,
                                   expert_image=self.expert_image)
        self.load_seconds = time.time() - t0

        bpb = PagedKVCache.bytes_per_block(cfg.num_layers, cfg.num_kv_heads,
                                           cfg.head_dim, self.kv_dtype)
        if kv_gb is None:
            free_b, _total = torch.cuda.mem_get_info(self.device)
            kv_bytes = max(int(free_b - 8e9), 2 << 30)  # leave 8 GB headroom
        else:
            kv_bytes = int(kv_gb * (1 << 30))
        max_blocks_per_seq = cfg.max_position // BLOCK_SIZE
        num_blocks = min(kv_bytes // bpb, max_seqs * max_blocks_per_seq + 1)
        self.cache = PagedKVCache(cfg.num_layers, cfg.num_kv_heads, cfg.head_dim,
                                  int(num_blocks), max_seqs, max_blocks_per_seq,
                                  self.device, kv_dtype=self.kv_dtype)
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
                self._prefill_graphs.clear()
                self._graph_failed("_prefill_graphs_broken",
                                   "prefill graph pre-capture failed", e)
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
            print(f"[cycleprof] enqueue {session_key} {len(prompt_tokens)}tok "
                  f"(t={time.time()%100:.3f})", file=sys.stderr)
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
                traceback.print_exc(file=sys.stderr)
                for r in list(self._active):
                    r.error = f"engine error: {e}"
                    self._complete(r, ok=False)

    def _try_admit(self, req: GenRequest) -> bool:
        """True = admitted; False = deferred (all slots held by ACTIVE
        requests — retry when one completes). Other failures resolve the
        future with an error (the caller blocks on req.done)."""
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

    def _graph_failed(self, flag: str, what: str, e: Exception,
                      fence: bool = True) -> None:
        """Turn one family of graphs off for good (`flag`) and say why. A
        capture that aborted mid-graph can leave stale stream state, so the
        device is fenced before the eager fallback runs."""
        print(f"[room_amd] {what}: {e}", file=sys.stderr)
        setattr(self, flag, True)
        if fence:
            try:
                torch.cuda.synchronize(self.device)
            except Exception:
                pass

    def _accept(self, reqs: list[GenRequest], rows: list,
                advance_pos: bool) -> None:
        for r in accept_tokens(reqs, rows, advance_pos):
            self._complete(r, ok=True)

    def _prefill_step(self, reqs: list[GenRequest]) -> None:
        t0 = time.time()
        plan = plan_prefill(reqs)
        for slot, need in plan.capacity:
            self.cache.ensure_capacity(slot, need)
        dev, n, sampled = self.device, len(plan.tokens), plan.sampled_reqs
        logits = None
        if (self.graphs_enabled and self.prefill_graphs_enabled
                and not self._graphs_broken
                and not self._prefill_graphs_broken
                and n > 8 and len(sampled) <= PREFILL_MAX_ROWS):
            # graph path: pad the chunk to a fixed bucket shape and replay
            # the captured forward (the eager forward is python-launch-bound
            # at ~30 ms/chunk — more than the GPU work it enqueues)
            tb, seg_graph = prefill_graph_shape(n, plan.segments)
            qtiles_host = qtile_list(seg_graph, ops.flash_prefill_qtile())
            self.stats["prefill_prep_time"] += time.time() - t0
            try:
                g = self._prefill_graphs.get(tb)
                if g is None:
                    g = self._prefill_graphs[tb] = _PrefillGraph(self, tb)
                logits = g.run(plan.tokens, plan.seq_ids, plan.q_pos,
                               plan.last_rows, qtiles_host)[:len(sampled)]
            except Exception as e:
                self._graph_failed("_prefill_graphs_broken",
                                   "hipGraph prefill disabled", e)
        if logits is None:
            tokens_t = torch.tensor(plan.tokens, dtype=torch.int64, device=dev)
            seq_t = torch.tensor(plan.seq_ids, dtype=torch.int32, device=dev)
            pos_t = torch.tensor(plan.q_pos, dtype=torch.int32, device=dev)
            rows_t = torch.tensor(plan.last_rows, dtype=torch.int64, device=dev)
            qtiles = (ops.build_qtile_desc(plan.segments, dev)
                      if n > 8 else None)
            self.stats["prefill_prep_time"] += time.time() - t0
            logits = self.model.forward(
                tokens_t, seq_t, pos_t, self.cache.block_table,
                self.cache.kcaches, self.cache.vcaches, logits_rows=rows_t,
                qtile_desc=qtiles, kscales=self.cache.kscales,
                vscales=self.cache.vscales)
        self.stats["prefill_enq_time"] += time.time() - t0
        self.stats["prefill_tokens"] += n
        if sampled:
            self._accept(sampled, [self._sample(sampled, logits)], False)
        self.stats["prefill_time"] += time.time() - t0

    def _plan_decode(self, reqs: list[GenRequest], positions: list[int]):
        plan = plan_decode(
            len(reqs), positions,
            [r.max_new_tokens - len(r.out_tokens) for r in reqs],
            self.wide_rows, self.graphs_enabled, self._graphs_broken,
            self._wide_graphs_broken)
        for r in reqs:
            self.cache.ensure_capacity(r.slot, r.pos + plan.steps)
        self.model.attn_splits = plan.band
        return plan

    def _decode_step(self, reqs: list[GenRequest]) -> None:
        if not reqs:
            return
        t0 = time.time()
        dev, n = self.device, len(reqs)
        positions = [r.pos for r in reqs]
        plan = self._plan_decode(reqs, positions)
        rows = None
        if plan.use_graph:
            key = (plan.bucket, plan.band)
            try:
                g = self._graphs.get(key)
                if g is None:
                    g = self._graphs[key] = _DecodeGraph(self, plan.bucket)
                    self.stats["graphs_captured"] = len(self._graphs)
                hist = g.run_block(reqs, plan.steps)
                rows = [hist[s * g.bucket: s * g.bucket + n]
                        for s in range(plan.steps)]
            except Exception as e:
                # a wide failure turns off only the wide graphs, and fences
                flag, what = (("_wide_graphs_broken", "wide decode")
                              if plan.wide else ("_graphs_broken", "decode"))
                self._graph_failed(flag, f"hipGraph {what} disabled", e,
                                   fence=plan.wide)
                plan = self._plan_decode(reqs, positions)   # eager now
        if rows is None:
            # eager fallback: one step
            tokens_t = torch.tensor([r.last_token for r in reqs],
                                    dtype=torch.int64, device=dev)
            seq_t = torch.tensor([r.slot for r in reqs], dtype=torch.int32,
                                 device=dev)
            pos_t = torch.tensor(positions, dtype=torch.int32, device=dev)
            for r in reqs:
                r.pos += 1
            logits = self.model.forward(tokens_t, seq_t, pos_t,
                                        self.cache.block_table,
                                        self.cache.kcaches, self.cache.vcaches,
                                        kscales=self.cache.kscales,
                                        vscales=self.cache.vscales)
            rows = [self._sample(reqs, logits, positions)]
        self._accept(reqs, rows, advance_pos=plan.use_graph)
        self.stats["decode_steps"] += plan.steps
        if plan.use_graph:
            self.stats["decode_graph_steps"] += plan.steps
        if plan.wide:
            self.stats["decode_wide_steps"] += plan.steps
        self.stats["decode_tokens"] += plan.steps * n
        self.stats["decode_time"] += time.time() - t0

    def _sample(self, reqs: list[GenRequest], logits: torch.Tensor,
                ctrs: list[int] | None = None) -> list[int]:
        """One sample_rows call with per-row parameters, one host sync. The
        draw counter is the position of the token that produced the logits
        row (default: the last prefilled one), as in the decode graphs."""
        dev = self.device
        if ctrs is None:
            ctrs = [r.pos - 1 for r in reqs]
        i32, f32, seeds, wins = _sampling_rows(reqs)
        ring = torch.zeros(len(reqs), RING, dtype=torch.int32)
        pack_ring(wins, ring)
        ti = torch.tensor(i32 + [ctrs], dtype=torch.int32, device=dev)
        tf = torch.tensor(f32, dtype=torch.float32, device=dev)
        return ops.sample_rows(
            logits, tf[0], tf[1], ti[0],
            torch.tensor(seeds, dtype=torch.int64, device=dev), ti[3],
            tf[2], tf[3], tf[4], ti[1], ring.to(dev), ti[2],
            append=False).tolist()


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
