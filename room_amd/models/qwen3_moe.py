"""Qwen3-MoE (qwen3-coder-30b = Qwen3-30B-A3B shape) — MI355X-native forward.

The reference pinned `qwen3-coder:30b` served by an external Ollama sidecar
(src/shared/local-model.ts:3-5); here the model runs in-process: weights are
bf16 tensors resident in HBM3E, and the hot ops are the CDNA4 HIP kernels in
room_amd/ops (RMSNorm, fused QK-norm+RoPE+KV-scatter, split-KV paged
attention, MFMA flash prefill, H-split router + top-k, MoE pair GEMV /
grouped MFMA GEMM, BN-specialized dense GEMV, two-stage sampling). At decode
every projection (QKV/O/router/lm_head) runs on the hand-written GEMVs; wide
decode (9-64 rows) runs them and the MoE on the skinny MFMA GEMM;
prefill's large GEMMs go through hipBLASLt via torch.nn.functional.linear.
With expert_dtype="fp8" (opt-in) the expert weights are also held as
block-scaled e4m3 and both decode paths read those (ops/csrc/moe_fp8.hip);
with expert_image=False on top they are held ONLY as e4m3 and prefill's
grouped GEMM reads them too.

Inference-only (no autograd); a training path is out of scope for the
reference's semantics (it never trains).
"""
from __future__ import annotations

from dataclasses import dataclass

import torch
import torch.nn.functional as F

from .. import ops
from ..ops.reference import (dequantize_fp8_block, quantize_fp8_block,
                             rope_tables)

EXPERT_DTYPES = ("bf16", "fp8")


@dataclass
class Qwen3MoEConfig:
    vocab_size: int = 151936
    hidden_size: int = 2048
    num_layers: int = 48
    num_q_heads: int = 32
    num_kv_heads: int = 4
    head_dim: int = 128
    num_experts: int = 128
    num_experts_per_tok: int = 8
    moe_intermediate_size: int = 768
    rms_eps: float = 1e-6
    rope_theta: float = 10_000_000.0
    max_position: int = 16384
    # GEMV→grouped-GEMM switchover: below this many tokens the decode GEMV
    # path wins (per-pair weight streaming); above it, grouped MFMA GEMM.
    moe_grouped_threshold: int = 16

    @staticmethod
    def qwen3_coder_30b() -> "Qwen3MoEConfig":
        return Qwen3MoEConfig()

    @staticmethod
    def tiny(vocab: int = 4096) -> "Qwen3MoEConfig":
        """Small config for smoke tests / CPU-free validation on one GPU call."""
        return Qwen3MoEConfig(vocab_size=vocab, hidden_size=512, num_layers=4,
                              num_q_heads=8, num_kv_heads=1, head_dim=128,
                              num_experts=16, num_experts_per_tok=4,
                              moe_intermediate_size=256, max_position=4096)


WIDE_MAX_ROWS = ops.SKINNY_MAX_ROWS   # tallest wide-decode batch


def forward_mode(T: int, has_qtiles: bool,
                 wide_rows: tuple[int, int] | None = (9, WIDE_MAX_ROWS)) -> str:
    """Which layer a forward of T rows runs: "decode" (T ≤ 8, GEMV kernels),
    "wide" (9..64 rows without q-tile descriptors: a decode batch — prefill
    chunks of that size always carry descriptors) or "prefill". wide_rows
    narrows the wide range to lo ≤ T ≤ hi (the engine passes the range where
    wide mode measured faster); None sends every such batch to the prefill
    layer."""
    if T <= 8:
        return "decode"
    if (wide_rows is not None and not has_qtiles
            and max(9, wide_rows[0]) <= T <= min(WIDE_MAX_ROWS, wide_rows[1])):
        return "wide"
    return "prefill"


@dataclass
class _Step:
    """Per-forward inputs and buffers shared by every layer of one forward()
    call (nothing here outlives the call)."""
    seq_ids: torch.Tensor
    q_pos: torch.Tensor
    block_table: torch.Tensor
    qtile_desc: torch.Tensor | None
    hbuf: torch.Tensor                      # normed activations [T, H]
    pair_token: torch.Tensor | None = None  # MoE pair -> token row [T*K]
    pair_row: torch.Tensor | None = None    # identity pair map [T*K]
    # decode (T ≤ 8) buffers; empty_delta is decode-only
    qkv: torch.Tensor | None = None
    empty_delta: torch.Tensor | None = None
    part: torch.Tensor | None = None
    part_ml: torch.Tensor | None = None
    # wide-decode-only (9 ≤ T ≤ 64) buffers, on top of qkv/part/part_ml
    obuf: torch.Tensor | None = None        # O projection output [T, H]
    attn: torch.Tensor | None = None
    router_logits: torch.Tensor | None = None
    gateup: torch.Tensor | None = None      # [T*K, 2I]
    hmid: torch.Tensor | None = None        # [T*K, I]
    z: torch.Tensor | None = None           # [T*K, H]
    moe_out: torch.Tensor | None = None     # [T, H]


def _check_expert_args(expert_dtype: str, expert_image: bool) -> None:
    if expert_dtype not in EXPERT_DTYPES:
        raise ValueError(f"expert_dtype must be one of {EXPERT_DTYPES}, "
                         f"got {expert_dtype!r}")
    if not expert_image and expert_dtype != "fp8":
        raise ValueError('expert_image=False needs expert_dtype="fp8": with '
                         f"{expert_dtype} experts the bf16 tensors are the "
                         "only copy of the weights")


class Qwen3MoELayer:
    def __init__(self, cfg: Qwen3MoEConfig, device: torch.device,
                 gen: torch.Generator, expert_dtype: str = "bf16",
                 expert_image: bool = True):
        _check_expert_args(expert_dtype, expert_image)
        h, d = cfg.hidden_size, cfg.head_dim
        qdim = cfg.num_q_heads * d
        kvdim = cfg.num_kv_heads * d
        std = 0.02

        def rnd(*shape):
            return torch.empty(*shape, dtype=torch.bfloat16, device=device).normal_(
                0, std, generator=gen)

        self.input_norm_w = torch.ones(h, dtype=torch.bfloat16, device=device)
        self.post_attn_norm_w = torch.ones(h, dtype=torch.bfloat16, device=device)
        self.q_norm_w = torch.ones(d, dtype=torch.bfloat16, device=device)
        self.k_norm_w = torch.ones(d, dtype=torch.bfloat16, device=device)
        self.wqkv = rnd(qdim + 2 * kvdim, h)      # fused QKV projection
        self.wo = rnd(h, qdim)
        self.router_w = rnd(cfg.num_experts, h)
        if not expert_image:
            # fp8 only: each bf16 tensor is quantised and released before the
            # next is drawn (same generator order as the image build), and
            # the layer gets no w13 / w2 attribute at all, so no bf16 path
            # can run on it by accident
            w = rnd(cfg.num_experts, 2 * cfg.moe_intermediate_size, h)
            self.w13_q, self.w13_s = quantize_fp8_block(w)
            del w
            w = rnd(cfg.num_experts, h, cfg.moe_intermediate_size)
            self.w2_q, self.w2_s = quantize_fp8_block(w)
            del w
            return
        self.w13 = rnd(cfg.num_experts, 2 * cfg.moe_intermediate_size, h)
        self.w2 = rnd(cfg.num_experts, h, cfg.moe_intermediate_size)
        if expert_dtype == "fp8":
            # block-scaled e4m3 for the decode kernels; w13/w2 become the
            # bf16 image, which holds exactly the fp8 weights' values (the
            # quantiser's scales are powers of two), for the prefill GEMM
            self.w13_q, self.w13_s = quantize_fp8_block(self.w13)
            self.w13 = dequantize_fp8_block(self.w13_q, self.w13_s).to(
                torch.bfloat16)
            self.w2_q, self.w2_s = quantize_fp8_block(self.w2)
            self.w2 = dequantize_fp8_block(self.w2_q, self.w2_s).to(
                torch.bfloat16)


class Qwen3MoEModel:
    """Flat-tensor model (no nn.Module overhead on the decode path)."""

    def __init__(self, cfg: Qwen3MoEConfig, device: str | torch.device = "cuda",
                 seed: int = 1234, expert_dtype: str = "bf16",
                 expert_image: bool = True):
        _check_expert_args(expert_dtype, expert_image)
        self.cfg = cfg
        # "fp8": expert weights also held as e4m3 with a scale per 128x128
        # block, read by the decode paths (narrow GEMVs, wide skinny GEMM);
        # prefill reads their exact bf16 image
        self.expert_dtype = expert_dtype
        # False (fp8 only): no bf16 image; prefill's grouped GEMM reads the
        # e4m3 weights (moe_grouped_gemm128_fp8) with the image path's bits
        self.expert_image = bool(expert_image)
        self.device = torch.device(device)
        gen = torch.Generator(device=self.device)
        gen.manual_seed(seed)
        h = cfg.hidden_size
        self.embed = torch.empty(cfg.vocab_size, h, dtype=torch.bfloat16,
                                 device=self.device).normal_(0, 0.02, generator=gen)
        # one layer at a time: the quantiser's f32 transients stay per-layer
        self.layers = [Qwen3MoELayer(cfg, self.device, gen, expert_dtype,
                                     self.expert_image)
                       for _ in range(cfg.num_layers)]
        self.final_norm_w = torch.ones(h, dtype=torch.bfloat16, device=self.device)
        self.lm_head = torch.empty(cfg.vocab_size, h, dtype=torch.bfloat16,
                                   device=self.device).normal_(0, 0.02, generator=gen)
        # decode split-KV band (32 short / 64 long contexts); the engine sets
        # this per decode step (and per captured graph band)
        self.attn_splits = 32
        # capture-safe GEMMs: hipBLASLt aborts hipGraph capture, so captured
        # prefill forwards route dense projections through the grouped MFMA
        # kernel (single-expert). The engine flips this around capture.
        self.capture_gemm = False
        self._dense_desc: dict = {}   # T -> (desc, pair_token) for E=1 GEMMs
        self._dense_wpad: dict = {}   # id(w) -> N-padded weight (N % 64 != 0)
        # wide decode: batch sizes that run _wide_layer. The engine narrows
        # this to its measured range, or clears it (None) for its kill
        # switch, which restores the prefill layer for those batches
        self.wide_rows: tuple[int, int] | None = (9, WIDE_MAX_ROWS)
        self._wide_rpad: dict = {}    # id(router_w) -> 16-row-padded weight
        cos_t, sin_t = rope_tables(cfg.max_position, cfg.head_dim, cfg.rope_theta)
        self.cos_t = cos_t.to(self.device)
        self.sin_t = sin_t.to(self.device)
        self.scale = cfg.head_dim ** -0.5

    def num_params(self) -> int:
        cfg = self.cfg
        l0 = self.layers[0]
        w13, w2 = ((l0.w13, l0.w2) if self.expert_image
                   else (l0.w13_q, l0.w2_q))
        per_layer = (l0.wqkv.numel() + l0.wo.numel() + l0.router_w.numel()
                     + w13.numel() + w2.numel())
        return self.embed.numel() + self.lm_head.numel() + cfg.num_layers * per_layer

    def _dense(self, x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
        """Dense projection: hipBLASLt eager; grouped MFMA when capturing."""
        if not self.capture_gemm:
            return F.linear(x, w)
        T = x.size(0)
        dp = self._dense_desc.get(T)
        if dp is None:
            pe = torch.zeros(T, dtype=torch.int32, device=x.device)
            desc = ops.moe_build_desc_device(pe, 1)
            pt = torch.arange(T, dtype=torch.int32, device=x.device)
            dp = self._dense_desc[T] = (desc, pt)
        N = w.size(0)
        if N % 64:  # e.g. tiny-config router (16 experts): pad N, slice out
            wp = self._dense_wpad.get(id(w))
            if wp is None:
                wp = torch.zeros((N + 63) // 64 * 64, w.size(1),
                                 dtype=w.dtype, device=w.device)
                wp[:N] = w
                self._dense_wpad[id(w)] = wp
            w = wp
        y = torch.empty(T, w.size(0), dtype=torch.bfloat16, device=x.device)
        ops.dense_grouped_gemm(y, x, w, dp[0], dp[1])
        return y[:, :N] if N != w.size(0) else y

    @torch.inference_mode()
    def forward(self, tokens: torch.Tensor, seq_ids: torch.Tensor,
                q_pos: torch.Tensor, block_table: torch.Tensor,
                kcaches: list[torch.Tensor], vcaches: list[torch.Tensor],
                logits_rows: torch.Tensor | None = None,
                qtile_desc: torch.Tensor | None = None,
                kscales: list[torch.Tensor] | None = None,
                vscales: list[torch.Tensor] | None = None) -> torch.Tensor:
        """tokens/seq_ids/q_pos: [T] on device. kcaches/vcaches: one pair per
        layer. logits_rows: row indices to compute logits for (default: all).
        kscales/vscales: the per-row scales of an fp8 KV cache, one pair per
        layer (PagedKVCache(kv_dtype="fp8")); None with bf16 caches.
        Returns fp32 logits [R, vocab]."""
        cfg = self.cfg
        T = tokens.numel()
        dev = self.device
        # decode-mode (T ≤ 8): dense projections use the hand-written GEMV
        # (hipBLASLt ~1.1 TB/s on M≤8 skinny shapes) and attention uses the
        # split-KV flash-decode kernels so the tiny grid still fills the chip.
        # wide mode (9..64 rows, no q-tiles): the same attention, every GEMM
        # on the skinny MFMA kernel (_wide_layer).
        mode = forward_mode(T, qtile_desc is not None, self.wide_rows)
        decode = mode == "decode"
        wide = mode == "wide"
        qdim = cfg.num_q_heads * cfg.head_dim
        kvdim = cfg.num_kv_heads * cfg.head_dim
        x = self.embed[tokens.long()]              # [T, H] bf16 (residual stream)
        # per-forward state shared by every layer
        st = _Step(seq_ids=seq_ids, q_pos=q_pos, block_table=block_table,
                   qtile_desc=qtile_desc,
                   hbuf=torch.empty_like(x))       # normed activations
        if (kscales is None) != (vscales is None):
            raise ValueError("kscales and vscales go together")
        moe_out = None                             # pending delta for fused add
        # layer-invariant MoE pair/token indices (was re-built 48×/step: an
        # arange+repeat_interleave kernel pair per layer in the decode graph)
        K = cfg.num_experts_per_tok
        st.pair_token = torch.arange(
            T, device=dev, dtype=torch.int32).repeat_interleave(K)
        st.pair_row = torch.arange(T * K, device=dev, dtype=torch.int32)
        if decode or wide:
            st.qkv = torch.empty(T, qdim + 2 * kvdim, dtype=torch.bfloat16,
                                 device=dev)
            if decode:
                x_alt = torch.empty_like(x)  # residual ping-pong for fused norms
                st.empty_delta = torch.empty(0, dtype=torch.float32,
                                             device=dev)
            nsp = ops.attn_nsplits()
            st.part = torch.empty(T, cfg.num_q_heads, nsp, cfg.head_dim,
                                  dtype=torch.float32, device=dev)
            st.part_ml = torch.empty(T, cfg.num_q_heads, nsp, 2,
                                     dtype=torch.float32, device=dev)
        if wide:
            bf = dict(dtype=torch.bfloat16, device=dev)
            st.obuf = torch.empty(T, cfg.hidden_size, **bf)
            I, P = cfg.moe_intermediate_size, T * K
            st.attn = torch.empty(T, cfg.num_q_heads, cfg.head_dim, **bf)
            st.router_logits = torch.empty(
                T, (cfg.num_experts + 15) // 16 * 16, dtype=torch.float32,
                device=dev)
            st.gateup = torch.empty(P, 2 * I, **bf)
            st.hmid = torch.empty(P, I, **bf)
            st.z = torch.empty(P, cfg.hidden_size, **bf)
            st.moe_out = torch.empty(T, cfg.hidden_size, **bf)

        for li, layer in enumerate(self.layers):
            # fp8 KV cache: the layer's row scales ride along with its caches
            # (no extra argument in bf16 mode)
            sc = ({} if kscales is None
                  else dict(kscale=kscales[li], vscale=vscales[li]))
            if decode:
                x, x_alt, moe_out = self._decode_layer(
                    layer, kcaches[li], vcaches[li], st, x, x_alt, moe_out,
                    **sc)
            elif wide:
                moe_out = self._wide_layer(
                    layer, kcaches[li], vcaches[li], st, x, moe_out,
                    **sc)
            else:
                moe_out = self._prefill_layer(
                    layer, kcaches[li], vcaches[li], st, x, moe_out,
                    **sc)

        # final residual add + norm; skip lm_head entirely for logits-free
        # prefill chunks (an empty logits_rows means "no sampling this chunk")
        if logits_rows is not None and logits_rows.numel() == 0:
            return torch.empty(0, cfg.vocab_size, dtype=torch.float32,
                               device=x.device)
        hbuf = st.hbuf
        ops.fused_add_rmsnorm(hbuf, x, moe_out, self.final_norm_w, cfg.rms_eps)
        sel = hbuf if logits_rows is None else hbuf[logits_rows.long()]
        if sel.size(0) <= 8:
            # B-specialized GEMV (the earlier 2.5 TB/s vs hipBLASLt 3 TB/s
            # comparison predates the exact-batch template)
            logits = torch.empty(sel.size(0), cfg.vocab_size,
                                 dtype=torch.float32, device=x.device)
            ops.gemv(logits, sel.contiguous(), self.lm_head)
        elif wide:
            # f32 logits straight from the MFMA accumulators: no hipBLASLt
            # (capture-safe) and no bf16 rounding before the sampler
            logits = torch.empty(sel.size(0), cfg.vocab_size,
                                 dtype=torch.float32, device=x.device)
            ops.skinny_gemm(logits, sel.contiguous(), self.lm_head)
        else:
            logits = F.linear(sel, self.lm_head).float()
        return logits

    def _decode_layer(self, layer: Qwen3MoELayer, kcache: torch.Tensor,
                      vcache: torch.Tensor, st: "_Step", x: torch.Tensor,
                      x_alt: torch.Tensor, moe_out: torch.Tensor | None,
                      kscale: torch.Tensor | None = None,
                      vscale: torch.Tensor | None = None):
        """One layer at T ≤ 8: every projection on the hand-written GEMVs,
        split-KV attention, pair-GEMV MoE. Returns (x, x_alt, moe_out); the
        residual ping-pongs between x and x_alt at T ≤ 2."""
        cfg = self.cfg
        T = x.size(0)
        qdim = cfg.num_q_heads * cfg.head_dim
        hbuf, qkv = st.hbuf, st.qkv
        # --- attention block
        if T <= 2:
            # fused add(moe_prev)+RMSNorm+QKV-GEMV: one kernel replaces
            # fused_add_rmsnorm (or rmsnorm) + gemv, with their bits; the
            # residual lands in the other ping-pong buffer. Faster than the
            # pair at B ≤ 2 (8.6 → 6.7 and 9.4 → 7.8 µs per layer); at B = 5
            # it ties (11.6 vs 11.8) and at B = 8 it loses (14.2 vs 17.0), so
            # larger batches keep the two launches
            if moe_out is None:
                ops.gemv_addnorm(qkv, x, st.empty_delta, x, layer.input_norm_w,
                                 layer.wqkv, cfg.rms_eps)
            else:
                ops.gemv_addnorm(qkv, x, moe_out, x_alt, layer.input_norm_w,
                                 layer.wqkv, cfg.rms_eps)
                x, x_alt = x_alt, x
        else:
            if moe_out is None:
                ops.rmsnorm(hbuf, x, layer.input_norm_w, cfg.rms_eps)
            else:
                ops.fused_add_rmsnorm(hbuf, x, moe_out, layer.input_norm_w,
                                      cfg.rms_eps)
            ops.gemv(qkv, hbuf, layer.wqkv)
        # q stays a strided view into qkv (the attention kernels take a
        # row stride; .contiguous() copies profiled at 0.67 ms/step)
        q = qkv[:, :qdim].view(T, cfg.num_q_heads, cfg.head_dim)
        ops.qk_rope_write_kv(qkv, cfg.num_q_heads, kcache, vcache,
                             layer.q_norm_w, layer.k_norm_w, self.cos_t,
                             self.sin_t, st.block_table, st.seq_ids, st.q_pos,
                             cfg.rms_eps, kscale, vscale)
        attn = torch.empty(T, cfg.num_q_heads, cfg.head_dim,
                           dtype=torch.bfloat16, device=x.device)
        ops.paged_attention_split(attn, q, kcache, vcache, st.block_table,
                                  st.seq_ids, st.q_pos, st.part, st.part_ml,
                                  self.scale, splits=self.attn_splits,
                                  k_scale=kscale, v_scale=vscale)
        # O projection with the residual add in its epilogue (x updated in
        # place), then the post-attention norm inside the router GEMV, which
        # also leaves the normed rows in hbuf for the MoE: no norm launch
        ops.gemv_residual(x, attn.reshape(T, qdim), layer.wo)
        # --- MoE block
        topk_ids, topk_w = ops.router_norm_gemv_topk(
            hbuf, x, layer.post_attn_norm_w, layer.router_w,
            cfg.num_experts_per_tok, cfg.rms_eps)
        return x, x_alt, self._moe(hbuf, layer, topk_ids, topk_w, st)

    def _wide_layer(self, layer: Qwen3MoELayer, kcache: torch.Tensor,
                    vcache: torch.Tensor, st: "_Step", x: torch.Tensor,
                    moe_out: torch.Tensor | None,
                    kscale: torch.Tensor | None = None,
                    vscale: torch.Tensor | None = None) -> torch.Tensor:
        """One layer at 9 ≤ T ≤ 64 (a decode batch): every projection and
        both MoE GEMMs on the skinny MFMA GEMM, split-KV attention per row,
        expert-sorted MoE with the gather combine. No hipBLASLt (capture-
        safe) and no float atomics (run-to-run deterministic). x is updated
        in place; returns moe_out."""
        cfg = self.cfg
        T = x.size(0)
        qdim = cfg.num_q_heads * cfg.head_dim
        hbuf, qkv = st.hbuf, st.qkv
        # --- attention block
        if moe_out is None:
            ops.rmsnorm(hbuf, x, layer.input_norm_w, cfg.rms_eps)
        else:
            ops.fused_add_rmsnorm(hbuf, x, moe_out, layer.input_norm_w,
                                  cfg.rms_eps)
        ops.skinny_gemm(qkv, hbuf, layer.wqkv)
        q = qkv[:, :qdim].view(T, cfg.num_q_heads, cfg.head_dim)
        ops.qk_rope_write_kv(qkv, cfg.num_q_heads, kcache, vcache,
                             layer.q_norm_w, layer.k_norm_w, self.cos_t,
                             self.sin_t, st.block_table, st.seq_ids, st.q_pos,
                             cfg.rms_eps, kscale, vscale)
        ops.paged_attention_split(st.attn, q, kcache, vcache, st.block_table,
                                  st.seq_ids, st.q_pos, st.part, st.part_ml,
                                  self.scale, splits=self.attn_splits,
                                  k_scale=kscale, v_scale=vscale)
        ops.skinny_gemm(st.obuf, st.attn.view(T, qdim), layer.wo)
        # --- MoE block
        ops.fused_add_rmsnorm(hbuf, x, st.obuf, layer.post_attn_norm_w,
                              cfg.rms_eps)
        E = cfg.num_experts
        wr = layer.router_w
        if E % 16:   # reduced test configs: pad the router to a full fragment
            wr = self._wide_rpad.get(id(layer.router_w))
            if wr is None:
                wr = torch.zeros(st.router_logits.size(1), cfg.hidden_size,
                                 dtype=torch.bfloat16, device=x.device)
                wr[:E] = layer.router_w
                self._wide_rpad[id(layer.router_w)] = wr
        ops.skinny_gemm(st.router_logits, hbuf, wr)
        logits = (st.router_logits if E % 16 == 0
                  else st.router_logits[:, :E].contiguous())
        topk_ids, topk_w = ops.moe_router(logits, cfg.num_experts_per_tok)
        return self._moe_wide(hbuf, layer, topk_ids, topk_w, st)

    def _moe_wide(self, hbuf: torch.Tensor, layer: Qwen3MoELayer,
                  topk_ids: torch.Tensor, topk_w: torch.Tensor,
                  st: "_Step") -> torch.Tensor:
        """_moe's expert-sorted path on 16-row tiles: at ≤ 64 tokens an
        expert sees a handful of rows, so the skinny GEMM streams each
        touched expert's panel once instead of filling a 128-row tile."""
        cfg = self.cfg
        flat_expert = topk_ids.flatten()
        order = torch.argsort(flat_expert)
        pair_expert = flat_expert[order].int().contiguous()
        pair_token = st.pair_token[order].contiguous()
        P = pair_token.numel()
        inv_order = torch.empty_like(order)
        inv_order[order] = torch.arange(P, device=hbuf.device)
        inv_order = inv_order.int().contiguous()
        desc = ops.moe_build_desc_device(pair_expert, cfg.num_experts, bm=16)
        if self.expert_dtype == "fp8":
            ops.moe_grouped_gemm_skinny_fp8(st.gateup, hbuf, layer.w13_q,
                                            layer.w13_s, pair_token, desc)
            ops.silu_mul(st.hmid, st.gateup)
            ops.moe_grouped_gemm_skinny_fp8(st.z, st.hmid, layer.w2_q,
                                            layer.w2_s, st.pair_row, desc)
        else:
            ops.moe_grouped_gemm_skinny(st.gateup, hbuf, layer.w13,
                                        pair_token, desc)
            ops.silu_mul(st.hmid, st.gateup)
            # the down GEMM reads h rows per sorted pair: identity pair map
            ops.moe_grouped_gemm_skinny(st.z, st.hmid, layer.w2, st.pair_row,
                                        desc)
        ops.moe_combine_gather(st.moe_out, st.z, topk_w.contiguous(),
                               inv_order)
        return st.moe_out

    def _prefill_layer(self, layer: Qwen3MoELayer, kcache: torch.Tensor,
                       vcache: torch.Tensor, st: "_Step", x: torch.Tensor,
                       moe_out: torch.Tensor | None,
                       kscale: torch.Tensor | None = None,
                       vscale: torch.Tensor | None = None) -> torch.Tensor:
        """One layer at T > 8: dense projections through _dense, MFMA flash
        prefill (or the unified paged kernel without q-tile descriptors),
        grouped-GEMM MoE. x is updated in place; returns moe_out."""
        cfg = self.cfg
        T = x.size(0)
        qdim = cfg.num_q_heads * cfg.head_dim
        hbuf = st.hbuf
        # --- attention block
        if moe_out is None:
            ops.rmsnorm(hbuf, x, layer.input_norm_w, cfg.rms_eps)
        else:
            ops.fused_add_rmsnorm(hbuf, x, moe_out, layer.input_norm_w,
                                  cfg.rms_eps)
        qkv = self._dense(hbuf, layer.wqkv)
        q = qkv[:, :qdim].view(T, cfg.num_q_heads, cfg.head_dim)
        ops.qk_rope_write_kv(qkv, cfg.num_q_heads, kcache, vcache,
                             layer.q_norm_w, layer.k_norm_w, self.cos_t,
                             self.sin_t, st.block_table, st.seq_ids, st.q_pos,
                             cfg.rms_eps, kscale, vscale)
        attn = torch.empty(T, cfg.num_q_heads, cfg.head_dim,
                           dtype=torch.bfloat16, device=x.device)
        if st.qtile_desc is not None:
            ops.flash_prefill(attn, q, kcache, vcache, st.block_table,
                              st.seq_ids, st.q_pos, st.qtile_desc, self.scale,
                              kscale, vscale)
            o = self._dense(attn.reshape(T, qdim), layer.wo)
        else:
            ops.paged_attention(attn, q, kcache, vcache, st.block_table,
                                st.seq_ids, st.q_pos, self.scale,
                                kscale, vscale)
            o = F.linear(attn.reshape(T, qdim), layer.wo)
        # --- MoE block
        ops.fused_add_rmsnorm(hbuf, x, o, layer.post_attn_norm_w, cfg.rms_eps)
        router_logits = self._dense(hbuf, layer.router_w).float()
        topk_ids, topk_w = ops.moe_router(router_logits,
                                          cfg.num_experts_per_tok)
        return self._moe(hbuf, layer, topk_ids, topk_w, st)

    def _moe(self, hbuf: torch.Tensor, layer: Qwen3MoELayer,
             topk_ids: torch.Tensor, topk_w: torch.Tensor,
             st: "_Step") -> torch.Tensor:
        cfg = self.cfg
        T = hbuf.size(0)
        H, I = cfg.hidden_size, cfg.moe_intermediate_size

        if T < cfg.moe_grouped_threshold:
            # GEMV per (token, expert) pair; the f32 accumulator feeds
            # fused_add_rmsnorm directly (templated input dtype — skips a
            # cast kernel per layer)
            out = torch.empty(T, H, dtype=torch.float32, device=hbuf.device)
            pair_token = st.pair_token
            pair_expert = topk_ids.flatten().contiguous()
            pair_w = topk_w.flatten().contiguous()
            P = pair_token.numel()
            h = torch.empty(P, I, dtype=torch.bfloat16, device=hbuf.device)
            if self.expert_dtype == "fp8":
                ops.moe_gemv_h_fp8(h, hbuf, layer.w13_q, layer.w13_s,
                                   pair_token, pair_expert, out_zero=out)
                ops.moe_gemv_down_fp8(out, h, layer.w2_q, layer.w2_s, pair_w,
                                      pair_token, pair_expert)
                return out
            ops.moe_gemv_h(h, hbuf, layer.w13, pair_token, pair_expert,
                           out_zero=out)
            ops.moe_gemv_down(out, h, layer.w2, pair_w, pair_token, pair_expert)
            return out

        # sort pairs by expert, grouped MFMA GEMMs
        flat_expert = topk_ids.flatten()
        order = torch.argsort(flat_expert)
        pair_expert = flat_expert[order].int().contiguous()
        pair_token = st.pair_token[order].contiguous()
        P = pair_token.numel()
        inv_order = torch.empty_like(order)
        inv_order[order] = torch.arange(P, device=hbuf.device)
        inv_order = inv_order.int().contiguous()
        desc = ops.moe_build_desc_device(pair_expert, cfg.num_experts)
        lean = not self.expert_image      # fp8 without the bf16 image
        gateup = torch.empty(P, 2 * I, dtype=torch.bfloat16, device=hbuf.device)
        if lean:
            ops.moe_grouped_gemm128_fp8(gateup, hbuf, layer.w13_q,
                                        layer.w13_s, pair_token, desc)
        else:
            ops.moe_grouped_gemm128(gateup, hbuf, layer.w13, pair_token, desc)
        h = torch.empty(P, I, dtype=torch.bfloat16, device=hbuf.device)
        ops.silu_mul(h, gateup)
        z = torch.empty(P, H, dtype=torch.bfloat16, device=hbuf.device)
        # the down GEMM reads h rows per sorted pair: identity pair map
        if lean:
            ops.moe_grouped_gemm128_fp8(z, h, layer.w2_q, layer.w2_s,
                                        st.pair_row, desc)
        else:
            ops.moe_grouped_gemm128(z, h, layer.w2, st.pair_row, desc)
        out_bf = torch.empty(T, H, dtype=torch.bfloat16, device=hbuf.device)
        ops.moe_combine_gather(out_bf, z, topk_w.contiguous(), inv_order)
        return out_bf
