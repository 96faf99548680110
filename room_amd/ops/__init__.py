"""CDNA4 kernel library bindings.

On a GPU box the extension MUST load — there is no eager/PyTorch fallback for
the compute path (a silent fallback would fake GPU test results). CPU-only
environments (CI here) can import this module; calling any op raises.
"""
from __future__ import annotations

import contextlib

import torch

from ..engine.step_plan import qtile_list

_C = None
_import_error: Exception | None = None
try:
    from room_amd import _C  # type: ignore
except Exception as e:  # pragma: no cover
    _import_error = e

if _C is None and torch.cuda.is_available():
    raise ImportError(
        "room_amd._C HIP extension missing on a GPU machine — build it with "
        "`PYTORCH_ROCM_ARCH=gfx950 python setup.py build_ext --inplace`. "
        f"Import error: {_import_error}")


def _require():
    if _C is None:
        raise RuntimeError(
            f"room_amd._C not available (CPU-only environment?): {_import_error}")
    return _C


@contextlib.contextmanager
def check_only():
    """Inside the block every op returns after its argument checks and before
    its launch, and the tensors may live on any one device: for testing the
    wrappers' contracts (csrc/checks.h). Process-wide; nothing in the engine
    uses it."""
    C = _require()
    before = C.check_only()
    C.set_check_only(True)
    try:
        yield
    finally:
        C.set_check_only(before)


def rmsnorm(out: torch.Tensor, x: torch.Tensor, weight: torch.Tensor,
            eps: float = 1e-6) -> torch.Tensor:
    _require().rmsnorm(out, x, weight, eps)
    return out


def fused_add_rmsnorm(out: torch.Tensor, residual: torch.Tensor, x: torch.Tensor,
                      weight: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    _require().fused_add_rmsnorm(out, residual, x, weight, eps)
    return out


def qk_norm_rope(q: torch.Tensor, k: torch.Tensor, q_w: torch.Tensor,
                 k_w: torch.Tensor, cos_t: torch.Tensor, sin_t: torch.Tensor,
                 positions: torch.Tensor, n_qheads: int, n_kvheads: int,
                 head_dim: int = 128, eps: float = 1e-6) -> None:
    _require().qk_norm_rope(q, k, q_w, k_w, cos_t, sin_t, positions,
                            n_qheads, n_kvheads, head_dim, eps)


def qk_rope_write_kv(qkv: torch.Tensor, n_qheads: int,
                     kcache: torch.Tensor, vcache: torch.Tensor,
                     q_w: torch.Tensor, k_w: torch.Tensor,
                     cos_t: torch.Tensor, sin_t: torch.Tensor,
                     block_table: torch.Tensor, seq_ids: torch.Tensor,
                     positions: torch.Tensor, eps: float = 1e-6,
                     k_scale: torch.Tensor | None = None,
                     v_scale: torch.Tensor | None = None) -> None:
    """Fused per-head QK RMSNorm + RoPE + paged KV scatter, operating directly
    on the packed [T, (Hq+2Hk)*D] projection output (no q/k/v copies).

    fp8 KV cache: with float8_e4m3fn caches, k_scale and v_scale
    [NB, Hk, 16] f32 are required; every written row gets the bytes and the
    scale of reference.quantize_kv_rows of the row the bf16 form stores, and
    Q gets the same bits. (The same two arguments on the three attention ops
    below: their output is bit-equal to the bf16 op on the cache's image,
    dequantize_kv_rows(...).to(bf16).)"""
    _require().qk_rope_write_kv(qkv, kcache, vcache, q_w, k_w, cos_t,
                                sin_t, block_table, seq_ids, positions,
                                n_qheads, eps, k_scale, v_scale)


def silu_mul(out: torch.Tensor, gateup: torch.Tensor) -> torch.Tensor:
    _require().silu_mul(out, gateup)
    return out


def paged_attention(out: torch.Tensor, q: torch.Tensor, kcache: torch.Tensor,
                    vcache: torch.Tensor, block_table: torch.Tensor,
                    seq_ids: torch.Tensor, q_pos: torch.Tensor,
                    scale: float, k_scale: torch.Tensor | None = None,
                    v_scale: torch.Tensor | None = None) -> torch.Tensor:
    _require().paged_attention(out, q, kcache, vcache, block_table, seq_ids,
                               q_pos, scale, k_scale, v_scale)
    return out


def write_kv(kcache: torch.Tensor, vcache: torch.Tensor, k: torch.Tensor,
             v: torch.Tensor, block_table: torch.Tensor, seq_ids: torch.Tensor,
             q_pos: torch.Tensor) -> None:
    _require().write_kv(kcache, vcache, k, v, block_table, seq_ids, q_pos)


def attn_nsplits() -> int:
    """Decode split-KV NSPLITS (compiled into the kernel)."""
    if _C is not None and hasattr(_C, "attn_nsplits"):
        return int(_C.attn_nsplits())
    return 32


def paged_attention_split(out: torch.Tensor, q: torch.Tensor, kcache: torch.Tensor,
                          vcache: torch.Tensor, block_table: torch.Tensor,
                          seq_ids: torch.Tensor, q_pos: torch.Tensor,
                          part: torch.Tensor, part_ml: torch.Tensor,
                          scale: float, splits: int = 32,
                          k_scale: torch.Tensor | None = None,
                          v_scale: torch.Tensor | None = None) -> torch.Tensor:
    """Split-KV flash-decode: part [T, Hq, NSPLITS_MAX, 128] f32, part_ml
    [.., 2]; `splits` (32 short / 64 long contexts) sets the launch grid —
    shorter per-WG chunk chains win once the serial span passes ~8k."""
    _require().paged_attention_split(out, q, kcache, vcache, block_table,
                                     seq_ids, q_pos, part, part_ml, scale,
                                     splits, k_scale, v_scale)
    return out


def gemv(y: torch.Tensor, x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """y[B,N] = x[B,H] @ w[N,H]^T for B<=8 (decode projections)."""
    _require().gemv(y, x, w)
    return y


def gemv_residual(r: torch.Tensor, x: torch.Tensor, w: torch.Tensor
                  ) -> torch.Tensor:
    """r[B,N] = bf16(bf16(x[B,H] @ w[N,H]^T) + r) in place for B<=8: the
    decode O projection with the residual add in its epilogue. Same bits in r
    as gemv (bf16 out) followed by fused_add_rmsnorm's add."""
    _require().gemv_residual(r, x, w)
    return r


def flash_prefill(out: torch.Tensor, q: torch.Tensor, kcache: torch.Tensor,
                  vcache: torch.Tensor, block_table: torch.Tensor,
                  seq_ids: torch.Tensor, q_pos: torch.Tensor,
                  tile_desc: torch.Tensor, scale: float,
                  k_scale: torch.Tensor | None = None,
                  v_scale: torch.Tensor | None = None) -> torch.Tensor:
    """MFMA flash prefill; tile_desc [G,2] = (row0, n_tokens≤32), one sequence
    per tile (build with build_qtile_desc). q may be a row-strided view of
    the packed qkv; out, the caches, the block table and the int32 vectors
    must be contiguous (checked by the wrapper)."""
    _require().flash_prefill(out, q, kcache, vcache, block_table, seq_ids,
                             q_pos, tile_desc, scale, k_scale, v_scale)
    return out


def flash_prefill_qtile() -> int:
    """Q rows per flash_prefill tile (FP_QTOK, compiled into the kernel)."""
    if _C is not None and hasattr(_C, "flash_prefill_qtile"):
        return int(_C.flash_prefill_qtile())
    return 32


def build_qtile_desc(segments: list, device) -> torch.Tensor:
    """Q-tile descriptors from host-known prefill segments [(row0, count), ...]
    (one sequence per segment) — no device sync."""
    desc = qtile_list(segments, flash_prefill_qtile())
    if not desc:
        return torch.zeros(0, 2, dtype=torch.int32, device=device)
    return torch.tensor(desc, dtype=torch.int32, device=device)


def gemv_addnorm(y: torch.Tensor, x: torch.Tensor, delta: torch.Tensor,
                 x_out: torch.Tensor, gamma: torch.Tensor, w: torch.Tensor,
                 eps: float = 1e-6) -> torch.Tensor:
    """y = rmsnorm(x + delta)·γ @ w^T; x_out = x + delta (pass delta with
    numel 0 for a plain norm+gemv; x_out is then not written). Decode-path
    fusion (B ≤ 8) with the bits of fused_add_rmsnorm (or rmsnorm) followed by
    gemv."""
    _require().gemv_addnorm(y, x, delta, x_out, gamma, w, eps)
    return y


def moe_router(logits: torch.Tensor, k: int) -> tuple[torch.Tensor, torch.Tensor]:
    T = logits.size(0)
    ids = torch.empty(T, k, dtype=torch.int32, device=logits.device)
    w = torch.empty(T, k, dtype=torch.float32, device=logits.device)
    _require().moe_router(ids, w, logits, k)
    return ids, w


def router_gemv_topk(x: torch.Tensor, wr: torch.Tensor,
                     k: int) -> tuple[torch.Tensor, torch.Tensor]:
    """Decode router: 4-way H-split partial GEMV (wide grid) + top-k kernel
    that sums the partials on load. Replaces gemv + moe_router."""
    T = x.size(0)
    ids = torch.empty(T, k, dtype=torch.int32, device=x.device)
    w = torch.empty(T, k, dtype=torch.float32, device=x.device)
    _require().router_gemv_topk(ids, w, x, wr, k)
    return ids, w


def router_norm_gemv_topk(hbuf: torch.Tensor, r: torch.Tensor,
                          gamma: torch.Tensor, wr: torch.Tensor, k: int,
                          eps: float = 1e-6
                          ) -> tuple[torch.Tensor, torch.Tensor]:
    """Decode router on the residual rows r [T, H]: hbuf = rmsnorm(r)·γ and
    the top-k of hbuf @ wr^T, with the norm computed inside the router GEMV
    (one wave per expert row and token). Same bits in hbuf, ids and weights
    as rmsnorm followed by router_gemv_topk."""
    T = r.size(0)
    ids = torch.empty(T, k, dtype=torch.int32, device=r.device)
    w = torch.empty(T, k, dtype=torch.float32, device=r.device)
    _require().router_norm_gemv_topk(ids, w, hbuf, r, gamma, wr, k, eps)
    return ids, w


def moe_gemv_h(h: torch.Tensor, x: torch.Tensor, w13: torch.Tensor,
               pair_token: torch.Tensor, pair_expert: torch.Tensor,
               out_zero: torch.Tensor | None = None) -> torch.Tensor:
    """Gate/up GEMV + silu-mul per (token, expert) pair. out_zero: optional
    f32 tensor zero-filled as a side job (the down kernel's accumulator)."""
    if out_zero is None:
        out_zero = torch.empty(0, dtype=torch.float32, device=h.device)
    _require().moe_gemv_h(h, x, w13, pair_token, pair_expert, out_zero)
    return h


def moe_gemv_down(out: torch.Tensor, h: torch.Tensor, w2: torch.Tensor,
                  pair_w: torch.Tensor, pair_token: torch.Tensor,
                  pair_expert: torch.Tensor) -> torch.Tensor:
    _require().moe_gemv_down(out, h, w2, pair_w, pair_token, pair_expert)
    return out


def moe_grouped_gemm128(out: torch.Tensor, x: torch.Tensor, w: torch.Tensor,
                        pair_token: torch.Tensor, tile_desc: torch.Tensor
                        ) -> torch.Tensor:
    """Grouped MFMA GEMM: expert weight panels read once per 128-row m-tile
    (tile_desc from moe_build_desc_device)."""
    _require().moe_grouped_gemm128(out, x, w, pair_token, tile_desc)
    return out


def skinny_gemm(y: torch.Tensor, x: torch.Tensor, w: torch.Tensor
                ) -> torch.Tensor:
    """y[M,N] = x[M,K] @ w[N,K]^T for 1 <= M <= 64 (wide-decode projections):
    one MFMA tile of 16/32/48/64 rows chosen from M, weights streamed straight
    into registers. y is bf16 or f32. A row's result does not depend on M or
    on the other rows."""
    if x.size(0) > SKINNY_MAX_ROWS:
        raise ValueError(f"skinny_gemm handles at most {SKINNY_MAX_ROWS} rows, "
                         f"got {x.size(0)}")
    _require().skinny_gemm(y, x, w)
    return y


def moe_grouped_gemm_skinny(out: torch.Tensor, x: torch.Tensor,
                            w: torch.Tensor, pair_token: torch.Tensor,
                            tile_desc: torch.Tensor) -> torch.Tensor:
    """Grouped MFMA GEMM over 16-row m-tiles (tile_desc from
    moe_build_desc_device(..., bm=16)): out[p] = x[pair_token[p]] @ w[e]^T."""
    _require().moe_grouped_gemm_skinny(out, x, w, pair_token, tile_desc)
    return out


SKINNY_MAX_ROWS = 64   # tallest skinny_gemm tile (4 MFMA row fragments)


# ---- fp8 expert weights (expert_dtype="fp8"): e4m3fn bytes in the bf16
# layouts plus one f32 scale per 128x128 block (reference.quantize_fp8_block).
# Activations stay bf16, accumulation f32; see csrc/moe_fp8.hip.

def moe_gemv_h_fp8(h: torch.Tensor, x: torch.Tensor, w13_q: torch.Tensor,
                   w13_s: torch.Tensor, pair_token: torch.Tensor,
                   pair_expert: torch.Tensor,
                   out_zero: torch.Tensor | None = None) -> torch.Tensor:
    """moe_gemv_h on fp8 weights: w13_q [E, 2I, H] float8_e4m3fn, w13_s
    [E, 2I/128, H/128] f32; H and I multiples of 128."""
    if out_zero is None:
        out_zero = torch.empty(0, dtype=torch.float32, device=h.device)
    _require().moe_gemv_h_fp8(h, x, w13_q, w13_s, pair_token, pair_expert,
                              out_zero)
    return h


def moe_gemv_down_fp8(out: torch.Tensor, h: torch.Tensor, w2_q: torch.Tensor,
                      w2_s: torch.Tensor, pair_w: torch.Tensor,
                      pair_token: torch.Tensor, pair_expert: torch.Tensor
                      ) -> torch.Tensor:
    """moe_gemv_down on fp8 weights: w2_q [E, H, I] float8_e4m3fn, w2_s
    [E, H/128, I/128] f32."""
    _require().moe_gemv_down_fp8(out, h, w2_q, w2_s, pair_w, pair_token,
                                 pair_expert)
    return out


def moe_grouped_gemm_skinny_fp8(out: torch.Tensor, x: torch.Tensor,
                                w_q: torch.Tensor, w_s: torch.Tensor,
                                pair_token: torch.Tensor,
                                tile_desc: torch.Tensor) -> torch.Tensor:
    """moe_grouped_gemm_skinny on fp8 weights: w_q [E, N, K] float8_e4m3fn,
    w_s [E, N/128, K/128] f32. A row's bits depend on (N, K) only."""
    _require().moe_grouped_gemm_skinny_fp8(out, x, w_q, w_s, pair_token,
                                           tile_desc)
    return out


def moe_grouped_gemm128_fp8(out: torch.Tensor, x: torch.Tensor,
                            w_q: torch.Tensor, w_s: torch.Tensor,
                            pair_token: torch.Tensor, tile_desc: torch.Tensor
                            ) -> torch.Tensor:
    """moe_grouped_gemm128 on fp8 weights (prefill): out [P, N] bf16, x [T, K]
    bf16, w_q [E, N, K] float8_e4m3fn, w_s [E, N/128, K/128] f32, tile_desc
    from moe_build_desc_device(..., bm=128). A weight tile is staged as
    bf16_rne(f32(q) · s) and then runs the bf16 kernel's MFMA sequence, so out
    equals moe_grouped_gemm128 on dequantize_fp8_block(w_q, w_s).to(bf16) bit
    for bit (unlike the decode fp8 kernels, which scale f32 partial sums).
    Allocates nothing."""
    _require().moe_grouped_gemm128_fp8(out, x, w_q, w_s, pair_token,
                                       tile_desc)
    return out


def moe_desc_gmax(num_pairs: int, num_experts: int, bm: int = 128) -> int:
    """Descriptor rows that always suffice: every expert can end in one
    ragged tile on top of the ceil(P/bm) full ones."""
    return num_experts + (num_pairs + bm - 1) // bm


def moe_build_desc_device(pair_expert_sorted: torch.Tensor,
                          num_experts: int, bm: int = 128) -> torch.Tensor:
    """Sync-free [GMAX,3] (expert,row0,msize) descriptors of bm-row m-tiles
    (128 for moe_grouped_gemm128, 16 for moe_grouped_gemm_skinny); GMAX
    computed from the host-known pair count, empty tiles zero-sized."""
    P = pair_expert_sorted.numel()
    gmax = moe_desc_gmax(P, num_experts, bm)
    # NOT torch.bincount: its nbins probe (.max().item()) host-syncs, which
    # aborts hipGraph capture — scatter_add_ is sync-free
    counts = torch.zeros(num_experts, dtype=torch.int64,
                         device=pair_expert_sorted.device)
    counts.scatter_add_(0, pair_expert_sorted.long(),
                        torch.ones(P, dtype=torch.int64,
                                   device=pair_expert_sorted.device))
    desc = torch.empty(gmax, 3, dtype=torch.int32,
                       device=pair_expert_sorted.device)
    _require().moe_build_desc(desc, counts, bm)
    return desc


def dense_grouped_gemm(y: torch.Tensor, x: torch.Tensor, w: torch.Tensor,
                       desc: torch.Tensor, pair_token: torch.Tensor
                       ) -> torch.Tensor:
    """Capture-safe dense GEMM y[T,N] = x[T,H] @ w[N,H]^T via the grouped
    MFMA kernel with a single expert. hipBLASLt is faster eager but its
    internal calls abort hipGraph capture; inside captured prefill forwards
    this path runs instead (desc/pair_token prebuilt per T by the model)."""
    _require().moe_grouped_gemm128(y, x, w.unsqueeze(0), pair_token, desc)
    return y


def moe_combine_gather(out: torch.Tensor, z: torch.Tensor, topk_w: torch.Tensor,
                       inv_order: torch.Tensor) -> torch.Tensor:
    _require().moe_combine_gather(out, z, topk_w, inv_order)
    return out


def sample_tokens(logits: torch.Tensor, seeds: torch.Tensor, top_k: int = 40,
                  temperature: float = 0.7, top_p: float = 0.95) -> torch.Tensor:
    """One parameter set for the whole batch: sample_rows with the scalars
    broadcast per row, penalties off, draw 0 of each row's seed."""
    if not 1 <= top_k <= MAX_TOP_K:
        raise ValueError(f"top_k must be 1..{MAX_TOP_K}")
    B, dev = logits.size(0), logits.device
    f32 = dict(dtype=torch.float32, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    zi = torch.zeros(B, **i32)
    zf = torch.zeros(B, **f32)
    return sample_rows(
        logits, torch.full((B,), temperature, **f32),
        torch.full((B,), top_p, **f32), torch.full((B,), top_k, **i32),
        seeds, zi, torch.ones(B, **f32), zf, zf, zi,
        torch.zeros(B, RING, **i32), zi, append=False)


RING = 256        # token-history ring entries per row (SMP_RING in sampling.hip)
MAX_TOP_K = 64    # largest top_k (SMP_MAXK)


def sample_rows(logits: torch.Tensor, temperature: torch.Tensor,
                top_p: torch.Tensor, top_k: torch.Tensor, seeds: torch.Tensor,
                ctr: torch.Tensor, repetition_penalty: torch.Tensor,
                presence_penalty: torch.Tensor, frequency_penalty: torch.Tensor,
                repeat_last_n: torch.Tensor, ring: torch.Tensor,
                ring_len: torch.Tensor, append: bool = False,
                out: torch.Tensor | None = None) -> torch.Tensor:
    """Per-row sampler: every parameter is a device tensor with one entry per
    logits row. temperature ≤ 1e-5 is greedy; top_k 1..64; the draw is a pure
    function of (seeds[b], ctr[b]), both read-only. Penalties (llama.cpp
    order: repetition, then frequency·count + presence) apply to the tokens
    among the last repeat_last_n pushes of the row's ring ([B, 256] int32,
    push j at ring[b][j % 256], ring_len = pushes so far); repeat_last_n 0
    turns them off for the row. append=True pushes the picked token into the
    ring and bumps ring_len on the device. Two launches, no sync, no
    allocation when `out` is given (hipGraph-capturable)."""
    if out is None:
        out = torch.empty(logits.size(0), dtype=torch.int32,
                          device=logits.device)
    # two-stage sampler: per-slice register top-8 scan, then one wave per row
    _require().sample_rows(out, logits, temperature, top_p, top_k, seeds, ctr,
                           repetition_penalty, presence_penalty,
                           frequency_penalty, repeat_last_n, ring, ring_len,
                           append)
    return out


def vs_topk(mat: torch.Tensor, query: torch.Tensor, k: int,
            nblocks: int = 512) -> tuple[torch.Tensor, torch.Tensor]:
    """Cosine top-k over an HBM-resident [N, 384] bf16 matrix (rows L2-normed)."""
    dev = mat.device
    nblocks = min(nblocks, max(1, (mat.size(0) + 255) // 256))
    cand_v = torch.empty(nblocks, k, dtype=torch.float32, device=dev)
    cand_i = torch.empty(nblocks, k, dtype=torch.int32, device=dev)
    out_v = torch.empty(k, dtype=torch.float32, device=dev)
    out_i = torch.empty(k, dtype=torch.int64, device=dev)
    _require().vs_topk(out_v, out_i, cand_v, cand_i, mat, query, k)
    return out_v, out_i


def vs_topk_scoped(mat: torch.Tensor, tags: torch.Tensor, queries: torch.Tensor,
                   scopes: torch.Tensor, k: int, nblocks: int = 512
                   ) -> tuple[torch.Tensor, torch.Tensor]:
    """Room-scoped cosine top-k for a batch of 1..8 queries in one pass over
    the [N, 384] bf16 matrix. tags [N] int32 holds each row's room id (0 =
    global row); scopes [Q] int32 holds -1 (every row) or a room id s (rows
    tagged s or 0). Returns (values [Q, k] f32 descending, row indices [Q, k]
    int64); slots beyond the rows in scope hold -inf / -1."""
    dev = mat.device
    nq = queries.size(0)
    # the merge kernel holds every block's list head in one wave: ≤ 512 blocks
    nblocks = min(nblocks, 512, max(1, (mat.size(0) + 255) // 256))
    cand_v = torch.empty(nq, nblocks, k, dtype=torch.float32, device=dev)
    cand_i = torch.empty(nq, nblocks, k, dtype=torch.int32, device=dev)
    out_v = torch.empty(nq, k, dtype=torch.float32, device=dev)
    out_i = torch.empty(nq, k, dtype=torch.int64, device=dev)
    _require().vs_topk_scoped(out_v, out_i, cand_v, cand_i, mat, tags, queries,
                              scopes, k)
    return out_v, out_i


# ---- memory encoder (MiniEncoder impl="hip"); see csrc/encoder.hip. Rows of
# all texts are packed without padding; cu_rows [B+1] int32 holds cumulative
# row offsets, every segment 1..ENCODER_MAX_PIECES rows.

ENCODER_DIM = 384
ENCODER_MAX_PIECES = 128   # ENC_MAXLEN in encoder.hip


def _check_cu_rows(op: str, cu_rows: torch.Tensor, rows: int,
                   cu_rows_host) -> None:
    """Segment checks run on host values: cu_rows_host (a list or CPU tensor
    the caller already has; no device sync) or a copy of cu_rows."""
    if cu_rows.dtype != torch.int32 or cu_rows.dim() != 1 or cu_rows.numel() < 2:
        raise RuntimeError(f"{op}: cu_rows must be int32 [B+1]")
    cu = cu_rows_host if cu_rows_host is not None else cu_rows.cpu()
    cu = [int(v) for v in cu]
    if len(cu) != cu_rows.numel() or cu[0] != 0:
        raise RuntimeError(f"{op}: cu_rows must start at 0 and hold B+1 offsets")
    for lo, hi in zip(cu, cu[1:]):
        if not 1 <= hi - lo <= ENCODER_MAX_PIECES:
            raise RuntimeError(
                f"{op}: segment length {hi - lo} outside "
                f"1..{ENCODER_MAX_PIECES}")
    if cu[-1] != rows:
        raise RuntimeError(f"{op}: cu_rows[-1] = {cu[-1]} but {rows} rows")


def encoder_embed(x: torch.Tensor, feats: torch.Tensor, pos_ids: torch.Tensor,
                  pos_table: torch.Tensor) -> torch.Tensor:
    """x[r] = Σ of the row's four sparse ±0.5 features + pos_table[pos_ids[r]]
    as bf16 [R, 384]. feats [R, 4] int32, each (index << 1) | (1 for +0.5, 0
    for -0.5); features sharing an index accumulate. pos_table f32 [P, 384]."""
    _require().encoder_embed(x, feats, pos_ids, pos_table)
    return x


def encoder_attention(out: torch.Tensor, qkv: torch.Tensor,
                      cu_rows: torch.Tensor, cu_rows_host=None) -> torch.Tensor:
    """Bidirectional softmax attention inside each packed segment. qkv
    [R, 1152] bf16, rows q|k|v of 12 heads x 32; out [R, 384] bf16; scale
    32^-0.5 applied inside. A segment's output depends on its own rows only
    and has the same bits wherever it sits in the pack."""
    if qkv.dim() != 2 or qkv.size(1) != 3 * ENCODER_DIM:
        raise RuntimeError("encoder_attention: qkv rows are q|k|v, 1152 wide")
    _check_cu_rows("encoder_attention", cu_rows, qkv.size(0), cu_rows_host)
    _require().encoder_attention(out, qkv, cu_rows)
    return out


def gelu_(u: torch.Tensor) -> torch.Tensor:
    """Exact (erf) GELU in place on a contiguous bf16 tensor."""
    _require().gelu_(u)
    return u


def encoder_pool(out: torch.Tensor, h: torch.Tensor, cu_rows: torch.Tensor,
                 mu: torch.Tensor, cu_rows_host=None,
                 normalize: bool = True) -> torch.Tensor:
    """out[b] = L2-normalised (mean of segment b's rows of h - mu), f32
    [B, 384]; rows summed first to last. normalize=False writes the centred
    mean itself."""
    if h.dim() != 2 or h.size(1) != ENCODER_DIM:
        raise RuntimeError("encoder_pool: h must be [R, 384]")
    _check_cu_rows("encoder_pool", cu_rows, h.size(0), cu_rows_host)
    _require().encoder_pool(out, h, cu_rows, mu, normalize)
    return out
