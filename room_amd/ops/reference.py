"""Pure-PyTorch fp32 reference implementations of every HIP kernel.

Used ONLY by numerics tests (tests/test_kernels_gpu.py compares each CDNA4
kernel against these on random inputs) and never on the GPU compute path.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F


def rmsnorm_ref(x: torch.Tensor, w: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    xf = x.float()
    scale = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return (xf * scale * w.float()).to(x.dtype)


def fused_add_rmsnorm_ref(residual: torch.Tensor, x: torch.Tensor, w: torch.Tensor,
                          eps: float = 1e-6) -> tuple[torch.Tensor, torch.Tensor]:
    new_res = (residual.float() + x.float()).to(x.dtype)
    return rmsnorm_ref(new_res, w, eps), new_res


def rope_tables(max_pos: int, head_dim: int, theta: float) -> tuple[torch.Tensor, torch.Tensor]:
    half = head_dim // 2
    inv_freq = 1.0 / (theta ** (torch.arange(0, half, dtype=torch.float64) / half))
    pos = torch.arange(max_pos, dtype=torch.float64)
    ang = torch.outer(pos, inv_freq)
    return ang.cos().float(), ang.sin().float()


def qk_norm_rope_ref(q: torch.Tensor, k: torch.Tensor, q_w: torch.Tensor,
                     k_w: torch.Tensor, cos_t: torch.Tensor, sin_t: torch.Tensor,
                     positions: torch.Tensor, eps: float = 1e-6
                     ) -> tuple[torch.Tensor, torch.Tensor]:
    """q: [T, Hq, D], k: [T, Hk, D]; per-head RMSNorm then rotate-half RoPE."""

    def one(x, w):
        xf = x.float()
        scale = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
        xn = xf * scale * w.float()
        half = x.size(-1) // 2
        c = cos_t[positions.long()].unsqueeze(1)  # [T,1,half]
        s = sin_t[positions.long()].unsqueeze(1)
        x1, x2 = xn[..., :half], xn[..., half:]
        out = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)
        return out.to(x.dtype)

    return one(q, q_w), one(k, k_w)


def silu_mul_ref(gateup: torch.Tensor) -> torch.Tensor:
    inter = gateup.size(-1) // 2
    g, u = gateup[..., :inter].float(), gateup[..., inter:].float()
    return (F.silu(g) * u).to(gateup.dtype)


def paged_attention_ref(q: torch.Tensor, kcache: torch.Tensor, vcache: torch.Tensor,
                        block_table: torch.Tensor, seq_ids: torch.Tensor,
                        q_pos: torch.Tensor, scale: float) -> torch.Tensor:
    """q: [T, Hq, D]; caches [NB, Hk, BS, D]. Gathers each token's KV prefix
    and does fp32 SDPA per token."""
    T, Hq, D = q.shape
    Hk, BS = kcache.size(1), kcache.size(2)
    group = Hq // Hk
    out = torch.zeros_like(q, dtype=torch.float32)
    for t in range(T):
        seq = int(seq_ids[t])
        bound = int(q_pos[t]) + 1
        nblocks = (bound + BS - 1) // BS
        blocks = block_table[seq, :nblocks].long()
        k = kcache[blocks].transpose(0, 1).reshape(Hk, nblocks * BS, D)[:, :bound]
        v = vcache[blocks].transpose(0, 1).reshape(Hk, nblocks * BS, D)[:, :bound]
        for hq in range(Hq):
            hk = hq // group
            scores = (q[t, hq].float() @ k[hk].float().T) * scale
            p = torch.softmax(scores, dim=-1)
            out[t, hq] = p @ v[hk].float()
    return out.to(q.dtype)


def moe_router_ref(logits: torch.Tensor, k: int) -> tuple[torch.Tensor, torch.Tensor]:
    probs = torch.softmax(logits.float(), dim=-1)
    topw, topi = probs.topk(k, dim=-1)
    topw = topw / topw.sum(-1, keepdim=True)
    return topi.int(), topw.float()


def moe_ref(x: torch.Tensor, w13: torch.Tensor, w2: torch.Tensor,
            topk_ids: torch.Tensor, topk_w: torch.Tensor) -> torch.Tensor:
    """x: [T,H]; w13: [E,2I,H]; w2: [E,H,I]; returns [T,H] fp32."""
    T, H = x.shape
    I = w2.size(2)
    out = torch.zeros(T, H, dtype=torch.float32, device=x.device)
    for t in range(T):
        for j in range(topk_ids.size(1)):
            e = int(topk_ids[t, j])
            gu = x[t].float() @ w13[e].float().T  # [2I]
            h = F.silu(gu[:I]) * gu[I:]
            # the kernels round h to bf16 between stages; mirror that
            h = h.to(torch.bfloat16).float()
            z = h @ w2[e].float().T  # [H]
            out[t] += float(topk_w[t, j]) * z
    return out


FP8_BLOCK = 128      # scale block edge of the fp8 expert-weight format
FP8_E4M3_MAX = 448.0


def quantize_fp8_block(w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """Block-scaled e4m3 quantiser of the fp8 expert-weight mode. w: bf16 or
    f32 [..., N, K] with N and K multiples of 128. Returns (q, scale): q
    float8_e4m3fn of w's shape, scale f32 [..., N/128, K/128] with
    w ≈ q · scale per 128×128 block. A block's scale is the power of two
    2^ceil(log2(amax/448)) (1.0 for an all-zero block), so |w/scale| ≤ 448,
    the cast never overflows, and every dequantised value is exactly
    representable in bf16. Plain torch; runs on CPU and GPU."""
    if w.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError(f"quantize_fp8_block takes bf16 or f32, got {w.dtype}")
    if w.dim() < 2 or w.size(-2) % FP8_BLOCK or w.size(-1) % FP8_BLOCK:
        raise ValueError("quantize_fp8_block needs [..., N, K] with N and K "
                         f"multiples of {FP8_BLOCK}, got {tuple(w.shape)}")
    B = FP8_BLOCK
    lead, N, K = w.shape[:-2], w.size(-2), w.size(-1)
    wb = w.float().reshape(*lead, N // B, B, K // B, B)
    amax = wb.abs().amax(dim=(-3, -1))                    # [..., N/B, K/B]
    # frexp: amax/448 = m · 2^e with m in [0.5, 1), so ceil(log2) is e, or
    # e − 1 at an exact power of two (m = 0.5); no log rounding involved
    m, e = torch.frexp(amax / FP8_E4M3_MAX)
    e = torch.where(m == 0.5, e - 1, e)
    scale = torch.where(amax > 0, torch.ldexp(torch.ones_like(amax), e),
                        torch.ones_like(amax))
    q = (wb / scale[..., :, None, :, None]).reshape(w.shape)
    return q.to(torch.float8_e4m3fn), scale


def dequantize_fp8_block(q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """f32 q.float() · scale with each scale expanded over its 128×128 block."""
    B = FP8_BLOCK
    s = scale.repeat_interleave(B, dim=-2).repeat_interleave(B, dim=-1)
    return q.float() * s


KV_FP8_MIN_EXP = -64   # smallest row-scale exponent of the fp8 KV cache


def quantize_kv_rows(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """Row-scaled e4m3 quantiser of the fp8 KV cache (kv_dtype="fp8"): the
    row form of quantize_fp8_block. x: bf16 or f32 [..., D]; it is rounded to
    bf16 first, as the cache writer sees bf16 rows. Returns (q, scale): q
    float8_e4m3fn of x's shape, scale f32 [...] with one entry per row. A
    row's scale is 2^e with e the smallest integer such that
    amax ≤ 448·2^e, clamped to e ≥ −64 (1.0 for an all-zero row), and q is
    the round-to-nearest-even e4m3 of x·2^−e. So |x/scale| ≤ 448, the cast
    never saturates, and every q·scale is exactly a bf16 value. Plain torch;
    runs on CPU and GPU."""
    if x.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError(f"quantize_kv_rows takes bf16 or f32, got {x.dtype}")
    xb = x.to(torch.bfloat16).float()
    amax = xb.abs().amax(dim=-1)
    # frexp: amax = m · 2^E with m in [0.5, 1) and 448 = 0.875 · 2^9, so the
    # exponent is E − 9, or E − 8 once m passes 0.875; no division, no log
    m, e = torch.frexp(amax)
    e = torch.where(m > 0.875, e - 8, e - 9).clamp_(min=KV_FP8_MIN_EXP)
    one = torch.ones_like(amax)
    scale = torch.where(amax > 0, torch.ldexp(one, e), one)
    q = xb / scale.unsqueeze(-1)      # a power of two: the division is exact
    return q.to(torch.float8_e4m3fn), scale


def dequantize_kv_rows(q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """f32 q.float() · scale with each row's scale over its D values. Every
    value is exactly representable in bf16 (quantize_kv_rows), so
    .to(bfloat16) of the result is the cache's bf16 image."""
    return q.float() * scale.unsqueeze(-1)


def vs_topk_ref(mat: torch.Tensor, query: torch.Tensor, k: int
                ) -> tuple[torch.Tensor, torch.Tensor]:
    scores = mat.float() @ query.float()
    v, i = scores.topk(k)
    return v, i


def vs_topk_scoped_ref(mat: torch.Tensor, tags: torch.Tensor,
                       queries: torch.Tensor, scopes: torch.Tensor, k: int
                       ) -> tuple[torch.Tensor, torch.Tensor]:
    """Scope rule: scope < 0 admits every row; scope s admits rows tagged s
    or 0 (global). Slots beyond the rows in scope hold -inf / -1."""
    scores = (mat.float() @ queries.float().T).T            # [Q, N]
    sc = scopes.view(-1, 1)
    tg = tags.view(1, -1)
    admit = (sc < 0) | (tg == 0) | (tg == sc)                # [Q, N]
    scores = scores.masked_fill(~admit, float("-inf"))
    kk = min(k, scores.size(1))
    v, i = scores.topk(kk, dim=1)
    i = i.masked_fill(v == float("-inf"), -1)
    if kk < k:
        pad = (scores.size(0), k - kk)
        v = torch.cat([v, v.new_full(pad, float("-inf"))], dim=1)
        i = torch.cat([i, i.new_full(pad, -1)], dim=1)
    return v, i


# ---- memory encoder (csrc/encoder.hip): fp32 math on the given values

def encoder_embed_ref(feats: torch.Tensor, pos_ids: torch.Tensor,
                      pos_table: torch.Tensor) -> torch.Tensor:
    """feats [R, 4] int32 of (index << 1) | plus; collisions accumulate. The
    ±0.5 sums are exact, so the result is one f32 add and one rounding."""
    R = feats.size(0)
    v = torch.zeros(R, pos_table.size(1), dtype=torch.float32,
                    device=feats.device)
    idx = (feats >> 1).long()
    sign = (feats & 1).float() - 0.5
    v.scatter_add_(1, idx, sign)
    return (v + pos_table.float()[pos_ids.long()]).to(torch.bfloat16)


def encoder_attention_ref(qkv: torch.Tensor, cu_rows: list[int],
                          heads: int = 12) -> torch.Tensor:
    """Bidirectional softmax attention per packed segment, fp32, on rows of
    q|k|v; returns fp32 [R, D]."""
    R, D = qkv.size(0), qkv.size(1) // 3
    hd = D // heads
    out = torch.empty(R, D, dtype=torch.float32, device=qkv.device)
    for lo, hi in zip(cu_rows, cu_rows[1:]):
        seg = qkv[lo:hi].float().view(hi - lo, 3, heads, hd)
        q, k, v = (seg[:, i].transpose(0, 1) for i in range(3))   # [H, T, hd]
        s = (q @ k.transpose(-1, -2)) * hd ** -0.5
        out[lo:hi] = (torch.softmax(s, dim=-1) @ v).transpose(0, 1).reshape(
            hi - lo, D)
    return out


def gelu_ref(u: torch.Tensor) -> torch.Tensor:
    return F.gelu(u.float()).to(torch.bfloat16)


def encoder_pool_ref(h: torch.Tensor, cu_rows: list[int], mu: torch.Tensor,
                     normalize: bool = True) -> torch.Tensor:
    rows = [h[lo:hi].float().mean(0) - mu.float()
            for lo, hi in zip(cu_rows, cu_rows[1:])]
    out = torch.stack(rows)
    return F.normalize(out, dim=-1) if normalize else out


RING = 256   # token-history ring entries per row


def ring_window_ref(ring: torch.Tensor, ring_len: int, last_n: int) -> list[int]:
    """Tokens of pushes max(0, len − n) … len − 1 of one row's ring, oldest
    first; push j lives at ring[j % 256]. n is capped at the ring size."""
    n = min(int(last_n), int(ring_len), RING)
    ring = ring.tolist()
    return [int(ring[j % RING]) for j in range(ring_len - n, ring_len)]


def apply_penalties_ref(logits: torch.Tensor, window: list[int], rep: float,
                        presence: float, freq: float) -> torch.Tensor:
    """llama.cpp/Ollama order on one row of raw logits: a token that occurs
    c ≥ 1 times in the window gets x = x/rep if x > 0 else x·rep, then
    x −= c·freq + presence. Tokens outside the vocabulary are ignored."""
    x = logits.float().clone()
    V = x.numel()
    counts: dict[int, int] = {}
    for t in window:
        if 0 <= t < V:
            counts[t] = counts.get(t, 0) + 1
    rep_t = torch.tensor(rep, dtype=torch.float32)
    for t, c in counts.items():
        v = x[t]
        v = v / rep_t if v > 0 else v * rep_t
        x[t] = v - torch.tensor(c * freq + presence, dtype=torch.float32)
    return x


def sample_dist_ref(logits: torch.Tensor, window: list[int], params: dict
                    ) -> torch.Tensor:
    """Exact final distribution [V] of one row: penalties → top-k →
    temperature softmax → smallest prefix (by descending probability) whose
    cumulative mass ≥ top_p, crossing token included → renormalise.
    params: temperature, top_p, top_k and optionally repetition_penalty /
    presence_penalty / frequency_penalty. temperature ≤ 1e-5 is greedy."""
    x = apply_penalties_ref(logits, window,
                            params.get("repetition_penalty", 1.0),
                            params.get("presence_penalty", 0.0),
                            params.get("frequency_penalty", 0.0)).double()
    out = torch.zeros_like(x)
    k = min(int(params["top_k"]), x.numel())
    v, i = x.topk(k)
    if params["temperature"] <= 1e-5:
        out[i[0]] = 1.0
        return out
    p = torch.softmax(v / params["temperature"], dim=-1)
    cum = p.cumsum(-1)
    cut = int((cum >= params["top_p"]).nonzero()[0]) + 1 \
        if bool((cum >= params["top_p"]).any()) else k
    out[i[:cut]] = p[:cut] / p[:cut].sum()
    return out
