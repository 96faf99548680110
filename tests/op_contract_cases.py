"""Minimal valid arguments for every op of room_amd._C, shared by
test_op_contracts.py (check-only mode, any host) and test_op_contracts_gpu.py
(real launches).

A case is the op's positional argument list as (name, value) pairs in the
order of its C++ signature. A tensor argument is an `A` (dtype, shape, which
of its sizes the wrapper checks against this tensor, optional contents); any
other value is passed as it is. Shapes are the smallest the contracts admit:
T = 2 tokens, Hq = 8, Hk = 1, head dim 128, NB = 4 cache blocks of 16,
H = 512, E = 16, K = 4, I = 128, V = 4096, N = 64; the fp8-weight ops use
N = K = 128. Index tensors hold valid contents (the wrappers cannot check
those), so the same arguments can be launched.
"""
import torch

BF, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
I32, I64, FP8 = torch.int32, torch.int64, torch.float8_e4m3fn

T, HQ, HK, D, NB, BS = 2, 8, 1, 128, 4, 16
H, E, K, I, V, N = 512, 16, 4, 128, 4096, 64
P = T * K                    # (token, expert) pairs
F8N = 128                    # N = K of the fp8-weight ops
ENC, R = 384, 2              # encoder width, packed rows
NSPLITS = 64                 # attn_nsplits()


class A:
    """One tensor argument. dims: the dimensions whose size this wrapper
    checks against this tensor, as d (mutated by +1) or (d, delta); None =
    all of them. A size that only other arguments are measured against (the
    token count read off `positions`, say) is not listed: growing it makes
    those arguments wrong, not this one. rank=False: the op takes any rank."""

    def __init__(self, dtype, *shape, dims=None, value=None, rank=True):
        self.dtype, self.shape, self.value, self.rank = dtype, shape, value, rank
        dims = range(len(shape)) if dims is None else dims
        self.dims = [d if isinstance(d, tuple) else (d, 1) for d in dims]

    def make(self, dev, dtype=None, shape=None):
        """The argument on dev: its listed contents, else ones (f32) or
        zeros. A mutated shape drops the contents."""
        if self.value is not None and shape is None:
            t = torch.tensor(self.value, dtype=torch.float64)
        else:
            fill = torch.ones if self.dtype is F32 else torch.zeros
            t = fill(self.shape if shape is None else tuple(shape))
        return t.to(dtype or self.dtype).to(dev)


def _kv(fp8):
    dt = FP8 if fp8 else BF
    caches = [("kcache", A(dt, NB, HK, BS, D, dims=(2, 3))),
              ("vcache", A(dt, NB, HK, BS, D))]
    scales = ([("k_scale", A(F32, NB, HK, BS)), ("v_scale", A(F32, NB, HK, BS))]
              if fp8 else [("k_scale", None), ("v_scale", None)])
    return caches, scales


def _paging(pos_name, pos_dims=None):
    return [("block_table", A(I32, 1, NB, dims=())),
            ("seq_ids", A(I32, T)),
            (pos_name, A(I32, T, dims=pos_dims, value=[3, 20]))]


def _attention(fp8, extra, tail):
    caches, scales = _kv(fp8)
    return ([("out", A(BF, T, HQ, D)), ("q", A(BF, T, HQ, D, dims=(1, 2)))]
            + caches + _paging("q_pos") + extra + tail + scales)


def _qk_rope_write_kv(fp8):
    caches, scales = _kv(fp8)
    return ([("qkv", A(BF, T, (HQ + 2 * HK) * D))] + caches
            + [("q_w", A(BF, D)), ("k_w", A(BF, D)),
               ("cos_t", A(F32, 64, D // 2, dims=(1,))),
               ("sin_t", A(F32, 64, D // 2))]
            + _paging("positions", pos_dims=())
            + [("n_qheads", HQ), ("eps", 1e-6)] + scales)


_SPLIT = [("part", A(F32, T, HQ, NSPLITS, D, dims=((0, -1), 1, 2, 3))),
          ("part_ml", A(F32, T, HQ, NSPLITS, 2, dims=((0, -1), 1, 2, 3)))]
_PAIRS = [("pair_token", A(I32, P)), ("pair_expert", A(I32, P))]
_DESC = ("tile_desc", A(I32, 1, 3, dims=(1,), value=[[0, 0, P]]))


def _norm(f32_in=False):
    return [("out", A(BF, T, H)), ("residual", A(BF, T, H)),
            ("in", A(F32 if f32_in else BF, T, H, dims=(1,))),
            ("weight", A(BF, H)), ("eps", 1e-6)]


def _gemv(y):
    return [(y, A(BF, T, N)), ("x", A(BF, T, H, dims=(1,))),
            ("w", A(BF, N, H, dims=(1,)))]


def _addnorm(delta):
    return [("y", A(BF, T, N)), ("x", A(BF, T, H, dims=(1,))),
            ("delta", delta), ("x_out", A(BF, T, H)), ("gamma", A(BF, H)),
            ("w", A(BF, N, H, dims=(1,))), ("eps", 1e-6)]


def _grouped(n, k, weights):
    return ([("out", A(BF, P, n, dims=(1,))), ("x", A(BF, T, k, dims=(1,)))]
            + weights + [("pair_token", A(I32, P)), _DESC])


def _fp8_w(q, s, n, k):
    return [(q, A(FP8, E, n, k, dims=(1, 2))), (s, A(F32, E, n // 128, k // 128))]


def _router_out():
    return [("topk_ids", A(I32, T, K)), ("topk_w", A(F32, T, K))]


def _vec(name, dtype, value=None):
    return (name, A(dtype, T, value=value))


CASES = {
    "rmsnorm": [a for a in _norm() if a[0] != "residual"],
    "fused_add_rmsnorm": _norm(),
    "fused_add_rmsnorm/f32": _norm(f32_in=True),
    "qk_norm_rope": [
        ("q", A(BF, T, HQ, D)), ("k", A(BF, T, HK, D)), ("q_w", A(BF, D)),
        ("k_w", A(BF, D)), ("cos_t", A(F32, 64, D // 2, dims=(1,))),
        ("sin_t", A(F32, 64, D // 2)),
        ("positions", A(I32, T, dims=(), value=[3, 20])),
        ("n_qheads", HQ), ("n_kvheads", HK), ("head_dim", D), ("eps", 1e-6)],
    "qk_rope_write_kv": _qk_rope_write_kv(False),
    "qk_rope_write_kv/fp8kv": _qk_rope_write_kv(True),
    "silu_mul": [("out", A(BF, T, I)), ("gateup", A(BF, T, 2 * I, dims=(1,)))],
    "paged_attention": _attention(False, [], [("scale", D ** -0.5)]),
    "paged_attention/fp8kv": _attention(True, [], [("scale", D ** -0.5)]),
    "write_kv": (_kv(False)[0]
                 + [("k", A(BF, T, HK, D, dims=(1, 2))), ("v", A(BF, T, HK, D))]
                 + _paging("q_pos")),
    "moe_router": _router_out() + [("logits", A(F32, T, E, dims=())), ("K", K)],
    "router_gemv_topk": _router_out() + [
        ("x", A(BF, T, H, dims=(1,))), ("wr", A(BF, E, H, dims=(1,))), ("K", K)],
    "router_norm_gemv_topk": _router_out() + [
        ("hbuf", A(BF, T, H)), ("r", A(BF, T, H, dims=(1,))),
        ("gamma", A(BF, H)), ("wr", A(BF, E, H, dims=(1,))), ("K", K),
        ("eps", 1e-6)],
    "moe_gemv_h": [
        ("h", A(BF, P, I, dims=())), ("x", A(BF, T, H, dims=(1,))),
        ("w13", A(BF, E, 2 * I, H, dims=(1, 2)))] + _PAIRS + [
        ("out_zero", A(F32, T, H, dims=(), rank=False))],
    "moe_gemv_down": [
        ("out", A(F32, T, H, dims=())), ("h", A(BF, P, I, dims=(1,))),
        ("w2", A(BF, E, H, I, dims=(1, 2))), ("pair_w", A(F32, P))] + _PAIRS,
    "moe_grouped_gemm128": _grouped(N, H, [("w", A(BF, E, N, H, dims=(1, 2)))]),
    "moe_build_desc": [
        ("desc", A(I32, E + 1, 3, dims=(1,))),
        ("counts", A(I64, E, dims=(), value=[P] + [0] * (E - 1))), ("bm", 128)],
    "skinny_gemm": [("y", A(BF, T, N)), ("x", A(BF, T, H, dims=(1,))),
                    ("w", A(BF, N, H))],
    "moe_grouped_gemm_skinny": _grouped(
        N, H, [("w", A(BF, E, N, H, dims=(1, 2)))]),
    "moe_combine_gather": [
        ("out", A(BF, T, H, dims=(1,))), ("z", A(BF, P, H, dims=(1,))),
        ("topk_w", A(F32, T, K, dims=(0,))),
        ("inv_order", A(I32, P, value=list(range(P))))],
    "moe_gemv_h_fp8": [
        ("h", A(BF, P, I, dims=(1,))), ("x", A(BF, T, F8N, dims=(1,)))]
        + _fp8_w("w13_q", "w13_s", 2 * I, F8N) + _PAIRS + [
        ("out_zero", A(F32, T, F8N, dims=(), rank=False))],
    "moe_gemv_down_fp8": [
        ("out", A(F32, T, F8N, dims=(1,))), ("h", A(BF, P, I, dims=(1,)))]
        + _fp8_w("w2_q", "w2_s", F8N, I) + [("pair_w", A(F32, P))] + _PAIRS,
    "moe_grouped_gemm_skinny_fp8": _grouped(
        F8N, F8N, _fp8_w("w_q", "w_s", F8N, F8N)),
    "moe_grouped_gemm128_fp8": _grouped(
        F8N, F8N, _fp8_w("w_q", "w_s", F8N, F8N)),
    "paged_attention_split": _attention(
        False, _SPLIT, [("scale", D ** -0.5), ("splits", 32)]),
    "paged_attention_split/fp8kv": _attention(
        True, _SPLIT, [("scale", D ** -0.5), ("splits", 64)]),
    "flash_prefill": _attention(
        False, [("tile_desc", A(I32, 1, 2, dims=(1,), value=[[0, T]]))],
        [("scale", D ** -0.5)]),
    "flash_prefill/fp8kv": _attention(
        True, [("tile_desc", A(I32, 1, 2, dims=(1,), value=[[0, T]]))],
        [("scale", D ** -0.5)]),
    "gemv": _gemv("y"),
    "gemv_residual": _gemv("r"),
    # delta with no element: a plain norm + gemv, delta itself is not read
    "gemv_addnorm": _addnorm(lambda dev: torch.empty(0, device=dev)),
    "gemv_addnorm/delta": _addnorm(A(F32, T, H)),
    "sample_rows": [
        _vec("out_tokens", I32), ("logits", A(F32, T, V, dims=())),
        _vec("temperature", F32), _vec("top_p", F32), _vec("top_k", I32, [1, 4]),
        _vec("seeds", I64), _vec("ctr", I32), _vec("repetition_penalty", F32),
        _vec("presence_penalty", F32), _vec("frequency_penalty", F32),
        _vec("repeat_last_n", I32), ("ring", A(I32, T, 256)),
        _vec("ring_len", I32), ("append", True)],
    "hist_append": [("hist", A(I32, 2 * T)), ("ctr", A(I32, 1)),
                    ("toks", A(I32, T, dims=())), ("kmax", 2)],
    "vs_topk": [
        ("out_v", A(F32, K)), ("out_i", A(I64, K)),
        ("cand_v", A(F32, 2, K, dims=(1,))), ("cand_i", A(I32, 2, K)),
        ("mat", A(BF, N, ENC, dims=(1,))), ("query", A(F32, ENC)), ("K", K)],
    "vs_topk_scoped": [
        ("out_v", A(F32, T, K)), ("out_i", A(I64, T, K)),
        ("cand_v", A(F32, T, 2, K, dims=(0, 2))), ("cand_i", A(I32, T, 2, K)),
        ("mat", A(BF, N, ENC, dims=(1,))), ("tags", A(I32, N)),
        ("queries", A(F32, T, ENC, dims=(1,))),
        ("scopes", A(I32, T, value=[-1, 0])), ("K", K)],
    "encoder_embed": [
        ("x", A(BF, R, ENC, dims=(1,))), ("feats", A(I32, R, 4)),
        ("pos_ids", A(I32, R)), ("pos_table", A(F32, 4, ENC, dims=(1,)))],
    "encoder_attention": [
        ("out", A(BF, R, ENC)), ("qkv", A(BF, R, 3 * ENC, dims=(1,))),
        ("cu_rows", A(I32, 2, dims=((0, -1),), value=[0, R]))],
    "gelu_": [("u", A(BF, T, 8, dims=(1,), rank=False))],
    "encoder_pool": [
        ("out", A(F32, 1, ENC)), ("h", A(BF, R, ENC, dims=(1,))),
        ("cu_rows", A(I32, 2, dims=((0, -1),), value=[0, R])),
        ("mu", A(F32, ENC)),
        ("normalize", True)],
}

# what bindings.cpp binds besides the ops
NOT_OPS = {"attn_nsplits", "flash_prefill_qtile", "set_check_only", "check_only"}


def op_of(case: str) -> str:
    return case.split("/")[0]


def build(case: str, dev) -> list:
    """The case's positional arguments on dev."""
    return [v.make(dev) if isinstance(v, A) else v(dev) if callable(v) else v
            for _, v in CASES[case]]
