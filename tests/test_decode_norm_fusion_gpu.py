"""The decode layer's two add + RMSNorm launches folded into their neighbours:
the O projection adds the residual in its epilogue (gemv_residual), the
router GEMV computes the post-attention norm itself (router_norm_gemv_topk),
and gemv_addnorm (input norm inside the QKV projection, wired in at B <= 2)
is rebuilt to match its unfused pair bit for bit at every B <= 8. All are
built to give the bits of the ops they replace, so every check here is
torch.equal against the composition of those ops on the same inputs.
GPU-only."""
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from room_amd import ops
from room_amd.engine.kv_cache import PagedKVCache
from room_amd.models.qwen3_moe import Qwen3MoEConfig, Qwen3MoEModel

DEV = torch.device("cuda", 0)
BF = dict(dtype=torch.bfloat16, device=DEV)


# ------------------------------------------- O GEMV with residual epilogue
@pytest.mark.parametrize("H,N", [(512, 64), (4096, 2048), (2048, 66)])
@pytest.mark.parametrize("B", [1, 5, 8])
def test_gemv_residual_matches_gemv_then_add(B, H, N):
    """H/512 = 1 (generic loop), 8 and 4 (hoisted loads); N = 66 ends inside
    the last workgroup. A guard row after the residual catches a store past
    row B."""
    torch.manual_seed(60 + B)
    a = torch.randn(B, H, **BF)
    w = torch.randn(N, H, **BF) * 0.05
    x0 = torch.randn(B, N, **BF)

    obuf = torch.empty(B, N, **BF)
    ops.gemv(obuf, a, w)
    # fused_add_rmsnorm takes rows of a multiple of 8 columns: pad with zero
    # columns (the add is per element, so columns < N get the same bits)
    NP = (N + 7) // 8 * 8
    res_pad = torch.zeros(B, NP, **BF)
    o_pad = torch.zeros(B, NP, **BF)
    res_pad[:, :N] = x0
    o_pad[:, :N] = obuf
    ops.fused_add_rmsnorm(torch.empty(B, NP, **BF), res_pad, o_pad,
                          torch.ones(NP, **BF), 1e-6)
    res_old = res_pad[:, :N]

    buf = torch.full((B + 1, N), 7.0, **BF)
    buf[:B] = x0
    ops.gemv_residual(buf[:B], a, w)
    assert torch.equal(buf[:B], res_old)
    assert (buf[B] == 7.0).all()
    assert not torch.equal(res_old, x0)         # the add did something


# ------------------------------------------------------- router with norm
def _router_case(T, E, H, K, seed, tie=False):
    torch.manual_seed(seed)
    r0 = torch.randn(T, H, **BF)
    delta = torch.randn(T, H, **BF) * 0.3
    gamma = 1 + 0.2 * torch.randn(H, **BF)
    wr = torch.randn(E, H, **BF) * 0.05
    if tie:
        # copies of the row that leads for token 0: bit-equal logits among
        # the leaders, in one lane's pair (2i, 2i+1) and across lanes
        h = torch.empty(T, H, **BF)
        ops.rmsnorm(h, r0, gamma, 1e-6)
        lead = int((h.float() @ wr.float().t())[0].argmax())
        copies = [c for c in (lead ^ 1, (lead + 37) % E)]
        wr[copies] = wr[lead].clone()
    return r0, delta, gamma, wr


@pytest.mark.parametrize("T,E,H,K,tie", [
    (5, 128, 2048, 8, False), (1, 16, 512, 4, False), (8, 128, 2048, 8, False),
    (3, 16, 4096, 4, False), (5, 128, 2048, 8, True)])
def test_router_norm_matches_norm_then_router(T, E, H, K, tie):
    """H = 2048 takes the kernel with every load hoisted, 512 and 4096 the
    generic loops (512: one emulated norm wave holds the whole row; 4096: two
    vectors per emulated thread). Reference: fused_add_rmsnorm (residual add
    and norm) then router_gemv_topk; the fused op gets the added residual."""
    r0, delta, gamma, wr = _router_case(T, E, H, K, 70 + T + H, tie)
    res = r0.clone()
    h_old = torch.empty(T, H, **BF)
    ops.fused_add_rmsnorm(h_old, res, delta, gamma, 1e-6)
    ids_old, w_old = ops.router_gemv_topk(h_old, wr, K)
    # rmsnorm of the added residual is the same normed row
    h_plain = torch.empty(T, H, **BF)
    ops.rmsnorm(h_plain, res, gamma, 1e-6)
    assert torch.equal(h_plain, h_old)

    hbuf = torch.full((T + 1, H), 7.0, **BF)
    res_in = res.clone()
    ids, w = ops.router_norm_gemv_topk(hbuf[:T], res_in, gamma, wr, K, 1e-6)
    assert torch.equal(res_in, res)             # input rows left alone
    assert torch.equal(hbuf[:T], h_old)
    assert (hbuf[T] == 7.0).all()
    assert torch.equal(ids, ids_old)
    assert torch.equal(w, w_old)
    if tie:
        # the tie is real: token 0's leaders include two bit-equal logits
        logits = h_old.float() @ wr.float().t()
        top = logits[0].topk(3).values
        assert (top[:-1] == top[1:]).any()


# ------------------------------------------------- add + norm + GEMV
@pytest.fixture(scope="module")
def addnorm_weights():
    """One W and γ per H, shared by every case (N = 1024; N = 20 is its first
    20 rows)."""
    torch.manual_seed(80)
    return {H: (torch.randn(1024, H, **BF) * 0.05,
                1 + 0.2 * torch.randn(H, **BF)) for H in (512, 2048, 4096)}


@pytest.mark.parametrize("H", [512, 2048, 4096])
@pytest.mark.parametrize("B", [1, 2, 3, 5, 8])
def test_gemv_addnorm_matches_norm_then_gemv(addnorm_weights, B, H):
    """N = 20 (ends inside a workgroup of 8 rows) and 1024, delta f32 / bf16 /
    none, bf16
    output (f32 at one point per case): x_out and y equal fused_add_rmsnorm
    (or rmsnorm) -> gemv, and a second call repeats the first bit for bit.
    H = 512 runs the generic loops (one norm wave holds the row), 2048 and
    4096 the hoisted ones (one and two vectors per unit lane)."""
    w_all, gamma = addnorm_weights[H]
    torch.manual_seed(81 + B)
    x = torch.randn(B, H, **BF)
    deltas = (torch.randn(B, H, dtype=torch.float32, device=DEV) * 0.3,
              torch.randn(B, H, **BF) * 0.3,
              torch.empty(0, dtype=torch.float32, device=DEV))
    for N in (20, 1024):
        w = w_all[:N]
        for delta in deltas:
            res = x.clone()
            h = torch.empty(B, H, **BF)
            if delta.numel():
                ops.fused_add_rmsnorm(h, res, delta, gamma, 1e-6)
            else:
                ops.rmsnorm(h, res, gamma, 1e-6)
            for dt in ((torch.bfloat16, torch.float32) if N == 20
                       else (torch.bfloat16,)):
                y_old = torch.empty(B, N, dtype=dt, device=DEV)
                ops.gemv(y_old, h, w)
                out = []
                for _ in range(2):
                    y = torch.full((B + 1, N), 7.0, dtype=dt, device=DEV)
                    x_out = torch.full((B + 1, H), 7.0, **BF)
                    xin = x.clone()
                    ops.gemv_addnorm(y[:B], xin, delta, x_out[:B], gamma, w,
                                     1e-6)
                    assert torch.equal(xin, x)
                    assert (y[B] == 7.0).all() and (x_out[B] == 7.0).all()
                    out.append((y[:B], x_out[:B]))
                tag = (B, H, N, str(delta.dtype), delta.numel() > 0, str(dt))
                assert torch.equal(out[0][0], y_old), tag
                assert torch.equal(out[0][0], out[1][0]), tag
                if delta.numel():
                    assert torch.equal(out[0][1], res), tag
                    assert torch.equal(out[1][1], res), tag
                else:                           # x_out is not written
                    assert (out[0][1] == 7.0).all(), tag


# ----------------------------------------------------- one decode layer
class _OldWiring(Qwen3MoEModel):
    """The decode layer as it was wired before the fusion, from the ops that
    remain: O GEMV -> fused_add_rmsnorm -> router_gemv_topk."""

    def _decode_layer(self, layer, kcache, vcache, st, x, x_alt, moe_out):
        cfg = self.cfg
        T = x.size(0)
        qdim = cfg.num_q_heads * cfg.head_dim
        hbuf, qkv = st.hbuf, st.qkv
        if moe_out is None:
            ops.rmsnorm(hbuf, x, layer.input_norm_w, cfg.rms_eps)
        else:
            ops.fused_add_rmsnorm(hbuf, x, moe_out, layer.input_norm_w,
                                  cfg.rms_eps)
        ops.gemv(qkv, hbuf, layer.wqkv)
        q = qkv[:, :qdim].view(T, cfg.num_q_heads, cfg.head_dim)
        ops.qk_rope_write_kv(qkv, cfg.num_q_heads, kcache, vcache,
                             layer.q_norm_w, layer.k_norm_w, self.cos_t,
                             self.sin_t, st.block_table, st.seq_ids, st.q_pos,
                             cfg.rms_eps)
        attn = torch.empty(T, cfg.num_q_heads, cfg.head_dim, **BF)
        ops.paged_attention_split(attn, q, kcache, vcache, st.block_table,
                                  st.seq_ids, st.q_pos, st.part, st.part_ml,
                                  self.scale, splits=self.attn_splits)
        obuf = torch.empty(T, cfg.hidden_size, **BF)
        ops.gemv(obuf, attn.reshape(T, qdim), layer.wo)
        ops.fused_add_rmsnorm(hbuf, x, obuf, layer.post_attn_norm_w,
                              cfg.rms_eps)
        topk_ids, topk_w = ops.router_gemv_topk(hbuf, layer.router_w,
                                                cfg.num_experts_per_tok)
        return x, x_alt, self._moe(hbuf, layer, topk_ids, topk_w, st)


class _Rec:
    """Keeps what a decode layer hands to its MoE (normed rows, expert ids
    and weights) and the residual it returns: everything the fusion touches,
    all of it upstream of the MoE's float atomics."""

    def _decode_layer(self, layer, kcache, vcache, st, x, x_alt, moe_out):
        out = super()._decode_layer(layer, kcache, vcache, st, x, x_alt,
                                    moe_out)
        self.seen["residual"] = out[0].clone()
        return out

    def _moe(self, hbuf, layer, topk_ids, topk_w, st):
        self.seen = dict(hbuf=hbuf.clone(), ids=topk_ids.clone(),
                         w=topk_w.clone())
        return super()._moe(hbuf, layer, topk_ids, topk_w, st)


class _RecNew(_Rec, Qwen3MoEModel):
    pass


class _RecOld(_Rec, _OldWiring):
    pass


def test_decode_layer_logits_match_old_wiring():
    """One decode layer of the tiny config at T = 5 (the unfused input-norm
    branch): logits of the new wiring equal the old wiring's bit for bit.
    Rows decode at positions 0, 3, 17, 30, 31 over a cache filled by the same
    calls. First the layer's state before the MoE (residual, normed rows,
    expert ids and weights), which is all the fusion touches and is
    deterministic, then the logits."""
    cfg = dataclasses.replace(Qwen3MoEConfig.tiny(), num_layers=1)
    new = _RecNew(cfg, DEV, seed=11)
    old = _RecOld(cfg, DEV, seed=11)
    assert torch.equal(new.layers[0].wo, old.layers[0].wo)
    # norm weights off one, so that γ takes part
    g = torch.Generator(device=DEV).manual_seed(5)
    for name in ("input_norm_w", "post_attn_norm_w"):
        v = 1 + 0.2 * torch.randn(cfg.hidden_size, generator=g, device=DEV)
        setattr(new.layers[0], name, v.to(torch.bfloat16))
        setattr(old.layers[0], name, v.to(torch.bfloat16))

    T, lens = 5, [0, 3, 17, 30, 31]
    i32 = dict(dtype=torch.int32, device=DEV)
    tok = torch.randint(0, cfg.vocab_size, (T,),
                        generator=torch.Generator().manual_seed(6)).to(DEV)
    seq_t = torch.arange(T, **i32)
    pos_t = torch.tensor(lens, **i32)
    logits = []
    for model in (old, new):
        cache = PagedKVCache(cfg.num_layers, cfg.num_kv_heads, cfg.head_dim,
                             T * 4 + 1, T, cfg.max_position // 16, DEV)
        kg = torch.Generator(device=DEV).manual_seed(8)
        for c in cache.kcaches + cache.vcaches:
            c.copy_(torch.randn(c.shape, generator=kg, device=DEV).to(c.dtype))
        for s, n in enumerate(lens):
            assert cache.alloc_seq() == s
            cache.ensure_capacity(s, n + 1)
        logits.append(model.forward(tok, seq_t, pos_t, cache.block_table,
                                    cache.kcaches, cache.vcaches))
    assert sorted(old.seen) == ["hbuf", "ids", "residual", "w"]
    for name in old.seen:
        assert torch.equal(old.seen[name], new.seen[name]), name
    assert torch.isfinite(logits[0]).all()
    assert torch.equal(logits[0], logits[1]), (
        "the layer's state before the MoE is bit-equal (checked above), so "
        "this difference comes from moe_gemv_down: it sums each output's four "
        "expert terms with f32 atomics in no fixed order, and a last-bit "
        "difference survives the bf16 rounding with the residual only within "
        "2^-16 of a rounding boundary")
