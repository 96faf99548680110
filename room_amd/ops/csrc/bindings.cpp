// Python bindings for room_amd._C — the CDNA4 kernel library.
#include <torch/extension.h>
#include "checks.h"

void rmsnorm(torch::Tensor out, torch::Tensor in, torch::Tensor weight, double eps);
void fused_add_rmsnorm(torch::Tensor out, torch::Tensor residual, torch::Tensor in,
                       torch::Tensor weight, double eps);
void qk_norm_rope(torch::Tensor q, torch::Tensor k, torch::Tensor q_w,
                  torch::Tensor k_w, torch::Tensor cos_t, torch::Tensor sin_t,
                  torch::Tensor positions, int64_t n_qheads, int64_t n_kvheads,
                  int64_t head_dim, double eps);
void qk_rope_write_kv(torch::Tensor qkv, torch::Tensor kcache,
                      torch::Tensor vcache, torch::Tensor q_w, torch::Tensor k_w,
                      torch::Tensor cos_t, torch::Tensor sin_t,
                      torch::Tensor block_table, torch::Tensor seq_ids,
                      torch::Tensor positions, int64_t n_qheads, double eps,
                      c10::optional<torch::Tensor> k_scale,
                      c10::optional<torch::Tensor> v_scale);
void silu_mul(torch::Tensor out, torch::Tensor gateup);
void paged_attention(torch::Tensor out, torch::Tensor q, torch::Tensor kcache,
                     torch::Tensor vcache, torch::Tensor block_table,
                     torch::Tensor seq_ids, torch::Tensor q_pos, double scale,
                     c10::optional<torch::Tensor> k_scale,
                     c10::optional<torch::Tensor> v_scale);
void write_kv(torch::Tensor kcache, torch::Tensor vcache, torch::Tensor k,
              torch::Tensor v, torch::Tensor block_table, torch::Tensor seq_ids,
              torch::Tensor q_pos);
void moe_router(torch::Tensor topk_ids, torch::Tensor topk_w, torch::Tensor logits,
                int64_t K);
void router_gemv_topk(torch::Tensor topk_ids, torch::Tensor topk_w,
                      torch::Tensor x, torch::Tensor wr, int64_t K);
void router_norm_gemv_topk(torch::Tensor topk_ids, torch::Tensor topk_w,
                           torch::Tensor hbuf, torch::Tensor r,
                           torch::Tensor gamma, torch::Tensor wr, int64_t K,
                           double eps);
void moe_gemv_h(torch::Tensor h, torch::Tensor x, torch::Tensor w13,
                torch::Tensor pair_token, torch::Tensor pair_expert,
                torch::Tensor out_zero);
void moe_gemv_down(torch::Tensor out, torch::Tensor h, torch::Tensor w2,
                   torch::Tensor pair_w, torch::Tensor pair_token,
                   torch::Tensor pair_expert);
void moe_grouped_gemm128(torch::Tensor out, torch::Tensor x, torch::Tensor w,
                         torch::Tensor pair_token, torch::Tensor tile_desc);
void moe_build_desc(torch::Tensor desc, torch::Tensor counts, int64_t bm);
void skinny_gemm(torch::Tensor y, torch::Tensor x, torch::Tensor w);
void moe_grouped_gemm_skinny(torch::Tensor out, torch::Tensor x,
                             torch::Tensor w, torch::Tensor pair_token,
                             torch::Tensor tile_desc);
void moe_combine_gather(torch::Tensor out, torch::Tensor z, torch::Tensor topk_w,
                        torch::Tensor inv_order);
void moe_gemv_h_fp8(torch::Tensor h, torch::Tensor x, torch::Tensor w13_q,
                    torch::Tensor w13_s, torch::Tensor pair_token,
                    torch::Tensor pair_expert, torch::Tensor out_zero);
void moe_gemv_down_fp8(torch::Tensor out, torch::Tensor h, torch::Tensor w2_q,
                       torch::Tensor w2_s, torch::Tensor pair_w,
                       torch::Tensor pair_token, torch::Tensor pair_expert);
void moe_grouped_gemm_skinny_fp8(torch::Tensor out, torch::Tensor x,
                                 torch::Tensor w_q, torch::Tensor w_s,
                                 torch::Tensor pair_token,
                                 torch::Tensor tile_desc);
void moe_grouped_gemm128_fp8(torch::Tensor out, torch::Tensor x,
                             torch::Tensor w_q, torch::Tensor w_s,
                             torch::Tensor pair_token,
                             torch::Tensor tile_desc);
void paged_attention_split(torch::Tensor out, torch::Tensor q,
                           torch::Tensor kcache, torch::Tensor vcache,
                           torch::Tensor block_table, torch::Tensor seq_ids,
                           torch::Tensor q_pos, torch::Tensor part,
                           torch::Tensor part_ml, double scale,
                           int64_t splits,
                           c10::optional<torch::Tensor> k_scale,
                           c10::optional<torch::Tensor> v_scale);
int64_t attn_nsplits();
int64_t flash_prefill_qtile();
void flash_prefill(torch::Tensor out, torch::Tensor q, torch::Tensor kcache,
                   torch::Tensor vcache, torch::Tensor block_table,
                   torch::Tensor seq_ids, torch::Tensor q_pos,
                   torch::Tensor tile_desc, double scale,
                   c10::optional<torch::Tensor> k_scale,
                   c10::optional<torch::Tensor> v_scale);
void gemv(torch::Tensor y, torch::Tensor x, torch::Tensor w);
void gemv_residual(torch::Tensor r, torch::Tensor x, torch::Tensor w);
void gemv_addnorm(torch::Tensor y, torch::Tensor x, torch::Tensor delta,
                  torch::Tensor x_out, torch::Tensor gamma, torch::Tensor w,
                  double eps);
void sample_rows(torch::Tensor out_tokens, torch::Tensor logits,
                 torch::Tensor temperature, torch::Tensor top_p,
                 torch::Tensor top_k, torch::Tensor seeds, torch::Tensor ctr,
                 torch::Tensor repetition_penalty,
                 torch::Tensor presence_penalty,
                 torch::Tensor frequency_penalty, torch::Tensor repeat_last_n,
                 torch::Tensor ring, torch::Tensor ring_len, bool append);
void hist_append(torch::Tensor hist, torch::Tensor ctr, torch::Tensor toks,
                 int64_t kmax);
void vs_topk(torch::Tensor out_v, torch::Tensor out_i, torch::Tensor cand_v,
             torch::Tensor cand_i, torch::Tensor mat, torch::Tensor query,
             int64_t K);
void vs_topk_scoped(torch::Tensor out_v, torch::Tensor out_i,
                    torch::Tensor cand_v, torch::Tensor cand_i,
                    torch::Tensor mat, torch::Tensor tags,
                    torch::Tensor queries, torch::Tensor scopes, int64_t K);
void encoder_embed(torch::Tensor x, torch::Tensor feats, torch::Tensor pos_ids,
                   torch::Tensor pos_table);
void encoder_attention(torch::Tensor out, torch::Tensor qkv,
                       torch::Tensor cu_rows);
void gelu_(torch::Tensor u);
void encoder_pool(torch::Tensor out, torch::Tensor h, torch::Tensor cu_rows,
                  torch::Tensor mu, bool normalize);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("set_check_only", &set_check_only,
        "process-wide: every op returns after its argument checks, before its "
        "launch (for testing the checks); off by default");
  m.def("check_only", &check_only, "whether check-only mode is on");
  m.def("rmsnorm", &rmsnorm, "RMSNorm (bf16, CDNA4)");
  m.def("fused_add_rmsnorm", &fused_add_rmsnorm, "residual += x; rmsnorm(residual)");
  m.def("qk_norm_rope", &qk_norm_rope, "fused per-head QK RMSNorm + RoPE");
  m.def("qk_rope_write_kv", &qk_rope_write_kv,
        "fused QK-norm + RoPE + paged KV write");
  m.def("silu_mul", &silu_mul, "silu(gate) * up");
  m.def("paged_attention", &paged_attention, "paged causal attention (GQA 8:1)");
  m.def("write_kv", &write_kv, "scatter K/V rows into paged cache");
  m.def("moe_router", &moe_router, "softmax top-k router");
  m.def("router_gemv_topk", &router_gemv_topk,
        "H-split router GEMV + top-k (two kernels, wide grid)");
  m.def("router_norm_gemv_topk", &router_norm_gemv_topk,
        "RMSNorm + H-split router GEMV + top-k; also stores the normed rows");
  m.def("moe_gemv_h", &moe_gemv_h, "MoE gate/up GEMV + silu-mul (decode)");
  m.def("moe_gemv_down", &moe_gemv_down, "MoE down GEMV + weighted scatter-add");
  m.def("moe_grouped_gemm128", &moe_grouped_gemm128, "BM=128 grouped MFMA GEMM");
  m.def("moe_build_desc", &moe_build_desc, "device-side tile desc builder",
        pybind11::arg("desc"), pybind11::arg("counts"),
        pybind11::arg("bm") = 128);
  m.def("skinny_gemm", &skinny_gemm,
        "dense MFMA GEMM for 1..64 rows (wide decode projections)");
  m.def("moe_grouped_gemm_skinny", &moe_grouped_gemm_skinny,
        "BM=16 grouped MFMA GEMM, weights straight to VGPRs (wide decode)");
  m.def("moe_combine_gather", &moe_combine_gather, "atomics-free MoE combine");
  m.def("moe_gemv_h_fp8", &moe_gemv_h_fp8,
        "MoE gate/up GEMV + silu-mul, block-scaled e4m3 weights (decode)");
  m.def("moe_gemv_down_fp8", &moe_gemv_down_fp8,
        "MoE down GEMV + weighted scatter-add, block-scaled e4m3 weights");
  m.def("moe_grouped_gemm_skinny_fp8", &moe_grouped_gemm_skinny_fp8,
        "BM=16 grouped MFMA GEMM, block-scaled e4m3 weights (wide decode)");
  m.def("moe_grouped_gemm128_fp8", &moe_grouped_gemm128_fp8,
        "BM=128 grouped MFMA GEMM, block-scaled e4m3 weights (prefill)");
  m.def("attn_nsplits", &attn_nsplits, "NSPLITS constant");
  m.def("paged_attention_split", &paged_attention_split,
        "split-KV flash-decode paged attention");
  m.def("flash_prefill", &flash_prefill, "MFMA flash-attention prefill");
  m.def("flash_prefill_qtile", &flash_prefill_qtile, "q-tile rows constant");
  m.def("gemv", &gemv, "dense skinny-batch GEMV (decode projections)");
  m.def("gemv_residual", &gemv_residual,
        "r += bf16(x @ w^T) in place (decode O projection + residual add)");
  m.def("gemv_addnorm", &gemv_addnorm,
        "fused residual-add + RMSNorm + GEMV (decode)");
  m.def("sample_rows", &sample_rows,
        "two-stage sampler, per-row parameters, penalties and seeded draws");
  m.def("hist_append", &hist_append, "token-history append (multi-step decode)");
  m.def("vs_topk", &vs_topk, "vector-store cosine top-k over bf16 matrix");
  m.def("vs_topk_scoped", &vs_topk_scoped,
        "room-scoped cosine top-k for a batch of up to 8 queries");
  m.def("encoder_embed", &encoder_embed,
        "memory encoder input rows: hash features + position row");
  m.def("encoder_attention", &encoder_attention,
        "bidirectional MFMA attention over packed segments (head dim 32)");
  m.def("gelu_", &gelu_, "exact (erf) GELU in place (bf16)");
  m.def("encoder_pool", &encoder_pool,
        "segment mean, centring and L2 normalisation");
}
