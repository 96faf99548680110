// Mixture-of-Experts kernels for Qwen3-30B-A3B on CDNA4 (gfx950).
//   E=128 experts, top-8, hidden H=2048, expert intermediate I=768.
//
// Weight layouts (we own them):
//   W13: [E, 2*I, H]  — gate rows [0,I), up rows [I,2I); each row contiguous
//                       over H (GEMV-friendly streaming, MFMA B-operand rows)
//   W2:  [E, H, I]    — down-proj rows contiguous over I
//
// Decode path (few tokens): wave-per-output GEMV — each (token,expert) pair
//   is bandwidth-bound on expert weights; 64-lane dot with 16 B/lane loads.
// Prefill path (many tokens): grouped MFMA GEMM (16x16x32 bf16) with LDS
//   tiles and +16B row padding against bank conflicts; tokens pre-sorted by
//   expert, tile descriptors built on the device.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include "common.h"
#include "checks.h"

// ---------------------------------------------------------------- router
// softmax over E<=128 logits, pick top-K<=8, renormalize their probs.
// one wave per token; lane l owns logits[2l], [2l+1] (-inf past E).
// Two selections with the same result (descending value, lowest index first
// among equals): router_select below for the decode router, where a handful
// of waves wait on each other's shuffles and latency is everything, and the
// K-round tournament in moe_router_kernel for prefill, where thousands of
// tokens keep the CUs full and the tournament's lower instruction count wins
// (rank counting measured 8.4 -> 12.1 us per prefill call).
//
// Selection by rank counting: the 128 logits go through LDS to every lane, and
// a lane counts for each of its two logits how many logits beat it (greater,
// or equal with a lower index). The ranks are a permutation of 0..127, so the
// logit of rank r < K is the winner of slot r: descending value, lowest index
// first among equals. One pass of independent compares replaces K rounds of
// two dependent 6-shuffle tournaments.
// The first pass counts strictly greater logits only (a compare and an
// add-with-carry each). Equal logits share such a count, so if no two logits
// claim the same slot below K the counts are the ranks; otherwise (bit-equal
// logits among the leaders, rare) a second pass applies the index rule.
DEV void router_select(int* __restrict__ topk_ids, float* __restrict__ topk_w,
                       float l0, float l1, int t, int lane, int K) {
  __shared__ float lg[2 * WAVE];
  __shared__ float slot_p[8];

  const float m = wave_reduce_max(fmaxf(l0, l1));
  const float denom = wave_reduce_sum(__expf(l0 - m) + __expf(l1 - m));

  lg[2 * lane] = l0;
  lg[2 * lane + 1] = l1;
  __syncthreads();
  int r0 = 0, r1 = 0;
  #pragma unroll
  for (int jl = 0; jl < WAVE; ++jl) {
    const float a = lg[2 * jl], b = lg[2 * jl + 1];   // indices 2jl, 2jl+1
    r0 += (int)(a > l0) + (int)(b > l0);
    r1 += (int)(a > l1) + (int)(b > l1);
  }
  bool shared_slot = false;   // wave-uniform
  for (int k = 0; k < K; ++k)
    shared_slot |= __popcll(__ballot(r0 == k)) + __popcll(__ballot(r1 == k)) > 1;
  if (shared_slot) {
    r0 = 0; r1 = 0;
    #pragma unroll 8
    for (int jl = 0; jl < WAVE; ++jl) {
      const float a = lg[2 * jl], b = lg[2 * jl + 1];
      const bool lt = jl < lane, le = jl <= lane;
      r0 += (int)(a > l0 || (a == l0 && lt)) + (int)(b > l0 || (b == l0 && lt));
      r1 += (int)(a > l1 || (a == l1 && le)) + (int)(b > l1 || (b == l1 && lt));
    }
  }
  const float p0 = __expf(l0 - m) / denom, p1 = __expf(l1 - m) / denom;
  if (r0 < K) slot_p[r0] = p0;
  if (r1 < K) slot_p[r1] = p1;
  __syncthreads();
  float picked_sum = 0.f;   // slot order, as the serial selection summed it
  for (int k = 0; k < K; ++k) picked_sum += slot_p[k];
  // Qwen3 norm_topk_prob; each slot has exactly one writer
  if (r0 < K) {
    topk_ids[(long)t * K + r0] = 2 * lane;
    topk_w[(long)t * K + r0] = p0 / picked_sum;
  }
  if (r1 < K) {
    topk_ids[(long)t * K + r1] = 2 * lane + 1;
    topk_w[(long)t * K + r1] = p1 / picked_sum;
  }
}

// prefill router: K-round shuffle tournament (see above)
__global__ void moe_router_kernel(int* __restrict__ topk_ids,      // [T, K]
                                  float* __restrict__ topk_w,      // [T, K]
                                  const float* __restrict__ logits,  // [T, E]
                                  int E, int K) {
  const int t = blockIdx.x;
  const int lane = threadIdx.x;
  const float l0 = (2 * lane < E) ? logits[(long)t * E + 2 * lane] : -INFINITY;
  const float l1 = (2 * lane + 1 < E) ? logits[(long)t * E + 2 * lane + 1] : -INFINITY;

  float m = wave_reduce_max(fmaxf(l0, l1));
  float e0 = __expf(l0 - m), e1 = __expf(l1 - m);
  float denom = wave_reduce_sum(e0 + e1);

  // iterative top-K selection by masking (K ≤ 8)
  float v0 = l0, v1 = l1;
  float picked_sum = 0.f;
  float probs[8];
  int winners[8];
  for (int k = 0; k < K; ++k) {
    float best = fmaxf(v0, v1);
    float gmax = wave_reduce_max(best);
    // first lane holding gmax wins; prefer slot 0
    int cand_id = (v0 == gmax) ? 2 * lane : ((v1 == gmax) ? 2 * lane + 1 : INT_MAX);
    int winner = cand_id;
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1)
      winner = min(winner, __shfl_xor(winner, off, WAVE));
    float prob = __expf(gmax - m) / denom;
    probs[k] = prob;       // every lane tracks the same values
    winners[k] = winner;
    picked_sum += prob;
    if (winner == 2 * lane) v0 = -INFINITY;
    if (winner == 2 * lane + 1) v1 = -INFINITY;
  }
  // lane 0 writes ids + renormalized weights (Qwen3 norm_topk_prob) — single
  // writer, no cross-lane visibility assumptions on global memory
  if (lane == 0) {
    for (int k = 0; k < K; ++k) {
      topk_ids[(long)t * K + k] = winners[k];
      topk_w[(long)t * K + k] = probs[k] / picked_sum;
    }
  }
}

// ------------------------------------------------- H-split router GEMV
// The router projection (N=128 outputs) maps to only N/4=32 workgroups in
// the generic wave-per-output GEMV — latency-starved at 10.8 µs for 0.5 MB.
// Split H into RS=4 slices: wave (n, s) computes a partial dot (4× the
// parallelism, one 512-element burst per wave); the router top-k kernel
// sums the 4 partials when it loads each logit (an f32x4 vector read).
#define RS 4

__global__ __launch_bounds__(256)
void router_gemv_partial_kernel(float* __restrict__ yp,   // [B, N, RS]
                                const short* __restrict__ x,   // [B, H]
                                const short* __restrict__ w,   // [N, H]
                                int B, int H, int N) {
  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + wid;
  const int s = blockIdx.y;
  if (n >= N) return;
  const int hs = H / RS;
  const int h0 = s * hs;
  float acc[8];
  #pragma unroll
  for (int b = 0; b < 8; ++b) acc[b] = 0.f;
  const short* wrow = w + (long)n * H + h0;
  for (int base = lane * 8; base < hs; base += WAVE * 8) {
    bf16x8 wv = *reinterpret_cast<const bf16x8*>(wrow + base);
    float wf[8];
    #pragma unroll
    for (int j = 0; j < 8; ++j) wf[j] = bf2f(wv[j]);
    #pragma unroll
    for (int b = 0; b < 8; ++b) {
      if (b < B) {
        acc[b] = dot8_unfused(acc[b], wf, *reinterpret_cast<const bf16x8*>(
            x + (long)b * H + h0 + base));
      }
    }
  }
  #pragma unroll
  for (int b = 0; b < 8; ++b) {
    if (b < B) {
      const float r = wave_reduce_sum(acc[b]);
      if (lane == 0) yp[((long)b * N + n) * RS + s] = r;
    }
  }
}

// router_gemv_partial with the post-attention RMSNorm folded in: the input is
// the residual row r[b], not a normed row. One wave per (expert row n, batch
// row b), grid (N/4, B). The wave loads r[b], γ and its W row up front; while
// the cold W row is in flight it computes the row's sum of squares in the
// order rmsnorm's 256-thread block does (vector v belongs to thread v mod 256:
// accumulator q stands for that block's wave q, lane for lane; each is
// reduced by the same butterfly and they combine as block_reduce_sum combines
// four waves), forms xn = bf16(r·scale·γ) as the norm kernel does, and takes
// the RS quarter dots with router_gemv_partial's lane → element mapping. So
// yp, and hbuf (stored by the n = 0 wave of each b, for moe_gemv_h), hold the
// bits of rmsnorm → router_gemv_partial. H2048: every load issued before the
// first use; otherwise any H with H % 32 == 0, loads inside the loops.
template <bool H2048>
__global__ __launch_bounds__(256)
void router_norm_gemv_partial_kernel(float* __restrict__ yp,   // [B, N, RS]
                                     short* __restrict__ hbuf, // [B, H]
                                     const short* __restrict__ r,     // [B, H]
                                     const short* __restrict__ gamma, // [H]
                                     const short* __restrict__ w,     // [N, H]
                                     int H, int N, float eps) {
  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + wid;
  const int b = blockIdx.y;
  if (n >= N) return;
  const bool store_h = n == 0;
  const short* wrow = w + (long)n * H;
  const short* rrow = r + (long)b * H;
  short* hrow = hbuf + (long)b * H;
  float ss[RS], acc[RS];
  #pragma unroll
  for (int q = 0; q < RS; ++q) { ss[q] = 0.f; acc[q] = 0.f; }

  // xn = bf16(r·scale·γ) for one vector; its quarter-dot step against wv
  auto norm_dot = [&](float a, bf16x8 rv, bf16x8 gv, bf16x8 wv, float scale,
                      int off) {
    bf16x8 xn;
    float wf[8];
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
      xn[j] = f2bf(bf2f(rv[j]) * scale * bf2f(gv[j]));
      wf[j] = bf2f(wv[j]);
    }
    if (store_h) *reinterpret_cast<bf16x8*>(hrow + off) = xn;
    return dot8_unfused(a, wf, xn);
  };

  if constexpr (H2048) {
    bf16x8 wv[RS], rv[RS], gv[RS];
    // loads return in issue order: r and γ (L2 hits) go first so the norm
    // runs while the W row (cold, HBM) is still in flight behind them
    #pragma unroll
    for (int q = 0; q < RS; ++q)
      rv[q] = *reinterpret_cast<const bf16x8*>(rrow + (q * WAVE + lane) * 8);
    #pragma unroll
    for (int q = 0; q < RS; ++q)
      gv[q] = *reinterpret_cast<const bf16x8*>(gamma + (q * WAVE + lane) * 8);
    __builtin_amdgcn_sched_barrier(0);
    #pragma unroll
    for (int q = 0; q < RS; ++q)
      wv[q] = *reinterpret_cast<const bf16x8*>(wrow + (q * WAVE + lane) * 8);
    __builtin_amdgcn_sched_barrier(0);
    #pragma unroll
    for (int q = 0; q < RS; ++q) ss[q] = sumsq8(0.f, rv[q]);
    wave_reduce_sum_n<RS>(ss);
    const float scale = rsqrtf(((ss[0] + ss[2]) + (ss[1] + ss[3])) / H + eps);
    #pragma unroll
    for (int q = 0; q < RS; ++q)
      acc[q] = norm_dot(0.f, rv[q], gv[q], wv[q], scale, (q * WAVE + lane) * 8);
  } else {
    const int vecs = H / 8;
    #pragma unroll
    for (int q = 0; q < RS; ++q)
      for (int v = q * WAVE + lane; v < vecs; v += 4 * WAVE)
        ss[q] = sumsq8(ss[q], *reinterpret_cast<const bf16x8*>(rrow + v * 8));
    wave_reduce_sum_n<RS>(ss);
    const float scale = rsqrtf(((ss[0] + ss[2]) + (ss[1] + ss[3])) / H + eps);
    const int hs = H / RS;
    #pragma unroll
    for (int q = 0; q < RS; ++q)
      for (int base = lane * 8; base < hs; base += WAVE * 8) {
        const int off = q * hs + base;
        acc[q] = norm_dot(acc[q],
                          *reinterpret_cast<const bf16x8*>(rrow + off),
                          *reinterpret_cast<const bf16x8*>(gamma + off),
                          *reinterpret_cast<const bf16x8*>(wrow + off), scale,
                          off);
      }
  }
  wave_reduce_sum_n<RS>(acc);
  if (lane == 0) {
    f32x4 o;
    #pragma unroll
    for (int q = 0; q < RS; ++q) o[q] = acc[q];
    *reinterpret_cast<f32x4*>(yp + ((long)b * N + n) * RS) = o;
  }
}

// moe_router over RS-partial logits: lane l owns logits 2l, 2l+1; each is an
// f32x4 load + horizontal sum. Same ids/weights as moe_router's selection.
__global__ __launch_bounds__(WAVE)
void moe_router_p4_kernel(int* __restrict__ topk_ids,
                          float* __restrict__ topk_w,
                          const float* __restrict__ yp,  // [T, E, RS]
                          int E, int K) {
  const int t = blockIdx.x;
  const int lane = threadIdx.x;
  float l0 = -INFINITY, l1 = -INFINITY;
  if (2 * lane < E) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(
        yp + ((long)t * E + 2 * lane) * RS);
    l0 = v[0] + v[1] + v[2] + v[3];
  }
  if (2 * lane + 1 < E) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(
        yp + ((long)t * E + 2 * lane + 1) * RS);
    l1 = v[0] + v[1] + v[2] + v[3];
  }
  router_select(topk_ids, topk_w, l0, l1, t, lane, K);
}

// ---------------------------------------------------------------- GEMV path
// h[p][j] = silu(dot(x_t, Wg_row_j)) * dot(x_t, Wu_row_j)
// grid: (npairs, I/4); block 256 = 4 waves; wave w computes output j.
// NIT = H/512 when known at compile time (4 for the model): the row's 3*NIT
// loads are all issued before the first FMA, as in gemv_row_dot; 0 = any H.
template <int NIT>
__global__ __launch_bounds__(256)
void moe_gemv_h_kernel(short* __restrict__ h,             // [P, I]
                       const short* __restrict__ x,        // [T, H]
                       const short* __restrict__ w13,      // [E, 2I, H]
                       const int* __restrict__ pair_token,  // [P]
                       const int* __restrict__ pair_expert, // [P]
                       float* __restrict__ out_zero,        // [zero_n] or null
                       long zero_n, int H, int I) {
  // side job: zero the downstream accumulator (out of moe_gemv_down) here —
  // the grid has ~2M threads vs ~10k floats to clear, and this kernel always
  // runs right before the down kernel, so the separate fill launch it
  // replaces (4.8 µs/layer, 2.8% of the decode step) is absorbed for free.
  if (out_zero != nullptr) {
    const long gid = ((long)blockIdx.y * gridDim.x + blockIdx.x) * blockDim.x
                     + threadIdx.x;
    if (gid < zero_n) out_zero[gid] = 0.f;
  }
  const int p = blockIdx.x;
  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.y * 4 + wid;
  if (j >= I) return;
  const int t = pair_token[p];
  const int e = pair_expert[p];
  const short* xrow = x + (long)t * H;
  const short* grow = w13 + ((long)e * 2 * I + j) * H;
  const short* urow = w13 + ((long)e * 2 * I + I + j) * H;

  float dg = 0.f, du = 0.f;
  if constexpr (NIT > 0) {
    bf16x8 xv[NIT], gv[NIT], uv[NIT];
    #pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int base = lane * 8 + it * WAVE * 8;
      gv[it] = *reinterpret_cast<const bf16x8*>(grow + base);
      uv[it] = *reinterpret_cast<const bf16x8*>(urow + base);
      xv[it] = *reinterpret_cast<const bf16x8*>(xrow + base);
    }
    __builtin_amdgcn_sched_barrier(0);   // keep the loads ahead of the FMAs
    #pragma unroll
    for (int it = 0; it < NIT; ++it) {
      #pragma unroll
      for (int q_ = 0; q_ < 8; ++q_) {
        float xf = bf2f(xv[it][q_]);
        dg += xf * bf2f(gv[it][q_]);
        du += xf * bf2f(uv[it][q_]);
      }
    }
  } else {
    for (int base = lane * 8; base < H; base += WAVE * 8) {
      bf16x8 xv = *reinterpret_cast<const bf16x8*>(xrow + base);
      bf16x8 gv = *reinterpret_cast<const bf16x8*>(grow + base);
      bf16x8 uv = *reinterpret_cast<const bf16x8*>(urow + base);
      #pragma unroll
      for (int q_ = 0; q_ < 8; ++q_) {
        float xf = bf2f(xv[q_]);
        dg += xf * bf2f(gv[q_]);
        du += xf * bf2f(uv[q_]);
      }
    }
  }
  dg = wave_reduce_sum(dg);
  du = wave_reduce_sum(du);
  if (lane == 0) {
    float s = dg / (1.0f + __expf(-dg));
    h[(long)p * I + j] = f2bf(s * du);
  }
}

// z[t] += w_p * (h_p @ W2_e^T): wave per output dim o; atomic f32 add.
// NIT = I/128 when known at compile time (6 for the model): all loads of the
// row issued before the first FMA; 0 = any multiple of 128.
template <int NIT>
__global__ __launch_bounds__(256)
void moe_gemv_down_kernel(float* __restrict__ out,         // [T, H] f32
                          const short* __restrict__ h,      // [P, I]
                          const short* __restrict__ w2,     // [E, H, I]
                          const float* __restrict__ pair_w,  // [P]
                          const int* __restrict__ pair_token,
                          const int* __restrict__ pair_expert,
                          int H, int I) {
  // 16 lanes per output, 4 outputs per wave: the I=768 row is 1.5 full-wave
  // bursts (the second one 50% idle) and a 6-shuffle reduction per 1.5 KB in
  // the wave-per-output shape; 16-lane groups keep every lane busy (6 bursts
  // of 128 elems) and cut the reduction to 4 shuffles per output.
  const int p = blockIdx.x;
  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int grp = lane >> 4;       // output within the wave
  const int sub = lane & 15;       // 16 lanes per output
  const int o = (blockIdx.y * 4 + wid) * 4 + grp;
  if (o >= H) return;
  const int t = pair_token[p];
  const int e = pair_expert[p];
  const short* hrow = h + (long)p * I;
  const short* wrow = w2 + ((long)e * H + o) * I;

  float d = 0.f;
  if constexpr (NIT > 0) {
    bf16x8 hv[NIT], wv[NIT];
    #pragma unroll
    for (int it = 0; it < NIT; ++it) {
      wv[it] = *reinterpret_cast<const bf16x8*>(wrow + sub * 8 + it * 16 * 8);
      hv[it] = *reinterpret_cast<const bf16x8*>(hrow + sub * 8 + it * 16 * 8);
    }
    __builtin_amdgcn_sched_barrier(0);   // keep the loads ahead of the FMAs
    #pragma unroll
    for (int it = 0; it < NIT; ++it) {
      #pragma unroll
      for (int q_ = 0; q_ < 8; ++q_) d += bf2f(hv[it][q_]) * bf2f(wv[it][q_]);
    }
  } else {
    for (int base = sub * 8; base < I; base += 16 * 8) {
      bf16x8 hv = *reinterpret_cast<const bf16x8*>(hrow + base);
      bf16x8 wv = *reinterpret_cast<const bf16x8*>(wrow + base);
      #pragma unroll
      for (int q_ = 0; q_ < 8; ++q_) d += bf2f(hv[q_]) * bf2f(wv[q_]);
    }
  }
  #pragma unroll
  for (int off = 8; off > 0; off >>= 1) d += __shfl_xor(d, off, WAVE);
  if (sub == 0)
    atomicAdd(out + (long)t * H + o, d * pair_w[p]);
}

// ---------------------------------------------------------------- wrappers

// What the three routers share: E <= 128 experts, 1 <= K <= min(8, E) picks,
// and topk_ids [rows, K] int32, topk_w [rows, K] f32 to hold them.
static void router_check(OpChecks& c, const torch::Tensor& topk_ids,
                         const torch::Tensor& topk_w, int64_t rows, int64_t E,
                         int64_t K) {
  c.range("E", E, 1, 128);
  c.range("K", K, 1, std::min<int64_t>(8, E));
  c.tensor("topk_ids", topk_ids, kI32, {rows, K});
  c.tensor("topk_w", topk_w, kF32, {rows, K});
}

// The decode routers' GEMV: x [B, H] bf16 rows (at most 8) against wr [E, H]
// bf16, every quarter of H in 8-wide vectors.
struct RouterDims { int B, H, E; };
static RouterDims router_gemv_check(OpChecks& c, const char* xname,
                                    const torch::Tensor& x,
                                    const torch::Tensor& wr, int min_rows) {
  c.tensor(xname, x, kBF16, {-1, -1});
  const int B = c.size_range(xname, x, 0, min_rows, 8);
  const int H = c.size_multiple(xname, x, 1, RS * 8);
  c.tensor("wr", wr, kBF16, {-1, H});
  return {B, H, c.fits_int("wr.size(0)", wr.size(0))};
}

void moe_router(torch::Tensor topk_ids, torch::Tensor topk_w, torch::Tensor logits,
                int64_t K) {
  OpChecks c("moe_router");
  c.tensor("logits", logits, kF32, {-1, -1});
  const int T = c.fits_int("logits.size(0)", logits.size(0));
  const int E = c.fits_int("logits.size(1)", logits.size(1));
  router_check(c, topk_ids, topk_w, T, E, K);
  c.grid(T);
  if (check_only()) return;
  dim3 grid(T), block(WAVE);
  hipStream_t s = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(moe_router_kernel, grid, block, 0, s,
                     topk_ids.data_ptr<int>(), topk_w.data_ptr<float>(),
                     logits.data_ptr<float>(), E, (int)K);
  HIP_CHECK_KERNEL();
}

// persistent RS-partial logits buffer per (B, E): allocation-free on graph
// replay
static float* router_partials(int B, int E, c10::Device dev) {
  static std::unordered_map<long, torch::Tensor> parts;
  const long key = (long)B * 1024 + E;
  auto it = parts.find(key);
  if (it == parts.end())
    it = parts.emplace(key, torch::empty(
        {(long)B * E * RS},
        torch::TensorOptions().device(dev).dtype(torch::kFloat32))).first;
  return it->second.data_ptr<float>();
}

void router_gemv_topk(torch::Tensor topk_ids, torch::Tensor topk_w,
                      torch::Tensor x, torch::Tensor wr, int64_t K) {
  OpChecks c("router_gemv_topk");
  const auto [B, H, E] = router_gemv_check(c, "x", x, wr, 0);
  router_check(c, topk_ids, topk_w, B, E, K);
  if (check_only()) return;
  float* yp = router_partials(B, E, x.device());
  hipStream_t s = c10::hip::getCurrentHIPStream();
  dim3 g1((E + 3) / 4, RS);
  hipLaunchKernelGGL(router_gemv_partial_kernel, g1, dim3(256), 0, s,
                     yp, (const short*)x.data_ptr(),
                     (const short*)wr.data_ptr(), B, H, E);
  HIP_CHECK_KERNEL();
  hipLaunchKernelGGL(moe_router_p4_kernel, dim3(B), dim3(WAVE), 0, s,
                     topk_ids.data_ptr<int>(), topk_w.data_ptr<float>(),
                     yp, E, (int)K);
  HIP_CHECK_KERNEL();
}

void router_norm_gemv_topk(torch::Tensor topk_ids, torch::Tensor topk_w,
                           torch::Tensor hbuf, torch::Tensor r,
                           torch::Tensor gamma, torch::Tensor wr, int64_t K,
                           double eps) {
  OpChecks c("router_norm_gemv_topk");
  const auto [B, H, E] = router_gemv_check(c, "r", r, wr, 1);
  router_check(c, topk_ids, topk_w, B, E, K);
  c.tensor("hbuf", hbuf, kBF16, {B, H});
  c.tensor("gamma", gamma, kBF16, {H});
  if (check_only()) return;
  float* yp = router_partials(B, E, r.device());
  hipStream_t s = c10::hip::getCurrentHIPStream();
  dim3 g1((E + 3) / 4, B);
  #define ROUTER_NORM(H2048) hipLaunchKernelGGL( \
      router_norm_gemv_partial_kernel<H2048>, g1, dim3(256), 0, s, yp, \
      (short*)hbuf.data_ptr(), (const short*)r.data_ptr(), \
      (const short*)gamma.data_ptr(), (const short*)wr.data_ptr(), H, E, \
      (float)eps)
  if (H == RS * WAVE * 8) ROUTER_NORM(true); else ROUTER_NORM(false);
  #undef ROUTER_NORM
  HIP_CHECK_KERNEL();
  hipLaunchKernelGGL(moe_router_p4_kernel, dim3(B), dim3(WAVE), 0, s,
                     topk_ids.data_ptr<int>(), topk_w.data_ptr<float>(),
                     yp, E, (int)K);
  HIP_CHECK_KERNEL();
}

void moe_gemv_h(torch::Tensor h, torch::Tensor x, torch::Tensor w13,
                torch::Tensor pair_token, torch::Tensor pair_expert,
                torch::Tensor out_zero) {
  OpChecks c("moe_gemv_h");
  moe_gemv_h_check(c, h, x, pair_token, pair_expert, out_zero);
  const int P = h.size(0), I = h.size(1);
  const int H = c.size_multiple("x", x, 1, WAVE * 8);
  bf16_check_weights(c, "w13", w13, 2 * (int64_t)I, H);
  if (check_only()) return;
  dim3 grid(P, (I + 3) / 4), block(256);
  const bool zero = out_zero.defined() && out_zero.numel() > 0;
  float* zp = zero ? out_zero.data_ptr<float>() : nullptr;
  const long zn = zero ? out_zero.numel() : 0;
  hipStream_t s = c10::hip::getCurrentHIPStream();
  #define MOE_H_GO(NIT) hipLaunchKernelGGL( \
      moe_gemv_h_kernel<NIT>, grid, block, 0, s, (short*)h.data_ptr(), \
      (const short*)x.data_ptr(), (const short*)w13.data_ptr(), \
      pair_token.data_ptr<int>(), pair_expert.data_ptr<int>(), zp, zn, H, I)
  if (H == 4 * WAVE * 8) MOE_H_GO(4); else MOE_H_GO(0);
  #undef MOE_H_GO
  HIP_CHECK_KERNEL();
}

void moe_gemv_down(torch::Tensor out, torch::Tensor h, torch::Tensor w2,
                   torch::Tensor pair_w, torch::Tensor pair_token,
                   torch::Tensor pair_expert) {
  OpChecks c("moe_gemv_down");
  moe_gemv_down_check(c, out, h, pair_w, pair_token, pair_expert);
  const int P = h.size(0), H = out.size(1), I = h.size(1);
  bf16_check_weights(c, "w2", w2, H, I);
  if (check_only()) return;
  dim3 grid(P, (H + 15) / 16), block(256);   // 16 outputs per WG
  hipStream_t s = c10::hip::getCurrentHIPStream();
  #define MOE_DOWN_GO(NIT) hipLaunchKernelGGL( \
      moe_gemv_down_kernel<NIT>, grid, block, 0, s, out.data_ptr<float>(), \
      (const short*)h.data_ptr(), (const short*)w2.data_ptr(), \
      pair_w.data_ptr<float>(), pair_token.data_ptr<int>(), \
      pair_expert.data_ptr<int>(), H, I)
  if (I == 6 * 16 * 8) MOE_DOWN_GO(6); else MOE_DOWN_GO(0);
  #undef MOE_DOWN_GO
  HIP_CHECK_KERNEL();
}

// ------------------------------------------------ grouped MFMA GEMM (prefill)
// C[P_sorted, N] = X[token(p), :] @ W[e, :, :]^T for tokens grouped by expert.
// tile_desc per m-tile: (expert, pair_row_start, m_size); the n-tile comes
// from grid.y.
//
// MFMA fragment layouts (gfx950 mfma_f32_16x16x32_bf16, verified vs torch in
// tests/test_kernels_gpu.py):
//   A (16×32): lane l holds A[l&15][(l>>4)*8 .. +8]
//   B (32×16): lane l holds B[(l>>4)*8 .. +8][l&15]
//   C (16×16): lane l, reg r ↦ row (l>>4)*4 + r, col l&15
typedef __attribute__((ext_vector_type(4))) float cfrag_t;
typedef __attribute__((ext_vector_type(2))) float f32x2;

// A BM=16 tile re-reads each expert's weight panel ceil(rows/16)× per layer
// (~8× at 2k-token prefill → 6.4 GB/layer). BM=128 reads W once per expert
// m-tile: 8 waves (512 threads), wave w owns rows [16w, 16w+16) × BN=64.
// LDS rows padded +8 bf16 so ds_read_b128 across rows spreads banks (G4).

#define G2_BM 128
#define G2_BN 64
#define G2_BK 64
#define G2_PAD 8

// Only <G2_BM, G2_BN, G2_BK> is instantiated. BN=128 (half the X-tile
// re-reads), BK=128 and BM=256 were each measured no faster; see
// profiles/PERF_NOTES.md.
//
// W8 = true (moe_grouped_gemm128_fp8): w holds e4m3fn bytes, w_s one f32
// scale per 128x128 block [E, N/128, H/128]. Only the W staging differs: a
// thread loads 8 B = 8 k of one row, and the tile reaches LDS as
// bf16_rne(f32(q) * s), the bits of dequantize_fp8_block(...).to(bf16). A
// 64-column n-tile and a 64-wide k-step lie inside one scale block, so s is
// one workgroup-uniform load per k-step. From LDS on (MFMA order, epilogue)
// both instantiations run the same code: the outputs are bit-equal to the
// bf16 kernel on the dequantised weights.
template <int BM, int BN, int BK = G2_BK, bool W8 = false>
__global__ __launch_bounds__(512)
void moe_grouped_gemm128_kernel(short* __restrict__ out,      // [P, N]
                                const short* __restrict__ x,   // [T, H]
                                const void* __restrict__ wv,   // [E, N, H]
                                const float* __restrict__ w_s, // W8 only
                                const int* __restrict__ pair_token,
                                const int* __restrict__ tile_desc,  // [G,3]
                                int H, int N) {
  const int g = blockIdx.x;
  const int msize = tile_desc[g * 3 + 2];
  if (msize == 0) return;                 // past the live tile count
  const int e = tile_desc[g * 3 + 0];
  const int row0 = tile_desc[g * 3 + 1];
  const int n0 = blockIdx.y * BN;         // n-tile from the grid

  const int tid = threadIdx.x;
  const int wid = tid >> 6;       // wave index: MF 16-row m-slices each
  const int lane = tid & 63;

  __shared__ short xs[BM][BK + G2_PAD];
  __shared__ short ws[BN][BK + G2_PAD];

  // bf16: the expert's panel; W8: the same panel, one byte per element
  const short* wbase = W8 ? nullptr
                          : reinterpret_cast<const short*>(wv) + (long)e * N * H;
  const uint8_t* qbase = W8
      ? reinterpret_cast<const uint8_t*>(wv) + (long)e * N * H : nullptr;
  const float* sbase = W8
      ? w_s + ((long)e * (N / 128) + n0 / 128) * (H / 128) : nullptr;
  constexpr int NF = BN / 16;             // n-fragments per wave
  constexpr int MF = BM / 128;            // m-fragments per wave (1 or 2)

  cfrag_t acc[MF][NF];
  #pragma unroll
  for (int mf = 0; mf < MF; ++mf)
    #pragma unroll
    for (int nf = 0; nf < NF; ++nf) acc[mf][nf] = cfrag_t{0.f, 0.f, 0.f, 0.f};

  for (int k0 = 0; k0 < H; k0 += BK) {
    // stage X tile: BM rows × 64 k = BM*8 vec8 → BM/64 per thread
    #pragma unroll
    for (int it = 0; it < BM * BK / 64 / G2_BK; ++it) {
      const int idx = tid + it * 512;
      const int r = (idx * 8) / BK;
      const int c = (idx * 8) % BK;
      bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (r < msize) {
        const int tok = pair_token[row0 + r];
        v = *reinterpret_cast<const bf16x8*>(x + (long)tok * H + k0 + c);
      }
      *reinterpret_cast<bf16x8*>(&xs[r][c]) = v;
    }
    // stage W tile: BN rows × 64 k → BN/64 vec8 per thread
    #pragma unroll
    for (int it = 0; it < BN * BK / 64 / G2_BK; ++it) {
      const int idx = tid + it * 512;
      const int r = (idx * 8) / BK;
      const int c = (idx * 8) % BK;
      bf16x8 v;
      if constexpr (W8) {
        // 8 e4m3 bytes -> f32 (exact) -> one multiply by the block scale ->
        // bf16 round-to-nearest-even
        const int2 q = *reinterpret_cast<const int2*>(
            qbase + (long)(n0 + r) * H + k0 + c);
        const float sc = sbase[k0 / 128];
        const f32x2 p0 = __builtin_amdgcn_cvt_pk_f32_fp8(q.x, false);
        const f32x2 p1 = __builtin_amdgcn_cvt_pk_f32_fp8(q.x, true);
        const f32x2 p2 = __builtin_amdgcn_cvt_pk_f32_fp8(q.y, false);
        const f32x2 p3 = __builtin_amdgcn_cvt_pk_f32_fp8(q.y, true);
        v[0] = f2bf(p0[0] * sc); v[1] = f2bf(p0[1] * sc);
        v[2] = f2bf(p1[0] * sc); v[3] = f2bf(p1[1] * sc);
        v[4] = f2bf(p2[0] * sc); v[5] = f2bf(p2[1] * sc);
        v[6] = f2bf(p3[0] * sc); v[7] = f2bf(p3[1] * sc);
      } else {
        v = *reinterpret_cast<const bf16x8*>(
            wbase + (long)(n0 + r) * H + k0 + c);
      }
      *reinterpret_cast<bf16x8*>(&ws[r][c]) = v;
    }
    __syncthreads();

    #pragma unroll
    for (int kk = 0; kk < BK / 32; ++kk) {
      const int akoff = kk * 32 + (lane >> 4) * 8;
      #pragma unroll
      for (int mf = 0; mf < MF; ++mf) {
        const int arow = mf * 128 + wid * 16 + (lane & 15);
        bf16x8 a = *reinterpret_cast<const bf16x8*>(&xs[arow][akoff]);
        #pragma unroll
        for (int nf = 0; nf < NF; ++nf) {
          const int bcol = nf * 16 + (lane & 15);
          bf16x8 b = *reinterpret_cast<const bf16x8*>(&ws[bcol][akoff]);
          acc[mf][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[mf][nf], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }

  const int ccol_base = lane & 15;
  #pragma unroll
  for (int mf = 0; mf < MF; ++mf) {
    const int crow = mf * 128 + wid * 16 + (lane >> 4) * 4;
    #pragma unroll
    for (int nf = 0; nf < NF; ++nf) {
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = crow + r;
        if (m < msize)
          out[(long)(row0 + m) * N + n0 + nf * 16 + ccol_base] = f2bf(acc[mf][nf][r]);
      }
    }
  }
}

void moe_grouped_gemm128(torch::Tensor out, torch::Tensor x, torch::Tensor w,
                         torch::Tensor pair_token, torch::Tensor tile_desc) {
  OpChecks c("moe_grouped_gemm128");
  grouped_gemm_check(c, false, out, x, pair_token, tile_desc);
  const int H = x.size(1), N = out.size(1), G = tile_desc.size(0);
  bf16_check_weights(c, "w", w, N, H);
  if (check_only()) return;
  hipStream_t s = c10::hip::getCurrentHIPStream();
  dim3 grid(G, N / G2_BN), block(512);
  hipLaunchKernelGGL((moe_grouped_gemm128_kernel<G2_BM, G2_BN>), grid, block, 0, s,
                     (short*)out.data_ptr(), (const short*)x.data_ptr(),
                     (const void*)w.data_ptr(), (const float*)nullptr,
                     pair_token.data_ptr<int>(), tile_desc.data_ptr<int>(),
                     H, N);
  HIP_CHECK_KERNEL();
}

// launch of the e4m3 instantiation; every argument is checked by its caller,
// moe_grouped_gemm128_fp8 in moe_fp8.hip (N, H multiples of 128, G >= 1)
void moe_grouped_gemm128_fp8_launch(short* out, const short* x,
                                    const uint8_t* w_q, const float* w_s,
                                    const int* pair_token, const int* tile_desc,
                                    int G, int H, int N, hipStream_t s) {
  dim3 grid(G, N / G2_BN), block(512);
  hipLaunchKernelGGL(
      (moe_grouped_gemm128_kernel<G2_BM, G2_BN, G2_BK, true>), grid, block, 0,
      s, out, x, (const void*)w_q, w_s, pair_token, tile_desc, H, N);
}

// gather-combine: out[t] = Σ_k w[t,k] * z[inv_order[t*K+k]] — an atomicAdd
// scatter combine cost 33M atomics/layer at 2k-token prefill (0.9 ms/layer).
// inv_order maps (token, k) → sorted-pair row of z.
__global__ void moe_combine_gather_kernel(short* __restrict__ out,  // [T, H] bf16
                                          const short* __restrict__ z,  // [P, H]
                                          const float* __restrict__ topk_w,  // [T, K]
                                          const int* __restrict__ inv_order,  // [T*K]
                                          int H, int K) {
  const int t = blockIdx.x;
  float w[8];
  int p[8];
  for (int k = 0; k < K; ++k) {
    w[k] = topk_w[(long)t * K + k];
    p[k] = inv_order[(long)t * K + k];
  }
  for (int i = threadIdx.x * 8; i < H; i += blockDim.x * 8) {
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < K; ++k) {
      bf16x8 zv = *reinterpret_cast<const bf16x8*>(z + (long)p[k] * H + i);
      #pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += w[k] * bf2f(zv[j]);
    }
    bf16x8 o;
    #pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = f2bf(acc[j]);
    *reinterpret_cast<bf16x8*>(out + (long)t * H + i) = o;
  }
}

void moe_combine_gather(torch::Tensor out, torch::Tensor z, torch::Tensor topk_w,
                        torch::Tensor inv_order) {
  OpChecks c("moe_combine_gather");
  c.tensor("out", out, kBF16, {-1, -1});
  const int T = c.fits_int("out.size(0)", out.size(0));
  const int H = c.size_multiple("out", out, 1, 8);
  c.tensor("z", z, kBF16, {-1, H});
  c.tensor("topk_w", topk_w, kF32, {T, -1});
  const int K = c.size_range("topk_w", topk_w, 1, 1, 8);
  c.tensor("inv_order", inv_order, kI32, {(int64_t)T * K});
  c.grid(T);
  if (check_only()) return;
  dim3 grid(T), block(256);
  hipStream_t s = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(moe_combine_gather_kernel, grid, block, 0, s,
                     (short*)out.data_ptr(), (const short*)z.data_ptr(),
                     topk_w.data_ptr<float>(), inv_order.data_ptr<int>(), H, K);
  HIP_CHECK_KERNEL();
}

// device-side tile-descriptor builder: removes the per-layer host syncs that
// data-dependent repeat_interleave shapes forced (profiled: ~6 syncs/layer
// serialized prefill on the CPU). desc[GMAX,3] = (expert, row_start, m_size);
// unused slots get m_size=0 and the GEMM early-exits. GMAX is host-computed
// from P alone (≤ E + ceil(P/G2_BM)), so grids stay static.
__global__ void moe_build_desc_kernel(int* __restrict__ desc,      // [GMAX, 3]
                                      const long* __restrict__ counts,  // [E]
                                      int E, int bm, int gmax) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int g = 0;
  long row = 0;
  for (int e = 0; e < E; ++e) {
    const long c = counts[e];
    for (long m0 = 0; m0 < c && g < gmax; m0 += bm) {
      desc[g * 3 + 0] = e;
      desc[g * 3 + 1] = (int)(row + m0);
      desc[g * 3 + 2] = (int)min((long)bm, c - m0);
      ++g;
    }
    row += c;
  }
  for (; g < gmax; ++g) desc[g * 3 + 2] = 0;
}

void moe_build_desc(torch::Tensor desc, torch::Tensor counts, int64_t bm) {
  OpChecks c("moe_build_desc");
  c.tensor("desc", desc, kI32, {-1, 3});
  c.tensor("counts", counts, kI64, {-1});
  const int E = c.fits_int("counts.size(0)", counts.size(0));
  const int gmax = c.fits_int("desc.size(0)", desc.size(0));
  c.range("bm", bm, 1, G2_BM);
  if (check_only()) return;
  hipStream_t s = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(moe_build_desc_kernel, dim3(1), dim3(64), 0, s,
                     desc.data_ptr<int>(), counts.data_ptr<long>(), E, (int)bm,
                     gmax);
  HIP_CHECK_KERNEL();
}
