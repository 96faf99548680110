// HBM-resident semantic-memory vector store: cosine scores + top-k.
// vs_topk: one query over every row. vs_topk_scoped (second half of this
// file): up to 8 queries per pass, each restricted to one room's rows.
//
// Replaces the reference's sqlite-vec CPU scan (src/shared/embeddings.ts:16-27,
// db-queries.ts:995-1010 `vec_distance_cosine` over BLOB rows). The matrix
// lives in HBM as [N, 384] bf16, rows L2-normalized at insert time, so cosine
// = plain dot. BASELINE config 4 sizes this at 10M × 384 (7.4 GB bf16 — a
// fraction of 288 GB HBM3E).
//
// Kernel: wave-per-row dot (384 dims / 64 lanes = 6 bf16 = 3×bf16x2 loads per
// lane → coalesced 1536 B per wave-instruction step), grid-stride; per-block
// top-k into a global candidate buffer; final merge of (blocks × k)
// candidates by a single-block second kernel.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include "common.h"
#include "checks.h"

#define VS_DIM 384
#define VS_MAXK 64
#define VS_BLOCK 256   // 4 waves

__global__ __launch_bounds__(VS_BLOCK)
void vs_score_topk_kernel(float* __restrict__ cand_v,   // [nblocks, K]
                          int* __restrict__ cand_i,     // [nblocks, K]
                          const short* __restrict__ mat,  // [N, 384] bf16 (L2-normed)
                          const float* __restrict__ query,  // [384] (L2-normed)
                          int N, int K) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int waves_per_grid = gridDim.x * (VS_BLOCK / WAVE);
  const int gwave = blockIdx.x * (VS_BLOCK / WAVE) + wid;

  // query → registers (6 f32 per lane)
  float qreg[6];
  #pragma unroll
  for (int j = 0; j < 6; ++j) qreg[j] = query[lane * 6 + j];

  // per-wave local top-K kept by lane0..K-1? Simpler: per-wave insertion into
  // LDS list guarded by lane 0 (scores arrive one per row iteration).
  __shared__ float lv[VS_BLOCK / WAVE][VS_MAXK];
  __shared__ int li[VS_BLOCK / WAVE][VS_MAXK];
  if (lane < K) { lv[wid][lane] = -INFINITY; li[wid][lane] = -1; }

  float lmin = -INFINITY;
  for (long r = gwave; r < N; r += waves_per_grid) {
    const short* mrow = mat + r * VS_DIM + lane * 6;
    float dot = 0.f;
    // 6 bf16 per lane: one 4-wide + one 2-wide load
    bf16x4 a = *reinterpret_cast<const bf16x4*>(mrow);
    short b0 = mrow[4], b1 = mrow[5];
    dot = qreg[0] * bf2f(a[0]) + qreg[1] * bf2f(a[1]) + qreg[2] * bf2f(a[2])
        + qreg[3] * bf2f(a[3]) + qreg[4] * bf2f(b0) + qreg[5] * bf2f(b1);
    dot = wave_reduce_sum(dot);
    if (lane == 0 && dot > lmin) {
      int pos = K - 1;
      while (pos > 0 && lv[wid][pos - 1] < dot) {
        lv[wid][pos] = lv[wid][pos - 1]; li[wid][pos] = li[wid][pos - 1]; --pos;
      }
      lv[wid][pos] = dot; li[wid][pos] = (int)r;
      lmin = lv[wid][K - 1];
    }
    lmin = __shfl(lmin, 0, WAVE);
  }
  __syncthreads();

  // merge the block's 4 wave-lists (sorted desc) → block top-K by wave 0
  if (wid == 0 && lane == 0) {
    int p[VS_BLOCK / WAVE] = {0, 0, 0, 0};
    for (int k = 0; k < K; ++k) {
      float best = -INFINITY; int bw = 0;
      #pragma unroll
      for (int w = 0; w < VS_BLOCK / WAVE; ++w) {
        if (p[w] < K && lv[w][p[w]] > best) { best = lv[w][p[w]]; bw = w; }
      }
      cand_v[(long)blockIdx.x * K + k] = best;
      cand_i[(long)blockIdx.x * K + k] = (best == -INFINITY) ? -1 : li[bw][p[bw]];
      if (best != -INFINITY) ++p[bw];
    }
  }
}

// final merge: one block, iterative argmax over nblocks*K candidates (small)
__global__ void vs_merge_kernel(float* __restrict__ out_v,  // [K]
                                long* __restrict__ out_i,   // [K]
                                float* __restrict__ cand_v,
                                int* __restrict__ cand_i,
                                int ncand, int K) {
  const int lane = threadIdx.x & 63;
  if (threadIdx.x >= WAVE) return;
  for (int k = 0; k < K; ++k) {
    float best = -INFINITY; int besti = -1;
    for (int i = lane; i < ncand; i += WAVE) {
      if (cand_v[i] > best) { best = cand_v[i]; besti = i; }
    }
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      float ov = __shfl_xor(best, o, WAVE);
      int oi = __shfl_xor(besti, o, WAVE);
      if (ov > best) { best = ov; besti = oi; }
    }
    besti = __shfl(besti, 0, WAVE);   // consistent winner everywhere
    if (lane == 0) {
      out_v[k] = best;
      out_i[k] = (besti >= 0) ? (long)cand_i[besti] : -1;
    }
    if (lane == 0 && besti >= 0) cand_v[besti] = -INFINITY;
  }
}

void vs_topk(torch::Tensor out_v, torch::Tensor out_i, torch::Tensor cand_v,
             torch::Tensor cand_i, torch::Tensor mat, torch::Tensor query,
             int64_t K) {
  OpChecks c("vs_topk");
  c.range("K", K, 1, VS_MAXK);
  c.tensor("mat", mat, kBF16, {-1, VS_DIM});
  const int N = c.fits_int("mat.size(0)", mat.size(0));
  c.tensor("query", query, kF32, {VS_DIM});
  c.tensor("cand_v", cand_v, kF32, {-1, K});
  const int nblocks = c.fits_int("cand_v.size(0)", cand_v.size(0));
  c.fits_int("cand_v.numel()", nblocks * K);
  c.tensor("cand_i", cand_i, kI32, {nblocks, K});
  c.tensor("out_v", out_v, kF32, {K});
  c.tensor("out_i", out_i, kI64, {K});
  c.grid(nblocks);
  if (check_only()) return;
  hipStream_t s = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(vs_score_topk_kernel, dim3(nblocks), dim3(VS_BLOCK), 0, s,
                     cand_v.data_ptr<float>(), cand_i.data_ptr<int>(),
                     (const short*)mat.data_ptr(), query.data_ptr<float>(),
                     (int)N, (int)K);
  HIP_CHECK_KERNEL();
  hipLaunchKernelGGL(vs_merge_kernel, dim3(1), dim3(WAVE), 0, s,
                     out_v.data_ptr<float>(), out_i.data_ptr<long>(),
                     cand_v.data_ptr<float>(), cand_i.data_ptr<int>(),
                     nblocks * (int)K, (int)K);
  HIP_CHECK_KERNEL();
}

// ---------------------------------------------------------------------------
// Room-scoped, batched variant: Q ≤ 8 queries share one pass over the matrix.
//
// tags[r] is the room id of row r (0 = global row). scopes[q] < 0 admits every
// row; scopes[q] = s admits rows with tag == s or tag == 0.
//
// A wave takes 64 consecutive rows per grid-stride step: one coalesced 256 B
// tag read, a ballot of "some query admits this row", then a wave-uniform walk
// over the set bits only — rows no query admits are never read, so a scoped
// search over a multi-room store costs its own rows + 4 B/row of tags. Each
// admitted row is loaded once and dotted against all Q queries (Q is a
// template parameter: every register array is statically indexed). The Q
// partial sums are reduced with a halving butterfly: each of the first
// log2(QP) shuffle steps halves the number of live sums per lane, so Q = 8
// costs 4+2+1+3 = 10 shuffles instead of 48, and query q's total lands in the
// lane group [q*64/QP, (q+1)*64/QP).
//
// A wave sees only N / (8·nblocks) rows, a dozen times K, so its top-K list
// changes often (≈ K·ln(rows/K) times per query). While scanning, the sorted
// list of query q therefore lives across the wave's lanes (element i in lane
// i, one VGPR pair per query): an insertion is one ballot for the rank and
// one shift-by-one shuffle, against a lane-0 shift loop through LDS in
// vs_score_topk_kernel (N=1M, K=20: Q=1 390 → 289 µs, 1/8-scope 135 → 68 µs).
// The lists go to LDS once, after the scan, for the block merge.
//
// The row loop is a dependent chain (load → 6 shuffle steps → compare), so it
// is latency-bound at 2 waves/SIMD: 8-wave blocks (512 blocks → 16 waves/CU)
// measured Q=1 289 → 197 µs and Q=5 859 → 555 µs over 4-wave blocks.
// ---------------------------------------------------------------------------
#define VS_MAXQ 8
#define VS_SBLOCK 512   // 8 waves
#define VS_LPAD (VS_MAXK + 1)   // merge threads of different queries hit different banks

struct VsRow { unsigned w0, w1, w2; };   // 3 × bf16x2 per lane

DEV VsRow vs_load_row(const short* __restrict__ mat, long r, int lane) {
  // dims {128j + 2*lane, +1}: each of the 3 loads is a fully coalesced 256 B
  const unsigned* p = reinterpret_cast<const unsigned*>(mat + r * VS_DIM) + lane;
  VsRow x;
  x.w0 = p[0]; x.w1 = p[64]; x.w2 = p[128];
  return x;
}

DEV float vs_lo(unsigned w) { return __uint_as_float(w << 16); }
DEV float vs_hi(unsigned w) { return __uint_as_float(w & 0xffff0000u); }

template <int Q>
// ≥ 4 waves/SIMD (≤ 128 VGPRs) so two 8-wave blocks fit a CU at every Q
__global__ __launch_bounds__(VS_SBLOCK) __attribute__((amdgpu_waves_per_eu(4)))
void vs_scoped_score_kernel(float* __restrict__ cand_v,        // [Q, nblocks, K]
                            int* __restrict__ cand_i,          // [Q, nblocks, K]
                            const short* __restrict__ mat,     // [N, 384] bf16
                            const int* __restrict__ tags,      // [N]
                            const float* __restrict__ queries, // [Q, 384]
                            const int* __restrict__ scopes,    // [Q]
                            int N, int K) {
  constexpr int QP = Q <= 1 ? 1 : Q <= 2 ? 2 : Q <= 4 ? 4 : 8;
  constexpr int GRP = WAVE / QP;
  constexpr int NW = VS_SBLOCK / WAVE;
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int waves_per_grid = gridDim.x * NW;
  const int gwave = blockIdx.x * NW + wid;
  const int ntiles = (int)(((long)N + WAVE - 1) / WAVE);

  float qreg[Q][6];
  int sc[Q];
  #pragma unroll
  for (int q = 0; q < Q; ++q) {
    #pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float2 t = *reinterpret_cast<const float2*>(
          queries + q * VS_DIM + 128 * j + 2 * lane);
      qreg[q][2 * j] = t.x; qreg[q][2 * j + 1] = t.y;
    }
    sc[q] = scopes[q];
  }

  // per-query sorted top-K, element i in lane i (lanes ≥ K stay -inf / -1)
  float lv[Q];
  int li[Q];
  float lmin[Q];   // wave-uniform K-th best per query
  #pragma unroll
  for (int q = 0; q < Q; ++q) { lv[q] = -INFINITY; li[q] = -1; lmin[q] = -INFINITY; }

  for (int t = gwave; t < ntiles; t += waves_per_grid) {
    const long r0 = (long)t * WAVE;
    const long rl = r0 + lane;
    int tag = -1;
    bool any = false;
    if (rl < N) {
      tag = tags[rl];
      #pragma unroll
      for (int q = 0; q < Q; ++q) any |= (sc[q] < 0) | (tag == 0) | (tag == sc[q]);
    }
    unsigned long long mask = __ballot(any);
    if (mask == 0) continue;

    int b = __ffsll(mask) - 1;
    VsRow cur = vs_load_row(mat, r0 + b, lane);
    while (true) {
      mask &= mask - 1;
      // next admitted row's load is issued before this row's reduction
      const int nb = mask ? __ffsll(mask) - 1 : b;
      const VsRow nxt = vs_load_row(mat, r0 + nb, lane);

      const float x0 = vs_lo(cur.w0), x1 = vs_hi(cur.w0), x2 = vs_lo(cur.w1),
                  x3 = vs_hi(cur.w1), x4 = vs_lo(cur.w2), x5 = vs_hi(cur.w2);
      float a[QP];
      #pragma unroll
      for (int q = 0; q < QP; ++q) {
        if (q < Q) {
          a[q] = qreg[q][0] * x0 + qreg[q][1] * x1 + qreg[q][2] * x2
               + qreg[q][3] * x3 + qreg[q][4] * x4 + qreg[q][5] * x5;
        } else {
          a[q] = 0.f;
        }
      }
      // halving butterfly: QP live sums → 1, then plain butterfly to the end
      int off = 32;
      #pragma unroll
      for (int cnt = QP; cnt > 1; cnt >>= 1, off >>= 1) {
        const int half = cnt >> 1;
        const bool hi = (lane & off) != 0;
        #pragma unroll
        for (int j = 0; j < half; ++j) {
          const float send = hi ? a[j] : a[j + half];
          const float keep = hi ? a[j + half] : a[j];
          a[j] = keep + __shfl_xor(send, off, WAVE);
        }
      }
      #pragma unroll
      for (; off > 0; off >>= 1) a[0] += __shfl_xor(a[0], off, WAVE);

      const int rtag = __builtin_amdgcn_readlane(tag, b);
      #pragma unroll
      for (int q = 0; q < Q; ++q) {
        // query q's total sits in lane group q; everything below is uniform
        const float dot = __int_as_float(
            __builtin_amdgcn_readlane(__float_as_int(a[0]), q * GRP));
        const bool admit = (sc[q] < 0) | (rtag == 0) | (rtag == sc[q]);
        if (admit && dot > lmin[q]) {
          // rank = entries ≥ dot; lanes past it take their left neighbour
          const int pos = __popcll(__ballot(lv[q] >= dot));
          const float up_v = __shfl_up(lv[q], 1, WAVE);
          const int up_i = __shfl_up(li[q], 1, WAVE);
          if (lane >= pos && lane < K) {
            lv[q] = (lane == pos) ? dot : up_v;
            li[q] = (lane == pos) ? (int)(r0 + b) : up_i;
          }
          lmin[q] = __int_as_float(
              __builtin_amdgcn_readlane(__float_as_int(lv[q]), K - 1));
        }
      }
      if (mask == 0) break;
      cur = nxt; b = nb;
    }
  }

  // wave lists → LDS for the block merge
  __shared__ float slv[NW][Q][VS_LPAD];
  __shared__ int sli[NW][Q][VS_LPAD];
  #pragma unroll
  for (int q = 0; q < Q; ++q) { slv[wid][q][lane] = lv[q]; sli[wid][q][lane] = li[q]; }
  __syncthreads();

  // thread q merges query q's 4 wave-lists (sorted desc) → block top-K
  if (threadIdx.x < Q) {
    const int q = threadIdx.x;
    int p[NW];
    #pragma unroll
    for (int w = 0; w < NW; ++w) p[w] = 0;
    const long base = ((long)q * gridDim.x + blockIdx.x) * K;
    for (int k = 0; k < K; ++k) {
      float best = -INFINITY; int bw = -1, bi = -1;
      #pragma unroll
      for (int w = 0; w < NW; ++w) {
        if (p[w] < K) {
          const float v = slv[w][q][p[w]];
          if (v > best) { best = v; bw = w; bi = sli[w][q][p[w]]; }
        }
      }
      cand_v[base + k] = best;
      cand_i[base + k] = bi;
      #pragma unroll
      for (int w = 0; w < NW; ++w) p[w] += (w == bw);
    }
  }
}

// final merge: one wave per query. Every block's list is sorted descending,
// so the global top-K is a K-round tournament over the list heads: a lane
// owns up to VS_MLISTS lists (head value, its successor prefetched, position —
// all in statically indexed registers), a round is a lane-local max plus one
// shuffle argmax, and only the winning lane touches memory (one value load,
// one index load). Re-scanning all nblocks*K candidates per round, as
// vs_merge_kernel does, cost 0.37 ms more at nblocks=512, K=20 (Q=1 total
// 761 → 390 µs) — more than the 0.77 GB scan itself.
#define VS_MLISTS 8   // lists per lane → nblocks ≤ 512

__global__ __launch_bounds__(WAVE)
void vs_scoped_merge_kernel(float* __restrict__ out_v,         // [Q, K]
                            long* __restrict__ out_i,          // [Q, K]
                            const float* __restrict__ cand_v,  // [Q, nblocks, K]
                            const int* __restrict__ cand_i,
                            int nblocks, int K) {
  const int lane = threadIdx.x;
  const float* cv = cand_v + (long)blockIdx.x * nblocks * K;
  const int* ci = cand_i + (long)blockIdx.x * nblocks * K;
  float head[VS_MLISTS], next[VS_MLISTS];
  int pos[VS_MLISTS];
  #pragma unroll
  for (int j = 0; j < VS_MLISTS; ++j) {
    const int l = lane + WAVE * j;
    head[j] = (l < nblocks) ? cv[l * K] : -INFINITY;
    next[j] = (l < nblocks && K > 1) ? cv[l * K + 1] : -INFINITY;
    pos[j] = 0;
  }
  for (int k = 0; k < K; ++k) {
    float best = -INFINITY; int bj = -1;
    #pragma unroll
    for (int j = 0; j < VS_MLISTS; ++j) {
      if (head[j] > best) { best = head[j]; bj = j; }
    }
    float wv = best; int wl = lane;
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(wv, o, WAVE);
      const int ol = __shfl_xor(wl, o, WAVE);
      // ties go to the lower lane so every lane agrees on the winner
      if (ov > wv || (ov == wv && ol < wl)) { wv = ov; wl = ol; }
    }
    if (wv == -INFINITY) {        // fewer than K rows in scope: pad
      if (lane == 0) {
        out_v[(long)blockIdx.x * K + k] = -INFINITY;
        out_i[(long)blockIdx.x * K + k] = -1;
      }
    } else if (lane == wl) {
      #pragma unroll
      for (int j = 0; j < VS_MLISTS; ++j) {
        if (j == bj) {
          const int at = (lane + WAVE * j) * K + pos[j];
          out_v[(long)blockIdx.x * K + k] = wv;
          out_i[(long)blockIdx.x * K + k] = (long)ci[at];
          ++pos[j];
          head[j] = next[j];
          next[j] = (pos[j] + 1 < K) ? cv[at + 2] : -INFINITY;
        }
      }
    }
  }
}

template <int Q>
static void vs_scoped_launch(hipStream_t s, int nblocks, float* cand_v,
                             int* cand_i, const short* mat, const int* tags,
                             const float* queries, const int* scopes, int N,
                             int K) {
  hipLaunchKernelGGL(vs_scoped_score_kernel<Q>, dim3(nblocks), dim3(VS_SBLOCK),
                     0, s, cand_v, cand_i, mat, tags, queries, scopes, N, K);
}

void vs_topk_scoped(torch::Tensor out_v, torch::Tensor out_i,
                    torch::Tensor cand_v, torch::Tensor cand_i,
                    torch::Tensor mat, torch::Tensor tags,
                    torch::Tensor queries, torch::Tensor scopes, int64_t K) {
  OpChecks c("vs_topk_scoped");
  c.range("K", K, 1, VS_MAXK);
  c.tensor("mat", mat, kBF16, {-1, VS_DIM});
  const long N = c.fits_int("mat.size(0)", mat.size(0));
  c.tensor("tags", tags, kI32, {N});
  c.tensor("queries", queries, kF32, {-1, VS_DIM});
  const long Q = c.size_range("queries", queries, 0, 1, VS_MAXQ);
  c.tensor("scopes", scopes, kI32, {Q});
  // the merge wave holds every block's list head: at most 512 blocks
  c.tensor("cand_v", cand_v, kF32, {Q, -1, K});
  const int nblocks = c.size_range("cand_v", cand_v, 1, 1, WAVE * VS_MLISTS);
  c.tensor("cand_i", cand_i, kI32, {Q, nblocks, K});
  c.tensor("out_v", out_v, kF32, {Q, K});
  c.tensor("out_i", out_i, kI64, {Q, K});
  if (check_only()) return;
  hipStream_t s = c10::hip::getCurrentHIPStream();
  float* cv = cand_v.data_ptr<float>();
  int* ci = cand_i.data_ptr<int>();
  const short* m = (const short*)mat.data_ptr();
  const int* tg = tags.data_ptr<int>();
  const float* qs = queries.data_ptr<float>();
  const int* sp = scopes.data_ptr<int>();
  switch (Q) {
    case 1: vs_scoped_launch<1>(s, nblocks, cv, ci, m, tg, qs, sp, (int)N, (int)K); break;
    case 2: vs_scoped_launch<2>(s, nblocks, cv, ci, m, tg, qs, sp, (int)N, (int)K); break;
    case 3: vs_scoped_launch<3>(s, nblocks, cv, ci, m, tg, qs, sp, (int)N, (int)K); break;
    case 4: vs_scoped_launch<4>(s, nblocks, cv, ci, m, tg, qs, sp, (int)N, (int)K); break;
    case 5: vs_scoped_launch<5>(s, nblocks, cv, ci, m, tg, qs, sp, (int)N, (int)K); break;
    case 6: vs_scoped_launch<6>(s, nblocks, cv, ci, m, tg, qs, sp, (int)N, (int)K); break;
    case 7: vs_scoped_launch<7>(s, nblocks, cv, ci, m, tg, qs, sp, (int)N, (int)K); break;
    default: vs_scoped_launch<8>(s, nblocks, cv, ci, m, tg, qs, sp, (int)N, (int)K); break;
  }
  HIP_CHECK_KERNEL();
  hipLaunchKernelGGL(vs_scoped_merge_kernel, dim3((int)Q), dim3(WAVE), 0, s,
                     out_v.data_ptr<float>(), out_i.data_ptr<long>(), cv, ci,
                     nblocks, (int)K);
  HIP_CHECK_KERNEL();
}
