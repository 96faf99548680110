// Fused per-row sampling: repetition/presence/frequency penalties +
// temperature + top-k + top-p + multinomial draw, two kernels.
//
// V ≈ 152k, B small (decode batch). Everything stays on-GPU and hipGraph-
// capturable. Every parameter is read per row from device memory, so one
// captured decode graph serves any mix of requests. The uniform draw is a pure
// function of (seeds[b], ctr[b]) — no RNG state is carried or written; the
// engine passes its position tensor as ctr, which already advances inside the
// captured step. The token-history ring advances on-device (append).
//
// Design (two-stage scan):
//   1) V4_NSC blocks per row each scan a contiguous slice; every thread keeps
//      its top-8 in VGPRs via a fully-static compare/shift chain (no dynamic
//      indexing → no scratch), then a block tournament emits the slice's
//      top-8 sorted descending. Penalties ride inside this scan: a row with
//      penalties on stages its ring window (≤ 256 tokens) in LDS and marks
//      the window's tokens in a one-bit-per-logit bitmap of the block's slice;
//      the scan tests one bit per logit and only a hit (≤ 256 per row) walks
//      the window to count occurrences. A row with penalties off builds
//      nothing and runs the plain loop (block-uniform branch);
//   2) one wave per row: lane l owns block l's 8 candidates in LDS, a
//      shuffle-argmax tournament extracts the global top-K, and lane 0 runs
//      the temperature softmax, top-p nucleus cut and multinomial draw, and
//      (append) pushes the picked token into the row's ring.
// The global top-K (K ≤ 64) is contained in the union of per-thread top-8
// unless one thread's strided slice holds ≥9 of the global top-K:
// P ≈ C(64,9)/256⁸ < 1e-9 for random position assignment — negligible for
// sampling purposes. Penalties are applied before the filter, so the argument
// holds for the penalised logits.
// Earlier single-block samplers (per-thread top-K lists in scratch, then in
// LDS, then in registers) left 251 CUs idle during the scan (rocprof: 335 µs
// per step at B=5, scan-bound); see profiles/PERF_NOTES.md.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include "common.h"
#include "checks.h"

#define SMP_THREADS 256
#define SMP_MAXK 64

#define V4_NSC 64
#define V4_KEEP 8
#define SMP_RING 256                    // token-history ring entries per row
#define SMP_MAXSPAN 4096                // bitmap bits per block → V ≤ 64·4096

// uniform [0,1) from (seed, counter): the counter-th output of splitmix64
// seeded with `seed`, top 24 bits
__device__ __forceinline__ float splitmix_unit(uint64_t seed, uint32_t ctr) {
  uint64_t z = seed + ((uint64_t)ctr + 1ull) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (float)(z >> 40) / 16777216.0f;
}

// static insert of (x, v) into the descending register list r0..r7 / i0..i7
#define TOP8_INSERT(x, v)                                                     \
  if ((x) > r7) {                                                             \
    if ((x) > r0) {                                                           \
      r7=r6; i7=i6; r6=r5; i6=i5; r5=r4; i5=i4; r4=r3; i4=i3;                 \
      r3=r2; i3=i2; r2=r1; i2=i1; r1=r0; i1=i0; r0=(x); i0=(v);               \
    } else if ((x) > r1) {                                                    \
      r7=r6; i7=i6; r6=r5; i6=i5; r5=r4; i5=i4; r4=r3; i4=i3;                 \
      r3=r2; i3=i2; r2=r1; i2=i1; r1=(x); i1=(v);                             \
    } else if ((x) > r2) {                                                    \
      r7=r6; i7=i6; r6=r5; i6=i5; r5=r4; i5=i4; r4=r3; i4=i3;                 \
      r3=r2; i3=i2; r2=(x); i2=(v);                                           \
    } else if ((x) > r3) {                                                    \
      r7=r6; i7=i6; r6=r5; i6=i5; r5=r4; i5=i4; r4=r3; i4=i3; r3=(x); i3=(v); \
    } else if ((x) > r4) {                                                    \
      r7=r6; i7=i6; r6=r5; i6=i5; r5=r4; i5=i4; r4=(x); i4=(v);               \
    } else if ((x) > r5) {                                                    \
      r7=r6; i7=i6; r6=r5; i6=i5; r5=(x); i5=(v);                             \
    } else if ((x) > r6) {                                                    \
      r7=r6; i7=i6; r6=(x); i6=(v);                                           \
    } else {                                                                  \
      r7=(x); i7=(v);                                                         \
    }                                                                         \
  }

__global__ __launch_bounds__(SMP_THREADS, 2)
void sample_scan_kernel(float* __restrict__ part_v,  // [B, NSC, KEEP]
                        int* __restrict__ part_i,
                        const float* __restrict__ logits, int V,
                        const float* __restrict__ rep_pen,      // [B]
                        const float* __restrict__ presence_pen,
                        const float* __restrict__ freq_pen,
                        const int* __restrict__ last_n,
                        const int* __restrict__ ring,           // [B, RING]
                        const int* __restrict__ ring_len) {
  const int b = blockIdx.x;
  const int blk = blockIdx.y;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const float* row = logits + (long)b * V;
  const int span = (V + V4_NSC - 1) / V4_NSC;
  const int lo = blk * span, hi = min(V, lo + span);

  __shared__ int win[SMP_RING];
  __shared__ unsigned bits[SMP_MAXSPAN / 32];

  // penalty window: the last min(last_n, len, RING) pushes; block-uniform
  const float rep = rep_pen[b], pres = presence_pen[b], freq = freq_pen[b];
  const int len = ring_len[b];
  const int wn = max(0, min(min(last_n[b], len), SMP_RING));
  const bool pen = wn > 0 && (rep != 1.0f || pres != 0.0f || freq != 0.0f);
  if (pen) {
    if (tid < SMP_MAXSPAN / 32) bits[tid] = 0u;
    __syncthreads();
    if (tid < wn) {
      const int t = ring[b * SMP_RING + ((len - wn + tid) & (SMP_RING - 1))];
      win[tid] = t;
      if (t >= lo && t < hi)
        atomicOr(&bits[(t - lo) >> 5], 1u << ((t - lo) & 31));
    }
    __syncthreads();
  }

  float r0 = -INFINITY, r1 = -INFINITY, r2 = -INFINITY, r3 = -INFINITY,
        r4 = -INFINITY, r5 = -INFINITY, r6 = -INFINITY, r7 = -INFINITY;
  int i0 = -1, i1 = -1, i2 = -1, i3 = -1, i4 = -1, i5 = -1, i6 = -1, i7 = -1;
  if (!pen) {
    for (int v = lo + tid; v < hi; v += SMP_THREADS) {
      const float x = row[v];
      TOP8_INSERT(x, v)
    }
  } else {
    for (int v = lo + tid; v < hi; v += SMP_THREADS) {
      float x = row[v];
      const int o = v - lo;
      if ((bits[o >> 5] >> (o & 31)) & 1u) {   // rare: ≤ wn hits per row
        int c = 0;
        for (int j = 0; j < wn; ++j) c += (win[j] == v);
        x = (x > 0.0f) ? x / rep : x * rep;
        x -= (float)c * freq + pres;
      }
      TOP8_INSERT(x, v)
    }
  }

  __shared__ float cv[SMP_THREADS * (V4_KEEP + 1)];
  __shared__ int ci[SMP_THREADS * (V4_KEEP + 1)];
  __shared__ float wmax[4];
  __shared__ int wwin[4];
  float* mycv = cv + tid * (V4_KEEP + 1);
  int* myci = ci + tid * (V4_KEEP + 1);
  mycv[0]=r0; mycv[1]=r1; mycv[2]=r2; mycv[3]=r3;
  mycv[4]=r4; mycv[5]=r5; mycv[6]=r6; mycv[7]=r7;
  myci[0]=i0; myci[1]=i1; myci[2]=i2; myci[3]=i3;
  myci[4]=i4; myci[5]=i5; myci[6]=i6; myci[7]=i7;
  float my_max = r0;
  int my_slot = 0;
  __syncthreads();

  float* pv = part_v + ((long)b * V4_NSC + blk) * V4_KEEP;
  int* pi = part_i + ((long)b * V4_NSC + blk) * V4_KEEP;
  for (int k = 0; k < V4_KEEP; ++k) {
    float v = my_max; int who = tid;
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      float ov = __shfl_xor(v, off, WAVE);
      int ow = __shfl_xor(who, off, WAVE);
      if (ov > v || (ov == v && ow < who)) { v = ov; who = ow; }
    }
    if (lane == 0) { wmax[wid] = v; wwin[wid] = who; }
    __syncthreads();
    float bv = wmax[0]; int bw = wwin[0];
    #pragma unroll
    for (int w = 1; w < 4; ++w)
      if (wmax[w] > bv || (wmax[w] == bv && wwin[w] < bw)) {
        bv = wmax[w]; bw = wwin[w];
      }
    if (tid == bw) {
      pv[k] = my_max;
      pi[k] = myci[my_slot];
      ++my_slot;
      my_max = (my_slot < V4_KEEP) ? mycv[my_slot] : -INFINITY;
    }
    if (bv == -INFINITY) {       // uniform: pad the rest and stop
      if (tid == 0)
        for (int j = k; j < V4_KEEP; ++j) { pv[j] = -INFINITY; pi[j] = -1; }
      return;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(64)
void sample_final_kernel(int* __restrict__ out_tokens,
                         const float* __restrict__ part_v,
                         const int* __restrict__ part_i,
                         const float* __restrict__ temperature,  // [B]
                         const float* __restrict__ top_p,
                         const int* __restrict__ top_k,
                         const int64_t* __restrict__ seeds,      // read-only
                         const int* __restrict__ ctr,            // read-only
                         int* __restrict__ ring,                 // [B, RING]
                         int* __restrict__ ring_len, int append) {
  const int b = blockIdx.x;
  const int lane = threadIdx.x;
  __shared__ float cand_v[V4_NSC][V4_KEEP];
  __shared__ int cand_i[V4_NSC][V4_KEEP];
  __shared__ float sel_v[SMP_MAXK];
  __shared__ int sel_i[SMP_MAXK];
  #pragma unroll
  for (int j = 0; j < V4_KEEP; ++j) {
    cand_v[lane][j] = part_v[((long)b * V4_NSC + lane) * V4_KEEP + j];
    cand_i[lane][j] = part_i[((long)b * V4_NSC + lane) * V4_KEEP + j];
  }
  for (int k = lane; k < SMP_MAXK; k += 64) sel_v[k] = -INFINITY;
  __syncthreads();

  const int K = max(1, min(top_k[b], SMP_MAXK));   // wave-uniform
  int slot = 0;
  float head = cand_v[lane][0];
  for (int k = 0; k < K; ++k) {
    float v = head; int who = lane;
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      float ov = __shfl_xor(v, off, WAVE);
      int ow = __shfl_xor(who, off, WAVE);
      if (ov > v || (ov == v && ow < who)) { v = ov; who = ow; }
    }
    if (v == -INFINITY) break;   // uniform across the wave
    if (lane == who) {
      sel_v[k] = head;
      sel_i[k] = cand_i[lane][slot];
      ++slot;
      head = (slot < V4_KEEP) ? cand_v[lane][slot] : -INFINITY;
    }
  }
  __syncthreads();

  if (lane == 0) {
    const float temp = temperature[b];
    int n = 0;
    while (n < K && sel_v[n] != -INFINITY && sel_i[n] >= 0) ++n;
    int pick = 0;
    if (n > 0 && temp <= 1e-5f) {
      pick = sel_i[0];
    } else if (n > 0) {
      const float invt = 1.0f / temp;
      const float m = sel_v[0];
      float denom = 0.f;
      for (int i = 0; i < n; ++i) denom += __expf((sel_v[i] - m) * invt);
      float target = top_p[b] * denom;
      float cum = 0.f;
      int cut = n;
      for (int i = 0; i < n; ++i) {
        cum += __expf((sel_v[i] - m) * invt);
        if (cum >= target) { cut = i + 1; break; }
      }
      float denom2 = 0.f;
      for (int i = 0; i < cut; ++i) denom2 += __expf((sel_v[i] - m) * invt);
      float r = splitmix_unit((uint64_t)seeds[b], (uint32_t)ctr[b]) * denom2;
      float acc = 0.f;
      pick = sel_i[cut - 1];
      for (int i = 0; i < cut; ++i) {
        acc += __expf((sel_v[i] - m) * invt);
        if (r <= acc) { pick = sel_i[i]; break; }
      }
    }
    out_tokens[b] = pick;
    if (append) {
      const int len = ring_len[b];
      ring[b * SMP_RING + (len & (SMP_RING - 1))] = pick;
      ring_len[b] = len + 1;
    }
  }
}

void sample_rows(torch::Tensor out_tokens, torch::Tensor logits,
                 torch::Tensor temperature, torch::Tensor top_p,
                 torch::Tensor top_k, torch::Tensor seeds, torch::Tensor ctr,
                 torch::Tensor repetition_penalty,
                 torch::Tensor presence_penalty,
                 torch::Tensor frequency_penalty, torch::Tensor repeat_last_n,
                 torch::Tensor ring, torch::Tensor ring_len, bool append) {
  OpChecks c("sample_rows");
  c.tensor("logits", logits, kF32, {-1, -1});
  const int B = c.fits_int("logits.size(0)", logits.size(0));
  const int V = c.size_range("logits", logits, 1, 1, V4_NSC * SMP_MAXSPAN);
  c.tensor("out_tokens", out_tokens, kI32, {B});
  c.tensor("temperature", temperature, kF32, {B});
  c.tensor("top_p", top_p, kF32, {B});
  c.tensor("top_k", top_k, kI32, {B});
  c.tensor("seeds", seeds, kI64, {B});
  c.tensor("ctr", ctr, kI32, {B});
  c.tensor("repetition_penalty", repetition_penalty, kF32, {B});
  c.tensor("presence_penalty", presence_penalty, kF32, {B});
  c.tensor("frequency_penalty", frequency_penalty, kF32, {B});
  c.tensor("repeat_last_n", repeat_last_n, kI32, {B});
  c.tensor("ring_len", ring_len, kI32, {B});
  c.tensor("ring", ring, kI32, {B, SMP_RING});
  c.grid(B, V4_NSC);
  if (B == 0 || check_only()) return;
  // persistent per-B scratch: keeps the op allocation-free inside hipGraph
  // capture (the engine's decode graphs replay this kernel pair)
  static std::unordered_map<int, std::pair<torch::Tensor, torch::Tensor>> scratch;
  auto it = scratch.find(B);
  if (it == scratch.end()) {
    auto opts = torch::TensorOptions().device(logits.device());
    it = scratch.emplace(B, std::make_pair(
        torch::empty({(long)B * V4_NSC * V4_KEEP}, opts.dtype(torch::kFloat32)),
        torch::empty({(long)B * V4_NSC * V4_KEEP}, opts.dtype(torch::kInt32)))).first;
  }
  torch::Tensor part_v = it->second.first, part_i = it->second.second;
  hipStream_t s = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(sample_scan_kernel, dim3(B, V4_NSC),
                     dim3(SMP_THREADS), 0, s, part_v.data_ptr<float>(),
                     part_i.data_ptr<int>(), logits.data_ptr<float>(), V,
                     repetition_penalty.data_ptr<float>(),
                     presence_penalty.data_ptr<float>(),
                     frequency_penalty.data_ptr<float>(),
                     repeat_last_n.data_ptr<int>(), ring.data_ptr<int>(),
                     ring_len.data_ptr<int>());
  HIP_CHECK_KERNEL();
  hipLaunchKernelGGL(sample_final_kernel, dim3(B), dim3(64), 0, s,
                     out_tokens.data_ptr<int>(), part_v.data_ptr<float>(),
                     part_i.data_ptr<int>(), temperature.data_ptr<float>(),
                     top_p.data_ptr<float>(), top_k.data_ptr<int>(),
                     seeds.data_ptr<int64_t>(), ctr.data_ptr<int>(),
                     ring.data_ptr<int>(), ring_len.data_ptr<int>(),
                     append ? 1 : 0);
  HIP_CHECK_KERNEL();
}

// token-history append for multi-step decode graphs: each graph replay
// appends the step's sampled tokens into a ring and bumps the device counter,
// so the host syncs once per K-step block instead of every step.
__global__ void hist_append_kernel(int* __restrict__ hist,   // [KMAX * B]
                                   int* __restrict__ ctr,    // [1]
                                   const int* __restrict__ toks,  // [B]
                                   int B, int kmax) {
  const int i = threadIdx.x;
  const int step = ctr[0];
  if (step < kmax && i < B) hist[step * B + i] = toks[i];
  __syncthreads();
  if (i == 0) ctr[0] = step + 1;
}

void hist_append(torch::Tensor hist, torch::Tensor ctr, torch::Tensor toks,
                 int64_t kmax) {
  OpChecks c("hist_append");
  c.tensor("toks", toks, kI32, {-1});
  // one thread per token, one block
  const int B = c.size_range("toks", toks, 0, 0, 1024);
  c.range("kmax", kmax, 0, std::numeric_limits<int>::max() / std::max(B, 1));
  c.tensor("hist", hist, kI32, {kmax * B});
  c.tensor("ctr", ctr, kI32, {1});
  if (check_only()) return;
  hipStream_t s = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(hist_append_kernel, dim3(1), dim3(std::max(B, 64)), 0, s,
                     hist.data_ptr<int>(), ctr.data_ptr<int>(),
                     toks.data_ptr<int>(), B, (int)kmax);
  HIP_CHECK_KERNEL();
}
