// Dense skinny-batch GEMV: y[B, N] = x[B, H] @ W[N, H]^T  (decode projections).
//
// hipBLASLt runs these M≤8 shapes at ~1.1 TB/s (measured, scripts/
// gpu_op_microbench.py); this kernel streams W once for ALL batch rows
// (x rows are L2-resident) with 16 B/lane coalesced loads. Used for the
// QKV/O/router/lm_head projections at decode; prefill keeps hipBLASLt.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include "common.h"

#define GEMV_MAXB 8

// this lane's 8 elements of each of the BN rows at xs (row stride H)
template <int BN>
DEV void gemv_load_x(bf16x8 (&xv)[BN], const short* xs, int H) {
  #pragma unroll
  for (int b = 0; b < BN; ++b)
    xv[b] = *reinterpret_cast<const bf16x8*>(xs + (long)b * H);
}

// acc[b] += dot(w, x_b) over this lane's 8 elements, j ascending.
template <int BN>
DEV void gemv_fma8(float (&acc)[BN], bf16x8 wv, const bf16x8 (&xv)[BN]) {
  float wf[8];
  #pragma unroll
  for (int j = 0; j < 8; ++j) wf[j] = bf2f(wv[j]);
  #pragma unroll
  for (int b = 0; b < BN; ++b) {
    #pragma unroll
    for (int j = 0; j < 8; ++j) acc[b] += wf[j] * bf2f(xv[b][j]);
  }
}

// One wave's BN dot products of the W row at wrow with the rows at xs (row
// stride H, global or LDS). NIT = H/512 is the trip count when it is known at
// compile time (4 and 8 are the decode projections): every W load of the row
// is then issued before the first FMA, so the row costs one HBM round trip
// and not NIT in series; the x loads (L2 or LDS hits) run one iteration ahead
// of their FMAs. NIT = 0 takes any multiple of 512 and loads inside the loop.
// The FMA order per accumulator is the same in both.
template <int BN, int NIT>
DEV void gemv_row_dot(float (&acc)[BN], const short* wrow, const short* xs,
                      int H, int lane) {
  #pragma unroll
  for (int b = 0; b < BN; ++b) acc[b] = 0.f;
  if constexpr (NIT > 0) {
    constexpr int HC = NIT * WAVE * 8;
    // x loads run PF iterations ahead of their FMAs; 2 measured slower
    // in-bench (more registers, nothing left to hide)
    constexpr int PF = 1;
    bf16x8 wv[NIT], xv[PF + 1][BN];
    #pragma unroll
    for (int it = 0; it < NIT; ++it)
      wv[it] = *reinterpret_cast<const bf16x8*>(wrow + lane * 8 + it * WAVE * 8);
    #pragma unroll
    for (int it = 0; it < PF && it < NIT; ++it)
      gemv_load_x<BN>(xv[it], xs + lane * 8 + it * WAVE * 8, HC);
    // the scheduler otherwise sinks every load back to its first use; pin
    // the issue order at each stage
    __builtin_amdgcn_sched_barrier(0);
    #pragma unroll
    for (int it = 0; it < NIT; ++it) {
      if (it + PF < NIT)
        gemv_load_x<BN>(xv[(it + PF) % (PF + 1)],
                        xs + lane * 8 + (it + PF) * WAVE * 8, HC);
      __builtin_amdgcn_sched_barrier(0);
      gemv_fma8<BN>(acc, wv[it], xv[it % (PF + 1)]);
      __builtin_amdgcn_sched_barrier(0);
    }
  } else {
    for (int base = lane * 8; base < H; base += WAVE * 8) {
      bf16x8 xv[BN];
      gemv_load_x<BN>(xv, xs + base, H);
      gemv_fma8<BN>(acc, *reinterpret_cast<const bf16x8*>(wrow + base), xv);
    }
  }
}

// The BN wave sums run as one interleaved xor butterfly (same pairing as
// wave_reduce_sum, so the same bits), which overlaps their shuffle latencies.
// Every lane then holds every sum: lane b stores row b, one store in all.
template <bool F32OUT, int BN>
DEV void gemv_reduce_store(float (&acc)[BN], void* y, int N, int n, int lane) {
  wave_reduce_sum_n<BN>(acc);
  float r = acc[0];
  #pragma unroll
  for (int b = 1; b < BN; ++b) r = (lane == b) ? acc[b] : r;
  if (lane < BN) {
    if (F32OUT)
      ((float*)y)[(long)lane * N + n] = r;
    else
      ((short*)y)[(long)lane * N + n] = f2bf(r);
  }
}

// BN = exact batch (compile-time): the generic MAXB=8 unroll carried 8 acc
// registers + per-lane bounds branches at any B — register pressure blocked
// software-pipelining of the 8 independent H-iterations.
// NIT = H/512 when specialized, 0 = any H (see gemv_row_dot).
template <bool F32OUT, int BN, int NIT>
__global__ __launch_bounds__(256)
void gemv_kernel(void* __restrict__ y,           // [BN, N] bf16 or f32
                 const short* __restrict__ x,     // [BN, H]
                 const short* __restrict__ w,     // [N, H]
                 int H, int N) {
  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + wid;
  if (n >= N) return;

  float acc[BN];
  gemv_row_dot<BN, NIT>(acc, w + (long)n * H, x, H, lane);
  gemv_reduce_store<F32OUT, BN>(acc, y, N, n, lane);
}

// x-rows staged through LDS once per WG: at B≥3 the per-wave x re-reads
// dominate L2 traffic (B=5, H=2048: each wave pulls 20 KB of x per dot →
// ~100 MB of L2 reads per QKV call across the 1280-WG grid; staging reads
// them once per WG). Dot loop is identical, sourced from LDS.
template <bool F32OUT, int BN, int NIT>
__global__ __launch_bounds__(256)
void gemv_ldsx_kernel(void* __restrict__ y,           // [BN, N]
                      const short* __restrict__ x,     // [BN, H]
                      const short* __restrict__ w,     // [N, H]
                      int H, int N) {
  extern __shared__ short xs[];                        // [BN * H]
  for (int i = threadIdx.x * 8; i < BN * H; i += 256 * 8)
    *reinterpret_cast<bf16x8*>(&xs[i]) =
        *reinterpret_cast<const bf16x8*>(x + i);
  __syncthreads();

  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + wid;
  if (n >= N) return;

  float acc[BN];
  gemv_row_dot<BN, NIT>(acc, w + (long)n * H, xs, H, lane);
  gemv_reduce_store<F32OUT, BN>(acc, y, N, n, lane);
}

template <bool F32OUT, int NIT>
static void gemv_launch(void* y, const short* x, const short* w, int B, int H,
                        int N, hipStream_t s) {
  dim3 grid((N + 3) / 4), block(256);
  const size_t lds = (size_t)B * H * sizeof(short);
  // LDS staging wins only on very wide-N shapes (lm_head: 152k rows,
  // 176 -> 151 us at B=5) where the grid's aggregate L2 x-traffic is the
  // bottleneck; on the 2-5k-row projections the barrier+occupancy cost
  // outweighs it (9.4 -> 9.9 us measured). Gate on N.
  const bool use_lds = B >= 3 && lds <= 64 * 1024 && N >= 16384;
  switch (B) {
#define GEMV_CASE(BN) \
    case BN: \
      if (use_lds) \
        hipLaunchKernelGGL((gemv_ldsx_kernel<F32OUT, BN, NIT>), grid, block, lds, \
                           s, y, x, w, H, N); \
      else \
        hipLaunchKernelGGL((gemv_kernel<F32OUT, BN, NIT>), grid, block, 0, s, \
                           y, x, w, H, N); \
      break;
    GEMV_CASE(1) GEMV_CASE(2) GEMV_CASE(3) GEMV_CASE(4)
    GEMV_CASE(5) GEMV_CASE(6) GEMV_CASE(7) GEMV_CASE(8)
#undef GEMV_CASE
    default: TORCH_CHECK(false, "gemv handles B<=8");
  }
}

void gemv(torch::Tensor y, torch::Tensor x, torch::Tensor w) {
  const int B = x.size(0), H = x.size(1), N = w.size(0);
  TORCH_CHECK(B >= 1 && B <= GEMV_MAXB,
              "gemv handles B<=8 (decode); use hipBLASLt above");
  TORCH_CHECK(x.dtype() == torch::kBFloat16 && w.dtype() == torch::kBFloat16);
  TORCH_CHECK(H % (WAVE * 8) == 0, "H must be a multiple of 512");
  hipStream_t s = c10::hip::getCurrentHIPStream();
  #define GEMV_GO(FO, NIT) gemv_launch<FO, NIT>( \
      y.data_ptr(), (const short*)x.data_ptr(), (const short*)w.data_ptr(), \
      B, H, N, s)
  #define GEMV_NIT(FO) do { switch (H / (WAVE * 8)) { \
    case 4: GEMV_GO(FO, 4); break; \
    case 8: GEMV_GO(FO, 8); break; \
    default: GEMV_GO(FO, 0); break; } } while (0)
  if (y.dtype() == torch::kFloat32) GEMV_NIT(true); else GEMV_NIT(false);
  #undef GEMV_NIT
  #undef GEMV_GO
  HIP_CHECK_KERNEL();
}

// ------------------------------------------------ fused add+RMSNorm+GEMV
// y[B,N] = rmsnorm(x + delta)·γ @ W^T, and (block 0 only) x_out = x + delta.
// Folds the per-layer fused_add_rmsnorm kernel and the normed-activation
// buffer round-trip into the projection itself: each wave already streams the
// full activation row, so the row norm is one extra L1-hot pass (decode chains
// ~14 dependent small kernels/layer; every removed kernel removes a
// launch+fill/drain bubble — see profiles/PERF_NOTES.md).
// Norm matches fused_add_rmsnorm semantics: computed over the bf16-rounded sum.
template <bool F32OUT, bool DELTA_F32, bool HAS_DELTA, int BN, int NIT>
__global__ __launch_bounds__(256)
void gemv_addnorm_kernel(void* __restrict__ y,            // [BN, N]
                         const short* __restrict__ x,      // [BN, H]
                         const void* __restrict__ delta_,  // [BN, H] or null
                         short* __restrict__ x_out,        // [BN, H]
                         const short* __restrict__ gamma,  // [H]
                         const short* __restrict__ w,      // [N, H]
                         int H, int N, float eps) {
  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + wid;

  // pass 1 (block-cooperative): row sums of squares, bf16-rounded to match
  // fused_add_rmsnorm. All 256 threads share the work (a per-wave pass was
  // measured as a B=5 regression: 4× redundant VALU across the block).
  __shared__ float ss_sh[BN];
  if (threadIdx.x < BN) ss_sh[threadIdx.x] = 0.f;
  __syncthreads();
  #pragma unroll
  for (int b = 0; b < BN; ++b) {
    {
      float ss = 0.f;
      for (int base = threadIdx.x * 8; base < H; base += 256 * 8) {
        bf16x8 xv = *reinterpret_cast<const bf16x8*>(x + (long)b * H + base);
        #pragma unroll
        for (int j = 0; j < 8; ++j) {
          float v = bf2f(xv[j]);
          if (HAS_DELTA) {
            if (DELTA_F32)
              v += ((const float*)delta_)[(long)b * H + base + j];
            else
              v += bf2f(((const short*)delta_)[(long)b * H + base + j]);
            v = bf2f(f2bf(v));
          }
          ss += v * v;
        }
      }
      ss = wave_reduce_sum(ss);
      if (lane == 0) atomicAdd(&ss_sh[b], ss);
    }
  }
  __syncthreads();
  float scale[BN];
  #pragma unroll
  for (int b = 0; b < BN; ++b)
    scale[b] = rsqrtf(ss_sh[b] / H + eps);

  // pass 1.5 (block-cooperative): stage xn = (x+δ)·scale·γ into LDS once, so
  // the dot loop is lean (w-load + LDS-load + FMA; no per-wave re-add/round)
  extern __shared__ short xn_sh[];  // [B][H] bf16
  #pragma unroll
  for (int b = 0; b < BN; ++b) {
    {
      for (int base = threadIdx.x * 8; base < H; base += 256 * 8) {
        bf16x8 xv = *reinterpret_cast<const bf16x8*>(x + (long)b * H + base);
        bf16x8 gv = *reinterpret_cast<const bf16x8*>(gamma + base);
        bf16x8 o;
        #pragma unroll
        for (int j = 0; j < 8; ++j) {
          float v = bf2f(xv[j]);
          if (HAS_DELTA) {
            if (DELTA_F32)
              v += ((const float*)delta_)[(long)b * H + base + j];
            else
              v += bf2f(((const short*)delta_)[(long)b * H + base + j]);
            v = bf2f(f2bf(v));
          }
          o[j] = f2bf(v * scale[b] * bf2f(gv[j]));
        }
        *reinterpret_cast<bf16x8*>(&xn_sh[b * H + base]) = o;
      }
    }
  }
  __syncthreads();

  // block 0 stores the updated residual (other blocks never read x_out here)
  if (HAS_DELTA && blockIdx.x == 0) {
    for (int i = threadIdx.x * 8; i < BN * H; i += 256 * 8) {
      bf16x8 xv = *reinterpret_cast<const bf16x8*>(x + i);
      bf16x8 o;
      #pragma unroll
      for (int j = 0; j < 8; ++j) {
        float v = bf2f(xv[j]);
        if (DELTA_F32) v += ((const float*)delta_)[i + j];
        else v += bf2f(((const short*)delta_)[i + j]);
        o[j] = f2bf(v);
      }
      *reinterpret_cast<bf16x8*>(x_out + i) = o;
    }
  }
  if (n >= N) return;

  // pass 2: lean dot against the LDS-staged normed rows
  float acc[BN];
  gemv_row_dot<BN, NIT>(acc, w + (long)n * H, xn_sh, H, lane);
  gemv_reduce_store<F32OUT, BN>(acc, y, N, n, lane);
}

void gemv_addnorm(torch::Tensor y, torch::Tensor x, torch::Tensor delta,
                  torch::Tensor x_out, torch::Tensor gamma, torch::Tensor w,
                  double eps) {
  const int B = x.size(0), H = x.size(1), N = w.size(0);
  TORCH_CHECK(B <= GEMV_MAXB && H % (WAVE * 8) == 0);
  TORCH_CHECK(x.dtype() == torch::kBFloat16 && w.dtype() == torch::kBFloat16);
  const bool has_delta = delta.numel() > 0;
  const bool delta_f32 = has_delta && delta.dtype() == torch::kFloat32;
  const bool f32out = y.dtype() == torch::kFloat32;
  dim3 grid((N + 3) / 4), block(256);
  const size_t lds = (size_t)B * H * sizeof(short);  // staged normed rows
  TORCH_CHECK(lds <= 160 * 1024, "B*H too large for LDS staging");
  hipStream_t s = c10::hip::getCurrentHIPStream();
  const void* dptr = has_delta ? delta.data_ptr() : nullptr;
  #define LAUNCH_AN2(FO, DF, HD, BN, NIT) hipLaunchKernelGGL( \
      (gemv_addnorm_kernel<FO, DF, HD, BN, NIT>), grid, block, lds, s, y.data_ptr(), \
      (const short*)x.data_ptr(), dptr, (short*)x_out.data_ptr(), \
      (const short*)gamma.data_ptr(), (const short*)w.data_ptr(), \
      H, N, (float)eps)
  #define LAUNCH_AN1(FO, DF, HD, BN) do { switch (H / (WAVE * 8)) { \
    case 4: LAUNCH_AN2(FO, DF, HD, BN, 4); break; \
    case 8: LAUNCH_AN2(FO, DF, HD, BN, 8); break; \
    default: LAUNCH_AN2(FO, DF, HD, BN, 0); break; } } while (0)
  #define LAUNCH_AN(FO, DF, HD) do { switch (B) { \
    case 1: LAUNCH_AN1(FO, DF, HD, 1); break; \
    case 2: LAUNCH_AN1(FO, DF, HD, 2); break; \
    case 3: LAUNCH_AN1(FO, DF, HD, 3); break; \
    case 4: LAUNCH_AN1(FO, DF, HD, 4); break; \
    case 5: LAUNCH_AN1(FO, DF, HD, 5); break; \
    case 6: LAUNCH_AN1(FO, DF, HD, 6); break; \
    case 7: LAUNCH_AN1(FO, DF, HD, 7); break; \
    default: LAUNCH_AN1(FO, DF, HD, 8); break; } } while (0)
  if (!has_delta) {
    if (f32out) LAUNCH_AN(true, false, false); else LAUNCH_AN(false, false, false);
  } else if (delta_f32) {
    if (f32out) LAUNCH_AN(true, true, true); else LAUNCH_AN(false, true, true);
  } else {
    if (f32out) LAUNCH_AN(true, false, true); else LAUNCH_AN(false, false, true);
  }
  #undef LAUNCH_AN
  #undef LAUNCH_AN1
  #undef LAUNCH_AN2
  HIP_CHECK_KERNEL();
}
