// FP8 expert weights for decode on CDNA4 (gfx950): the fp8 twins of
// moe_gemv_h / moe_gemv_down (moe.hip) and of the grouped launch of
// skinny_gemm_kernel (skinny_gemm.hip).
//
// Format: weights are OCP e4m3fn (gfx950's native fp8, not fnuz), one byte per
// element in the bf16 layouts ([E, 2I, H] and [E, H, I], rows contiguous over
// k), with one f32 scale per 128x128 block: scale[e][n/128][k/128]. Any
// positive finite scale is accepted.
//
// Numeric contract (all three kernels): a weight byte is converted to f32 or
// bf16 UNSCALED (both conversions are exact), products x*q accumulate in f32,
// and the block scale multiplies the f32 partial sum of its k-block:
//   out = sum_blocks s_b * sum_{k in b} x_k q_k.
// Activations stay bf16; no fp8 MFMA (that would quantise x).
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include "common.h"
#include "checks.h"

typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;

#define FP8_BLK 128   // scale block edge, in n and in k

// 16 fp8 (one 16-B load) dotted with 16 bf16 (two 16-B loads), unscaled.
// v_cvt_pk_f32_fp8 turns two bytes of a word into two f32.
DEV float dot16_fp8(const i32x4 q, const bf16x8 x0, const bf16x8 x1) {
  float s = 0.f;
  #pragma unroll
  for (int w = 0; w < 4; ++w) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(q[w], false);
    const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8(q[w], true);
    const bf16x8& xv = (w < 2) ? x0 : x1;
    const int b = (w & 1) * 4;
    s += bf2f(xv[b + 0]) * lo[0];
    s += bf2f(xv[b + 1]) * lo[1];
    s += bf2f(xv[b + 2]) * hi[0];
    s += bf2f(xv[b + 3]) * hi[1];
  }
  return s;
}

// gate and up rows against the same x: x converted once
DEV void dot16x2_fp8(float& pg, float& pu, const i32x4 g, const i32x4 u,
                     const bf16x8 x0, const bf16x8 x1) {
  pg = 0.f; pu = 0.f;
  #pragma unroll
  for (int w = 0; w < 4; ++w) {
    const f32x2 gl = __builtin_amdgcn_cvt_pk_f32_fp8(g[w], false);
    const f32x2 gh = __builtin_amdgcn_cvt_pk_f32_fp8(g[w], true);
    const f32x2 ul = __builtin_amdgcn_cvt_pk_f32_fp8(u[w], false);
    const f32x2 uh = __builtin_amdgcn_cvt_pk_f32_fp8(u[w], true);
    const bf16x8& xv = (w < 2) ? x0 : x1;
    const int b = (w & 1) * 4;
    const float a0 = bf2f(xv[b + 0]), a1 = bf2f(xv[b + 1]);
    const float a2 = bf2f(xv[b + 2]), a3 = bf2f(xv[b + 3]);
    pg += a0 * gl[0]; pu += a0 * ul[0];
    pg += a1 * gl[1]; pu += a1 * ul[1];
    pg += a2 * gh[0]; pu += a2 * uh[0];
    pg += a3 * gh[1]; pu += a3 * uh[1];
  }
}

// ---------------------------------------------------------------- GEMV path
// h[p][j] = silu(dot(x_t, Wg_row_j)) * dot(x_t, Wu_row_j), fp8 rows.
// Grid, wave-per-output shape, out_zero side job and epilogue of
// moe_gemv_h_kernel. A row is H bytes: a lane loads 16 B = 16 k per
// iteration, a wave 1024 k; a lane's 16 k lie inside one 128-block, so it
// scales its own 16-product sum before adding it to the running dot. The gate
// row j and the up row I+j lie in different N-blocks: two scales per k-block.
// NIT = H/1024 when known at compile time (2 for the model): every load of
// the row pair, scales included, is issued before the first FMA. 0 = any
// multiple of 128; lanes past the row's end (H = 512: lanes 32..63) idle.
template <int NIT>
__global__ __launch_bounds__(256)
void moe_gemv_h_fp8_kernel(short* __restrict__ h,              // [P, I]
                           const short* __restrict__ x,         // [T, H]
                           const uint8_t* __restrict__ w13,     // [E, 2I, H]
                           const float* __restrict__ w13_s,     // [E, 2I/128, H/128]
                           const int* __restrict__ pair_token,  // [P]
                           const int* __restrict__ pair_expert, // [P]
                           float* __restrict__ out_zero,        // [zero_n] or null
                           long zero_n, int H, int I) {
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
  const int KB = H / FP8_BLK, NB = 2 * I / FP8_BLK;
  const short* xrow = x + (long)t * H;
  const uint8_t* grow = w13 + ((long)e * 2 * I + j) * H;
  const uint8_t* urow = w13 + ((long)e * 2 * I + I + j) * H;
  const float* gs = w13_s + ((long)e * NB + j / FP8_BLK) * KB;
  const float* us = w13_s + ((long)e * NB + (I + j) / FP8_BLK) * KB;

  float dg = 0.f, du = 0.f;
  if constexpr (NIT > 0) {
    i32x4 gv[NIT], uv[NIT];
    bf16x8 xv[NIT][2];
    float sg[NIT], su[NIT];
    #pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int base = lane * 16 + it * WAVE * 16;
      gv[it] = *reinterpret_cast<const i32x4*>(grow + base);
      uv[it] = *reinterpret_cast<const i32x4*>(urow + base);
      xv[it][0] = *reinterpret_cast<const bf16x8*>(xrow + base);
      xv[it][1] = *reinterpret_cast<const bf16x8*>(xrow + base + 8);
      sg[it] = gs[base / FP8_BLK];
      su[it] = us[base / FP8_BLK];
    }
    __builtin_amdgcn_sched_barrier(0);   // keep the loads ahead of the FMAs
    #pragma unroll
    for (int it = 0; it < NIT; ++it) {
      float pg, pu;
      dot16x2_fp8(pg, pu, gv[it], uv[it], xv[it][0], xv[it][1]);
      dg += sg[it] * pg;
      du += su[it] * pu;
    }
  } else {
    for (int base = lane * 16; base < H; base += WAVE * 16) {
      const i32x4 gv = *reinterpret_cast<const i32x4*>(grow + base);
      const i32x4 uv = *reinterpret_cast<const i32x4*>(urow + base);
      const bf16x8 x0 = *reinterpret_cast<const bf16x8*>(xrow + base);
      const bf16x8 x1 = *reinterpret_cast<const bf16x8*>(xrow + base + 8);
      const float sg = gs[base / FP8_BLK], su = us[base / FP8_BLK];
      float pg, pu;
      dot16x2_fp8(pg, pu, gv, uv, x0, x1);
      dg += sg * pg;
      du += su * pu;
    }
  }
  dg = wave_reduce_sum(dg);
  du = wave_reduce_sum(du);
  if (lane == 0) {
    float s = dg / (1.0f + __expf(-dg));
    h[(long)p * I + j] = f2bf(s * du);
  }
}

// z[t] += w_p * (h_p @ W2_e^T), fp8 rows: the 16-lanes-per-output shape and
// the f32 atomicAdd combine of moe_gemv_down_kernel. A row is I bytes: the 16
// lanes of an output cover 256 k per iteration, 16 k each.
// NIT = I/256 when known at compile time (3 for the model); 0 = any multiple
// of 128 (I = 128: lanes 8..15 of a group idle).
template <int NIT>
__global__ __launch_bounds__(256)
void moe_gemv_down_fp8_kernel(float* __restrict__ out,          // [T, H] f32
                              const short* __restrict__ h,       // [P, I]
                              const uint8_t* __restrict__ w2,    // [E, H, I]
                              const float* __restrict__ w2_s,    // [E, H/128, I/128]
                              const float* __restrict__ pair_w,  // [P]
                              const int* __restrict__ pair_token,
                              const int* __restrict__ pair_expert,
                              int H, int I) {
  const int p = blockIdx.x;
  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int grp = lane >> 4;       // output within the wave
  const int sub = lane & 15;       // 16 lanes per output
  const int o = (blockIdx.y * 4 + wid) * 4 + grp;
  if (o >= H) return;
  const int t = pair_token[p];
  const int e = pair_expert[p];
  const int KB = I / FP8_BLK;
  const short* hrow = h + (long)p * I;
  const uint8_t* wrow = w2 + ((long)e * H + o) * I;
  const float* ws = w2_s + ((long)e * (H / FP8_BLK) + o / FP8_BLK) * KB;

  float d = 0.f;
  if constexpr (NIT > 0) {
    i32x4 wv[NIT];
    bf16x8 hv[NIT][2];
    float sc[NIT];
    #pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int base = sub * 16 + it * 16 * 16;
      wv[it] = *reinterpret_cast<const i32x4*>(wrow + base);
      hv[it][0] = *reinterpret_cast<const bf16x8*>(hrow + base);
      hv[it][1] = *reinterpret_cast<const bf16x8*>(hrow + base + 8);
      sc[it] = ws[base / FP8_BLK];
    }
    __builtin_amdgcn_sched_barrier(0);   // keep the loads ahead of the FMAs
    #pragma unroll
    for (int it = 0; it < NIT; ++it)
      d += sc[it] * dot16_fp8(wv[it], hv[it][0], hv[it][1]);
  } else {
    for (int base = sub * 16; base < I; base += 16 * 16) {
      const i32x4 wv = *reinterpret_cast<const i32x4*>(wrow + base);
      const bf16x8 h0 = *reinterpret_cast<const bf16x8*>(hrow + base);
      const bf16x8 h1 = *reinterpret_cast<const bf16x8*>(hrow + base + 8);
      d += ws[base / FP8_BLK] * dot16_fp8(wv, h0, h1);
    }
  }
  #pragma unroll
  for (int off = 8; off > 0; off >>= 1) d += __shfl_xor(d, off, WAVE);
  if (sub == 0)
    atomicAdd(out + (long)t * H + o, d * pair_w[p]);
}

// ------------------------------------------- grouped skinny MFMA GEMM, fp8 w
// The grouped launch of skinny_gemm_kernel (MF = 1, NW = 4 waves splitting K,
// 16-row tiles from a [G,3] descriptor) with fp8 weights: HBM -> VGPR ->
// v_cvt_scalef32_pk_bf16_fp8 (scale 1.0: exact) -> mfma_f32_16x16x32_bf16.
// No LDS in the main loop; wave partials summed through LDS in wave order.
//
// A workgroup owns NF = 2 adjacent 16-column fragments of one tile (32
// columns). At one byte per weight the x operand is two thirds of what a
// one-fragment workgroup pulls into its registers; two fragments share each
// x load and put twice the weight bytes in flight per workgroup (measured
// 59 -> 53 us gate/up, 33 -> 28 us down at 16 rows; profiles/PERF_NOTES.md).
//
// K is cut into CK = 128 wide chunks (one 128-B line of every weight row);
// wave v owns chunks v, v+4, v+8, ... ascending. A chunk is exactly one
// 128-wide scale block and the workgroup's 32 columns lie inside one 128-tall
// one, so a chunk's scale is wave-uniform: the chunk's MFMAs accumulate from
// zero and the scaled chunk sum is added to the running accumulator,
// acc += s * chunk.
//
// k-permutation (both operands): inside a chunk the 16-lane group g owns the
// CK/4 consecutive k [g*CK/4, (g+1)*CK/4) — CK/4 weight bytes per fragment,
// CK/2 x bytes per lane — and feeds CK/32 MFMAs per fragment, elements
// 8i..8i+7 to the i-th.
//
// Row independence: chunk ownership, accumulation order and the partial
// order (p0+p1)+p2+p3 depend on K alone; U only batches loads.
//
// Only <CK = 128, NF = 2> is instantiated: CK = 64 (the bf16 kernel's chunk
// count) and NF = 1 were each measured slower at the model's shapes.
template <int CK, int NF>
struct Fp8Chunk {
  static constexpr int NQ = CK / 64;    // 16-B weight loads per lane and row
  static constexpr int NM = CK / 32;    // MFMAs per fragment, 16-B x loads
  i32x4 w[NF][NQ];
  bf16x8 x[NM];
};

// wp: the lane's row of fragment 0; fragment f's row lies 16 rows (fstride
// bytes) further
template <int CK, int NF>
DEV void fp8_chunk_load(Fp8Chunk<CK, NF>& c, const uint8_t* wp, long fstride,
                        const short* xp) {
  #pragma unroll
  for (int f = 0; f < NF; ++f)
    #pragma unroll
    for (int q = 0; q < Fp8Chunk<CK, NF>::NQ; ++q)
      c.w[f][q] = *reinterpret_cast<const i32x4*>(wp + f * fstride + q * 16);
  #pragma unroll
  for (int m = 0; m < Fp8Chunk<CK, NF>::NM; ++m)
    c.x[m] = *reinterpret_cast<const bf16x8*>(xp + m * 8);
}

// 8 fp8 (two words) -> 8 bf16, unscaled
DEV bf16x8 fp8x8_to_bf16(int w0, int w1) {
  i32x4 r;
  r[0] = __builtin_bit_cast(int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, false));
  r[1] = __builtin_bit_cast(int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, true));
  r[2] = __builtin_bit_cast(int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, false));
  r[3] = __builtin_bit_cast(int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, true));
  return __builtin_bit_cast(bf16x8, r);
}

template <int CK, int NF>
DEV void fp8_chunk_mma(f32x4 (&acc)[NF], const Fp8Chunk<CK, NF>& c, float s) {
  #pragma unroll
  for (int f = 0; f < NF; ++f) {
    f32x4 part = f32x4{0.f, 0.f, 0.f, 0.f};
    #pragma unroll
    for (int m = 0; m < Fp8Chunk<CK, NF>::NM; ++m) {
      const i32x4 q = c.w[f][m / 2];
      const bf16x8 a = (m & 1) ? fp8x8_to_bf16(q[2], q[3])
                               : fp8x8_to_bf16(q[0], q[1]);
      part = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, c.x[m], part, 0, 0, 0);
    }
    #pragma unroll
    for (int r = 0; r < 4; ++r) acc[f][r] += s * part[r];
  }
}

#define SKF_NW 4     // waves per workgroup (the K split)
#define SKF_CK 128   // k-chunk width
#define SKF_NF 2     // 16-column fragments per workgroup

template <int CK, int U, int NF>
__global__ __launch_bounds__(SKF_NW * 64)
void skinny_gemm_fp8_kernel(void* __restrict__ out,             // [rows, N]
                            const short* __restrict__ x,         // [T, K]
                            const uint8_t* __restrict__ w,       // [E, N, K]
                            const float* __restrict__ w_s,       // [E, N/128, K/128]
                            const int* __restrict__ pair_token,  // [rows]
                            const int* __restrict__ tile_desc,   // [G,3]
                            int K, int N, int f32out) {
  // cross-wave reduction buffer: the kernel's only LDS
  __shared__ f32x4 red[SKF_NW * NF * 64];

  const int g = blockIdx.y;
  const int msize = tile_desc[g * 3 + 2];
  if (msize == 0) return;               // past the live tile count
  const int e = tile_desc[g * 3 + 0];
  const int row0 = tile_desc[g * 3 + 1];
  const int n0 = blockIdx.x * 16 * NF;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int fr = lane & 15;             // A row (n) / B column (m)
  const int fg = lane >> 4;             // 16-lane group: k [fg*CK/4, +CK/4)
  const int C = K / CK;                 // chunks
  constexpr int KPL = CK / 4;           // k per lane per chunk

  const uint8_t* wrow = w + ((long)e * N + n0 + fr) * K + fg * KPL;
  const float* srow = w_s + ((long)e * (N / FP8_BLK) + n0 / FP8_BLK)
                            * (K / FP8_BLK);
  const int m_ld = min(fr, msize - 1);  // rows >= msize re-read the last row
  const short* xrow = x + (long)pair_token[row0 + m_ld] * K + fg * KPL;

  f32x4 acc[NF];
  #pragma unroll
  for (int f = 0; f < NF; ++f) acc[f] = f32x4{0.f, 0.f, 0.f, 0.f};
  const long fstride = 16L * K;
  int c = wid;
  // groups of U chunks: every load of the group issued before its first MFMA
  for (; c + (U - 1) * SKF_NW < C; c += U * SKF_NW) {
    Fp8Chunk<CK, NF> ch[U];
    float sc[U];
    #pragma unroll
    for (int u = 0; u < U; ++u) {
      const long ko = (long)(c + u * SKF_NW) * CK;
      fp8_chunk_load<CK, NF>(ch[u], wrow + ko, fstride, xrow + ko);
      sc[u] = srow[ko / FP8_BLK];
    }
    __builtin_amdgcn_sched_barrier(0);   // keep the loads ahead of the MFMAs
    #pragma unroll
    for (int u = 0; u < U; ++u) fp8_chunk_mma<CK, NF>(acc, ch[u], sc[u]);
  }
  // remaining chunks one at a time (same ascending order)
  for (; c < C; c += SKF_NW) {
    const long ko = (long)c * CK;
    Fp8Chunk<CK, NF> ch;
    fp8_chunk_load<CK, NF>(ch, wrow + ko, fstride, xrow + ko);
    fp8_chunk_mma<CK, NF>(acc, ch, srow[ko / FP8_BLK]);
  }

  // cross-wave reduction through LDS, fixed order (p0+p1)+p2+p3
  #pragma unroll
  for (int f = 0; f < NF; ++f) red[(wid * NF + f) * 64 + lane] = acc[f];
  __syncthreads();
  if (wid < NF) {                       // wave f finishes fragment f
    f32x4 s = red[wid * 64 + lane];
    #pragma unroll
    for (int v = 1; v < SKF_NW; ++v) s += red[(v * NF + wid) * 64 + lane];
    if (fr < msize) {
      const long o = (long)(row0 + fr) * N + n0 + wid * 16 + fg * 4;
      if (f32out) {
        *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(out) + o) = s;
      } else {
        bf16x4 b;
        #pragma unroll
        for (int r = 0; r < 4; ++r) b[r] = f2bf(s[r]);
        *reinterpret_cast<bf16x4*>(reinterpret_cast<short*>(out) + o) = b;
      }
    }
  }
}

// ---------------------------------------------------------------- wrappers

void moe_gemv_h_fp8(torch::Tensor h, torch::Tensor x, torch::Tensor w13_q,
                    torch::Tensor w13_s, torch::Tensor pair_token,
                    torch::Tensor pair_expert, torch::Tensor out_zero) {
  OpChecks c("moe_gemv_h_fp8");
  moe_gemv_h_check(c, h, x, pair_token, pair_expert, out_zero);
  const int64_t P = h.size(0), H = x.size(1), I = h.size(1);
  c.require(P >= 1, "h holds no row");
  c.size_multiple("h", h, 1, FP8_BLK);
  c.size_multiple("x", x, 1, FP8_BLK);
  fp8_check_weights(c, "w13_q", w13_q, "w13_s", w13_s, 2 * I, H);
  if (check_only()) return;
  dim3 grid(P, (I + 3) / 4), block(256);
  const bool zero = out_zero.defined() && out_zero.numel() > 0;
  float* zp = zero ? out_zero.data_ptr<float>() : nullptr;
  const long zn = zero ? out_zero.numel() : 0;
  hipStream_t s = c10::hip::getCurrentHIPStream();
  #define MOE_H8_GO(NIT) hipLaunchKernelGGL( \
      moe_gemv_h_fp8_kernel<NIT>, grid, block, 0, s, (short*)h.data_ptr(), \
      (const short*)x.data_ptr(), (const uint8_t*)w13_q.data_ptr(), \
      w13_s.data_ptr<float>(), pair_token.data_ptr<int>(), \
      pair_expert.data_ptr<int>(), zp, zn, (int)H, (int)I)
  if (H == 2 * WAVE * 16) MOE_H8_GO(2); else MOE_H8_GO(0);
  #undef MOE_H8_GO
  HIP_CHECK_KERNEL();
}

void moe_gemv_down_fp8(torch::Tensor out, torch::Tensor h, torch::Tensor w2_q,
                       torch::Tensor w2_s, torch::Tensor pair_w,
                       torch::Tensor pair_token, torch::Tensor pair_expert) {
  OpChecks c("moe_gemv_down_fp8");
  moe_gemv_down_check(c, out, h, pair_w, pair_token, pair_expert);
  const int64_t P = h.size(0), H = out.size(1), I = h.size(1);
  c.require(P >= 1, "h holds no row");
  c.size_multiple("out", out, 1, FP8_BLK);
  fp8_check_weights(c, "w2_q", w2_q, "w2_s", w2_s, H, I);
  if (check_only()) return;
  dim3 grid(P, (H + 15) / 16), block(256);   // 16 outputs per WG
  hipStream_t s = c10::hip::getCurrentHIPStream();
  #define MOE_DOWN8_GO(NIT) hipLaunchKernelGGL( \
      moe_gemv_down_fp8_kernel<NIT>, grid, block, 0, s, out.data_ptr<float>(), \
      (const short*)h.data_ptr(), (const uint8_t*)w2_q.data_ptr(), \
      w2_s.data_ptr<float>(), pair_w.data_ptr<float>(), \
      pair_token.data_ptr<int>(), pair_expert.data_ptr<int>(), (int)H, (int)I)
  if (I == 3 * 16 * 16) MOE_DOWN8_GO(3); else MOE_DOWN8_GO(0);
  #undef MOE_DOWN8_GO
  HIP_CHECK_KERNEL();
}

namespace {

template <int CK, int U, int NF>
void skf_launch(void* out, const short* x, const uint8_t* w, const float* ws,
                const int* pt, const int* desc, int G, int K, int N,
                int f32out, hipStream_t s) {
  dim3 grid(N / (16 * NF), G), block(SKF_NW * 64);
  hipLaunchKernelGGL((skinny_gemm_fp8_kernel<CK, U, NF>), grid, block, 0, s, out,
                     x, w, ws, pt, desc, K, N, f32out);
}

// U: the largest load group that divides a wave's chunk count (from K alone)
void skf_dispatch_u(void* out, const short* x, const uint8_t* w,
                    const float* ws, const int* pt, const int* desc, int G,
                    int K, int N, int f32out, hipStream_t s) {
  const int cpw = (K / SKF_CK + SKF_NW - 1) / SKF_NW;
  #define SKF_GO(U) skf_launch<SKF_CK, U, SKF_NF>(out, x, w, ws, pt, desc, G, \
                                                  K, N, f32out, s)
  if (cpw % 4 == 0) { SKF_GO(4); return; }
  if (cpw % 3 == 0) { SKF_GO(3); return; }
  if (cpw % 2 == 0) { SKF_GO(2); return; }
  SKF_GO(1);
  #undef SKF_GO
}

}  // namespace

// grouped, BM=16 tiles (tile_desc from moe_build_desc with bm=16)
void moe_grouped_gemm_skinny_fp8(torch::Tensor out, torch::Tensor x,
                                 torch::Tensor w_q, torch::Tensor w_s,
                                 torch::Tensor pair_token,
                                 torch::Tensor tile_desc) {
  OpChecks c("moe_grouped_gemm_skinny_fp8");
  grouped_gemm_check(c, true, out, x, pair_token, tile_desc);
  const int64_t K = x.size(1), N = out.size(1), G = tile_desc.size(0);
  fp8_check_weights(c, "w_q", w_q, "w_s", w_s, N, K);
  if (check_only()) return;
  hipStream_t s = c10::hip::getCurrentHIPStream();
  const int f32out = out.dtype() == torch::kFloat32;
  skf_dispatch_u(out.data_ptr(), (const short*)x.data_ptr(),
                 (const uint8_t*)w_q.data_ptr(), w_s.data_ptr<float>(),
                 pair_token.data_ptr<int>(), tile_desc.data_ptr<int>(),
                 (int)G, (int)K, (int)N, f32out, s);
  HIP_CHECK_KERNEL();
}

// ------------------------------------------------ prefill grouped GEMM, fp8 w
// BM=128 tiles (tile_desc from moe_build_desc with bm=128). The kernel is the
// W8 instantiation of moe_grouped_gemm128_kernel in moe.hip, which shares the
// bf16 kernel's MFMA loop. Its numeric contract is NOT the one at the top of
// this file: the scale is applied to the weight, bf16_rne(f32(q) * s), while
// the tile is staged, so the result equals moe_grouped_gemm128 on
// dequantize_fp8_block(w_q, w_s).to(bf16) bit for bit.
void moe_grouped_gemm128_fp8_launch(short* out, const short* x,
                                    const uint8_t* w_q, const float* w_s,
                                    const int* pair_token, const int* tile_desc,
                                    int G, int H, int N, hipStream_t s);

void moe_grouped_gemm128_fp8(torch::Tensor out, torch::Tensor x,
                             torch::Tensor w_q, torch::Tensor w_s,
                             torch::Tensor pair_token,
                             torch::Tensor tile_desc) {
  OpChecks c("moe_grouped_gemm128_fp8");
  grouped_gemm_check(c, false, out, x, pair_token, tile_desc);
  const int64_t K = x.size(1), N = out.size(1), G = tile_desc.size(0);
  c.require(G >= 1, "tile_desc holds no tile");
  fp8_check_weights(c, "w_q", w_q, "w_s", w_s, N, K);
  if (check_only()) return;
  hipStream_t s = c10::hip::getCurrentHIPStream();
  moe_grouped_gemm128_fp8_launch(
      (short*)out.data_ptr(), (const short*)x.data_ptr(),
      (const uint8_t*)w_q.data_ptr(), w_s.data_ptr<float>(),
      pair_token.data_ptr<int>(), tile_desc.data_ptr<int>(), (int)G, (int)K,
      (int)N, s);
  HIP_CHECK_KERNEL();
}
