// Common helpers for room_amd CDNA4 (gfx950) kernels.
// Target: MI355X only — wave64, 256 CUs / 8 XCDs, LDS 160 KiB/CU, HBM3E 8 TB/s.
// No CUDA compatibility, no multi-arch dispatch.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <cstdint>

#define WAVE 64
#define DEV __device__ __forceinline__

// bf16 x8 = 16B vector load unit (coalescing sweet spot, guide G13)
typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) short bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) float f32x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;

DEV float bf2f(short u) {
  union { float f; uint32_t u32; } c;
  c.u32 = (uint32_t)(uint16_t)u << 16;
  return c.f;
}

DEV short f2bf(float f) {
  union { float f; uint32_t u32; } c;
  c.f = f;
  // round-to-nearest-even
  uint32_t lsb = (c.u32 >> 16) & 1;
  c.u32 += 0x7fff + lsb;
  return (short)(c.u32 >> 16);
}

// acc + Σ f_j² over one 8-vector, j ascending: the per-vector step of every
// RMSNorm row sum. Kernels that must agree bit for bit on a row's sum of
// squares (the norm kernels and the fusions that fold a norm into a GEMV) all
// take it from here. Each square is rounded before its add (no fma
// contraction), which is what the norm kernels have always compiled to.
DEV float sumsq8(float acc, bf16x8 v) {
  #pragma clang fp contract(off)
  #pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float f = bf2f(v[j]);
    acc += f * f;
  }
  return acc;
}

// acc + Σ w_j·x_j over one 8-vector, j ascending, each product rounded before
// its add: the router GEMV's step, shared by its plain and norm-fused kernels.
DEV float dot8_unfused(float acc, const float (&wf)[8], bf16x8 xv) {
  #pragma clang fp contract(off)
  #pragma unroll
  for (int j = 0; j < 8; ++j) acc += wf[j] * bf2f(xv[j]);
  return acc;
}

// full-wave sum reduction (64 lanes)
DEV float wave_reduce_sum(float v) {
  #pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    v += __shfl_xor(v, off, WAVE);
  return v;
}

// N independent full-wave sums in one interleaved butterfly: the N shuffles of
// a level are in flight together. Same xor pairing as wave_reduce_sum, so each
// v[i] gets the same bits as wave_reduce_sum(v[i]).
template <int N>
DEV void wave_reduce_sum_n(float (&v)[N]) {
  #pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    float o[N];
    #pragma unroll
    for (int i = 0; i < N; ++i) o[i] = __shfl_xor(v[i], off, WAVE);
    #pragma unroll
    for (int i = 0; i < N; ++i) v[i] += o[i];
  }
}

DEV float wave_reduce_max(float v) {
  #pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    v = fmaxf(v, __shfl_xor(v, off, WAVE));
  return v;
}

// block-level sum reduce across up to 16 waves; smem must be float[16]
DEV float block_reduce_sum(float v, float* smem) {
  int lane = threadIdx.x & (WAVE - 1);
  int wid = threadIdx.x / WAVE;
  v = wave_reduce_sum(v);
  if (lane == 0) smem[wid] = v;
  __syncthreads();
  int nw = (blockDim.x + WAVE - 1) / WAVE;
  v = (lane < nw) ? smem[lane] : 0.0f;
  v = wave_reduce_sum(v);
  return __shfl(v, 0, WAVE);
}

DEV float block_reduce_max(float v, float* smem) {
  int lane = threadIdx.x & (WAVE - 1);
  int wid = threadIdx.x / WAVE;
  v = wave_reduce_max(v);
  if (lane == 0) smem[wid] = v;
  __syncthreads();
  int nw = (blockDim.x + WAVE - 1) / WAVE;
  v = (lane < nw) ? smem[lane] : -INFINITY;
  v = wave_reduce_max(v);
  return __shfl(v, 0, WAVE);
}

#define HIP_CHECK_KERNEL() do { \
    hipError_t e = hipGetLastError(); \
    if (e != hipSuccess) { \
      TORCH_CHECK(false, "HIP kernel launch failed: ", hipGetErrorString(e)); \
    } \
  } while (0)
