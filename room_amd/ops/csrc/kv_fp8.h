// fp8 KV cache rows (ROOMAMD_KV_DTYPE=fp8): conversions shared by the writer
// (norm_rope.hip) and the three readers (paged_attn.hip, flash_prefill.hip).
//
// Format: a cached row is 128 OCP e4m3fn bytes plus one f32 scale, the power
// of two 2^e with e the smallest integer such that amax <= 448 * 2^e over the
// row's bf16 values (e >= -64; an all-zero row has scale 1.0). That is
// reference.quantize_kv_rows. Every q * scale is exactly a bf16 value, so a
// reader that converts on load sees the bits of the bf16 cache holding
// bf16(f32(q) * scale) (the "image") and runs the bf16 code unchanged.
#pragma once

#include "common.h"

#define KV_FP8_MIN_EXP (-64)

// (The wrapper-side check of the four ops is kv_fp8_check in checks.h.)

// Row scale from the row's largest |bf16| bit pattern (0..0x7f7f), in integer
// arithmetic. amax = 1.m * 2^(be - 127) and 448 = 1.75 * 2^8, so
// e = be - 135, plus one when the mantissa is above .75 (7 bits: 0x60).
// Subnormal rows (be = 0) land far below the clamp. Returns e.
DEV int kv_fp8_scale_exp(uint32_t amax_bf16_bits) {
  if (amax_bf16_bits == 0) return 0;
  const int be = (int)(amax_bf16_bits >> 7);
  const int e = be - 135 + ((amax_bf16_bits & 0x7f) > 0x60 ? 1 : 0);
  return max(e, KV_FP8_MIN_EXP);
}

// 2^e as f32 for -126 <= e <= 127
DEV float kv_fp8_exp2i(int e) {
  return __builtin_bit_cast(float, (uint32_t)(e + 127) << 23);
}

// One bf16 value of a row with scale 2^e -> its e4m3 byte (round to nearest
// even; |x * 2^-e| <= 448, so nothing saturates).
DEV uint8_t kv_fp8_quantize(short x_bf16, int e) {
  const float v = bf2f(x_bf16) * kv_fp8_exp2i(-e);
  return (uint8_t)(__builtin_amdgcn_cvt_pk_fp8_f32(v, v, 0, false) & 0xff);
}

// The writer's row step for a 128-thread workgroup, thread i holding element
// i of the row as bf16: block max of |o| (on the bit patterns, which order
// like the values), the scale, one byte per thread, and the scale from
// thread 0. smem: uint32_t[2].
DEV void kv_fp8_store_row(uint8_t* __restrict__ row, float* __restrict__ scale,
                          short o, uint32_t* smem) {
  uint32_t a = (uint32_t)o & 0x7fffu;
  #pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    a = max(a, (uint32_t)__shfl_xor((int)a, off, WAVE));
  if ((threadIdx.x & (WAVE - 1)) == 0) smem[threadIdx.x / WAVE] = a;
  __syncthreads();
  const int e = kv_fp8_scale_exp(max(smem[0], smem[1]));
  row[threadIdx.x] = kv_fp8_quantize(o, e);
  if (threadIdx.x == 0) *scale = kv_fp8_exp2i(e);
}

typedef __attribute__((ext_vector_type(4))) uint32_t kv_u32x4;
typedef __attribute__((ext_vector_type(2))) uint32_t kv_u32x2;

// Two e4m3 bytes (the low or the high half of w) times s -> two bf16 in one
// dword, the lower byte in the low half.
template <bool HI>
DEV uint32_t kv_fp8x2_to_bf16(uint32_t w, float s) {
  return __builtin_bit_cast(
      uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, s, HI));
}

// Four / eight consecutive bytes of one row times the row's scale -> the
// image's bf16 values, in order.
DEV kv_u32x2 kv_fp8x4_to_bf16(uint32_t w, float s) {
  return kv_u32x2{kv_fp8x2_to_bf16<false>(w, s), kv_fp8x2_to_bf16<true>(w, s)};
}

DEV kv_u32x4 kv_fp8x8_to_bf16(kv_u32x2 w, float s) {
  return kv_u32x4{kv_fp8x2_to_bf16<false>(w[0], s),
                  kv_fp8x2_to_bf16<true>(w[0], s),
                  kv_fp8x2_to_bf16<false>(w[1], s),
                  kv_fp8x2_to_bf16<true>(w[1], s)};
}
