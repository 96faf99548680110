// Memory-encoder kernels (MiniEncoder impl="hip") for CDNA4 (gfx950).
//
// The encoder is a 6-layer pre-RMSNorm transformer: 384 dim, 12 heads of 32,
// FFN 1536, at most 128 pieces per text. The forward runs on rows of all texts
// packed without padding; cu_rows [B+1] holds the cumulative row offsets, text
// b owns rows [cu_rows[b], cu_rows[b+1]). The projections run on
// moe_grouped_gemm_skinny and the norms on rmsnorm / fused_add_rmsnorm; this
// file holds the rest:
//
//   encoder_embed      input rows: sparse ±0.5 hash features + position row
//   encoder_attention  bidirectional softmax attention inside each segment
//   gelu_              exact (erf) GELU in place
//   encoder_pool       segment mean, centring, L2 normalisation
//
// Batch invariance: every kernel here works on one segment (or one row) at a
// time, reads no row outside it, and reduces in an order fixed by the
// segment's own length. A text's result therefore has the same bits alone, in
// any batch and at any place in the pack.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include "common.h"
#include "checks.h"

#define ENC_DIM 384
#define ENC_HEADS 12
#define ENC_HD 32                 // head dim: one k-step of mfma 16x16x32
#define ENC_QKV (3 * ENC_DIM)
#define ENC_MAXLEN 128            // pieces per text: 8 key tiles of 16
#define ENC_VPAD 8                // bf16 padding of a V^T row in LDS

// ---------------------------------------------------------------- embed
// x[r][c] = Σ_k (feats[r][k] >> 1 == c ? ±0.5 : 0) + pos_table[pos_ids[r]][c].
// A feature packs (index << 1) | (1 for +0.5, 0 for -0.5); features that share
// an index accumulate. Sums of ±0.5 are exact in f32, so the row is one f32
// add and one rounding away from the table. One wave per row, 8 columns per
// lane (48 lanes busy).
__global__ __launch_bounds__(256)
void encoder_embed_kernel(short* __restrict__ x,             // [R, 384]
                          const int* __restrict__ feats,      // [R, 4]
                          const int* __restrict__ pos_ids,    // [R]
                          const float* __restrict__ pos_table,  // [P, 384]
                          int R, int P) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= R || lane >= ENC_DIM / 8) return;
  const int c0 = lane * 8;
  int f[4];
  #pragma unroll
  for (int k = 0; k < 4; ++k) f[k] = feats[(long)row * 4 + k];
  const int pos = min(max(pos_ids[row], 0), P - 1);
  const float* prow = pos_table + (long)pos * ENC_DIM + c0;
  const f32x4 p0 = *reinterpret_cast<const f32x4*>(prow);
  const f32x4 p1 = *reinterpret_cast<const f32x4*>(prow + 4);
  bf16x8 o;
  #pragma unroll
  for (int j = 0; j < 8; ++j) {
    float v = 0.f;
    #pragma unroll
    for (int k = 0; k < 4; ++k)
      if ((f[k] >> 1) == c0 + j) v += (f[k] & 1) ? 0.5f : -0.5f;
    o[j] = f2bf(v + (j < 4 ? p0[j] : p1[j - 4]));
  }
  *reinterpret_cast<bf16x8*>(x + (long)row * ENC_DIM + c0) = o;
}

// ---------------------------------------------------------------- attention
// One workgroup per (text, head), 4 waves; wave w takes the 16-row query tiles
// w and w + 4. Fragment layouts: above moe_grouped_gemm128_kernel (moe.hip).
//
//   V^T     the head's V is staged once per workgroup as vt[dim][key] in LDS
//           (8.5 KiB), keys >= len zero, so a masked p = 0 never meets a
//           foreign or non-finite value. The only barrier follows it.
//   scores  S^T[key][q] = K_tile · Q^T, one mfma_f32_16x16x32_bf16 per 16-key
//           tile (head dim 32 = one k-step). A comes straight from qkv: lane
//           (n, g) reads 16 B of key row n; B is the query tile, lane (n, g)
//           reads 16 B of query row n. Accumulator t holds
//           S[key 16t + 4g + r][query n] in register r: a query's whole score
//           row (8 accumulators) lives in the registers of the four lanes
//           n, n+16, n+32, n+48.
//   softmax exact two-pass form. Keys >= len are set to -inf before the max;
//           max and sum run over the 32 registers in index order, then over g
//           (shuffles xor 16, xor 32).
//   P·V     O^T[dim][q] += V^T · P, k = the 32 keys of two score tiles: k-slot
//           8g + j is key 32p + 4g + j for j < 4 and key 32p + 16 + 4g + j - 4
//           for j >= 4, which for the B operand are exactly the registers of
//           accumulators 2p and 2p + 1 (the paged_attn_split_kernel trick).
//           The A operand is two 8-B LDS reads of vt[dim n (+16)].
//           acc[dt][r] = O[query n][dim 16 dt + 4g + r].
// Rows past the segment's end re-read its last row (clamped index): such
// query columns are never stored and such keys are masked, so no row outside
// the segment is ever read.
__global__ __launch_bounds__(256)
void encoder_attention_kernel(short* __restrict__ out,        // [R, 384]
                              const short* __restrict__ qkv,   // [R, 1152]
                              const int* __restrict__ cu_rows,  // [B+1]
                              int R, float scale) {
  const int b = blockIdx.x;
  const int h = blockIdx.y;
  const int row0 = cu_rows[b];
  const int len = min(cu_rows[b + 1] - row0, ENC_MAXLEN);
  // host-checked; a bad descriptor must still never leave the buffers
  if (len <= 0 || row0 < 0 || row0 + len > R) return;

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int n = lane & 15;
  const int g = lane >> 4;

  __shared__ __attribute__((aligned(16))) short vt[ENC_HD][ENC_MAXLEN + ENC_VPAD];

  const short* base = qkv + (long)row0 * ENC_QKV + h * ENC_HD;
  #pragma unroll
  for (int it = 0; it < ENC_MAXLEN * 4 / 256; ++it) {
    const int i = tid + it * 256;
    const int key = i >> 2, c = i & 3;
    bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (key < len)
      v = *reinterpret_cast<const bf16x8*>(
          base + (long)key * ENC_QKV + 2 * ENC_DIM + c * 8);
    #pragma unroll
    for (int j = 0; j < 8; ++j) vt[c * 8 + j][key] = v[j];
  }
  __syncthreads();

  const int nqt = (len + 15) >> 4;
  for (int qt = wave; qt < nqt; qt += 4) {
    const int qrow = min(qt * 16 + n, len - 1);
    const bf16x8 qf = *reinterpret_cast<const bf16x8*>(
        base + (long)qrow * ENC_QKV + g * 8);

    f32x4 s[ENC_MAXLEN / 16];
    #pragma unroll
    for (int t = 0; t < ENC_MAXLEN / 16; ++t) {
      s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (t * 16 < len) {                       // wave-uniform
        const int krow = min(t * 16 + n, len - 1);
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(
            base + (long)krow * ENC_QKV + ENC_DIM + g * 8);
        s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf, s[t], 0, 0, 0);
      }
    }

    float m = -INFINITY;
    #pragma unroll
    for (int t = 0; t < ENC_MAXLEN / 16; ++t) {
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[t][r] = (t * 16 + 4 * g + r < len) ? s[t][r] * scale : -INFINITY;
        m = fmaxf(m, s[t][r]);
      }
    }
    m = fmaxf(m, __shfl_xor(m, 16, WAVE));
    m = fmaxf(m, __shfl_xor(m, 32, WAVE));     // key 0 is valid: m is finite

    float l = 0.f;
    #pragma unroll
    for (int t = 0; t < ENC_MAXLEN / 16; ++t) {
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[t][r] = __expf(s[t][r] - m);          // masked keys: exactly 0
        l += s[t][r];
      }
    }
    l += __shfl_xor(l, 16, WAVE);
    l += __shfl_xor(l, 32, WAVE);

    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    #pragma unroll
    for (int p = 0; p < ENC_MAXLEN / 32; ++p) {
      if (p * 32 < len) {                       // wave-uniform
        bf16x8 pf;
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          pf[r] = f2bf(s[2 * p][r]);
          pf[4 + r] = f2bf(s[2 * p + 1][r]);
        }
        #pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          const short* vrow = &vt[dt * 16 + n][p * 32 + 4 * g];
          const bf16x4 a0 = *reinterpret_cast<const bf16x4*>(vrow);
          const bf16x4 a1 = *reinterpret_cast<const bf16x4*>(vrow + 16);
          const bf16x8 af = {a0[0], a0[1], a0[2], a0[3],
                             a1[0], a1[1], a1[2], a1[3]};
          acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, pf, acc[dt],
                                                            0, 0, 0);
        }
      }
    }

    if (qt * 16 + n < len) {
      const float inv = 1.f / l;
      short* orow = out + (long)(row0 + qt * 16 + n) * ENC_DIM + h * ENC_HD
                    + 4 * g;
      #pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        bf16x4 o;
        #pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = f2bf(acc[dt][r] * inv);
        *reinterpret_cast<bf16x4*>(orow + dt * 16) = o;
      }
    }
  }
}

// ---------------------------------------------------------------- gelu
// u = 0.5 u (1 + erf(u / sqrt 2)) in place, 8 values per lane.
__global__ __launch_bounds__(256)
void gelu_kernel(short* __restrict__ u, long nvec) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nvec) return;
  bf16x8 v = *reinterpret_cast<const bf16x8*>(u + i * 8);
  #pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float f = bf2f(v[j]);
    v[j] = f2bf(0.5f * f * (1.f + erff(f * 0.70710678118654752440f)));
  }
  *reinterpret_cast<bf16x8*>(u + i * 8) = v;
}

// ---------------------------------------------------------------- pool
// out[b] = normalize(mean over the segment's rows of h - mu). One workgroup per
// text, 192 lanes x 2 columns; the rows are summed first to last. With
// normalize = 0 the centred mean itself is written (used to estimate mu).
__global__ __launch_bounds__(192)
void encoder_pool_kernel(float* __restrict__ out,            // [B, 384]
                         const short* __restrict__ h,         // [R, 384]
                         const int* __restrict__ cu_rows,     // [B+1]
                         const float* __restrict__ mu,        // [384]
                         int R, int normalize) {
  __shared__ float red[16];
  const int b = blockIdx.x;
  const int c = threadIdx.x * 2;
  const int row0 = cu_rows[b];
  int len = min(cu_rows[b + 1] - row0, ENC_MAXLEN);
  if (len <= 0 || row0 < 0 || row0 + len > R) len = 0;   // host-checked
  float s0 = 0.f, s1 = 0.f;
  const short* p = h + (long)row0 * ENC_DIM + c;
  for (int r = 0; r < len; ++r) {
    const uint32_t v = *reinterpret_cast<const uint32_t*>(p + (long)r * ENC_DIM);
    s0 += bf2f((short)(v & 0xffffu));
    s1 += bf2f((short)(v >> 16));
  }
  const float d = (float)max(len, 1);
  float v0 = s0 / d - mu[c], v1 = s1 / d - mu[c + 1];
  if (normalize) {
    const float ss = block_reduce_sum(v0 * v0 + v1 * v1, red);
    const float inv = 1.f / fmaxf(sqrtf(ss), 1e-12f);
    v0 *= inv;
    v1 *= inv;
  }
  out[(long)b * ENC_DIM + c] = v0;
  out[(long)b * ENC_DIM + c + 1] = v1;
}

// ---------------------------------------------------------------- wrappers

// R packed rows (1 <= R, R * 1152 within int) in B = cu_rows.numel() - 1
// segments, 1 <= B <= R. The offsets themselves are the caller's contract
// (ops._check_cu_rows checks them on host values).
static int64_t enc_check_segments(OpChecks& c, const torch::Tensor& cu_rows,
                                  int64_t R) {
  c.range("R", R, 1, 0x7fffffffL / ENC_QKV);
  c.tensor("cu_rows", cu_rows, kI32, {-1});
  return c.size_range("cu_rows", cu_rows, 0, 2, R + 1) - 1;
}

void encoder_embed(torch::Tensor x, torch::Tensor feats, torch::Tensor pos_ids,
                   torch::Tensor pos_table) {
  OpChecks c("encoder_embed");
  c.tensor("x", x, kBF16, {-1, ENC_DIM});
  const int64_t R = x.size(0);
  c.range("R", R, 1, 0x7fffffffL / ENC_QKV);
  c.tensor("feats", feats, kI32, {R, 4});
  c.tensor("pos_ids", pos_ids, kI32, {R});
  c.tensor("pos_table", pos_table, kF32, {-1, ENC_DIM});
  c.size_range("pos_table", pos_table, 0, 1, std::numeric_limits<int>::max());
  if (check_only()) return;
  hipStream_t s = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(encoder_embed_kernel, dim3((R + 3) / 4), dim3(256), 0, s,
                     (short*)x.data_ptr(), feats.data_ptr<int>(),
                     pos_ids.data_ptr<int>(), pos_table.data_ptr<float>(),
                     (int)R, (int)pos_table.size(0));
  HIP_CHECK_KERNEL();
}

void encoder_attention(torch::Tensor out, torch::Tensor qkv,
                       torch::Tensor cu_rows) {
  OpChecks c("encoder_attention");
  c.tensor("qkv", qkv, kBF16, {-1, ENC_QKV});   // rows are q|k|v
  const int64_t R = qkv.size(0);
  c.tensor("out", out, kBF16, {R, ENC_DIM});
  const int64_t B = enc_check_segments(c, cu_rows, R);
  c.grid(B, ENC_HEADS);
  if (check_only()) return;
  hipStream_t s = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(encoder_attention_kernel, dim3(B, ENC_HEADS), dim3(256),
                     0, s, (short*)out.data_ptr(),
                     (const short*)qkv.data_ptr(), cu_rows.data_ptr<int>(),
                     (int)R, 0.17677669529663688110f /* 32^-0.5 */);
  HIP_CHECK_KERNEL();
}

void gelu_(torch::Tensor u) {
  OpChecks c("gelu_");
  c.require(u.defined(), "u is undefined");
  c.tensor("u", u, kBF16, u.sizes());   // any shape, contiguous
  c.require(u.numel() % 8 == 0, "u holds ", u.numel(),
            " elements, not a multiple of 8");
  const long nvec = u.numel() / 8;
  c.grid((nvec + 255) / 256);
  if (nvec == 0 || check_only()) return;
  hipStream_t s = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(gelu_kernel, dim3((nvec + 255) / 256), dim3(256), 0, s,
                     (short*)u.data_ptr(), nvec);
  HIP_CHECK_KERNEL();
}

void encoder_pool(torch::Tensor out, torch::Tensor h, torch::Tensor cu_rows,
                  torch::Tensor mu, bool normalize) {
  OpChecks c("encoder_pool");
  c.tensor("h", h, kBF16, {-1, ENC_DIM});
  const int64_t R = h.size(0);
  const int64_t B = enc_check_segments(c, cu_rows, R);
  c.tensor("out", out, kF32, {B, ENC_DIM});
  c.tensor("mu", mu, kF32, {ENC_DIM});
  c.grid(B);
  if (check_only()) return;
  hipStream_t s = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(encoder_pool_kernel, dim3(B), dim3(192), 0, s,
                     out.data_ptr<float>(), (const short*)h.data_ptr(),
                     cu_rows.data_ptr<int>(), mu.data_ptr<float>(), (int)R,
                     normalize ? 1 : 0);
  HIP_CHECK_KERNEL();
}
