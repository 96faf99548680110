// MFMA flash-attention prefill over the paged KV cache.
//
// One workgroup = (q-tile of ≤32 tokens of ONE sequence) × (kv head);
// 512 threads = 8 waves; wave w = q-head w of the GQA group. The KV prefix is
// walked in chunks of 64 positions from position 0 with an online softmax.
//   M = 32 tokens (2 row blocks mt), N = 64 kv positions/chunk (4 blocks nt),
//   D = 128. Per chunk per wave: 32 score MFMAs + 32 P·V MFMAs, all
//   mfma_f32_16x16x32_bf16.
//
// Where the operands live:
//   Q   registers. The wave's 32×128 fragment (softmax scale folded in, one
//       bf16 rounding) is loaded once as the B operand of the score product:
//       qf[mt][kk] = Q[mt*16 + (lane&15)][kk*32 + 8*(lane>>4) .. +8].
//   S   registers. The product is swapped, Sᵀ = K·Qᵀ (K rows from LDS are the
//       A operand), so by the C map (col = lane&15, row = 4*(lane>>4) + r)
//       st[mt][nt][r] is the score of q row mt*16 + (lane&15) at position
//       nt*16 + 4*(lane>>4) + r: a lane owns 16 of its row's 64 scores. Row
//       max = in-lane chain + two exchanges (lanes ^16, ^32). The row sum is
//       carried as a per-lane partial (the rescale factor is row-wide) and
//       combined once in the epilogue.
//   P   registers. st[mt][2s] and st[mt][2s+1], rounded to bf16, are the
//       B operand of Oᵀ += Vᵀ·Pᵀ for k-step s as they stand: element j of a
//       lane is position 32s + 16*(j>>2) + 4*(lane>>4) + (j&3).
//   V   row-major in LDS; the matching Vᵀ A operand is two transposed reads
//       (ds_read_b64_tr_b16) of the 4-row × 16-dim blocks at rows
//       32s + 4*(lane>>4) and 16 below. Every lane is active at those reads
//       (short tiles pad with zero q rows, they do not branch).
//   O   registers, transposed: oacc[mt][nf][r] is dim nf*16 + 4*(lane>>4) + r
//       of q row mt*16 + (lane&15), so the rescale is one factor per lane and
//       mt, and the epilogue stores 4 contiguous dims (8 B) per fragment.
//
// LDS: two buffers of {K tile, V tile}, each tile 64 rows × 256 B, staged
// with 16-byte stores; 64 KiB in all. off(row, ch) of 16-byte chunk ch:
//   K: 256*row + 16*(ch ^ (row & 15))
//      ds_read_b128 is served in 16-lane groups such as lanes {0-3, 12-15,
//      20-27}: rows {0-3, 12-15} at chunk c and rows {4-11} at chunk c^1,
//      i.e. slots c ^ {0-3, 12-15} and c ^ {4-11}: 16 distinct 16-byte slots
//      of the 256-byte bank row, conflict-free; the other three groups alike.
//   V: 256*row + 16*(ch ^ ((row & 7) << 1))
//      a transposed read is served per 32-lane half, which takes the 32-byte
//      segment of dims 16nf..16nf+15 from 8 rows with distinct row & 7: the
//      XOR moves them to 8 distinct 32-byte segments, 64 banks once each,
//      conflict-free. Bit 0 of ch is untouched, so a segment stays contiguous.
//   Stores: 8 consecutive lanes write the 8 chunks of half a row, XORed into
//   8 distinct slots: conflict-free on the 32-bank store rule.
//
// Pipeline: the loads of chunk c+1 (block ids fetched one chunk further
// ahead, so no load waits on another) are issued before the score product of
// chunk c and written to the other buffer after its P·V product; one block
// barrier per chunk.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include "common.h"
#include "kv_fp8.h"
#include "checks.h"

#define FP_BS 16          // paged KV block size
#define FP_QTOK 32        // q tokens per tile (2 MFMA row-blocks)
#define FP_CHUNK 64       // kv positions per chunk (4 MFMA col-blocks)
#define FP_D 128
#define FP_QH 8           // GQA group
#define FP_TILE_B (FP_CHUNK * FP_D * 2)   // bytes of one K or V tile in LDS

typedef __attribute__((ext_vector_type(4))) float fpfrag_t;
typedef __attribute__((ext_vector_type(2))) float fp_f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 fp_bf16x2;
typedef __attribute__((address_space(3))) bf16x4 fp_lds_bf16x4;

// two f32 -> two bf16 (round to nearest even) in one dword, lo in the low half
DEV uint32_t fp_pack_bf16(float lo, float hi) {
  return __builtin_bit_cast(
      uint32_t, __builtin_convertvector(fp_f32x2{lo, hi}, fp_bf16x2));
}

// F8: the caches hold e4m3 bytes and kscale/vscale [NB, Hk, 16] one f32 per
// row (kv_fp8.h). Only the staging step differs: a thread loads 8 B of K,
// 8 B of V and the row's two scales and writes the image's bf16 values, so
// the LDS tiles hold what the bf16 form stages.
template <bool F8>
__global__ __launch_bounds__(512, 1)
void flash_prefill_kernel(short* __restrict__ out,         // [T, Hq, D]
                          const short* __restrict__ q,      // [T, Hq, D]
                          const std::conditional_t<F8, uint8_t, short>*
                              __restrict__ kcache,          // [NB, Hk, 16, D]
                          const std::conditional_t<F8, uint8_t, short>*
                              __restrict__ vcache,
                          const int* __restrict__ block_table,
                          const int* __restrict__ seq_ids,
                          const int* __restrict__ q_pos,
                          const int* __restrict__ tile_desc,  // [G, 2]: row0, n
                          int n_kvheads, int max_blocks, int q_row_stride,
                          float scale,
                          const float* __restrict__ kscale,
                          const float* __restrict__ vscale) {
  const int g = blockIdx.x;
  const int hk = blockIdx.y;
  const int row0 = tile_desc[g * 2 + 0];
  const int ntok = tile_desc[g * 2 + 1];
  if (ntok <= 0) return;          // whole workgroup: a zero-count tile
  const int tid = threadIdx.x;
  const int wid = tid >> 6;       // q head within group
  const int lane = tid & 63;
  const int lrow = lane & 15;     // q row within a row block
  const int lgrp = lane >> 4;     // 16-lane group
  const int n_qheads = n_kvheads * FP_QH;
  const int hq = hk * FP_QH + wid;

  // [buffer][K, V][64 rows × 256 B]
  __shared__ __attribute__((aligned(16))) char kv_s[2][2][FP_TILE_B];

  // ---- Q fragment (B operand of the score product) and the rows' bounds
  bf16x8 qf[2][4];
  int bnd[2];
  #pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    const int tk = mt * 16 + lrow;
    bnd[mt] = 0;                  // pad row: every score masked
    #pragma unroll
    for (int kk = 0; kk < 4; ++kk) qf[mt][kk] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    if (tk < ntok) {
      bnd[mt] = q_pos[row0 + tk] + 1;
      const short* qp = q + (long)(row0 + tk) * q_row_stride + hq * FP_D
                        + lgrp * 8;
      #pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        bf16x8 v = *reinterpret_cast<const bf16x8*>(qp + kk * 32);
        // fold the softmax scale into Q: no multiply per score in the loop
        #pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = f2bf(bf2f(v[j]) * scale);
        qf[mt][kk] = v;
      }
    }
  }
  // the 16 lanes of any group hold all 32 rows between them
  int bmax = max(bnd[0], bnd[1]), bmin = min(bnd[0], bnd[1]);
  #pragma unroll
  for (int off = 8; off > 0; off >>= 1) {
    bmax = max(bmax, __shfl_xor(bmax, off, WAVE));
    bmin = min(bmin, __shfl_xor(bmin, off, WAVE));
  }
  const int bound_max = __builtin_amdgcn_readfirstlane(bmax);
  const int bound_min = __builtin_amdgcn_readfirstlane(bmin);  // full tiles

  const int seq = seq_ids[row0];
  const int* btab = block_table + (long)seq * max_blocks;
  const long kv_stride_block = (long)n_kvheads * FP_BS * FP_D;

  // ---- staging: a thread moves chunk sch of rows srow and srow + 32
  using raw_t = std::conditional_t<F8, kv_u32x2, bf16x8>;
  const int srow = tid >> 4, sch = tid & 15;
  const long slice_off = ((long)hk * FP_BS + (srow & 15)) * FP_D + sch * 8;
  const int k_wr = srow * 256 + ((sch ^ (srow & 15)) << 4);
  const int v_wr = srow * 256 + ((sch ^ ((srow & 7) << 1)) << 4);
  raw_t kraw[2], vraw[2];
  float ksc[2], vsc[2];
  int blk[2];

  // block ids of the thread's two rows of the chunk at `base`
  auto load_blk = [&](int base) {
    #pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int pos = base + srow + it * 32;
      blk[it] = (pos < bound_max) ? btab[pos / FP_BS] : 0;
    }
  };
  // issue the loads of the chunk at `base` (blk holds its block ids);
  // positions at or past bound_max are staged as zeros, never read
  auto issue = [&](int base) {
    #pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int pos = base + srow + it * 32;
      kraw[it] = raw_t{};
      vraw[it] = raw_t{};
      ksc[it] = vsc[it] = 1.f;
      if (pos < bound_max) {
        const long off = (long)blk[it] * kv_stride_block + slice_off;
        kraw[it] = *reinterpret_cast<const raw_t*>(kcache + off);
        vraw[it] = *reinterpret_cast<const raw_t*>(vcache + off);
        if constexpr (F8) {
          const long soff = ((long)blk[it] * n_kvheads + hk) * FP_BS
                            + (srow & 15);
          ksc[it] = kscale[soff];
          vsc[it] = vscale[soff];
        }
      }
    }
  };
  // write the loaded chunk into buffer b
  auto commit = [&](int b) {
    #pragma unroll
    for (int it = 0; it < 2; ++it) {
      bf16x8 kv, vv;
      if constexpr (F8) {
        kv = __builtin_bit_cast(bf16x8, kv_fp8x8_to_bf16(kraw[it], ksc[it]));
        vv = __builtin_bit_cast(bf16x8, kv_fp8x8_to_bf16(vraw[it], vsc[it]));
      } else {
        kv = kraw[it];
        vv = vraw[it];
      }
      *reinterpret_cast<bf16x8*>(&kv_s[b][0][k_wr + it * 32 * 256]) = kv;
      *reinterpret_cast<bf16x8*>(&kv_s[b][1][v_wr + it * 32 * 256]) = vv;
    }
  };

  // per-lane read offsets. K row read: row nt*16 + lrow, chunk kk*4 + lgrp.
  int k_rd[4];
  #pragma unroll
  for (int kk = 0; kk < 4; ++kk)
    k_rd[kk] = lrow * 256 + (((kk * 4 + lgrp) ^ lrow) << 4);
  // V transposed read: lane 4q+p of a group names row q, dims 4p..4p+3 of
  // the block; rows 32s + 16h + 4*lgrp + q, so row & 7 = 4*(lgrp&1) + q.
  const int v_q = lrow >> 2, v_p = lrow & 3;
  const int v_x = 4 * (lgrp & 1) + v_q;
  const int v_rd = (4 * lgrp + v_q) * 256 + v_p * 8;

  float m_run[2] = {-INFINITY, -INFINITY};
  float l_run[2] = {0.f, 0.f};   // this lane's share of the row sum
  fpfrag_t oacc[2][8];
  #pragma unroll
  for (int mt = 0; mt < 2; ++mt)
    #pragma unroll
    for (int nf = 0; nf < 8; ++nf) oacc[mt][nf] = fpfrag_t{0.f, 0.f, 0.f, 0.f};

  load_blk(0);
  issue(0);
  load_blk(FP_CHUNK);
  commit(0);
  __syncthreads();

  int cur = 0;
  for (int base = 0; base < bound_max; base += FP_CHUNK, cur ^= 1) {
    const bool more = base + FP_CHUNK < bound_max;
    if (more) {
      issue(base + FP_CHUNK);
      load_blk(base + 2 * FP_CHUNK);
    }
    const char* kb = kv_s[cur][0];
    const char* vb = kv_s[cur][1];

    // ---- Sᵀ = K·Qᵀ: 4 position blocks × 2 row blocks × 4 k-steps
    fpfrag_t st[2][4];
    #pragma unroll
    for (int mt = 0; mt < 2; ++mt)
      #pragma unroll
      for (int nt = 0; nt < 4; ++nt)
        st[mt][nt] = fpfrag_t{0.f, 0.f, 0.f, 0.f};
    #pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      #pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(
            kb + nt * 16 * 256 + k_rd[kk]);
        st[0][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, qf[0][kk], st[0][nt], 0, 0, 0);
        st[1][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, qf[1][kk], st[1][nt], 0, 0, 0);
      }
    }

    // ---- causal mask + online softmax, in registers. Chunks entirely below
    // every row's bound of a full tile skip the compares (which would all be
    // false, so the bits are the masked path's).
    const bool interior = (ntok == FP_QTOK) && (base + FP_CHUNK <= bound_min);
    float rs[2];
    bf16x8 pb[2][2];
    #pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      if (!interior) {
        const int lim = bnd[mt] - base - 4 * lgrp;   // visible: 16nt + r < lim
        #pragma unroll
        for (int nt = 0; nt < 4; ++nt)
          #pragma unroll
          for (int r = 0; r < 4; ++r)
            if (nt * 16 + r >= lim) st[mt][nt][r] = -INFINITY;
      }
      float mx = -INFINITY;
      #pragma unroll
      for (int nt = 0; nt < 4; ++nt)
        #pragma unroll
        for (int r = 0; r < 4; ++r) mx = fmaxf(mx, st[mt][nt][r]);
      mx = fmaxf(mx, __shfl_xor(mx, 16, WAVE));
      mx = fmaxf(mx, __shfl_xor(mx, 32, WAVE));
      const float m_new = fmaxf(m_run[mt], mx);
      // nothing visible yet (m_new = -inf): p = exp(-inf - 0) = 0, rs = 1
      const float m_safe = (m_new == -INFINITY) ? 0.f : m_new;
      rs[mt] = (m_run[mt] == m_new) ? 1.f : __expf(m_run[mt] - m_safe);
      float psum = 0.f;
      #pragma unroll
      for (int nt = 0; nt < 4; ++nt)
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = __expf(st[mt][nt][r] - m_safe);
          st[mt][nt][r] = p;
          psum += p;
        }
      l_run[mt] = l_run[mt] * rs[mt] + psum;
      m_run[mt] = m_new;
      #pragma unroll
      for (int s = 0; s < 2; ++s) {
        const kv_u32x4 w = {
            fp_pack_bf16(st[mt][2 * s][0], st[mt][2 * s][1]),
            fp_pack_bf16(st[mt][2 * s][2], st[mt][2 * s][3]),
            fp_pack_bf16(st[mt][2 * s + 1][0], st[mt][2 * s + 1][1]),
            fp_pack_bf16(st[mt][2 * s + 1][2], st[mt][2 * s + 1][3])};
        pb[mt][s] = __builtin_bit_cast(bf16x8, w);
      }
    }
    // rs == 1 everywhere once the running max has settled: skip the pass
    if (!__all(rs[0] == 1.f && rs[1] == 1.f)) {
      #pragma unroll
      for (int mt = 0; mt < 2; ++mt)
        #pragma unroll
        for (int nf = 0; nf < 8; ++nf) oacc[mt][nf] *= rs[mt];
    }

    // ---- Oᵀ += Vᵀ·Pᵀ: 8 dim blocks × 2 row blocks × 2 k-steps
    #pragma unroll
    for (int s = 0; s < 2; ++s) {
      #pragma unroll
      for (int nf = 0; nf < 8; ++nf) {
        const char* va = vb + s * 32 * 256 + v_rd + (((2 * nf) ^ (v_x << 1)) << 4);
        const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (fp_lds_bf16x4*)(va));
        const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (fp_lds_bf16x4*)(va + 16 * 256));
        const bf16x8 a = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        oacc[0][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, pb[0][s], oacc[0][nf], 0, 0, 0);
        oacc[1][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, pb[1][s], oacc[1][nf], 0, 0, 0);
      }
    }

    // the other buffer was last read before the previous barrier
    if (more) commit(cur ^ 1);
    __syncthreads();
  }

  // ---- epilogue: combine the row sum's four partials, normalize, store
  #pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    float l = l_run[mt];
    l += __shfl_xor(l, 16, WAVE);
    l += __shfl_xor(l, 32, WAVE);
    const float inv_l = (l > 0.f) ? 1.0f / l : 0.f;
    const int tk = mt * 16 + lrow;
    if (tk >= ntok) continue;
    short* orow = out + ((long)(row0 + tk) * n_qheads + hq) * FP_D + 4 * lgrp;
    #pragma unroll
    for (int nf = 0; nf < 8; ++nf) {
      const kv_u32x2 w = {
          fp_pack_bf16(oacc[mt][nf][0] * inv_l, oacc[mt][nf][1] * inv_l),
          fp_pack_bf16(oacc[mt][nf][2] * inv_l, oacc[mt][nf][3] * inv_l)};
      *reinterpret_cast<kv_u32x2*>(orow + nf * 16) = w;
    }
  }
}

void flash_prefill(torch::Tensor out, torch::Tensor q, torch::Tensor kcache,
                   torch::Tensor vcache, torch::Tensor block_table,
                   torch::Tensor seq_ids, torch::Tensor q_pos,
                   torch::Tensor tile_desc, double scale,
                   c10::optional<torch::Tensor> k_scale,
                   c10::optional<torch::Tensor> v_scale) {
  OpChecks c("flash_prefill");
  const bool fp8 = kv_fp8_check(c, kcache, vcache, k_scale, v_scale);
  attn_check_tokens(c, out, q, kcache, block_table, seq_ids, q_pos);
  c.tensor("tile_desc", tile_desc, kI32, {-1, 2});
  const int n_kvheads = kcache.size(1);
  const int G = c.fits_int("tile_desc.size(0)", tile_desc.size(0));
  c.grid(G, n_kvheads);
  if (check_only()) return;
  const int max_blocks = block_table.size(1);
  dim3 grid(G, n_kvheads), block(512);
  hipStream_t s = c10::hip::getCurrentHIPStream();
  if (fp8)
    hipLaunchKernelGGL(flash_prefill_kernel<true>, grid, block, 0, s,
                       (short*)out.data_ptr(), (const short*)q.data_ptr(),
                       (const uint8_t*)kcache.data_ptr(),
                       (const uint8_t*)vcache.data_ptr(),
                       block_table.data_ptr<int>(), seq_ids.data_ptr<int>(),
                       q_pos.data_ptr<int>(), tile_desc.data_ptr<int>(),
                       n_kvheads, max_blocks, (int)q.stride(0), (float)scale,
                       k_scale->data_ptr<float>(), v_scale->data_ptr<float>());
  else
    hipLaunchKernelGGL(flash_prefill_kernel<false>, grid, block, 0, s,
                       (short*)out.data_ptr(), (const short*)q.data_ptr(),
                       (const short*)kcache.data_ptr(),
                       (const short*)vcache.data_ptr(),
                       block_table.data_ptr<int>(), seq_ids.data_ptr<int>(),
                       q_pos.data_ptr<int>(), tile_desc.data_ptr<int>(),
                       n_kvheads, max_blocks, (int)q.stride(0), (float)scale,
                       (const float*)nullptr, (const float*)nullptr);
  HIP_CHECK_KERNEL();
}

int64_t flash_prefill_qtile() { return FP_QTOK; }
