// Paged attention for GQA (Qwen3-30B-A3B: 32 q heads / 4 kv heads / head_dim 128).
//
// Every query token attends to the paged KV cache of its sequence up to its
// own position (causal). Sessions are KV-cache residency (SURVEY §5
// "session-as-KV-cache"), so every phase reads the same cache.
//
// Layouts (chosen for these kernels, we own the cache):
//   K,V cache: [num_blocks, kv_heads, BLOCK_SIZE, head_dim] bf16
//   block_table: [num_seqs, max_blocks] int32
//
// Two kernels:
//   paged_attn_kernel        one workgroup per (query token, kv head), VALU
//                            dot products, online softmax over 32-position
//                            chunks. Serves any T.
//   paged_attn_split_kernel  decode: the KV range of a (token, kv head) is
//                            split over grid.z workgroups, scores and P·V run
//                            on the matrix cores straight from registers, and
//                            paged_attn_merge_kernel combines the partials.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include "common.h"
#include "kv_fp8.h"
#include "checks.h"

#define BLOCK_SIZE 16
#define CHUNK 32          // kv positions per iteration
#define QH_PER_KV 8       // GQA group width (32/4)
#define HEAD_DIM 128

// Workgroup = (query token, kv head): 256 threads = 4 waves.
//   score phase: thread (h = t>>5, j = t&31) computes dot(q[h], k[pos_j])
//                (full 128-dim dot per thread; rows stream through L1)
//   value phase: thread (h = t>>5, d4 = (t&31)*4) accumulates 4 output dims;
//                V reads are 32×8B consecutive = coalesced per head-group.
// Online softmax with per-head running max/sum (flash-style, fp32).
//
// F8 (all kernels of this file): the caches hold e4m3 bytes and kscale/vscale
// [NB, Hk, BS] one f32 per row (kv_fp8.h). Bytes become the image's bf16
// values as they are loaded; everything after the load is the bf16 code.
template <bool F8>
using kv_elem_t = std::conditional_t<F8, uint8_t, short>;

template <bool F8>
__global__ __launch_bounds__(256)
void paged_attn_kernel(short* __restrict__ out,          // [T, Hq, D]
                       const short* __restrict__ q,      // [T, Hq, D]
                       const kv_elem_t<F8>* __restrict__ kcache, // [NB, Hk, BS, D]
                       const kv_elem_t<F8>* __restrict__ vcache,
                       const int* __restrict__ block_table,  // [S, MB]
                       const int* __restrict__ seq_ids,      // [T]
                       const int* __restrict__ q_pos,        // [T] absolute pos
                       int n_kvheads, int max_blocks, int q_row_stride,
                       float scale,
                       const float* __restrict__ kscale,  // F8: [NB, Hk, BS]
                       const float* __restrict__ vscale) {
  const int t = blockIdx.x;       // query token
  const int hk = blockIdx.y;      // kv head
  const int tid = threadIdx.x;
  const int h = tid >> 5;         // 0..7: q-head within group
  const int sub = tid & 31;       // score: position lane / value: dim quarter
  const int seq = seq_ids[t];
  const int bound = q_pos[t] + 1; // causal: attend to [0, bound)

  const int hq = hk * QH_PER_KV + h;
  const int n_qheads = n_kvheads * QH_PER_KV;

  __shared__ float q_s[QH_PER_KV][HEAD_DIM];
  __shared__ float p_s[QH_PER_KV][CHUNK];

  // load q for the 8 heads of this group into LDS (fp32)
  for (int i = tid; i < QH_PER_KV * HEAD_DIM; i += blockDim.x) {
    int hh = i / HEAD_DIM, dd = i % HEAD_DIM;
    q_s[hh][dd] = bf2f(q[(long)t * q_row_stride
                         + (hk * QH_PER_KV + hh) * HEAD_DIM + dd]);
  }
  __syncthreads();

  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;

  const long kv_stride_block = (long)n_kvheads * BLOCK_SIZE * HEAD_DIM;
  const int* btab = block_table + (long)seq * max_blocks;

  for (int base = 0; base < bound; base += CHUNK) {
    // ---- score phase: this thread scores position base+sub for head h
    {
      const int pos = base + sub;
      float s = -INFINITY;
      if (pos < bound) {
        const int blk = btab[pos / BLOCK_SIZE];
        const kv_elem_t<F8>* krow = kcache + (long)blk * kv_stride_block
                            + ((long)hk * BLOCK_SIZE + (pos % BLOCK_SIZE)) * HEAD_DIM;
        float ks = 1.f;
        if constexpr (F8)
          ks = kscale[((long)blk * n_kvheads + hk) * BLOCK_SIZE + pos % BLOCK_SIZE];
        float dot = 0.f;
        #pragma unroll
        for (int v8 = 0; v8 < HEAD_DIM / 8; ++v8) {
          bf16x8 kv;
          if constexpr (F8)
            kv = __builtin_bit_cast(bf16x8, kv_fp8x8_to_bf16(
                *reinterpret_cast<const kv_u32x2*>(krow + v8 * 8), ks));
          else
            kv = *reinterpret_cast<const bf16x8*>(krow + v8 * 8);
          #pragma unroll
          for (int j = 0; j < 8; ++j) dot += q_s[h][v8 * 8 + j] * bf2f(kv[j]);
        }
        s = dot * scale;
      }
      p_s[h][sub] = s;
    }
    __syncthreads();

    // ---- softmax + value phase: thread owns dims [sub*4, sub*4+4) of head h
    {
      float chunk_max = -INFINITY;
      #pragma unroll
      for (int j = 0; j < CHUNK; ++j) chunk_max = fmaxf(chunk_max, p_s[h][j]);
      const float m_new = fmaxf(m_run, chunk_max);
      if (m_new != -INFINITY) {
        const float rescale = (m_run == -INFINITY) ? 0.f : __expf(m_run - m_new);
        acc[0] *= rescale; acc[1] *= rescale; acc[2] *= rescale; acc[3] *= rescale;
        l_run *= rescale;
        const int lim = min(CHUNK, bound - base);
        for (int j = 0; j < lim; ++j) {
          const float w = __expf(p_s[h][j] - m_new);
          l_run += w;
          const int pos = base + j;
          const int blk = btab[pos / BLOCK_SIZE];
          const kv_elem_t<F8>* vrow = vcache + (long)blk * kv_stride_block
                              + ((long)hk * BLOCK_SIZE + (pos % BLOCK_SIZE)) * HEAD_DIM
                              + sub * 4;
          bf16x4 vv;
          if constexpr (F8)
            vv = __builtin_bit_cast(bf16x4, kv_fp8x4_to_bf16(
                *reinterpret_cast<const uint32_t*>(vrow),
                vscale[((long)blk * n_kvheads + hk) * BLOCK_SIZE
                       + pos % BLOCK_SIZE]));
          else
            vv = *reinterpret_cast<const bf16x4*>(vrow);
          acc[0] += w * bf2f(vv[0]);
          acc[1] += w * bf2f(vv[1]);
          acc[2] += w * bf2f(vv[2]);
          acc[3] += w * bf2f(vv[3]);
        }
        m_run = m_new;
      }
    }
    __syncthreads();
  }

  const float inv_l = (l_run > 0.f) ? 1.0f / l_run : 0.f;
  short* orow = out + ((long)t * n_qheads + hq) * HEAD_DIM + sub * 4;
  bf16x4 o;
  #pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = f2bf(acc[j] * inv_l);
  *reinterpret_cast<bf16x4*>(orow) = o;

  // NOTE: the value phase recomputes l_run identically in all 32 threads of a
  // head (each walks the same 32 scores) — redundant VALU, zero extra HBM.
}

// ------------------------------------------------ KV cache scatter
// Write new K/V rows for T tokens into their paged slots.
__global__ void write_kv_kernel(short* __restrict__ kcache,
                                short* __restrict__ vcache,
                                const short* __restrict__ k,   // [T, Hk, D]
                                const short* __restrict__ v,
                                const int* __restrict__ block_table,
                                const int* __restrict__ seq_ids,
                                const int* __restrict__ q_pos,
                                int n_kvheads, int max_blocks) {
  const int t = blockIdx.x;
  const int seq = seq_ids[t];
  const int pos = q_pos[t];
  const int blk = block_table[(long)seq * max_blocks + pos / BLOCK_SIZE];
  const long dst_base = ((long)blk * n_kvheads) * BLOCK_SIZE * HEAD_DIM
                        + (long)(pos % BLOCK_SIZE) * HEAD_DIM;
  // threads cover Hk * D elements in 8-wide vectors
  const int total_vec = n_kvheads * HEAD_DIM / 8;
  for (int i = threadIdx.x; i < total_vec; i += blockDim.x) {
    const int hh = (i * 8) / HEAD_DIM;
    const int dd = (i * 8) % HEAD_DIM;
    const long dst = dst_base + (long)hh * BLOCK_SIZE * HEAD_DIM + dd;
    *reinterpret_cast<bf16x8*>(kcache + dst) =
        *reinterpret_cast<const bf16x8*>(k + ((long)t * n_kvheads + hh) * HEAD_DIM + dd);
    *reinterpret_cast<bf16x8*>(vcache + dst) =
        *reinterpret_cast<const bf16x8*>(v + ((long)t * n_kvheads + hh) * HEAD_DIM + dd);
  }
}

// ---------------------------------------------------------------- wrappers

void paged_attention(torch::Tensor out, torch::Tensor q, torch::Tensor kcache,
                     torch::Tensor vcache, torch::Tensor block_table,
                     torch::Tensor seq_ids, torch::Tensor q_pos, double scale,
                     c10::optional<torch::Tensor> k_scale,
                     c10::optional<torch::Tensor> v_scale) {
  OpChecks c("paged_attention");
  const bool fp8 = kv_fp8_check(c, kcache, vcache, k_scale, v_scale);
  const int T = attn_check_tokens(c, out, q, kcache, block_table, seq_ids, q_pos);
  const int n_kvheads = kcache.size(1);
  c.grid(T, n_kvheads);
  if (check_only()) return;
  const int max_blocks = block_table.size(1);
  dim3 grid(T, n_kvheads), block(256);
  hipStream_t s = c10::hip::getCurrentHIPStream();
  if (fp8)
    hipLaunchKernelGGL(paged_attn_kernel<true>, grid, block, 0, s,
                       (short*)out.data_ptr(), (const short*)q.data_ptr(),
                       (const uint8_t*)kcache.data_ptr(),
                       (const uint8_t*)vcache.data_ptr(),
                       block_table.data_ptr<int>(), seq_ids.data_ptr<int>(),
                       q_pos.data_ptr<int>(), n_kvheads, max_blocks,
                       (int)q.stride(0), (float)scale,
                       k_scale->data_ptr<float>(), v_scale->data_ptr<float>());
  else
    hipLaunchKernelGGL(paged_attn_kernel<false>, grid, block, 0, s,
                       (short*)out.data_ptr(), (const short*)q.data_ptr(),
                       (const short*)kcache.data_ptr(),
                       (const short*)vcache.data_ptr(),
                       block_table.data_ptr<int>(), seq_ids.data_ptr<int>(),
                       q_pos.data_ptr<int>(), n_kvheads, max_blocks,
                       (int)q.stride(0), (float)scale,
                       (const float*)nullptr, (const float*)nullptr);
  HIP_CHECK_KERNEL();
}

void write_kv(torch::Tensor kcache, torch::Tensor vcache, torch::Tensor k,
              torch::Tensor v, torch::Tensor block_table, torch::Tensor seq_ids,
              torch::Tensor q_pos) {
  OpChecks c("write_kv");
  // bf16 caches only: the fp8 writer is qk_rope_write_kv
  c.tensor("kcache", kcache, kBF16, {-1, -1, BLOCK_SIZE, HEAD_DIM});
  c.tensor("vcache", vcache, kBF16, kcache.sizes());
  const int n_kvheads = c.fits_int("kcache.size(1)", kcache.size(1));
  c.tensor("k", k, kBF16, {-1, n_kvheads, HEAD_DIM});
  const int T = c.fits_int("k.size(0)", k.size(0));
  c.tensor("v", v, kBF16, {T, n_kvheads, HEAD_DIM});
  check_paging(c, block_table, seq_ids, T);
  c.tensor("q_pos", q_pos, kI32, {T});
  c.grid(T);
  if (check_only()) return;
  const int max_blocks = block_table.size(1);
  dim3 grid(T), block(128);
  hipStream_t s = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(write_kv_kernel, grid, block, 0, s,
                     (short*)kcache.data_ptr(), (short*)vcache.data_ptr(),
                     (const short*)k.data_ptr(), (const short*)v.data_ptr(),
                     block_table.data_ptr<int>(), seq_ids.data_ptr<int>(),
                     q_pos.data_ptr<int>(), n_kvheads, max_blocks);
  HIP_CHECK_KERNEL();
}

// ------------------------------------------------ split-KV flash-decode
// Decode grids are tiny (T = batch ≈ swarm width, 4 kv heads → ~20 workgroups
// for 256 CUs). Split the KV range across NSPLITS workgroups per (token, kv
// head); each writes an unnormalized partial (acc, m, l); a merge kernel
// combines. NSPLITS is static so the decode step stays hipGraph-capturable.

// grid.z is 32 or 64 and static per captured decode graph. On this kernel 32
// splits win at every measured context (B=5: 21.8 vs 24.0 us at 8k tokens,
// 36.8 vs 38.3 us at 16k; profiles/PERF_NOTES.md): 64 splits double the
// empty-split dispatch and the merge traffic and no longer shorten a serial
// chunk chain. The engine still selects 64 from 16384 tokens.
#define NSPLITS 32          // default split count (short contexts)
#define NSPLITS_MAX 64      // part-buffer layout stride; grid.z may be 32 or 64

// A split's span is cut into tiles of TILE = BLOCK_SIZE positions, so a tile
// is exactly one cache block: 16 K rows and 16 V rows of 256 B, contiguous.
// The workgroup's 4 waves take the tiles round-robin, two per iteration (wave
// w: tiles w and w+4, then w+8 and w+12, ...), and each keeps a private
// running (m, l, acc) for the 8 q heads; there is no LDS and no block barrier
// in the tile loop. The waves combine once at the end through LDS, in wave
// order, so the result is the same every launch.
//
// Per tile pair and wave (lane l: n = l & 15, g = l >> 4):
//   loads   all 16 (2 tiles x 4 K + 4 V, 16 B per lane each) are issued
//           before the first MFMA. Up to 4096 tokens at 32 splits that is the
//           wave's whole share of the split in flight at once.
//   scores  S^T[pos][head] = K_tile · Q^T on mfma_f32_16x16x32_bf16. The A
//           operand comes straight from the cache: lane (n, g) reads 16 B of
//           row n per k-step, four k-steps cover the 256-B row. Q^T is the B
//           operand, loaded once per wave; head columns 8..15 are zero.
//           The accumulator holds S[pos 4g + r][head n] in register r.
//   softmax per head = per lane column, over both tiles at once: max over the
//           8 registers and over g (shuffles xor 16, xor 32). The row sum
//           stays a per-lane partial until the epilogue (the rescale factor
//           is uniform per column).
//   P·V     O^T[dim][head] += V^T · P on mfma_f32_16x16x32_bf16, k = the 32
//           positions of the pair. A sum may run over its terms in any order
//           as long as both operands agree: k-slot 8g + j is row 4g + j of the
//           first tile for j < 4 and row 4g + j - 4 of the second for j >= 4.
//           For the B operand those are exactly the two score accumulators'
//           registers, so P goes in with no lane movement. For the A operand
//           lane (n, g) loads 16 B (dims 8n..8n+7) of rows 4g..4g+3 of both
//           tiles, and MFMA m takes element m of each of the eight, i.e. its
//           16 output rows are dims 8i + m. The 8x8 transpose is in-lane
//           (v_perm_b32); V never touches LDS.
//           acc[m][r] = O[head n][dim 32g + 8r + m].
// Rows at positions >= hi load a valid row of the same block (clamped row
// index, so p = 0 never meets uninitialised cache) and score -inf; a pair
// without a second tile loads its first tile twice and masks the copy.
//
// F8: lane (n, g) loads 8 B where the bf16 form loads 16 B (the same 8
// elements), plus the scales of the rows it reads: one for K row min(n, last)
// and four for V rows min(4g + j, last), so every byte and every scale it
// consumes belongs to a row < hi. All of a pair's loads still issue before
// the first MFMA; the bytes are then converted into the same kr / vr
// registers and the rest is shared.
#define TILE 16
#define SPLIT_WAVES 4
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

// 3 waves per SIMD: 640 workgroups at B = 5 are 2.5 waves per SIMD. The bound
// also keeps the accumulators in VGPRs, where the rescale can reach them.
template <bool F8>
__global__ __launch_bounds__(256, 3)
void paged_attn_split_kernel(float* __restrict__ part,   // [T, Hq, NSPLITS, D]
                             float* __restrict__ part_ml, // [T, Hq, NSPLITS, 2]
                             const short* __restrict__ q,
                             const kv_elem_t<F8>* __restrict__ kcache,
                             const kv_elem_t<F8>* __restrict__ vcache,
                             const int* __restrict__ block_table,
                             const int* __restrict__ seq_ids,
                             const int* __restrict__ q_pos,
                             int n_kvheads, int max_blocks, int q_row_stride,
                             float scale,
                             const float* __restrict__ kscale,
                             const float* __restrict__ vscale) {
  static_assert(TILE == BLOCK_SIZE, "a tile is one cache block");
  const int t = blockIdx.x;
  const int hk = blockIdx.y;
  const int split = blockIdx.z;
  const int tid = threadIdx.x;
  const int h = tid >> 5;        // epilogue: q head / 4-dim group
  const int sub = tid & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform
  const int n = tid & 15;        // tile loop: MFMA column / operand row
  const int g = (tid & 63) >> 4;
  const int seq = seq_ids[t];
  const int bound = q_pos[t] + 1;
  const int n_qheads = n_kvheads * QH_PER_KV;
  const int hq = hk * QH_PER_KV + h;

  // split range, CHUNK-aligned; split count = launch grid.z (32 short / 64 long
  // contexts), buffer layout stride fixed at NSPLITS_MAX
  const int nsp = gridDim.z;
  const int span = ((bound + nsp - 1) / nsp + CHUNK - 1) & ~(CHUNK - 1);
  const int lo = split * span;
  const int hi = min(bound, lo + span);

  float* ml = part_ml + (((long)t * n_qheads + hq) * NSPLITS_MAX + split) * 2;
  float* acc_out = part + (((long)t * n_qheads + hq) * NSPLITS_MAX + split) * HEAD_DIM;

  if (lo >= hi) {  // empty split still writes a neutral partial
    if (sub == 0) { ml[0] = -INFINITY; ml[1] = 0.f; }
    *reinterpret_cast<f32x4*>(acc_out + sub * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
    return;
  }

  __shared__ float o_s[SPLIT_WAVES][QH_PER_KV][HEAD_DIM];
  __shared__ float ml_s[SPLIT_WAVES][QH_PER_KV][2];

  // Q^T B-fragments: element j of k-step ks = q[head n][32 ks + 8 g + j]
  bf16x8 qf[HEAD_DIM / 32];
  {
    const short* qrow = q + (long)t * q_row_stride
                        + (hk * QH_PER_KV + (n & (QH_PER_KV - 1))) * HEAD_DIM + g * 8;
    #pragma unroll
    for (int ks = 0; ks < HEAD_DIM / 32; ++ks) {
      qf[ks] = *reinterpret_cast<const bf16x8*>(qrow + ks * 32);
      if (n >= QH_PER_KV) qf[ks] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
  }

  f32x4 acc[HEAD_DIM / TILE];
  #pragma unroll
  for (int m = 0; m < HEAD_DIM / TILE; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;

  const long kv_stride_block = (long)n_kvheads * BLOCK_SIZE * HEAD_DIM;
  const int* btab = block_table + (long)seq * max_blocks;
  const int tile_end = (hi + TILE - 1) / TILE;   // lo is a multiple of TILE

  auto issue_loads = [&](bf16x8 (&kr)[4], u32x4 (&vr)[4], int tile) {
    const int blk = btab[tile];
    const int last = min(hi - tile * TILE, TILE) - 1;   // last valid row
    const long boff = (long)blk * kv_stride_block + (long)hk * BLOCK_SIZE * HEAD_DIM;
    // wave-uniform block base + 32-bit lane byte offset
    const char* kblk = reinterpret_cast<const char*>(kcache + boff);
    const char* vblk = reinterpret_cast<const char*>(vcache + boff);
    const unsigned koff = (min(n, last) * HEAD_DIM + g * 8) * 2;
    #pragma unroll
    for (int ks = 0; ks < 4; ++ks)
      kr[ks] = *reinterpret_cast<const bf16x8*>(kblk + koff + ks * 64);
    #pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned voff = (min(4 * g + j, last) * HEAD_DIM + n * 8) * 2;
      vr[j] = *reinterpret_cast<const u32x4*>(vblk + voff);
    }
  };

  // F8: a lane's share of one tile as loaded, before conversion
  struct RawTile { kv_u32x2 k[4], v[4]; float ks, vs[4]; };
  auto issue_loads_f8 = [&](RawTile& r, int tile) {
    const int blk = btab[tile];
    const int last = min(hi - tile * TILE, TILE) - 1;   // last valid row
    const long bh = (long)blk * n_kvheads + hk;         // wave-uniform
    const char* kblk = reinterpret_cast<const char*>(kcache)
                       + bh * (BLOCK_SIZE * HEAD_DIM);
    const char* vblk = reinterpret_cast<const char*>(vcache)
                       + bh * (BLOCK_SIZE * HEAD_DIM);
    const int krow = min(n, last);
    const unsigned koff = krow * HEAD_DIM + g * 8;
    #pragma unroll
    for (int ks = 0; ks < 4; ++ks)
      r.k[ks] = *reinterpret_cast<const kv_u32x2*>(kblk + koff + ks * 32);
    r.ks = kscale[bh * BLOCK_SIZE + krow];
    #pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int vrow = min(4 * g + j, last);
      r.v[j] = *reinterpret_cast<const kv_u32x2*>(vblk + vrow * HEAD_DIM + n * 8);
      r.vs[j] = vscale[bh * BLOCK_SIZE + vrow];
    }
  };
  auto convert_f8 = [&](bf16x8 (&kr)[4], u32x4 (&vr)[4], const RawTile& r) {
    #pragma unroll
    for (int ks = 0; ks < 4; ++ks)
      kr[ks] = __builtin_bit_cast(bf16x8, kv_fp8x8_to_bf16(r.k[ks], r.ks));
    #pragma unroll
    for (int j = 0; j < 4; ++j) vr[j] = kv_fp8x8_to_bf16(r.v[j], r.vs[j]);
  };

  for (int t0 = lo / TILE + wave; t0 < tile_end; t0 += 2 * SPLIT_WAVES) {
    const bool two = t0 + SPLIT_WAVES < tile_end;
    const int t1 = two ? t0 + SPLIT_WAVES : t0;
    bf16x8 k0[4], k1[4];
    u32x4 v0[4], v1[4];
    if constexpr (F8) {
      RawTile r0, r1;
      issue_loads_f8(r0, t0);
      issue_loads_f8(r1, t1);
      __builtin_amdgcn_sched_barrier(0);
      convert_f8(k0, v0, r0);
      convert_f8(k1, v1, r1);
    } else {
      issue_loads(k0, v0, t0);
      issue_loads(k1, v1, t1);
      __builtin_amdgcn_sched_barrier(0);   // keep the loads ahead of the MFMAs
    }

    f32x4 s0 = f32x4{0.f, 0.f, 0.f, 0.f}, s1 = s0;
    #pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      s0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k0[ks], qf[ks], s0, 0, 0, 0);
      s1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k1[ks], qf[ks], s1, 0, 0, 0);
    }
    const int hi1 = two ? hi : 0;        // masks the duplicate tile
    const int row0 = t0 * TILE + 4 * g, row1 = t1 * TILE + 4 * g;
    float tmax = -INFINITY;
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      s0[r] = (row0 + r < hi) ? s0[r] * scale : -INFINITY;
      s1[r] = (row1 + r < hi1) ? s1[r] * scale : -INFINITY;
      tmax = fmaxf(tmax, fmaxf(s0[r], s1[r]));
    }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 16, WAVE));
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, WAVE));
    // the first tile's first row is always valid, so m_new is finite
    const float m_new = fmaxf(m_run, tmax);
    const float alpha = __expf(m_run - m_new);   // 0 on the wave's first pair
    bf16x8 pf;
    float psum = 0.f;
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float p0 = __expf(s0[r] - m_new), p1 = __expf(s1[r] - m_new);
      psum += p0 + p1;
      pf[r] = f2bf(p0);
      pf[4 + r] = f2bf(p1);
    }
    l_run = l_run * alpha + psum;
    m_run = m_new;
    #pragma unroll
    for (int m = 0; m < HEAD_DIM / TILE; ++m) {
      // element m of the eight V rows: dword m >> 1, low or high half
      const uint32_t sel = (m & 1) ? 0x07060302u : 0x05040100u;
      const int d = m >> 1;
      const u32x4 vt = u32x4{__builtin_amdgcn_perm(v0[1][d], v0[0][d], sel),
                             __builtin_amdgcn_perm(v0[3][d], v0[2][d], sel),
                             __builtin_amdgcn_perm(v1[1][d], v1[0][d], sel),
                             __builtin_amdgcn_perm(v1[3][d], v1[2][d], sel)};
      acc[m] *= alpha;
      acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          __builtin_bit_cast(bf16x8, vt), pf, acc[m], 0, 0, 0);
    }
  }

  // ---- combine the 4 waves' partials in wave order
  l_run += __shfl_xor(l_run, 16, WAVE);
  l_run += __shfl_xor(l_run, 32, WAVE);
  if (n < QH_PER_KV) {
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      float* dst = &o_s[wave][n][32 * g + 8 * r];
      *reinterpret_cast<f32x4*>(dst) =
          f32x4{acc[0][r], acc[1][r], acc[2][r], acc[3][r]};
      *reinterpret_cast<f32x4*>(dst + 4) =
          f32x4{acc[4][r], acc[5][r], acc[6][r], acc[7][r]};
    }
    if (g == 0) { ml_s[wave][n][0] = m_run; ml_s[wave][n][1] = l_run; }
  }
  __syncthreads();

  float mw[SPLIT_WAVES], m_star = -INFINITY;
  #pragma unroll
  for (int w = 0; w < SPLIT_WAVES; ++w) {
    mw[w] = ml_s[w][h][0];
    m_star = fmaxf(m_star, mw[w]);
  }
  // a wave without tiles holds (m = -inf, l = 0, zeros): f = 0 adds exactly +0
  float l_tot = 0.f;
  f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
  #pragma unroll
  for (int w = 0; w < SPLIT_WAVES; ++w) {
    const float f = (mw[w] == -INFINITY) ? 0.f : __expf(mw[w] - m_star);
    l_tot += ml_s[w][h][1] * f;
    o += *reinterpret_cast<const f32x4*>(&o_s[w][h][sub * 4]) * f;
  }
  if (sub == 0) { ml[0] = m_star; ml[1] = l_tot; }
  *reinterpret_cast<f32x4*>(acc_out + sub * 4) = o;
}

// merge: one wave per (t, hq); lane d-pairs combine the NSPLITS partials
template <int NS>
__global__ __launch_bounds__(128)
void paged_attn_merge_kernel(short* __restrict__ out,       // [T, Hq, D]
                             const float* __restrict__ part,
                             const float* __restrict__ part_ml,
                             int n_qheads) {
  const int t = blockIdx.x;
  const int hq = blockIdx.y;
  const int d = threadIdx.x;  // 128 threads = one dim each
  const float* ml = part_ml + (((long)t * n_qheads + hq) * NSPLITS_MAX) * 2;
  const float* pacc = part + (((long)t * n_qheads + hq) * NSPLITS_MAX) * HEAD_DIM;

  // Every load is issued before the first use: the partials were written by
  // workgroups on other XCDs, so each load is an Infinity-Cache/HBM round trip
  // and a load-wait-use loop over the splits pays NS of them in series.
  float mv[NS], lv[NS], pv[NS];
  #pragma unroll
  for (int s = 0; s < NS; ++s) {
    mv[s] = ml[2 * s];
    lv[s] = ml[2 * s + 1];
    pv[s] = pacc[(long)s * HEAD_DIM + d];
  }
  float m_star = -INFINITY;
  #pragma unroll
  for (int s = 0; s < NS; ++s) m_star = fmaxf(m_star, mv[s]);
  // Branch-free, in split order. An empty split holds (m = -inf, l = 0,
  // zeros), so with f = 0 it adds exactly +0 to both sums.
  float l_tot = 0.f, a = 0.f;
  #pragma unroll
  for (int s = 0; s < NS; ++s) {
    const float f = (mv[s] == -INFINITY) ? 0.f : __expf(mv[s] - m_star);
    l_tot += lv[s] * f;
    a += pv[s] * f;
  }
  out[((long)t * n_qheads + hq) * HEAD_DIM + d] =
      f2bf(l_tot > 0.f ? a / l_tot : 0.f);
}

int64_t attn_nsplits() { return NSPLITS_MAX; }

void paged_attention_split(torch::Tensor out, torch::Tensor q,
                           torch::Tensor kcache, torch::Tensor vcache,
                           torch::Tensor block_table, torch::Tensor seq_ids,
                           torch::Tensor q_pos, torch::Tensor part,
                           torch::Tensor part_ml, double scale,
                           int64_t splits,
                           c10::optional<torch::Tensor> k_scale,
                           c10::optional<torch::Tensor> v_scale) {
  OpChecks c("paged_attention_split");
  const bool fp8 = kv_fp8_check(c, kcache, vcache, k_scale, v_scale);
  c.require(splits == 32 || splits == 64, "splits = ", splits,
            " must be 32 or 64");
  const int T = attn_check_tokens(c, out, q, kcache, block_table, seq_ids, q_pos);
  const int n_kvheads = kcache.size(1);
  const int n_qheads = n_kvheads * QH_PER_KV;
  // the partials may be allocated for more tokens than this call has
  c.tensor("part", part, kF32, {-1, n_qheads, NSPLITS_MAX, HEAD_DIM});
  c.tensor("part_ml", part_ml, kF32, {-1, n_qheads, NSPLITS_MAX, 2});
  c.require(part.size(0) >= T && part_ml.size(0) >= T,
            "part and part_ml hold fewer than the ", T, " tokens of q");
  c.grid(T, n_kvheads, splits);
  c.grid(T, n_qheads);
  if (check_only()) return;
  const int max_blocks = block_table.size(1);
  hipStream_t s = c10::hip::getCurrentHIPStream();
  dim3 g1(T, n_kvheads, (unsigned)splits);
  if (fp8)
    hipLaunchKernelGGL(paged_attn_split_kernel<true>, g1, dim3(256), 0, s,
                       part.data_ptr<float>(), part_ml.data_ptr<float>(),
                       (const short*)q.data_ptr(),
                       (const uint8_t*)kcache.data_ptr(),
                       (const uint8_t*)vcache.data_ptr(),
                       block_table.data_ptr<int>(), seq_ids.data_ptr<int>(),
                       q_pos.data_ptr<int>(), n_kvheads, max_blocks,
                       (int)q.stride(0), (float)scale,
                       k_scale->data_ptr<float>(), v_scale->data_ptr<float>());
  else
    hipLaunchKernelGGL(paged_attn_split_kernel<false>, g1, dim3(256), 0, s,
                       part.data_ptr<float>(), part_ml.data_ptr<float>(),
                       (const short*)q.data_ptr(),
                       (const short*)kcache.data_ptr(),
                       (const short*)vcache.data_ptr(),
                       block_table.data_ptr<int>(), seq_ids.data_ptr<int>(),
                       q_pos.data_ptr<int>(), n_kvheads, max_blocks,
                       (int)q.stride(0), (float)scale,
                       (const float*)nullptr, (const float*)nullptr);
  HIP_CHECK_KERNEL();
  dim3 g2(T, n_qheads);
  if (splits == 64)
    hipLaunchKernelGGL(paged_attn_merge_kernel<64>, g2, dim3(HEAD_DIM), 0, s,
                       (short*)out.data_ptr(), part.data_ptr<float>(),
                       part_ml.data_ptr<float>(), n_qheads);
  else
    hipLaunchKernelGGL(paged_attn_merge_kernel<32>, g2, dim3(HEAD_DIM), 0, s,
                       (short*)out.data_ptr(), part.data_ptr<float>(),
                       part_ml.data_ptr<float>(), n_qheads);
  HIP_CHECK_KERNEL();
}
