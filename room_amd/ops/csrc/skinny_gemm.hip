// Skinny grouped MFMA GEMM for wide decode (9..64 rows) on CDNA4 (gfx950).
//
//   out[row0+m, n] = Σ_k x[pair_token[row0+m], k] · w[e, n, k]
//
// over tiles (e, row0, msize) from a [G,3] descriptor (the format of
// moe_grouped_gemm128), or one dense tile (e=0, row0=0, msize=M). bf16 in,
// f32 accumulate, bf16 or f32 out.
//
// At M ≤ 64 the work is weight-bandwidth-bound, so the weights never touch
// LDS: a workgroup owns one 16-column fragment of one tile, its NW waves
// split K, and each wave loads its weight slices from HBM straight into the
// VGPRs that feed the MFMA. K is cut into 64-wide chunks (one 128-B line of
// every weight row); wave v owns chunks v, v+NW, v+2NW, ... in ascending
// order, and the loads of U chunks are issued before their first MFMA.
//
// k-permutation (shared by both operands): inside a chunk the 16-lane group
// g = lane>>4 owns the 16 consecutive k values [16g, 16g+16) — 32 B per
// lane, the four groups cover the whole 128-B line — and feeds two
// mfma_f32_16x16x32_bf16: elements 0..7 are the group's k-slice of the
// first, elements 8..15 of the second. A sum over k does not care about the
// order as long as A and B agree on it.
//
// Operands: A = w (rows n), B = xᵀ (columns m), so C[n][m] (layouts above
// moe_grouped_gemm128_kernel): lane l, reg r holds out[m = l&15][n0 +
// (l>>4)*4 + r] — four consecutive n per lane, one 8/16-B store.
//
// x: with this decomposition no two waves of a workgroup read the same x
// element (a chunk has one owner), so an LDS stage has nothing to share. The
// first version staged x through LDS all the same (full lines, padded rows,
// barriers every 256·XR k): at 64 rows the staging, not the weights, set the
// time (QKV 24.8 µs at M=64 against 8.6 at M=16; docs/KERNELS.md). The same
// k-permutation makes the direct load line-shaped too — a wave's x operand
// for one chunk is the full 128-B line of each of its 16 rows — so x is read
// from L2 straight into the B operand, and the main loop has no barrier.
// Rows ≥ msize re-read the tile's last row: an MFMA column depends on its
// own B column only, and those columns are never stored.
//
// Row independence: which chunks a wave owns, the order it accumulates them
// in and the order the wave partials are summed in (p0+p1)+p2+... depend on
// (N, K) alone through NW — not on M, the tile height, the row's place in
// the tile or its neighbours (U only batches loads). An output therefore has
// the same bits in every instantiation, whoever shares its batch.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include "common.h"
#include "checks.h"

// MF: 16-row MFMA fragments per tile (BM = 16·MF). NW: waves per workgroup
// (the K split). U: chunks per wave with loads in flight together, (1+MF)·8
// VGPRs each.
template <int MF, int NW, int U>
__global__ __launch_bounds__(NW * 64)
void skinny_gemm_kernel(void* __restrict__ out,             // [rows, N]
                        const short* __restrict__ x,         // [T, K]
                        const short* __restrict__ w,         // [E, N, K]
                        const int* __restrict__ pair_token,  // [rows] or null
                        const int* __restrict__ tile_desc,   // [G,3] or null
                        int M, int K, int N, int f32out) {
  // cross-wave reduction buffer: the kernel's only LDS
  __shared__ f32x4 red[NW * MF * 64];

  int e = 0, row0 = 0, msize = M;
  if (tile_desc != nullptr) {
    const int g = blockIdx.y;
    msize = tile_desc[g * 3 + 2];
    if (msize == 0) return;             // past the live tile count
    e = tile_desc[g * 3 + 0];
    row0 = tile_desc[g * 3 + 1];
  }
  const int n0 = blockIdx.x * 16;
  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int fr = lane & 15;             // A row (n) / B column (m)
  const int fg = lane >> 4;             // 16-lane group: k [16fg, 16fg+16)
  const int C = K / 64;                 // chunks

  const short* wrow = w + ((long)e * N + n0 + fr) * K + fg * 16;
  const short* xrow[MF];
  #pragma unroll
  for (int mf = 0; mf < MF; ++mf) {
    const int m = min(mf * 16 + fr, msize - 1);
    const int tok = pair_token != nullptr ? pair_token[row0 + m] : row0 + m;
    xrow[mf] = x + (long)tok * K + fg * 16;
  }

  f32x4 acc[MF];
  #pragma unroll
  for (int mf = 0; mf < MF; ++mf) acc[mf] = f32x4{0.f, 0.f, 0.f, 0.f};

  int c = wid;
  // groups of U chunks: every load of the group issued before its first MFMA
  for (; c + (U - 1) * NW < C; c += U * NW) {
    bf16x8 wv[U][2], xv[U][MF][2];
    #pragma unroll
    for (int u = 0; u < U; ++u) {
      const long ko = (long)(c + u * NW) * 64;
      wv[u][0] = *reinterpret_cast<const bf16x8*>(wrow + ko);
      wv[u][1] = *reinterpret_cast<const bf16x8*>(wrow + ko + 8);
    }
    #pragma unroll
    for (int u = 0; u < U; ++u) {
      const long ko = (long)(c + u * NW) * 64;
      #pragma unroll
      for (int mf = 0; mf < MF; ++mf) {
        xv[u][mf][0] = *reinterpret_cast<const bf16x8*>(xrow[mf] + ko);
        xv[u][mf][1] = *reinterpret_cast<const bf16x8*>(xrow[mf] + ko + 8);
      }
    }
    __builtin_amdgcn_sched_barrier(0);   // keep the loads ahead of the MFMAs
    #pragma unroll
    for (int u = 0; u < U; ++u) {
      #pragma unroll
      for (int mf = 0; mf < MF; ++mf) {
        acc[mf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            wv[u][0], xv[u][mf][0], acc[mf], 0, 0, 0);
        acc[mf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            wv[u][1], xv[u][mf][1], acc[mf], 0, 0, 0);
      }
    }
  }
  // remaining chunks one at a time (same ascending order)
  for (; c < C; c += NW) {
    const long ko = (long)c * 64;
    const bf16x8 w0 = *reinterpret_cast<const bf16x8*>(wrow + ko);
    const bf16x8 w1 = *reinterpret_cast<const bf16x8*>(wrow + ko + 8);
    bf16x8 x0[MF], x1[MF];
    #pragma unroll
    for (int mf = 0; mf < MF; ++mf) {
      x0[mf] = *reinterpret_cast<const bf16x8*>(xrow[mf] + ko);
      x1[mf] = *reinterpret_cast<const bf16x8*>(xrow[mf] + ko + 8);
    }
    #pragma unroll
    for (int mf = 0; mf < MF; ++mf) {
      acc[mf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, x0[mf], acc[mf],
                                                        0, 0, 0);
      acc[mf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1, x1[mf], acc[mf],
                                                        0, 0, 0);
    }
  }

  // cross-wave reduction through LDS, fixed order (p0+p1)+p2+...
  #pragma unroll
  for (int mf = 0; mf < MF; ++mf) red[(wid * MF + mf) * 64 + lane] = acc[mf];
  __syncthreads();
  const int mf = wid;                   // wave v finishes fragment v (NW ≥ MF)
  if (mf < MF) {
    f32x4 s = red[mf * 64 + lane];
    #pragma unroll
    for (int v = 1; v < NW; ++v) s += red[(v * MF + mf) * 64 + lane];
    const int m = mf * 16 + fr;
    if (m < msize) {
      const long o = (long)(row0 + m) * N + n0 + fg * 4;
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

namespace {

template <int MF, int NW, int U>
void sk_launch(void* out, const short* x, const short* w, const int* pt,
               const int* desc, int G, int M, int K, int N, int f32out,
               hipStream_t s) {
  dim3 grid(N / 16, G), block(NW * 64);
  hipLaunchKernelGGL((skinny_gemm_kernel<MF, NW, U>), grid, block, 0, s, out,
                     x, w, pt, desc, M, K, N, f32out);
}

// Waves per workgroup from (N, K) alone — never from M, which would break
// row independence. Dense shapes with few column fragments (O: 128, router:
// 8) split K further until ~2048 waves are in flight or a wave would own
// fewer than 2 chunks; grouped launches have tiles × fragments workgroups.
int sk_waves(bool grouped, int K, int N) {
  int nw = 4;
  if (grouped) return nw;
  const int frags = N / 16, C = K / 64;
  while (nw < 16 && frags * nw < 2048 && C / (nw * 2) >= 2) nw *= 2;
  return nw;
}

// U: the largest load group that divides a wave's chunk count and keeps the
// loads in flight, U·(1+MF)·8 VGPRs, within 96 (128 at MF=1)
template <int MF, int NW>
void sk_dispatch_u(void* out, const short* x, const short* w, const int* pt,
                   const int* desc, int G, int M, int K, int N, int f32out,
                   hipStream_t s) {
  const int cpw = (K / 64 + NW - 1) / NW;
  #define SK_GO(U) sk_launch<MF, NW, U>(out, x, w, pt, desc, G, M, K, N, \
                                        f32out, s)
  // (16 waves cap a lane at 128 VGPRs: U=8 would spill there)
  if constexpr (MF == 1 && NW <= 8) { if (cpw % 8 == 0) { SK_GO(8); return; } }
  if constexpr (MF <= 2) { if (cpw % 4 == 0) { SK_GO(4); return; } }
  if constexpr (MF <= 3) { if (cpw % 3 == 0) { SK_GO(3); return; } }
  if (cpw % 2 == 0) { SK_GO(2); return; }
  SK_GO(1);
  #undef SK_GO
}

template <int MF>
void sk_dispatch_nw(int NW, void* out, const short* x, const short* w,
                    const int* pt, const int* desc, int G, int M, int K,
                    int N, int f32out, hipStream_t s) {
  switch (NW) {
    case 4: sk_dispatch_u<MF, 4>(out, x, w, pt, desc, G, M, K, N, f32out, s); break;
    case 8: sk_dispatch_u<MF, 8>(out, x, w, pt, desc, G, M, K, N, f32out, s); break;
    default: sk_dispatch_u<MF, 16>(out, x, w, pt, desc, G, M, K, N, f32out, s); break;
  }
}

void sk_dispatch(int MF, int NW, void* out, const short* x, const short* w,
                 const int* pt, const int* desc, int G, int M, int K, int N,
                 int f32out, hipStream_t s) {
  switch (MF) {
    case 1: sk_dispatch_nw<1>(NW, out, x, w, pt, desc, G, M, K, N, f32out, s); break;
    case 2: sk_dispatch_nw<2>(NW, out, x, w, pt, desc, G, M, K, N, f32out, s); break;
    case 3: sk_dispatch_nw<3>(NW, out, x, w, pt, desc, G, M, K, N, f32out, s); break;
    default: sk_dispatch_nw<4>(NW, out, x, w, pt, desc, G, M, K, N, f32out, s); break;
  }
}

}  // namespace

// y[M,N] = x[M,K] @ w[N,K]^T, 1 ≤ M ≤ 64: one tile, height from M
void skinny_gemm(torch::Tensor y, torch::Tensor x, torch::Tensor w) {
  OpChecks c("skinny_gemm");
  c.tensor("x", x, kBF16, {-1, -1});
  const int64_t M = c.size_range("x", x, 0, 1, 64);   // one tile, height from M
  const int64_t K = c.size_multiple("x", x, 1, 64);
  c.tensor("w", w, kBF16, {-1, K});
  const int64_t N = c.size_multiple("w", w, 0, 16);
  c.tensor("y", y, bf16_or_f32(y), {M, N});
  c.grid(N / 16);
  if (check_only()) return;
  hipStream_t s = c10::hip::getCurrentHIPStream();
  sk_dispatch((int)(M + 15) / 16, sk_waves(false, (int)K, (int)N),
              y.data_ptr(), (const short*)x.data_ptr(),
              (const short*)w.data_ptr(), nullptr, nullptr, 1, (int)M, (int)K,
              (int)N, y.dtype() == torch::kFloat32, s);
  HIP_CHECK_KERNEL();
}

// grouped, BM=16 tiles (tile_desc from moe_build_desc with bm=16)
void moe_grouped_gemm_skinny(torch::Tensor out, torch::Tensor x,
                             torch::Tensor w, torch::Tensor pair_token,
                             torch::Tensor tile_desc) {
  OpChecks c("moe_grouped_gemm_skinny");
  grouped_gemm_check(c, true, out, x, pair_token, tile_desc);
  const int64_t K = x.size(1), N = out.size(1), G = tile_desc.size(0);
  bf16_check_weights(c, "w", w, N, K);
  if (check_only()) return;
  hipStream_t s = c10::hip::getCurrentHIPStream();
  sk_dispatch(1, sk_waves(true, (int)K, (int)N), out.data_ptr(),
              (const short*)x.data_ptr(), (const short*)w.data_ptr(),
              pair_token.data_ptr<int>(), tile_desc.data_ptr<int>(), (int)G,
              16, (int)K, (int)N, out.dtype() == torch::kFloat32, s);
  HIP_CHECK_KERNEL();
}
