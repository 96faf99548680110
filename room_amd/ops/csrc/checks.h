// Argument checks for the op wrappers: the one vocabulary every wrapper uses.
//
// The rule: a wrong shape must be a Python error, never an out-of-bounds
// access. A wrapper reads: checks (each naming op and argument), then sizes,
// then the launch, and no data_ptr() reaches a launch unless that tensor's
// dtype, rank, sizes, contiguity (or permitted strides) and device were
// checked against the sizes the kernel is given.
//
// Checks read metadata only: no sync, no .item(), no copy, no allocation on
// the passing path. They run inside stream capture and on the eager decode
// path. What they cannot see is the CONTENTS of index tensors (block_table,
// seq_ids, q_pos / positions, pair_token, pair_expert, inv_order, tile_desc
// rows, cu_rows, pos_ids): those stay the caller's contract.
//
// Check-only mode (set_check_only, Python ops.check_only()): every wrapper
// returns after its checks and before its launch, and "on the GPU" relaxes to
// "all on one device", so the checks themselves can be tested on any host
// without launching anything on a bad shape.
#pragma once

#include <torch/extension.h>
#include <initializer_list>
#include <limits>
#include <sstream>
#include <string>

inline bool& check_only_flag() {
  static bool on = false;
  return on;
}
inline bool check_only() { return check_only_flag(); }
inline void set_check_only(bool on) { check_only_flag() = on; }

constexpr auto kBF16 = torch::kBFloat16;
constexpr auto kF32 = torch::kFloat32;
constexpr auto kI32 = torch::kInt32;
constexpr auto kI64 = torch::kInt64;
constexpr auto kFP8 = torch::kFloat8_e4m3fn;

// Carries the op name into every message and the device the op's tensors
// share: the first checked tensor sets it, every later one must match, so a
// tensor that was checked at all was checked for its device.
struct OpChecks {
  const char* op;
  const char* dev_of = nullptr;   // the argument that set dev
  c10::Device dev{c10::kCPU};

  explicit OpChecks(const char* op_) : op(op_) {}

  // t is a defined, contiguous tensor of this dtype and these sizes (-1 = any)
  void tensor(const char* name, const torch::Tensor& t, torch::ScalarType dtype,
              at::IntArrayRef dims) {
    if (!(shaped(t, dtype, dims) && t.is_contiguous()))
      fail(name, "contiguous ", t, dtype, dims);
    device(name, t);
  }

  // The row-strided views the attention ops accept (q as a view of the packed
  // qkv rows): sizes as above, everything inside a row dense, the row stride a
  // multiple of 8 elements and the first row 16-byte aligned (vector loads).
  void row_strided(const char* name, const torch::Tensor& t,
                   torch::ScalarType dtype, at::IntArrayRef dims) {
    bool ok = shaped(t, dtype, dims) && t.dim() >= 2;
    if (ok) {
      int64_t dense = 1;
      for (int64_t i = t.dim() - 1; i >= 1; --i) {
        ok = ok && t.stride(i) == dense;
        dense *= t.size(i);
      }
      ok = ok && t.stride(0) >= 0 && t.stride(0) % 8 == 0 &&
           reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
    }
    if (!ok) fail(name, "16-byte aligned rows (dense, row stride % 8 == 0) of ",
                  t, dtype, dims);
    device(name, t);
  }

  // A size that other arguments are measured against, read off the (already
  // checked) tensor that defines it: in lo..hi, or a positive multiple of m.
  // Either way it fits the kernel's int and comes back as one.
  int size_range(const char* name, const torch::Tensor& t, int d, int64_t lo,
                 int64_t hi) {
    const int64_t v = t.size(d);
    hi = std::min<int64_t>(hi, std::numeric_limits<int>::max());
    TORCH_CHECK(v >= lo && v <= hi, op, ": ", name, ".size(", d, ") = ", v,
                " must be in ", lo, "..", hi);
    return (int)v;
  }
  int size_multiple(const char* name, const torch::Tensor& t, int d, int64_t m) {
    const int64_t v = t.size(d);
    TORCH_CHECK(v >= m && v % m == 0 && v <= std::numeric_limits<int>::max(),
                op, ": ", name, ".size(", d, ") = ", v,
                " must be a positive multiple of ", m);
    return (int)v;
  }

  // v is passed to a kernel as int
  int fits_int(const char* name, int64_t v) {
    TORCH_CHECK(v >= 0 && v <= std::numeric_limits<int>::max(), op, ": ", name,
                " = ", v, " does not fit the kernel's int");
    return (int)v;
  }

  // launch dimensions; a zero extent is left to the launch itself
  void grid(int64_t x, int64_t y = 1, int64_t z = 1) {
    TORCH_CHECK(x >= 0 && x <= 2147483647LL && y >= 0 && y <= 65535 && z >= 0 &&
                z <= 65535, op, ": launch grid (", x, ", ", y, ", ", z,
                ") exceeds (2^31-1, 65535, 65535)");
  }

  void multiple(const char* name, int64_t v, int64_t m) {
    TORCH_CHECK(v >= m && v % m == 0, op, ": ", name, " = ", v,
                " must be a positive multiple of ", m);
  }

  void range(const char* name, int64_t v, int64_t lo, int64_t hi) {
    TORCH_CHECK(v >= lo && v <= hi, op, ": ", name, " = ", v, " must be in ",
                lo, "..", hi);
  }

  template <typename... Msg>
  void require(bool ok, const Msg&... msg) {
    TORCH_CHECK(ok, op, ": ", msg...);
  }

 private:
  static bool shaped(const torch::Tensor& t, torch::ScalarType dtype,
                     at::IntArrayRef dims) {
    if (!t.defined() || t.scalar_type() != dtype ||
        t.dim() != (int64_t)dims.size())
      return false;
    for (size_t i = 0; i < dims.size(); ++i)
      if (dims[i] >= 0 && t.size(i) != dims[i]) return false;
    return true;
  }

  void device(const char* name, const torch::Tensor& t) {
    if (!dev_of) {
      TORCH_CHECK(t.is_cuda() || check_only(), op, ": ", name,
                  " must be on the GPU, got ", t.device());
      dev = t.device();
      dev_of = name;
    }
    TORCH_CHECK(t.device() == dev, op, ": ", name, " is on ", t.device(),
                " but ", dev_of, " is on ", dev,
                "; all tensors of a call share one device");
  }

  [[noreturn]] void fail(const char* name, const char* layout,
                         const torch::Tensor& t, torch::ScalarType dtype,
                         at::IntArrayRef dims) const {
    std::ostringstream want, got;
    want << "[";
    for (size_t i = 0; i < dims.size(); ++i) {
      if (i) want << ", ";
      if (dims[i] < 0) want << "*"; else want << dims[i];
    }
    want << "]";
    if (t.defined())
      got << t.scalar_type() << " " << t.sizes() << " strides " << t.strides();
    else
      got << "an undefined tensor";
    TORCH_CHECK(false, op, ": ", name, " must be ", layout, dtype, " ",
                want.str(), ", got ", got.str());
  }
};

// the dtype of an output (or delta) that may be bf16 or f32
inline torch::ScalarType bf16_or_f32(const torch::Tensor& t) {
  return t.defined() && t.scalar_type() == kF32 ? kF32 : kBF16;
}

// ---------------------------------------------------------------- shared
// Contracts that several ops share. The bf16 / fp8 twins of an op call the
// same function and differ only in their weight arguments.

constexpr int64_t FP8_BLOCK = 128;   // scale block edge of the e4m3 weights

// bf16 expert weights [E, N, K] (E from the tensor)
inline void bf16_check_weights(OpChecks& c, const char* name,
                               const torch::Tensor& w, int64_t N, int64_t K) {
  c.tensor(name, w, kBF16, {-1, N, K});
  c.require(w.size(0) >= 1, name, " holds no expert");
}

// e4m3fn expert weights [E, N, K] with one f32 scale per 128x128 block
// [E, N/128, K/128]; N and K multiples of 128
inline void fp8_check_weights(OpChecks& c, const char* qname,
                              const torch::Tensor& q, const char* sname,
                              const torch::Tensor& s, int64_t N, int64_t K) {
  c.multiple("N (the weights' rows)", N, FP8_BLOCK);
  c.multiple("K (the weights' columns)", K, FP8_BLOCK);
  c.tensor(qname, q, kFP8, {-1, N, K});
  c.require(q.size(0) >= 1, qname, " holds no expert");
  c.tensor(sname, s, kF32, {q.size(0), N / FP8_BLOCK, K / FP8_BLOCK});
}

// the decode MoE pair vectors: one (token, expert) per row of h
inline void fp8_check_pairs(OpChecks& c, const torch::Tensor& pair_token,
                            const torch::Tensor& pair_expert, int64_t P) {
  c.tensor("pair_token", pair_token, kI32, {P});
  c.tensor("pair_expert", pair_expert, kI32, {P});
}

// Paged KV caches [NB, Hk, 16, 128], bf16, or e4m3fn with k_scale / v_scale
// [NB, Hk, 16] f32; scales are given exactly when the caches are e4m3.
// Returns whether this is the fp8 form.
inline bool kv_fp8_check(OpChecks& c, const torch::Tensor& kcache,
                         const torch::Tensor& vcache,
                         const c10::optional<torch::Tensor>& k_scale,
                         const c10::optional<torch::Tensor>& v_scale) {
  auto is_fp8 = [](const torch::Tensor& t) {
    return t.defined() && t.scalar_type() == kFP8;
  };
  // either cache in e4m3 selects the fp8 form; the other must then match
  const bool fp8 = is_fp8(kcache) || is_fp8(vcache);
  const auto dt = fp8 ? kFP8 : kBF16;
  c.tensor("kcache", kcache, dt, {-1, -1, 16, 128});
  c.tensor("vcache", vcache, dt, kcache.sizes());
  c.require(k_scale.has_value() == v_scale.has_value(),
            "k_scale and v_scale go together");
  c.require(!fp8 || k_scale.has_value(),
            "float8_e4m3fn kcache / vcache need k_scale and v_scale");
  c.require(fp8 || !k_scale.has_value(),
            "k_scale / v_scale given with bfloat16 kcache / vcache");
  if (fp8) {
    c.tensor("k_scale", *k_scale, kF32, {kcache.size(0), kcache.size(1), 16});
    c.tensor("v_scale", *v_scale, kF32, {kcache.size(0), kcache.size(1), 16});
  }
  c.fits_int("kcache.size(1)", kcache.size(1));
  return fp8;
}

// How the attention ops and the KV writers find a token's cache rows: the
// block table [S, MB] and one sequence id per token.
inline void check_paging(OpChecks& c, const torch::Tensor& block_table,
                         const torch::Tensor& seq_ids, int64_t T) {
  c.tensor("block_table", block_table, kI32, {-1, -1});
  c.fits_int("block_table.size(1)", block_table.size(1));
  c.tensor("seq_ids", seq_ids, kI32, {T});
}

// The per-token arguments of the three attention ops, after kv_fp8_check:
// q [T, Hq, 128] with Hq = 8 Hk (GQA 8:1; q may be a row-strided view of the
// packed qkv), out contiguous and shaped like q, the paging tensors and one
// position per token. Returns T.
inline int attn_check_tokens(OpChecks& c, const torch::Tensor& out,
                             const torch::Tensor& q, const torch::Tensor& kcache,
                             const torch::Tensor& block_table,
                             const torch::Tensor& seq_ids,
                             const torch::Tensor& q_pos) {
  const int64_t n_qheads = kcache.size(1) * 8;
  c.row_strided("q", q, kBF16, {-1, n_qheads, 128});
  const int T = c.fits_int("q.size(0)", q.size(0));
  c.fits_int("q.stride(0)", q.stride(0));
  c.tensor("out", out, kBF16, {T, n_qheads, 128});
  check_paging(c, block_table, seq_ids, T);
  c.tensor("q_pos", q_pos, kI32, {T});
  return T;
}

// moe_gemv_h / moe_gemv_h_fp8 apart from the weights: h [P, I] bf16, x [T, H]
// bf16, the pair vectors, and the optional f32 buffer zeroed as a side job.
inline void moe_gemv_h_check(OpChecks& c, const torch::Tensor& h,
                             const torch::Tensor& x,
                             const torch::Tensor& pair_token,
                             const torch::Tensor& pair_expert,
                             const torch::Tensor& out_zero) {
  c.tensor("h", h, kBF16, {-1, -1});
  c.tensor("x", x, kBF16, {-1, -1});
  const int64_t P = h.size(0), I = c.fits_int("h.size(1)", h.size(1));
  c.fits_int("x.size(1)", x.size(1));
  fp8_check_pairs(c, pair_token, pair_expert, P);
  c.grid(P, (I + 3) / 4);
  if (out_zero.defined() && out_zero.numel() > 0) {
    c.tensor("out_zero", out_zero, kF32, out_zero.sizes());
    c.require(out_zero.numel() <= P * ((I + 3) / 4) * 256,
              "out_zero is larger than the grid that zeroes it");
  }
}

// moe_gemv_down / moe_gemv_down_fp8 apart from the weights: out [T, H] f32,
// h [P, I] bf16 with I a multiple of 128, pair_w [P] f32, the pair vectors.
inline void moe_gemv_down_check(OpChecks& c, const torch::Tensor& out,
                                const torch::Tensor& h,
                                const torch::Tensor& pair_w,
                                const torch::Tensor& pair_token,
                                const torch::Tensor& pair_expert) {
  c.tensor("out", out, kF32, {-1, -1});
  c.tensor("h", h, kBF16, {-1, -1});
  const int64_t P = h.size(0), H = c.fits_int("out.size(1)", out.size(1));
  c.size_multiple("h", h, 1, 128);
  c.tensor("pair_w", pair_w, kF32, {P});
  fp8_check_pairs(c, pair_token, pair_expert, P);
  c.grid(P, (H + 15) / 16);
}

// The grouped GEMMs apart from the weights: out [P, N], x [T, K] bf16 with K a
// multiple of 64, pair_token [P], tile_desc [G, 3] int32.
//   moe_grouped_gemm_skinny / _fp8 (tiles of at most 16 rows): out bf16 or
//     f32, N a multiple of 16, 1..65535 tiles on grid.y
//   moe_grouped_gemm128 / _fp8 (at most 128 rows): out bf16, N a multiple of
//     64, the tiles on grid.x
inline void grouped_gemm_check(OpChecks& c, bool skinny,
                               const torch::Tensor& out, const torch::Tensor& x,
                               const torch::Tensor& pair_token,
                               const torch::Tensor& tile_desc) {
  c.tensor("x", x, kBF16, {-1, -1});
  c.size_multiple("x", x, 1, 64);
  c.tensor("out", out, skinny ? bf16_or_f32(out) : kBF16, {-1, -1});
  const int N = c.size_multiple("out", out, 1, skinny ? 16 : 64);
  c.tensor("pair_token", pair_token, kI32, {out.size(0)});
  c.tensor("tile_desc", tile_desc, kI32, {-1, 3});
  const int64_t G = tile_desc.size(0);
  if (skinny) {
    c.size_range("tile_desc", tile_desc, 0, 1, 65535);
    c.grid(N / 16, G);
  } else {
    c.grid(G, N / 64);
  }
}
