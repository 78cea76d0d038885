// What the five MLA decode bindings (torch_binding_mla.cpp, _mla_ragged.cpp, _mla_fp8.cpp, _mla_sparse.cpp, _mla_sparse_fp8.cpp)
// share beyond torch_binding_decode.h, written once: the checks of q [B, H, S_q, 576], of the latent pool as each binding
// describes it (Pool), of kv_new, `out` and the index lists, the placement checks, and the tail of a call as one struct, MlaCall,
// filled by prepare_mla.  A binding keeps the order of its checks, its workspace call and its C call; the packed binding keeps
// the checks whose wording is its own ("packed q", "the latent pool") and takes the pool's conditions and the tail from here.
// The order and the text of every check are a recorded surface (tests/golden/quant_errors.json, mla_errors.json).
// Host code only; include after the C headers.
#pragma once
#include <string>

#include "torch_binding_decode.h"

namespace {

inline std::string num(int64_t v) { return std::to_string((long long)v); }

// The latent pool [num_pages, page_size, row]: rows of 576 values in q's dtype with element strides, or (fp8) 656 bytes in a
// uint8 tensor with byte strides.  Either way rows and pages start on 16-byte boundaries: `gran` elements.
struct Pool {
  bool fp8;
  int64_t row() const { return fp8 ? 656 : 576; }
  int64_t gran() const { return fp8 ? 16 : 8; }
};

// Can the kernels address q [B, H, S_q, 576] / out [B, H, S_q, 512] in place?  (an output's rows are distinct memory)
inline bool rows_ok(const Tensor& t, bool output) {
  if (t.stride(3) != 1 || (t.size(2) > 1 && t.stride(2) < t.size(3))) return false;
  for (int i = 0; i < 3; ++i)
    if (t.size(i) != 1 && (t.stride(i) < 0 || t.stride(i) % 8 != 0 || (output && t.stride(i) == 0))) return false;
  return true;
}
// ... and the pool?  It is never copied -- the append writes it --, so anything else is refused.
inline bool pool_in_place(const Tensor& KV, Pool pool) {
  return KV.stride(2) == 1 && KV.stride(1) >= pool.row() && KV.stride(1) % pool.gran() == 0 &&
         (KV.size(0) == 1 || (KV.stride(0) >= 0 && KV.stride(0) % pool.gran() == 0));
}

inline void check_q(const Tensor& Q) {
  FA_ASSERT(Q.dim() == 4, "q must be [B, H, S_q, 576] (got " + num(Q.dim()) + " dims)");
  FA_ASSERT(Q.size(3) == 576, "q's last dim must be 576: 512 latent dims, then 64 RoPE dims (got " + num(Q.size(3)) + ")");
}
inline void check_pool_shape(const Tensor& KV, Pool pool) {
  FA_ASSERT(KV.dim() == 3, (pool.fp8 ? "kv_cache must be [num_pages, page_size, 656]: one latent head (got "
                                     : "kv_cache must be [num_pages, page_size, 576]: one latent head (got ") + num(KV.dim()) + " dims)");
  FA_ASSERT(KV.size(2) == pool.row(), (pool.fp8 ? "kv_cache's last dim must be 656 bytes (got " : "kv_cache's last dim must be 576 (got ") +
                                          num(KV.size(2)) + ")");
}
inline void check_q_dtype(const Tensor& Q) {
  FA_ASSERT(Q.scalar_type() == at::kHalf || Q.scalar_type() == at::kBFloat16, "q's dtype must be float16 or bfloat16");
}
inline void check_pool_dtype(const Tensor& KV, const Tensor& Q, Pool pool) {
  if (pool.fp8)
    FA_ASSERT(KV.scalar_type() == at::kByte,
              "kv_cache must be torch.uint8: rows of 512 e4m3 bytes, 4 fp32 scales and 64 RoPE values in q's dtype");
  else
    FA_ASSERT(KV.scalar_type() == Q.scalar_type(), "kv_cache must have q's dtype");
}
inline void check_sizes(const Tensor& Q, const Tensor& KV) {
  FA_ASSERT(Q.size(0) >= 1 && Q.size(1) >= 1 && Q.size(2) >= 1 && KV.size(0) >= 1, "q and kv_cache must not be empty");
  FA_ASSERT(KV.size(1) >= 32 && KV.size(1) % 32 == 0,
            "the page size (kv_cache.shape[1] = " + num(KV.size(1)) + ") must be a positive multiple of 32");
}
// the index lists [B, S_q, topk] of the two sparse bindings
inline void check_indices(const Tensor& indices, int64_t B, int64_t Sq) {
  FA_ASSERT(indices.scalar_type() == at::kInt && indices.dim() == 3 && indices.size(0) == B && indices.size(1) == Sq &&
                indices.size(2) >= 1 && indices.size(2) <= (1 << 24),
            "indices must be an int32 tensor [B, S_q, topk] with 1 <= topk <= 2^24");
  FA_ASSERT((indices.size(2) == 1 || indices.stride(2) == 1) && (B == 1 || indices.stride(0) >= 0) && (Sq == 1 || indices.stride(1) >= 0),
            "indices must have unit stride along topk and non-negative batch and row strides");
}
inline void check_pool_in_place(const Tensor& KV, Pool pool) {
  FA_ASSERT(pool_in_place(KV, pool),
            pool.fp8 ? "kv_cache must be addressable in place: unit stride along the 656 bytes, a row stride that is a multiple of 16 bytes "
                       "(got " + num(KV.stride(1)) + ") and a page stride that is a multiple of 16 bytes"
                     : "kv_cache must be addressable in place: unit stride along the 576 dims, 16-byte aligned rows (a row stride that is a "
                       "multiple of 8 elements, got " + num(KV.stride(1)) + ") and a page stride that is a multiple of 8 elements");
}
inline void check_new_and_out(const OptTensor& kv_new, const OptTensor& out, const Tensor& Q, Pool pool) {
  const int64_t B = Q.size(0), H = Q.size(1), Sq = Q.size(2);
  if (kv_new.has_value()) {
    FA_ASSERT(kv_new->dim() == 3 && kv_new->size(0) == B && kv_new->size(1) == Sq && kv_new->size(2) == 576,
              pool.fp8 ? "kv_new must be [B, S_q, 576]: one unquantised row per query row"
                       : "kv_new must be [B, S_q, 576]: one cached row per query row");
    FA_ASSERT(kv_new->scalar_type() == Q.scalar_type() && !kv_new->requires_grad(),
              "kv_new must have q's dtype and must not require grad");
  }
  if (out.has_value()) {
    FA_ASSERT(out->dim() == 4 && out->size(0) == B && out->size(1) == H && out->size(2) == Sq && out->size(3) == 512 &&
                  out->scalar_type() == Q.scalar_type(),
              "out must be [B, H, S_q, 512] in q's dtype");
    FA_ASSERT(rows_ok(*out, true) && !out->requires_grad(),
              "out must be addressable in place (unit stride along the 512 dims, strides that are non-zero multiples of 8 "
              "elements) and must not require grad");
  }
}
// The checks that need a device, behind the binding's own no-grad check.  list: the sparse bindings' indices, or nullptr.
inline void check_placement(const Tensor& Q, const Tensor& KV, const Tensor* list, const Tensor& seqlens, const Tensor& table,
                            const OptTensor& kv_new, const OptTensor& out) {
  FA_ASSERT(Q.is_cuda() && KV.is_cuda() && (!list || list->is_cuda()) && seqlens.is_cuda() && table.is_cuda(),
            list ? "q, kv_cache, indices, cache_seqlens and block_table must be device tensors"
                 : "q, kv_cache, cache_seqlens and block_table must be device tensors");
  FA_ASSERT(KV.device() == Q.device() && (!list || list->device() == Q.device()) && seqlens.device() == Q.device() &&
                table.device() == Q.device() && (!kv_new.has_value() || kv_new->device() == Q.device()) &&
                (!out.has_value() || out->device() == Q.device()),
            "all tensors must be on q's device");
  FA_ASSERT(reinterpret_cast<uintptr_t>(KV.data_ptr()) % 16 == 0 && (!out.has_value() || reinterpret_cast<uintptr_t>(out->data_ptr()) % 16 == 0),
            "kv_cache and out must be 16-byte aligned");
  FA_ASSERT(KV.size(0) <= INT32_MAX && table.size(1) <= INT32_MAX && Q.size(0) <= INT32_MAX && Q.size(1) <= INT32_MAX &&
                Q.size(2) <= INT32_MAX,
            "too many pages, sequences, heads or rows");
}

// ---- the tail of a call ---------------------------------------------------------------------------------------------------------
// What the C call takes, prepared: q as the kernels read it (in place through its strides when they can, a contiguous copy
// otherwise), kv_new contiguous (undefined: no append), O (the caller's `out`, written in place, if it gives one) and LSE from
// the caching allocator on q's device, the page geometry, the scale (softmax_scale <= 0: 576 ** -0.5) and the stride arrays:
// qs / os {batch, head, row}, or {row, head} of a packed call; ks {page, row} in the pool's unit.
struct MlaCall {
  Tensor Qp, Kn, O, LSE;
  int S_new = 0, page = 0, num_pages = 0, max_pages = 0;
  float scale = 0.f;
  long long qs[3], os[3], ks[2];
  c10::OptionalDeviceGuard guard;
  MlaCall() = default;
  MlaCall(const MlaCall&) = delete;
  const void* kn() const { return Kn.defined() ? Kn.data_ptr() : nullptr; }
};
inline void prepare_mla(MlaCall& c, const Tensor& Q, const Tensor& KV, const Tensor& table, const OptTensor& kv_new,
                        const OptTensor& out, double softmax_scale, bool packed) {
  const bool in_place = packed ? packed_ok(Q, false) : reinterpret_cast<uintptr_t>(Q.data_ptr()) % 16 == 0 && rows_ok(Q, false);
  c.Qp = in_place ? Q : Q.clone(at::MemoryFormat::Contiguous);
  if (kv_new.has_value()) {
    c.Kn = contiguous16(*kv_new);
    c.S_new = packed ? 1 : (int)Q.size(2);
  }
  c.page = (int)KV.size(1), c.num_pages = (int)KV.size(0), c.max_pages = (int)table.size(1);
  c.scale = softmax_scale > 0.0 ? (float)softmax_scale : (float)(1.0 / std::sqrt(576.0));
  c.guard.reset_device(Q.device());
  std::vector<int64_t> o(Q.sizes().begin(), Q.sizes().end());
  o.back() = 512;
  c.O = out.has_value() ? *out : torch::empty(o, Q.options().memory_format(at::MemoryFormat::Contiguous));
  c.LSE = packed ? torch::empty({Q.size(1), Q.size(0)}, Q.options().dtype(at::kFloat))
                 : torch::empty({Q.size(0), Q.size(1), Q.size(2)}, Q.options().dtype(at::kFloat));
  if (packed) {
    long long q3[3], o3[3];   // packed_strides: {ignored, head, row}; the call takes {row, head}
    packed_strides(c.Qp, q3);
    packed_strides(c.O, o3);
    c.qs[0] = q3[2], c.qs[1] = q3[1], c.os[0] = o3[2], c.os[1] = o3[1];
  } else {
    strides3(c.Qp, c.qs);
    strides3(c.O, c.os);
  }
  c.ks[0] = KV.size(0) > 1 ? KV.stride(0) : KV.size(1) * KV.stride(1), c.ks[1] = KV.stride(1);
}

}  // namespace
