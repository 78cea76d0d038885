// What the PyTorch-ROCm bindings share -- torch_binding.cpp directly, the decode bindings (torch_binding_paged.cpp, _fp4.cpp,
// _fp8_token.cpp, _quant_softcap.cpp, _mla.cpp) through torch_binding_decode.h, which holds what only they share: how a bad
// argument is raised, and the checks and stride helpers that are the same in more than one of them.  Host code only; each
// binding is one translation unit and includes this after the C headers (check_rc names their fa_last_error()).
// Not here, because they differ: torch_binding.cpp's strided_ok / strides3 (a null result for a contiguous tensor, a copy
// where the others refuse) and its check_rc for plain return codes.
#pragma once
#include <torch/extension.h>

#include <string>

namespace {

using torch::Tensor;
using OptTensor = c10::optional<Tensor>;

// bad arguments raise AssertionError, as everywhere in the package (the reference does, M:133-136)
[[noreturn]] inline void assertion(const std::string& msg) {
  PyErr_SetString(PyExc_AssertionError, msg.c_str());
  throw pybind11::error_already_set();
}
#define FA_ASSERT(cond, msg) \
  do {                       \
    if (!(cond)) assertion(msg); \
  } while (0)

// a return code or a workspace function's byte count: negative is the library's refusal
inline void check_rc(long long rc, const char* what) {
  if (rc < 0) throw std::runtime_error(std::string(what) + " failed (code " + std::to_string(rc) + "): " + fa_last_error());
}

// a tensor the kernels read as contiguous 16-byte aligned rows: itself, or a copy
inline Tensor contiguous16(const Tensor& t) {
  return (t.is_contiguous() && reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0) ? t : t.clone(at::MemoryFormat::Contiguous);
}

// element strides {batch | page, head, row} of a 4-d tensor addressed in place, a size-1 dimension with a harmless one
inline void strides3(const Tensor& t, long long* v) {
  v[0] = t.size(0) > 1 ? t.stride(0) : t.size(1) * t.size(2) * t.size(3);
  v[1] = t.size(1) > 1 ? t.stride(1) : 0;
  v[2] = t.size(2) > 1 ? t.stride(2) : t.size(3);
}
// q [B, H, S_q, D]: contiguous, or rows of unit head-dim stride and strides that are multiples of 8 elements
inline bool dense_ok(const Tensor& t) {
  if (reinterpret_cast<uintptr_t>(t.data_ptr()) % 16) return false;
  if (t.is_contiguous()) return true;
  bool ok = t.stride(3) == 1 && t.stride(2) >= t.size(3);
  for (int i = 0; i < 3 && ok; ++i) ok = t.size(i) == 1 || (t.stride(i) >= 0 && t.stride(i) % 8 == 0);
  return ok;
}

// an fp32 vector of a call (`what`: its name), once its dtype and shape are checked
inline void check_vec_placement(const Tensor& t, const std::string& what, const c10::Device& dev) {
  FA_ASSERT(t.is_contiguous() && !t.requires_grad(), what + " must be contiguous and must not require grad");
  FA_ASSERT(t.is_cuda() && t.device() == dev, what + " must be a device tensor on q's device");
}

// block_table of a paged call with B sequences
inline void check_block_table(const Tensor& table, int64_t B) {
  FA_ASSERT(table.scalar_type() == at::kInt && table.dim() == 2 && table.size(0) == B && table.size(1) >= 1 &&
                (table.size(1) == 1 || table.stride(1) == 1) && (B == 1 || table.stride(0) >= table.size(1)),
            "block_table must be an int32 tensor [B, max_pages_per_seq] with unit stride along the pages");
}

// k_new / v_new [B, H_kv, S_new, D] of a call, and (packed ones too) where they live
inline void check_new_shape(const Tensor& k_new, const Tensor& v_new, int64_t B, int64_t Hk, int64_t D) {
  FA_ASSERT(k_new.dim() == 4 && k_new.sizes() == v_new.sizes() && k_new.size(0) == B && k_new.size(1) == Hk &&
                k_new.size(3) == D && k_new.size(2) >= 1,
            "k_new and v_new must be [B, H_kv, S_new, D] with S_new >= 1");
}
inline void check_new_placement(const Tensor& k_new, const Tensor& v_new, const Tensor& Q) {
  FA_ASSERT(k_new.device() == Q.device() && v_new.device() == Q.device() && k_new.scalar_type() == Q.scalar_type() &&
                v_new.scalar_type() == Q.scalar_type() && !k_new.requires_grad() && !v_new.requires_grad(),
            "k_new and v_new must be on q's device with q's dtype and must not require grad");
}

// ---- packed variable-length queries (include/mi355fa_ragged.h, include/mi355fa_ragged_fp4.h): what the two packed calls
// share, whatever their pools hold ----
// The geometry of the queries.  cu == nullptr: q [B, H, S_q, D], k_new / v_new [B, H_kv, S_new, D]; otherwise packed q
// [total_q, H, D] with cu_seqlens_q [B + 1], k_new / v_new [total_q, H_kv, D] and an optional `out` written in place.
struct Queries {
  const Tensor* cu = nullptr;
  const c10::optional<Tensor>* out = nullptr;
};

// Can the kernels address the packed [total_q, H, D] tensor in place?  A 16-byte aligned base, D innermost, head and row
// strides that are multiples of 8 elements (16-byte rows), rows at least D apart; an output's heads and rows are distinct
// memory.  A size-1 dimension may carry any stride: packed_strides gives it a harmless one.
inline bool packed_ok(const Tensor& t, bool output) {
  if (reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 || t.stride(2) != 1) return false;
  if (t.size(0) > 1 && (t.stride(0) < t.size(2) || t.stride(0) % 8 != 0 || t.stride(0) >= (1ll << 30))) return false;
  if (t.size(1) > 1 && (t.stride(1) < 0 || t.stride(1) % 8 != 0 || t.stride(1) >= (1ll << 30))) return false;
  if (output && t.size(1) > 1 && t.stride(1) < t.size(2)) return false;
  return true;
}
inline void packed_strides(const Tensor& t, long long* v) {   // {ignored, head, row}
  v[0] = 0;
  v[1] = t.size(1) > 1 ? t.stride(1) : t.size(2);
  v[2] = t.size(0) > 1 ? t.stride(0) : t.size(1) * t.size(2);
}

inline void check_cu_seqlens(const Tensor& cu) {
  FA_ASSERT(cu.scalar_type() == at::kInt && cu.dim() == 1 && cu.numel() >= 2 && cu.is_contiguous(),
            "cu_seqlens_q must be a contiguous int32 vector of B + 1 entries");
}

// packed k_new / v_new of a step with Tq query rows
inline void check_new_shape_packed(const Tensor& k_new, const Tensor& v_new, int64_t Tq, int64_t Hk, int64_t D) {
  FA_ASSERT(k_new.dim() == 3 && k_new.sizes() == v_new.sizes() && k_new.size(0) == Tq && k_new.size(1) == Hk && k_new.size(2) == D,
            "k_new and v_new must be [total_q, H_kv, D]: one key and one value per query row");
}

// The result of a packed call: `out`, written in place through its strides -- a result the caller asked for here is never
// produced in a copy --, or a new contiguous tensor.
inline Tensor packed_result(const c10::optional<Tensor>& out, const Tensor& Q) {
  if (!out.has_value()) return torch::empty(Q.sizes(), Q.options().memory_format(at::MemoryFormat::Contiguous));
  FA_ASSERT(out->sizes() == Q.sizes() && out->scalar_type() == Q.scalar_type(), "out must have q's shape and dtype");
  FA_ASSERT(out->is_cuda() && out->device() == Q.device() && !out->requires_grad(),
            "out must be on q's device and must not require grad");
  FA_ASSERT(packed_ok(*out, true),
            "out must be addressable in place: 16-byte aligned rows with unit head-dim stride, head and row strides that are "
            "multiples of 8 elements");
  return *out;
}

}  // namespace
