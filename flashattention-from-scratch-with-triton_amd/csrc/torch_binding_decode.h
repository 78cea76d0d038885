// What the decode bindings (torch_binding_paged.cpp, _fp4.cpp, _fp8_token.cpp, _quant_softcap.cpp and, for its few common
// lines, _mla.cpp) share beyond torch_binding_common.h, written once: the in-place conditions on byte caches and fp32 row scales,
// the fp32 vector arguments, the checks every quantised cache runs between those of its format and its in-place conditions, and
// the tail of a call as plain functions over one struct, DecodeCall.  A binding keeps the checks of its format, its workspace
// call and its launches: those argument lists differ.  The order of the checks is a recorded surface
// (tests/golden/paged_errors.json, quant_errors.json).
//
// What every one of these calls does: O (unless the caller gives `out`), LSE and the workspace come from the caching allocator;
// q / out, the caches and their scales are addressed in place through their strides -- caches and scales are written in place,
// with k_new / v_new --; the launch goes to the current stream; nothing synchronises or reads cu_seqlens_q, cache_seqlens,
// block_table, descales or scales, so a step can be captured in a graph.  Inference only: no autograd.
// Host code only; include after the C headers (mi355fa_opts and MI355FA_BF16 are theirs).
#pragma once
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <c10/core/DeviceGuard.h>

#include <cmath>
#include <tuple>

#include "torch_binding_common.h"

namespace {

// Can the kernels address the byte tensor [slices, H_kv, rows, rowb] in place?  A base aligned to `gran` bytes, unit stride
// along the row, strides that are multiples of `gran` and one (slice, head) slice inside 2^31 bytes.  Caches and scales are
// never copied -- the append writes them --, so anything else is refused.
inline bool bytes_ok(const Tensor& t, int64_t gran) {
  if (reinterpret_cast<uintptr_t>(t.data_ptr()) % gran || t.stride(3) != 1 || (t.size(2) > 1 && t.stride(2) < t.size(3))) return false;
  if ((t.size(2) - 1) * t.stride(2) + t.size(3) > ((1ll << 31) - 1)) return false;
  for (int i = 0; i < 3; ++i)
    if (t.size(i) != 1 && (t.stride(i) < 0 || t.stride(i) % gran != 0)) return false;
  return true;
}
inline void check_caches_in_place(const Tensor& Kc, const Tensor& Vc) {
  FA_ASSERT(bytes_ok(Kc, 16) && bytes_ok(Vc, 16) && (Kc.size(2) == 1 || Kc.stride(2) == Vc.stride(2)),
            "the caches must be addressable in place: 16-byte aligned rows with unit stride along the row, strides that are "
            "multiples of 16 bytes, one row stride for K and V");
}
// the fp32 row scales [slices, H_kv, rows]: any non-negative element strides, one (slice, head) slice inside 2^31 bytes
inline bool row_scales_ok(const Tensor& t) {
  for (int i = 0; i < 3; ++i)
    if (t.size(i) != 1 && t.stride(i) < 0) return false;
  return (t.size(2) - 1) * (t.size(2) > 1 ? t.stride(2) : 1) * 4 + 4 <= ((1ll << 31) - 1);
}
// their element strides {batch | page, head, row}, a size-1 dimension with a harmless one
inline void row_scale_strides(const Tensor& t, long long* v) {
  v[0] = t.size(0) > 1 ? t.stride(0) : t.size(1) * t.size(2);
  v[1] = t.size(1) > 1 ? t.stride(1) : 0;
  v[2] = t.size(2) > 1 ? t.stride(2) : 1;
}

// an fp32 device vector of the call: (n,) or, where the argument has a per-sequence form, (B, n)
inline void check_vec(const OptTensor& t, const char* what, bool per_sequence, int64_t B, int64_t n, const c10::Device& dev) {
  if (!t.has_value()) return;
  const std::string w(what);
  FA_ASSERT(t->scalar_type() == at::kFloat, w + " must be float32");
  FA_ASSERT((t->dim() == 1 && t->size(0) == n) || (per_sequence && t->dim() == 2 && t->size(0) == B && t->size(1) == n),
            w + " has the wrong shape");
  check_vec_placement(*t, w, dev);
}
// the sinks of a quantised cache's call
inline void check_sinks(const OptTensor& sinks, int64_t Hq, const c10::Device& dev) {
  if (!sinks.has_value()) return;
  FA_ASSERT(sinks->scalar_type() == at::kFloat && sinks->dim() == 1 && sinks->size(0) == Hq, "sinks must be float32 of shape (H,)");
  check_vec_placement(*sinks, "sinks", dev);
}
inline const float* fptr(const Tensor& t) { return t.defined() ? (const float*)t.data_ptr() : nullptr; }
inline const float* fptr(const OptTensor& t) { return t.has_value() ? (const float*)t->data_ptr() : nullptr; }

// k_descale / v_descale as the kernels take them: one batch stride serves both, so a (H_kv,) vector beside a (B, H_kv) one is
// expanded
struct Descales {
  Tensor k, v;
  long long bstride = 0;
};
inline Descales expand_descales(const OptTensor& kd, const OptTensor& vd, int64_t B, int64_t Hk) {
  Descales d;
  if (kd.has_value()) d.k = *kd;
  if (vd.has_value()) d.v = *vd;
  if ((d.k.defined() && d.k.dim() == 2) || (d.v.defined() && d.v.dim() == 2)) {
    d.bstride = Hk;
    if (d.k.defined() && d.k.dim() == 1) d.k = d.k.expand({B, Hk}).contiguous();
    if (d.v.defined() && d.v.dim() == 1) d.v = d.v.expand({B, Hk}).contiguous();
  }
  return d;
}

inline void check_seqlens(const Tensor& seqlens, int64_t B, bool packed) {
  FA_ASSERT(seqlens.scalar_type() == at::kInt && seqlens.dim() == 1 && seqlens.numel() == B && seqlens.is_contiguous(),
            packed ? "cache_seqlens must be a contiguous int32 vector of B entries (cu_seqlens_q has B + 1)"
                   : "cache_seqlens must be a contiguous int32 vector of B entries");
}

// ---- the checks the quantised caches share.  g (torch_binding_common.h Queries): cu == nullptr is q [B, H, S_q, D], otherwise
// packed q [total_q, H, D] over paged pools; table: the block table of a paged cache, None for a padded one ----
struct Dims {
  int64_t B, Tq, Hq, Hk;   // sequences, packed rows (0: not packed), heads of q and of the caches
};
// in front of the format's checks
inline void check_packed_front(const Queries& g, const Tensor& Q, const OptTensor& table) {
  FA_ASSERT(!g.cu || table.has_value(), "packed queries go over paged pools: block_table is required");
  if (g.cu) FA_ASSERT(Q.size(0) >= 1, "q must have at least one row");
}
// behind them
inline void check_heads_new_window(const Tensor& Q, const Tensor& Kc, const OptTensor& k_new, const OptTensor& v_new,
                                   int64_t window_left, int64_t window_right) {
  FA_ASSERT(Kc.size(1) >= 1 && Q.size(1) % Kc.size(1) == 0, "q's head count must be a multiple of the caches' (H % H_kv == 0)");
  FA_ASSERT(k_new.has_value() == v_new.has_value(), "k_new and v_new must be given together");
  FA_ASSERT(window_left >= -1 && window_right >= -1 && window_left <= INT32_MAX && window_right <= INT32_MAX,
            "window_left / window_right must be >= -1 (-1 = unbounded) and fit in int32");
}
// Then: where the tensors live, q's dtype, cu_seqlens_q, cache_seqlens, the geometry of the paged or padded cache, no grad.
// Ks / Vs: the format's scale tensors (nullptr: it has none); base: the padded call's Python name; cache_grad: whether a cache
// that requires grad is refused here too.
inline Dims check_placement_and_geometry(const Queries& g, const Tensor& Q, const Tensor& Kc, const Tensor& Vc, const Tensor* Ks,
                                         const Tensor* Vs, const Tensor& seqlens, const OptTensor& table, const char* base,
                                         bool cache_grad) {
  const bool packed = g.cu != nullptr, paged = table.has_value();
  FA_ASSERT(Q.is_cuda() && Kc.is_cuda() && Vc.is_cuda() && (!Ks || (Ks->is_cuda() && Vs->is_cuda())) && seqlens.is_cuda() &&
                (!paged || table->is_cuda()) && (!packed || g.cu->is_cuda()),
            packed ? "q, the caches, the scales, cu_seqlens_q, cache_seqlens and block_table must be device tensors"
                   : "q, the caches, the scales, cache_seqlens and block_table must be device tensors");
  FA_ASSERT(Kc.device() == Q.device() && Vc.device() == Q.device() && (!Ks || (Ks->device() == Q.device() && Vs->device() == Q.device())) &&
                seqlens.device() == Q.device() && (!paged || table->device() == Q.device()) &&
                (!packed || g.cu->device() == Q.device()),
            "all tensors must be on q's device");
  FA_ASSERT(Q.scalar_type() == at::kHalf || Q.scalar_type() == at::kBFloat16, "q's dtype must be float16 or bfloat16");
  if (packed) check_cu_seqlens(*g.cu);
  const Dims d{packed ? g.cu->numel() - 1 : Q.size(0), packed ? Q.size(0) : 0, Q.size(1), Kc.size(1)};
  check_seqlens(seqlens, d.B, packed);
  if (paged) {
    FA_ASSERT(Kc.size(2) >= 32 && Kc.size(2) % 32 == 0, "the page size (k_cache.shape[2]) must be a positive multiple of 32");
    check_block_table(*table, d.B);
    FA_ASSERT(Kc.size(0) <= INT32_MAX && table->size(1) <= INT32_MAX && d.Tq <= INT32_MAX && d.B <= INT32_MAX,
              "too many pages, rows or sequences");
  } else {
    FA_ASSERT(Kc.size(0) == d.B, "the caches must have q's batch size");
    FA_ASSERT(Kc.size(2) <= INT32_MAX, "S_cache too large");
  }
  FA_ASSERT(!Q.requires_grad() && (!cache_grad || (!Kc.requires_grad() && !Vc.requires_grad())),
            std::string(base) + (packed ? "_ragged" : paged ? "_paged" : "") +
                (cache_grad ? " has no backward: q, k_cache and v_cache must not require grad" : " has no backward: q must not require grad"));
  return d;
}

// ---- the tail of a call -------------------------------------------------------------------------------------------------------
inline void* current_stream(const Tensor& Q) {
  return (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(Q.device().index()).stream();
}
inline int dtype_of(const Tensor& Q) { return Q.scalar_type() == at::kBFloat16 ? MI355FA_BF16 : MI355FA_FP16; }
inline long long table_stride_of(const Tensor& table, int64_t B) {
  return B > 1 ? (long long)table.stride(0) : (long long)(int)table.size(1);
}
// the workspace of the call to `fn`: `bytes` is what the library's <fn>_workspace_bytes returned (negative: its refusal)
inline Tensor workspace(long long bytes, const char* fn, const Tensor& Q) {
  check_rc(bytes, (std::string(fn) + "_workspace_bytes").c_str());
  return torch::empty({std::max<long long>(bytes, 1)}, Q.options().dtype(at::kByte));
}

// What a launch takes, prepared.  opts points into the stride arrays: a DecodeCall stays where it was made.
struct DecodeCall {
  Tensor Qp, Kn, Vn, O, LSE;   // q as the kernels read it, k_new / v_new likewise (undefined: no append), the results
  int B = 0, Tq = 0, H = 0, Hkv = 0, D = 0, Sq = 0, S_new = 0, rows = 0, num_pages = 0, max_pages = 0, dtype = 0;
  long long table_stride = 0, qs[3], os[3], ks[3], vs[3];
  float scale = 0.f;
  mi355fa_opts opts{};
  void* stream = nullptr;
  const void *q = nullptr, *kn = nullptr, *vn = nullptr;           // Qp's, Kn's and Vn's data (nullptr: no append)
  const int *cu = nullptr, *seqlens = nullptr, *table = nullptr;   // nullptr: not packed, not paged
  void* o = nullptr;
  float* lse = nullptr;
  c10::OptionalDeviceGuard guard;
  DecodeCall() = default;
  DecodeCall(const DecodeCall&) = delete;
};

// k_new / v_new checked and made contiguous, q in place through its strides when the kernels can, a contiguous copy otherwise,
// the integer geometry and the scale (softmax_scale <= 0: 1/sqrt(D))
inline void prepare_inputs(DecodeCall& c, const Queries& g, const Tensor& Q, const Tensor& Kc, const OptTensor& k_new,
                           const OptTensor& v_new, const Dims& d, double softmax_scale) {
  const bool packed = g.cu != nullptr;
  const int64_t Dq = Q.size(packed ? 2 : 3);
  if (k_new.has_value()) {
    if (packed)
      check_new_shape_packed(*k_new, *v_new, d.Tq, d.Hk, Dq);
    else
      check_new_shape(*k_new, *v_new, d.B, d.Hk, Dq);
    check_new_placement(*k_new, *v_new, Q);
    c.Kn = contiguous16(*k_new);
    c.Vn = contiguous16(*v_new);
    if (!packed) c.S_new = (int)k_new->size(2);
  }
  c.Qp = (packed ? packed_ok(Q, false) : dense_ok(Q)) ? Q : Q.clone(at::MemoryFormat::Contiguous);
  c.B = (int)d.B, c.Tq = (int)d.Tq, c.H = (int)d.Hq, c.Hkv = (int)d.Hk, c.D = (int)Dq;
  c.Sq = packed ? 0 : (int)Q.size(2), c.rows = (int)Kc.size(2);
  c.scale = softmax_scale > 0.0 ? (float)softmax_scale : (float)(1.0 / std::sqrt((double)c.D));
}
// O (a packed call's `out`, written in place, if it gives one) and LSE from the caching allocator on q's device, the table's
// geometry (table == nullptr: a padded cache), the stride arrays and opts, the current stream, q's dtype, the pointers
inline void prepare_launch(DecodeCall& c, const Queries& g, const Tensor& Q, const Tensor& Kc, const Tensor& Vc,
                           const Tensor& seqlens, const Tensor* table) {
  const bool packed = g.cu != nullptr;
  c.guard.reset_device(Q.device());
  c.O = packed ? packed_result(*g.out, Q) : torch::empty(Q.sizes(), Q.options().memory_format(at::MemoryFormat::Contiguous));
  c.LSE = packed ? torch::empty({Q.size(1), Q.size(0)}, Q.options().dtype(at::kFloat))
                 : torch::empty({Q.size(0), Q.size(1), Q.size(2)}, Q.options().dtype(at::kFloat));
  if (table) {
    c.num_pages = (int)Kc.size(0), c.max_pages = (int)table->size(1);
    c.table_stride = table_stride_of(*table, packed ? g.cu->numel() - 1 : Q.size(0));
    c.table = (const int*)table->data_ptr();
  }
  strides3(Kc, c.ks);
  strides3(Vc, c.vs);
  c.opts.size = sizeof(c.opts);
  c.opts.k_strides = c.ks;
  c.opts.v_strides = c.vs;
  if (packed) {
    packed_strides(c.Qp, c.qs);
    packed_strides(c.O, c.os);
    c.opts.q_strides = c.qs;
    c.opts.o_strides = c.os;
    c.cu = (const int*)g.cu->data_ptr();
  } else {
    strides3(c.Qp, c.qs);
    c.opts.q_strides = c.Qp.is_contiguous() ? nullptr : c.qs;
  }
  c.stream = current_stream(Q);
  c.q = c.Qp.data_ptr(), c.kn = c.Kn.defined() ? c.Kn.data_ptr() : nullptr, c.vn = c.Vn.defined() ? c.Vn.data_ptr() : nullptr;
  c.seqlens = (const int*)seqlens.data_ptr(), c.o = c.O.data_ptr(), c.lse = (float*)c.LSE.data_ptr();
  c.dtype = dtype_of(Q);
}

}  // namespace
