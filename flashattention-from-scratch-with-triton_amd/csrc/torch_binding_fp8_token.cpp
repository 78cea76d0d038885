// Host-side binding of fa_fwd_kvcache_fp8_token, fa_fwd_kvcache_fp8_token_paged and fa_fwd_kvcache_fp8_token_ragged
// (include/mi355fa_kvcache_fp8_token.h) for PyTorch-ROCm: decoding attention over an e4m3 KV cache with one fp32 scale per cached
// token and K/V head -- padded, paged, and with packed variable-length queries over paged pools -- for fp8_token_kvcache.py.  One
// module, _mi355fa_fp8_token_torch.so, beside _mi355fa_torch.so, _mi355fa_paged_torch.so and _mi355fa_fp4_torch.so, whose sets of
// functions are recorded surfaces.  It does what torch_binding_fp4.cpp does: O, LSE and the workspace come from the caching
// allocator, q, the caches and the scale tensors are addressed in place through their strides -- caches and scales are written in
// place, with k_new / v_new --, the launch goes to the current stream, and nothing here synchronises or reads cache_seqlens,
// block_table, cu_seqlens_q or the scales, so a step can be captured in a graph.  Inference only: no autograd.
//
// Built by csrc/Makefile with g++ (host code only).
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <c10/core/DeviceGuard.h>
#include <torch/extension.h>

#include <cmath>
#include <string>
#include <tuple>

#include "../../include/mi355fa_kvcache_fp8_token.h"
#include "torch_binding_common.h"

namespace {

// Can the kernels address the e4m3 cache [slices, H_kv, rows, D] in place?  A 16-byte aligned base, unit stride along the row,
// strides that are multiples of 16 bytes and one (slice, head) slice inside 2^31 bytes.  Caches are never copied -- the append
// writes them --, so anything else is refused.
bool cache_ok(const Tensor& t) {
  if (reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 || t.stride(3) != 1 || (t.size(2) > 1 && t.stride(2) < t.size(3))) return false;
  if ((t.size(2) - 1) * t.stride(2) + t.size(3) > ((1ll << 31) - 1)) return false;
  for (int i = 0; i < 3; ++i)
    if (t.size(i) != 1 && (t.stride(i) < 0 || t.stride(i) % 16 != 0)) return false;
  return true;
}
// and the fp32 scales [slices, H_kv, rows]: any non-negative element strides, one (slice, head) slice inside 2^31 bytes
bool scales_ok(const Tensor& t) {
  for (int i = 0; i < 3; ++i)
    if (t.size(i) != 1 && t.stride(i) < 0) return false;
  return (t.size(2) - 1) * (t.size(2) > 1 ? t.stride(2) : 1) * 4 + 4 <= ((1ll << 31) - 1);
}
// element strides {batch | page, head, row} of a 3-d scale tensor, a size-1 dimension with a harmless one
void scale_strides(const Tensor& t, long long* v) {
  v[0] = t.size(0) > 1 ? t.stride(0) : t.size(1) * t.size(2);
  v[1] = t.size(1) > 1 ? t.stride(1) : 0;
  v[2] = t.size(2) > 1 ? t.stride(2) : 1;
}

// Kc / Vc: float8_e4m3fn [B | num_pages, H_kv, S_cache | page_size, D]; Ks / Vs: float32 [.., H_kv, rows]; table: int32
// [B, max_pages] for a paged cache, None for a padded one.  softmax_scale <= 0: 1/sqrt(D).  g (torch_binding_common.h Queries):
// cu == nullptr is q [B, H, S_q, D] and fa_fwd_kvcache_fp8_token / _paged, otherwise packed q [total_q, H, D] over paged pools and
// fa_fwd_kvcache_fp8_token_ragged, the one form with D = 256.
std::tuple<Tensor, Tensor> token_impl(const Queries& g, const Tensor& Q, const Tensor& Kc, const Tensor& Vc, const Tensor& Ks,
                                      const Tensor& Vs, const Tensor& seqlens, const c10::optional<Tensor>& table,
                                      const c10::optional<Tensor>& k_new, const c10::optional<Tensor>& v_new,
                                      int64_t window_left, int64_t window_right, double softmax_scale,
                                      const c10::optional<Tensor>& sinks) {
  const bool packed = g.cu != nullptr, paged = table.has_value();
  const char* name = packed  ? "flash_attention_kvcache_fp8_token_ragged"
                     : paged ? "flash_attention_kvcache_fp8_token_paged"
                             : "flash_attention_kvcache_fp8_token";
  const int qdim = packed ? 3 : 4;
  FA_ASSERT(Q.dim() == qdim && Kc.dim() == 4 && Vc.dim() == 4 && Ks.dim() == 3 && Vs.dim() == 3,
            packed ? "q must be [total_q, H, D], the pools [num_pages, H_kv, page_size, D] and the scales [num_pages, H_kv, page_size]"
                   : "q must be [B, H, S_q, D], the caches [.., H_kv, rows, D] and the scales [.., H_kv, rows]");
  FA_ASSERT(!packed || paged, "packed queries go over paged pools: block_table is required");
  if (packed) FA_ASSERT(Q.size(0) >= 1, "q must have at least one row");
  FA_ASSERT(Kc.scalar_type() == at::kFloat8_e4m3fn && Vc.scalar_type() == at::kFloat8_e4m3fn,
            "k_cache and v_cache must be torch.float8_e4m3fn");
  FA_ASSERT(Ks.scalar_type() == at::kFloat && Vs.scalar_type() == at::kFloat, "k_scale and v_scale must be float32");
  const int64_t Dq = Q.size(qdim - 1);
  if (packed)
    FA_ASSERT(Dq == 64 || Dq == 128 || Dq == 256, "packed queries over a per-token-scaled cache take head dim 64, 128 or 256");
  else
    FA_ASSERT(Dq == 64 || Dq == 128, "a per-token-scaled cache takes head dim 64 or 128");
  FA_ASSERT(Kc.sizes() == Vc.sizes() && Kc.size(3) == Dq, "k_cache and v_cache must have the same shape, rows of D bytes");
  FA_ASSERT(Ks.sizes() == Vs.sizes() && Ks.size(0) == Kc.size(0) && Ks.size(1) == Kc.size(1) && Ks.size(2) == Kc.size(2),
            "k_scale and v_scale must have the caches' shape without D");
  FA_ASSERT(Kc.size(1) >= 1 && Q.size(1) % Kc.size(1) == 0, "q's head count must be a multiple of the caches' (H % H_kv == 0)");
  FA_ASSERT(k_new.has_value() == v_new.has_value(), "k_new and v_new must be given together");
  FA_ASSERT(window_left >= -1 && window_right >= -1 && window_left <= INT32_MAX && window_right <= INT32_MAX,
            "window_left / window_right must be >= -1 (-1 = unbounded) and fit in int32");
  FA_ASSERT(Q.is_cuda() && Kc.is_cuda() && Vc.is_cuda() && Ks.is_cuda() && Vs.is_cuda() && seqlens.is_cuda() &&
                (!paged || table->is_cuda()) && (!packed || g.cu->is_cuda()),
            packed ? "q, the caches, the scales, cu_seqlens_q, cache_seqlens and block_table must be device tensors"
                   : "q, the caches, the scales, cache_seqlens and block_table must be device tensors");
  FA_ASSERT(Kc.device() == Q.device() && Vc.device() == Q.device() && Ks.device() == Q.device() && Vs.device() == Q.device() &&
                seqlens.device() == Q.device() && (!paged || table->device() == Q.device()) &&
                (!packed || g.cu->device() == Q.device()),
            "all tensors must be on q's device");
  FA_ASSERT(Q.scalar_type() == at::kHalf || Q.scalar_type() == at::kBFloat16, "q's dtype must be float16 or bfloat16");
  if (packed) check_cu_seqlens(*g.cu);
  const int64_t B = packed ? g.cu->numel() - 1 : Q.size(0), Tq = packed ? Q.size(0) : 0, Hq = Q.size(1), Hk = Kc.size(1);
  FA_ASSERT(seqlens.scalar_type() == at::kInt && seqlens.dim() == 1 && seqlens.numel() == B && seqlens.is_contiguous(),
            packed ? "cache_seqlens must be a contiguous int32 vector of B entries (cu_seqlens_q has B + 1)"
                   : "cache_seqlens must be a contiguous int32 vector of B entries");
  if (paged) {
    FA_ASSERT(Kc.size(2) >= 32 && Kc.size(2) % 32 == 0, "the page size (k_cache.shape[2]) must be a positive multiple of 32");
    check_block_table(*table, B);
    FA_ASSERT(Kc.size(0) <= INT32_MAX && table->size(1) <= INT32_MAX && Tq <= INT32_MAX && B <= INT32_MAX,
              "too many pages, rows or sequences");
  } else {
    FA_ASSERT(Kc.size(0) == B, "the caches must have q's batch size");
    FA_ASSERT(Kc.size(2) <= INT32_MAX, "S_cache too large");
  }
  FA_ASSERT(!Q.requires_grad(), std::string(name) + " has no backward: q must not require grad");
  if (sinks.has_value()) {
    FA_ASSERT(sinks->scalar_type() == at::kFloat && sinks->dim() == 1 && sinks->size(0) == Hq, "sinks must be float32 of shape (H,)");
    check_vec_placement(*sinks, "sinks", Q.device());
  }
  FA_ASSERT(cache_ok(Kc) && cache_ok(Vc) && (Kc.size(2) == 1 || Kc.stride(2) == Vc.stride(2)),
            "the caches must be addressable in place: 16-byte aligned rows with unit stride along the row, strides that are "
            "multiples of 16 bytes, one row stride for K and V");
  FA_ASSERT(scales_ok(Ks) && scales_ok(Vs) && !Ks.requires_grad() && !Vs.requires_grad(),
            "the scales must be addressable in place: non-negative strides, one (batch, head) slice below 2^31 bytes, no grad");
  Tensor Kn, Vn;
  int S_new = 0;
  if (k_new.has_value()) {
    if (packed)
      check_new_shape_packed(*k_new, *v_new, Tq, Hk, Dq);
    else
      check_new_shape(*k_new, *v_new, B, Hk, Dq);
    check_new_placement(*k_new, *v_new, Q);
    Kn = contiguous16(*k_new);
    Vn = contiguous16(*v_new);
    if (!packed) S_new = (int)k_new->size(2);
  }
  // q as the kernels read it: in place through its strides when they can, a contiguous copy otherwise
  const Tensor Qp = (packed ? packed_ok(Q, false) : dense_ok(Q)) ? Q : Q.clone(at::MemoryFormat::Contiguous);
  const int H = (int)Hq, Hkv = (int)Hk, D = (int)Dq, Sq = packed ? 0 : (int)Q.size(2), rows = (int)Kc.size(2);
  const float scale = softmax_scale > 0.0 ? (float)softmax_scale : (float)(1.0 / std::sqrt((double)D));
  c10::OptionalDeviceGuard guard(Q.device());
  Tensor O = packed ? packed_result(*g.out, Q) : torch::empty(Q.sizes(), Q.options().memory_format(at::MemoryFormat::Contiguous));
  Tensor LSE = packed ? torch::empty({Hq, Tq}, Q.options().dtype(at::kFloat))
                      : torch::empty({B, Hq, Q.size(2)}, Q.options().dtype(at::kFloat));
  const int num_pages = paged ? (int)Kc.size(0) : 0, max_pages = paged ? (int)table->size(1) : 0;
  const char* ws_fn = packed  ? "fa_fwd_kvcache_fp8_token_ragged_workspace_bytes"
                      : paged ? "fa_fwd_kvcache_fp8_token_paged_workspace_bytes"
                              : "fa_fwd_kvcache_fp8_token_workspace_bytes";
  const long long ws_bytes = packed  ? fa_fwd_kvcache_fp8_token_ragged_workspace_bytes((int)Tq, (int)B, H, Hkv, max_pages, rows, D)
                             : paged ? fa_fwd_kvcache_fp8_token_paged_workspace_bytes((int)B, H, Hkv, Sq, max_pages, rows, S_new, D)
                                     : fa_fwd_kvcache_fp8_token_workspace_bytes((int)B, H, Hkv, Sq, rows, S_new, D);
  check_rc(ws_bytes, ws_fn);
  Tensor ws = torch::empty({std::max<long long>(ws_bytes, 1)}, Q.options().dtype(at::kByte));
  long long qs[3], os[3], ks[3], vs[3], kss[3], vss[3];
  strides3(Kc, ks);
  strides3(Vc, vs);
  scale_strides(Ks, kss);
  scale_strides(Vs, vss);
  mi355fa_opts opts{};
  opts.size = sizeof(opts);
  opts.k_strides = ks;
  opts.v_strides = vs;
  if (packed) {
    packed_strides(Qp, qs);
    packed_strides(O, os);
    opts.q_strides = qs;
    opts.o_strides = os;
  } else {
    strides3(Qp, qs);
    opts.q_strides = Qp.is_contiguous() ? nullptr : qs;
  }
  void* stream = (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(Q.device().index()).stream();
  const void *kn = Kn.defined() ? Kn.data_ptr() : nullptr, *vn = Vn.defined() ? Vn.data_ptr() : nullptr;
  const float* sk = sinks.has_value() ? (const float*)sinks->data_ptr() : nullptr;
  const int dtype = Q.scalar_type() == at::kBFloat16 ? MI355FA_BF16 : MI355FA_FP16;
  const long long table_stride = paged ? (B > 1 ? (long long)table->stride(0) : (long long)max_pages) : 0;
  float *ksp = (float*)Ks.data_ptr(), *vsp = (float*)Vs.data_ptr();
  if (packed) {
    check_rc(fa_fwd_kvcache_fp8_token_ragged(Qp.data_ptr(), Kc.data_ptr(), Vc.data_ptr(), ksp, vsp, kn, vn,
                                             (const int*)g.cu->data_ptr(), (const int*)seqlens.data_ptr(),
                                             (const int*)table->data_ptr(), kss, vss, sk, O.data_ptr(), (float*)LSE.data_ptr(),
                                             ws.data_ptr(), ws_bytes, (int)Tq, (int)B, H, Hkv, num_pages, rows, max_pages,
                                             table_stride, D, dtype, scale, (int)window_left, (int)window_right, &opts, stream),
             "fa_fwd_kvcache_fp8_token_ragged");
  } else if (paged) {
    check_rc(fa_fwd_kvcache_fp8_token_paged(Qp.data_ptr(), Kc.data_ptr(), Vc.data_ptr(), ksp, vsp, kn, vn,
                                            (const int*)seqlens.data_ptr(), (const int*)table->data_ptr(), kss, vss, sk,
                                            O.data_ptr(), (float*)LSE.data_ptr(), ws.data_ptr(), ws_bytes, (int)B, H, Hkv, Sq,
                                            num_pages, rows, max_pages, table_stride, S_new, D, dtype, scale, (int)window_left,
                                            (int)window_right, &opts, stream),
             "fa_fwd_kvcache_fp8_token_paged");
  } else {
    check_rc(fa_fwd_kvcache_fp8_token(Qp.data_ptr(), Kc.data_ptr(), Vc.data_ptr(), ksp, vsp, kn, vn,
                                      (const int*)seqlens.data_ptr(), kss, vss, sk, O.data_ptr(), (float*)LSE.data_ptr(),
                                      ws.data_ptr(), ws_bytes, (int)B, H, Hkv, Sq, rows, S_new, D, dtype, scale, (int)window_left,
                                      (int)window_right, &opts, stream),
             "fa_fwd_kvcache_fp8_token");
  }
  return {O, LSE};
}

std::tuple<Tensor, Tensor> kvcache_fp8_token_forward(const Tensor& Q, const Tensor& Kc, const Tensor& Vc, const Tensor& Ks,
                                                     const Tensor& Vs, const Tensor& seqlens,
                                                     const c10::optional<Tensor>& table, const c10::optional<Tensor>& k_new,
                                                     const c10::optional<Tensor>& v_new, int64_t window_left,
                                                     int64_t window_right, double softmax_scale,
                                                     const c10::optional<Tensor>& sinks) {
  return token_impl(Queries{}, Q, Kc, Vc, Ks, Vs, seqlens, table, k_new, v_new, window_left, window_right, softmax_scale, sinks);
}

std::tuple<Tensor, Tensor> kvcache_fp8_token_ragged_forward(const Tensor& Q, const Tensor& Kc, const Tensor& Vc, const Tensor& Ks,
                                                            const Tensor& Vs, const Tensor& cu, const Tensor& seqlens,
                                                            const Tensor& table, const c10::optional<Tensor>& k_new,
                                                            const c10::optional<Tensor>& v_new, int64_t window_left,
                                                            int64_t window_right, double softmax_scale,
                                                            const c10::optional<Tensor>& sinks,
                                                            const c10::optional<Tensor>& out) {
  return token_impl(Queries{&cu, &out}, Q, Kc, Vc, Ks, Vs, seqlens, c10::optional<Tensor>(table), k_new, v_new, window_left,
                    window_right, softmax_scale, sinks);
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "PyTorch-ROCm binding of fa_fwd_kvcache_fp8_token, _paged and _ragged (libmi355fa.so): decoding attention over an "
            "e4m3 KV cache with one fp32 scale per cached token and K/V head";
  m.def("kvcache_fp8_token_forward", &kvcache_fp8_token_forward, pybind11::arg("q"), pybind11::arg("k_cache"),
        pybind11::arg("v_cache"), pybind11::arg("k_scale"), pybind11::arg("v_scale"), pybind11::arg("cache_seqlens"),
        pybind11::arg("block_table"), pybind11::arg("k_new"), pybind11::arg("v_new"), pybind11::arg("window_left"),
        pybind11::arg("window_right"), pybind11::arg("softmax_scale"), pybind11::arg("sinks"),
        "O, LSE = attention of q over the per-token-scaled e4m3 cache (block_table: its pages), after appending k_new / v_new "
        "(None: no append)");
  m.def("kvcache_fp8_token_ragged_forward", &kvcache_fp8_token_ragged_forward, pybind11::arg("q"), pybind11::arg("k_cache"),
        pybind11::arg("v_cache"), pybind11::arg("k_scale"), pybind11::arg("v_scale"), pybind11::arg("cu_seqlens_q"),
        pybind11::arg("cache_seqlens"), pybind11::arg("block_table"), pybind11::arg("k_new"), pybind11::arg("v_new"),
        pybind11::arg("window_left"), pybind11::arg("window_right"), pybind11::arg("softmax_scale"), pybind11::arg("sinks"),
        pybind11::arg("out"),
        "O, LSE = attention of the packed q over the per-token-scaled e4m3 pages block_table names, after appending k_new / v_new "
        "(None: no append)");
}
