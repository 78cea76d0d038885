// Host-side binding of fa_fwd_kvcache_quant_softcap, _paged and _ragged (include_quant/mi355fa_kvcache_quant_softcap.h) for
// PyTorch-ROCm: soft-capped decoding attention over a per-tensor e4m3, a per-token-scaled e4m3 or an MXFP4 KV cache -- padded,
// paged, and with packed variable-length queries over paged pools -- for quant_softcap_kvcache.py.  One module,
// _mi355fa_quant_softcap_torch.so, beside the others, whose sets of functions are recorded surfaces.  It does what
// torch_binding_fp4.cpp and torch_binding_fp8_token.cpp do: O, LSE and the workspace come from the caching allocator, q, the caches
// and the scale tensors are addressed in place through their strides -- caches and scales are written in place, with k_new /
// v_new --, the launch goes to the current stream, and nothing here synchronises or reads cache_seqlens, block_table,
// cu_seqlens_q, the descales or the scales, so a step can be captured in a graph.  Inference only: no autograd.
//
// Built by csrc/Makefile with g++ (host code only).
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <c10/core/DeviceGuard.h>
#include <torch/extension.h>

#include <cmath>
#include <string>
#include <tuple>

#include "../../include_quant/mi355fa_kvcache_quant_softcap.h"
#include "torch_binding_common.h"

namespace {

// Can the kernels address the byte tensor [slices, H_kv, rows, rowb] in place?  A base aligned to `gran` bytes, unit stride
// along the row, strides that are multiples of `gran` and one (slice, head) slice inside 2^31 bytes.  Caches and scales are
// never copied -- the append writes them --, so anything else is refused.
bool bytes_ok(const Tensor& t, int64_t gran) {
  if (reinterpret_cast<uintptr_t>(t.data_ptr()) % gran || t.stride(3) != 1 || (t.size(2) > 1 && t.stride(2) < t.size(3))) return false;
  if ((t.size(2) - 1) * t.stride(2) + t.size(3) > ((1ll << 31) - 1)) return false;
  for (int i = 0; i < 3; ++i)
    if (t.size(i) != 1 && (t.stride(i) < 0 || t.stride(i) % gran != 0)) return false;
  return true;
}
// the fp32 row scales [slices, H_kv, rows]: any non-negative element strides, one (slice, head) slice inside 2^31 bytes
bool row_scales_ok(const Tensor& t) {
  for (int i = 0; i < 3; ++i)
    if (t.size(i) != 1 && t.stride(i) < 0) return false;
  return (t.size(2) - 1) * (t.size(2) > 1 ? t.stride(2) : 1) * 4 + 4 <= ((1ll << 31) - 1);
}
void row_scale_strides(const Tensor& t, long long* v) {
  v[0] = t.size(0) > 1 ? t.stride(0) : t.size(1) * t.size(2);
  v[1] = t.size(1) > 1 ? t.stride(1) : 0;
  v[2] = t.size(2) > 1 ? t.stride(2) : 1;
}
// an fp32 descale of the call: (H_kv,) or (B, H_kv)
void check_descale(const c10::optional<Tensor>& t, const char* what, int64_t B, int64_t n, const c10::Device& dev) {
  if (!t.has_value()) return;
  const std::string w(what);
  FA_ASSERT(t->scalar_type() == at::kFloat, w + " must be float32");
  FA_ASSERT((t->dim() == 1 && t->size(0) == n) || (t->dim() == 2 && t->size(0) == B && t->size(1) == n), w + " has the wrong shape");
  check_vec_placement(*t, w, dev);
}

// format: the header's MI355FA_QUANT_* (the Python wrapper derives it from the tensors).  Kc / Vc: float8_e4m3fn [.., H_kv, rows, D]
// (E4M3, E4M3_TOKEN) or uint8 [.., H_kv, rows, D / 2] (MXFP4); Ks / Vs: float32 [.., H_kv, rows] (E4M3_TOKEN), uint8
// [.., H_kv, rows, D / 32] (MXFP4) or None (E4M3); Kd / Vd: float32 (H_kv,) or (B, H_kv), E4M3 only; table: int32 [B, max_pages] for a
// paged cache, None for a padded one.  softmax_scale <= 0: 1/sqrt(D).  g (torch_binding_common.h Queries): cu == nullptr is q
// [B, H, S_q, D], otherwise packed q [total_q, H, D] over paged pools.
std::tuple<Tensor, Tensor> quant_impl(const Queries& g, const Tensor& Q, const Tensor& Kc, const Tensor& Vc, const Tensor& seqlens,
                                      const c10::optional<Tensor>& table, double softcap, int64_t format,
                                      const c10::optional<Tensor>& Ks, const c10::optional<Tensor>& Vs,
                                      const c10::optional<Tensor>& Kd, const c10::optional<Tensor>& Vd,
                                      const c10::optional<Tensor>& k_new, const c10::optional<Tensor>& v_new, int64_t window_left,
                                      int64_t window_right, double softmax_scale) {
  const bool packed = g.cu != nullptr, paged = table.has_value();
  const bool e4m3 = format == MI355FA_QUANT_E4M3, token = format == MI355FA_QUANT_E4M3_TOKEN, fp4 = format == MI355FA_QUANT_MXFP4;
  const char* name = packed  ? "flash_attention_kvcache_quant_softcap_ragged"
                     : paged ? "flash_attention_kvcache_quant_softcap_paged"
                             : "flash_attention_kvcache_quant_softcap";
  FA_ASSERT(e4m3 || token || fp4, "format must be 0 (per-tensor e4m3), 1 (per-token e4m3) or 2 (MXFP4)");
  const int qdim = packed ? 3 : 4;
  FA_ASSERT(Q.dim() == qdim && Kc.dim() == 4 && Vc.dim() == 4,
            packed ? "q must be [total_q, H, D] and the pools 4-d [num_pages, H_kv, page_size, row]"
                   : "q must be [B, H, S_q, D] and the caches 4-d [.., H_kv, rows, row]");
  FA_ASSERT(!packed || paged, "packed queries go over paged pools: block_table is required");
  if (packed) FA_ASSERT(Q.size(0) >= 1, "q must have at least one row");
  FA_ASSERT(Ks.has_value() == Vs.has_value() && Ks.has_value() == !e4m3,
            "k_scale and v_scale come with a per-token e4m3 or an MXFP4 cache, and with no other");
  FA_ASSERT(e4m3 || (!Kd.has_value() && !Vd.has_value()), "k_descale / v_descale belong to a per-tensor e4m3 cache");
  const int64_t Dq = Q.size(qdim - 1);
  if (fp4) {
    for (const Tensor* t : {&Kc, &Vc, &*Ks, &*Vs})
      FA_ASSERT(t->scalar_type() == at::kByte, "the MXFP4 caches and their scales are passed as bytes");
    FA_ASSERT(Ks->dim() == 4 && Vs->dim() == 4, "the MXFP4 scales must be [.., H_kv, rows, D / 32]");
  } else {
    FA_ASSERT(Kc.scalar_type() == at::kFloat8_e4m3fn && Vc.scalar_type() == at::kFloat8_e4m3fn,
              "k_cache and v_cache must be torch.float8_e4m3fn");
    if (token)
      FA_ASSERT(Ks->scalar_type() == at::kFloat && Vs->scalar_type() == at::kFloat && Ks->dim() == 3 && Vs->dim() == 3,
                "k_scale and v_scale must be float32 [.., H_kv, rows]");
  }
  if (e4m3)
    FA_ASSERT(Dq == 64 || Dq == 128 || Dq == 256, "a per-tensor e4m3 cache takes head dim 64, 128 or 256");
  else if (packed)
    FA_ASSERT(Dq == 64 || Dq == 128 || Dq == 256, "packed queries over a per-token e4m3 or an MXFP4 cache take head dim 64, 128 or 256");
  else
    FA_ASSERT(Dq == 64 || Dq == 128, "a per-token e4m3 or an MXFP4 cache takes head dim 64 or 128 (256 with packed queries)");
  FA_ASSERT(Kc.sizes() == Vc.sizes() && Kc.size(3) == (fp4 ? Dq / 2 : Dq),
            "k_cache and v_cache must have the same shape, rows of D bytes (MXFP4: D / 2)");
  if (!e4m3) {
    FA_ASSERT(Ks->sizes() == Vs->sizes() && Ks->size(0) == Kc.size(0) && Ks->size(1) == Kc.size(1) && Ks->size(2) == Kc.size(2) &&
                  (!fp4 || Ks->size(3) == Dq / 32),
              "k_scale and v_scale must have the caches' leading dimensions (MXFP4: and rows of D / 32 bytes)");
  }
  FA_ASSERT(Kc.size(1) >= 1 && Q.size(1) % Kc.size(1) == 0, "q's head count must be a multiple of the caches' (H % H_kv == 0)");
  FA_ASSERT(k_new.has_value() == v_new.has_value(), "k_new and v_new must be given together");
  FA_ASSERT(window_left >= -1 && window_right >= -1 && window_left <= INT32_MAX && window_right <= INT32_MAX,
            "window_left / window_right must be >= -1 (-1 = unbounded) and fit in int32");
  FA_ASSERT(std::isfinite(softcap) && softcap > 0.0, "softcap must be finite and > 0");
  FA_ASSERT(Q.is_cuda() && Kc.is_cuda() && Vc.is_cuda() && (e4m3 || (Ks->is_cuda() && Vs->is_cuda())) && seqlens.is_cuda() &&
                (!paged || table->is_cuda()) && (!packed || g.cu->is_cuda()),
            packed ? "q, the caches, the scales, cu_seqlens_q, cache_seqlens and block_table must be device tensors"
                   : "q, the caches, the scales, cache_seqlens and block_table must be device tensors");
  FA_ASSERT(Kc.device() == Q.device() && Vc.device() == Q.device() &&
                (e4m3 || (Ks->device() == Q.device() && Vs->device() == Q.device())) && seqlens.device() == Q.device() &&
                (!paged || table->device() == Q.device()) && (!packed || g.cu->device() == Q.device()),
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
  FA_ASSERT(!Q.requires_grad() && !Kc.requires_grad() && !Vc.requires_grad(),
            std::string(name) + " has no backward: q, k_cache and v_cache must not require grad");
  check_descale(Kd, "k_descale", B, Hk, Q.device());
  check_descale(Vd, "v_descale", B, Hk, Q.device());
  FA_ASSERT(bytes_ok(Kc, 16) && bytes_ok(Vc, 16) && (Kc.size(2) == 1 || Kc.stride(2) == Vc.stride(2)),
            "the caches must be addressable in place: 16-byte aligned rows with unit stride along the row, strides that are "
            "multiples of 16 bytes, one row stride for K and V");
  if (fp4)
    FA_ASSERT(bytes_ok(*Ks, Dq / 32) && bytes_ok(*Vs, Dq / 32),
              "the scales must be addressable in place: rows of D / 32 bytes with unit stride, aligned to D / 32 bytes, strides "
              "that are multiples of D / 32 bytes");
  if (token)
    FA_ASSERT(row_scales_ok(*Ks) && row_scales_ok(*Vs) && !Ks->requires_grad() && !Vs->requires_grad(),
              "the scales must be addressable in place: non-negative strides, one (batch, head) slice below 2^31 bytes, no grad");
  // one batch stride serves both descale vectors: a (H_kv,) vector beside a (B, H_kv) one is expanded
  Tensor Kdt, Vdt;
  long long dstride = 0;
  if (Kd.has_value()) Kdt = *Kd;
  if (Vd.has_value()) Vdt = *Vd;
  if ((Kdt.defined() && Kdt.dim() == 2) || (Vdt.defined() && Vdt.dim() == 2)) {
    dstride = Hk;
    if (Kdt.defined() && Kdt.dim() == 1) Kdt = Kdt.expand({B, Hk}).contiguous();
    if (Vdt.defined() && Vdt.dim() == 1) Vdt = Vdt.expand({B, Hk}).contiguous();
  }
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
  const int H = (int)Hq, Hkv = (int)Hk, D = (int)Dq, Sq = packed ? 0 : (int)Q.size(2), rows = (int)Kc.size(2), fmt = (int)format;
  const float scale = softmax_scale > 0.0 ? (float)softmax_scale : (float)(1.0 / std::sqrt((double)D));
  c10::OptionalDeviceGuard guard(Q.device());
  Tensor O = packed ? packed_result(*g.out, Q) : torch::empty(Q.sizes(), Q.options().memory_format(at::MemoryFormat::Contiguous));
  Tensor LSE = packed ? torch::empty({Hq, Tq}, Q.options().dtype(at::kFloat))
                      : torch::empty({B, Hq, Q.size(2)}, Q.options().dtype(at::kFloat));
  const int num_pages = paged ? (int)Kc.size(0) : 0, max_pages = paged ? (int)table->size(1) : 0;
  const char* ws_fn = packed  ? "fa_fwd_kvcache_quant_softcap_ragged_workspace_bytes"
                      : paged ? "fa_fwd_kvcache_quant_softcap_paged_workspace_bytes"
                              : "fa_fwd_kvcache_quant_softcap_workspace_bytes";
  const long long ws_bytes =
      packed  ? fa_fwd_kvcache_quant_softcap_ragged_workspace_bytes(fmt, (int)Tq, (int)B, H, Hkv, max_pages, rows, D)
      : paged ? fa_fwd_kvcache_quant_softcap_paged_workspace_bytes(fmt, (int)B, H, Hkv, Sq, max_pages, rows, S_new, D)
              : fa_fwd_kvcache_quant_softcap_workspace_bytes(fmt, (int)B, H, Hkv, Sq, rows, S_new, D);
  check_rc(ws_bytes, ws_fn);
  Tensor ws = torch::empty({std::max<long long>(ws_bytes, 1)}, Q.options().dtype(at::kByte));
  long long qs[3], os[3], ks[3], vs[3], kss[3], vss[3];
  strides3(Kc, ks);
  strides3(Vc, vs);
  mi355fa_quant_cache cache{};
  cache.format = fmt;
  if (e4m3) {
    cache.k_descale = Kdt.defined() ? (const float*)Kdt.data_ptr() : nullptr;
    cache.v_descale = Vdt.defined() ? (const float*)Vdt.data_ptr() : nullptr;
    cache.descale_bstride = dstride;
  } else {
    if (fp4) {
      strides3(*Ks, kss);
      strides3(*Vs, vss);
    } else {
      row_scale_strides(*Ks, kss);
      row_scale_strides(*Vs, vss);
    }
    cache.k_scale = Ks->data_ptr();
    cache.v_scale = Vs->data_ptr();
    cache.k_scale_strides = kss;
    cache.v_scale_strides = vss;
  }
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
  const int dtype = Q.scalar_type() == at::kBFloat16 ? MI355FA_BF16 : MI355FA_FP16;
  const long long table_stride = paged ? (B > 1 ? (long long)table->stride(0) : (long long)max_pages) : 0;
  if (packed) {
    check_rc(fa_fwd_kvcache_quant_softcap_ragged(Qp.data_ptr(), Kc.data_ptr(), Vc.data_ptr(), kn, vn, (const int*)g.cu->data_ptr(),
                                                 (const int*)seqlens.data_ptr(), (const int*)table->data_ptr(), O.data_ptr(),
                                                 (float*)LSE.data_ptr(), ws.data_ptr(), ws_bytes, (int)Tq, (int)B, H, Hkv,
                                                 num_pages, rows, max_pages, table_stride, D, dtype, scale, (float)softcap,
                                                 (int)window_left, (int)window_right, &cache, &opts, stream),
             "fa_fwd_kvcache_quant_softcap_ragged");
  } else if (paged) {
    check_rc(fa_fwd_kvcache_quant_softcap_paged(Qp.data_ptr(), Kc.data_ptr(), Vc.data_ptr(), kn, vn, (const int*)seqlens.data_ptr(),
                                                (const int*)table->data_ptr(), O.data_ptr(), (float*)LSE.data_ptr(), ws.data_ptr(),
                                                ws_bytes, (int)B, H, Hkv, Sq, num_pages, rows, max_pages, table_stride, S_new, D,
                                                dtype, scale, (float)softcap, (int)window_left, (int)window_right, &cache, &opts,
                                                stream),
             "fa_fwd_kvcache_quant_softcap_paged");
  } else {
    check_rc(fa_fwd_kvcache_quant_softcap(Qp.data_ptr(), Kc.data_ptr(), Vc.data_ptr(), kn, vn, (const int*)seqlens.data_ptr(),
                                          O.data_ptr(), (float*)LSE.data_ptr(), ws.data_ptr(), ws_bytes, (int)B, H, Hkv, Sq, rows,
                                          S_new, D, dtype, scale, (float)softcap, (int)window_left, (int)window_right, &cache, &opts,
                                          stream),
             "fa_fwd_kvcache_quant_softcap");
  }
  return {O, LSE};
}

std::tuple<Tensor, Tensor> kvcache_quant_softcap_forward(const Tensor& Q, const Tensor& Kc, const Tensor& Vc, const Tensor& seqlens,
                                                         const c10::optional<Tensor>& table, double softcap, int64_t format,
                                                         const c10::optional<Tensor>& Ks, const c10::optional<Tensor>& Vs,
                                                         const c10::optional<Tensor>& Kd, const c10::optional<Tensor>& Vd,
                                                         const c10::optional<Tensor>& k_new, const c10::optional<Tensor>& v_new,
                                                         int64_t window_left, int64_t window_right, double softmax_scale) {
  return quant_impl(Queries{}, Q, Kc, Vc, seqlens, table, softcap, format, Ks, Vs, Kd, Vd, k_new, v_new, window_left, window_right,
                    softmax_scale);
}

std::tuple<Tensor, Tensor> kvcache_quant_softcap_ragged_forward(const Tensor& Q, const Tensor& Kc, const Tensor& Vc, const Tensor& cu,
                                                                const Tensor& seqlens, const Tensor& table, double softcap,
                                                                int64_t format, const c10::optional<Tensor>& Ks,
                                                                const c10::optional<Tensor>& Vs, const c10::optional<Tensor>& Kd,
                                                                const c10::optional<Tensor>& Vd, const c10::optional<Tensor>& k_new,
                                                                const c10::optional<Tensor>& v_new, int64_t window_left,
                                                                int64_t window_right, double softmax_scale,
                                                                const c10::optional<Tensor>& out) {
  return quant_impl(Queries{&cu, &out}, Q, Kc, Vc, seqlens, c10::optional<Tensor>(table), softcap, format, Ks, Vs, Kd, Vd, k_new,
                    v_new, window_left, window_right, softmax_scale);
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "PyTorch-ROCm binding of fa_fwd_kvcache_quant_softcap, _paged and _ragged (libmi355fa.so): soft-capped decoding "
            "attention over per-tensor e4m3, per-token e4m3 and MXFP4 KV caches";
  m.def("kvcache_quant_softcap_forward", &kvcache_quant_softcap_forward, pybind11::arg("q"), pybind11::arg("k_cache"),
        pybind11::arg("v_cache"), pybind11::arg("cache_seqlens"), pybind11::arg("block_table"), pybind11::arg("softcap"),
        pybind11::arg("format"), pybind11::arg("k_scale"), pybind11::arg("v_scale"), pybind11::arg("k_descale"),
        pybind11::arg("v_descale"), pybind11::arg("k_new"), pybind11::arg("v_new"), pybind11::arg("window_left"),
        pybind11::arg("window_right"), pybind11::arg("softmax_scale"),
        "O, LSE = soft-capped attention of q over the quantised cache (block_table: its pages), after appending k_new / v_new "
        "(None: no append)");
  m.def("kvcache_quant_softcap_ragged_forward", &kvcache_quant_softcap_ragged_forward, pybind11::arg("q"), pybind11::arg("k_cache"),
        pybind11::arg("v_cache"), pybind11::arg("cu_seqlens_q"), pybind11::arg("cache_seqlens"), pybind11::arg("block_table"),
        pybind11::arg("softcap"), pybind11::arg("format"), pybind11::arg("k_scale"), pybind11::arg("v_scale"),
        pybind11::arg("k_descale"), pybind11::arg("v_descale"), pybind11::arg("k_new"), pybind11::arg("v_new"),
        pybind11::arg("window_left"), pybind11::arg("window_right"), pybind11::arg("softmax_scale"), pybind11::arg("out"),
        "O, LSE = soft-capped attention of the packed q over the quantised pages block_table names, after appending k_new / v_new "
        "(None: no append)");
}
