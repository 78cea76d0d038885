// Host-side binding of fa_fwd_kvcache_paged (include/mi355fa_paged.h) and fa_fwd_kvcache_ragged (include/mi355fa_ragged.h)
// for PyTorch-ROCm: decoding attention over a paged KV cache, with q [B, H, S_q, D] for paged_kvcache.py or with packed
// variable-length queries [total_q, H, D] for ragged_kvcache.py.  One module, _mi355fa_paged_torch.so, beside
// _mi355fa_torch.so (torch_binding.cpp), whose set of functions is a recorded surface.  It does what kvcache_forward does
// there: O (unless a packed call gives one), LSE and the workspace come from the caching allocator, q / out and the pools
// are addressed in place through their strides -- the pools are written in place, with k_new / v_new --, the launch goes to
// the current stream, and nothing here synchronises or reads cu_seqlens_q, cache_seqlens or block_table, so a step can be
// captured in a graph.  Inference only: no autograd.
//
// Built by csrc/Makefile with g++ (host code only).
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <c10/core/DeviceGuard.h>
#include <torch/extension.h>

#include <cmath>
#include <string>
#include <tuple>

#include "../../include/mi355fa_ragged.h"
#include "torch_binding_common.h"

namespace {

// Can the kernels address the pool [num_pages, H_kv, page_size, D] in place?  16-byte aligned rows of unit head-dim stride,
// strides that are multiples of 16 bytes (esz: bytes per element) and one (page, head) slice inside 2^31 bytes.  A pool is
// never copied -- the append writes it and a copy of a whole pool is no decode step --, so anything else is refused.
bool pool_ok(const Tensor& t, int64_t esz) {
  if (reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 || t.stride(3) != 1 || t.stride(2) < t.size(3)) return false;
  if ((t.size(2) - 1) * t.stride(2) * esz + t.size(3) * esz > ((1ll << 31) - 1)) return false;
  for (int i = 0; i < 3; ++i)
    if (t.size(i) != 1 && (t.stride(i) < 0 || (t.stride(i) * esz) % 16 != 0)) return false;
  return true;
}

const float* fptr(const c10::optional<Tensor>& t) { return t.has_value() ? (const float*)t->data_ptr() : nullptr; }

// an fp32 device vector of the call: (n,) or, when B > 0, (B, n)
void check_vec(const c10::optional<Tensor>& t, const char* what, int64_t B, int64_t n, const c10::Device& dev) {
  if (!t.has_value()) return;
  const std::string w(what);
  FA_ASSERT(t->scalar_type() == at::kFloat, w + " must be float32");
  FA_ASSERT((t->dim() == 1 && t->size(0) == n) || (B > 0 && t->dim() == 2 && t->size(0) == B && t->size(1) == n),
            w + " has the wrong shape");
  check_vec_placement(*t, w, dev);
}

// The geometry of the queries (torch_binding_common.h Queries): cu == nullptr is fa_fwd_kvcache_paged, otherwise
// fa_fwd_kvcache_ragged.
// softmax_scale <= 0: 1/sqrt(D); softcap <= 0: none.  The Python wrapper has refused the combinations of transforms.
std::tuple<Tensor, Tensor> paged_impl(const Queries& g, const Tensor& Q, const Tensor& Kp, const Tensor& Vp,
                                      const Tensor& seqlens, const Tensor& table, const c10::optional<Tensor>& k_new,
                                      const c10::optional<Tensor>& v_new, int64_t window_left, int64_t window_right,
                                      double softmax_scale, double softcap, const c10::optional<Tensor>& slopes,
                                      const c10::optional<Tensor>& sinks, const c10::optional<Tensor>& k_descale,
                                      const c10::optional<Tensor>& v_descale) {
  const bool packed = g.cu != nullptr;
  const int qdim = packed ? 3 : 4;
  FA_ASSERT(Q.dim() == qdim && Kp.dim() == 4 && Vp.dim() == 4,
            packed ? "q must be [total_q, H, D], the pools [num_pages, H_kv, page_size, D]"
                   : "q must be [B, H, S_q, D], the pools [num_pages, H_kv, page_size, D]");
  const bool fp8 = Kp.scalar_type() == at::kFloat8_e4m3fn;
  FA_ASSERT(Kp.sizes() == Vp.sizes() && Kp.scalar_type() == Vp.scalar_type(), "k_cache and v_cache must have the same shape and dtype");
  if (packed) FA_ASSERT(Q.size(0) >= 1, "q must have at least one row");
  const int64_t Dq = Q.size(qdim - 1);
  FA_ASSERT(Kp.size(3) == Dq, "the pools must have q's head dim");
  FA_ASSERT(Kp.size(1) >= 1 && Q.size(1) % Kp.size(1) == 0, "q's head count must be a multiple of the pools' (H % H_kv == 0)");
  FA_ASSERT(Kp.size(2) >= 32 && Kp.size(2) % 32 == 0, "the page size (k_cache.shape[2]) must be a positive multiple of 32");
  FA_ASSERT(k_new.has_value() == v_new.has_value(), "k_new and v_new must be given together");
  FA_ASSERT(window_left >= -1 && window_right >= -1 && window_left <= INT32_MAX && window_right <= INT32_MAX,
            "window_left / window_right must be >= -1 (-1 = unbounded) and fit in int32");
  FA_ASSERT(Q.is_cuda() && Kp.is_cuda() && Vp.is_cuda() && (!packed || g.cu->is_cuda()) && seqlens.is_cuda() && table.is_cuda(),
            packed ? "q, the pools, cu_seqlens_q, cache_seqlens and block_table must be device tensors"
                   : "q, the pools, cache_seqlens and block_table must be device tensors");
  FA_ASSERT(Kp.device() == Q.device() && Vp.device() == Q.device() && (!packed || g.cu->device() == Q.device()) &&
                seqlens.device() == Q.device() && table.device() == Q.device(),
            "all tensors must be on q's device");
  FA_ASSERT(Q.scalar_type() == at::kHalf || Q.scalar_type() == at::kBFloat16, "q's dtype must be float16 or bfloat16");
  FA_ASSERT(fp8 || Kp.scalar_type() == Q.scalar_type(), "the pools must have q's dtype or be torch.float8_e4m3fn");
  FA_ASSERT(Dq == 64 || Dq == 128 || Dq == 256, "head dim must be 64 or 128");   // (the decode kernels also exist at D = 256)
  if (packed) check_cu_seqlens(*g.cu);
  const int64_t B = packed ? g.cu->numel() - 1 : Q.size(0), Tq = packed ? Q.size(0) : 0, Hq = Q.size(1), Hk = Kp.size(1);
  FA_ASSERT(seqlens.scalar_type() == at::kInt && seqlens.dim() == 1 && seqlens.numel() == B && seqlens.is_contiguous(),
            packed ? "cache_seqlens must be a contiguous int32 vector of B entries (cu_seqlens_q has B + 1)"
                   : "cache_seqlens must be a contiguous int32 vector of B entries");
  check_block_table(table, B);
  FA_ASSERT(!Q.requires_grad() && !Kp.requires_grad() && !Vp.requires_grad(),
            std::string(packed ? "flash_attention_kvcache_ragged" : "flash_attention_kvcache_paged") +
                " has no backward: q, k_cache and v_cache must not require grad");
  check_vec(slopes, "alibi_slopes", B, Hq, Q.device());
  check_vec(sinks, "sinks", 0, Hq, Q.device());
  check_vec(k_descale, "k_descale", B, Hk, Q.device());
  check_vec(v_descale, "v_descale", B, Hk, Q.device());
  const int64_t esz = fp8 ? 1 : 2;
  FA_ASSERT(pool_ok(Kp, esz) && pool_ok(Vp, esz) && (Kp.size(2) == 1 || Kp.stride(2) == Vp.stride(2)),
            "the pools must be addressable in place: 16-byte aligned rows with unit head-dim stride, strides that are multiples "
            "of 16 bytes, one row stride for K and V");
  // one batch stride serves both descale vectors: a (H_kv,) vector beside a (B, H_kv) one is expanded
  Tensor Kd, Vd;
  long long dstride = 0;
  if (k_descale.has_value()) Kd = *k_descale;
  if (v_descale.has_value()) Vd = *v_descale;
  if ((Kd.defined() && Kd.dim() == 2) || (Vd.defined() && Vd.dim() == 2)) {
    dstride = Hk;
    if (Kd.defined() && Kd.dim() == 1) Kd = Kd.expand({B, Hk}).contiguous();
    if (Vd.defined() && Vd.dim() == 1) Vd = Vd.expand({B, Hk}).contiguous();
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
  const int H = (int)Hq, Hkv = (int)Hk, D = (int)Dq, page = (int)Kp.size(2);
  if (packed)
    FA_ASSERT(Kp.size(0) <= INT32_MAX && table.size(1) <= INT32_MAX && Tq <= INT32_MAX && B <= INT32_MAX,
              "too many pages, rows or sequences");
  else
    FA_ASSERT(Kp.size(0) <= INT32_MAX && table.size(1) <= INT32_MAX, "too many pages");
  const int num_pages = (int)Kp.size(0), max_pages = (int)table.size(1);
  const float scale = softmax_scale > 0.0 ? (float)softmax_scale : (float)(1.0 / std::sqrt((double)D));
  const int cache_dtype = fp8 ? MI355FA_PAGED_CACHE_FP8_E4M3 : MI355FA_PAGED_CACHE_16BIT;
  c10::OptionalDeviceGuard guard(Q.device());
  Tensor O = packed ? packed_result(*g.out, Q) : torch::empty(Q.sizes(), Q.options().memory_format(at::MemoryFormat::Contiguous));
  Tensor LSE = packed ? torch::empty({Hq, Tq}, Q.options().dtype(at::kFloat))
                      : torch::empty({B, Hq, Q.size(2)}, Q.options().dtype(at::kFloat));
  const int Sq = packed ? 0 : (int)Q.size(2);
  const long long ws_bytes =
      packed ? fa_fwd_kvcache_ragged_workspace_bytes((int)Tq, (int)B, H, Hkv, max_pages, page, D, cache_dtype)
             : fa_fwd_kvcache_paged_workspace_bytes((int)B, H, Hkv, Sq, max_pages, page, S_new, D, cache_dtype);
  check_rc(ws_bytes, packed ? "fa_fwd_kvcache_ragged_workspace_bytes" : "fa_fwd_kvcache_paged_workspace_bytes");
  Tensor ws = torch::empty({std::max<long long>(ws_bytes, 1)}, Q.options().dtype(at::kByte));
  long long qs[3], os[3], ks[3], vs[3];
  strides3(Kp, ks);
  strides3(Vp, vs);
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
  mi355fa_paged_mods mods{};
  mods.softcap = softcap > 0.0 ? (float)softcap : 0.f;
  mods.alibi_slopes = fptr(slopes);
  mods.slopes_batch_stride = slopes.has_value() && slopes->dim() == 2 ? (long long)slopes->size(1) : 0;
  mods.sinks = fptr(sinks);
  mods.k_descale = Kd.defined() ? (const float*)Kd.data_ptr() : nullptr;
  mods.v_descale = Vd.defined() ? (const float*)Vd.data_ptr() : nullptr;
  mods.descale_bstride = dstride;
  void* stream = (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(Q.device().index()).stream();
  const void *kn = Kn.defined() ? Kn.data_ptr() : nullptr, *vn = Vn.defined() ? Vn.data_ptr() : nullptr;
  const long long table_stride = B > 1 ? (long long)table.stride(0) : (long long)max_pages;
  const int dtype = Q.scalar_type() == at::kBFloat16 ? MI355FA_BF16 : MI355FA_FP16;
  if (packed)
    check_rc(fa_fwd_kvcache_ragged(Qp.data_ptr(), Kp.data_ptr(), Vp.data_ptr(), kn, vn, (const int*)g.cu->data_ptr(),
                                   (const int*)seqlens.data_ptr(), (const int*)table.data_ptr(), O.data_ptr(),
                                   (float*)LSE.data_ptr(), ws.data_ptr(), ws_bytes, (int)Tq, (int)B, H, Hkv, num_pages, page,
                                   max_pages, table_stride, D, dtype, cache_dtype, scale, (int)window_left, (int)window_right,
                                   &mods, &opts, stream),
             "fa_fwd_kvcache_ragged");
  else
    check_rc(fa_fwd_kvcache_paged(Qp.data_ptr(), Kp.data_ptr(), Vp.data_ptr(), kn, vn, (const int*)seqlens.data_ptr(),
                                  (const int*)table.data_ptr(), O.data_ptr(), (float*)LSE.data_ptr(), ws.data_ptr(), ws_bytes,
                                  (int)B, H, Hkv, Sq, num_pages, page, max_pages, table_stride, S_new, D, dtype, cache_dtype,
                                  scale, (int)window_left, (int)window_right, &mods, &opts, stream),
             "fa_fwd_kvcache_paged");
  return {O, LSE};
}

std::tuple<Tensor, Tensor> kvcache_paged_forward(const Tensor& Q, const Tensor& Kp, const Tensor& Vp, const Tensor& seqlens,
                                                 const Tensor& table, const c10::optional<Tensor>& k_new,
                                                 const c10::optional<Tensor>& v_new, int64_t window_left,
                                                 int64_t window_right, double softmax_scale, double softcap,
                                                 const c10::optional<Tensor>& slopes, const c10::optional<Tensor>& sinks,
                                                 const c10::optional<Tensor>& k_descale,
                                                 const c10::optional<Tensor>& v_descale) {
  return paged_impl(Queries{}, Q, Kp, Vp, seqlens, table, k_new, v_new, window_left, window_right, softmax_scale, softcap,
                    slopes, sinks, k_descale, v_descale);
}

std::tuple<Tensor, Tensor> kvcache_ragged_forward(const Tensor& Q, const Tensor& Kp, const Tensor& Vp, const Tensor& cu,
                                                  const Tensor& seqlens, const Tensor& table,
                                                  const c10::optional<Tensor>& k_new, const c10::optional<Tensor>& v_new,
                                                  int64_t window_left, int64_t window_right, double softmax_scale,
                                                  double softcap, const c10::optional<Tensor>& slopes,
                                                  const c10::optional<Tensor>& sinks, const c10::optional<Tensor>& k_descale,
                                                  const c10::optional<Tensor>& v_descale, const c10::optional<Tensor>& out) {
  return paged_impl(Queries{&cu, &out}, Q, Kp, Vp, seqlens, table, k_new, v_new, window_left, window_right, softmax_scale,
                    softcap, slopes, sinks, k_descale, v_descale);
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "PyTorch-ROCm binding of fa_fwd_kvcache_paged and fa_fwd_kvcache_ragged (libmi355fa.so): decoding attention over a "
            "paged KV cache, also with packed variable-length queries";
  m.def("kvcache_paged_forward", &kvcache_paged_forward, pybind11::arg("q"), pybind11::arg("k_cache"), pybind11::arg("v_cache"),
        pybind11::arg("cache_seqlens"), pybind11::arg("block_table"), pybind11::arg("k_new"), pybind11::arg("v_new"),
        pybind11::arg("window_left"), pybind11::arg("window_right"), pybind11::arg("softmax_scale"), pybind11::arg("softcap"),
        pybind11::arg("alibi_slopes"), pybind11::arg("sinks"), pybind11::arg("k_descale"), pybind11::arg("v_descale"),
        "O, LSE = attention of q over the pages block_table names, after appending k_new / v_new (None: no append)");
  m.def("kvcache_ragged_forward", &kvcache_ragged_forward, pybind11::arg("q"), pybind11::arg("k_cache"), pybind11::arg("v_cache"),
        pybind11::arg("cu_seqlens_q"), pybind11::arg("cache_seqlens"), pybind11::arg("block_table"), pybind11::arg("k_new"),
        pybind11::arg("v_new"), pybind11::arg("window_left"), pybind11::arg("window_right"), pybind11::arg("softmax_scale"),
        pybind11::arg("softcap"), pybind11::arg("alibi_slopes"), pybind11::arg("sinks"), pybind11::arg("k_descale"),
        pybind11::arg("v_descale"), pybind11::arg("out"),
        "O, LSE = attention of the packed q over the pages block_table names, after appending k_new / v_new (None: no append)");
}
